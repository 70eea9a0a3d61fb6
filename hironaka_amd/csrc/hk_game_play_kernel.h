// hk_game_play: the plain Hironaka game (hironaka/game.py:84-119 GameHironaka with hironaka/agent.py:85-98 RandomAgent
// / ChooseFirstAgent, and what hironaka/validator/hironaka_validator.py:30-48 playoff loops over) played forward over a
// batch of games, one game per lane.
//
// The frame is hk_morin_play_kernel.h's: a workgroup is one wave that owns `games_per_block` consecutive games, as many
// as have slices in kSearchLdsBytes, at most a wave.  Their rows are staged with the coalesced slab copy into slices of
// the odd stride search_lds_stride counts, lane g plays game g alone in its slice with the per-game routines of
// hk_game_generic.h, hk_hosts.h and hk_search_wave.h, and the final states leave the same way.  A move without
// reposition or rescale is expand_child; with them it is the same sequence with reposition_game between shift and
// Newton and rescale_game behind sort-compact.  The parent and child halves of a slice swap roles from move to move.
// HBM traffic: one read and one write of the state, and 8 B per move played when the moves are recorded.  No
// communication between workgroups; every loop is bounded by max_steps.
#pragma once

#include "hk_generic_kernel.h"
#include "hk_morin_play_kernel.h"

namespace hk {

constexpr int kGamePlayBatch = 16;         // loads per lane in flight while staging (hk_host_select_kernel.h)
constexpr uint32_t kStreamPlayAgent = 3u;  // RNG stream id of the random-legal agent (next to kStreamMorinTie)
constexpr int kGamePlayMaxDim = 7;

struct GamePlayArgs {
  const void* points;  // [batch] records of in_stride elements; the game is the first m*d
  void* points_out;    // [batch] records of out_stride elements
  const int32_t* class_in;  // [batch, max_steps] or NULL
  const int32_t* axis_in;   // [batch, max_steps] or NULL
  int32_t* class_out;       // [batch, max_steps] or NULL
  int32_t* axis_out;        // [batch, max_steps] or NULL
  int32_t* length_out;
  int32_t* outcome_out;
  int64_t in_stride, out_stride;
  uint64_t seed, game_offset;
  double value_threshold;  // <= 0: none
  uint32_t step_offset;
  int batch, m, d, max_steps, agent, reposition, rescale, reduce_root, rescale_root, lds_stride, games_per_block;
};

// whether a coordinate of a point of p exceeds thr (ListPoints.exceed_threshold, core/list_points.py:60-70)
template <typename T>
__device__ inline bool exceeds_game(const T* p, int m, int d, double thr) {
  bool over = false;
  for (int i = 0; i < m; ++i) {
    if (!(p[i * d] >= (T)0)) continue;
    for (int k = 0; k < d; ++k) over |= (double)p[i * d + k] > thr;
  }
  return over;
}

// One game, played by one lane in its slice `home` of the LDS, whose parent half holds the game on entry and the final
// state on return.  HOST: a fixed host's code, or HK_PLAY_HOST_FORCED for a launch whose every class is forced.
template <typename T, int HOST>
__device__ inline void play_lane(const GamePlayArgs& a, const LaneSlice<T>& home, int64_t g) {
  const int m = a.m, d = a.d, n = m * d, steps = a.max_steps;
  const unsigned flags = HK_SEM_LIST | HK_FLAG_COMPACT_SORTED;
  LaneSlice<T> s = home;  // s.par: the current state; par and chd swap after every move
  if (a.reduce_root) {    // Game.__init__'s get_newton_polytope (game.py:46-50)
    newton_game(s.par, m, d, (T)-1, flags);
    sort_compact_game(s.par, m, d, (T)-1, s.row);
  }
  if (a.rescale_root) rescale_game(s.par, m, d, (T)-1, flags);
  int np = num_points(s.par, m, d);
  int outcome = np < 2 ? HK_PLAY_ENDED : HK_PLAY_RUNNING;
  const int ncls = (1 << d) - d - 1;
  int len = 0;
  for (int t = 0; t < steps && outcome == HK_PLAY_RUNNING; ++t) {
    int cls = a.class_in ? a.class_in[g * steps + t] : -1;
    if (cls < 0 && HOST != HK_PLAY_HOST_FORCED)
      cls = d < kGamePlayMaxDim ? host_class_game<T, HOST, uint64_t>(s.par, m, d)
                                : host_class_game<T, HOST, Bits128>(s.par, m, d);
    if (cls < 0 || cls >= ncls) {
      outcome = HK_PLAY_NO_MOVE;
      break;
    }
    const uint32_t sub = decode_class(cls, d);
    int ax = a.axis_in ? a.axis_in[g * steps + t] : -1;
    if (ax >= 0) {
      if (ax >= d || !((sub >> ax) & 1u)) {
        outcome = HK_PLAY_NO_MOVE;
        break;
      }
    } else if (a.agent == HK_AGENT_CHOOSE_FIRST) {
      ax = __ffs((int)sub) - 1;
    } else if (a.agent == HK_AGENT_CHOOSE_LAST) {
      ax = 31 - __clz((int)sub);
    } else {  // agent.py:89-90, uniform over the subset
      const uint64_t gg = a.game_offset + (uint64_t)g;
      const U4 r = philox4x32((uint32_t)gg, (uint32_t)(gg >> 32), a.step_offset + (uint32_t)t, kStreamPlayAgent, a.seed);
      ax = nth_bit(sub, (int)mulhi32(r.x, (uint32_t)__popc(sub)));
    }
    for (int j = 0; j < d; ++j) s.c[j] = ((sub >> j) & 1u) ? (T)1 : (T)0;
    bool inexact = false;
    if (!a.reposition && !a.rescale) {
      np = expand_child(s, m, d, ax, inexact);
    } else {
      const T limit = sizeof(T) == 4 ? (T)16777216.0 : (T)9007199254740992.0;
      for (int e = 0; e < n; ++e) s.chd[e] = s.par[e];
      shift_game(s.chd, m, d, s.c, ax, (T)-1, flags);
      for (int i = 0; i < m; ++i) inexact |= s.chd[i * d + ax] >= limit;
      if (a.reposition) reposition_game(s.chd, m, d, (T)-1, flags);
      newton_game(s.chd, m, d, (T)-1, flags);
      sort_compact_game(s.chd, m, d, (T)-1, s.row);
      if (a.rescale) rescale_game(s.chd, m, d, (T)-1, flags);  // game.py:107-108
      np = num_points(s.chd, m, d);
    }
    T* const old = s.par;
    s.par = s.chd;
    s.chd = old;
    if (a.class_out) a.class_out[g * steps + t] = cls;
    if (a.axis_out) a.axis_out[g * steps + t] = ax;
    ++len;
    if (np < 2) outcome = HK_PLAY_ENDED;
    else if (a.value_threshold > 0.0 && exceeds_game(s.par, m, d, a.value_threshold)) outcome = HK_PLAY_VALUE_LIMIT;
    if (inexact && !a.rescale) outcome = HK_PLAY_INEXACT;
  }
  for (int t = len; t < steps; ++t) {
    if (a.class_out) a.class_out[g * steps + t] = -1;
    if (a.axis_out) a.axis_out[g * steps + t] = -1;
  }
  if (s.par != home.par)
    for (int e = 0; e < n; ++e) home.par[e] = s.par[e];
  a.length_out[g] = len;
  a.outcome_out[g] = outcome;
}

template <typename T, int HOST>
__global__ void __launch_bounds__(kWave) game_play_kernel(GamePlayArgs a) {
  extern __shared__ unsigned char hk_gp_lds[];
  T* lds = reinterpret_cast<T*>(hk_gp_lds);
  const int lane = threadIdx.x;
  const int n = a.m * a.d;
  const int64_t g0 = (int64_t)blockIdx.x * a.games_per_block;
  const int64_t left = (int64_t)a.batch - g0;
  const int ngames = left < a.games_per_block ? (int)left : a.games_per_block;
  copy_slab<T, true, kGamePlayBatch>(lds, const_cast<T*>(static_cast<const T*>(a.points)), a.in_stride, n, a.lds_stride,
                                     g0, ngames, lane);
  __syncthreads();
  if (lane < ngames) play_lane<T, HOST>(a, LaneSlice<T>(lds, lane, a.lds_stride, a.m, a.d), g0 + lane);
  __syncthreads();
  copy_slab<T, false, kGamePlayBatch>(lds, static_cast<T*>(a.points_out), a.out_stride, n, a.lds_stride, g0, ngames,
                                      lane);
}

}  // namespace hk
