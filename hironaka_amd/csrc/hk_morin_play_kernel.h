// hk_search_morin_play: the Morin game (hironaka/game.py:122-154 GameMorin with hironaka/agent.py:114-136 AgentMorin)
// played forward over a batch of games, one game per lane.
//
// A workgroup is one wave that owns `games_per_block` consecutive games: as many as have slices in kSearchLdsBytes, at
// most a wave.  Their rows are staged with the coalesced slab copy of hk_host_select_kernel.h into slices of the odd
// stride search_lds_stride counts, and lane g plays game g alone in its slice with the per-game routines of hk_hosts.h
// and hk_search_wave.h; the final states leave the same way.  A slice is hk_search_morin_kernel.h's: parent, child, the
// shift coefficients, sort_compact's row scratch, then the lane's d weights and the saved row p (morin_lds_extra):
// indexed at run time, they would land in scratch as register arrays.  Every move is expand_morin_child, whose parent
// and child halves swap roles from move to move.  HBM traffic: one read and one write of the state, the weights and the
// index, and 8 B per move played when the moves are recorded.  No communication between workgroups; every loop is
// bounded by max_steps.
#pragma once

#include "hk_generic_kernel.h"
#include "hk_search_morin_kernel.h"

namespace hk {

constexpr int kMorinPlayBatch = 16;        // loads per lane in flight while staging (hk_host_select_kernel.h)
constexpr uint32_t kStreamMorinTie = 2u;  // RNG stream id of the agent's random tie-break (next to kStreamPolicy / _Generate)

struct MorinPlayArgs {
  const void* points;  // [batch] records of in_stride elements; the game is the first m*d
  void* points_out;    // [batch] records of out_stride elements
  const int32_t* weights;
  int32_t* weights_out;
  const int32_t* dist;
  int32_t* dist_out;
  const int32_t* class_in;  // [batch, max_steps] or NULL
  const int32_t* axis_in;   // [batch, max_steps] or NULL
  int32_t* class_out;       // [batch, max_steps] or NULL
  int32_t* axis_out;        // [batch, max_steps] or NULL
  int32_t* length_out;
  int32_t* outcome_out;
  int64_t in_stride, out_stride;
  uint64_t seed, game_offset;
  uint32_t step_offset;
  int batch, m, d, max_steps, tie, weight_rule, reduce_root, lds_stride, games_per_block;
};

// the position of the row `prow` among the first np rows of p, -1 when it is not there
template <typename T>
__device__ inline int find_row(const T* p, const T* prow, int np, int d) {
  int at = -1;
  for (int i = 0; i < np; ++i) {
    bool same = true;
    for (int k = 0; k < d; ++k) same &= p[i * d + k] == prow[k];
    if (same) at = i;
  }
  return at;
}

// the k-th set bit of sub (k < popcount)
__device__ inline int nth_bit(uint32_t sub, int k) {
  for (int j = 0; j < k; ++j) sub &= sub - 1u;
  return __ffs((int)sub) - 1;
}

// HOST: a fixed host's code, or HK_MORIN_HOST_FORCED for a launch whose every class is forced
template <typename T, int HOST>
__global__ void __launch_bounds__(kWave) morin_play_kernel(MorinPlayArgs a) {
  extern __shared__ unsigned char hk_mp_lds[];
  T* lds = reinterpret_cast<T*>(hk_mp_lds);
  const int lane = threadIdx.x;
  const int m = a.m, d = a.d, n = m * d, steps = a.max_steps;
  const int64_t g0 = (int64_t)blockIdx.x * a.games_per_block;
  const int64_t left = (int64_t)a.batch - g0;
  const int ngames = left < a.games_per_block ? (int)left : a.games_per_block;
  copy_slab<T, true, kMorinPlayBatch>(lds, const_cast<T*>(static_cast<const T*>(a.points)), a.in_stride, n,
                                      a.lds_stride, g0, ngames, lane);
  __syncthreads();
  if (lane < ngames) {
    const int64_t g = g0 + lane;
    const unsigned flags = HK_SEM_LIST | HK_FLAG_COMPACT_SORTED;
    const LaneSlice<T> home(lds, lane, a.lds_stride, m, d);
    LaneSlice<T> s = home;  // s.par: the current state; par and chd swap after every move
    int32_t* w = reinterpret_cast<int32_t*>(home.row + d);  // d int32 in the space of d elements
    T* prow = home.row + 2 * d;
    for (int k = 0; k < d; ++k) w[k] = a.weights[g * d + k];
    int dist = a.dist[g];
    if (!(dist >= 0 && dist < m && s.par[(dist >= 0 && dist < m ? dist : 0) * d] >= (T)0)) dist = -1;
    bool track = true;
    if (a.reduce_root) {
      // Game.__init__'s get_newton_polytope with the row marked (core/list_points.py:86-116)
      track = dist >= 0;
      bool lost = false;
      if (track) {
        for (int k = 0; k < d; ++k) prow[k] = s.par[dist * d + k];
        for (int q = 0; q < m; ++q) {
          if (q == dist || !(s.par[q * d] >= (T)0)) continue;
          bool below = true;
          for (int k = 0; k < d; ++k) below &= s.par[q * d + k] <= prow[k];
          lost |= below;
        }
      }
      newton_game(s.par, m, d, (T)-1, flags);
      sort_compact_game(s.par, m, d, (T)-1, s.row);
      if (track) dist = lost ? -1 : find_row(s.par, prow, num_points(s.par, m, d), d);
    }
    int np = num_points(s.par, m, d);
    int outcome = track && dist < 0 ? HK_MORIN_NO_CONTRIBUTION : (np < 2 ? HK_MORIN_ENDED : HK_MORIN_RUNNING);
    const int ncls = (1 << d) - d - 1;
    int len = 0;
    for (int t = 0; t < steps && outcome == HK_MORIN_RUNNING; ++t) {
      int cls = a.class_in ? a.class_in[g * steps + t] : -1;
      if (cls < 0 && HOST != HK_MORIN_HOST_FORCED)
        cls = d < kMorinMaxDim ? host_class_game<T, HOST, uint64_t>(s.par, m, d)
                               : host_class_game<T, HOST, Bits128>(s.par, m, d);
      if (cls < 0 || cls >= ncls) {
        outcome = HK_MORIN_NO_MOVE;
        break;
      }
      const uint32_t sub = decode_class(cls, d);
      int ax = a.axis_in ? a.axis_in[g * steps + t] : -1;
      if (ax >= 0) {
        if (ax >= d || !((sub >> ax) & 1u)) {
          outcome = HK_MORIN_NO_MOVE;
          break;
        }
      } else {
        // agent.py:118-127 on the two lowest coordinates of the subset
        const int c0 = __ffs((int)sub) - 1, c1 = __ffs((int)(sub & (sub - 1u))) - 1;
        const int w0 = w[c0], w1 = w[c1];
        if (w0 != w1) {
          ax = w0 < w1 ? c0 : c1;
        } else if (a.tie == HK_MORIN_TIE_LOWEST) {
          ax = c0;
        } else if (a.tie == HK_MORIN_TIE_HIGHEST) {
          ax = 31 - __clz((int)sub);
        } else {
          const uint64_t gg = a.game_offset + (uint64_t)g;
          const U4 r = philox4x32((uint32_t)gg, (uint32_t)(gg >> 32), a.step_offset + (uint32_t)t, kStreamMorinTie, a.seed);
          ax = nth_bit(sub, (int)mulhi32(r.x, (uint32_t)__popc(sub)));
        }
      }
      const uint32_t wa = (uint32_t)w[ax];
      for (int i = 0; i < d; ++i) {
        if (!((sub >> i) & 1u) || i == ax) continue;
        w[i] = a.weight_rule == HK_MORIN_WEIGHTS_AGENT ? 0 : (int32_t)((uint32_t)w[i] - wa);
      }
      for (int j = 0; j < d; ++j) s.c[j] = ((sub >> j) & 1u) ? (T)1 : (T)0;
      bool inexact = false;
      int nd;
      np = expand_morin_child(s, prow, m, d, ax, track ? dist : 0, inexact, nd);
      T* const old = s.par;
      s.par = s.chd;
      s.chd = old;
      if (a.class_out) a.class_out[g * steps + t] = cls;
      if (a.axis_out) a.axis_out[g * steps + t] = ax;
      ++len;
      if (track) dist = nd;
      if (track && nd < 0) outcome = HK_MORIN_NO_CONTRIBUTION;
      else if (np < 2) outcome = HK_MORIN_ENDED;
      if (inexact) outcome = HK_MORIN_INEXACT;
    }
    for (int t = len; t < steps; ++t) {
      if (a.class_out) a.class_out[g * steps + t] = -1;
      if (a.axis_out) a.axis_out[g * steps + t] = -1;
    }
    if (s.par != home.par)
      for (int e = 0; e < n; ++e) home.par[e] = s.par[e];
    for (int k = 0; k < d; ++k) a.weights_out[g * d + k] = w[k];
    a.dist_out[g] = dist;
    a.length_out[g] = len;
    a.outcome_out[g] = outcome;
  }
  __syncthreads();
  copy_slab<T, false, kMorinPlayBatch>(lds, static_cast<T*>(a.points_out), a.out_stride, n, a.lds_stride, g0, ngames,
                                       lane);
}

}  // namespace hk
