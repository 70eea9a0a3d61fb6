// hk_search_morin_play: the Morin game (hironaka/game.py:122-154 GameMorin with hironaka/agent.py:114-136 AgentMorin)
// played forward over a batch of games, one game per lane.
//
// The frame is hk_lane_games.h's.  A slice is search_lds_stride's with morin_lds_extra behind the row scratch: the
// lane's d weights and the saved row p.  Every move is expand_morin_child.  HBM traffic: one read and one write of the
// state, the weights and the index, and 8 B per move played when the moves are recorded.  Every loop is bounded by
// max_steps.
#pragma once

#include "hk_lane_games.h"

namespace hk {

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

// HOST: a fixed host's code, or HK_MORIN_HOST_FORCED for a launch whose every class is forced
template <typename T, int HOST>
__global__ void __launch_bounds__(kWave) morin_play_kernel(MorinPlayArgs a) {
  extern __shared__ unsigned char hk_mp_lds[];
  T* lds = reinterpret_cast<T*>(hk_mp_lds);
  const int lane = threadIdx.x;
  const int m = a.m, d = a.d, n = m * d, steps = a.max_steps;
  const LaneBlock blk = lane_block(a.batch, a.games_per_block);
  stage_games(lds, a.points, a.in_stride, n, a.lds_stride, blk, lane);
  __syncthreads();
  if (lane < blk.ngames) {
    const int64_t g = blk.g0 + lane;
    const MoveRecords rec{a.class_in, a.axis_in, a.class_out, a.axis_out, steps};
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
        lost = row_contained(s.par, m, d, dist, prow);
      }
      newton_game(s.par, m, d, (T)-1, kListFlags);
      sort_compact_game(s.par, m, d, (T)-1, s.row);
      if (track) dist = lost ? -1 : find_row(s.par, prow, num_points(s.par, m, d), d);
    }
    int np = num_points(s.par, m, d);
    int outcome = track && dist < 0 ? HK_MORIN_NO_CONTRIBUTION : (np < 2 ? HK_MORIN_ENDED : HK_MORIN_RUNNING);
    int len = 0;
    for (int t = 0; t < steps && outcome == HK_MORIN_RUNNING; ++t) {
      int cls, ax;
      uint32_t sub;
      if (!forced_or_host_move<T, HOST>(rec, g, t, s.par, m, d, cls, sub, ax)) {
        outcome = HK_MORIN_NO_MOVE;
        break;
      }
      if (ax < 0) {
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
          ax = random_legal_axis(sub, a.game_offset + (uint64_t)g, a.step_offset + (uint32_t)t, kStreamMorinTie, a.seed);
        }
      }
      const uint32_t wa = (uint32_t)w[ax];
      for (int i = 0; i < d; ++i) {
        if (!((sub >> i) & 1u) || i == ax) continue;
        w[i] = a.weight_rule == HK_MORIN_WEIGHTS_AGENT ? 0 : (int32_t)((uint32_t)w[i] - wa);
      }
      subset_coeffs(s.c, sub, d);
      bool inexact = false;
      int nd;
      np = expand_morin_child(s, prow, m, d, ax, track ? dist : 0, inexact, nd);
      T* const old = s.par;
      s.par = s.chd;
      s.chd = old;
      record_move(rec, g, t, cls, ax);
      ++len;
      if (track) dist = nd;
      if (track && nd < 0) outcome = HK_MORIN_NO_CONTRIBUTION;
      else if (np < 2) outcome = HK_MORIN_ENDED;
      if (inexact) outcome = HK_MORIN_INEXACT;
    }
    finish_game(rec, g, len, home, s, n);
    for (int k = 0; k < d; ++k) a.weights_out[g * d + k] = w[k];
    a.dist_out[g] = dist;
    a.length_out[g] = len;
    a.outcome_out[g] = outcome;
  }
  __syncthreads();
  unstage_games(lds, a.points_out, a.out_stride, n, a.lds_stride, blk, lane);
}

}  // namespace hk
