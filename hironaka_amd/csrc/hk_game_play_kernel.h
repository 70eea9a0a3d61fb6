// hk_game_play: the plain Hironaka game (hironaka/game.py:84-119 GameHironaka with hironaka/agent.py:85-98 RandomAgent
// / ChooseFirstAgent, and what hironaka/validator/hironaka_validator.py:30-48 playoff loops over) played forward over a
// batch of games, one game per lane.
//
// The frame is hk_lane_games.h's, with search_lds_stride's slices.  A move is shift the child, [reposition], reduce the
// child, [rescale].  HBM traffic: one read and one write of the state, and 8 B per move played when the moves are
// recorded.  Every loop is bounded by max_steps.
#pragma once

#include "hk_lane_games.h"

namespace hk {

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

// One game, played by one lane in its slice `home` of the LDS, whose parent half holds the game on entry and the final
// state on return.  HOST: a fixed host's code, or HK_PLAY_HOST_FORCED for a launch whose every class is forced.
template <typename T, int HOST>
__device__ inline void play_lane(const GamePlayArgs& a, const LaneSlice<T>& home, int64_t g) {
  const int m = a.m, d = a.d, n = m * d, steps = a.max_steps;
  const MoveRecords rec{a.class_in, a.axis_in, a.class_out, a.axis_out, steps};
  LaneSlice<T> s = home;  // s.par: the current state; par and chd swap after every move
  if (a.reduce_root) {    // Game.__init__'s get_newton_polytope (game.py:46-50)
    newton_game(s.par, m, d, (T)-1, kListFlags);
    sort_compact_game(s.par, m, d, (T)-1, s.row);
  }
  if (a.rescale_root) rescale_game(s.par, m, d, (T)-1, kListFlags);
  int np = num_points(s.par, m, d);
  int outcome = np < 2 ? HK_PLAY_ENDED : HK_PLAY_RUNNING;
  int len = 0;
  for (int t = 0; t < steps && outcome == HK_PLAY_RUNNING; ++t) {
    int cls, ax;
    uint32_t sub;
    if (!forced_or_host_move<T, HOST>(rec, g, t, s.par, m, d, cls, sub, ax)) {
      outcome = HK_PLAY_NO_MOVE;
      break;
    }
    if (ax < 0)
      ax = a.agent == HK_AGENT_CHOOSE_FIRST  ? __ffs((int)sub) - 1
           : a.agent == HK_AGENT_CHOOSE_LAST ? 31 - __clz((int)sub)
                                             : random_legal_axis(sub, a.game_offset + (uint64_t)g,
                                                                 a.step_offset + (uint32_t)t, kStreamPlayAgent, a.seed);
    subset_coeffs(s.c, sub, d);
    bool inexact = false;
    shift_child(s, m, d, ax);
    note_inexact(s, m, d, ax, inexact);
    if (a.reposition) reposition_game(s.chd, m, d, (T)-1, kListFlags);
    np = reduce_child(s, m, d);
    if (a.rescale) {  // game.py:107-108
      rescale_game(s.chd, m, d, (T)-1, kListFlags);
      np = num_points(s.chd, m, d);
    }
    T* const old = s.par;
    s.par = s.chd;
    s.chd = old;
    record_move(rec, g, t, cls, ax);
    ++len;
    if (np < 2) outcome = HK_PLAY_ENDED;
    else if (a.value_threshold > 0.0 && exceeds_game(s.par, m, d, a.value_threshold)) outcome = HK_PLAY_VALUE_LIMIT;
    if (inexact && !a.rescale) outcome = HK_PLAY_INEXACT;
  }
  finish_game(rec, g, len, home, s, n);
  a.length_out[g] = len;
  a.outcome_out[g] = outcome;
}

template <typename T, int HOST>
__global__ void __launch_bounds__(kWave) game_play_kernel(GamePlayArgs a) {
  extern __shared__ unsigned char hk_gp_lds[];
  T* lds = reinterpret_cast<T*>(hk_gp_lds);
  const int lane = threadIdx.x;
  const int n = a.m * a.d;
  const LaneBlock blk = lane_block(a.batch, a.games_per_block);
  stage_games(lds, a.points, a.in_stride, n, a.lds_stride, blk, lane);
  __syncthreads();
  if (lane < blk.ngames) play_lane<T, HOST>(a, LaneSlice<T>(lds, lane, a.lds_stride, a.m, a.d), blk.g0 + lane);
  __syncthreads();
  unstage_games(lds, a.points_out, a.out_stride, n, a.lds_stride, blk, lane);
}

}  // namespace hk
