// hk_dqn_host_move / hk_dqn_agent_move: one greedy move of the DQN trainers' evaluation (FusedGame.host_move and
// agent_move with exploration off; include/hironaka_hip_dqn_move.h states the rules) as the two launches around the two
// network launches.
//
// dqn_host_move_kernel: a thread per game walks its row of Q-values (dqn_first_argmax), writes the class and the
// subset's 0/1 vector, and counts the class in a histogram of the workgroup's LDS; the workgroup then adds its non-zero
// bins to the caller's counts.  Integer atomics throughout, so the counts do not depend on the order.
//
// dqn_agent_move_kernel: the frame is hk_lane_games.h's with search_lds_stride's slices, used as
//   par  the game, moved in place      chd  the features of the moved game      c  the subset      row  the sort's scratch
// Lane g picks game g's axis from its d Q-values, makes the move with the per-game routines of hk_game_generic.h under
// HK_SEM_TORCH (dqn_agent_lane) and sorts a copy by coordinate 0; the wave copies both records out.  HBM traffic: one
// read and one write of the state, one write of the features, d Q-values and 13 B per game.  No communication between
// workgroups; every loop is bounded by m, d, m * d or the class count.
#pragma once

#include <limits>

#include "hk_lane_games.h"

namespace hk {

constexpr int kDqnMoveMaxDim = kLaneGameMaxDim;
constexpr int kDqnMoveMaxClasses = (1 << kDqnMoveMaxDim) - kDqnMoveMaxDim - 1;
constexpr int kDqnHostBlock = 256;
constexpr unsigned kDqnMoveFlags = HK_SEM_TORCH | HK_FLAG_AXIS_NOOP_IF_INVALID | HK_FLAG_IGNORE_ENDED;

// torch.argmax of v[0 .. n): the first index of the maximum; a NaN beats every number and the first NaN wins
template <typename Q>
__device__ inline int dqn_first_argmax(const Q* v, int n) {
  Q best = v[0];
  int at = 0;
  for (int j = 1; j < n; ++j) {
    const Q x = v[j];
    if (best != best) break;
    if (x != x || x > best) {
      best = x;
      at = j;
    }
  }
  return at;
}

// a class id as hk_step's load_coords clamps it
__device__ inline int dqn_clamp_class(int cls, int d) {
  const int ncls = (1 << d) - d - 1;
  return cls < 0 ? 0 : (cls >= ncls ? ncls - 1 : cls);
}

// The agent's axis: the argmax of q * mask + (1 - mask) * lowest (fused_game.py's expression, each operation rounded on
// its own: the library is built with -ffp-contract=off) when masked, else of q itself.  The argmax is
// dqn_first_argmax's, taken as the values come: no array that a run-time index would send to scratch.
template <typename Q>
__device__ inline int dqn_agent_axis(const Q* q, uint32_t sub, int d, bool masked) {
  const Q lowest = std::numeric_limits<Q>::lowest();
  Q best = (Q)0;
  int at = 0;
  for (int k = 0; k < d; ++k) {
    const Q mk = ((sub >> k) & 1u) ? (Q)1 : (Q)0;
    const Q kept = q[k] * mk;
    const Q rest = ((Q)1 - mk) * lowest;
    const Q x = masked ? kept + rest : q[k];
    if (k == 0 || (best == best && (x != x || x > best))) {
      best = x;
      at = k;
    }
  }
  return at;
}

struct DqnMoveOutcome {
  int axis;
  bool prev_done, done;
};

// One game: s.par holds the state on entry and the moved state on return, s.chd receives its rows by coordinate 0
// (descending, stable); s.c and s.row are scratch.  q: the game's d Q-values.
template <typename T, typename Q>
__device__ inline DqnMoveOutcome dqn_agent_lane(const LaneSlice<T>& s, const Q* q, int m, int d, int cls, bool masked,
                                                bool rescale, T pad) {
  DqnMoveOutcome o;
  o.prev_done = num_points(s.par, m, d) < 2;
  const uint32_t sub = decode_class(dqn_clamp_class(cls, d), d);
  o.axis = dqn_agent_axis(q, sub, d, masked);
  subset_coeffs(s.c, sub, d);
  stages_game(s.par, m, d, s.c, o.axis, pad, HK_STAGE_SHIFT | HK_STAGE_NEWTON | (rescale ? HK_STAGE_RESCALE : 0u),
              kDqnMoveFlags);
  o.done = num_points(s.par, m, d) < 2;
  for (int e = 0; e < m * d; ++e) s.chd[e] = s.par[e];
  feature_sort_game(s.chd, m, d, s.row, true);
  return o;
}

struct DqnHostMoveArgs {
  const void* q;
  int64_t q_stride;
  int32_t* class_out;
  void* coords_out;
  const uint8_t* prev_done;
  int32_t* counts;
  int batch, d, classes;
};

template <typename Q, typename T>
__global__ void __launch_bounds__(kDqnHostBlock) dqn_host_move_kernel(DqnHostMoveArgs a) {
  __shared__ int hist[kDqnMoveMaxClasses];
  const bool count = a.prev_done && a.counts;
  if (count) {
    for (int j = threadIdx.x; j < a.classes; j += kDqnHostBlock) hist[j] = 0;
    __syncthreads();
  }
  const int64_t b = (int64_t)blockIdx.x * kDqnHostBlock + threadIdx.x;
  if (b < a.batch) {
    const int cls = dqn_first_argmax(static_cast<const Q*>(a.q) + b * a.q_stride, a.classes);
    const uint32_t sub = decode_class(cls, a.d);
    a.class_out[b] = cls;
    T* out = static_cast<T*>(a.coords_out) + b * a.d;
    for (int j = 0; j < a.d; ++j) out[j] = ((sub >> j) & 1u) ? (T)1 : (T)0;
    if (count && !a.prev_done[b]) atomicAdd(&hist[cls], 1);
  }
  if (count) {
    __syncthreads();
    for (int j = threadIdx.x; j < a.classes; j += kDqnHostBlock)
      if (hist[j]) atomicAdd(a.counts + j, hist[j]);
  }
}

struct DqnAgentMoveArgs {
  void* points;
  const void* q;
  int64_t q_stride;
  const int32_t* class_id;
  int32_t* axis_out;
  void* features_out;
  uint8_t* done_out;
  int32_t* lengths;
  int32_t* counts;
  double pad;
  int batch, m, d, masked, rescale, lds_stride, games_per_block;
};

template <typename T, typename Q>
__global__ void __launch_bounds__(kWave) dqn_agent_move_kernel(DqnAgentMoveArgs a) {
  extern __shared__ unsigned char hk_dqn_move_lds[];
  T* lds = reinterpret_cast<T*>(hk_dqn_move_lds);
  const int lane = threadIdx.x;
  const int m = a.m, d = a.d, n = m * d;
  const LaneBlock blk = lane_block(a.batch, a.games_per_block);
  stage_games(lds, a.points, (int64_t)n, n, a.lds_stride, blk, lane);
  __syncthreads();
  const bool active = lane < blk.ngames;
  const int64_t g = blk.g0 + lane;
  DqnMoveOutcome o{-1, true, true};
  if (active) {
    const LaneSlice<T> s(lds, lane, a.lds_stride, m, d);
    o = dqn_agent_lane<T, Q>(s, static_cast<const Q*>(a.q) + g * a.q_stride, m, d, a.class_id[g], a.masked != 0,
                             a.rescale != 0, (T)a.pad);
    a.axis_out[g] = o.axis;
    a.done_out[g] = o.done ? 1 : 0;
    if (!o.prev_done) a.lengths[g] += 1;
  }
  if (a.counts) {
    for (int k = 0; k < d; ++k) {
      const unsigned long long moved = __ballot(active && !o.prev_done && o.axis == k);
      if (lane == 0 && moved) atomicAdd(a.counts + k, (int)__popcll(moved));
    }
  }
  __syncthreads();
  unstage_games(lds, a.points, (int64_t)n, n, a.lds_stride, blk, lane);
  unstage_games(lds + n, a.features_out, (int64_t)n, n, a.lds_stride, blk, lane);
}

// ---- the choice of instantiation: f(A(), B()) for the element types of the two dtypes -------------------------------
template <typename F>
int with_dqn_move_types(int dtype_a, int dtype_b, F&& f) {
  if (dtype_a == HK_F32) return dtype_b == HK_F32 ? f(float(), float()) : f(float(), double());
  return dtype_b == HK_F32 ? f(double(), float()) : f(double(), double());
}

}  // namespace hk
