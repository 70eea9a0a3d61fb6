// hk_unified_expand / hk_unified_prior: one expansion of the role-agnostic search tree (hironaka/jax/recurrent_fn.py:
// 126-199; include/hironaka_hip_unified.h states the rule).  A state is m * d points followed by a tail of d floats; a
// host state has a tail that is close to zero, an agent state carries the host's subset there.
//
// unified_kind_kernel: a thread per game reads the d tail floats of its parent and the wave ORs 1 into the caller's word
// when one of its games stands on a host state -- an atomic nobody waits for.
//
// unified_expand_kernel: the frame is hk_lane_games.h's with search_lds_stride's slices, used as
//   par  the observation features of the next points      chd ++ c  the parent state, then the next state
// so that the next state leaves as one record and the network's input as features ++ tail.  The parents of a block are
// not a slab (every game names its own node), so the wave gathers them record by record, consecutive lanes on
// consecutive elements.  Lane g then makes game g's move with the per-game routines of hk_game_generic.h (unified_lane)
// and the wave writes the records out the same way.  HBM traffic: one read of the parent state, one write of the next
// state, one of the network's input, 12 B per game.  No spinning; every loop is bounded by m, d or the block's games.
#pragma once

#include "hk_lane_games.h"

namespace hk {

constexpr int kUnifiedMaxDim = 5;  // the search takes at most 32 actions: 2^5 - 5 - 1 = 26, 2^6 - 6 - 1 = 57

struct UnifiedArgs {
  float* embeddings;  // [batch, nodes, m * d + d]
  const int32_t *parent, *action, *node;
  const int32_t* kind;
  float* net_in;
  int32_t* subset;
  float *reward, *discount_out;
  float discount;
  int batch, nodes, m, d, reposition, scale, lds_stride, games_per_block;
};

// jnp.isclose(tail, 0).all(): |x| <= 1e-8 in float on every entry; a NaN is not close
__device__ inline bool unified_host_state(const float* tail, int d) {
  bool host = true;
  for (int j = 0; j < d; ++j) host &= fabsf(tail[j]) <= 1e-8f;
  return host;
}

// a node index a game may read: the search hands over indices in [0, nodes); anything else reads the root
__device__ inline int unified_node(int node, int nodes) { return node >= 0 && node < nodes ? node : 0; }

constexpr int kUnifiedKindBlock = 256;

// (the kernels are templates on the element type, float: a translation unit that launches none of them, such as the
// host build of the lane body in tests/unified_lane.hip, then carries no device code)
template <typename T>
__global__ void __launch_bounds__(kUnifiedKindBlock) unified_kind_kernel(UnifiedArgs a, int32_t* kind) {
  const int64_t b = (int64_t)blockIdx.x * kUnifiedKindBlock + threadIdx.x;
  bool host = false;
  if (b < a.batch) {
    const int n = a.m * a.d;
    const int64_t at = (b * a.nodes + unified_node(a.parent[b], a.nodes)) * (n + a.d) + n;
    host = unified_host_state(a.embeddings + at, a.d);
  }
  const bool any = __ballot(host) != 0ull;
  if (any && (threadIdx.x & (kWave - 1)) == 0) atomicOr(kind, 1);
}

struct UnifiedOutcome {
  uint32_t subset;  // the bit mask of the next tail
  float reward;
};

// One game: s.chd ++ s.c holds the parent state on entry and the next state on return, s.par receives the observation
// features of the next points; s.row is scratch.  kind 1 (a host state somewhere in the batch): the points stay, the
// tail becomes the subset of the class `action`, clamped as hk_decode_host_class clamps.  kind 0: hk_step in JAX
// semantics with the tail as the float mask and `action` as the axis (axis_index: outside [0, d) it matches nothing),
// then a zero tail.  The reward is the agent's: -(done and not done before), as hk_step computes it.
__device__ inline UnifiedOutcome unified_lane(const LaneSlice<float>& s, int m, int d, int kind, int action,
                                              bool reposition, bool scale) {
  const int n = m * d;
  const bool prev_done = num_points(s.chd, m, d) < 2;
  uint32_t sub = 0u;
  if (kind) {
    const int ncls = (1 << d) - d - 1;
    sub = decode_class(action < 0 ? 0 : (action >= ncls ? ncls - 1 : action), d);
    subset_coeffs(s.c, sub, d);
  } else {
    const unsigned stages = HK_STAGE_SHIFT | (reposition ? HK_STAGE_REPOSITION : 0u) | HK_STAGE_NEWTON;
    stages_game(s.chd, m, d, s.c, action >= 0 && action < d ? action : -1, -1.0f, stages, HK_SEM_JAX);
    for (int j = 0; j < d; ++j) s.c[j] = 0.0f;
  }
  const bool done = num_points(s.chd, m, d) < 2;
  for (int e = 0; e < n; ++e) s.par[e] = s.chd[e];
  stages_game(s.par, m, d, s.row, -1, -1.0f, (scale ? HK_STAGE_RESCALE : 0u) | kStageFeatureSort, HK_SEM_JAX);
  return {sub, -1.0f * (float)(done && !prev_done)};
}

template <typename T>
__global__ void __launch_bounds__(kWave) unified_expand_kernel(UnifiedArgs a) {
  extern __shared__ unsigned char hk_unified_lds[];
  float* lds = reinterpret_cast<float*>(hk_unified_lds);
  const int lane = threadIdx.x;
  const int m = a.m, d = a.d, n = m * d, len = n + d, S = a.lds_stride;
  const LaneBlock blk = lane_block(a.batch, a.games_per_block);
  const int64_t g0 = blk.g0;
  const int ngames = blk.ngames;
  const bool active = lane < ngames;
  int from = 0, to = -1, act = 0;
  if (active) {
    from = unified_node(a.parent[g0 + lane], a.nodes);
    to = a.node[g0 + lane];
    to = to >= 0 && to < a.nodes ? to : -1;  // a node outside the table is not written
    act = a.action[g0 + lane];
  }
  const int kind = *a.kind != 0;
  // element k of the record of game g, g and k advancing as in copy_slab; the state lands in chd ++ c
  const int total = ngames * len;
  const int dg = kWave / len, de = kWave % len;
  int g = lane / len, k = lane % len;
  for (int base = 0; base < total; base += kWave) {
    const bool valid = base + lane < total;
    const int node = __shfl(from, valid ? g : 0);
    if (valid) lds[(size_t)g * S + n + k] = a.embeddings[((g0 + g) * a.nodes + node) * len + k];
    g += dg;
    k += de;
    if (k >= len) {
      k -= len;
      ++g;
    }
  }
  __syncthreads();
  if (active) {
    const LaneSlice<float> s(lds, lane, S, m, d);
    const UnifiedOutcome o = unified_lane(s, m, d, kind, act, a.reposition != 0, a.scale != 0);
    a.subset[g0 + lane] = (int32_t)o.subset;
    a.reward[g0 + lane] = o.reward;
    a.discount_out[g0 + lane] = -a.discount;
  }
  __syncthreads();
  g = lane / len, k = lane % len;
  for (int base = 0; base < total; base += kWave) {
    const bool valid = base + lane < total;
    const int node = __shfl(to, valid ? g : 0);
    if (valid) {
      const float* slice = lds + (size_t)g * S;
      if (node >= 0) a.embeddings[((g0 + g) * a.nodes + node) * len + k] = slice[n + k];
      a.net_in[(g0 + g) * len + k] = k < n ? slice[k] : slice[n + k];
    }
    g += dg;
    k += de;
    if (k >= len) {
      k -= len;
      ++g;
    }
  }
}

struct UnifiedPriorArgs {
  const int32_t* kind;
  const float *agent_logits, *agent_value, *host_logits, *host_value;
  const int32_t* subset;
  float *prior, *value;
  int batch, d, actions;
};

// a thread per element of prior [batch, actions]; the thread of column 0 writes the game's value too
template <typename T>
__global__ void __launch_bounds__(256) unified_prior_kernel(UnifiedPriorArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)a.batch * a.actions) return;
  const int64_t b = idx / a.actions;
  const int j = (int)(idx - b * a.actions);
  if (*a.kind != 0) {  // the next node is an agent node: its logits behind the mask, padded with -inf
    const bool open = j < a.d && (((uint32_t)a.subset[b] >> j) & 1u);
    a.prior[idx] = open ? a.agent_logits[b * a.d + j] : -INFINITY;
    if (j == 0) a.value[b] = a.agent_value[b];
  } else {
    a.prior[idx] = a.host_logits[idx];
    if (j == 0) a.value[b] = a.host_value[b];
  }
}

}  // namespace hk
