// hk_tree_expand: one level of a game tree under any host (hironaka/jax/search.py:73-113 search_tree_fix_host over a
// whole frontier).  The host ran outside; a launch makes, for every parent, one child per coordinate of the subset the
// host chose, and packs the children at the slots the caller's prefix sum assigns.
//
// The frame is hk_lane_games.h's, with search_lds_stride's slices: lane g makes parent g's children one after another
// in the child half of its slice.  The child sequence is its own: it takes its semantics at run time and has no inexact
// test.  Round r: every lane whose parent has more than r children makes child r, then the whole wave copies the round's
// children from LDS to their slots, consecutive lanes writing consecutive elements of a record.  The coefficients c sit
// right behind the child half, so the zero tail of a record (search.py:107) leaves in the same copy.  HBM traffic: one
// read of each parent however many children it has, one write of each child, 13 B of bookkeeping per child.  No
// spinning: a child's slot is known before the launch, and every loop is bounded by m, d or the parents of the block.
#pragma once

#include "hk_lane_games.h"

namespace hk {

struct TreeExpandArgs {
  const void* parents;  // [n_parents] records of in_stride elements; the state is the first m*d
  void* children;       // [capacity] records of out_stride elements
  const int32_t* class_id;
  const int64_t* child_offset;
  int32_t* child_parent;
  int32_t* child_axis;
  int32_t* child_num_points;
  uint8_t* child_done;
  uint32_t* status;
  int64_t in_stride, out_stride;
  int n_parents, capacity, m, d, list, reposition, zero_tail, lds_stride, parents_per_block;
};

template <typename T>
__global__ void __launch_bounds__(kWave) tree_expand_kernel(TreeExpandArgs a) {
  extern __shared__ unsigned char hk_te_lds[];
  T* lds = reinterpret_cast<T*>(hk_te_lds);
  const int lane = threadIdx.x;
  const int m = a.m, d = a.d, n = m * d;
  const LaneBlock blk = lane_block(a.n_parents, a.parents_per_block);
  const int64_t g0 = blk.g0;
  const int nparents = blk.ngames;
  // the subsets first: a block none of whose parents is expanded reads no state
  uint32_t sub = 0u;
  int64_t first = 0;
  if (lane < nparents) {
    const int cls = a.class_id[g0 + lane];
    if (cls >= 0 && cls < (1 << d) - d - 1) sub = decode_class(cls, d);
    first = a.child_offset[g0 + lane];
  }
  const int count = __popc(sub);
  if (__ballot(count > 0) == 0ull) return;
  stage_games(lds, a.parents, a.in_stride, n, a.lds_stride, blk, lane);
  __syncthreads();
  const LaneSlice<T> s(lds, lane < nparents ? lane : 0, a.lds_stride, m, d);
  const unsigned flags = a.list ? kListFlags : HK_SEM_JAX;
  const int len = n + (a.zero_tail ? d : 0);  // elements of a record that leave: the state, then c
  const int dg = kWave / len, de = kWave % len;
  bool overflow = false;
  for (int r = 0; r < d; ++r) {
    if (__ballot(count > r) == 0ull) break;
    int slot = -1;  // where this lane's child of the round goes; -1: it has none, or no room
    if (count > r) {
      const int ax = nth_bit(sub, r);
      subset_coeffs(s.c, sub, d);
      for (int e = 0; e < n; ++e) s.chd[e] = s.par[e];
      shift_game(s.chd, m, d, s.c, ax, (T)-1, flags);
      if (a.reposition) reposition_game(s.chd, m, d, (T)-1, flags);
      newton_game(s.chd, m, d, (T)-1, flags);
      if (a.list) sort_compact_game(s.chd, m, d, (T)-1, s.row);
      for (int j = 0; j < d; ++j) s.c[j] = (T)0;
      const int64_t want = first + r;
      if (want >= 0 && want < (int64_t)a.capacity) {
        slot = (int)want;
        const int np = num_points(s.chd, m, d);
        int nonneg = 0;
        for (int e = 0; e < n; ++e) nonneg += (s.chd[e] >= (T)0) ? 1 : 0;
        a.child_parent[slot] = (int32_t)(g0 + lane);
        a.child_axis[slot] = ax;
        a.child_num_points[slot] = np;
        a.child_done[slot] = (uint8_t)(a.list ? np < 2 : nonneg <= d);
      } else {
        overflow = true;
      }
    }
    __syncthreads();
    // the round's children leave: element k of the child of parent g, g and k advancing as in copy_slab
    T* const out = static_cast<T*>(a.children);
    const int total = nparents * len;
    int g = lane / len, k = lane % len;
    for (int base = 0; base < total; base += kWave) {
      const bool valid = base + lane < total;
      const int to = __shfl(slot, valid ? g : 0);
      if (valid && to >= 0) out[(int64_t)to * a.out_stride + k] = lds[(size_t)g * a.lds_stride + n + k];
      g += dg;
      k += de;
      if (k >= len) {
        k -= len;
        ++g;
      }
    }
    __syncthreads();
  }
  if (overflow) atomicOr(a.status, HK_TREE_OVERFLOW);
}

}  // namespace hk
