// hk_search_morin_tree: the Morin game tree under a fixed host (hironaka/util/search.py:53-93 search_tree_morin).
//
// The traversal, the batches, the renumbering and the trailing-sibling walk are hk_search_tree_kernel.h's: one wave
// per root, a stack of record indices sorted by preorder, one popped node per lane, tree_finish at the end.  What a
// node carries on top of its state: integer weights w[0..d) and the index `dist` of its distinguished point.
//
// Expanding a node with the host's list `coords` (host_order_game), for each a in coords, in list order:
//   pruned   w[a] > min_{i in coords} w[i]: no record.  A node's child records stay contiguous, so a record keeps its
//            rank among them next to its child index (the position in the host's list, with gaps where actions were
//            pruned), and an expanded record keeps its child count, which is no longer the popcount of its class.
//   weights  w'[i] = w[i] - w[a] for i in coords, i != a; every other weight is kept.
//   state    shift, REPOSITION (list semantics: every column minus its minimum), Newton, sort-compact.
//   lost     with p the distinguished row after shift and reposition: some other live row q has q_k <= p_k for all k
//            (an identical row counts: the reference marks p, the marked row sorts before its twin and is removed as
//            contained).  Then the child is a "No contribution" leaf: kind 1, dist -1, never expanded.
//   kept     kind 0, dist = the position of p in the sorted, compacted state, where p is unique.
//
// The lane's weights and the saved row p live behind LaneSlice::row in its LDS slice (morin_lds_extra), and a child is
// expand_morin_child, both in hk_lane_games.h.
//
// Dimension 7: the hitting-set hosts run on the two-word support bitmap (Bits128) there, on uint64_t below.
#pragma once

#include "hk_lane_games.h"
#include "hk_search_tree_kernel.h"

namespace hk {

struct SearchMorinArgs {
  const void* points;            // [batch, m, d] roots, used as given
  const int32_t* weights;        // [batch, d]
  const int32_t* distinguished;  // [batch] a row index of the root
  void* rec_states;              // [batch, max_nodes, m*d] workspace: the recorded states
  int32_t* rec_ints;             // [batch, rec_int_stride] workspace: search_tree's words, then the fields below
  int32_t* parent_out;           // [batch, max_nodes] each, in preorder id order
  int32_t* child_index_out;
  int32_t* axis_out;
  int32_t* depth_out;
  int32_t* num_points_out;
  int32_t* host_class_out;
  int32_t* kind_out;
  int32_t* distinguished_out;
  int32_t* weights_out;  // [batch, max_nodes, d]
  void* states_out;      // [batch, max_nodes, m*d] or NULL
  int32_t* count_out;
  int32_t* status_out;
  long long expand_limit;  // < 0: none
  size_t rec_int_stride;
  int m, d, max_depth, max_nodes, stack_nodes, lanes, lds_stride;
};

// int32 words per root in rec_ints: search_tree's, then child count, sibling rank, kind, dist and d weights per record
inline uint64_t search_morin_int_words(int max_nodes, int stack_nodes, int d) {
  return search_tree_int_words(max_nodes, stack_nodes) + (4ull + (uint64_t)d) * (uint64_t)max_nodes;
}

// HOST: the host code, one instantiation per host
template <typename T, int HOST>
__global__ void __launch_bounds__(kWave) search_morin_kernel(SearchMorinArgs a) {
  extern __shared__ unsigned char hk_sm_lds[];
  __shared__ int slot_rec[kWave];
  __shared__ int slot_lane[kWave];
  __shared__ int slot_dst[kWave];
  __shared__ int sh_last, sh_count;
  T* lds = reinterpret_cast<T*>(hk_sm_lds);
  const int lane = threadIdx.x;
  const int m = a.m, d = a.d, n = m * d, M = a.max_nodes;
  const size_t root = blockIdx.x;
  const T* src = static_cast<const T*>(a.points) + root * (size_t)n;
  T* rst = static_cast<T*>(a.rec_states) + root * (size_t)M * n;
  const TreeRecords rec(a.rec_ints + root * a.rec_int_stride, M);
  int32_t *const rpar = rec.par, *const rchd = rec.chd, *const rax = rec.ax, *const rdep = rec.dep, *const rnp = rec.np,
                 *const rcls = rec.cls, *const rfirst = rec.first, *const rsize = rec.size, *const bstart = rec.bstart,
                 *const stk = rec.stk;
  int32_t* rcnt = stk + a.stack_nodes;  // an expanded record's child records
  int32_t* rrank = rcnt + M;            // a record's position among its siblings' records
  int32_t* rkind = rrank + M;
  int32_t* rdist = rkind + M;
  int32_t* rw = rdist + M;  // [M, d]
  const long long L = a.expand_limit < 0 ? LLONG_MAX - 1 : a.expand_limit;

  // the root: record 0, batch 0
  const int np0 = num_points(src, m, d);
  const int dist0 = a.distinguished[root];
  bool valid = dist0 >= 0 && dist0 < m && src[(dist0 >= 0 && dist0 < m ? dist0 : 0) * d] >= (T)0;
  for (int k = 0; k < d; ++k) valid &= a.weights[root * (size_t)d + k] >= 0;
  for (int e = lane; e < n; e += kWave) rst[e] = src[e];
  if (lane < d) rw[lane] = a.weights[root * (size_t)d + lane];
  if (lane == 0) {
    rpar[0] = -1, rchd[0] = -1, rax[0] = -1, rdep[0] = 0, rnp[0] = np0, rcls[0] = -1, rfirst[0] = -1, rsize[0] = 1;
    rcnt[0] = 0, rrank[0] = 0, rkind[0] = 0, rdist[0] = dist0;
    bstart[0] = 0, bstart[1] = 1;
    stk[0] = 0;
  }
  int status = (np0 < 2 ? HK_SEARCH_ROOT_ENDED : 0) | (valid ? 0 : HK_SEARCH_ROOT_INVALID);
  int top = status == 0 && a.max_depth > 0 ? 1 : 0;  // wave-uniform from here on
  int nrec = 1, nb = 1;

  const LaneSlice<T> sl(lds, lane, a.lds_stride, m, d);
  int32_t* w = reinterpret_cast<int32_t*>(sl.row + d);  // d int32 in the space of d elements
  T* prow = sl.row + 2 * d;
  for (long long it = 0; top > 0 && it <= L; ++it) {
    int k = top < a.lanes ? top : a.lanes;
    if ((long long)k > L + 1 - it) k = (int)(L + 1 - it);
    __syncthreads();  // the previous iteration's reads of slot_* and the parent slices are done
    if (lane < k) slot_rec[lane] = stk[top - 1 - lane];  // lane 0: the smallest pending preorder number
    __syncthreads();
    wave_copy_states(k, n, lane, [&](int s) { return lds + (size_t)s * a.lds_stride; },
                     [&](int s) { return rst + (size_t)slot_rec[s] * n; });
    const bool active = lane < k;
    const int me = active ? slot_rec[lane] : -1;
    const int dep = active ? rdep[me] : 0;
    const int pd = active ? rdist[me] : 0;
    top -= k;
    __syncthreads();
    uint32_t order = 0, keep = 0;  // keep, bit j: the j-th action of the host's list is not pruned
    int nc = 0, cls = -1;
    if (active) {
      cls = d < kLaneGameMaxDim ? host_order_game<T, HOST, uint64_t>(sl.par, m, d, order, nc)
                                : host_order_game<T, HOST, Bits128>(sl.par, m, d, order, nc);
      for (int i = 0; i < d; ++i) w[i] = rw[(size_t)me * d + i];
      int wmin = INT_MAX;
      for (int j = 0; j < nc; ++j) {
        const int wi = w[(order >> (3 * j)) & 7u];
        wmin = wi < wmin ? wi : wmin;
      }
      for (int j = 0; j < nc; ++j) keep |= w[(order >> (3 * j)) & 7u] > wmin ? 0u : 1u << j;
    }
    const int made = __popc(keep);
    int tot;
    const int rbase = nrec + lane_prefix<kLaneGameMaxDim>(made, tot);  // this lane's first child record
    if (tot > M - nrec) {
      status |= HK_SEARCH_NODE_LIMIT;
      break;
    }
    const uint32_t sub = cls < 0 ? 0u : decode_class(cls, d);
    if (active) {
      rcls[me] = cls;
      rfirst[me] = made ? rbase : -1;
      rcnt[me] = made;
      subset_coeffs(sl.c, sub, d);
    }
    uint32_t push = 0;  // bit j: the child of the lane's j-th action may be expanded
    bool stop = false;
    for (int j = 0; j < d; ++j) {
      if (__ballot(j < nc) == 0) break;
      const bool live = (keep >> j) & 1u;
      const int r = rbase + __popc(keep & ((1u << j) - 1u));
      bool inexact = false;
      if (live) {
        const int ax = (int)((order >> (3 * j)) & 7u);
        int dist;
        const int np = expand_morin_child(sl, prow, m, d, ax, pd, inexact, dist);
        rpar[r] = me, rchd[r] = j, rax[r] = ax, rdep[r] = dep + 1, rnp[r] = np, rcls[r] = -1, rfirst[r] = -1,
        rsize[r] = 1;
        rcnt[r] = 0, rrank[r] = r - rbase, rkind[r] = dist < 0 ? 1 : 0, rdist[r] = dist;
        const int wa = w[ax];
        for (int i = 0; i < d; ++i) rw[(size_t)r * d + i] = ((sub >> i) & 1u) && i != ax ? w[i] - wa : w[i];
        if (dist >= 0 && np >= 2 && dep + 1 < a.max_depth) push |= 1u << j;
      }
      if (__ballot(inexact)) {
        status |= HK_SEARCH_INEXACT;
        stop = true;
        break;
      }
      const unsigned long long b = __ballot(live);
      const int cnt = (int)__popcll(b);
      if (cnt == 0) continue;  // every lane pruned its j-th action
      if (live) {
        const int rank = lane_rank(b);
        slot_lane[rank] = lane;
        slot_dst[rank] = r;
      }
      __syncthreads();
      wave_copy_states(cnt, n, lane, [&](int s) { return rst + (size_t)slot_dst[s] * n; },
                       [&](int s) { return lds + (size_t)slot_lane[s] * a.lds_stride + n; });
      __syncthreads();
    }
    if (stop) break;
    int ptot;
    const int ppre = lane_prefix<kLaneGameMaxDim>(__popc(push), ptot);
    if (ptot > a.stack_nodes - top) {
      status |= HK_SEARCH_STACK_LIMIT;
      break;
    }
    // the pushable children in reverse record order: the first child of the first popped node ends on top
    int q = ppre;
    for (int j = 0; j < d; ++j)
      if ((push >> j) & 1u) stk[top + ptot - 1 - q++] = rbase + __popc(keep & ((1u << j) - 1u));
    top += ptot;
    nrec += tot;
    if (tot > 0) bstart[++nb] = nrec;
  }
  __syncthreads();

  const TreeOutputs<T> out{a.parent_out, a.child_index_out, a.axis_out, a.depth_out, a.num_points_out,
                           a.host_class_out, static_cast<T*>(a.states_out), a.count_out, a.status_out};
  tree_finish(
      rec, rst, out, root, lane, n, M, d, nrec, nb, L, a.max_depth, status, slot_dst, sh_last, sh_count,
      [&](int r) { return rcnt[r]; }, [&](int r) { return rrank[r]; },
      [&](int r) { return rkind[r] == 0 && rnp[r] >= 2; },
      [&](int r, size_t o) {
        a.kind_out[o] = rkind[r];
        a.distinguished_out[o] = rdist[r];
        for (int i = 0; i < d; ++i) a.weights_out[o * d + i] = rw[(size_t)r * d + i];
      });
}

}  // namespace hk
