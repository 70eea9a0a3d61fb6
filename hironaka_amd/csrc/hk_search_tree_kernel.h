// hk_search_game_tree: the game tree under a fixed host, node by node (hironaka/util/search.py:35-50 search_tree).
//
// One workgroup of one wave per root, in two parts.
//
// Traversal.  Every created node becomes a record in the caller's workspace: its state, parent record, child index
// (the position in the parent's host list), axis, depth and number of points.  Nodes that may be expanded (>= 2
// points, depth < max_depth) wait on a stack of record indices that is kept sorted by preorder, the smallest on top.
// An iteration pops the k smallest, one per lane, and expands them in LDS with the list-semantics routines of
// hk_game_generic.h.  Every child is recorded, ended or not; the children of one parent are contiguous records in
// host order.  The stack stays sorted because the pending nodes root disjoint subtrees: the children of the i-th
// popped node come before the (i+1)-th popped node in preorder.  So they are pushed in reverse record order.
//
// Truncation at L = expand_limit.  Each iteration pops the smallest pending preorder number, which is larger than the
// previous iteration's, so after L+1 iterations every expandable node numbered <= L has been expanded, and the
// i-th popped node of iteration t is numbered >= t + i (no pop beyond L is needed).  Nodes beyond L that a wide pop
// expanded are recorded and then dropped.
//
// Renumbering.  Records form batches, one per iteration, and a batch's parents lie in earlier batches.  Subtree sizes
// go bottom-up over the batches; preorder ids go top-down (parent id + 1 + the sizes of the earlier siblings).  These
// ids equal the full tree's up to L+1.  The walk from node L+1 to the root then numbers the trailing siblings
// (L+2, ...): the children after the path child, the deepest parent first, as the reference creates them while its
// recursion unwinds.  Last, the records are scattered into the outputs by id.
//
// The renumbering and the scatter are tree_finish, which hk_search_morin_kernel.h calls as well.
//
// Bounded by construction: records stop at max_nodes, the stack at stack_nodes, depth at max_depth; every loop of the
// renumbering runs over recorded batches or up a parent chain of strictly decreasing record indices.
#pragma once

#include "hk_search_wave.h"

namespace hk {

struct SearchTreeArgs {
  const void* points;  // [batch, m, d] roots, used as given
  void* rec_states;    // [batch, max_nodes, m*d] workspace: the recorded states
  int32_t* rec_ints;   // [batch, rec_int_stride] workspace: the record fields, batch starts and the stack
  int32_t* parent_out;  // [batch, max_nodes] each, in preorder id order
  int32_t* child_index_out;
  int32_t* axis_out;
  int32_t* depth_out;
  int32_t* num_points_out;
  int32_t* host_class_out;
  void* states_out;  // [batch, max_nodes, m*d] or NULL
  int32_t* count_out;
  int32_t* status_out;
  long long expand_limit;  // < 0: none
  size_t rec_int_stride;
  int m, d, max_depth, max_nodes, stack_nodes, lanes, lds_stride;
};

// int32 words per root in rec_ints: nine record fields, max_nodes + 1 batch starts, the stack
inline uint64_t search_tree_int_words(int max_nodes, int stack_nodes) {
  return 10ull * (uint64_t)max_nodes + 1ull + (uint64_t)stack_nodes;
}

// The host's list for one game, in the reference's order.  Zeillinger and ZeillingerLex return [argmin v, argmax v]
// of the chosen pair (host.py:90-95, :116-127), or [0, 1] when they coincide: `order` packs the axes 3 bits each.  The
// other hosts' lists are ascending.  Returns the class id of the set, -1 for no list (nc = 0).  B as in host_class_game.
template <typename T, int HOST, typename B = uint64_t>
__device__ inline int host_order_game(const T* p, int m, int d, uint32_t& order, int& nc) {
  order = 0;
  nc = 0;
  if (HOST == HK_HOST_ZEILLINGER || HOST == HK_HOST_ZEILLINGER_LEX) {
    const int r = zeillinger_list_pair<T, HOST == HK_HOST_ZEILLINGER_LEX>(p, m, d);
    if (r < 0) return -1;
    order = (uint32_t)(r >> 3) | ((uint32_t)(r & 7) << 3);
    nc = 2;
    return encode_mask((1u << (r >> 3)) | (1u << (r & 7)));
  }
  const int cls = host_class_game<T, HOST, B>(p, m, d);
  if (cls < 0) return -1;
  const uint32_t sub = decode_class(cls, d);
  for (int j = 0; j < d; ++j)
    if ((sub >> j) & 1u) order |= (uint32_t)j << (3 * nc++);
  return cls;
}

// The record fields of one root in rec_ints, each max_nodes long, then the batch starts and the stack
struct TreeRecords {
  int32_t *par, *chd, *ax, *dep, *np, *cls, *first, *size, *id, *bstart, *stk;
  __device__ TreeRecords(int32_t* iw, int M)
      : par(iw), chd(par + M), ax(chd + M), dep(ax + M), np(dep + M), cls(np + M), first(cls + M), size(first + M),
        id(size + M), bstart(id + M),  // M + 1: batch b holds the records [bstart[b], bstart[b+1])
        stk(bstart + M + 1) {}
};

// the outputs the tree operators share, [batch, max_nodes] each
template <typename T>
struct TreeOutputs {
  int32_t *parent, *child_index, *axis, *depth, *num_points, *host_class;
  T* states;
  int32_t *count, *status;
};

// After the traversal: the renumbering and the scatter by id (see the head of this file), for hk_search_game_tree and
// hk_search_morin_tree.  children(r): the child records of an expanded record r, contiguous from first[r]; rank(r): r's
// position among its siblings' records; expandable(r): whether the reference would expand r (apart from its depth);
// extra(r, o): writes the operator's own outputs of record r to slot o.
template <typename T, typename Children, typename Rank, typename Expandable, typename Extra>
__device__ inline void tree_finish(const TreeRecords& rec, const T* rst, const TreeOutputs<T>& out, size_t root, int lane,
                                   int n, int M, int d, int nrec, int nb, long long L, int max_depth, int status,
                                   int* slot_dst, int& sh_last, int& sh_count, Children children, Rank rank,
                                   Expandable expandable, Extra extra) {
  int32_t *const rpar = rec.par, *const rchd = rec.chd, *const rax = rec.ax, *const rdep = rec.dep, *const rnp = rec.np,
                 *const rcls = rec.cls, *const rfirst = rec.first, *const rsize = rec.size, *const rid = rec.id,
                 *const bstart = rec.bstart;
  const size_t out0 = root * (size_t)M;
  if (status & (HK_SEARCH_NODE_LIMIT | HK_SEARCH_STACK_LIMIT | HK_SEARCH_INEXACT)) {
    if (lane == 0) {
      out.count[root] = nrec;
      out.status[root] = status;
    }
    return;
  }

  // subtree sizes, bottom-up: a batch's children lie in later batches
  for (int b = nb - 1; b >= 0; --b) {
    for (int r = bstart[b] + lane; r < bstart[b + 1]; r += kWave) {
      const int f = rfirst[r];
      if (f < 0) continue;
      const int cnt = children(r);
      int s = 1;
      for (int i = 0; i < cnt; ++i) s += rsize[f + i];
      rsize[r] = s;
    }
    __syncthreads();
  }
  // preorder ids, top-down; -1 beyond L+1
  if (lane == 0) {
    rid[0] = 0;
    sh_last = -1;  // the record numbered L+1, if the tree has one
  }
  __syncthreads();
  for (int b = 1; b < nb; ++b) {
    for (int r = bstart[b] + lane; r < bstart[b + 1]; r += kWave) {
      const int pid = rid[rpar[r]];
      int id = -1;
      if (pid >= 0) {
        long long v = (long long)pid + 1;
        for (int t = 1, e = rank(r); t <= e; ++t) v += rsize[r - t];
        if (v <= L + 1) id = (int)v;
        if (v == L + 1) sh_last = r;
      }
      rid[r] = id;
    }
    __syncthreads();
  }
  // the trailing siblings, numbered from L+2 while walking up from node L+1
  if (lane == 0) {
    int count = nrec;
    if (sh_last >= 0) {
      int next = (int)(L + 2);
      for (int cur = sh_last; cur > 0;) {
        const int p = rpar[cur], ci = rank(cur);
        const int cnt = children(p);
        for (int k = ci + 1; k < cnt; ++k) rid[cur - ci + k] = next++;
        cur = p;
      }
      count = next;
    }
    sh_count = count;
  }
  __syncthreads();
  const int count = sh_count;

  // scatter by id
  T* sout = out.states;
  bool cut = false;
  for (int cb = 0; cb < nrec; cb += kWave) {
    const int r = cb + lane;
    int id = r < nrec ? rid[r] : -1;
    if (id >= count) id = -1;  // not reached: ids are < count by construction
    if (id >= 0) {
      const size_t o = out0 + (size_t)id;
      const bool inside = id <= L;  // expanded by the reference when it holds >= 2 points
      out.parent[o] = r == 0 ? -1 : rid[rpar[r]];
      out.child_index[o] = rchd[r];
      out.axis[o] = rax[r];
      out.depth[o] = rdep[r];
      out.num_points[o] = rnp[r];
      out.host_class[o] = inside && expandable(r) && rdep[r] < max_depth ? rcls[r] : -1;
      cut |= inside && expandable(r) && rdep[r] >= max_depth;
      extra(r, o);
    }
    if (sout) {
      slot_dst[lane] = id;
      __syncthreads();
      const int cn = nrec - cb < kWave ? nrec - cb : kWave;
      for (int e = lane; e < cn * n; e += kWave) {  // wave_copy_states, but only the records that have an id
        const int s = e / n;
        if (slot_dst[s] >= 0) sout[(out0 + (size_t)slot_dst[s]) * n + (e - s * n)] = rst[(size_t)(cb + s) * n + (e - s * n)];
      }
      __syncthreads();
    }
  }
  if (__ballot(cut)) status |= HK_SEARCH_DEPTH_LIMIT;
  if (lane == 0) {
    out.count[root] = count;
    out.status[root] = status;
  }
}

// HOST: the host code, one instantiation per host
template <typename T, int HOST>
__global__ void __launch_bounds__(kWave) search_tree_kernel(SearchTreeArgs a) {
  extern __shared__ unsigned char hk_st_lds[];
  __shared__ int slot_rec[kWave];
  __shared__ int slot_lane[kWave];
  __shared__ int slot_dst[kWave];
  __shared__ int sh_last, sh_count;
  T* lds = reinterpret_cast<T*>(hk_st_lds);
  const int lane = threadIdx.x;
  const int m = a.m, d = a.d, n = m * d, M = a.max_nodes;
  const size_t root = blockIdx.x;
  const T* src = static_cast<const T*>(a.points) + root * (size_t)n;
  T* rst = static_cast<T*>(a.rec_states) + root * (size_t)M * n;
  const TreeRecords rec(a.rec_ints + root * a.rec_int_stride, M);
  int32_t *const rpar = rec.par, *const rchd = rec.chd, *const rax = rec.ax, *const rdep = rec.dep, *const rnp = rec.np,
                 *const rcls = rec.cls, *const rfirst = rec.first, *const rsize = rec.size, *const bstart = rec.bstart,
                 *const stk = rec.stk;
  const long long L = a.expand_limit < 0 ? LLONG_MAX - 1 : a.expand_limit;

  // the root: record 0, batch 0
  const int np0 = num_points(src, m, d);
  for (int e = lane; e < n; e += kWave) rst[e] = src[e];
  if (lane == 0) {
    rpar[0] = -1, rchd[0] = -1, rax[0] = -1, rdep[0] = 0, rnp[0] = np0, rcls[0] = -1, rfirst[0] = -1, rsize[0] = 1;
    bstart[0] = 0, bstart[1] = 1;
    stk[0] = 0;
  }
  int status = np0 < 2 ? HK_SEARCH_ROOT_ENDED : 0;
  int top = np0 >= 2 && a.max_depth > 0 ? 1 : 0;  // wave-uniform from here on
  int nrec = 1, nb = 1;

  const LaneSlice<T> sl(lds, lane, a.lds_stride, m, d);
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
    top -= k;
    __syncthreads();
    uint32_t order = 0;
    int nc = 0, cls = -1;
    if (active) cls = host_order_game<T, HOST>(sl.par, m, d, order, nc);
    int tot;
    const int rbase = nrec + lane_prefix(nc, tot);  // this lane's first child record
    if (tot > M - nrec) {
      status |= HK_SEARCH_NODE_LIMIT;
      break;
    }
    if (active) {
      rcls[me] = cls;
      rfirst[me] = nc ? rbase : -1;
      const uint32_t sub = cls < 0 ? 0u : decode_class(cls, d);
      for (int j = 0; j < d; ++j) sl.c[j] = ((sub >> j) & 1u) ? (T)1 : (T)0;
    }
    uint32_t push = 0;  // bit j: the lane's j-th child may be expanded
    bool stop = false;
    for (int j = 0; j < d; ++j) {
      const bool live = j < nc;
      bool inexact = false;
      if (live) {
        const int ax = (int)((order >> (3 * j)) & 7u);
        const int np = expand_child(sl, m, d, ax, inexact);
        const int r = rbase + j;
        rpar[r] = me, rchd[r] = j, rax[r] = ax, rdep[r] = dep + 1, rnp[r] = np, rcls[r] = -1, rfirst[r] = -1,
        rsize[r] = 1;
        if (np >= 2 && dep + 1 < a.max_depth) push |= 1u << j;
      }
      if (__ballot(inexact)) {
        status |= HK_SEARCH_INEXACT;
        stop = true;
        break;
      }
      const unsigned long long b = __ballot(live);
      const int cnt = (int)__popcll(b);
      if (cnt == 0) break;  // j >= nc on every lane
      if (live) {
        const int rank = lane_rank(b);
        slot_lane[rank] = lane;
        slot_dst[rank] = rbase + j;
      }
      __syncthreads();
      wave_copy_states(cnt, n, lane, [&](int s) { return rst + (size_t)slot_dst[s] * n; },
                       [&](int s) { return lds + (size_t)slot_lane[s] * a.lds_stride + n; });
      __syncthreads();
    }
    if (stop) break;
    int ptot;
    const int ppre = lane_prefix(__popc(push), ptot);
    if (ptot > a.stack_nodes - top) {
      status |= HK_SEARCH_STACK_LIMIT;
      break;
    }
    // the pushable children in reverse record order: the first child of the first popped node ends on top
    int q = ppre;
    for (int j = 0; j < d; ++j)
      if ((push >> j) & 1u) stk[top + ptot - 1 - q++] = rbase + j;
    top += ptot;
    nrec += tot;
    if (tot > 0) bstart[++nb] = nrec;
  }
  __syncthreads();

  const TreeOutputs<T> out{a.parent_out, a.child_index_out, a.axis_out, a.depth_out, a.num_points_out,
                           a.host_class_out, static_cast<T*>(a.states_out), a.count_out, a.status_out};
  tree_finish(
      rec, rst, out, root, lane, n, M, d, nrec, nb, L, a.max_depth, status, slot_dst, sh_last, sh_count,
      [&](int r) { return __popc(decode_class(rcls[r], d)); }, [&](int r) { return rchd[r]; },
      [&](int r) { return rnp[r] >= 2; }, [](int, size_t) {});
}

}  // namespace hk
