// hk_search_depth: exhaustive worst-case game length under a fixed host (hironaka/util/search.py:9-32).
//
// One workgroup of one wave per root; the root's pending nodes live on a LIFO stack in the caller's workspace (an
// entry = the max_points*dim coordinates, plus an int32 depth in a parallel array).  Every iteration pops up to
// `lanes` nodes from the top, one per lane, and expands them in LDS with the list-semantics routines of
// hk_game_generic.h: the host's subset I (hk_hosts.h: Zeillinger, all coordinates, ZeillingerLex or a weak
// Spivakovsky host), then per axis a in I a copy of the parent, shift x_a <- sum_{k in I} x_k, Newton, sort-compact.  Children with >= 2 points are pushed back, in axis-then-lane
// order, at positions a wave prefix sum hands out.  Depth max and node count are independent of the traversal order;
// the stack's peak size is not.
//
// Bounded by construction: every iteration visits >= 1 node, nodes stop at max_nodes, children stop at max_depth and
// at the stack's capacity.  No communication between workgroups.
#pragma once

#include "hk_search_wave.h"

namespace hk {

struct SearchDepthArgs {
  const void* points;  // [batch, m, d] roots, used as given
  void* stack;         // [batch, stack_nodes, m*d] states
  int32_t* stack_depth;  // [batch, stack_nodes]
  int32_t* depth_out;
  unsigned long long* nodes_out;
  int32_t* status_out;
  unsigned long long max_nodes;
  int m, d, host, max_depth, stack_nodes, lanes, lds_stride;
};

// HOST: the host code, one instantiation per host (a.host is not read)
template <typename T, int HOST>
__global__ void __launch_bounds__(kWave) search_depth_kernel(SearchDepthArgs a) {
  extern __shared__ unsigned char hk_sd_lds[];
  __shared__ int slot_lane[kWave];
  __shared__ int lane_max[kWave];
  T* lds = reinterpret_cast<T*>(hk_sd_lds);
  const int lane = threadIdx.x;
  const int m = a.m, d = a.d, n = m * d, L = a.lanes;
  const size_t root = blockIdx.x;
  const T* src = static_cast<const T*>(a.points) + root * (size_t)n;
  T* stk = static_cast<T*>(a.stack) + root * (size_t)a.stack_nodes * (size_t)n;
  int32_t* sdep = a.stack_depth + root * (size_t)a.stack_nodes;

  if (num_points(src, m, d) < 2) {
    if (lane == 0) {
      a.depth_out[root] = 0;
      a.nodes_out[root] = 0ull;
      a.status_out[root] = HK_SEARCH_ROOT_ENDED;
    }
    return;
  }
  for (int e = lane; e < n; e += kWave) stk[e] = src[e];
  if (lane == 0) sdep[0] = 0;
  __syncthreads();

  const LaneSlice<T> sl(lds, lane, a.lds_stride, m, d);
  int top = 1;  // wave-uniform from here on
  unsigned long long nodes = 0;
  int status = 0;
  int my_max = -1;
  while (top > 0) {
    int k = top < L ? top : L;
    if ((unsigned long long)k > a.max_nodes - nodes) k = (int)(a.max_nodes - nodes);
    const int base = top - k;
    __syncthreads();  // the previous iteration's reads of the parent slices are done
    // pop: the k top entries are contiguous, copied by the whole wave.  This loop and the push are written out rather
    // than wave_copy_states: through the helper the 2 048-root batch of scripts/probe_search_depth.py ran 1.6 % slower.
    for (int e = lane; e < k * n; e += kWave) {
      const int s = e / n;
      lds[(size_t)s * a.lds_stride + (e - s * n)] = stk[(size_t)base * n + e];
    }
    const bool active = lane < k;
    const int dep = active ? sdep[base + lane] : 0;
    top = base;
    nodes += (unsigned long long)k;
    __syncthreads();
    if (active && dep > my_max) my_max = dep;
    const bool capped = active && dep >= a.max_depth;
    if (__ballot(capped)) status |= HK_SEARCH_DEPTH_LIMIT;
    const bool expand = active && !capped;
    uint32_t subset = 0;
    if (expand) {
      // -1 (a zero row, or |U| < 2 for WeakSpivakovsky) only at a root that is not Newton-reduced: no children.  Never
      // for Zeillinger, whose -1 needs fewer than 2 points, which no visited node holds.  All coordinates skips the
      // class round trip: its decode loop costs the float64 instance an occupancy level.
      const int cls = host_class_game<T, HOST>(sl.par, m, d);
      subset = HOST == HK_HOST_ALL_COORD ? (1u << d) - 1u : cls < 0 ? 0u : decode_class(cls, d);
      for (int j = 0; j < d; ++j) sl.c[j] = ((subset >> j) & 1u) ? (T)1 : (T)0;
    }
    bool stop = false;
    for (int j = 0; j < d; ++j) {
      bool live = expand && ((subset >> j) & 1u);
      bool inexact = false;
      if (live) live = expand_child(sl, m, d, j, inexact) >= 2;
      if (__ballot(inexact)) {
        status |= HK_SEARCH_INEXACT;
        stop = true;
        break;
      }
      const unsigned long long b = __ballot(live);
      const int cnt = (int)__popcll(b);
      if (cnt == 0) continue;
      if (top + cnt > a.stack_nodes) {
        status |= HK_SEARCH_STACK_LIMIT;
        stop = true;
        break;
      }
      if (live) {
        const int rank = lane_rank(b);
        slot_lane[rank] = lane;
        sdep[top + rank] = dep + 1;
      }
      __syncthreads();
      // push: the cnt new entries are contiguous, written by the whole wave
      for (int e = lane; e < cnt * n; e += kWave) {
        const int s = e / n;
        stk[(size_t)(top + s) * n + (e - s * n)] = lds[(size_t)slot_lane[s] * a.lds_stride + n + (e - s * n)];
      }
      top += cnt;
      __syncthreads();
    }
    if (stop) break;
    if (nodes >= a.max_nodes && top > 0) {
      status |= HK_SEARCH_NODE_LIMIT;
      break;
    }
  }
  lane_max[lane] = my_max;
  __syncthreads();
  if (lane == 0) {
    int mx = -1;
    for (int l = 0; l < kWave; ++l) mx = lane_max[l] > mx ? lane_max[l] : mx;
    a.depth_out[root] = mx + 1;
    a.nodes_out[root] = nodes;
    a.status_out[root] = status;
  }
}

}  // namespace hk
