// What hk_search_depth, hk_search_game_tree and hk_search_morin_tree share: one workgroup of one wave per root, whose
// lanes expand one node each in a private slice of the dynamic LDS; and the whole-wave copy of states between those
// slices and memory that the two tree operators use.
#pragma once

#include "hk_hosts.h"

namespace hk {

constexpr int kSearchLdsBytes = 64 * 1024;  // dynamic LDS per workgroup: two or more roots share a CU

// LDS elements per lane: parent, child, the shift coefficients c, sort_compact's row scratch and `extra` elements
// behind them that a kernel keeps for itself; odd, so that the lanes' private slices start in different banks
inline int search_lds_stride(int m, int d, int extra = 0) { return (2 * m * d + 2 * d + extra) | 1; }

// A lane's slice of the dynamic LDS, laid out as search_lds_stride counts it
template <typename T>
struct LaneSlice {
  T *par, *chd, *c, *row;
  __device__ LaneSlice(T* lds, int lane, int stride, int m, int d)
      : par(lds + (size_t)lane * stride), chd(par + m * d), c(chd + m * d), row(c + d) {}
};

// Launches kernel over `batch` roots, one wave each, after filling in a.lds_stride and a.lanes (the lanes whose slices
// fit into kSearchLdsBytes, at most a wave).  Args: the kernel's argument block, with m, d, lds_stride and lanes.
// extra_lds: elements a lane keeps behind LaneSlice::row.
template <typename T, typename Args>
int launch_search(void (*kernel)(Args), Args a, int batch, hipStream_t stream, int extra_lds = 0) {
  a.lds_stride = search_lds_stride(a.m, a.d, extra_lds);
  const int per_lane = a.lds_stride * (int)sizeof(T);
  a.lanes = kSearchLdsBytes / per_lane < kWave ? kSearchLdsBytes / per_lane : kWave;
  const size_t lds = (size_t)a.lanes * per_lane;
  launch_prepare();
  hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(kWave), lds, stream, a);
  return launch_status();
}

// The child that the agent's axis `ax` makes of the game in s.par, written to s.chd: shift by the host's coefficients
// in s.c, Newton, sort-compact, all in list semantics.  ORs into `inexact` whether a shifted coordinate reached 2^24
// (float) / 2^53 (double), from where on integers are no longer exact.  Returns the child's number of points.
template <typename T>
__device__ inline int expand_child(const LaneSlice<T>& s, int m, int d, int ax, bool& inexact) {
  const T limit = sizeof(T) == 4 ? (T)16777216.0 : (T)9007199254740992.0;
  const unsigned flags = HK_SEM_LIST | HK_FLAG_COMPACT_SORTED;
  for (int e = 0; e < m * d; ++e) s.chd[e] = s.par[e];
  shift_game(s.chd, m, d, s.c, ax, (T)-1, flags);
  for (int i = 0; i < m; ++i) inexact |= s.chd[i * d + ax] >= limit;
  newton_game(s.chd, m, d, (T)-1, flags);
  sort_compact_game(s.chd, m, d, (T)-1, s.row);
  return num_points(s.chd, m, d);
}

// the number of lanes below this one whose bit is set in the wave mask b
__device__ inline int lane_rank(unsigned long long b) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// exclusive prefix over the lanes of a per-lane count in 0..MAXV, and the wave's total
template <int MAXV = 6>
__device__ inline int lane_prefix(int v, int& total) {
  int pre = 0;
  total = 0;
  for (int j = 0; j < MAXV; ++j) {
    const unsigned long long b = __ballot(v > j);
    pre += lane_rank(b);
    total += (int)__popcll(b);
  }
  return pre;
}

// The whole wave copies k states of n elements: state s from src(s) to dst(s).  No per-state condition: a test of
// dst(s) against null in this loop cost search_tree 14 % of its time on the 5552-deep root.
template <typename Dst, typename Src>
__device__ inline void wave_copy_states(int k, int n, int lane, Dst dst, Src src) {
  for (int e = lane; e < k * n; e += kWave) {
    const int s = e / n;
    dst(s)[e - s * n] = src(s)[e - s * n];
  }
}

}  // namespace hk
