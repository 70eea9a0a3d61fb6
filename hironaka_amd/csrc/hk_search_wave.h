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

// The launch shape of the one-game-per-lane operators: the games whose LDS slices of lds_stride elements fit into
// kSearchLdsBytes, at most a wave; the workgroups that `count` games then take; the dynamic LDS of one workgroup
struct LaneGeometry {
  int per_block;
  unsigned grid;
  size_t lds;
};
inline LaneGeometry lane_geometry(int lds_stride, size_t elem_size, int64_t count) {
  const int per_game = lds_stride * (int)elem_size;
  const int per_block = kSearchLdsBytes / per_game < kWave ? kSearchLdsBytes / per_game : kWave;
  return {per_block, (unsigned)((count + per_block - 1) / per_block), (size_t)per_block * per_game};
}

// Launches kernel over `batch` roots, one wave each, after filling in a.lds_stride and a.lanes (lane_geometry's games
// per block).  Args: the kernel's argument block, with m, d, lds_stride and lanes.  extra_lds: elements a lane keeps
// behind LaneSlice::row.
template <typename T, typename Args>
int launch_search(void (*kernel)(Args), Args a, int batch, hipStream_t stream, int extra_lds = 0) {
  a.lds_stride = search_lds_stride(a.m, a.d, extra_lds);
  const LaneGeometry geo = lane_geometry(a.lds_stride, sizeof(T), batch);
  a.lanes = geo.per_block;
  return launch_kernel(kernel, dim3((unsigned)batch), dim3(kWave), geo.lds, stream, a);
}

constexpr unsigned kListFlags = HK_SEM_LIST | HK_FLAG_COMPACT_SORTED;  // the semantics every lane game is played in

// The pieces of a move.  "Shift the child": the game in s.par copied to s.chd and shifted along `ax` by the host's
// coefficients in s.c.
template <typename T>
__device__ inline void shift_child(const LaneSlice<T>& s, int m, int d, int ax) {
  for (int e = 0; e < m * d; ++e) s.chd[e] = s.par[e];
  shift_game(s.chd, m, d, s.c, ax, (T)-1, kListFlags);
}

// from here on integers are no longer exact: 2^24 (float) / 2^53 (double)
template <typename T>
constexpr T kExactLimit = sizeof(T) == 4 ? (T)16777216.0 : (T)9007199254740992.0;

// The inexact test behind the shift: ORs into `inexact` whether a shifted coordinate of s.chd reached kExactLimit.
template <typename T>
__device__ inline void note_inexact(const LaneSlice<T>& s, int m, int d, int ax, bool& inexact) {
  for (int i = 0; i < m; ++i) inexact |= s.chd[i * d + ax] >= kExactLimit<T>;
}

// "Reduce the child": Newton and sort-compact on s.chd.  Returns its number of points.
template <typename T>
__device__ inline int reduce_child(const LaneSlice<T>& s, int m, int d) {
  newton_game(s.chd, m, d, (T)-1, kListFlags);
  sort_compact_game(s.chd, m, d, (T)-1, s.row);
  return num_points(s.chd, m, d);
}

// The child that the agent's axis `ax` makes of the game in s.par, written to s.chd, all in list semantics: shift,
// the inexact test, reduce.  Returns the child's number of points.  The test is note_inexact's loop written out: as a
// call it flips the sense of the loop's exit compare in hk_search_depth and hk_search_game_tree, whose code is pinned.
template <typename T>
__device__ inline int expand_child(const LaneSlice<T>& s, int m, int d, int ax, bool& inexact) {
  shift_child(s, m, d, ax);
  for (int i = 0; i < m; ++i) inexact |= s.chd[i * d + ax] >= kExactLimit<T>;
  return reduce_child(s, m, d);
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
