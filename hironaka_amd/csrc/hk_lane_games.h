// The frame of the one-game-per-lane operators: hk_host_select, hk_search_morin_play, hk_game_play, hk_env_step and
// hk_tree_expand (and the Morin tree search, whose lanes expand nodes the same way).
//
// A workgroup is one wave that owns `games_per_block` consecutive games: as many as have slices in kSearchLdsBytes, at
// most a wave (lane_geometry, hk_search_wave.h).  The wave stages their records with the coalesced slab copy of the
// generic kernel (stage_games), kLaneGameBatch loads per lane in flight, into LDS slices of an odd stride, so that lane
// g walks its own game conflict-free.  Lane g then works on game g alone in its slice with the per-game routines of
// hk_game_generic.h, hk_hosts.h and hk_search_wave.h, and the wave copies the result out the same way (unstage_games).
// A slice is search_lds_stride's LaneSlice -- parent, child, the shift coefficients, sort_compact's row scratch, then
// what a kernel keeps for itself -- unless a kernel says otherwise.  A move is "shift the child", what the game puts in
// between, "reduce the child" (hk_search_wave.h); the parent and child halves swap roles from move to move.  No
// communication between workgroups; every loop of a lane is bounded by the sizes in its argument block.
//
// Here: the block prologue and the staging, the helpers of a move, the Morin child, the moves a game is given and
// leaves (hk_game_play and hk_search_morin_play), and the choice of instantiation the C entries share (their record
// buffers are judged by span_bytes and overlap, hk_common.h).
#pragma once

#include "hk_generic_kernel.h"
#include "hk_hosts.h"
#include "hk_search_wave.h"

namespace hk {

constexpr int kLaneGameBatch = 16;  // loads per lane in flight while staging
constexpr int kLaneGameMaxDim = 7;  // the hitting-set hosts run on the two-word support bitmap (Bits128) there
constexpr int kLaneHostForced = -1;  // HOST of a launch whose every class is forced
static_assert(HK_PLAY_HOST_FORCED == kLaneHostForced && HK_MORIN_HOST_FORCED == kLaneHostForced, "one forced code");
static_assert(HK_PLAY_NO_MOVE == HK_MORIN_NO_MOVE, "forced_or_host_move's callers share the outcome of its refusal");

// ---- the block ------------------------------------------------------------------------------------------------------
// the first game of this workgroup and how many it has
struct LaneBlock {
  int64_t g0;
  int ngames;
};
__device__ inline LaneBlock lane_block(int batch, int games_per_block) {
  const int64_t g0 = (int64_t)blockIdx.x * games_per_block;
  const int64_t left = (int64_t)batch - g0;
  return {g0, left < games_per_block ? (int)left : games_per_block};
}

// the wave copies the first n elements of the block's records (stride elements apart) into the lanes' slices / back
template <typename T>
__device__ inline void stage_games(T* lds, const void* src, int64_t stride, int n, int lds_stride, const LaneBlock& b,
                                   int lane) {
  copy_slab<T, true, kLaneGameBatch>(lds, const_cast<T*>(static_cast<const T*>(src)), stride, n, lds_stride, b.g0,
                                     b.ngames, lane);
}
template <typename T>
__device__ inline void unstage_games(T* lds, void* dst, int64_t stride, int n, int lds_stride, const LaneBlock& b,
                                     int lane) {
  copy_slab<T, false, kLaneGameBatch>(lds, static_cast<T*>(dst), stride, n, lds_stride, b.g0, b.ngames, lane);
}

// ---- the helpers of a move ------------------------------------------------------------------------------------------
// the class the fixed host HOST picks for the game p, at any dimension up to kLaneGameMaxDim
template <typename T, int HOST>
__device__ inline int host_class_any(const T* p, int m, int d) {
  return d < kLaneGameMaxDim ? host_class_game<T, HOST, uint64_t>(p, m, d) : host_class_game<T, HOST, Bits128>(p, m, d);
}

// the shift coefficients of the subset sub
template <typename T>
__device__ inline void subset_coeffs(T* c, uint32_t sub, int d) {
  for (int j = 0; j < d; ++j) c[j] = ((sub >> j) & 1u) ? (T)1 : (T)0;
}

// the k-th set bit of sub (k < popcount)
__device__ inline int nth_bit(uint32_t sub, int k) {
  for (int j = 0; j < k; ++j) sub &= sub - 1u;
  return __ffs((int)sub) - 1;
}

// a coordinate of sub drawn uniformly (agent.py:89-90) from the Philox block (game, counter, stream) under seed
__device__ inline int random_legal_axis(uint32_t sub, uint64_t game, uint32_t counter, uint32_t stream, uint64_t seed) {
  const U4 r = philox4x32((uint32_t)game, (uint32_t)(game >> 32), counter, stream, seed);
  return nth_bit(sub, (int)mulhi32(r.x, (uint32_t)__popc(sub)));
}

// whether a coordinate of a point of p exceeds thr (ListPoints.exceed_threshold, core/list_points.py:60-70)
template <typename T>
__device__ inline bool exceeds_game(const T* p, int m, int d, double thr) {
  bool over = false;
  for (int i = 0; i < m; ++i) {
    if (!(p[i * d] >= (T)0)) continue;
    for (int k = 0; k < d; ++k) over |= (double)p[i * d + k] > thr;
  }
  return over;
}

// the position of the row `prow` among the first np rows of p, -1 when it is not there
template <typename T>
__device__ inline int find_row(const T* p, const T* prow, int np, int d) {
  int at = -1;
  for (int i = 0; i < np; ++i) {
    bool same = true;
    for (int k = 0; k < d; ++k) same &= p[i * d + k] == prow[k];
    if (same) at = i;
  }
  return at;
}

// whether a live row of p other than row `at` has q_k <= prow_k for all k: Newton then removes prow, the copy of row
// `at` (an identical row counts: the reference marks the row, the marked one sorts before its twin and is removed)
template <typename T>
__device__ inline bool row_contained(const T* p, int m, int d, int at, const T* prow) {
  bool lost = false;
  for (int q = 0; q < m; ++q) {
    if (q == at || !(p[q * d] >= (T)0)) continue;
    bool below = true;
    for (int k = 0; k < d; ++k) below &= p[q * d + k] <= prow[k];
    lost |= below;
  }
  return lost;
}

// ---- the Morin child --------------------------------------------------------------------------------------------------
// LDS elements per lane behind LaneSlice::row: d weights (int32, one per element) and the row p.  Indexed at run time,
// they would land in scratch as register arrays.
inline int morin_lds_extra(int d) { return 2 * d; }

// One Morin child of the game in s.par whose distinguished row is `pd`: the state goes to s.chd as expand_child's does,
// with the reposition between shift and reduce.  prow: d elements of scratch for the row p.  Returns the number of
// points; `dist` receives p's position in the child, -1 when it was lost.
template <typename T>
__device__ inline int expand_morin_child(const LaneSlice<T>& s, T* prow, int m, int d, int ax, int pd, bool& inexact,
                                         int& dist) {
  shift_child(s, m, d, ax);
  note_inexact(s, m, d, ax, inexact);
  reposition_game(s.chd, m, d, (T)-1, kListFlags);
  for (int k = 0; k < d; ++k) prow[k] = s.chd[pd * d + k];
  const bool lost = row_contained(s.chd, m, d, pd, prow);
  const int np = reduce_child(s, m, d);
  dist = lost ? -1 : find_row(s.chd, prow, np, d);
  return np;
}

// ---- the moves a game is given and the moves it leaves (hk_game_play, hk_search_morin_play) ----------------------------
struct MoveRecords {
  const int32_t *class_in, *axis_in;  // [batch, steps] or NULL: entries < 0 leave the move to the host / the agent
  int32_t *class_out, *axis_out;      // [batch, steps] or NULL
  int steps;
};

// Move t of game g, whose state is p.  cls: the forced class, else the one the fixed host HOST picks (kLaneHostForced:
// none); sub: its subset; ax: the forced axis, -1 where the agent is to choose.  false: no move -- no class, or a
// forced axis outside the subset.
template <typename T, int HOST>
__device__ inline bool forced_or_host_move(const MoveRecords& r, int64_t g, int t, const T* p, int m, int d, int& cls,
                                           uint32_t& sub, int& ax) {
  cls = r.class_in ? r.class_in[g * r.steps + t] : -1;
  if (cls < 0 && HOST != kLaneHostForced) cls = host_class_any<T, HOST>(p, m, d);
  if (cls < 0 || cls >= (1 << d) - d - 1) return false;
  sub = decode_class(cls, d);
  ax = r.axis_in ? r.axis_in[g * r.steps + t] : -1;
  return ax < 0 || (ax < d && ((sub >> ax) & 1u));
}

__device__ inline void record_move(const MoveRecords& r, int64_t g, int t, int cls, int ax) {
  if (r.class_out) r.class_out[g * r.steps + t] = cls;
  if (r.axis_out) r.axis_out[g * r.steps + t] = ax;
}

// What a lane does once its game is over after `len` moves: -1 behind the recorded moves, and the final state, which
// sits in s.par, copied to the parent half of its slice `home` when the halves ended up swapped.
template <typename T>
__device__ inline void finish_game(const MoveRecords& r, int64_t g, int len, const LaneSlice<T>& home,
                                   const LaneSlice<T>& s, int n) {
  for (int t = len; t < r.steps; ++t) record_move(r, g, t, -1, -1);
  if (s.par != home.par)
    for (int e = 0; e < n; ++e) home.par[e] = s.par[e];
}

// ---- the choice of instantiation the C entries share -----------------------------------------------------------------
// with_fixed_host for "a fixed host, or this one extra code": f(T(), other) when host is other's value
// (HK_PLAY_HOST_FORCED, HK_MORIN_HOST_FORCED, or 0 for the environments' agent mode)
template <int OTHER, typename F>
int with_fixed_host_or(int dtype, int host, std::integral_constant<int, OTHER> other, F&& f) {
  if (host == OTHER) return dtype == HK_F32 ? f(float(), other) : f(double(), other);
  return with_fixed_host(dtype, host, f);
}

}  // namespace hk
