// The deterministic hosts of hironaka/host.py beyond Zeillinger, on one game in list semantics (ListPoints): a row is
// a point when p[i*d] >= 0 (the availability test of zeillinger_list_game: a NaN coordinate 0 is a hole), rows are
// read in row order and holes may sit anywhere.  Each routine returns the class id (encode_mask) of the host's subset,
// or -1 for "no subset".  Runtime m and d; d <= 6 for the hitting-set hosts (their support bitmap has 2^d bits), d = 7
// with the two-word bitmap that hk_search_morin_tree alone uses.
//
//   zeillinger_list_pair      Zeillinger / ZeillingerLex as ordered pairs (hk_search_game_tree's child order)
//   zeillinger_lex_list_game  ZeillingerLex      host.py:116-127  (Zeillinger's key, ties broken lexicographically)
//   weak_spivakovsky_game     WeakSpivakovsky    host.py:357-378  (a minimal hitting set, first in combinations order)
//   min_hitting_game          WeakSpivakovskyMinHitting  host.py:381-427  (a minimal hitting set, smallest integer)
//
//   host_class_game<T, HOST>  any fixed host, chosen at compile time (zeillinger_list_game for Zeillinger)
//
// -1 cases: fewer than 2 points (every host here; the reference returns []), and for the hitting-set hosts a zero row,
// whose empty support no subset meets.  WeakSpivakovsky also gives -1 when the union U of the supports has fewer than
// 2 coordinates.  The reference misbehaves on these inputs: WeakSpivakovsky appends no subset for that game, and
// WeakSpivakovskyMinHitting decodes its sentinel 65536 (coordinate 16) for a zero row.  No Newton-reduced state with
// >= 2 points has a zero row or |U| < 2.  WeakSpivakovskyMinHitting is well defined at |U| = 1 (the lone coordinate and
// the smallest other one) and returns that.
#pragma once

#include <type_traits>

#include "hk_game_generic.h"

namespace hk {

// The ordered lists of Zeillinger (LEX false, host.py:90-95) and ZeillingerLex (LEX true, host.py:116-127) over
// Zeillinger._select_coord's pairs (host.py:70-89): pairs i<j of the points in row order, v = P_i - P_j, key (L, S) as
// in zeillinger_list_game.  Each pair has r = [first argmin v, first argmax v] ([0, 1] if they coincide), packed as
// r[0] * 8 + r[1].  Zeillinger takes the first pair of the smallest key; ZeillingerLex takes, among the pairs of the
// smallest key, the lexicographically smallest r (the orientation P_i - P_j matters, not just the unordered pair).  One
// pass: a strictly smaller key restarts the candidate, an equal key keeps the smaller r.  Returns r, -1 for fewer than
// 2 points.  For LEX false the pair is chosen exactly as in zeillinger_list_game, which the rollout kernels use.
template <typename T, bool LEX>
__device__ inline int zeillinger_list_pair(const T* p, int m, int d) {
  T bestL = (T)0;
  int bestS = 0, bestR = -1;
  for (int i = 0; i < m; ++i) {
    if (!(p[i * d] >= (T)0)) continue;
    for (int j = i + 1; j < m; ++j) {
      if (!(p[j * d] >= (T)0)) continue;
      T mx = p[i * d] - p[j * d], mn = mx;
      int lo = 0, hi = 0;
      for (int k = 1; k < d; ++k) {
        const T v = p[i * d + k] - p[j * d + k];
        if (v < mn) { mn = v; lo = k; }
        if (v > mx) { mx = v; hi = k; }
      }
      int cnt = 0;
      for (int k = 0; k < d; ++k) {
        const T v = p[i * d + k] - p[j * d + k];
        cnt += (v == mx) + (v == mn);
      }
      const T L = mx - mn;
      const int r = lo == hi ? 1 : lo * 8 + hi;  // [0, 1] when argmin == argmax
      if (bestR < 0 || L < bestL || (L == bestL && cnt < bestS)) {
        bestL = L;
        bestS = cnt;
        bestR = r;
      } else if (LEX && L == bestL && cnt == bestS && r < bestR) {
        bestR = r;
      }
    }
  }
  return bestR;
}

// ZeillingerLex._get_coord (host.py:116-127): the class id of the pair zeillinger_list_pair<T, true> picks
template <typename T>
__device__ inline int zeillinger_lex_list_game(const T* p, int m, int d) {
  const int r = zeillinger_list_pair<T, true>(p, m, d);
  return r < 0 ? -1 : encode_mask((1u << (r >> 3)) | (1u << (r & 7)));
}

// The hitting-set hosts keep one bit per possible support: 2^d bits.  uint64_t serves d <= 6; Bits128 is the two-word
// form for d = 7, which only hk_search_morin_tree instantiates.  The bm_* helpers are all the hosts need of either.
struct Bits128 {
  uint64_t lo, hi;
};

__device__ inline uint64_t bm_one(uint64_t) { return 1ull; }
__device__ inline Bits128 bm_one(Bits128) { return Bits128{1ull, 0ull}; }
__device__ inline void bm_set(uint64_t& b, uint32_t s) { b |= 1ull << s; }
__device__ inline void bm_set(Bits128& b, uint32_t s) {
  if (s < 64u) b.lo |= 1ull << s;
  else b.hi |= 1ull << (s - 64u);
}
__device__ inline bool bm_test(uint64_t b, uint32_t s) { return ((b >> s) & 1ull) != 0; }
__device__ inline bool bm_test(const Bits128& b, uint32_t s) {
  return (((s < 64u ? b.lo : b.hi) >> (s & 63u)) & 1ull) != 0;
}
// b | (b << n), n a power of two: 1..32 for one word, 1..64 for two
__device__ inline uint64_t bm_or_shl(uint64_t b, uint32_t n) { return b | (b << n); }
__device__ inline Bits128 bm_or_shl(const Bits128& b, uint32_t n) {
  if (n >= 64u) return Bits128{b.lo, b.hi | b.lo};
  return Bits128{b.lo | (b.lo << n), b.hi | (b.hi << n) | (b.lo >> (64u - n))};
}
__device__ inline bool bm_disjoint(uint64_t a, uint64_t b) { return (a & b) == 0; }
__device__ inline bool bm_disjoint(const Bits128& a, const Bits128& b) { return ((a.lo & b.lo) | (a.hi & b.hi)) == 0; }
template <typename B>
struct bm_log2 {
  static constexpr int value = 6;
};
template <>
struct bm_log2<Bits128> {
  static constexpr int value = 7;
};

// Which supports occur: bit s of the result is set when some point's set of nonzero coordinates is s (x != 0: NaN
// counts as nonzero and -0.0 as zero, as np.nonzero does).  d <= 6 (B = uint64_t) or d <= 7 (Bits128).  `npts` receives
// the number of points.
template <typename T, typename B = uint64_t>
__device__ inline B support_bitmap(const T* p, int m, int d, int& npts) {
  B occ{};
  int n = 0;
  for (int i = 0; i < m; ++i) {
    if (!(p[i * d] >= (T)0)) continue;
    uint32_t s = 0;
    for (int k = 0; k < d; ++k) s |= (p[i * d + k] != (T)0) ? (1u << k) : 0u;
    bm_set(occ, s);
    ++n;
  }
  npts = n;
  return occ;
}

// bit s set for every s that is a subset of x (x < 2^6, or 2^7 for Bits128): the supports a candidate with complement x
// misses
template <typename B = uint64_t>
__device__ inline B subsets_of(uint32_t x) {
  B b = bm_one(B{});  // {empty set}
  for (int k = 0; k < bm_log2<B>::value; ++k)
    if ((x >> k) & 1u) b = bm_or_shl(b, 1u << k);
  return b;
}

// c meets every occurring support: no support lies inside the complement of c
template <typename B>
__device__ inline bool hits_all(const B& occ, uint32_t c, uint32_t full) {
  return bm_disjoint(occ, subsets_of<B>(full & ~c));
}

// WeakSpivakovsky._select_coord (host.py:357-378): U = the union of the supports; candidates are the c within U with
// |c| >= 2 that meet every support.  combinations(U, i) runs over sorted coordinate tuples in lexicographic order, so
// the host takes the smallest |c|, then the lexicographically first tuple: for equal sizes, the largest bit-reversed c.
template <typename T, typename B = uint64_t>
__device__ inline int weak_spivakovsky_game(const T* p, int m, int d) {
  int npts;
  const B occ = support_bitmap<T, B>(p, m, d, npts);
  if (npts < 2) return -1;
  const uint32_t full = (1u << d) - 1u;
  uint32_t U = 0;
  for (uint32_t s = 0; s <= full; ++s) U |= bm_test(occ, s) ? s : 0u;
  int best = -1, bestPc = 0;
  uint32_t bestRev = 0;
  for (uint32_t c = 3; c <= full; ++c) {
    if ((c & ~U) != 0) continue;
    const int pc = __popc(c);
    if (pc < 2 || !hits_all(occ, c, full)) continue;
    const uint32_t rev = __brev(c);  // the order among equal sizes only: the shift by 32 - d is common to all
    if (best < 0 || pc < bestPc || (pc == bestPc && rev > bestRev)) {
      best = (int)c;
      bestPc = pc;
      bestRev = rev;
    }
  }
  return best < 0 ? -1 : encode_mask((uint32_t)best);
}

// WeakSpivakovskyMinHitting._select_coord (host.py:381-427): candidates are all c with |c| >= 2 that meet every
// support; subset_route orders them by (|c|, c).  The reference's masks have 16 bits: a bit >= d meets no support, so
// the first hit lies within the d coordinates.
template <typename T, typename B = uint64_t>
__device__ inline int min_hitting_game(const T* p, int m, int d) {
  int npts;
  const B occ = support_bitmap<T, B>(p, m, d, npts);
  if (npts < 2) return -1;
  const uint32_t full = (1u << d) - 1u;
  int best = -1, bestPc = 0;
  for (uint32_t c = 3; c <= full; ++c) {
    const int pc = __popc(c);
    if (pc < 2 || (best >= 0 && pc >= bestPc) || !hits_all(occ, c, full)) continue;
    best = (int)c;  // ascending c: the first hit of a size is the smallest of that size
    bestPc = pc;
  }
  return best < 0 ? -1 : encode_mask((uint32_t)best);
}

// the class id a fixed host (HOST: HK_HOST_ALL_COORD .. HK_HOST_MIN_HITTING) picks on one game in list semantics
// (B: the support bitmap of the hitting-set hosts, uint64_t for d <= 6)
template <typename T, int HOST, typename B = uint64_t>
__device__ inline int host_class_game(const T* p, int m, int d) {
  if (HOST == HK_HOST_ALL_COORD) return encode_mask((1u << d) - 1u);
  if (HOST == HK_HOST_ZEILLINGER) return zeillinger_list_game(p, m, d);
  if (HOST == HK_HOST_ZEILLINGER_LEX) return zeillinger_lex_list_game(p, m, d);
  if (HOST == HK_HOST_WEAK_SPIVAKOVSKY) return weak_spivakovsky_game<T, B>(p, m, d);
  return min_hitting_game<T, B>(p, m, d);
}

// ---- host side of the fixed-host operators (hk_host_select, hk_search_depth, hk_search_game_tree) -------------------
// Shapes they accept: the hitting-set hosts keep one bit per possible support (2^6 bits), and hk_search_game_tree
// packs a node's host list 3 bits per axis into one word.
constexpr int kFixedHostMaxPoints = 64;
constexpr int kFixedHostMaxDim = 6;

inline bool fixed_host(int host) { return host >= HK_HOST_ALL_COORD && host <= HK_HOST_MIN_HITTING; }

// f(T(), std::integral_constant<int, HOST>()) for the element type of dtype (HK_F32 -> float, else double) and a fixed
// host; HK_ERR_UNSUPPORTED for any other host
template <typename F>
int with_fixed_host(int dtype, int host, F&& f) {
  auto on = [&](auto t) -> int {
    switch (host) {
      case HK_HOST_ALL_COORD: return f(t, std::integral_constant<int, HK_HOST_ALL_COORD>());
      case HK_HOST_ZEILLINGER: return f(t, std::integral_constant<int, HK_HOST_ZEILLINGER>());
      case HK_HOST_ZEILLINGER_LEX: return f(t, std::integral_constant<int, HK_HOST_ZEILLINGER_LEX>());
      case HK_HOST_WEAK_SPIVAKOVSKY: return f(t, std::integral_constant<int, HK_HOST_WEAK_SPIVAKOVSKY>());
      case HK_HOST_MIN_HITTING: return f(t, std::integral_constant<int, HK_HOST_MIN_HITTING>());
    }
    return HK_ERR_UNSUPPORTED;
  };
  return dtype == HK_F32 ? on(float()) : on(double());
}

}  // namespace hk
