// The two remaining hosts of hironaka/host.py on one game in list semantics (a row is a point when its coordinate 0
// is >= 0, rows are read in row order, holes may sit anywhere), as hk_hosts.h has the others.  Both return the host's
// subset as a bit mask (bit k <-> coordinate k), not as a class id: Spivakovsky's subset may hold 0 or 1 coordinates.
//
//   spivakovsky_game         Spivakovsky        host.py:130-290  (the host the game was solved with)
//   random_spivakovsky_game  RandomSpivakovsky  host.py:293-354  (a minimal hitting set of >= 2 coordinates, drawn
//                                                                 uniformly)
//
// Both give 0 for fewer than 2 points.  Plain C++ with __popc and __brev only, so that the header also builds for the
// host (tests/spivakovsky_routines.hip).
#pragma once

#include <limits>

#include "hk_hosts.h"

namespace hk {

constexpr int kSpivakovskyMaxDim = 6;      // the loops over coordinates unroll to it: mn and q stay in registers
constexpr double kSpivakovskyOne = 0.999;  // the reference's "reaches 1" (host.py:215, 258)

// Spivakovsky._select_coord (host.py:223-290) on the game's double copy w (m rows of d doubles, d <= 6), which it
// uses as its work space: the rows never move, so the projections of a level overwrite the coordinates that stay
// active.  Python's floats are doubles and its sum() runs left to right (CPython 3.10); so do the sums here, and the
// two divisions of a level are IEEE divisions.
//
// act: the active coordinates (the reference's coord_dict), alive: the rows left (its pts); both only shrink and both
// are walked in ascending order, the reference's.  A level (host.py:235-279): mn = the minimum of every active
// coordinate over alive, mv = v - mn the moved point.  A row with mv == 0 on all of act ends the levels.  Otherwise md
// = the smallest coordinate sum of a moved row, S = the active coordinates that are > 0 in a row of that sum; S joins
// the result, I = act \ S.  With q = mv / md and t = the sum of q over S, a row stays alive when t < 0.999, and its
// coordinates in I become q / (1 - t).  The last step (host.py:186-221) runs on what is alive after the levels, on
// the values as they stand (not the moved ones): the first subset of 1 .. |act| - 1 active coordinates, by size and
// then in itertools.combinations order, on which every alive row sums to >= 0.999 (in the reference's words, not
// < 0.999) joins the result; the full set is never tried.  Among equal sizes combinations order is the descending
// order of the bit-reversed mask (hk_hosts.h, weak_spivakovsky_game).
//
// The levels are capped at d: on finite, non-negative rows S is non-empty at every level, so the cap is never met; on
// anything else it ends the loop.  Every access is to w[i * d + k] with i < m and k < d.
__device__ inline uint32_t spivakovsky_game(double* w, int m, int d) {
  uint64_t alive = 0;
  int npts = 0;
  for (int i = 0; i < m; ++i)
    if (w[i * d] >= 0.0) {
      alive |= 1ull << i;
      ++npts;
    }
  if (npts < 2) return 0u;
  uint32_t act = (1u << d) - 1u, res = 0u;
  for (int level = 0; level < d && alive != 0; ++level) {
    double mn[kSpivakovskyMaxDim];
    bool first = true;
    for (int i = 0; i < m; ++i) {
      if (!((alive >> i) & 1ull)) continue;
#pragma unroll
      for (int k = 0; k < kSpivakovskyMaxDim; ++k)
        if (k < d) {
          const double v = w[i * d + k];
          if (first || v < mn[k]) mn[k] = v;
        }
      first = false;
    }
    double md = std::numeric_limits<double>::infinity();
    uint32_t S = 0;
    bool zero_row = false;
    for (int i = 0; i < m; ++i) {
      if (!((alive >> i) & 1ull)) continue;
      double s = 0.0;
      uint32_t pos = 0;
      bool zero = true;
#pragma unroll
      for (int k = 0; k < kSpivakovskyMaxDim; ++k)
        if (k < d && ((act >> k) & 1u)) {
          const double mv = w[i * d + k] - mn[k];
          s += mv;
          pos |= mv > 0.0 ? (1u << k) : 0u;
          zero &= mv == 0.0;
        }
      zero_row |= zero;
      if (s < md) {
        md = s;
        S = 0;
      }
      if (s == md) S |= pos;
    }
    if (zero_row) break;
    res |= S;
    const uint32_t I = act & ~S;
    for (int i = 0; i < m; ++i) {
      if (!((alive >> i) & 1ull)) continue;
      double q[kSpivakovskyMaxDim];
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < kSpivakovskyMaxDim; ++k)
        if (k < d && ((act >> k) & 1u)) {
          q[k] = (w[i * d + k] - mn[k]) / md;
          if ((S >> k) & 1u) t += q[k];
        }
      if (t < kSpivakovskyOne) {
        const double scale = 1.0 - t;
#pragma unroll
        for (int k = 0; k < kSpivakovskyMaxDim; ++k)
          if (k < d && ((I >> k) & 1u)) w[i * d + k] = q[k] / scale;
      } else {
        alive &= ~(1ull << i);
      }
    }
    if (I != 0) act = I;
  }
  if (alive == 0) return res;
  const int nact = __popc(act);
  uint32_t best = 0, bestRev = 0;
  int bestPc = 0;
  for (uint32_t c = 1; c < (1u << d); ++c) {
    if ((c & ~act) != 0) continue;
    const int pc = __popc(c);
    const uint32_t rev = __brev(c);
    if (pc >= nact || (best != 0 && (pc > bestPc || (pc == bestPc && rev < bestRev)))) continue;
    bool permissible = true;
    for (int i = 0; i < m; ++i) {
      if (!((alive >> i) & 1ull)) continue;
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < kSpivakovskyMaxDim; ++k)
        if (k < d && ((c >> k) & 1u)) s += w[i * d + k];
      permissible &= !(s < kSpivakovskyOne);
    }
    if (permissible) {
      best = c;
      bestPc = pc;
      bestRev = rev;
    }
  }
  return res | best;
}

// RandomSpivakovsky._select_coord (host.py:307-354) built with dim = d: the candidates are the c with |c| >= 2 that
// meet every support (support_bitmap: x != 0), of the smallest such size, in ascending integer order (subset_route's);
// the host draws one uniformly.  Here: candidate number mulhi32(word, n) of the n, word = the first word of the Philox
// block (game, step, kStreamRandomSpivakovsky) under seed.  0 when nothing meets every support (a zero row), where the
// reference raises from randint(0, -1).
template <typename T, typename B = uint64_t>
__device__ inline uint32_t random_spivakovsky_game(const T* p, int m, int d, uint64_t game, uint32_t step,
                                                   uint64_t seed) {
  int npts;
  const B occ = support_bitmap<T, B>(p, m, d, npts);
  if (npts < 2) return 0u;
  const uint32_t full = (1u << d) - 1u;
  int size = 0;
  uint32_t n = 0;
  for (uint32_t c = 3; c <= full; ++c) {
    const int pc = __popc(c);
    if (pc < 2 || (n != 0 && pc > size) || !hits_all(occ, c, full)) continue;
    n = (n == 0 || pc < size) ? 1u : n + 1u;
    size = pc;
  }
  if (n == 0) return 0u;
  const U4 r = philox4x32((uint32_t)game, (uint32_t)(game >> 32), step, kStreamRandomSpivakovsky, seed);
  uint32_t left = mulhi32(r.x, n), pick = 0;
  for (uint32_t c = 3; c <= full; ++c) {
    if (__popc(c) != size || !hits_all(occ, c, full)) continue;
    if (left == 0) {
      pick = c;
      break;
    }
    --left;
  }
  return pick;
}

}  // namespace hk
