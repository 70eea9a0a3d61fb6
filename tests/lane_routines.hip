// The per-game routines of the one-game-per-lane operators, built for the host: a stand-alone program over
// hk_game_generic.h, hk_hosts.h, hk_search_wave.h, hk_lane_games.h and the lane bodies of hk_game_play_kernel.h and
// hk_env_step_kernel.h (no library, no device).  tests/test_lane_routines.py compiles it twice -- with AddressSanitizer
// and UndefinedBehaviorSanitizer, and with the library's own host-relevant flags -- and compares what it computes with
// the oracle and the rules, bit for bit.  For this translation unit alone `__device__` means host and device, and the
// five intrinsics the routines use (__popc, __brev, __ffs, __clz, __umulhi) have host stand-ins below.
//
// Every game of a case file runs 2 x 4 times:
//   * two memory layouts.  "exact": every pointer a routine receives (par, chd, c, row, the Morin extra, each move
//     record, length and outcome) is its own heap allocation of exactly the documented length, so that an overrun by
//     one element lands in a redzone.  "production": three adjacent slices built by LaneSlice / EnvSlice with
//     search_lds_stride / env_lds_stride / morin_lds_extra, the game in the middle one; both neighbours, the stride's
//     spare element and the neighbouring games' records hold a canary that is checked after the routine returns;
//   * four fills of everything that is not an input of the routine: a quiet NaN, a large finite value, the pad -1 and 0.
// The results of all eight runs must be identical bit for bit; those of the first are written out.  A fill-dependent
// result or a touched canary is reported on stderr and makes the exit status 1; a sanitizer report aborts.
//
// usage: lane_routines CASES RESULTS
//
// CASES (binary, little-endian, no padding):
//   char[4] "HKLR", int32 version (1), int32 blocks, then per block
//     int32  routine, dtype (0 float, 1 double), m, d
//     uint32 flags                      HK_SEM_* | HK_FLAG_* of the hk_game_generic.h routines
//     int32  count                      games in the block
//     int32  nTi, nIi, nDi              inputs per game: elements of the dtype, int32, float64
//     int32  nTo, nIo, nDo              results per game, likewise
//     int32  ipar[8]; float64 dpar[4]   per-routine parameters (the table below)
//     T[count * nTi], int32[count * nIi], float64[count * nDi]    the packed inputs, game after game
// RESULTS: per block T[count * nTo], int32[count * nIo], float64[count * nDo].
// The program derives the six lengths from the routine itself and refuses a block whose header disagrees.
//
// Routines (n = m * d; S = ipar[1], the length of a move record; u64 values travel as two int32: low, high):
//  id routine              ipar / dpar                 T in            int32 in                 results
//   1 num_points                                       p[n]                                     I: count
//   2 stages_game          0 stages  d0 pad            p[n] (+c[d] if  axis                     T: p[n]
//                                                      SHIFT is set)
//   3 rescale_game         d0 pad                      p[n]                                     T: p[n]
//   4 zeillinger           0: 0 _game, 1 _list_game    p[n]                                     I: class
//   5 feature_sort_game    0 coord0                    p[n]                                     T: p[n]
//   6 zeillinger_list_pair 0 LEX                       p[n]                                     I: r
//   7 host_class_game      0 HOST, 1: 1 for Bits128    p[n]                                     I: class
//   8 shift_child                                      par[n] c[d]     ax                       T: chd[n] par[n]
//   9 note_inexact                                     chd[n]          ax, inexact on entry     I: inexact
//  10 reduce_child                                     chd[n]                                   T: chd[n]  I: np
//  11 expand_child                                     par[n] c[d]     ax                       T: chd[n]  I: np inexact
//  12 expand_morin_child                               par[n] c[d]     ax, pd                   T: chd[n]  I: np inexact dist
//  13 find_row                                         p[n] prow[d]    np                       I: position
//  14 row_contained                                    p[n] prow[d]    at                       I: lost
//  15 exceeds_game         (float64 in: thr)           p[n]                                     I: over
//  16 nth_bit                                                          sub, k                   I: bit
//  17 random_legal_axis                                                sub, game, counter,      I: axis
//                                                                      stream, seed
//  18 subset_coeffs                                                    sub                      T: c[d]
//  19 forced_or_host_move  0 HOST, 1 S, 2 bits: 1      p[n]            t, class_in[S],          I: moved cls sub ax
//                          class_in, 2 axis_in                         axis_in[S]                  (-9: left unset)
//  20 record_move          1 S, 2 bits: 4 class_out,                   t, cls, ax               I: class_out[S] axis_out[S]
//                          8 axis_out                                                              (-7 on entry; 0: absent)
//  21 finish_game          1 S, 2 bits as record_move  state[n]        len, halves swapped      T: home.par[n]
//                                                                                               I: class_out[S] axis_out[S]
//  22 play_lane            0 HOST (-1 forced), 1 S,    par[n]          class_in[S] axis_in[S]   T: par[n]  I: length outcome
//                          2 bits 1|2|4|8, 3 agent,                    game_offset seed            class_out[S] axis_out[S]
//                          4 HK_PLAY_* flags                           step_offset
//                          (float64 in: value_threshold)
//  23 env_move             0 reposition                p[n]            sub, ax                  T: p[n]
//  24 extent_game                                      p[n]                                     I: extent
//  25 env_fresh            0 max_value, 1 HK_ENV_*                     game, seed               T: p[n]  I: np
//  26 env_host_step        0 HOST, 1 HK_ENV_*          p[n]            action, class            T: p[n]  I: class stopped
//                          (float64 in: value_threshold, invalid_move_penalty)                     exceed  D: reward
//  27 env_agent_step       0 agent, 1 HK_ENV_*,        p[n]            mask, game, step count,  T: p[n]  I: axis stopped
//                          2 step_threshold                            agent_seed                  exceed  D: reward
//                          (float64 in: value_threshold, threshold_penalty)
// The two env steps run on the game's extent (extent_game), as env_step_kernel calls them.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))

namespace host_standins {
inline int popc(unsigned x) { return __builtin_popcount(x); }
inline unsigned brev(unsigned x) { return __builtin_bitreverse32(x); }
inline int ffs(int x) { return __builtin_ffs(x); }
inline int clz(int x) { return x == 0 ? 32 : __builtin_clz((unsigned)x); }  // the hardware's value at 0
inline unsigned umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
}  // namespace host_standins
#define __popc host_standins::popc
#define __brev host_standins::brev
#define __ffs host_standins::ffs
#define __clz host_standins::clz
#define __umulhi host_standins::umulhi

#include "hk_env_step_kernel.h"
#include "hk_game_play_kernel.h"

using namespace hk;

namespace {

enum Routine : int {
  kNumPoints = 1, kStages, kRescale, kZeillinger, kFeatureSort, kListPair, kHostClass, kShiftChild, kNoteInexact,
  kReduceChild, kExpandChild, kExpandMorin, kFindRow, kRowContained, kExceeds, kNthBit, kRandomAxis, kSubsetCoeffs,
  kForcedOrHost, kRecordMove, kFinishGame, kPlayLane, kEnvMove, kExtent, kEnvFresh, kEnvHostStep, kEnvAgentStep,
  kRoutineEnd
};

struct Header {
  int32_t routine, dtype, m, d;
  uint32_t flags;
  int32_t count, nTi, nIi, nDi, nTo, nIo, nDo;
  int32_t ipar[8];
  double dpar[4];
};
static_assert(sizeof(Header) == 20 * 4 + 4 * 8, "the header is packed");

int failures = 0;

void fail(const Header& h, int game, int layout, int fill, const char* what) {
  if (++failures <= 20)
    fprintf(stderr, "FAILED routine %d dtype %d m %d d %d game %d layout %s fill %d: %s\n", h.routine, h.dtype, h.m,
            h.d, game, layout ? "production" : "exact", fill, what);
}

bool env_routine(int r) { return r >= kEnvMove && r <= kEnvAgentStep; }
bool morin_routine(int r) { return r == kExpandMorin || r == kFindRow || r == kRowContained; }
int record_len(const Header& h) { return h.routine >= kForcedOrHost && h.routine <= kPlayLane ? h.ipar[1] : 0; }

// the per-game lengths a routine takes and gives: {nTi, nIi, nDi, nTo, nIo, nDo}
struct Lengths {
  int v[6];
};
Lengths lengths(const Header& h) {
  const int d = h.d, n = h.m * h.d, S = record_len(h);
  switch (h.routine) {
    case kNumPoints: return {{n, 0, 0, 0, 1, 0}};
    case kStages: return {{n + ((h.ipar[0] & HK_STAGE_SHIFT) ? d : 0), 1, 0, n, 0, 0}};
    case kRescale: return {{n, 0, 0, n, 0, 0}};
    case kZeillinger: return {{n, 0, 0, 0, 1, 0}};
    case kFeatureSort: return {{n, 0, 0, n, 0, 0}};
    case kListPair: return {{n, 0, 0, 0, 1, 0}};
    case kHostClass: return {{n, 0, 0, 0, 1, 0}};
    case kShiftChild: return {{n + d, 1, 0, 2 * n, 0, 0}};
    case kNoteInexact: return {{n, 2, 0, 0, 1, 0}};
    case kReduceChild: return {{n, 0, 0, n, 1, 0}};
    case kExpandChild: return {{n + d, 1, 0, n, 2, 0}};
    case kExpandMorin: return {{n + d, 2, 0, n, 3, 0}};
    case kFindRow: return {{n + d, 1, 0, 0, 1, 0}};
    case kRowContained: return {{n + d, 1, 0, 0, 1, 0}};
    case kExceeds: return {{n, 0, 1, 0, 1, 0}};
    case kNthBit: return {{0, 2, 0, 0, 1, 0}};
    case kRandomAxis: return {{0, 7, 0, 0, 1, 0}};
    case kSubsetCoeffs: return {{0, 1, 0, d, 0, 0}};
    case kForcedOrHost: return {{n, 1 + 2 * S, 0, 0, 4, 0}};
    case kRecordMove: return {{0, 3, 0, 0, 2 * S, 0}};
    case kFinishGame: return {{n, 2, 0, n, 2 * S, 0}};
    case kPlayLane: return {{n, 2 * S + 5, 1, n, 2 + 2 * S, 0}};
    case kEnvMove: return {{n, 2, 0, n, 0, 0}};
    case kExtent: return {{n, 0, 0, 0, 1, 0}};
    case kEnvFresh: return {{0, 4, 0, n, 1, 0}};
    case kEnvHostStep: return {{n, 2, 2, n, 3, 1}};
    case kEnvAgentStep: return {{n, 6, 2, n, 3, 1}};
  }
  return {{-1, -1, -1, -1, -1, -1}};
}

uint64_t u64_of(const int32_t* lo_hi) { return (uint64_t)(uint32_t)lo_hi[0] | ((uint64_t)(uint32_t)lo_hi[1] << 32); }

template <typename T>
T fill_value(int fill) {
  switch (fill) {
    case 0: return std::numeric_limits<T>::quiet_NaN();
    case 1: return (T)1e30;
    case 2: return (T)-1;
  }
  return (T)0;
}
int32_t fill_int(int fill) {
  const int32_t v[4] = {0x7FC00000, 1000000007, -1, 0};
  return v[fill];
}
constexpr int32_t kCanaryInt = 0x5A5A5A5A;
template <typename T>
T canary() {
  return (T)-7654321;
}

// the memory one game runs in, under either layout
template <typename T>
struct Frame {
  bool prod, env;
  int m, d, n, S, extra, stride, used;
  int64_t g;
  std::vector<void*> owned;
  T *lds = nullptr, *par, *chd = nullptr, *c, *row, *ext = nullptr;
  int32_t *rec[4], *len, *outc;  // class_in, axis_in, class_out, axis_out

  template <typename U>
  U* take(size_t count) {
    void* p = malloc(count * sizeof(U) ? count * sizeof(U) : 1);
    owned.push_back(p);
    return static_cast<U*>(p);
  }

  Frame(const Header& h, bool production)
      : prod(production), env(env_routine(h.routine)), m(h.m), d(h.d), n(h.m * h.d), S(record_len(h)),
        extra(morin_routine(h.routine) ? morin_lds_extra(h.d) : 0) {
    stride = env ? env_lds_stride(m, d) : search_lds_stride(m, d, extra);
    used = env ? n + 2 * d : 2 * n + 2 * d + extra;
    g = prod ? 1 : 0;
    const int games = prod ? 3 : 1;
    for (int k = 0; k < 4; ++k) rec[k] = take<int32_t>((size_t)games * S);
    len = take<int32_t>(games);
    outc = take<int32_t>(games);
    if (prod) {
      lds = take<T>((size_t)3 * stride);
      if (env) {
        const EnvSlice<T> s(lds, 1, stride, n, d);
        par = s.par, c = s.c, row = s.row;
      } else {
        const LaneSlice<T> s(lds, 1, stride, m, d);
        par = s.par, chd = s.chd, c = s.c, row = s.row;
        ext = extra ? row + d : nullptr;
      }
    } else {
      par = take<T>(n);
      if (!env) chd = take<T>(n);
      c = take<T>(d);
      row = take<T>(d);
      if (extra) ext = take<T>(extra);
    }
  }
  ~Frame() {
    for (void* p : owned) free(p);
  }
  Frame(const Frame&) = delete;

  // the slice as the kernels build it, then its members pointed at this frame's parts
  LaneSlice<T> lane_slice() const {
    LaneSlice<T> s(par, 0, stride, 0, 0);
    s.par = par, s.chd = chd, s.c = c, s.row = row;
    return s;
  }
  EnvSlice<T> env_slice() const {
    EnvSlice<T> s(par, 0, stride, 0, 0);
    s.par = par, s.c = c, s.row = row;
    return s;
  }

  void reset(int fill) {
    const T fv = fill_value<T>(fill);
    const int32_t fi = fill_int(fill);
    if (prod) {
      for (int e = 0; e < 3 * stride; ++e) lds[e] = canary<T>();
      for (int e = 0; e < used; ++e) par[e] = fv;
      for (int k = 0; k < 4; ++k)
        for (int e = 0; e < 3 * S; ++e) rec[k][e] = (e / (S ? S : 1) == 1) ? fi : kCanaryInt;
      for (int e = 0; e < 3; ++e) len[e] = outc[e] = e == 1 ? fi : kCanaryInt;
    } else {
      for (int e = 0; e < n; ++e) par[e] = fv;
      for (int e = 0; e < n && chd; ++e) chd[e] = fv;
      for (int e = 0; e < d; ++e) c[e] = row[e] = fv;
      for (int e = 0; e < extra; ++e) ext[e] = fv;
      for (int k = 0; k < 4; ++k)
        for (int e = 0; e < S; ++e) rec[k][e] = fi;
      len[0] = outc[0] = fi;
    }
  }
  bool canaries_intact() const {
    if (!prod) return true;
    const T cv = canary<T>();
    bool ok = true;
    for (int e = 0; e < 3 * stride; ++e)
      if (e < stride || e >= stride + used) ok &= memcmp(&lds[e], &cv, sizeof(T)) == 0;
    for (int k = 0; k < 4; ++k)
      for (int e = 0; e < 3 * S; ++e)
        if (e / S != 1) ok &= rec[k][e] == kCanaryInt;
    ok &= len[0] == kCanaryInt && len[2] == kCanaryInt && outc[0] == kCanaryInt && outc[2] == kCanaryInt;
    return ok;
  }
  int32_t* mine(int k) const { return rec[k] + g * S; }
};

template <typename T, typename B>
int host_class_of(int host, const T* p, int m, int d) {
  switch (host) {
    case HK_HOST_ALL_COORD: return host_class_game<T, HK_HOST_ALL_COORD, B>(p, m, d);
    case HK_HOST_ZEILLINGER: return host_class_game<T, HK_HOST_ZEILLINGER, B>(p, m, d);
    case HK_HOST_ZEILLINGER_LEX: return host_class_game<T, HK_HOST_ZEILLINGER_LEX, B>(p, m, d);
    case HK_HOST_WEAK_SPIVAKOVSKY: return host_class_game<T, HK_HOST_WEAK_SPIVAKOVSKY, B>(p, m, d);
    case HK_HOST_MIN_HITTING: return host_class_game<T, HK_HOST_MIN_HITTING, B>(p, m, d);
  }
  fprintf(stderr, "no host %d\n", host);
  exit(2);
}

// f(std::integral_constant<int, HOST>()) for a fixed host or kLaneHostForced
template <typename F>
void with_host(int host, F&& f) {
  switch (host) {
    case kLaneHostForced: return f(std::integral_constant<int, kLaneHostForced>());
    case HK_HOST_ALL_COORD: return f(std::integral_constant<int, HK_HOST_ALL_COORD>());
    case HK_HOST_ZEILLINGER: return f(std::integral_constant<int, HK_HOST_ZEILLINGER>());
    case HK_HOST_ZEILLINGER_LEX: return f(std::integral_constant<int, HK_HOST_ZEILLINGER_LEX>());
    case HK_HOST_WEAK_SPIVAKOVSKY: return f(std::integral_constant<int, HK_HOST_WEAK_SPIVAKOVSKY>());
    case HK_HOST_MIN_HITTING: return f(std::integral_constant<int, HK_HOST_MIN_HITTING>());
  }
  fprintf(stderr, "no host %d\n", host);
  exit(2);
}

template <typename T>
void copy_in(T* dst, const T* src, int count) {
  for (int e = 0; e < count; ++e) dst[e] = src[e];
}

// the move records a routine is handed: absent ones are NULL
template <typename T>
MoveRecords records_of(const Frame<T>& f, int bits) {
  return MoveRecords{(bits & 1) ? f.rec[0] : nullptr, (bits & 2) ? f.rec[1] : nullptr, (bits & 4) ? f.rec[2] : nullptr,
                     (bits & 8) ? f.rec[3] : nullptr, f.S};
}
template <typename T>
void records_out(const Frame<T>& f, int bits, int32_t* io) {
  for (int e = 0; e < f.S; ++e) {
    io[e] = (bits & 4) ? f.mine(2)[e] : 0;
    io[f.S + e] = (bits & 8) ? f.mine(3)[e] : 0;
  }
}

// one game of block h in frame f, which reset() has filled: inputs in, the routine, results out
template <typename T>
void run_game(const Header& h, Frame<T>& f, const T* ti, const int32_t* ii, const double* di, T* to, int32_t* io,
              double* dout) {
  const int m = h.m, d = h.d, n = m * d, S = f.S;
  const T pad = (T)h.dpar[0];
  switch (h.routine) {
    case kNumPoints:
      copy_in(f.par, ti, n);
      io[0] = num_points(f.par, m, d);
      break;
    case kStages:
      copy_in(f.par, ti, n);
      if (h.ipar[0] & HK_STAGE_SHIFT) copy_in(f.c, ti + n, d);
      stages_game(f.par, m, d, f.c, ii[0], pad, (unsigned)h.ipar[0], h.flags);
      copy_in(to, f.par, n);
      break;
    case kRescale:
      copy_in(f.par, ti, n);
      rescale_game(f.par, m, d, pad, h.flags);
      copy_in(to, f.par, n);
      break;
    case kZeillinger:
      copy_in(f.par, ti, n);
      io[0] = h.ipar[0] ? zeillinger_list_game(f.par, m, d) : zeillinger_game(f.par, m, d);
      break;
    case kFeatureSort:
      copy_in(f.par, ti, n);
      feature_sort_game(f.par, m, d, f.row, h.ipar[0] != 0);
      copy_in(to, f.par, n);
      break;
    case kListPair:
      copy_in(f.par, ti, n);
      io[0] = h.ipar[0] ? zeillinger_list_pair<T, true>(f.par, m, d) : zeillinger_list_pair<T, false>(f.par, m, d);
      break;
    case kHostClass:
      copy_in(f.par, ti, n);
      io[0] = h.ipar[1] ? host_class_of<T, Bits128>(h.ipar[0], f.par, m, d)
                        : host_class_of<T, uint64_t>(h.ipar[0], f.par, m, d);
      break;
    case kShiftChild:
      copy_in(f.par, ti, n);
      copy_in(f.c, ti + n, d);
      shift_child(f.lane_slice(), m, d, ii[0]);
      copy_in(to, f.chd, n);
      copy_in(to + n, f.par, n);
      break;
    case kNoteInexact: {
      copy_in(f.chd, ti, n);
      bool inexact = ii[1] != 0;
      note_inexact(f.lane_slice(), m, d, ii[0], inexact);
      io[0] = inexact;
      break;
    }
    case kReduceChild:
      copy_in(f.chd, ti, n);
      io[0] = reduce_child(f.lane_slice(), m, d);
      copy_in(to, f.chd, n);
      break;
    case kExpandChild: {
      copy_in(f.par, ti, n);
      copy_in(f.c, ti + n, d);
      bool inexact = false;
      io[0] = expand_child(f.lane_slice(), m, d, ii[0], inexact);
      io[1] = inexact;
      copy_in(to, f.chd, n);
      break;
    }
    case kExpandMorin: {
      copy_in(f.par, ti, n);
      copy_in(f.c, ti + n, d);
      bool inexact = false;
      int dist = -9;
      io[0] = expand_morin_child(f.lane_slice(), f.ext + d, m, d, ii[0], ii[1], inexact, dist);
      io[1] = inexact;
      io[2] = dist;
      copy_in(to, f.chd, n);
      break;
    }
    case kFindRow:
      copy_in(f.chd, ti, n);
      copy_in(f.ext + d, ti + n, d);
      io[0] = find_row(f.chd, f.ext + d, ii[0], d);
      break;
    case kRowContained:
      copy_in(f.chd, ti, n);
      copy_in(f.ext + d, ti + n, d);
      io[0] = row_contained(f.chd, m, d, ii[0], f.ext + d);
      break;
    case kExceeds:
      copy_in(f.par, ti, n);
      io[0] = exceeds_game(f.par, m, d, di[0]);
      break;
    case kNthBit:
      io[0] = nth_bit((uint32_t)ii[0], ii[1]);
      break;
    case kRandomAxis:
      io[0] = random_legal_axis((uint32_t)ii[0], u64_of(ii + 1), (uint32_t)ii[3], (uint32_t)ii[4], u64_of(ii + 5));
      break;
    case kSubsetCoeffs:
      subset_coeffs(f.c, (uint32_t)ii[0], d);
      copy_in(to, f.c, d);
      break;
    case kForcedOrHost: {
      copy_in(f.par, ti, n);
      copy_in(f.mine(0), ii + 1, S);
      copy_in(f.mine(1), ii + 1 + S, S);
      const MoveRecords rec = records_of(f, h.ipar[2]);
      with_host(h.ipar[0], [&](auto host) {
        int cls = -9, ax = -9;
        uint32_t sub = (uint32_t)-9;
        io[0] = forced_or_host_move<T, decltype(host)::value>(rec, f.g, ii[0], f.par, m, d, cls, sub, ax);
        io[1] = cls, io[2] = (int32_t)sub, io[3] = ax;
      });
      break;
    }
    case kRecordMove: {
      for (int e = 0; e < S; ++e) f.mine(2)[e] = f.mine(3)[e] = -7;
      record_move(records_of(f, h.ipar[2]), f.g, ii[0], ii[1], ii[2]);
      records_out(f, h.ipar[2], io);
      break;
    }
    case kFinishGame: {
      const LaneSlice<T> home = f.lane_slice();
      LaneSlice<T> s = home;
      if (ii[1]) s.par = home.chd, s.chd = home.par;
      copy_in(s.par, ti, n);
      for (int e = 0; e < ii[0]; ++e) f.mine(2)[e] = f.mine(3)[e] = 7;
      finish_game(records_of(f, h.ipar[2]), f.g, ii[0], home, s, n);
      copy_in(to, home.par, n);
      records_out(f, h.ipar[2], io);
      break;
    }
    case kPlayLane: {
      copy_in(f.par, ti, n);
      copy_in(f.mine(0), ii, S);
      copy_in(f.mine(1), ii + S, S);
      const MoveRecords rec = records_of(f, h.ipar[2]);
      GamePlayArgs a{};
      a.class_in = rec.class_in, a.axis_in = rec.axis_in, a.class_out = rec.class_out, a.axis_out = rec.axis_out;
      a.length_out = f.len, a.outcome_out = f.outc;
      a.seed = u64_of(ii + 2 * S + 2);
      a.game_offset = u64_of(ii + 2 * S) - (uint64_t)f.g;  // play_lane adds g back
      a.step_offset = (uint32_t)ii[2 * S + 4];
      a.value_threshold = di[0];
      a.batch = 3, a.m = m, a.d = d, a.max_steps = S, a.agent = h.ipar[3];
      a.reposition = (h.ipar[4] & HK_PLAY_REPOSITION) != 0, a.rescale = (h.ipar[4] & HK_PLAY_RESCALE) != 0;
      a.reduce_root = (h.ipar[4] & HK_PLAY_REDUCE_ROOT) != 0, a.rescale_root = (h.ipar[4] & HK_PLAY_RESCALE_ROOT) != 0;
      with_host(h.ipar[0], [&](auto host) { play_lane<T, decltype(host)::value>(a, f.lane_slice(), f.g); });
      copy_in(to, f.par, n);
      io[0] = f.len[f.g], io[1] = f.outc[f.g];
      records_out(f, h.ipar[2], io + 2);
      break;
    }
    case kEnvMove:
      copy_in(f.par, ti, n);
      env_move(f.env_slice(), m, d, (uint32_t)ii[0], ii[1], h.ipar[0] != 0);
      copy_in(to, f.par, n);
      break;
    case kExtent:
      copy_in(f.par, ti, n);
      io[0] = extent_game(f.par, m, d);
      break;
    case kEnvFresh: {
      EnvStepArgs a{};
      a.m = m, a.d = d, a.max_value = h.ipar[0], a.flags = (uint32_t)h.ipar[1], a.seed = u64_of(ii + 2);
      io[0] = env_fresh<T>(a, f.env_slice(), u64_of(ii));
      copy_in(to, f.par, n);
      break;
    }
    case kEnvHostStep: {
      copy_in(f.par, ti, n);
      EnvStepArgs a{};
      a.m = m, a.d = d, a.flags = (uint32_t)h.ipar[1], a.value_threshold = di[0], a.invalid_move_penalty = di[1];
      const EnvSlice<T> s = f.env_slice();
      const int ext = extent_game(s.par, m, d);
      int cls = ii[1];
      EnvOutcome o{};
      with_host(h.ipar[0], [&](auto host) {
        if constexpr (decltype(host)::value > 0) o = env_host_step<T, decltype(host)::value>(a, s, ext, ii[0], cls);
      });
      copy_in(to, f.par, n);
      io[0] = cls, io[1] = o.stopped, io[2] = o.exceed;
      dout[0] = o.reward;
      break;
    }
    case kEnvAgentStep: {
      copy_in(f.par, ti, n);
      EnvStepArgs a{};
      a.m = m, a.d = d, a.agent = h.ipar[0], a.flags = (uint32_t)h.ipar[1], a.step_threshold = h.ipar[2];
      a.value_threshold = di[0], a.threshold_penalty = di[1], a.agent_seed = u64_of(ii + 4);
      const EnvSlice<T> s = f.env_slice();
      const int ext = extent_game(s.par, m, d);
      int ax = -9;
      const EnvOutcome o = env_agent_step<T>(a, s, ext, (uint32_t)ii[0], u64_of(ii + 1), ii[3], ax);
      copy_in(to, f.par, n);
      io[0] = ax, io[1] = o.stopped, io[2] = o.exceed;
      dout[0] = o.reward;
      break;
    }
  }
}

template <typename U>
std::vector<U> read_vec(FILE* fp, size_t count) {
  std::vector<U> v(count);
  if (count && fread(v.data(), sizeof(U), count, fp) != count) {
    fprintf(stderr, "short case file\n");
    exit(2);
  }
  return v;
}
template <typename U>
void write_vec(FILE* fp, const std::vector<U>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(U), v.size(), fp) != v.size()) {
    fprintf(stderr, "short write\n");
    exit(2);
  }
}

bool differ(const void* a, const void* b, size_t bytes) { return bytes != 0 && memcmp(a, b, bytes) != 0; }

template <typename T>
void run_block(const Header& h, FILE* in, FILE* out) {
  const size_t count = (size_t)h.count;
  const std::vector<T> ti = read_vec<T>(in, count * h.nTi);
  const std::vector<int32_t> ii = read_vec<int32_t>(in, count * h.nIi);
  const std::vector<double> di = read_vec<double>(in, count * h.nDi);
  std::vector<T> to(count * h.nTo), to2(h.nTo);
  std::vector<int32_t> io(count * h.nIo), io2(h.nIo);
  std::vector<double> dout(count * h.nDo), dout2(h.nDo);
  Frame<T> exact(h, false), production(h, true);
  for (size_t g = 0; g < count; ++g) {
    for (int run = 0; run < 8; ++run) {
      const int layout = run >> 2, fill = run & 3;
      Frame<T>& f = layout ? production : exact;
      f.reset(fill);
      T* t_out = run ? to2.data() : to.data() + g * h.nTo;
      int32_t* i_out = run ? io2.data() : io.data() + g * h.nIo;
      double* d_out = run ? dout2.data() : dout.data() + g * h.nDo;
      run_game<T>(h, f, ti.data() + g * h.nTi, ii.data() + g * h.nIi, di.data() + g * h.nDi, t_out, i_out, d_out);
      if (!f.canaries_intact()) fail(h, (int)g, layout, fill, "a canary outside the game's slice or records changed");
      if (run && (differ(t_out, to.data() + g * h.nTo, sizeof(T) * h.nTo) ||
                  differ(i_out, io.data() + g * h.nIo, sizeof(int32_t) * h.nIo) ||
                  differ(d_out, dout.data() + g * h.nDo, sizeof(double) * h.nDo)))
        fail(h, (int)g, layout, fill, "the result differs from that of the exact layout under the NaN fill");
    }
  }
  write_vec(out, to);
  write_vec(out, io);
  write_vec(out, dout);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s CASES RESULTS\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "cannot open the files\n");
    return 2;
  }
  char magic[4];
  int32_t head[2];
  if (fread(magic, 1, 4, in) != 4 || memcmp(magic, "HKLR", 4) != 0 || fread(head, 4, 2, in) != 2 || head[0] != 1) {
    fprintf(stderr, "not a case file of version 1\n");
    return 2;
  }
  for (int b = 0; b < head[1]; ++b) {
    Header h;
    if (fread(&h, sizeof(h), 1, in) != 1) {
      fprintf(stderr, "short case file\n");
      return 2;
    }
    const Lengths want = lengths(h);
    const int got[6] = {h.nTi, h.nIi, h.nDi, h.nTo, h.nIo, h.nDo};
    const bool sized = h.routine >= kNumPoints && h.routine < kRoutineEnd && h.m >= 1 && h.m <= kFixedHostMaxPoints &&
                       h.d >= 2 && h.d <= kLaneGameMaxDim && h.count >= 0 && memcmp(want.v, got, sizeof(got)) == 0;
    if (!sized || (record_len(h) < 1 && h.routine >= kForcedOrHost && h.routine <= kPlayLane)) {
      fprintf(stderr, "block %d: routine %d does not take this header\n", b, h.routine);
      return 2;
    }
    if (h.dtype == HK_F32) run_block<float>(h, in, out);
    else run_block<double>(h, in, out);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  if (failures) fprintf(stderr, "%d failures\n", failures);
  return failures ? 1 : 0;
}
