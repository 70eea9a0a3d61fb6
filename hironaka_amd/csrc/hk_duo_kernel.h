// Two lanes per game: steps and rollouts for batches that do not fill the device.
//
// hk::fast_kernel holds a game in ONE lane, so 65 536 games are 1024 instruction streams for the 1024 SIMDs of
// an MI355X, and a lone wave per SIMD issues an instruction only every ~7.7 cycles: the
// vector ALUs idle half of the time and nothing overlaps the load / store bursts.  hk::duo_kernel deals the
// live rows of a game alternately to a PAIR of lanes (compact rank r -> lane r & 1, slot r >> 1; 32 games per
// wave), so the same batch is twice the waves, each with about half the instructions:
//   * shift is per row; reposition / rescale reduce over a lane's own rows and meet the partner's result
//     through one DPP exchange (quad_perm [1,0,3,2]) per coordinate;
//   * the domination test: a lane runs its own rows' triangle, and of the cross pairs (mine a, partner's b)
//     only those with a <= b, in BOTH directions -- the partner does the same from its side, so every cross
//     pair is visited once (the diagonal twice, consistently); what a lane finds out about the partner's rows
//     travels back through one exchange per slot;
//   * everything else (policies, finished-game counts, the exactness guard and its whole-wave fallback on the
//     generic routines, bucketed straight-line bodies, re-gathering when the widest game narrows) follows
//     hk_fast_kernel.h.
// Row order (which of two equal rows survives, _jax_ops.py:15-40) is the compact rank, i.e. the physical row
// order, exactly as in the one-lane kernel.
#pragma once

#include "hk_fast_kernel.h"
#include "hk_lds_dma.h"

namespace hk {

constexpr int kDuoGames = kWave / 2;

// The two parts around the step loops that won their alternations, one bit each, so that a dev build can take one out
// again (-DHK_DUO_LEGS=<mask>; scripts/build_probe.sh passes it on: mask 0 is the time line "before"; the product builds
// with all of them): 1 the slab by LDS-DMA, 2 the scan's guard as a word and the wave maximum by DPP, 4 the
// finished-game counts of a plain rollout as a histogram in LDS and a prefix sum across lanes (duo_length_counts).
// profiles/duo_prologue_ab.txt holds the alternations of 1 and 2 and those of the two parts that tied and are gone: a
// full wave's final stores without per-chunk predicates, and the finished-game counts behind the final stores (in
// profiles/duo_prologue_timeline*.txt the counts are 0.9 us of the wave's end wherever they stand);
// profiles/duo_epilogue_ab.txt those of 4, of the action window's variants (HK_DUO_PRE_BLOCKS, HK_DUO_FILL_CHAINS
// below) and of the part that lost and is gone: the publish's padding rows in straight line.
#ifndef HK_DUO_LEGS
#define HK_DUO_LEGS 7
#endif
#ifdef HK_DUO_PROBE
// dev builds (scripts/build_probe.sh): a row of time stamps per wave in a buffer of the probe's own -- one copy per
// translation unit; the unit that instantiates the kernels reads it back (hk_duo_spec.hip: hk_duo_probe_read)
constexpr int kDuoProbeRow = 48, kDuoProbeWaves = 4096;
static __device__ int32_t duo_probe_rows[kDuoProbeWaves * kDuoProbeRow];
// (the final store takes two stamps: a parameter of the probe build only)
#define HK_DUO_PROBE_PARAM , int32_t* probe = nullptr
#define HK_DUO_PROBE_ARG(p) , p
#else
#define HK_DUO_PROBE_PARAM
#define HK_DUO_PROBE_ARG(p)
#endif
constexpr bool kDuoLegDma = (HK_DUO_LEGS & 1) != 0, kDuoLegScan = (HK_DUO_LEGS & 2) != 0;
constexpr bool kDuoLegCounts = (HK_DUO_LEGS & 4) != 0;

// the partner lane's value: DPP quad_perm [1, 0, 3, 2]
__device__ __forceinline__ int duo_other_i(int v) { return qperm_i<0xB1>(v); }
__device__ __forceinline__ float duo_other(float v) { return __int_as_float(duo_other_i(__float_as_int(v))); }

// the wave's lanes with `p` as a scalar mask (a bool in, the compare's own mask out: __any / __ballot take an int and
// put a select and a second compare in front of the branch)
__device__ __forceinline__ uint64_t duo_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

template <int M, int D>
struct DuoGeom {
  using G = FastGeom<M, D>;
  static constexpr int CH = (G::C + 1) / 2;                       // slots per lane
  static constexpr int QH = (kDuoGames * G::Q + kWave - 1) / kWave;  // slab chunks per lane
  // plain rollouts deal their rows level by level in straight line, publish only the rows that changed and store the final
  // state write-through (duo_kernel)
  // where the rows take up to 30 registers: at (20,4) -- 40 -- the headline instantiation sits at the 168 VGPRs of three
  // waves per SIMD, and each change costs it the third wave (169 with the partial publish, 185 with the level deal, 169
  // with the write-through final stores' descriptor): it keeps the slot-by-slot deal, the refill and non-temporal stores
  static constexpr bool kLean = CH * D <= 30;
};

// ---- slab I/O for 32 games per wave (see hk_fast_kernel.h: all requests in flight before the first use) --
template <int M, int D>
struct DuoSlabRegs {
  typename VecOf<FastGeom<M, D>::W>::type v[DuoGeom<M, D>::QH];
};

template <int M, int D, bool CONTIG>
__device__ __forceinline__ void duo_slab_issue_impl(DuoSlabRegs<M, D>& r, const float* base, int64_t in_stride,
                                                    int ngames, int lane) {
  using G = FastGeom<M, D>;
  using V = typename VecOf<G::W>::type;
  const int total = ngames * G::Q;
#pragma unroll
  for (int it = 0; it < DuoGeom<M, D>::QH; ++it) {
    int q = lane + it * kWave;
    q = q < total ? q : total - 1;
    r.v[it] = *reinterpret_cast<const V*>(base + slab_chunk_global<M, D, CONTIG>(q, in_stride));
  }
}

template <int M, int D>
__device__ __forceinline__ void duo_slab_issue(DuoSlabRegs<M, D>& r, const float* in, int64_t in_stride, int64_t g0,
                                               int ngames, int lane) {
  const float* base = in + g0 * in_stride;
  if (in_stride == FastGeom<M, D>::N) duo_slab_issue_impl<M, D, true>(r, base, in_stride, ngames, lane);
  else duo_slab_issue_impl<M, D, false>(r, base, in_stride, ngames, lane);
}

template <int M, int D>
__device__ __forceinline__ void duo_slab_commit(DuoSlabRegs<M, D>& r, float* lds, int ngames, int lane) {
  using G = FastGeom<M, D>;
  using V = typename VecOf<G::W>::type;
  const int total = ngames * G::Q;
#pragma unroll
  for (int it = 0; it < DuoGeom<M, D>::QH; ++it) asm volatile("" : "+v"(r.v[it]));
#pragma unroll
  for (int it = 0; it < DuoGeom<M, D>::QH; ++it) {
    const int q = lane + it * kWave;
    if (q < total) *reinterpret_cast<V*>(lds + slab_chunk_lds<M, D>(q)) = r.v[it];
  }
}

// The slab by LDS-DMA (hk_quad_kernel.h: quad_slab_load), where the two-lane image IS the contiguous slab -- 16-byte
// chunks, no row padding in LDS (FastGeom::S == N: (20,3), (4,3)) -- and the caller's records are contiguous and 16-byte
// aligned (the kernel checks both, wave-uniform): lane l of request `it` moves 16 B to image + (it * 64 + l) * 16.  No
// registers, no ds_write, no commit under per-chunk masks: one VGPR offset, the slab's base in SGPRs, the rest in the
// instructions' immediate offsets.  A full wave's requests are whole but for the constant mask of the last one; on the
// batch's last slab the lanes past its end sit out (nothing is written past the games the wave owns).  Completion is the
// wave's vmcnt.  Every other layout (strided or unaligned records, other chunk widths, padded images) stays on the
// register path above.
template <int M, int D>
struct DuoDma {
  using G = FastGeom<M, D>;
  static constexpr bool kShape = kDuoLegDma && G::W == 4 && G::S == G::N;
};

template <int M, int D>
__device__ __forceinline__ void duo_slab_dma(const float* base, float* image, int ngames, int lane) {
  using G = FastGeom<M, D>;
  constexpr int FULL = kDuoGames * G::Q;  // requests of a full slab
  constexpr int QH = DuoGeom<M, D>::QH;   // ... per lane
  constexpr int kImm = kDmaImm;  // (the immediate offset moves the global AND the LDS address)
  static_assert(DuoDma<M, D>::kShape, "the image is the slab");
  const float* src = base + (unsigned)lane * 4;  // request `it`: + it * 64 * 4 floats, in the immediate
  const unsigned total = (unsigned)ngames * G::Q;
  if (ngames == kDuoGames) {  // (wave-uniform) every request but the last one whole
    unrolled_while<0, QH>([&](auto ic) {
      constexpr int it = decltype(ic)::value;
      if ((it + 1) * kWave <= FULL || lane < FULL - it * kWave)
        lds_dma<16, (it * kWave * 16) % kImm>(src + (it * kWave * 16) / kImm * (kImm / 4),
                                             image + (it * kWave * 16) / kImm * (kImm / 4));
      return true;
    });
  } else {  // the batch's last slab: lanes past its end sit out
    unrolled_while<0, QH>([&](auto ic) {
      constexpr int it = decltype(ic)::value;
      if ((unsigned)lane + it * kWave < total)
        lds_dma<16, (it * kWave * 16) % kImm>(src + (it * kWave * 16) / kImm * (kImm / 4),
                                             image + (it * kWave * 16) / kImm * (kImm / 4));
      return true;
    });
  }
}

// How a slab's chunks leave for memory.  Plain and non-temporal stores keep their lines, dirty, in the XCD's L2.
// Write-through stores (sc1) cost a plain store each, drain while the launch's other waves still play and leave nothing
// to write back; the line is dropped from the writer's L2, so the next reader is served from the Infinity Cache.
// Measured on the headline: the kernel is 4 % shorter than with non-temporal stores, the gap to
// the next dispatch the same; plain stores and `sc1 nt` lost.
constexpr int kStorePlain = 0, kStoreNT = 1, kStoreWT = 2;

// kBatch: image chunks read per round (everything at once for the final store; fewer inside the recording loop,
// whose register budget the rows own)
// (write-through: 16-byte chunks of contiguous records, through a buffer descriptor over the wave's own slab -- its
// range check bounds every store once more; other chunk widths and strided records stay non-temporal)
template <int M, int D, bool CONTIG, int kBatch, int ST = kStorePlain>
__device__ __forceinline__ void duo_store_slab_impl(const float* lds, float* base, int64_t out_stride, int ngames,
                                                    int lane HK_DUO_PROBE_PARAM) {
  using G = FastGeom<M, D>;
  using V = typename VecOf<G::W>::type;
  constexpr int QH = DuoGeom<M, D>::QH;
  constexpr bool kWT = ST == kStoreWT && CONTIG && G::W == 4;
  const int total = ngames * G::Q;
#pragma unroll
  for (int i0 = 0; i0 < QH; i0 += kBatch) {
    V v[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {  // the image holds kDuoGames games whatever ngames is
      int q = lane + (i0 + u) * kWave;
      q = q < kDuoGames * G::Q ? q : kDuoGames * G::Q - 1;
      v[u] = *reinterpret_cast<const V*>(lds + slab_chunk_lds<M, D>(q));
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) asm volatile("" : "+v"(v[u]));
#ifdef HK_DUO_PROBE
    if (probe && lane == 0) probe[0] = (int32_t)wall_clock64();  // the image is in registers
#endif
    if constexpr (kWT) {
      typedef unsigned int vu4 __attribute__((ext_vector_type(4)));
      // (the descriptor from wave-uniform values: the slab's base as two scalar halves, its bytes)
      const uint64_t b = (uint64_t)base;
      const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)b), bhi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
      const int bytes = __builtin_amdgcn_readfirstlane(total * G::W * (int)sizeof(float));
      const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)bhi << 32) | blo), 0, bytes, 0x00020000);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int q = lane + (i0 + u) * kWave;
        if (i0 + u < QH && q < total)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(vu4, v[u]), rsrc, q * G::W * (int)sizeof(float), 0,
                                                 16);  // aux: sc1
      }
    } else {
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int q = lane + (i0 + u) * kWave;
        if (i0 + u < QH && q < total) {
          V* dst = reinterpret_cast<V*>(base + slab_chunk_global<M, D, CONTIG>(q, out_stride));
          if constexpr (ST != kStorePlain) __builtin_nontemporal_store(v[u], dst);
          else *dst = v[u];
        }
      }
    }
  }
}

template <int M, int D, int kBatch = DuoGeom<M, D>::QH, int ST = kStorePlain>
__device__ inline void duo_store_slab(const float* lds, float* out, int64_t out_stride, int64_t g0, int ngames,
                                      int lane HK_DUO_PROBE_PARAM) {
  float* base = out + g0 * out_stride;
  if (out_stride == FastGeom<M, D>::N) duo_store_slab_impl<M, D, true, kBatch, ST>(lds, base, out_stride, ngames, lane HK_DUO_PROBE_ARG(probe));
  else duo_store_slab_impl<M, D, false, kBatch, ST>(lds, base, out_stride, ngames, lane HK_DUO_PROBE_ARG(probe));
#ifdef HK_DUO_PROBE
  if (probe && lane == 0) probe[1] = (int32_t)wall_clock64();  // the stores are issued
#endif
}

// The parts of the step loops themselves, one bit each as HK_DUO_LEGS above (-DHK_DUO_STEPS=<mask>; scripts/build_probe.sh
// passes it on; profiles/duo_levels_ab.txt holds their alternations): 1 a level of seven slots per lane in the plain
// rollouts' staircase (DuoLadderT), 2 the domination test's verdicts as sign bits of a word per row on the narrow levels
// (d_newton_signs).
#ifndef HK_DUO_STEPS
#define HK_DUO_STEPS 3
#endif
constexpr bool kDuoStepSeven = (HK_DUO_STEPS & 1) != 0, kDuoStepSigns = (HK_DUO_STEPS & 2) != 0;

// slots per lane: 1..6, 8, 10, ...; SEVEN: 1..8, 10, ... -- a wave whose widest game has 13 or 14 rows plays its first
// steps on 49 pair tests per lane, not 64.  The plain rollouts of ten slots per lane take the seven (duo_kernel: Ladder);
// single steps, recording rollouts and Zeillinger's host (kDuoZeilDpp: its unrolled pair loop ends at six slots) keep the
// ladder they had.
template <bool SEVEN>
struct DuoLadderT {
  static constexpr int next_bucket(int nb) { return nb < (SEVEN ? 8 : 6) ? nb + 1 : nb + 2; }
};
using DuoLadder = DuoLadderT<false>;

// ---- image <-> registers ----------------------------------------------------------------------------------
// the set bits of `mask` in ascending order are the game's live rows; lane h takes the ranks h, h + 2, ...
// slot by slot, with an early exit at the first slot past smax (SB: compile-time bound of the slots touched); a slot
// past the lane's last row becomes a hole
template <int M, int CH, int D, int SB = CH>
__device__ __forceinline__ void duo_gather_slots(float (&q)[CH * D], const float* mine, uint32_t mask, int smax, int h) {
  mask = h ? (mask & (mask - 1)) : mask;  // (the second lane drops the first bit once: one bit scan per slot)
  unrolled_while<0, SB>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    if (s >= smax) return false;
    const bool has = mask != 0;
    const float* row = mine + (has ? mask_first(mask) : 0) * D;
    mask &= mask - 1;
    mask &= mask - 1;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const float v = row[k];
      q[s * D + k] = has ? v : INFINITY;
    }
    return true;
  });
}

// One level of the deal, straight line on NB slots per lane: the lane's own ranks first (the second lane drops the
// mask's first bit once; a slot then costs one bit scan and two clears), then every read of the image back to back and
// one wait.  A slot past the lane's last row reads `hole`, a row of +inf in LDS: it becomes a hole without a select.
// Slots [NB, SB) are set to holes here, by every level of a dispatch alike: levels that wrote different sets of slots
// were merged by the compiler into stores at a run-time index, which put the rows into scratch memory.
template <int CH, int D, int NB, int SB = NB>
__device__ __forceinline__ void duo_gather_level(float (&q)[CH * D], const float* mine, const float* hole, uint32_t mask,
                                                 int h) {
  mask = h ? (mask & (mask - 1)) : mask;
  const float* row[NB];
#pragma unroll
  for (int s = 0; s < NB; ++s) {
    row[s] = mask != 0 ? mine + mask_first(mask) * D : hole;
    mask &= mask - 1;
    mask &= mask - 1;
  }
#pragma unroll
  for (int s = 0; s < NB; ++s)
#pragma unroll
    for (int k = 0; k < D; ++k) q[s * D + k] = row[s][k];
#pragma unroll
  for (int e = NB * D; e < SB * D; ++e) q[e] = INFINITY;
}

// slots [0, smax) from the image.  LEVELS: the body is the smallest LADDER level that covers smax (wave-uniform), SB
// at most, and every slot up to SB is written; else slot by slot.
template <int M, int CH, int D, bool LEVELS, typename LADDER = DuoLadder, int SB = CH>
__device__ __forceinline__ void duo_gather(float (&q)[CH * D], const float* mine, const float* hole, uint32_t mask,
                                           int smax, int h) {
  if constexpr (LEVELS) {
    StagesFor<LADDER, SB>::run(smax, [&](auto nb) {
      duo_gather_level<CH, D, decltype(nb)::value, SB>(q, mine, hole, mask, h);
      return 0;
    });
  } else {
    duo_gather_slots<M, CH, D, SB>(q, mine, mask, smax, h);
  }
}

// the lane's live rows back to their slots, straight line on NB slots; returns the lane's part of the mask of the
// game's slots still alive
template <int CH, int D, int NB>
__device__ __forceinline__ uint32_t duo_scatter_level(const float (&q)[CH * D], float* mine, uint32_t mask, int h) {
  mask = h ? (mask & (mask - 1)) : mask;
  uint32_t alive = 0;
#pragma unroll
  for (int s = 0; s < NB; ++s) {
    if (mask != 0 && q[s * D] < INFINITY) {
      const int slot = mask_first(mask);
      alive |= 1u << slot;
      float* row = mine + slot * D;
#pragma unroll
      for (int k = 0; k < D; ++k) row[k] = q[s * D + k];
    }
    mask &= mask - 1;
    mask &= mask - 1;
  }
  return alive;
}

// the lane's live rows back to their slots; returns the mask of the GAME's slots still alive
// (slot by slot with an early exit: where the width is not known at compile time -- the publish, the recording loop --
// few slots are in use, and levels that read different sets of slots end up reading the rows from scratch memory)
template <int M, int CH, int D, int SB = CH>
__device__ __forceinline__ uint32_t duo_scatter(const float (&q)[CH * D], float* mine, uint32_t mask, int smax, int h) {
  mask = h ? (mask & (mask - 1)) : mask;
  uint32_t alive = 0;
  unrolled_while<0, SB>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    if (s >= smax) return false;
    if (mask != 0 && q[s * D] < INFINITY) {
      const int slot = mask_first(mask);
      alive |= 1u << slot;
      float* row = mine + slot * D;
#pragma unroll
      for (int k = 0; k < D; ++k) row[k] = q[s * D + k];
    }
    mask &= mask - 1;
    mask &= mask - 1;
    return true;
  });
  return lanes_or<2>(alive);
}

// `dead`: rows of the game's image to overwrite with the padding row; the pair shares them by rank
// (in straight line over the slots per lane at entry, as duo_scatter, it lost its alternation -- x1.008 alone,
// profiles/duo_epilogue_ab.txt -- and took the (20,3) records instantiation from 168 to 191 VGPRs)
template <int D>
__device__ __forceinline__ void duo_pad_rows(float* mine, uint32_t dead, float pad, int h) {
  dead = h ? (dead & (dead - 1)) : dead;
  while (dead != 0) {
    float* row = mine + mask_first(dead) * D;
#pragma unroll
    for (int k = 0; k < D; ++k) row[k] = pad;
    dead &= dead - 1;
    dead &= dead - 1;
  }
}

// one pass over the lane's HALF of the game's image (rows h * ceil(M / 2) ...): bitmask of the fully available rows of
// the whole game (the partner's half through DPP) + representability of the lane's half (the caller ANDs over the wave)
template <int M, int D>
__device__ __forceinline__ void duo_scan_half(const float* mine, float fill, int h, uint32_t& live, bool& ok) {
  static_assert(M <= 32, "the game's mask is one word");
  constexpr int C = (M + 1) / 2;
  const int i0 = h * C;
  const float* base = mine + i0 * D;
  uint32_t mask = 0;
  const uint32_t fill_bits = __float_as_uint(fill);
  // The guard as a word per lane: a row that is neither available nor the fill row ORs the bits in which its extrema
  // differ from the fill value into `off` (not zero: one of the two differs), an available row ORs zero -- the select
  // rides on the compare the row's mask bit needs anyway; one compare after the last row.  (As a bool per row it was two
  // more compares and three scalar and/or instructions chained through SGPR pairs, row after row.)
  uint32_t off = 0;
  bool okb = true;
#pragma unroll
  for (int r = 0; r < C; ++r) {
    // (M odd: the second lane's last row lies past the game -- its read stays inside the wave's image and is not counted)
    const bool valid = (M % 2 == 0) || r + 1 < C || h == 0;
    uint32_t hi = __float_as_uint(base[r * D]), lo = hi;
#pragma unroll
    for (int k = 1; k < D; ++k) {
      const uint32_t u = __float_as_uint(base[r * D + k]);
      hi = u > hi ? u : hi;
      lo = u < lo ? u : lo;
    }
    const bool ge = hi < 0x7F800000u;
    if constexpr (DuoGeom<M, D>::kLean && kDuoLegScan) {
      const uint32_t differs = (hi ^ fill_bits) | (lo ^ fill_bits);  // zero: the fill row
      off |= (ge || !valid) ? 0u : differs;
    } else {  // ((20,4) sits at the registers of its third wave: it keeps the chain of scalar masks)
      const bool fl = (lo == fill_bits) && (hi == fill_bits);
      okb &= (ge | fl | !valid);
    }
    mask |= (ge && valid) ? (1u << r) : 0u;
  }
  ok = (DuoGeom<M, D>::kLean && kDuoLegScan) ? off == 0u : okb;
  mask <<= i0;
  live = lanes_or<2>(mask);
}

// wave-wide maximum of a small non-negative int, in straight line: a running maximum within rows of 16 lanes by DPP row
// shifts, the rows' maxima carried over by two row broadcasts, lane 63 read (wave_sum_u32 in hk_fast_kernel.h is the
// same walk with a sum).  hk::wave_max counts down from its bound `hi`, a compare, two branches and four scalar
// instructions per candidate: about ten rounds from 20 after the scan.  Whole wave active (callers sit under wave-uniform
// branches).  DPP false ((20,4): DuoGeom::kLean, the registers of its third wave): the countdown.
template <bool DPP>
__device__ __forceinline__ int duo_wave_max(int v, int hi) {
  if constexpr (!DPP) return wave_max(v, hi);
  auto mx = [](int a, int b) { return a > b ? a : b; };
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true));   // row_shr:1 (lanes shifted in: 0)
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true));   // row_shr:2
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true));   // row_shr:4
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true));   // row_shr:8
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false));  // row_bcast:15 -> rows 1, 3
  v = mx(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false));  // row_bcast:31 -> rows 2, 3
  return __builtin_amdgcn_readlane(v, kWave - 1);
}

// The per-step finished-game counts of a wave (add_length_counts in hk_common.h: step s counts the games whose first
// finished step is <= s) in closed form, for episodes of at most kWave - 1 steps: they are the running sum of a histogram
// of at most 32 small integers.  `hist` is 64 words of LDS: every lane zeroes its word, the lane that speaks for a
// finished game adds one to hist[length] (ds_add_u32), lane s reads hist[s] -- a wave's LDS instructions complete in
// order, so the three need no wait between them --, an inclusive prefix sum across the lanes follows -- DPP row shifts
// within rows of 16, two row broadcasts, the walk of wave_sum_u32 without its v_readlane -- and lane s <= nsteps with a
// non-zero total issues the one atomic of add_length_counts.  Step 0 is part of the sum (games finished at entry:
// length 0), so there is no entry count of its own.  The ballot form went VALU -> SGPR pair -> s_bcnt1 -> VALU once per
// step: 20 dependent rounds, 1 us of every wave's end.  Whole wave active.
// (The zeroing store stands here and not in the prologue, where the wave waits for its slab anyway: from there -- from
// anywhere ahead of the step loops -- it cost (10,3) six to eight registers and a wave per SIMD, (20,4) its third wave.)
__device__ __forceinline__ void duo_length_counts(uint32_t* hist, uint32_t* slot, uint32_t stride, int nsteps, bool counted,
                                                  int length, int lane) {
  hist[lane] = 0u;
  if (counted && length >= 0) __hip_atomic_fetch_add(hist + length, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();  // (a workgroup is one wave)
  uint32_t v = hist[lane];
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);   // row_shr:1 (lanes shifted in: 0)
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);   // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);   // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
  if (lane <= nsteps && v) count_add(slot + (size_t)lane * stride, v);
}

// ---- the stages on NB slots per lane ----------------------------------------------------------------------
// _jax_ops.py:15-73 across the pair.  Own rows i < j as in b_newton (rank 2i+h < 2j+h).  Cross pairs (mine a,
// partner's b) with a <= b: my rank 2a+h, the partner's 2b+1-h, so my row is the earlier one unless a == b and
// h == 1.  With t = max_k(mine - other), u = min_k(mine - other):
//   mine earlier:  other removed iff t <= 0;            mine removed iff u >= 0 and t > 0
//   other earlier: other removed iff t <= 0 and u < 0;  mine removed iff u >= 0
// acc[] <= 0 marks my row removed; oth[] <= 0 marks the partner's slot removed (sent back at the end).
//
// The verdicts as sign bits (kDuoStepSigns).  On this path a coordinate is a bit pattern in [+0, +inf] (the exactness
// guard admits no sign bit; sums, x - min and quotients of such values keep it clear), so a difference is never -0 and
// t >= u.  With T = bits(t) - 1 and U = bits(u), as integers:
//   t <= 0           iff  T < 0   (+0 wraps to -1; a negative t keeps its sign bit: its magnitude is not zero)
//   u >= 0 and t > 0 iff  U >= 0 and T >= 0   (u >= 0 gives t >= 0, and then t > 0 iff its bits are not zero)
//   u < 0            iff  U < 0
// so "the later row removed" is the sign of T, "the earlier row removed" the sign of ~(U | T), and a row's verdicts meet
// by OR in ONE word per row: an add and two three-input bit operations per pair, where the float form was a compare, a
// select and two minima.  Equal rows (t = u = +0: T = -1) remove the later one alone, as before.  A hole against a live
// row gives t = u = -inf or +inf, signs as for any other value; which verdict a hole itself gets -- against a live row, or
// against another hole, where t and u are NaN -- does not matter: removing it writes +inf over +inf.
// The form costs two registers.  The plain rollouts without records of the lean shapes of eight slots per lane and more
// take it (duo_kernel: kSigns): the (8,4) headline instantiation would lose its seventh wave per SIMD (71 -> 73 VGPRs),
// (20,4) its third (168 -> 170), and so would the (20,3) run-time instantiation with the small records (168 -> 170).
constexpr int kDuoSignsMinSlots = 8;
// Levels of up to four slots per lane take it -- the levels every wave plays, and the one-slot level most of all.  On the
// wide levels the pinned accumulators (below) order the pair tests more strictly than the float minima did, and the form
// loses: at (20,3) on every level 15.10 us per launch against 14.76 on levels 1..6 and 14.48 on 1..4, the level of seven
// alone 16.38 against 14.61 (profiles/duo_levels_ab.txt).
constexpr int kDuoSignsMaxLevel = 4;
template <int CH, int D, int NB>
__device__ __forceinline__ void d_newton_signs(float (&q)[CH * D], int h) {
  uint32_t acc[NB], oth[NB];  // sign bit set: my row / the partner's slot is removed
#pragma unroll
  for (int i = 0; i + 1 < NB; ++i) {
#pragma unroll
    for (int j = i + 1; j < NB; ++j) {
      float t, u;
      diff_extrema<D>(&q[i * D], &q[j * D], t, u);
      const uint32_t T = __float_as_uint(t) - 1u, U = __float_as_uint(u);
      acc[j] = (i == 0) ? T : (acc[j] | T);
      acc[i] = (i == 0 && j == 1) ? ~(U | T) : (acc[i] | ~(U | T));
      // (pinned pair by pair: integer ORs, unlike the float minima, may be regrouped across the scheduling barriers, and
      // the regrouped form kept a row of verdicts alive per accumulator -- 24 to 70 registers more, a wave per SIMD or two)
      asm volatile("" : "+v"(acc[i]), "+v"(acc[j]));
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  const uint32_t late = 0u - (uint32_t)h;  // all ones: on the diagonal the partner's row is the earlier one
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float o[D];
#pragma unroll
    for (int k = 0; k < D; ++k) o[k] = duo_other(q[b * D + k]);
    {  // diagonal
      float t, u;
      diff_extrema<D>(&q[b * D], o, t, u);
      const uint32_t T = __float_as_uint(t) - 1u, U = __float_as_uint(u);
      const uint32_t va = ~U & (~T | late);  // mine: u >= 0 and (t > 0 or late)
      acc[b] = (NB == 1) ? va : (acc[b] | va);
      oth[b] = T & (U | ~late);              // the partner's: t <= 0 and (u < 0 or not late)
    }
#pragma unroll
    for (int a = 0; a < b; ++a) {
      float t, u;
      diff_extrema<D>(&q[a * D], o, t, u);
      const uint32_t T = __float_as_uint(t) - 1u, U = __float_as_uint(u);
      oth[b] |= T;
      acc[a] |= ~(U | T);
      asm volatile("" : "+v"(oth[b]), "+v"(acc[a]));
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    const bool removed = (int32_t)(acc[r] | (uint32_t)duo_other_i((int)oth[r])) < 0;
#pragma unroll
    for (int k = 0; k < D; ++k) q[r * D + k] = removed ? INFINITY : q[r * D + k];
  }
}

// SIGNS: the rows are those of a rollout (see d_newton_signs; a single step takes any real weights from its caller)
template <int CH, int D, int NB, bool SIGNS = false>
__device__ __forceinline__ void d_newton(float (&q)[CH * D], int h) {
  if constexpr (SIGNS && kDuoStepSigns && NB <= kDuoSignsMaxLevel) return d_newton_signs<CH, D, NB>(q, h);
  // (the accumulators take their FIRST contribution by assignment -- which one that is, is known at compile time --
  // instead of starting at +inf: min(+inf, x) was an instruction per slot, two with the canonicalising v_max)
  float acc[NB], oth[NB];
#pragma unroll
  for (int i = 0; i + 1 < NB; ++i) {
#pragma unroll
    for (int j = i + 1; j < NB; ++j) {
      float t, u;
      diff_extrema<D>(&q[i * D], &q[j * D], t, u);
      const float vi = (t > 0.0f) ? -u : 1.0f;
      acc[j] = (i == 0) ? t : hk_fmin(acc[j], t);
      acc[i] = (i == 0 && j == 1) ? vi : hk_fmin(acc[i], vi);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  const bool late = h != 0;  // on the diagonal the partner's row is the earlier one
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float o[D];
#pragma unroll
    for (int k = 0; k < D; ++k) o[k] = duo_other(q[b * D + k]);
    {  // diagonal
      float t, u;
      diff_extrema<D>(&q[b * D], o, t, u);
      const float va = (t > 0.0f || late) ? -u : 1.0f;
      acc[b] = (NB == 1) ? va : hk_fmin(acc[b], va);
      oth[b] = (u < 0.0f || !late) ? t : 1.0f;
    }
#pragma unroll
    for (int a = 0; a < b; ++a) {
      float t, u;
      diff_extrema<D>(&q[a * D], o, t, u);
      oth[b] = hk_fmin(oth[b], t);
      acc[a] = hk_fmin(acc[a], (t > 0.0f) ? -u : 1.0f);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    // (two compares, not a float minimum of a value that came through DPP: that one is canonicalised first)
    const bool r0 = acc[r] <= 0.0f, r1 = duo_other(oth[r]) <= 0.0f;
    const bool removed = r0 || r1;
#pragma unroll
    for (int k = 0; k < D; ++k) q[r * D + k] = removed ? INFINITY : q[r * D + k];
  }
}

// b_shift_mask without compares, for the one-slot level (a step on one slot per lane is a single dependent chain: nothing
// fills the wait states between a compare and the select that reads it; at two slots per lane the hot (10,3) rollout
// paid 19 registers and a wave per SIMD for it, so the wider levels keep the selects).  The subset's bits and the axis become
// words of all ones / zero (v_bfe_i32); a coordinate joins the sum through AND -- zero gives +0.0 as the select did,
// +inf stays +inf -- and the sum replaces the axis' coordinate through a bit-field insert.
template <int CH, int D, int NB>
__device__ __forceinline__ void d_shift_words(float (&q)[CH * D], uint32_t cmask, int axis, int np, unsigned flags) {
  bool apply = true;
  if (flags & HK_FLAG_AXIS_NOOP_IF_INVALID) apply = axis >= 0 && ((cmask >> axis) & 1u);
  if ((flags & HK_FLAG_IGNORE_ENDED) && np < 2) apply = false;
  const uint32_t onehot = apply ? 1u << (axis & 31) : 0u;  // (an axis past the dimension selects nothing, as k == axis did)
  uint32_t isax[D], in[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    isax[k] = (uint32_t)((int32_t)(onehot << (31 - k)) >> 31);
    in[k] = (uint32_t)((int32_t)(cmask << (31 - k)) >> 31);
    asm volatile("" : "+v"(isax[k]), "+v"(in[k]));  // (left in sight, the words are turned back into compares and selects)
  }
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    float s = __uint_as_float(__float_as_uint(q[r * D]) & in[0]);
#pragma unroll
    for (int k = 1; k < D; ++k) s = s + __uint_as_float(__float_as_uint(q[r * D + k]) & in[k]);  // order 0..D-1
#pragma unroll
    for (int k = 0; k < D; ++k)
      q[r * D + k] = __uint_as_float((__float_as_uint(s) & isax[k]) | (__float_as_uint(q[r * D + k]) & ~isax[k]));
  }
}

// one transition on slots [0, NB) of both lanes; returns the GAME's number of live rows
// (WORDS: the shift of a 0/1 subset as d_shift_words; SIGNS: the domination test as d_newton_signs)
template <int CH, int D, int NB, bool BIN = false, bool WORDS = false, bool SIGNS = false>
__device__ __forceinline__ int d_stages(float (&q)[CH * D], const float (&c)[D], int axis, int np, int h,
                                        unsigned flags, unsigned stages, uint32_t cmask = 0) {
  static_assert(!WORDS || BIN, "the subset as bits");
  static_assert(!SIGNS || BIN, "the rows of a rollout");
  if (stages & HK_STAGE_SHIFT) {
    if constexpr (WORDS) d_shift_words<CH, D, NB>(q, cmask, axis, np, flags);
    else if constexpr (BIN) b_shift_mask<CH, D, NB>(q, cmask, axis, np, flags);
    else b_shift<CH, D, NB>(q, c, axis, np, flags);
  }
  if (stages & HK_STAGE_REPOSITION) reposition<2, CH, D, NB, BIN>(q, flags);
  if (stages & HK_STAGE_NEWTON) d_newton<CH, D, NB, SIGNS>(q, h);
  if (stages & HK_STAGE_RESCALE) rescale<2, CH, D, NB>(q, flags);
  return live_rows<2, CH, D, NB>(q);
}

template <int CH, int D, int NB, bool BIN = false>
struct DuoStagesFor {
  static constexpr int kNext = DuoLadder::next_bucket(NB);
  static __device__ __forceinline__ int run(float (&q)[CH * D], int smax, const float (&c)[D], int axis, int np,
                                            int h, unsigned flags, unsigned stages, uint32_t cmask = 0) {
    if constexpr (NB >= CH) {
      return d_stages<CH, D, CH, BIN>(q, c, axis, np, h, flags, stages, cmask);
    } else {
      if (smax <= NB) return d_stages<CH, D, NB, BIN>(q, c, axis, np, h, flags, stages, cmask);
      return DuoStagesFor<CH, D, kNext, BIN>::run(q, smax, c, axis, np, h, flags, stages, cmask);
    }
  }
};

// ---- list semantics for plain rollouts: the pair's rows ranked in descending lexicographic order (coordinate 0
// first; rows are distinct after a Newton stage) and written to their rank, once, at the end of the launch -------------
template <int CH, int D>
__device__ __forceinline__ void duo_ranks_first(const float (&q)[CH * D], int smax, int (&rank)[CH]) {
#pragma unroll
  for (int s = 0; s < CH; ++s) rank[s] = 0;
  unrolled_while<0, CH>([&](auto bc) {
    constexpr int b = decltype(bc)::value;
    if (b >= smax) return false;
    float o[D];
#pragma unroll
    for (int k = 0; k < D; ++k) o[k] = duo_other(q[b * D + k]);
    const bool live_o = o[0] < INFINITY, live_b = q[b * D] < INFINITY;
    unrolled_while<0, CH>([&](auto ac) {
      constexpr int a = decltype(ac)::value;
      if (a >= smax) return false;
      rank[a] += (live_o && key_gt<D, kKeyFirst>(o, &q[a * D])) ? 1 : 0;                      // the partner's row b
      if (a != b) rank[a] += (live_b && key_gt<D, kKeyFirst>(&q[b * D], &q[a * D])) ? 1 : 0;  // my own row b
      return true;
    });
    return true;
  });
}

template <int CH, int D>
__device__ __forceinline__ void duo_scatter_ranked(const float (&q)[CH * D], float* mine, const int (&rank)[CH], int smax) {
  unrolled_while<0, CH>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    if (s >= smax) return false;
    if (q[s * D] < INFINITY) {
      float* row = mine + rank[s] * D;
#pragma unroll
      for (int k = 0; k < D; ++k) row[k] = q[s * D + k];
    }
    return true;
  });
}

// The policy stream of a pair: Philox block b (steps 4b .. 4b + 3, hk_common.h policy_words) is computed by the lane
// with (b & 1) == h only -- one Philox per lane per EIGHT steps -- and its word reaches the partner through DPP.
struct DuoPolicyCache {
  U4 r;
  uint32_t pair = 0xFFFFFFFFu;  // wave-uniform: `r` is block 2 * pair + h
};

__device__ inline void duo_policy_words(uint64_t gg, uint32_t step, uint64_t seed, DuoPolicyCache& cache, int h,
                                        uint32_t& host_word, uint32_t& agent_word) {
  const uint32_t block = step >> 2, pair = block >> 1;
  if (cache.pair != pair) {
    cache.r = philox4x32((uint32_t)gg, (uint32_t)(gg >> 32), (pair << 1) | (uint32_t)h, kStreamPolicy, seed);
    cache.pair = pair;
  }
  const uint32_t mine = u4_word(cache.r, step & 3u);
  const bool own = (int)(block & 1u) == h;
  // (the exchange as a statement of its own, pinned by an empty asm: written inside the select the compiler ran the
  // DPP move under the select's exec mask -- the partner lane inactive, its value read as zero)
  uint32_t theirs = (uint32_t)duo_other_i((int)mine);
  asm volatile("" : "+v"(theirs));
  const uint32_t w = own ? mine : theirs;
  host_word = w & 0xFFFF0000u;
  agent_word = w << 16;
}

// ---- Zeillinger's host on the pair's rows (jax/players.py:55-109; hk_fast_rows.h: c_zeillinger is the one-lane twin) --
// Over the pairs i < j of live rows (row-major order = rank order: the deals keep it): the characteristic vector
// (L, S) = (max - min, #max + #min) of P_i - P_j, differences that are constant (jnp.isclose) do not count, the first
// minimum wins, the subset is {argmin, argmax} of that difference; no pair: class 0.  Rank of (slot s, lane h) = 2 s + h.
// A lane takes its own slots a < b and, against the partner's rows (DPP), the slots b >= a (lane 1: b > a) -- every
// pair once, "mine" always the earlier row: NB^2 tests per lane where the one-lane kernel runs 2 NB^2 on half the
// waves.  "First" is explicit -- the pair's index 64 i + j breaks ties --, so the two lanes' bests merge by the same
// comparison.
// Buckets of more than kDuoZeilDpp slots per lane: the same pairs as a ROLLED loop over the game's rows parked by
// rank in its image (scratch between two deals) -- unrolled, 64 pair tests on 8 slots per lane spilled 692 B per lane
// and a first step took 51 us; lane h takes the rows i = h, h + 2, ... against every later row.  (Measured per
// 20-step episode of 65 536 games: DPP up to 4 slots 47.5 us, up to 6 slots 44.3 us; 242 VGPRs, no scratch.)
constexpr int kDuoZeilDpp = 6;

template <int CH, int D, int NB>
__device__ __forceinline__ int duo_zeillinger(const float (&q)[CH * D], int h, float* mine, int smax) {
  constexpr bool KEEP = NB <= kDuoZeilDpp;
  ZeilBest<D> best;
#pragma unroll
  for (int k = 0; k < D; ++k) best.bd[k] = 0.0f;
  if constexpr (KEEP) {
    float p[NB * D];
#pragma unroll
    for (int e = 0; e < NB * D; ++e) p[e] = duo_other(q[e]);
#pragma unroll
    for (int a = 0; a < NB; ++a) {
#pragma unroll
      for (int b = a + 1; b < NB; ++b)
        zeil_pair_cmp<D, true, false>(best, &q[a * D], &q[b * D], true, (128 * a + 2 * b) + 65 * h);
#pragma unroll
      for (int b = a; b < NB; ++b)
        zeil_pair_cmp<D, true>(best, &q[a * D], &p[b * D], (b > a) | (h == 0), (128 * a + 2 * b + 1) + 63 * h);
      if constexpr (NB > 3) __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    __syncthreads();  // (a workgroup is one wave)
#pragma unroll
    for (int s = 0; s < NB; ++s)
#pragma unroll
      for (int k = 0; k < D; ++k) mine[(2 * s + h) * D + k] = q[s * D + k];
    __syncthreads();
    const int n = 2 * smax;  // ranks in use (wave-uniform); holes are +inf
    // two pairs per pass with a best of their own each (two independent chains; the order of the merges does not
    // matter: the pair index is part of the key)
    ZeilBest<D> second;
#pragma nounroll
    for (int i = h; i + 1 < n; i += 2) {
      float pi[D];
#pragma unroll
      for (int k = 0; k < D; ++k) pi[k] = mine[i * D + k];
#pragma nounroll
      for (int j = i + 1; j < n; j += 2) {
        float pj[D], pk[D];
        const int j2 = (j + 1 < n) ? j + 1 : j;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          pj[k] = mine[j * D + k];
          pk[k] = mine[j2 * D + k];
        }
        zeil_pair2<D>(best, second, pi, pj, 64 * i + j, pi, pk, 64 * i + j + 1);  // (past the end: the last pair again, later)
      }
    }
    zeil_merge<D, false>(best, second);
  }
  {  // the partner's best
    ZeilBest<D> o;
    o.hi = (uint32_t)duo_other_i((int)best.hi);
    o.lo = (uint32_t)duo_other_i((int)best.lo);
    if constexpr (KEEP) {
#pragma unroll
      for (int k = 0; k < D; ++k) o.bd[k] = duo_other(best.bd[k]);
    }
    zeil_merge<D, KEEP>(best, o);
  }
  const bool have = best.have();
  if constexpr (!KEEP) {  // the chosen pair's difference from the parked rows
    const int i = have ? (int)((best.lo & 0xFFFFu) >> 6) : 0, j = have ? (int)(best.lo & 63u) : 0;
#pragma unroll
    for (int k = 0; k < D; ++k) best.bd[k] = mine[i * D + k] - mine[j * D + k];
    __syncthreads();  // (the image is written again by the next deal)
  }
  int lo = 0, hi = 0;
  float vlo = best.bd[0], vhi = best.bd[0];
#pragma unroll
  for (int k = 1; k < D; ++k) {
    if (best.bd[k] < vlo) { vlo = best.bd[k]; lo = k; }
    if (best.bd[k] > vhi) { vhi = best.bd[k]; hi = k; }
  }
  if (!have || lo == hi) return 0;
  return encode_mask((1u << lo) | (1u << hi));
}

// ---- the policy stream off the critical path (plain rollouts) ------------------------------------------------------
// A Philox block is ~115 instructions, 20 of them quarter-rate 32 x 32 -> 64 multiplies in a dependent chain of ten
// rounds: computed inside the step loop (one block per lane every four steps) it was a fifth of the loop's
// instructions and most of a late step's latency (a step on one slot per lane is ~40 instructions without it).  The
// words depend on (game, step) only, not on the state: a WINDOW of kDuoPreBlocks blocks per game (24 steps: four per block) is
// computed before the first step -- while the wave would otherwise only wait for its slab -- the lane's three blocks as
// three independent chains in ONE pass where the window has five or six blocks (no rows are in registers yet; as two
// chains and then one alone, the last pass -- the blocks of steps 16 .. 23, which 86 % of the headline's waves never
// play -- was the one with the least parallelism), DECODED (subset mask, axis: the decode was another ~15 instructions
// of every step) and parked in LDS, one byte per game and step; a step reads its byte (both lanes of a pair the same
// address).  Episodes longer than a window refill it between two passes over the staircase.
// Dev builds may change the window (-DHK_DUO_PRE_BLOCKS=<blocks>) and the number of independent Philox chains a lane
// runs at a time (-DHK_DUO_FILL_CHAINS=2 or 3); scripts/build_probe.sh passes both on.  A window of 16 steps (4 blocks:
// one pass of two chains, the refill for the waves that reach step 16) lost its alternation against the window of 24
// (profiles/duo_epilogue_ab.txt).
#ifndef HK_DUO_PRE_BLOCKS
#define HK_DUO_PRE_BLOCKS 6
#endif
#ifndef HK_DUO_FILL_CHAINS
#define HK_DUO_FILL_CHAINS 3
#endif
constexpr int kDuoPreBlocks = HK_DUO_PRE_BLOCKS;  // (a block serves four steps)
constexpr int kDuoFillChains = HK_DUO_FILL_CHAINS;
static_assert(kDuoPreBlocks >= 2 && kDuoPreBlocks % 2 == 0, "a pair of lanes fills two blocks at a time");
static_assert(kDuoFillChains == 2 || kDuoFillChains == 3, "two or three chains per lane");

// blocks [wb0, wb0 + nb) of the wave's games: lane (gi, h) computes blocks wb0 + h, wb0 + h + 2, ... and stores the
// DECODED actions of their steps, one byte per game and step: subset mask (D bits) | axis << 5
// CHAINS: independent Philox chains per lane and pass -- kDuoFillChains before the first step, two in a refill (the rows
// are in registers there: three chains cost (10,3), (8,4), (20,4) and the (20,3) records instantiations a wave per SIMD)
template <int D, int CHAINS = 2>
__device__ __forceinline__ void duo_policy_fill(uint8_t* act, uint64_t gg, uint32_t wb0, int nb, uint64_t seed,
                                                int host_policy, int agent_policy, int gi, int h) {
  static_assert(D <= 5 && D <= kPolicyShortDim, "an action travels as a byte; four steps per Philox block");
  auto put = [&](const U4& r, int b) {  // the four steps of block b
    int cls, axis;
    uint32_t mask;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t w = u4_word(r, k);
      policy_from_words<D>(w & 0xFFFF0000u, w << 16, host_policy, agent_policy, cls, axis, mask, 0);
      act[(4 * b + k) * kDuoGames + gi] = (uint8_t)(mask | ((uint32_t)axis << 5));
    }
  };
#pragma nounroll
  for (int i = 0; i < kDuoPreBlocks; i += 2 * CHAINS) {
    if (i >= nb) break;  // wave-uniform
    const int b0 = i + h, b1 = b0 + 2;
    if (CHAINS == 3 && i + 4 < nb) {  // (wave-uniform) three independent chains
      const int b2 = b0 + 4;
      const U4 r0 = philox4x32((uint32_t)gg, (uint32_t)(gg >> 32), wb0 + (uint32_t)b0, kStreamPolicy, seed);
      const U4 r1 = philox4x32((uint32_t)gg, (uint32_t)(gg >> 32), wb0 + (uint32_t)b1, kStreamPolicy, seed);
      const U4 r2 = philox4x32((uint32_t)gg, (uint32_t)(gg >> 32), wb0 + (uint32_t)b2, kStreamPolicy, seed);
      put(r0, b0);
      put(r1, b1);
      if (b2 < kDuoPreBlocks) put(r2, b2);
    } else if (i + 2 < nb) {  // (wave-uniform) two independent chains
      const U4 r0 = philox4x32((uint32_t)gg, (uint32_t)(gg >> 32), wb0 + (uint32_t)b0, kStreamPolicy, seed);
      const U4 r1 = philox4x32((uint32_t)gg, (uint32_t)(gg >> 32), wb0 + (uint32_t)b1, kStreamPolicy, seed);
      put(r0, b0);
      if (b1 < kDuoPreBlocks) put(r1, b1);
    } else {  // the window's last one or two blocks
      const U4 r0 = philox4x32((uint32_t)gg, (uint32_t)(gg >> 32), wb0 + (uint32_t)b0, kStreamPolicy, seed);
      if (b0 < kDuoPreBlocks) put(r0, b0);
    }
  }
}

// ---- the kernel: fused rollouts (MODE kModeRollout; kModeRolloutRec: with per-step observations / records) and
// single steps with the caller's actions (kModeStep: hk_step) -------------------------------------------------
// ACTS (plain rollouts): the kernel also writes the small per-step records (flush_records below) -- its own
// instantiation, the headline kernel carries none of it (measured: +0.4 us per 65 536-game episode as a run-time branch)
// ZEIL (plain rollouts): Zeillinger's host -- its choice depends on the state, so the policies stay inside the loop
// (duo_zeillinger on the rows in registers + the pair's Philox words), no action window; its own instantiation too.
template <int M, int D, int MODE, int HOT = kHotNone, bool ACTS = false, bool ZEIL = false>
__global__ __launch_bounds__(kWave, 2) void duo_kernel(const float* in0, int64_t in_stride0, int batch0,
                                                       const Params prm) {
  static_assert(!ACTS || MODE == kModeRollout, "the small records ride on the plain rollout");
  static_assert(!ZEIL || (MODE == kModeRollout && HOT == kHotNone && !ACTS), "Zeillinger's host: plain rollouts");
  constexpr bool kRec = MODE == kModeRolloutRec;
  constexpr bool kRoll = MODE == kModeRollout || kRec;
  // Plain rollouts of the lean shapes (DuoGeom::kLean) deal their rows level by level (duo_gather_level) and publish only
  // the rows that changed.  Not Zeillinger's host for the publish: it parks rows by rank in the image between two deals.
  constexpr bool kPartialPublish = MODE == kModeRollout && !ZEIL && DuoGeom<M, D>::kLean;
  constexpr bool kLevelDeal = MODE == kModeRollout && DuoGeom<M, D>::kLean;
  // the staircase's ladder (and the level deal's, which enters it): plain rollouts of ten slots per lane have a level of
  // seven.  Not (16,3), eight slots: with the sign-bit verdicts beside it its headline instantiation went from 85 to 111
  // VGPRs and from five waves per SIMD to four (either part alone: 85 and 78).
  constexpr bool kSigns = kDuoStepSigns && MODE == kModeRollout && !ACTS && DuoGeom<M, D>::kLean &&
                          DuoGeom<M, D>::CH >= kDuoSignsMinSlots;  // (d_newton_signs)
  using Ladder = DuoLadderT<kDuoStepSeven && MODE == kModeRollout && !ZEIL && DuoGeom<M, D>::CH >= 10>;
  using G = FastGeom<M, D>;
  constexpr int CH = DuoGeom<M, D>::CH;
  static_assert(M <= 32, "the live mask of a game travels as 32 bits");
  __shared__ __align__(16) float lds[kDuoGames * G::S];
  __shared__ float cbuf[kDuoGames * D];  // slow path only
  __shared__ float hole_row[D];          // +inf: what the deal reads for a slot without a row (duo_gather_level)
  // plain rollouts: the policy words of a window of steps (duo_policy_fill)
  // (one row more than the window: the step loop requests the NEXT step's byte while it works on this one)
  __shared__ __align__(16) uint8_t pol[(MODE == kModeRollout) ? (4 * kDuoPreBlocks + 1) * kDuoGames : 16];
  // plain rollouts of at most kWave - 1 steps: the histogram of the games' first finished steps (duo_length_counts)
  constexpr bool kHistCounts = MODE == kModeRollout && kDuoLegCounts;
  __shared__ uint32_t hist[kHistCounts ? kWave : 1];
  const int lane = threadIdx.x;
  const int h = lane & 1, gi = lane >> 1;
  const int64_t g0 = (int64_t)blockIdx.x * kDuoGames;
  const int64_t left = (int64_t)batch0 - g0;
  const int ngames = (int)(left < kDuoGames ? left : kDuoGames);
  const bool active = gi < ngames;
  const bool leader = active && h == 0;
  const int64_t g = g0 + gi;
#ifdef HK_DUO_PROBE  // dev builds (scripts/build_probe.sh): a time line per wave, written to duo_probe_rows
  // [0, 20) steps, 20 - 23 prologue, 24 scanned, 25 counts and lengths out, 26 published, 27 image read, 28 stores issued,
  // 29 counts out (plain rollouts: the counts alone, ahead of the records' flush and the lengths' store)
  __shared__ int32_t probe_buf[32];
  if (lane < 32) probe_buf[lane] = 0;
  const long long probe_t0 = wall_clock64();
  long long probe_t1 = 0, probe_t2 = 0;
  int probe_steps = 0, probe_smax = 0;
#endif
  // (the game id's load goes out BEFORE the slab's: loads return in order, and the action window -- filled while the
  // slab is in flight -- needs the id; behind the slab requests it would arrive with them: +0.9 us per episode;
  // the slab requests follow it at once; nothing touches the id before they are out)
  const bool has_ids = kRoll && prm.game_ids != nullptr;
  uint32_t raw_id = 0;  // (positions: non-negative; zero-extended below -- a sign extension would wait for the load here)
  DuoSlabRegs<M, D> slab;
  uint64_t gg;
  // (wave-uniform) the slab by LDS-DMA: contiguous, 16-byte aligned records of a shape whose image is the slab
  bool dma = false;
  if constexpr (DuoDma<M, D>::kShape) {
    // Launches with game ids keep the register path: with the id's load in flight beside LDS-DMA requests the compiler
    // waits for ALL of them where the id is first used (it does not count across the two kinds of request) -- for the
    // slab, before the action window that is meant to hide behind it.  For the same reason the two cases are two
    // branches from the id's load to its first use: joined in between, the launches WITHOUT ids waited for the register
    // the load might have been written to.
    if (has_ids) {
      if (active) raw_id = (uint32_t)prm.game_ids[g];
      __builtin_amdgcn_sched_barrier(0);
      duo_slab_issue<M, D>(slab, in0, in_stride0, g0, ngames, lane);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" : "+v"(raw_id));  // (the id has arrived: the slab's loads are counted behind it)
      gg = prm.game_offset + (uint64_t)raw_id;
    } else {
      dma = in_stride0 == G::N && ((uintptr_t)in0 & 15u) == 0;
      if (dma) duo_slab_dma<M, D>(in0 + g0 * G::N, lds, ngames, lane);
      else duo_slab_issue<M, D>(slab, in0, in_stride0, g0, ngames, lane);
      __builtin_amdgcn_sched_barrier(0);
      gg = prm.game_offset + (uint64_t)g;
    }
  } else {
    if (has_ids && active) raw_id = (uint32_t)prm.game_ids[g];
    __builtin_amdgcn_sched_barrier(0);
    duo_slab_issue<M, D>(slab, in0, in_stride0, g0, ngames, lane);
    __builtin_amdgcn_sched_barrier(0);
    gg = prm.game_offset + (has_ids ? (uint64_t)raw_id : (uint64_t)g);
  }
  // plain rollouts: the first window of policy words, computed while the slab is in flight
  uint32_t pol_b0 = prm.step_offset >> 2;  // first block of the window (wave-uniform)
  const uint32_t pol_last = (prm.steps > 0) ? (prm.step_offset + (uint32_t)prm.steps - 1u) >> 2 : pol_b0;
  if constexpr (MODE == kModeRollout && !ZEIL) {
    const uint32_t nb = pol_last - pol_b0 + 1u;
    duo_policy_fill<D, kDuoFillChains>(pol, gg, pol_b0, (int)(nb < (uint32_t)kDuoPreBlocks ? nb : (uint32_t)kDuoPreBlocks), prm.seed,
                       HOT ? (int)HK_HOST_RANDOM : prm.host_policy,
                       (HOT == kHotJax) ? (int)HK_AGENT_RANDOM
                                        : (HOT == kHotTorch) ? (int)HK_AGENT_RANDOM_LEGAL : prm.agent_policy, gi, h);
  }
#ifdef HK_DUO_PROBE
  if (lane == 0) probe_buf[21] = (int32_t)wall_clock64();  // the action window is filled
#endif
  float* mine = lds + gi * G::S;
  const float pad = (float)prm.pad;
  const unsigned flags = (HOT == kHotJax) ? (unsigned)HK_SEM_JAX : (HOT == kHotTorch) ? kHotTorchFlags : prm.flags;
  const unsigned stages = HOT ? (unsigned)(HK_STAGE_SHIFT | HK_STAGE_REPOSITION | HK_STAGE_NEWTON) : prm.stages;
  const float fill = ((flags & HK_SEM_MASK) == HK_SEM_JAX) ? -1.0f : pad;
  const int nsteps = kRoll ? prm.steps : 1;
  // plain rollouts under list semantics sort once, at the end (see hk_fast_kernel.h)
  constexpr bool kEndSort = MODE == kModeRollout && HOT == kHotNone;
  const bool end_sort = kEndSort && nsteps > 0 && (stages & HK_STAGE_NEWTON) &&
                        ((flags & HK_SEM_MASK) == HK_SEM_LIST || (flags & HK_FLAG_COMPACT_SORTED));
  bool rescale_pending = false;
  PolicyCache pcache;      // slow path (one lane per game computes)
  DuoPolicyCache dcache;
  float c[D];
  int axis_in = -1;
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = 0.0f;
  // step mode: the action loads join the slab's requests in flight (both lanes of a pair fetch them)
  RawActions<D> raw;
  const bool fetch_actions = !kRoll && (stages & HK_STAGE_SHIFT) && active;
  if (fetch_actions) fast_fetch_actions<D>(prm, g, M, raw);
  if constexpr (DuoDma<M, D>::kShape) {
    if (dma) wait_vmem_all();  // the slab is in the image
    else duo_slab_commit<M, D>(slab, lds, ngames, lane);
  } else {
    duo_slab_commit<M, D>(slab, lds, ngames, lane);
  }
  if (kLevelDeal && lane < D) hole_row[lane] = INFINITY;
  if (fetch_actions) fast_decode_actions<D>(prm, raw, c, axis_in);
  __syncthreads();
#ifdef HK_DUO_PROBE
  if (lane == 0) probe_buf[22] = (int32_t)wall_clock64();  // the slab is in LDS
#endif

  // ---- live rows, exactness guard: each lane of a pair scans its half of the game's rows, the masks meet through DPP
  // (rounds 2-4 had both lanes scan the whole game: 1.3 us of a wave's 15.7, scripts/probe_timeline.py) -----------
  uint32_t gmask;
  bool ok;
  duo_scan_half<M, D>(mine, fill, h, gmask, ok);
  if (!active) {
    gmask = 0;
    ok = true;
  }
  int np = mask_pop(gmask);
#ifdef HK_DUO_PROBE
  asm volatile("" : "+v"(np));
  if (lane == 0) probe_buf[24] = (int32_t)wall_clock64();  // scanned (the guard's vote and the wave maximum follow: probe_t1)
#endif
  int nmax = duo_wave_max<DuoGeom<M, D>::kLean && kDuoLegScan>(np, M);
  const bool exact = (fill == pad) && __all(ok) && nmax <= G::C;

  if (!exact) {
    // ---- slow path (whole wave): the pair's first lane runs the exact generic routines on the image ----------
    float* cs = cbuf + gi * D;
    np = leader ? num_points<float>(mine, M, D) : 2;
    int length = (np < 2) ? 0 : -1;
    if (kRoll && prm.count_ws) {
      const unsigned long long b0 = __ballot(leader && np < 2);
      if (lane == 0) count_add(prm.count_ws + blockIdx.x, (uint32_t)__popcll(b0));
    }
    for (int t = 0; t < nsteps; ++t) {
      int axis = axis_in, cls = 0;
      if (kRec && prm.obs_out) {
        __syncthreads();
        duo_store_slab<M, D, 2>(lds, (float*)prm.obs_out + (int64_t)t * prm.batch * G::N, (int64_t)G::N, g0, ngames, lane);
        __syncthreads();
      }
      if (kRoll) {
        uint32_t mask;
        const int zc = (prm.host_policy == HK_HOST_ZEILLINGER && leader) ? zeillinger_game<float>(mine, prm.m, prm.d) : 0;
        fast_policy<D>(prm, gg, prm.step_offset + (uint32_t)t, pcache, cls, axis, mask, zc);
        if (leader)
          for (int k = 0; k < prm.d; ++k) cs[k] = (float)((mask >> k) & 1u);
      } else if ((stages & HK_STAGE_SHIFT) && leader) {
        load_coords<float>(prm, g, cs);
      }
      const bool prev_done = np < 2;
      if (leader) {
        stages_game<float>(mine, prm.m, prm.d, cs, axis, pad, stages, flags);
        np = num_points<float>(mine, prm.m, prm.d);
      }
      const bool done = np < 2;
      if (done && length < 0) length = t + 1;
      if (kRoll && prm.count_ws) {
        const unsigned long long bd = __ballot(leader && done);
        if (lane == 0) count_add(prm.count_ws + (size_t)(t + 1) * prm.count_stride + blockIdx.x, (uint32_t)__popcll(bd));
      }
      if ((kRec || ACTS) && leader) {  // (ACTS: plain rollouts with the small records, flush_records below)
        const int64_t at = (int64_t)t * prm.batch + g;
        if (prm.r_host_class_out) prm.r_host_class_out[at] = cls;
        if (prm.r_axis_out) prm.r_axis_out[at] = axis;
        if (prm.r_done_out) prm.r_done_out[at] = done;
        if (prm.r_reward_out) prm.r_reward_out[at] = prm.reward_sign * (float)(done && !prev_done);
      }
      if (!kRoll && leader) {
        if (prm.done_out) prm.done_out[g] = done;
        if (prm.prev_done_out) prm.prev_done_out[g] = prev_done;
        if (prm.reward_out) prm.reward_out[g] = prm.reward_sign * (float)(done && !prev_done);
        if (prm.num_points_out) prm.num_points_out[g] = np;
      }
    }
    if (kRoll && leader && prm.game_length_out) prm.game_length_out[g] = length;
    __syncthreads();
    duo_store_slab<M, D>(lds, (float*)prm.out, prm.out_stride, g0, ngames, lane);
    return;
  }

  // ---- the pair's rows ----------------------------------------------------------------------------------
  // plain rollouts publish only what changed (see the end of the kernel): the rows that are live now are parked in the
  // slow path's buffer, which this path does not use otherwise -- not a register held across the loop
  if (kPartialPublish && h == 0) reinterpret_cast<uint32_t*>(cbuf)[gi] = gmask;
  int smax = (nmax + 1) >> 1;
#ifdef HK_DUO_PROBE
  probe_t1 = wall_clock64();
  probe_smax = smax;
#endif
  float q[CH * D];
  if constexpr (!kLevelDeal) {  // (the level deal writes every slot)
#pragma unroll
    for (int e = 0; e < CH * D; ++e) q[e] = INFINITY;
  }
  duo_gather<M, CH, D, kLevelDeal, Ladder>(q, mine, hole_row, gmask, smax, h);
#ifdef HK_DUO_PROBE
  {
    float sink = 0.0f;
#pragma unroll
    for (int e = 0; e < CH * D; ++e) sink += (q[e] < INFINITY) ? q[e] : 0.0f;
    asm volatile("" : "+v"(sink));
    if (lane == 0) probe_buf[23] = (int32_t)wall_clock64();  // the rows are in registers
  }
#endif
  if (!active) np = 2;
  int length = (np < 2) ? 0 : -1;
  // (wave-uniform) the counts of every step, step 0 included, in closed form after the loop
  const bool hist_counts = kHistCounts && nsteps < kWave;
  if (kRoll && prm.count_ws && !hist_counts) {
    const unsigned long long b0 = __ballot(leader && np < 2);
    if (lane == 0) count_add(prm.count_ws + blockIdx.x, (uint32_t)__popcll(b0));
  }
  uint32_t* count_slot = (kRoll && prm.count_ws) ? prm.count_ws + blockIdx.x : nullptr;
  uint32_t count_stride = prm.count_stride;
  uint32_t step0 = prm.step_offset;
  uint64_t seed = prm.seed;
  int host_policy = HOT ? (int)HK_HOST_RANDOM : prm.host_policy;
  int agent_policy = (HOT == kHotJax) ? (int)HK_AGENT_RANDOM
                                      : (HOT == kHotTorch) ? (int)HK_AGENT_RANDOM_LEGAL : prm.agent_policy;
  if (HOT)
    asm volatile("" : "+s"(count_slot), "+s"(count_stride), "+s"(step0), "+s"(seed));
  else
    asm volatile("" : "+s"(count_slot), "+s"(count_stride), "+s"(step0), "+s"(seed), "+s"(host_policy),
                 "+s"(agent_policy));
  // Plain rollouts write the small records (host class, axis, done, reward) too, when asked: they are a function of the
  // window's action bytes and of the game's first finished step, so no step stores them -- they go out per window
  // (before it moves, and after the last step), lane = (step within a pair, game of the wave): 128-B runs per step and
  // field (hk_quadroll_kernel.h does the same on 16 games).  Observations stay with kModeRolloutRec / the four-lane kernel.
  static_assert(kDuoGames == 32 && kWave == 64, "flush_records: two steps of the wave's games per instruction");
  int32_t* rec_cls = ACTS ? prm.r_host_class_out : nullptr;
  int32_t* rec_axis = ACTS ? prm.r_axis_out : nullptr;
  uint8_t* rec_done = ACTS ? prm.r_done_out : nullptr;
  float* rec_reward = ACTS ? prm.r_reward_out : nullptr;
  int64_t rec_batch = prm.batch;
  float rec_sign = prm.reward_sign;
  if constexpr (ACTS)  // (pinned: left to the compiler the stores' address arithmetic ends in an illegal VGPR -> SGPR copy)
    asm volatile("" : "+s"(rec_cls), "+s"(rec_axis), "+s"(rec_done), "+s"(rec_reward), "+s"(rec_batch), "+s"(rec_sign));
  constexpr bool want_small = ACTS;
  int t_rec = 0;  // the records of steps < t_rec are written
  auto flush_records = [&](int t_end) {  // (t_end: wave-uniform)
    if (t_rec < t_end) {
      const int gsel = lane & (kDuoGames - 1), sub = lane >> 5;
      const int lg = __shfl(length, gsel * 2);  // the game's first finished step (0: from the start, -1: not yet)
      const bool gok = gsel < ngames;
      const int64_t off = (int64_t)sub * rec_batch + gsel;
      const uint8_t* w = pol + (int)(step0 + (uint32_t)t_rec - (pol_b0 << 2)) * kDuoGames + lane;
      for (int ta = t_rec; ta < t_end; ta += 2, w += 2 * kDuoGames) {
        const int tt = ta + sub;
        if (gok && tt < t_end) {
          const uint32_t a = *w;
          const int64_t row = (int64_t)ta * rec_batch + g0;  // (scalar)
          if (rec_cls) (rec_cls + row)[off] = encode_mask(a & 31u);
          if (rec_axis) (rec_axis + row)[off] = (int32_t)(a >> 5);
          if (rec_done) (rec_done + row)[off] = lg >= 0 && tt + 1 >= lg;
          if (rec_reward) (rec_reward + row)[off] = rec_sign * (float)(lg >= 1 && tt + 1 == lg);
        }
      }
    }
    t_rec = t_end;
  };
  if constexpr (MODE == kModeRollout) {
    // ---- plain rollouts: a STAIRCASE of loops, one per bucket of slots per lane, entered from the top down.  smax
    // never grows, so the wave walks down the stairs once; each loop is straight-line for its own bucket -- no
    // per-step dispatch over the buckets, and only the slots the bucket covers are loop-carried registers (a single
    // loop over all buckets moves the whole row array at every back edge: 16 v_mov_b64 per step at (20,3)). -------
    static_assert(CH <= 6 || CH % 2 == 0, "bucket ladder: 1..6 or 1..8, then even numbers");
    // The wave's votes are scalar: a ballot, ANDed with the mask of the lanes that speak for a game (both lanes of a
    // pair: `amask`; its first lane: `lmask`), and a branch on the AND's own condition code.
    uint64_t amask = duo_ballot(active), lmask = duo_ballot(leader);
    asm volatile("" : "+s"(amask), "+s"(lmask));
    // A finished game stays finished, so its first finished step is the number of steps it was NOT finished after: a
    // counter on the pair's first lane (the only one read), one add per step on the not-done mask the step has anyway.
    // Games finished at entry start at -1, so that they read 0; a game never finished has counted every step.
    int open_steps = (np < 2) ? -1 : 0;
    auto length_at = [&](int tt) { return open_steps == tt ? -1 : open_steps + 1; };  // after tt steps (wave-uniform)
    int t = 0;
    bool stop = false;  // (set under a scalar branch only)
    while (t < nsteps && !stop) {  // one pass per window of policy words (episodes of up to 24 steps: one pass)
    if (!ZEIL && (uint32_t)((step0 + (uint32_t)t) >> 2) - pol_b0 >= (uint32_t)kDuoPreBlocks) {
      if constexpr (want_small) {
        length = length_at(t);
        flush_records(__builtin_amdgcn_readfirstlane(t));
      }
      __syncthreads();
      pol_b0 = (step0 + (uint32_t)t) >> 2;
      const uint32_t nb = pol_last - pol_b0 + 1u;
      duo_policy_fill<D>(pol, gg, pol_b0, (int)(nb < (uint32_t)kDuoPreBlocks ? nb : (uint32_t)kDuoPreBlocks), seed,
                         host_policy, agent_policy, gi, h);
      __syncthreads();
    }
    // last step (exclusive) the window covers
    const uint32_t wend_abs = (pol_b0 + (uint32_t)kDuoPreBlocks) << 2;
    const int tw = (!ZEIL && wend_abs - step0 < (uint32_t)nsteps) ? (int)(wend_abs - step0) : nsteps;
    // the action byte of step t, requested one step ahead: the LDS round trip (it opened every step: ds_read, wait)
    // runs behind the previous step's arithmetic
    uint32_t a_next = ZEIL ? 0u : pol[(int)(step0 + (uint32_t)t - (pol_b0 << 2)) * kDuoGames + gi];
    Levels<Ladder, CH>::run([&](auto nbc, auto loc) {
      constexpr int NB = decltype(nbc)::value, LO = decltype(loc)::value;
      if (!((smax > LO || LO == 0) && t < tw && !stop)) return;  // (a wave of empty games has smax 0: the last loop's)
#ifndef HK_NO_SETPRIO
      // The launch ends with its slowest waves -- the ones that start in a wide bucket or run many steps -- and the two
      // waves of a SIMD share its issue slots by priority, then age: a wave in a wide bucket outranks its neighbour
      // (who is ahead anyway), and so does one that is still running late in the episode.
      if (t >= 10) __builtin_amdgcn_s_setprio(3);
      else if constexpr (NB >= 6) __builtin_amdgcn_s_setprio(3);
      else if constexpr (NB >= 4) __builtin_amdgcn_s_setprio(2);
      else if constexpr (NB >= 2) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
#endif
      // steps [t, tend) at this level: ONE exit test per step; the rare ways out -- the wave's widest game fits the next
      // level down, every game sits at its fixed point -- pull the loop's end in from inside their own branch
      auto play = [&](int tend) {
        while (t < tend) {
          uint32_t mask;
          int axis;
          if constexpr (ZEIL) {
            // (a game with fewer than two rows has no pair: class 0 -- a wave of finished games skips the test)
            static_assert(NB <= kDuoZeilDpp || 2 * NB <= M, "the rolled pair loop parks ranks 0 .. 2 NB - 1 in the game's M rows");
            const int zc = (duo_ballot(np >= 2) & amask) != 0 ? duo_zeillinger<CH, D, NB>(q, h, mine, smax) : 0;
            uint32_t ra, rb;
            int cls;
            duo_policy_words(gg, step0 + (uint32_t)t, seed, dcache, h, ra, rb);
            policy_from_words<D>(ra, rb, host_policy, agent_policy, cls, axis, mask, zc);
          } else {
            const uint32_t a = a_next;
            a_next = pol[(int)(step0 + (uint32_t)t + 1u - (pol_b0 << 2)) * kDuoGames + gi];  // (past the window: not used)
            mask = a & 31u;
            axis = (int)(a >> 5);
          }
          const unsigned st = (end_sort && t + 1 == nsteps) ? (stages & ~(unsigned)HK_STAGE_RESCALE) : stages;
          rescale_pending = end_sort && t + 1 == nsteps && (stages & HK_STAGE_RESCALE);
          const int np_new = d_stages<CH, D, NB, true, (NB == 1), kSigns>(q, c, axis, np, h, flags, st, mask);
#ifdef HK_DUO_PROBE
          if (lane == 0 && t == 0) probe_buf[20] = (int32_t)wall_clock64();  // step 0: the stages are done
#endif
          // (the finished-game counts: ballots over the games' first finished steps after the loop -- a finished game
          // stays finished --, not an atomic per step in here)
          if constexpr (NB == 1) {
            // one slot per lane: a game is not finished while both lanes of its pair hold a row -- the ballot of the live
            // slots against itself one lane up, on the pair's first lane; the number of rows is never materialised
            const uint64_t live = duo_ballot(q[0] < INFINITY);
            const uint64_t open = live & (live >> 1) & lmask;
            open_steps += __builtin_amdgcn_inverse_ballot_w64(open) ? 1 : 0;
            np = __builtin_amdgcn_inverse_ballot_w64(open | (open << 1)) ? 2 : 0;  // (Zeillinger's host and the torch shift read it)
            // Fixed point: a game that is down to ONE point sitting at the origin (or to none) does not change any
            // more -- whatever the subset and the axis: the shift adds zeros, reposition / rescale find nothing to move,
            // the Newton stage has nothing to compare.  Once every game of the wave is there (a game reaches it one
            // step after it ends when reposition is on; the mean game lasts 5 steps, the longest of 32 about 13), the
            // rest of the episode changes nothing.
            if (open == 0) {
              // (the slot holds the game's point, a hole, or nothing; coordinates are bit patterns in [+0, +inf]: the
              // point is at the origin when the OR of its words is zero)
              uint32_t any_bits = __float_as_uint(q[0]);
#pragma unroll
              for (int k = 1; k < D; ++k) any_bits |= __float_as_uint(q[k]);
              if ((duo_ballot(any_bits != 0u) & live & amask) == 0) {
                stop = true;
                tend = 0;
              }
            }
          } else {
            np = np_new;
            open_steps += (leader && np >= 2) ? 1 : 0;
            // re-deal the rows when the widest game of the wave fits fewer slots per lane
            if ((duo_ballot(np >= 2 * smax - 1) & amask) == 0) {
              // (the test for the last step stays inside: pinned, or the two conditions are merged into one mask and the
              // branch on the vote's own condition code is lost)
              int left = nsteps - 1 - t;
              asm volatile("" : "+s"(left));
              if (left > 0) {
                __syncthreads();
                if constexpr (kLevelDeal) {  // (LO < smax <= NB: this level's straight-line deal, no dispatch)
                  gmask = lanes_or<2>(duo_scatter_level<CH, D, NB>(q, mine, gmask, h));
                  __syncthreads();
                  nmax = duo_wave_max<DuoGeom<M, D>::kLean && kDuoLegScan>(active ? np : 0, 2 * smax - 2);
                  smax = (nmax + 1) >> 1;
                  duo_gather_level<CH, D, NB>(q, mine, hole_row, gmask, h);  // slots [smax, NB) become holes again
                } else {
                  gmask = duo_scatter<M, CH, D, NB>(q, mine, gmask, smax, h);
                  __syncthreads();
                  const int sprev = smax;
                  nmax = duo_wave_max<DuoGeom<M, D>::kLean && kDuoLegScan>(active ? np : 0, 2 * smax - 2);
                  smax = (nmax + 1) >> 1;
                  duo_gather_slots<M, CH, D, NB>(q, mine, gmask, sprev, h);  // slots [smax, sprev) become holes again
                }
                tend = smax <= LO ? 0 : tend;  // the next level down takes over
              }
            }
          }
#ifdef HK_DUO_PROBE  // per-step stamps: the clock and the slots per lane after the step
          if (lane == 0 && t < 24) probe_buf[t] = (int32_t)((((uint32_t)wall_clock64()) << 4) | (uint32_t)(smax & 15));
#endif
          ++t;
        }
      };
      if constexpr (NB == 1) {
        // the last level raises its priority at step 10: two loops, not a compare in every step
        play(tw < 10 ? tw : 10);
        if (t < tw && !stop) {
#ifndef HK_NO_SETPRIO
          __builtin_amdgcn_s_setprio(3);
#endif
          play(tw);
        }
      } else {
        play(tw);
      }
    });
    }
    length = length_at(t);
#ifdef HK_DUO_PROBE
    probe_steps = t;
    probe_t2 = wall_clock64();
#endif
    // games whose first finished step is <= s: every step s >= 0 from the histogram, or -- episodes of kWave steps and
    // more -- every step s >= 1 by ballots (s = 0 was counted at entry)
    if (count_slot) {
      if (hist_counts) duo_length_counts(hist, count_slot, count_stride, nsteps, leader, length, lane);
      else add_length_counts(count_slot, count_stride, 1, nsteps, leader, length, lane);
    }
#ifdef HK_DUO_PROBE
    if (lane == 0) probe_buf[29] = (int32_t)wall_clock64();  // the counts are out
#endif
    if constexpr (want_small) {  // window by window up to the last step (the loop may have left at a fixed point)
      for (;;) {
        const uint32_t wend = ((pol_b0 + (uint32_t)kDuoPreBlocks) << 2) - step0;  // steps (from 0) the window reaches
        const int te = __builtin_amdgcn_readfirstlane((wend < (uint32_t)nsteps) ? (int)wend : nsteps);
        flush_records(te);
        if (te >= nsteps) break;
        __syncthreads();
        pol_b0 = (step0 + (uint32_t)te) >> 2;
        const uint32_t nb = pol_last - pol_b0 + 1u;
        duo_policy_fill<D>(pol, gg, pol_b0, (int)(nb < (uint32_t)kDuoPreBlocks ? nb : (uint32_t)kDuoPreBlocks), seed,
                           host_policy, agent_policy, gi, h);
        __syncthreads();
      }
    }
  }
  const bool want_obs = kRec && prm.obs_out != nullptr;
  const bool want_records = kRec && (prm.r_host_class_out || prm.r_axis_out || prm.r_done_out || prm.r_reward_out);
  for (int t = 0; MODE != kModeRollout && t < nsteps; ++t) {  // single steps and recording rollouts
    int axis = axis_in, cls = 0;
    if (want_obs) {  // state before the step: rebuild the image, store it coalesced
      __syncthreads();
      if (h == 0) fill_image<M, D>(mine, pad);
      __syncthreads();
      duo_scatter<M, CH, D>(q, mine, gmask, smax, h);
      __syncthreads();
      duo_store_slab<M, D, 2>(lds, (float*)prm.obs_out + (int64_t)t * prm.batch * G::N, (int64_t)G::N, g0, ngames, lane);
    }
    uint32_t mask = 0;
    if (kRoll) {
      uint32_t ra, rb;
      duo_policy_words(gg, step0 + (uint32_t)t, seed, dcache, h, ra, rb);
      policy_from_words<D>(ra, rb, host_policy, agent_policy, cls, axis, mask, 0);
    }
    const bool prev_done = np < 2;
    // (rollouts: the subset is the policy's 0/1 mask -- the shift as selects, see b_shift_mask)
    const unsigned st = (end_sort && t + 1 == nsteps) ? (stages & ~(unsigned)HK_STAGE_RESCALE) : stages;
    rescale_pending = end_sort && t + 1 == nsteps && (stages & HK_STAGE_RESCALE);
    np = DuoStagesFor<CH, D, 1, kRoll>::run(q, smax, c, axis, np, h, flags, st, mask);
    if (!active) np = 2;
    const bool done = np < 2;
    if (done && length < 0) length = t + 1;
    if (!kRoll && leader) {
      if (prm.done_out) prm.done_out[g] = done;
      if (prm.prev_done_out) prm.prev_done_out[g] = prev_done;
      if (prm.reward_out) prm.reward_out[g] = prm.reward_sign * (float)(done && !prev_done);
      if (prm.num_points_out) prm.num_points_out[g] = np;
    }
    if (want_records && leader) {
      const int64_t at = (int64_t)t * prm.batch + g;
      if (prm.r_host_class_out) prm.r_host_class_out[at] = cls;
      if (prm.r_axis_out) prm.r_axis_out[at] = axis;
      if (prm.r_done_out) prm.r_done_out[at] = done;
      if (prm.r_reward_out) prm.r_reward_out[at] = prm.reward_sign * (float)(done && !prev_done);
    }
    const unsigned long long bd = __ballot(leader && done);
    if (count_slot && lane == 0) count_add(count_slot + (size_t)(t + 1) * count_stride, (uint32_t)__popcll(bd));
    // Fixed point: a game that is down to ONE point sitting at the origin (or to none) does not change any more --
    // whatever the subset and the axis: the shift adds zeros, reposition / rescale find nothing to move, the Newton
    // stage has nothing to compare.  Once every game of the wave is there (a game reaches it one step after it ends
    // when reposition is on; the mean game lasts 5 steps, the longest of 32 about 13), the rest of the episode is
    // the finished-game counts, added in closed form.
    if (MODE == kModeRollout && smax == 1 && bd == __ballot(leader) && t + 1 < nsteps) {
      // (one slot per lane left: a lane holds the game's point, a hole, or nothing)
      bool still = true;
#pragma unroll
      for (int k = 0; k < D; ++k) still &= (q[k] == 0.0f);
      still |= !(q[0] < INFINITY);
      if (!__any(active && !still)) {
        if (count_slot && lane == 0)
          for (int tt = t + 1; tt < nsteps; ++tt) count_add(count_slot + (size_t)(tt + 1) * count_stride, (uint32_t)__popcll(bd));
        break;
      }
    }
    // re-deal the rows when the widest game of the wave fits fewer slots per lane
    if (t + 1 < nsteps && !__any(active && ((np + 1) >> 1) >= smax)) {
      __syncthreads();
      gmask = duo_scatter<M, CH, D>(q, mine, gmask, smax, h);
      __syncthreads();
      const int sprev = smax;
      nmax = duo_wave_max<DuoGeom<M, D>::kLean && kDuoLegScan>(active ? np : 0, 2 * smax - 2);
      smax = (nmax + 1) >> 1;
      duo_gather_slots<M, CH, D>(q, mine, gmask, sprev, h);  // slots [smax, sprev) become holes again
    }
  }
  if (kRoll && leader && prm.game_length_out) prm.game_length_out[g] = length;
#ifdef HK_DUO_PROBE
  if (lane == 0) probe_buf[25] = (int32_t)wall_clock64();  // the counts and the lengths are out
#endif

  // ---- publish ---------------------------------------------------------------------------------------------------
  __syncthreads();
  if (kPartialPublish && !end_sort) {
    // Rows keep their slots, and on this path every row of the loaded image was live or exactly the padding row
    // (duo_scan_half, `exact`: fill == pad); the re-deals wrote live slots only.  So the image already holds the padding
    // wherever a row was never live: the live rows go back to their slots, and the rows that were live at the start and
    // are not any more take the padding -- no refill of the whole image, one barrier less.
    const uint32_t alive = duo_scatter<M, CH, D>(q, mine, gmask, smax, h);
    duo_pad_rows<D>(mine, reinterpret_cast<const uint32_t*>(cbuf)[gi] & ~alive, pad, h);
  } else {
    // pad everywhere, live rows back in their slots (list semantics: in their rank's)
    if (h == 0) fill_image<M, D>(mine, pad);
    __syncthreads();
    if (kEndSort && end_sort) {
      int rank[CH];
      duo_ranks_first<CH, D>(q, smax, rank);
      if (rescale_pending) rescale<2, CH, D, CH>(q, flags);
      duo_scatter_ranked<CH, D>(q, mine, rank, smax);
    } else {
      duo_scatter<M, CH, D>(q, mine, gmask, smax, h);
    }
  }
  __syncthreads();
#ifdef HK_DUO_PROBE
  if (lane == 0) probe_buf[26] = (int32_t)wall_clock64();  // published: the image holds the final state
#endif
  // (plain rollouts: write-through for the lean shapes; at (20,4) the descriptor's registers cost the third wave: nt)
  constexpr int kFinalStore = MODE != kModeRollout ? kStorePlain : DuoGeom<M, D>::kLean ? kStoreWT : kStoreNT;
  duo_store_slab<M, D, DuoGeom<M, D>::QH, kFinalStore>(lds, (float*)prm.out, prm.out_stride, g0, ngames,
                                                       lane HK_DUO_PROBE_ARG(probe_buf + 27));
#ifdef HK_DUO_PROBE
  if (kRoll && lane == 0 && blockIdx.x < (unsigned)kDuoProbeWaves) {
    int32_t* w = duo_probe_rows + blockIdx.x * kDuoProbeRow;
    w[0] = (int32_t)probe_t0;
    w[1] = (int32_t)probe_t1;
    w[2] = (int32_t)probe_t2;
    w[3] = (int32_t)wall_clock64();
    w[4] = probe_steps;
    w[5] = probe_smax;
    w[6] = (int32_t)blockIdx.x;
    w[7] = (int32_t)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));  // HW_ID
    for (int i = 0; i < 32; ++i) w[8 + i] = probe_buf[i];
  }
#endif
}

// ---- host side -----------------------------------------------------------------------------------------------
// The instantiation duo_kernel<M, D, mode, hot, acts, zeil> that serves a request (mode < 0: none)
struct DuoVariant {
  int mode = -1;
  int hot = kHotNone;
  bool acts = false;  // the small records ride on the plain rollout (flush_records)
  bool zeil = false;
  bool none() const { return mode < 0; }
  constexpr int key() const { return mode < 0 ? -1 : ((mode * 8 + hot) * 2 + acts) * 2 + zeil; }
};
inline DuoVariant duo_variant(const Params& prm) {
  if (prm.mode == kModeStep) {
    // take_actions as the JAX trainer configures it (jax/util.py:83-125 with reposition, without rescale)
    const bool hot = prm.flags == HK_SEM_JAX && prm.stages == (HK_STAGE_SHIFT | HK_STAGE_REPOSITION | HK_STAGE_NEWTON);
    return {kModeStep, hot ? kHotJax : kHotNone};
  }
  if (prm.mode != kModeRollout) return {};
  if (prm.obs_out) return {kModeRolloutRec};
  if (prm.host_policy == HK_HOST_ZEILLINGER) return {kModeRollout, kHotNone, false, true};
  const int hot = fast_hot_config(prm);
  // (the small records alone ride on the plain rollout kernels: ACTS)
  if (small_records(prm)) return {kModeRollout, hot == kHotJax ? kHotJax : kHotNone, true};
  return {kModeRollout, hot};
}

inline int64_t duo_grid(const Params& prm) { return workgroups(prm.batch, kDuoGames); }

// steps and rollouts the two-lane kernel serves: those of a register-resident specialisation (fast_supported) of up to
// 32 rows, without class / feature outputs
inline bool duo_supported(const Params& prm, int dtype) {
  if (duo_variant(prm).none() || prm.m > 32) return false;
  if (prm.mode == kModeStep && (prm.class_out || (prm.stages & kStageFeatureSorts))) return false;
  // Zeillinger's host: plain rollouts (duo_kernel<..., ZEIL>); with records the one-lane kernel
  if (prm.mode == kModeRollout && prm.host_policy == HK_HOST_ZEILLINGER && any_records(prm)) return false;
  // sorted + compacted output: plain rollouts only (they sort once, at the end)
  if (sorted_output(prm) && (prm.mode != kModeRollout || any_records(prm))) return false;
  return fast_supported(prm, dtype);
}

template <int M, int D>
int launch_duo_t(Params prm, hipStream_t stream) {
  prm.games_per_block = kDuoGames;
  const auto go = [&](auto kernel) {
    return launch_kernel(kernel, duo_grid(prm), kWave, 0, stream, (const float*)prm.in, prm.in_stride, prm.batch, prm);
  };
  constexpr auto key = [](int mode, int hot = kHotNone, bool acts = false, bool zeil = false) {
    return DuoVariant{mode, hot, acts, zeil}.key();
  };
  switch (duo_variant(prm).key()) {  // one line per compiled instantiation
    case key(kModeRolloutRec): return go(duo_kernel<M, D, kModeRolloutRec>);
    case key(kModeRollout, kHotNone, false, true): return go(duo_kernel<M, D, kModeRollout, kHotNone, false, true>);
    case key(kModeRollout, kHotJax, true): return go(duo_kernel<M, D, kModeRollout, kHotJax, true>);
    case key(kModeRollout, kHotNone, true): return go(duo_kernel<M, D, kModeRollout, kHotNone, true>);
    case key(kModeStep, kHotJax): return go(duo_kernel<M, D, kModeStep, kHotJax>);
    case key(kModeStep): return go(duo_kernel<M, D, kModeStep>);
    case key(kModeRollout, kHotJax): return go(duo_kernel<M, D, kModeRollout, kHotJax>);
    case key(kModeRollout, kHotTorch): return go(duo_kernel<M, D, kModeRollout, kHotTorch>);
    case key(kModeRollout): return go(duo_kernel<M, D, kModeRollout>);
  }
  return HK_ERR_UNSUPPORTED;  // (duo_variant names no other)
}

// instantiated next to the one-lane specialisations (hk_fast_spec.hip); the dispatcher lives in the main unit
#ifndef HK_SPEC_TU
#define HK_X(M_, D_) extern template int launch_duo_t<M_, D_>(Params, hipStream_t);
HK_FAST_SPECS(HK_X)
#undef HK_X

inline int launch_duo(const Params& prm, hipStream_t stream) {
  return for_fast_spec(prm.m, prm.d, (int)HK_ERR_UNSUPPORTED, [&](auto s) { return launch_duo_t<s.M, s.D>(prm, stream); });
}
#endif

}  // namespace hk
