/*
 * hironaka_hip_spivakovsky.h -- Spivakovsky's host (hironaka/host.py:130-290) and RandomSpivakovsky (host.py:293-354)
 * as an operator, an addition within ABI 6 that a consumer detects by its symbol; part of the C ABI of hironaka_hip.h,
 * which includes this file; HK_F32 / HK_F64 and the status codes are defined there.  The entry point has no counterpart
 * in the CPU oracle: the Python binding lists it in hironaka_amd/_abi.py SPIVAKOVSKY_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 *
 * mask_out[g] = the subset `host` picks on game g as a bit mask (bit k <-> coordinate k).  A game is `max_points` rows
 * of `dim` coordinates at points + g*stride, in list semantics: a row with coordinate 0 >= 0 is a point (NaN is a
 * hole), read in row order; holes may sit anywhere.  A mask, not a class id (hk_decode_host_class): Spivakovsky's subset
 * may hold 0 or 1 coordinates, as the reference's does, and those have no class.  Fewer than 2 points give 0.
 *
 * HK_HOST_SPIVAKOVSKY  Values are doubles (a float32 state is widened first; the reference computes on Python floats),
 *   sums run left to right from 0, divisions are IEEE.  act = all coordinates, alive = all points, res = {}.  At most
 *   dim times, while alive is not empty:
 *     mn[k] = min over alive of coordinate k; mv = v - mn.  An alive row with mv == 0 on all of act ends the loop.
 *     s_i = the sum of mv_i over act; md = min s_i; S = the k in act with mv_i[k] > 0 in a row with s_i == md.
 *     res |= S; I = act \ S.  q = mv / md, t = the sum of q over S: a row stays alive only if t < 0.999, and then its
 *     coordinates k in I become q[k] / (1 - t).  If I is not empty, act = I.
 *   If alive is not empty then, the last step: over r = 1 .. |act| - 1 and the subsets of r active coordinates in
 *   lexicographic order of their sorted coordinates, the first one on which no alive row's sum (of its values as they
 *   stand) is < 0.999 is added to res; if there is none, nothing is.
 *   The contract is finite, non-negative points; on any other input the call still ends and reads and writes inside the
 *   game.
 * HK_HOST_RANDOM_SPIVAKOVSKY  supports = the sets of nonzero coordinates (NaN nonzero, -0.0 zero).  The candidates are
 *   the c within the `dim` coordinates with |c| >= 2 that meet every support, of the smallest such size, in ascending
 *   order as integers; the result is candidate number (word * n) >> 32 of the n, word = the first word of
 *   philox4x32(game lo, game hi, step, 5, seed) with game = game_offset + g.  0 when no c meets every support (a zero
 *   row), where the reference raises.  (The reference built with its default dim = 16 may also return coordinates the
 *   game does not have; this is the reference built with dim = `dim`.)  seed, game_offset and step are ignored by
 *   HK_HOST_SPIVAKOVSKY.
 *
 * dim 2..6, max_points 1..64, stride >= max_points*dim, HK_F32 / HK_F64, host 6..7.  Status, decided before any launch
 * and in this order: batch < 0, max_points < 1 or dim < 2 HK_ERR_SHAPE; another dtype, another host (the codes of
 * hk_host_select included), a larger dim or max_points HK_ERR_UNSUPPORTED; batch == 0 HK_OK with nothing launched; a
 * NULL pointer HK_ERR_NULL; a smaller stride HK_ERR_SHAPE; points not aligned to its element or mask_out to 4 bytes
 * HK_ERR_ALIGN.  hk_host_select, hk_search_depth and the other fixed-host operators refuse both codes.
 * Reads each game once, writes 4 B. */
#ifndef HIRONAKA_HIP_SPIVAKOVSKY_H
#define HIRONAKA_HIP_SPIVAKOVSKY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HK_HOST_SPIVAKOVSKY 6        /* host.py:130-290  Spivakovsky       */
#define HK_HOST_RANDOM_SPIVAKOVSKY 7 /* host.py:293-354  RandomSpivakovsky */

int hk_spivakovsky_select(const void* points, int64_t stride, int32_t* mask_out, int batch, int max_points, int dim,
                          int dtype, int host, uint64_t seed, uint64_t game_offset, uint32_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_SPIVAKOVSKY_H */
