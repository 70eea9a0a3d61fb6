/*
 * hironaka_hip_hosts.h -- the fixed hosts of hironaka/host.py as an operator (ABI 6), part of the C ABI of
 * hironaka_hip.h, which includes this file; the HK_HOST_* codes, HK_F32 / HK_F64 and the status codes are defined
 * there.  Its entry points have no counterpart in the CPU oracle (oracle/), which restates the entry points of
 * hironaka_hip.h itself: the Python binding lists them in hironaka_amd/_abi.py DEVICE_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 */
#ifndef HIRONAKA_HIP_HOSTS_H
#define HIRONAKA_HIP_HOSTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a deterministic host's choice as its own operator (ABI 6; hironaka/host.py select_coord on ListPoints) ----
 * class_out[g] = the class id (hk_decode_host_class) of the subset `host` picks on game g, or -1 = no subset.  A game
 * is `max_points` rows of `dim` coordinates at points + g*stride, in list semantics: a row with coordinate 0 >= 0 is a
 * point (NaN is a hole), read in row order; holes may sit anywhere.
 *   HK_HOST_ALL_COORD         every coordinate (ncls - 1), whatever the game holds
 *   HK_HOST_ZEILLINGER        bit for bit hk_zeillinger(..., HK_SEM_LIST)
 *   HK_HOST_ZEILLINGER_LEX    Zeillinger's key (L, S) over the pairs i<j; among the pairs of the smallest key, the
 *                             lexicographically smallest [first argmin, first argmax] of P_i - P_j ([0, 1] if equal)
 *   HK_HOST_WEAK_SPIVAKOVSKY  supports = the sets of nonzero coordinates (NaN nonzero, -0.0 zero), U their union: the
 *                             smallest c within U, |c| >= 2, meeting every support; first in lexicographic order of
 *                             its sorted coordinates
 *   HK_HOST_MIN_HITTING       the smallest (|c|, c) over all c, |c| >= 2, meeting every support
 * -1: fewer than 2 points; for the two hitting-set hosts also a zero row, and for HK_HOST_WEAK_SPIVAKOVSKY |U| < 2
 * (where the reference returns no subset or its sentinel 65536; no Newton-reduced state with >= 2 points gets there).
 * dim 2..6, max_points 1..64, stride >= max_points*dim, HK_F32 / HK_F64, host 1..5; a larger dim or max_points, another
 * dtype or host (HK_HOST_RANDOM included) is HK_ERR_UNSUPPORTED before any launch.  Reads each game once, writes 4 B. */
int hk_host_select(const void* points, int64_t stride, int32_t* class_out, int batch, int max_points, int dim,
                   int dtype, int host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_HOSTS_H */
