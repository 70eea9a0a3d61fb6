/*
 * hironaka_hip_customnet.h -- the gradient-free forward of CustomNet (the reference's hironaka/jax/net.py:73-103: one
 * tower of DenseResidueBlock / DenseBlock per point count, a policy head and a tanh value head over the chosen tower's
 * result and the features behind the points) in TWO launches: one groups the rows by their point count, one carries every
 * group's row tiles through the ONE tower its rows choose and through both heads, as hk_pvnet_forward carries its rows.
 * The reference runs all m towers on every row and multiplies m - 1 of the results by zero; here a row costs one tower.
 * An addition within ABI 6 that a consumer detects by its symbol, part of the C ABI of hironaka_hip.h, which includes this
 * file behind hironaka_hip_pvnet.h (hk_pvnet_block, the limits and the block kinds are that header's); HK_F32 and the
 * status codes are defined in hironaka_hip.h.  The entry points have no counterpart in the CPU oracle: the Python binding
 * lists them in hironaka_amd/_abi.py CUSTOMNET_PROTOTYPES.  Same conventions as hironaka_hip.h: device pointers, no
 * allocation, no synchronisation, an int status.
 *
 * ---- the rule: float, every operation rounded once unless it is written fma ----
 * Row b of the input is x[b, :K] with K = m d + e: m points of d coordinates, then e more features (`extra`: none for the
 * host, the d of the subset for the agent; any e >= 0).
 *   c = #{ i < m : x[b, i d] >= 0 }                   a NaN does not count; the rule does not ask that real points come first
 *   c <  m:  u = x[b, :(c + 1) d] ++ x[b, m d : m d + e]       the first c + 1 points and the extra
 *            h = the trunk of tower c on u: hk_pvnet_forward's rule to the bit -- per block of towers[c nblocks ..], in table
 *            order, Dense as ONE fma chain per output in ascending k from the bias, the group norms' balanced sums, relu
 *            (hironaka_hip_pvnet.h states it; tower c's first block has k = (c + 1) d + e, every later k the n before it)
 *   c == m:  h = +0 in every one of the n_last columns.  The reference's jax.nn.one_hot(m, m) is all zero: a row whose
 *            points are all there gets NO tower.  That is the reference's behaviour, followed here, not a special case of
 *            this library's making.
 *   z = h ++ x[b, m d : m d + e]                       n_last + e wide
 *   p[b, a] = Dense_policy(z)[a], a < actions          -> policy[b, :actions]      the same Dense chain over n_last + e inputs
 *   v[b]    = tanh(Dense_value(z)[0])                  -> value[b]
 *            HK_CUSTOMNET_RAW_VALUE is what HK_PVNET_RAW_VALUE is there: Dense_value(z)[0] itself is stored; the tanh is the
 *            device library's tanhf, which the rule does not pin to the bit
 * A row's result depends on that row alone: not on the rows it shares a tile with, nor on the order inside its group.
 * Nothing intermediate is written to memory but the grouping (below).  Every tower has nblocks blocks of the same output
 * widths and kinds; the towers differ in their parameters and in the k of their first block.
 *
 * ---- the tower table ----
 * `towers` points at m x nblocks hk_pvnet_block records IN DEVICE MEMORY, tower t's blocks at towers[t nblocks ..]: at
 * m = 5 and 8 blocks that is 4 480 bytes, more than a kernel argument holds.  Its pointers are device pointers.  The host
 * cannot read it, so ITS CONTENTS ARE THE CALLER'S RESPONSIBILITY (hironaka_amd.ops.CustomnetPlan checks every record
 * against hk_pvnet_forward's rules when it writes the table, once): kind DENSE or RESIDUE, the chain of widths from
 * (t + 1) d + e to n_last, every width in 1..HK_PVNET_MAX_WIDTH, a residue block's n in {32, 64, 128, 256}, weights that
 * are there and aligned to 4 bytes.  The entry point checks what the descriptor itself says; that no TOWER parameter
 * shares a byte with policy or value is checked by nobody (the plan does not know the outputs of a call, the entry point
 * cannot read the table): it is the caller's to see to.
 *
 * ---- the workspace ----
 * hk_customnet_workspace_bytes(batch, m) bytes, aligned to 16, the caller's between calls.  Its first 288 bytes hold the
 * counters of the first launch (a ticket and a histogram of c): the caller ZEROES THEM ONCE, before the first call; every
 * call that computes leaves them zero again (the first launch's last workgroup resets what it used), so nothing is asked
 * of the caller between calls and a replayed graph finds them as a first call does.  Everything else the first launch
 * writes before the second reads it: the tile count, one record {tower, first slot, rows, 0} per row tile, the
 * permutation of the rows grouped by c, c of every row.  A tile never holds rows of two groups: at most
 * batch / TR + m + 1 tiles, which is the second launch's grid; a workgroup at or beyond the stored count returns before
 * its first barrier.  0: batch < 0, or m outside 1..64.
 *
 * ---- the gate ----
 * gate NULL: the call computes.  Otherwise every workgroup of both launches returns where *gate != want when it runs,
 * having touched nothing but the gate: policy, value and the workspace (its counters zero) stay as they were
 * (hk_unified_pvnet_forward's contract, hironaka_hip_unified.h).
 *
 * ---- layouts ----
 * As hk_pvnet_forward's: x / policy are rows x_stride / policy_stride ELEMENTS apart (x_stride may exceed K -- a column
 * slice of a wider buffer --, be 0 or less than K; policy_stride >= actions); value[b] lies at element b * value_stride
 * (>= 1).  policy and value may be columns of one record.  The row tiles, the crossover and the FORCE bits are
 * hk_mlp_forward's; the crossover is judged on batch.
 *
 * ---- status, before any launch, in this order ----
 * A NULL descriptor HK_ERR_NULL; another dtype, an unknown flag or both FORCE flags HK_ERR_UNSUPPORTED; the scalars: d < 2,
 * m outside 1..64, e < 0, m d + e or n_last + e above HK_PVNET_MAX_WIDTH, n_last < 1, nblocks outside
 * 1..HK_PVNET_MAX_BLOCKS, actions outside 1..HK_PVNET_MAX_WIDTH - 1, batch < 0, x_stride < 0, policy_stride < actions or
 * value_stride < 1 HK_ERR_SHAPE; a NULL x, policy, value, towers, head weight or workspace HK_ERR_NULL; x, policy, value, a
 * head pointer or the gate not aligned to 4 bytes, towers not to 8, the workspace not to 16 HK_ERR_ALIGN; a row span
 * beyond 2^63 bytes, or workspace_bytes below hk_customnet_workspace_bytes(batch, m), HK_ERR_SHAPE; policy or value sharing
 * a byte with x, a head parameter, the tower table or the workspace HK_ERR_UNSUPPORTED.  batch == 0 is HK_OK with nothing
 * launched (after every other check). */
#ifndef HIRONAKA_HIP_CUSTOMNET_H
#define HIRONAKA_HIP_CUSTOMNET_H

#include <stdint.h>

#include "hironaka_hip_pvnet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HK_CUSTOMNET_MAX_POINTS 64
/* descriptor flags (the FORCE bits are HK_MLP_FORCE_TILE_SMALL / _LARGE) */
#define HK_CUSTOMNET_RAW_VALUE 1u
#define HK_CUSTOMNET_FORCE_TILE_SMALL 2u
#define HK_CUSTOMNET_FORCE_TILE_LARGE 4u

typedef struct hk_customnet_desc {
  const void* x;
  void* policy;
  void* value;
  const hk_pvnet_block* towers; /* device memory: [m][nblocks] */
  const void* policy_weight;    /* [actions, n_last + e] */
  const void* policy_bias;      /* [actions] or NULL     */
  const void* value_weight;     /* [1, n_last + e]       */
  const void* value_bias;       /* [1] or NULL           */
  void* workspace;
  const int32_t* gate; /* NULL: no gate */
  uint64_t workspace_bytes;
  int64_t x_stride;
  int64_t policy_stride;
  int64_t value_stride;
  int32_t batch;
  int32_t m;       /* points: 1 .. HK_CUSTOMNET_MAX_POINTS */
  int32_t d;       /* coordinates of a point: >= 2 */
  int32_t e;       /* features behind the points: >= 0 */
  int32_t nblocks; /* per tower: 1 .. HK_PVNET_MAX_BLOCKS */
  int32_t n_last;  /* the last block's n */
  int32_t actions; /* 1 .. HK_PVNET_MAX_WIDTH - 1 */
  int32_t want;    /* the gate's value at which the call computes */
  int32_t dtype;   /* HK_F32 */
  uint32_t flags;
} hk_customnet_desc;

uint64_t hk_customnet_workspace_bytes(int64_t batch, int32_t m);
int hk_customnet_forward(const hk_customnet_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_CUSTOMNET_H */
