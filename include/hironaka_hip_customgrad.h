/*
 * hironaka_hip_customgrad.h -- the training-mode forward of CustomNet (hironaka_hip_customnet.h: one tower per point
 * count, a policy head and a tanh value head over the chosen tower's result and the features behind the points) with what
 * its backward needs saved, and that backward.  Every row runs the ONE tower its point count names, forward and backward;
 * the reference's formula runs all m towers both ways on every row and multiplies m - 1 results by zero.  An addition
 * within ABI 6 that a consumer detects by its symbols, part of the C ABI of hironaka_hip.h, which includes this file
 * behind hironaka_hip_pvgrad.h.  The Python binding lists the entry points in hironaka_amd/_abi.py CUSTOMGRAD_PROTOTYPES.
 * Same conventions: device pointers owned by the caller, no allocation, no synchronisation, an int status decided on the
 * host before the first launch.  float32; the 16-row tile only; batch <= HK_PVGRAD_MAX_BATCH; m, d, e, widths, blocks and
 * actions as hk_customnet_forward accepts them.
 *
 * ---- launches: they depend neither on m nor on the data ----
 * hk_customgrad_forward: two (the grouping, one workgroup; the row tiles).  hk_customgrad_backward: two (the row chain;
 * the parameter gradients of every tower and of the heads).  The backward uses the grouping its forward left in the
 * workspace.  The row launches have batch / 16 + m + 1 workgroups, the worst case: a workgroup at or beyond the stored tile
 * count returns before its first barrier.  The parameter launch has one wave per (tower, Dense, 16 x 16 tile) with every
 * tower's first block counted at the full input width m d + e, plus the heads': a wave whose tile its tower does not have
 * returns.  No atomics, nobody waits for anybody.
 *
 * ---- the grouped order ----
 * c(b) is hironaka_hip_customnet.h's point count of row b.  The GROUPED ORDER s -> b(s) is the rows sorted by (c(b), b),
 * both ascending: the same on every launch, whatever the hardware does.  G_t are the rows with c == t in ascending b, R_t
 * their number; group t lies at the slots first[t] .. first[t] + R_t - 1.  A 16-row tile never mixes groups.
 *
 * ---- the rule: float, every operation rounded once unless it is written fma ----
 * CHAIN, ROWSUM and GNB are hironaka_hip_pvgrad.h's and hironaka_hip_mlp_train.h's.
 * Forward: policy and value have hk_customnet_forward's bits.  Saved in the workspace, in grouped order: the tower input
 * u = x[b, :(c+1)d] ++ extra of every row with c < m; per block what hk_pvgrad_forward saves (z1, a, z2, zp, h'); the
 * heads' input z = h ++ extra, with h = +0 where c == m.
 * Backward:
 *   heads   dzh as in hironaka_hip_pvgrad.h, from grad_policy / grad_value at the row's OWN index b and the stored value;
 *           HK_CUSTOMNET_RAW_VALUE behaves as HK_PVNET_RAW_VALUE there.
 *           D[b,k] = CHAIN(+0; dzh[b,j] * Wh[j,k], j = 0..A) for k < n_last only: the e columns of extra belong to the
 *           input, which gets no gradient.
 *           d_weight[j,k] = CHAIN(+0; dzh[b(s),j] * z[b(s),k], s = 0..B-1) for k < n_last + e;  d_bias[j] = ROWSUM over the
 *           same order: ALL rows, in grouped order.
 *   a row of c < m   runs the blocks of tower c backward from D exactly as hk_pvgrad_backward runs its trunk: relu mask,
 *           GNB, the residual, the projection.  The first block's input gets no gradient.
 *   a row of c == m  runs no tower.
 *   tower t's parameter gradients sum over G_t alone, in ascending b:
 *           d_weight[j,k] = CHAIN(+0; dz[b,j] * a_in[b,k], b in G_t);  d_bias, d_gn_scale and d_gn_bias are ROWSUM over
 *           G_t with a row's position in its group in the place of the row index.  The `+ (+0)` where R_t is no multiple
 *           of 16 is as in CHAIN; the rows of a chain's last 16-row step that lie outside the group contribute as
 *           +0 * +0, whatever the neighbouring group holds there.
 *   R_t == 0: every gradient of tower t is written as +0.  (The reference's formula gives such a tower zero too.)
 * Gradients are written, not accumulated.
 *
 * ---- the gradient table: offsets, not pointers ----
 * m x nblocks blocks of four gradient pointers per Dense fit neither a kernel argument nor a fixed-size descriptor.
 * `grad_table` points at m x nblocks hk_customgrad_block records IN DEVICE MEMORY, parallel to the tower table: tower t's
 * block l at grad_table[t nblocks + l].  A record holds OFFSETS in floats into ONE gradient buffer whose base a call
 * passes as `grads`; HK_CUSTOMGRAD_NONE says "not there" (a parameter that does not exist; a d_weight is always there).
 * The heads' offsets are the descriptor's own `policy` / `value`.  The host cannot read the table, so ITS CONTENTS ARE THE
 * CALLER'S RESPONSIBILITY, as the tower table's are (hironaka_amd.ops.CustomnetPlan writes both, once): offsets within
 * grad_floats, no two gradients sharing a float.  No call copies a table to the device.
 * n[l] and kind[l] are the blocks' output widths and kinds (every tower's are the same), which the host needs for the
 * workspace and the grids: they must be the tower table's.
 *
 * ---- the workspace (net.workspace, net.workspace_bytes) ----
 * hk_customgrad_workspace_bytes(desc) bytes aligned to 16 (a larger one changes no bit), 4-byte words:
 *   [0]                 the number of row tiles; [4 .. 68] first[c]; [72 .. 136] R_c; 144 words in all
 *   [144 ..]            batch / 16 + m + 1 tile records {tower, first slot, rows, 0}
 *   behind them         the permutation b(s), batch words, then zero to three unused words up to a multiple of four
 *   behind that, float  u [batch, m d + e] (a row of tower t uses its first (t+1) d + e columns)
 *                       per block, in order, hironaka_hip_pvgrad.h's arrays [batch, n] of that block's kind; the first
 *                       block of a residue trunk always has the three arrays of a projection (a tower whose input is as
 *                       wide as the block leaves them unused)
 *                       z [batch, n_last + e];  dzh [batch, actions + 1]
 * every array by slot.  Nothing has to be zeroed, and nothing is kept between a backward and the next forward.  The
 * forward writes the grouping, u, z1, a, z2, zp, h' and z; the backward the rest, and reads what the forward of the SAME
 * descriptor left there.  0: a descriptor whose sizes the forward would refuse, or batch <= 0.
 *
 * ---- status, before any launch, in this order ----
 * A NULL descriptor HK_ERR_NULL.  Everything hk_customnet_forward refuses of `net` but its workspace's size, with its
 * code (the workspace must be there and aligned to 16).  A gate or either FORCE_TILE flag HK_ERR_UNSUPPORTED.  n[l] outside
 * 1..HK_PVNET_MAX_WIDTH, a kind that is neither HK_PVNET_DENSE nor HK_PVNET_RESIDUE, a residue block's n outside {32, 64,
 * 128, 256}, n[nblocks - 1] != net.n_last, batch > HK_PVGRAD_MAX_BATCH, for the backward grad_policy_stride < actions or
 * grad_value_stride < 1, net.workspace_bytes below hk_customgrad_workspace_bytes(desc) HK_ERR_SHAPE.  For the backward a
 * NULL grad_table, grads, grad_policy or grad_value, or a head's d_weight that is HK_CUSTOMGRAD_NONE, HK_ERR_NULL;
 * grad_table not aligned to 8 bytes, grads, grad_policy or grad_value not to 4, HK_ERR_ALIGN; a head's gradient that ends
 * beyond grad_floats HK_ERR_SHAPE.  batch == 0 HK_OK with nothing launched.  The workspace or (backward) the gradient
 * buffer sharing a byte with x, a head parameter, a table, grad_policy, grad_value, policy, value or each other
 * HK_ERR_UNSUPPORTED.
 */
#ifndef HIRONAKA_HIP_CUSTOMGRAD_H
#define HIRONAKA_HIP_CUSTOMGRAD_H

#include <stdint.h>

#include "hironaka_hip_customnet.h"
#include "hironaka_hip_pvgrad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* an offset that says "this gradient is not there" */
#define HK_CUSTOMGRAD_NONE (-1)
/* words in front of the tile records; where first[c] and R_c begin */
#define HK_CUSTOMGRAD_HEADER 144
#define HK_CUSTOMGRAD_FIRST 4
#define HK_CUSTOMGRAD_SIZE 72

typedef struct hk_customgrad_dense {
  int64_t d_weight;   /* offsets in floats into the gradient buffer */
  int64_t d_bias;     /* or HK_CUSTOMGRAD_NONE                      */
  int64_t d_gn_scale; /* a normed Dense's                           */
  int64_t d_gn_bias;
} hk_customgrad_dense;

typedef struct hk_customgrad_block {
  hk_customgrad_dense dense1;
  hk_customgrad_dense dense2;
  hk_customgrad_dense proj;
} hk_customgrad_block;

typedef struct hk_customgrad_desc {
  hk_customnet_desc net;                 /* the forward's (gate NULL); `value` is read by the backward */
  const hk_customgrad_block* grad_table; /* device memory: [m][nblocks]; the backward's                */
  void* grads;                           /* the gradient buffer's base; the backward's                 */
  const void* grad_policy;               /* [batch, actions]; the backward's                           */
  const void* grad_value;                /* [batch]; the backward's                                    */
  int64_t grad_policy_stride;
  int64_t grad_value_stride;
  uint64_t grad_floats;       /* the gradient buffer's size in floats                       */
  hk_customgrad_dense policy; /* d_weight [actions, n_last + e], d_bias [actions]           */
  hk_customgrad_dense value;  /* d_weight [1, n_last + e], d_bias [1]                       */
  int32_t n[HK_PVNET_MAX_BLOCKS];    /* every tower's block widths ...                       */
  int32_t kind[HK_PVNET_MAX_BLOCKS]; /* ... and kinds, as the tower table has them           */
} hk_customgrad_desc;

uint64_t hk_customgrad_workspace_bytes(const hk_customgrad_desc* desc);
int hk_customgrad_forward(const hk_customgrad_desc* desc, void* stream);
int hk_customgrad_backward(const hk_customgrad_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_CUSTOMGRAD_H */
