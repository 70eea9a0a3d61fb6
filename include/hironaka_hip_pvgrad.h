/*
 * hironaka_hip_pvgrad.h -- the training-mode forward of a policy-value network of the MCTS trainer (hironaka_hip_pvnet.h:
 * a trunk of DenseResidueBlock / DenseBlock, a policy head and a tanh value head) with what its backward needs saved, and
 * that backward, in a handful of launches.  A GroupNorm(32) couples g = n / 32 <= 8 adjacent columns of ONE row, so a tile
 * of 16 rows runs backward through the whole stack as it runs forward; only the parameter gradients sum over rows.  An
 * addition within ABI 6 that a consumer detects by its symbols, part of the C ABI of hironaka_hip.h, which includes this
 * file behind hironaka_hip_pvloss.h (hk_pvnet_desc and the HK_PVNET_* limits are hironaka_hip_pvnet.h's).  The Python
 * binding lists the entry points in hironaka_amd/_abi.py PVGRAD_PROTOTYPES.  Same conventions: device pointers owned by
 * the caller, no allocation, no synchronisation, an int status decided on the host before the first launch.  The
 * descriptor is read on the HOST only: every launch is handed what it needs.
 *
 * ---- launches ----
 * hk_pvgrad_forward: one.  hk_pvgrad_backward: one for the row chain, then one per HK_PVGRAD_TABLE Denses in use (the
 * two heads count as one Dense each) for the parameter gradients: 1 + ceil((denses + 2) / HK_PVGRAD_TABLE), which is 2 up
 * to 38 Denses in the trunk (an [n] x 8 net has 16) and at most 4 (32 blocks that all project: 96 + 2).
 *
 * ---- the rule: float, every operation rounded once unless it is written fma (one rounding for both) ----
 * CHAIN and ROWSUM are hironaka_hip_mlp_train.h's, the `+ (+0)` where a chain's length is no multiple of 16 included.
 * Forward: hironaka_hip_pvnet.h's rule; policy and value are hk_pvnet_forward's to the bit.  Saved in the workspace: in
 * front of every group norm the Dense's result z, behind Dense1's norm and ReLU a = relu(GN1(z1)), every block's h'.
 * Backward, with G = grad_policy and, per row b, t = grad_value[b]:
 *   heads   dzh[b,j] = G[b,j] (j < A);  dzh[b,A] = t * (1 - v*v)   v: the stored tanh value (`value`), v*v rounded, then
 *                                                                   the subtraction, then the product;
 *                                                                   HK_PVNET_RAW_VALUE: dzh[b,A] = t
 *           D[b,k]   = CHAIN(+0; dzh[b,j] * Wh[j,k], j = 0 .. A)   Wh: the policy weight's rows, then the value weight's
 *   block   (from the last to the first; D' = the gradient at its output h', k / n its widths)
 *           e        = h' > 0 ? D' : +0
 *     dense   dz1 = e;                      D = CHAIN(+0; dz1[b,i] * W1[i,j], i < n)
 *     residue dz2 = GNB(e; z2, dense2);     da = CHAIN(+0; dz2[b,i] * W2[i,j], i < n);   da = a > 0 ? da : +0
 *             dz1 = GNB(da; z1, dense1);    d1 = CHAIN(+0; dz1[b,i] * W1[i,j], i < n)
 *             k == n: D = d1 + e            otherwise dzp = GNB(e; zp, proj);  D = d1 + CHAIN(+0; dzp[b,i] * Wp[i,j], i < n)
 *     The first block's input gets no gradient: its D is not computed.
 *   GNB(e; z, dense)   mean, d, inv from z exactly as the forward's GN computes them (the same bits);  xhat = d * inv
 *           u = e * scale[j] (scale NULL: e);  m1 = groupsum(u) / g;  m2 = groupsum(u * xhat) / g    (the balanced sums)
 *           dz = inv * ((u - m1) - xhat * m2)
 *           d_gn_bias[j] = ROWSUM(e[., j]);   d_gn_scale[j] = ROWSUM(e * xhat)      (e * xhat rounded, then summed)
 *   every Dense with input a_in:   d_weight[j,k] = CHAIN(+0; dz[b,j] * a_in[b,k], b = 0 .. B-1);  d_bias[j] = ROWSUM(dz[., j])
 * Gradients are written, not accumulated; a NULL gradient pointer (but d_weight) is not written.  At g = 1 (width 32) dz
 * is exactly zero for finite inputs, as the forward's d is -- not a special case.
 *
 * ---- layouts ----
 * `net` is hk_pvnet_forward's descriptor: x, policy, value, their strides, the block table.  grad_policy are rows of
 * `actions` floats grad_policy_stride ELEMENTS apart (>= actions), grad_value[b] lies at element b * grad_value_stride
 * (>= 1).  A gradient has its parameter's shape, dense.  The heads' d_gn_scale / d_gn_bias and the pointers of a Dense
 * the net does not use are not looked at.  The workspace, hk_pvgrad_workspace_bytes(desc) bytes aligned to 4 (a larger one
 * changes no bit), is dense [batch, n] arrays, block after block in table order, then dzh [batch, actions + 1]:
 *   dense block            h'  dz1
 *   residue block          z1  a  z2  h'  e  da  dz1  dz2  da*xhat1  e*xhat2     then, with a projection,  zp  dzp  e*xhatp
 * The forward writes z1, a, z2, zp and h', the backward the rest; the backward reads what the forward of the SAME
 * descriptor left there.  0 bytes: a descriptor the forward would refuse for its sizes, or batch <= 0.
 *
 * ---- limits ----
 * float32; the 16-row tile only; batch <= HK_PVGRAD_MAX_BATCH (hk_mlp_forward's crossover to the 64-row tile); blocks,
 * widths, normed widths and actions as in hk_pvnet_forward.
 *
 * ---- status, before any launch ----
 * Everything hk_pvnet_forward refuses of `net`, with the same code.  HK_ERR_SHAPE: batch > HK_PVGRAD_MAX_BATCH, a
 * workspace_bytes below hk_pvgrad_workspace_bytes(desc), for the backward grad_policy_stride < actions or
 * grad_value_stride < 1.  HK_ERR_NULL: a NULL descriptor or workspace; for the backward a NULL grad_policy or grad_value,
 * or a NULL d_weight of a Dense in use (the heads included).  HK_ERR_UNSUPPORTED: either FORCE_TILE flag; the workspace
 * (both ways) or a gradient (the backward) sharing a byte with anything read (x, a parameter, value, grad_policy,
 * grad_value) or with another thing written (policy and value for the forward).  HK_ERR_ALIGN: a pointer not aligned to
 * 4 bytes.  batch == 0: HK_OK, nothing launched (after every other check).
 */
#ifndef HIRONAKA_HIP_PVGRAD_H
#define HIRONAKA_HIP_PVGRAD_H

#include <stdint.h>

#include "hironaka_hip_pvnet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HK_PVGRAD_MAX_BATCH 4096
/* Denses per launch of the parameter gradients */
#define HK_PVGRAD_TABLE 40

typedef struct hk_pvgrad_dense {
  void* d_weight;   /* [n, k]                                  */
  void* d_bias;     /* [n] or NULL                             */
  void* d_gn_scale; /* [n] or NULL: a normed Dense's           */
  void* d_gn_bias;  /* [n] or NULL                             */
} hk_pvgrad_dense;

typedef struct hk_pvgrad_block {
  hk_pvgrad_dense dense1;
  hk_pvgrad_dense dense2;
  hk_pvgrad_dense proj;
} hk_pvgrad_block;

typedef struct hk_pvgrad_desc {
  hk_pvnet_desc net;        /* the forward's; `value` is read by the backward (the tanh's result) */
  const void* grad_policy;  /* [batch, actions]; the backward's */
  const void* grad_value;   /* [batch]; the backward's          */
  void* workspace;
  int64_t grad_policy_stride;
  int64_t grad_value_stride;
  uint64_t workspace_bytes;
  hk_pvgrad_dense policy; /* d_weight [actions, n_last], d_bias [actions] */
  hk_pvgrad_dense value;  /* d_weight [1, n_last], d_bias [1]             */
  hk_pvgrad_block block[HK_PVNET_MAX_BLOCKS];
} hk_pvgrad_desc;

uint64_t hk_pvgrad_workspace_bytes(const hk_pvgrad_desc* desc);
int hk_pvgrad_forward(const hk_pvgrad_desc* desc, void* stream);
int hk_pvgrad_backward(const hk_pvgrad_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_PVGRAD_H */
