/*
 * hironaka_hip_mlp_train.h -- the training-mode forward of a create_mlp stack (hironaka_hip_mlp.h: the head's concat, a
 * ReLU, `Linear [-> BatchNorm1d] -> ReLU` blocks, a last Linear) with batch statistics, and its backward, one launch
 * per layer each way.  An addition within ABI 6 that a consumer detects by its symbols, part of the C ABI of
 * hironaka_hip.h, which includes this file behind hironaka_hip_mlp.h (HK_MLP_MAX_LAYERS, HK_MLP_MAX_WIDTH, HK_MLP_RELU
 * and HK_MLP_INPUT_RELU are that header's).  The Python binding lists the entry points in hironaka_amd/_abi.py
 * MLP_TRAIN_PROTOTYPES.  Same conventions: device pointers owned by the caller, no allocation, no synchronisation, an
 * int status decided before the first launch.  The entry points are called hk_train_mlp_*: the names hk_mlp_* are
 * hironaka_hip_mlp.h's alone.
 *
 * ---- the rule: float, every operation rounded once unless it is written fma (one rounding for both) ----
 * Two sums appear.
 *   CHAIN(c0; p_0 .. p_{T-1}) of products p_t = u_t * v_t: acc = c0; acc = fma(u_t, v_t, acc) for t ascending; and where T
 *     is no multiple of 16, one more acc = acc + (+0) (a -0 becomes +0, everything else stays: the matrix instruction
 *     runs the chain on to the next multiple of 16 with zero terms).
 *   ROWSUM(v_0 .. v_{B-1}) over the B rows: sixteen partial sums p_i = ((+0 + v_i) + v_{i+16}) + v_{i+32} ... (rows
 *     congruent to i modulo 16, ascending; +0 where there is none), then q_i = p_i + p_{i+8} (i < 8), r_i = q_i + q_{i+4}
 *     (i < 4), s_i = r_i + r_{i+2} (i < 2), and s_0 + s_1.
 * Both depend on the sum's own length alone: not on the grid, not on which instantiation serves the batch.
 *
 * Forward.  Row b of the input is a_0[b, :] = x0[b, :k0] followed by x1[b, :k1], through x < 0 ? +0 : x with
 * HK_MLP_INPUT_RELU.  Per layer l, in table order, with B = batch as a float:
 *   Linear      z[b,j] = CHAIN(bias[j] (+0 where bias is NULL); a_l[b,k] * W[j,k], k = 0 .. K-1)
 *   batch norm  (HK_MLP_TRAIN_BN)
 *               mean[j] = ROWSUM(z[.,j]) / B;   var = ROWSUM((z - mean) * (z - mean)) / B
 *               inv[j] = 1 / sqrt(var + eps)    the square root and the divide correctly rounded
 *               xhat = (z - mean) * inv;        y = fma(xhat, gamma[j], beta[j])     gamma NULL: 1, beta NULL: +0
 *               running_mean[j] = fma(momentum, mean, (1 - momentum) * running_mean[j])
 *               running_var[j]  = fma(momentum, var * (B / (B - 1)), (1 - momentum) * running_var[j])
 *               num_batches_tracked += 1 (an int64; NULL: not kept)
 *               z, mean and inv are saved
 *   ReLU        (HK_MLP_RELU)  x < 0 ? +0 : x
 *   The block's output a_{l+1} is saved in `act`; the last layer's `act` is the result.
 *
 * Backward, from the last layer to the first, given G = grad_out (the gradient with respect to the last act):
 *   d[b,j]      last layer: G[b,j];  otherwise CHAIN(+0; dz_{l+1}[b,i] * W_{l+1}[i,j], i = 0 .. n_{l+1}-1)
 *   ReLU        d = act[b,j] > 0 ? d : +0
 *   batch norm  xhat as in the forward, from the saved z, mean and inv
 *               dbeta[j] = ROWSUM(d[.,j]);   dgamma[j] = ROWSUM(d * xhat)
 *               dz = (gamma * inv) * ((d - dbeta / B) - xhat * (dgamma / B))         gamma NULL: inv alone
 *               without a batch norm dz = d
 *   dbias[j]    = ROWSUM(dz[.,j])
 *   dW[j,k]     = CHAIN(+0; dz[b,j] * a_l[b,k], b = 0 .. B-1)
 * The gradients are written, not accumulated; a NULL gradient pointer is not written.  The first layer's input gets no
 * gradient.
 *
 * ---- layouts ----
 * x0 / x1 / grad_out are rows of k0 / k1 / n_last floats, x0_stride / x1_stride / grad_stride ELEMENTS apart (0 or less
 * than the width is allowed: nothing is written there).  z and act are dense [batch, n]; mean, inv and the vectors of
 * the parameters [n]; W and d_weight [n, k] row-major.  The workspace holds dz of two consecutive layers:
 * hk_train_mlp_workspace_bytes(desc) bytes, aligned to 4.  One workgroup carries 16 columns of a layer for ALL rows, so
 * the batch is at most HK_MLP_TRAIN_MAX_BATCH; hk_train_mlp_rows says which of the two instantiations (up to
 * HK_MLP_TRAIN_ROWS_SMALL rows, or up to the cap) serves a batch -- same bits.
 *
 * ---- status, before any launch ----
 * batch == 0 is HK_OK with nothing launched (after every other check).  HK_ERR_NULL: a NULL descriptor, x0, x1 with
 * k1 > 0, weight or act; with HK_MLP_TRAIN_BN a NULL z, mean, inv, running_mean or running_var; for the backward a NULL
 * grad_out, d_weight or workspace (more than one layer).  HK_ERR_SHAPE: nlayers, k, n, k0, k1, the chain of widths as
 * in hk_mlp_forward, a negative stride, batch < 0, batch > HK_MLP_TRAIN_MAX_BATCH, batch == 1 with a batch norm,
 * workspace_bytes below what the backward needs.  HK_ERR_UNSUPPORTED: another dtype, an unknown flag, a bn pointer
 * (bn_weight, bn_bias, running_*, num_batches_tracked, d_bn_*) without HK_MLP_TRAIN_BN, or something written (forward:
 * z, act, mean, inv, the running statistics; backward: every gradient and the workspace) that shares a byte with
 * something read or with another thing written.  HK_ERR_ALIGN: a pointer not aligned to 4 bytes (num_batches_tracked: 8).
 */
#ifndef HIRONAKA_HIP_MLP_TRAIN_H
#define HIRONAKA_HIP_MLP_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HK_MLP_TRAIN_MAX_BATCH 1024
#define HK_MLP_TRAIN_ROWS_SMALL 256
/* layer flag, next to HK_MLP_RELU */
#define HK_MLP_TRAIN_BN 2u

typedef struct hk_mlp_train_layer {
  const void* weight;        /* [n, k] */
  const void* bias;          /* [n] or NULL */
  const void* bn_weight;     /* [n] or NULL (affine=False) */
  const void* bn_bias;       /* [n] or NULL */
  void* running_mean;        /* [n], updated by the forward */
  void* running_var;         /* [n] */
  void* num_batches_tracked; /* one int64 or NULL */
  void* z;                   /* [batch, n] the Linear's output, saved where a batch norm follows */
  void* act;                 /* [batch, n] the block's output */
  void* mean;                /* [n] batch mean */
  void* inv;                 /* [n] 1 / sqrt(var + eps) */
  void* d_weight;            /* [n, k] */
  void* d_bias;              /* [n] or NULL */
  void* d_bn_weight;         /* [n] or NULL */
  void* d_bn_bias;           /* [n] or NULL */
  float eps;
  float momentum;
  int32_t k;
  int32_t n;
  uint32_t flags;
  int32_t reserved_;
} hk_mlp_train_layer;

typedef struct hk_mlp_train_desc {
  const void* x0;
  const void* x1;       /* NULL with k1 == 0 */
  const void* grad_out; /* [batch, n_last]; the backward's */
  void* workspace;      /* the backward's */
  int64_t x0_stride;
  int64_t x1_stride;
  int64_t grad_stride;
  uint64_t workspace_bytes;
  int32_t batch;
  int32_t k0;
  int32_t k1;
  int32_t nlayers;
  int32_t dtype; /* HK_F32 */
  uint32_t flags; /* HK_MLP_INPUT_RELU */
  hk_mlp_train_layer layer[HK_MLP_MAX_LAYERS];
} hk_mlp_train_desc;

int hk_train_mlp_rows(int64_t batch);
uint64_t hk_train_mlp_workspace_bytes(const hk_mlp_train_desc* desc);
int hk_train_mlp_forward(const hk_mlp_train_desc* desc, void* stream);
int hk_train_mlp_backward(const hk_mlp_train_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_MLP_TRAIN_H */
