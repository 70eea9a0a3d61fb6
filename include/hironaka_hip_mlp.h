/*
 * hironaka_hip_mlp.h -- the eval-mode forward of a Q-network built by the reference's create_mlp
 * (hironaka/trainer/nets.py:27-73: the head's flatten / concat, a ReLU, `Linear [-> BatchNorm1d] -> ReLU` blocks, a last
 * Linear) in ONE launch: a tile of batch rows stays in LDS from the features to the Q-values, the weights are read where
 * torch keeps them ([out, in] row-major), the products run on gfx950's f32-input MFMA.  An addition within ABI 6 that a
 * consumer detects by its symbol, part of the C ABI of hironaka_hip.h, which includes this file; HK_F32 and the status
 * codes are defined there.  The entry points have no counterpart in the CPU oracle: the Python binding lists them in
 * hironaka_amd/_abi.py MLP_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 *
 * ---- the rule: float, every operation rounded once unless it is written fma (one rounding for both) ----
 * Row b of the input is h[b, :] = x0[b, :k0] followed by x1[b, :k1] (k1 = 0: x0 alone).  Where the descriptor's four
 * in_bn pointers are not all NULL the batch norm below (with in_eps, over the k0 + k1 columns) is applied to it first
 * (create_mlp's net_arch that begins with 'b'), then with HK_MLP_INPUT_RELU the ReLU below (create_mlp's activation
 * behind the head).  Then per layer, in table order:
 *   Linear      z[b,j] = fma(h[b,K-1], W[j,K-1], ... fma(h[b,1], W[j,1], fma(h[b,0], W[j,0], bias[j])))
 *               one chain per output, k ascending, starting from bias[j], from +0 where bias is NULL
 *   batch norm  (eval mode; where the layer's four bn pointers are not all NULL)
 *               inv = 1 / sqrt(var[j] + eps)      the square root and the divide correctly rounded
 *               alpha = gamma[j] * inv;  y = fma(z - mean[j], alpha, beta[j])
 *               bn_weight NULL: alpha = inv;  bn_bias NULL: beta = +0
 *   ReLU        (HK_MLP_RELU)  x < 0 ? +0 : x     NaN stays NaN, -0 stays -0
 * The last layer's result goes to out[b, :n].  Nothing intermediate is written to memory.
 * The MFMA adds four k's per instruction, so the kernel carries every chain on to the next multiple of 16 with
 * fma(+0, +0, acc) BEHIND the real k's.  That returns acc for every acc but -0, which becomes +0: a chain that ends in
 * -0 (a -0 bias under products that are all zero, or an underflow from below) comes out as +0 where K is no multiple
 * of 16.  Every other value, NaN and the infinities included, is the rule's to the bit.
 *
 * ---- layouts ----
 * x0 / x1 / out are rows of k0 / k1 / n_last floats, x0_stride / x1_stride / out_stride ELEMENTS apart (an input stride
 * may be 0 or less than the width; out_stride >= n_last).  Batch-tail rows of a tile are never read or stored.
 * One workgroup carries HK_MLP_TILE_SMALL rows while each has a compute unit to itself (batch <= HK_MLP_TILE_CROSSOVER),
 * HK_MLP_TILE_LARGE beyond; hk_mlp_row_tile says which, HK_MLP_FORCE_TILE_SMALL / _LARGE override it (same bits).
 *
 * ---- status, before any launch ----
 * batch == 0 is HK_OK with nothing launched (after every other check).  A NULL descriptor, x0, out, x1 with k1 > 0, a
 * NULL weight, or a batch norm (a layer's or the input's) with its mean or var NULL while another of its four is set
 * is HK_ERR_NULL; nlayers outside 1..HK_MLP_MAX_LAYERS, k or n outside 1..HK_MLP_MAX_WIDTH, k0 < 1, k1 < 0, batch < 0,
 * layer l's k different from layer l-1's n (k0 + k1 for layer 0), x0_stride / x1_stride < 0 or out_stride < n_last
 * HK_ERR_SHAPE; another dtype, an unknown flag, both FORCE flags, or out sharing a byte with an input or a parameter
 * HK_ERR_UNSUPPORTED (ranges are judged from their first to their last element, but for out and an input of ONE row
 * stride: columns of the same records, which only have to keep apart inside a record); a pointer that is not aligned
 * to 4 bytes HK_ERR_ALIGN. */
#ifndef HIRONAKA_HIP_MLP_H
#define HIRONAKA_HIP_MLP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HK_MLP_MAX_LAYERS 32
#define HK_MLP_MAX_WIDTH 256
#define HK_MLP_TILE_SMALL 16
#define HK_MLP_TILE_LARGE 64
#define HK_MLP_TILE_CROSSOVER 4096 /* 16 rows x 256 compute units: the largest batch on 16-row tiles */
/* descriptor flags */
#define HK_MLP_INPUT_RELU 1u
#define HK_MLP_FORCE_TILE_SMALL 2u
#define HK_MLP_FORCE_TILE_LARGE 4u
/* layer flags */
#define HK_MLP_RELU 1u

typedef struct hk_mlp_layer {
  const void* weight;    /* [n, k] row-major, as nn.Linear keeps it */
  const void* bias;      /* [n] or NULL                              */
  const void* bn_mean;   /* [n] running_mean; all four NULL: no batch norm */
  const void* bn_var;    /* [n] running_var                          */
  const void* bn_weight; /* [n] or NULL (affine=False)               */
  const void* bn_bias;   /* [n] or NULL                              */
  float eps;
  int32_t k;
  int32_t n;
  uint32_t flags;
} hk_mlp_layer;

typedef struct hk_mlp_desc {
  const void* x0;
  const void* x1; /* NULL with k1 == 0 */
  void* out;
  const void* in_bn_mean; /* [k0 + k1]; all four NULL: no batch norm on the input */
  const void* in_bn_var;
  const void* in_bn_weight;
  const void* in_bn_bias;
  int64_t x0_stride;
  int64_t x1_stride;
  int64_t out_stride;
  int32_t batch;
  int32_t k0;
  int32_t k1;
  int32_t nlayers; /* 1 .. HK_MLP_MAX_LAYERS */
  int32_t dtype;   /* HK_F32                 */
  uint32_t flags;
  float in_eps;
  int32_t reserved_;
  hk_mlp_layer layer[HK_MLP_MAX_LAYERS];
} hk_mlp_desc;

int hk_mlp_row_tile(int64_t batch);
int hk_mlp_forward(const hk_mlp_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_MLP_H */
