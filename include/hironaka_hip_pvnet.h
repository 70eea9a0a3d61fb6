/*
 * hironaka_hip_pvnet.h -- the gradient-free forward of a policy-value network of the MCTS trainer (the reference's
 * hironaka/jax/net.py: DenseResNet / DenseNet, a trunk of DenseResidueBlock or DenseBlock followed by a policy head and a
 * tanh value head) in ONE launch: a tile of batch rows stays in LDS from the features to both heads, the weights are read
 * where torch keeps them ([out, in] row-major), the products run on gfx950's f32-input MFMA, the group norms in the
 * registers of the MFMA's result.  An addition within ABI 6 that a consumer detects by its symbol, part of the C ABI of
 * hironaka_hip.h, which includes this file; HK_F32 and the status codes are defined there.  The entry point has no
 * counterpart in the CPU oracle: the Python binding lists it in hironaka_amd/_abi.py PVNET_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 *
 * ---- the rule: float, every operation rounded once unless it is written fma (one rounding for both) ----
 * Row b of the input is h[b, :k0] = x[b, :k0].  Then per block, in table order (k: the block's input width, n: its output):
 *   dense block    (HK_PVNET_DENSE; DenseBlock)         h' = relu(Dense1(h))                       no norm
 *   residue block  (HK_PVNET_RESIDUE; DenseResidueBlock) y = GN2(Dense2(relu(GN1(Dense1(h)))))
 *                  o = h where k == n, otherwise o = GNp(Densep(h))      (the reference's res_proj / norm_proj)
 *                  h' = relu(o + y)                                       one rounded add
 *   Dense   z[b,j] = fma(h[b,K-1], W[j,K-1], ... fma(h[b,1], W[j,1], fma(h[b,0], W[j,0], bias[j])))
 *           hk_mlp_forward's Linear to the bit: one chain per output, k ascending, starting from bias[j], from +0 where
 *           bias is NULL; the MFMA carries every chain on to the next multiple of 16 with fma(+0, +0, acc), so a chain that
 *           ends in -0 comes out as +0 where K is no multiple of 16 (hironaka_hip_mlp.h); every other value is the rule's
 *   GN      flax's GroupNorm(num_groups = 32) on [B, n]: g = n / 32 columns per group, group c the columns c g .. c g + g - 1
 *           s = the balanced pairwise sum of the group's z: adjacent pairs, then pairs of those, then pairs of those
 *           mean = s / g;  d = z - mean;  q = the same balanced sum of the rounded products d * d;  var = q / g
 *           inv = 1 / sqrt(var + eps)        the square root and the divide correctly rounded; eps: the block's (flax: 1e-6)
 *           alpha = scale[j] * inv;  y = fma(d, alpha, gn_bias[j]);  scale NULL: alpha = inv;  gn_bias NULL: beta = +0
 *           (g = 1, width 32: d = 0 and y = gn_bias[j] for every finite z, as in flax -- not a special case)
 *   relu    x < 0 ? +0 : x     NaN stays NaN, -0 stays -0
 * and the heads on the last block's h':
 *   p[b, a] = Dense_policy(h')[a], a < actions                       -> policy[b, :actions]
 *   v[b]    = tanh(Dense_value(h')[0])                               -> value[b]
 *           HK_PVNET_RAW_VALUE stores Dense_value(h')[0] itself; the tanh is the device library's tanhf, which the rule
 *           does not pin to the bit
 * Nothing intermediate is written to memory.  A normed layer (every Dense of a residue block) has n in {32, 64, 128, 256};
 * a dense block's n is anything in 1..HK_PVNET_MAX_WIDTH.
 *
 * ---- layouts ----
 * x / policy are rows of k0 / actions floats, x_stride / policy_stride ELEMENTS apart (x_stride may be 0 or less than
 * k0; policy_stride >= actions); value[b] lies at element b * value_stride (>= 1).  Batch-tail rows of a tile are never
 * read or stored.  policy and value may be columns of one record; that they share no element is the caller's to see to.
 * The row tiles, the crossover between them and the FORCE flags are hk_mlp_forward's (hk_mlp_row_tile says which).
 *
 * ---- status, before any launch ----
 * batch == 0 is HK_OK with nothing launched (after every other check).  A NULL descriptor, x, policy, value, head weight,
 * a block's dense1 weight, a residue block's dense2 weight, or a residue block with k != n and no proj weight is
 * HK_ERR_NULL; nblocks outside 1..HK_PVNET_MAX_BLOCKS, k or n outside 1..HK_PVNET_MAX_WIDTH, k0 < 1, actions outside
 * 1..HK_PVNET_MAX_WIDTH - 1, batch < 0, a block's k different from the block before's n (k0 for block 0), a residue
 * block's n that is no multiple of 32, x_stride < 0, policy_stride < actions or value_stride < 1 HK_ERR_SHAPE; another
 * dtype, an unknown flag or kind, both FORCE flags, a residue block's n that is a multiple of 32 other than
 * 32 / 64 / 128 / 256, or policy or value sharing a byte with x or a parameter (ranges judged from their first to their
 * last element) HK_ERR_UNSUPPORTED; a pointer that is not aligned to 4 bytes HK_ERR_ALIGN.  A dense block's dense2, proj
 * and group-norm pointers are not looked at. */
#ifndef HIRONAKA_HIP_PVNET_H
#define HIRONAKA_HIP_PVNET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HK_PVNET_MAX_BLOCKS 32
#define HK_PVNET_MAX_WIDTH 256
/* block kinds */
#define HK_PVNET_DENSE 0
#define HK_PVNET_RESIDUE 1
/* descriptor flags (the FORCE bits are HK_MLP_FORCE_TILE_SMALL / _LARGE) */
#define HK_PVNET_RAW_VALUE 1u
#define HK_PVNET_FORCE_TILE_SMALL 2u
#define HK_PVNET_FORCE_TILE_LARGE 4u

typedef struct hk_pvnet_dense {
  const void* weight;   /* [n, k] row-major, as nn.Linear keeps it */
  const void* bias;     /* [n] or NULL                              */
  const void* gn_scale; /* [n] or NULL: the group norm's scale      */
  const void* gn_bias;  /* [n] or NULL: the group norm's bias       */
} hk_pvnet_dense;

typedef struct hk_pvnet_block {
  hk_pvnet_dense dense1;
  hk_pvnet_dense dense2; /* residue block */
  hk_pvnet_dense proj;   /* residue block with k != n: res_proj / norm_proj */
  float eps;
  int32_t k;
  int32_t n;
  int32_t kind; /* HK_PVNET_DENSE / HK_PVNET_RESIDUE */
} hk_pvnet_block;

typedef struct hk_pvnet_desc {
  const void* x;
  void* policy;
  void* value;
  const void* policy_weight; /* [actions, n_last] */
  const void* policy_bias;   /* [actions] or NULL */
  const void* value_weight;  /* [1, n_last]       */
  const void* value_bias;    /* [1] or NULL       */
  int64_t x_stride;
  int64_t policy_stride;
  int64_t value_stride;
  int32_t batch;
  int32_t k0;
  int32_t nblocks; /* 1 .. HK_PVNET_MAX_BLOCKS */
  int32_t actions; /* 1 .. HK_PVNET_MAX_WIDTH - 1 */
  int32_t dtype;   /* HK_F32 */
  uint32_t flags;
  hk_pvnet_block block[HK_PVNET_MAX_BLOCKS];
} hk_pvnet_desc;

int hk_pvnet_forward(const hk_pvnet_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_PVNET_H */
