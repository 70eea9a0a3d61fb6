// C ABI of hk_pvnet_forward (include/hironaka_hip_pvnet.h, an addition within ABI 6): argument validation and launch of
// hk::pvnet_kernel.  No allocation, no synchronisation; every status is decided before the launch.
#include "hk_pvnet_kernel.h"

using namespace hk;

namespace {

constexpr uint32_t kDescFlags = HK_PVNET_RAW_VALUE | HK_PVNET_FORCE_TILE_SMALL | HK_PVNET_FORCE_TILE_LARGE;

// the Denses a block of its kind uses
int denses(const hk_pvnet_block& B, const hk_pvnet_dense* (&d)[3]) {
  d[0] = &B.dense1;
  if (B.kind == HK_PVNET_DENSE) return 1;
  d[1] = &B.dense2;
  if (B.k == B.n) return 2;
  d[2] = &B.proj;
  return 3;
}

int validate(const hk_pvnet_desc* q) {
  if (const int bad = mlp_check_desc(q, kDescFlags)) return bad;
  if (mlp_forces_both_tiles(q->flags)) return HK_ERR_UNSUPPORTED;
  if (q->nblocks < 1 || q->nblocks > HK_PVNET_MAX_BLOCKS) return HK_ERR_SHAPE;
  if (q->batch < 0 || q->k0 < 1 || q->x_stride < 0) return HK_ERR_SHAPE;
  if (q->actions < 1 || q->actions > HK_PVNET_MAX_WIDTH - 1) return HK_ERR_SHAPE;
  if (q->policy_stride < q->actions || q->value_stride < 1) return HK_ERR_SHAPE;
  int64_t width = q->k0;
  for (int l = 0; l < q->nblocks; ++l) {
    const hk_pvnet_block& B = q->block[l];
    if (B.kind != HK_PVNET_DENSE && B.kind != HK_PVNET_RESIDUE) return HK_ERR_UNSUPPORTED;
    if (B.k < 1 || B.k > HK_PVNET_MAX_WIDTH || B.n < 1 || B.n > HK_PVNET_MAX_WIDTH || B.k != width) return HK_ERR_SHAPE;
    if (B.kind == HK_PVNET_RESIDUE && B.n % 32 != 0) return HK_ERR_SHAPE;
    if (B.kind == HK_PVNET_RESIDUE && !pvnet_normed_width(B.n)) return HK_ERR_UNSUPPORTED;
    width = B.n;
  }
  if (!q->x || !q->policy || !q->value || !q->policy_weight || !q->value_weight) return HK_ERR_NULL;
  const hk_pvnet_dense* d[3];
  for (int l = 0; l < q->nblocks; ++l)
    for (int i = 0, n = denses(q->block[l], d); i < n; ++i)
      if (!d[i]->weight) return HK_ERR_NULL;
  if (!all_aligned({q->x, q->policy, q->value, q->policy_weight, q->policy_bias, q->value_weight, q->value_bias}, 4))
    return HK_ERR_ALIGN;
  for (int l = 0; l < q->nblocks; ++l)
    for (int i = 0, n = denses(q->block[l], d); i < n; ++i)
      if (!all_aligned({d[i]->weight, d[i]->bias, d[i]->gn_scale, d[i]->gn_bias}, 4)) return HK_ERR_ALIGN;
  const uint64_t x_bytes = span_bytes(q->batch, q->x_stride, q->k0, sizeof(float));
  const uint64_t out_bytes[2] = {span_bytes(q->batch, q->policy_stride, q->actions, sizeof(float)),
                                 span_bytes(q->batch, q->value_stride, 1, sizeof(float))};
  if (q->batch > 0 && (!x_bytes || !out_bytes[0] || !out_bytes[1])) return HK_ERR_SHAPE;  // beyond 2^63 bytes
  const void* out[2] = {q->policy, q->value};
  for (int o = 0; o < 2; ++o) {
    auto shares = [&](const void* p, uint64_t bytes) { return overlap(out[o], out_bytes[o], p, bytes); };
    const uint64_t row = (uint64_t)width * sizeof(float);
    if (shares(q->x, x_bytes) || shares(q->policy_weight, row * (uint64_t)q->actions) || shares(q->value_weight, row) ||
        shares(q->policy_bias, (uint64_t)q->actions * sizeof(float)) || shares(q->value_bias, sizeof(float)))
      return HK_ERR_UNSUPPORTED;
    for (int l = 0; l < q->nblocks; ++l) {
      const hk_pvnet_block& B = q->block[l];
      const uint64_t vec = (uint64_t)B.n * sizeof(float);
      for (int i = 0, n = denses(B, d); i < n; ++i) {
        if (shares(d[i]->weight, vec * (uint64_t)(i == 1 ? B.n : B.k))) return HK_ERR_UNSUPPORTED;  // dense2 is [n, n]
        for (const void* p : {d[i]->bias, d[i]->gn_scale, d[i]->gn_bias})
          if (shares(p, vec)) return HK_ERR_UNSUPPORTED;
      }
    }
  }
  return HK_OK;
}

}  // namespace

extern "C" {

int hk_pvnet_forward(const hk_pvnet_desc* q, void* stream) {
  const int bad = validate(q);
  if (bad != HK_OK) return bad;
  if (q->batch == 0) return HK_OK;
  return mlp_launch(pvnet_kernel<HK_MLP_TILE_SMALL>, pvnet_kernel<HK_MLP_TILE_LARGE>, *q, (hipStream_t)stream);
}

// include/hironaka_hip_unified.h: hk_pvnet_forward's checks and launch shape (mlp_launch's), behind the gate
int hk_unified_pvnet_forward(const hk_pvnet_desc* q, const int32_t* gate, int32_t want, void* stream) {
  const int bad = validate(q);
  if (bad != HK_OK) return bad;
  if (!gate) return HK_ERR_NULL;
  if (!aligned(gate, 4)) return HK_ERR_ALIGN;
  if (q->batch == 0) return HK_OK;
  const int tr = mlp_row_tile(q->batch, q->flags);
  const auto kernel = tr == HK_MLP_TILE_LARGE ? pvnet_gated_kernel<HK_MLP_TILE_LARGE> : pvnet_gated_kernel<HK_MLP_TILE_SMALL>;
  return launch_kernel_lds(kernel, 48 * 1024, dim3((unsigned)workgroups(q->batch, tr)), dim3(kWave * mlp_waves(tr)),
                           mlp_lds_bytes(tr), (hipStream_t)stream, *q, gate, want);
}

}  // extern "C"
