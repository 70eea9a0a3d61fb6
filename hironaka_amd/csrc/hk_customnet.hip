// C ABI of hk_customnet_forward (include/hironaka_hip_customnet.h, an addition within ABI 6): argument validation and the
// two launches, hk::customnet_group_kernel and hk::customnet_kernel.  No allocation, no synchronisation; every status is
// decided before the first launch.  The tower table lies in device memory: its contents are the caller's (the header).
#include "hk_customnet_kernel.h"

using namespace hk;

namespace {

constexpr uint32_t kDescFlags = HK_CUSTOMNET_RAW_VALUE | HK_CUSTOMNET_FORCE_TILE_SMALL | HK_CUSTOMNET_FORCE_TILE_LARGE;

uint64_t workspace_bytes(int64_t batch, int32_t m) {
  if (batch < 0 || m < 1 || m > HK_CUSTOMNET_MAX_POINTS) return 0;
  const uint64_t words = kCustomnetHeader + 4 * (uint64_t)customnet_max_tiles(batch, m) + 2 * (uint64_t)batch;
  return (words * sizeof(int32_t) + 15) & ~(uint64_t)15;
}

int validate(const hk_customnet_desc* q) {
  if (const int bad = mlp_check_desc(q, kDescFlags)) return bad;
  if (mlp_forces_both_tiles(q->flags)) return HK_ERR_UNSUPPORTED;
  if (q->d < 2 || q->m < 1 || q->m > HK_CUSTOMNET_MAX_POINTS || q->e < 0) return HK_ERR_SHAPE;
  if ((int64_t)q->m * q->d + q->e > HK_PVNET_MAX_WIDTH) return HK_ERR_SHAPE;
  if (q->n_last < 1 || (int64_t)q->n_last + q->e > HK_PVNET_MAX_WIDTH) return HK_ERR_SHAPE;
  if (q->nblocks < 1 || q->nblocks > HK_PVNET_MAX_BLOCKS) return HK_ERR_SHAPE;
  if (q->actions < 1 || q->actions > HK_PVNET_MAX_WIDTH - 1) return HK_ERR_SHAPE;
  if (q->batch < 0 || q->x_stride < 0 || q->policy_stride < q->actions || q->value_stride < 1) return HK_ERR_SHAPE;
  if (!q->x || !q->policy || !q->value || !q->towers || !q->policy_weight || !q->value_weight || !q->workspace)
    return HK_ERR_NULL;
  if (!all_aligned({q->x, q->policy, q->value, q->policy_weight, q->policy_bias, q->value_weight, q->value_bias, q->gate}, 4) ||
      !aligned(q->towers, 8) || !aligned(q->workspace, 16))
    return HK_ERR_ALIGN;
  const int K = q->m * q->d + q->e;
  const uint64_t x_bytes = span_bytes(q->batch, q->x_stride, K, sizeof(float));
  const uint64_t out_bytes[2] = {span_bytes(q->batch, q->policy_stride, q->actions, sizeof(float)),
                                 span_bytes(q->batch, q->value_stride, 1, sizeof(float))};
  if (q->batch > 0 && (!x_bytes || !out_bytes[0] || !out_bytes[1])) return HK_ERR_SHAPE;  // beyond 2^63 bytes
  const uint64_t need = workspace_bytes(q->batch, q->m);
  if (q->workspace_bytes < need) return HK_ERR_SHAPE;
  const void* out[2] = {q->policy, q->value};
  const uint64_t row = (uint64_t)(q->n_last + q->e) * sizeof(float);
  for (int o = 0; o < 2; ++o) {
    auto shares = [&](const void* p, uint64_t bytes) { return overlap(out[o], out_bytes[o], p, bytes); };
    if (shares(q->x, x_bytes) || shares(q->policy_weight, row * (uint64_t)q->actions) || shares(q->value_weight, row) ||
        shares(q->policy_bias, (uint64_t)q->actions * sizeof(float)) || shares(q->value_bias, sizeof(float)) ||
        shares(q->towers, (uint64_t)q->m * q->nblocks * sizeof(hk_pvnet_block)) || shares(q->workspace, need))
      return HK_ERR_UNSUPPORTED;
  }
  return HK_OK;
}

}  // namespace

extern "C" {

uint64_t hk_customnet_workspace_bytes(int64_t batch, int32_t m) { return workspace_bytes(batch, m); }

int hk_customnet_forward(const hk_customnet_desc* q, void* stream) {
  const int bad = validate(q);
  if (bad != HK_OK) return bad;
  if (q->batch == 0) return HK_OK;
  const int tr = mlp_row_tile(q->batch, q->flags);
  const int grouped = launch_kernel(customnet_group_kernel, dim3((unsigned)workgroups(q->batch, kCustomnetGroupThreads)), dim3(kCustomnetGroupThreads), 0, (hipStream_t)stream, *q, tr);
  if (grouped != HK_OK) return grouped;
  const auto kernel = tr == HK_MLP_TILE_LARGE ? customnet_kernel<HK_MLP_TILE_LARGE> : customnet_kernel<HK_MLP_TILE_SMALL>;
  return launch_kernel_lds(kernel, 48 * 1024, dim3((unsigned)(workgroups(q->batch, tr) + q->m + 1)), dim3(kWave * mlp_waves(tr)),
                           mlp_lds_bytes(tr), (hipStream_t)stream, *q);
}

}  // extern "C"
