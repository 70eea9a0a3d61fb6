// C ABI of hk_customgrad_forward / hk_customgrad_backward (include/hironaka_hip_customgrad.h, an addition within ABI 6):
// argument validation, the workspace's size and the launches of hk::customgrad_group_kernel, customgrad_forward_kernel,
// customgrad_rows_kernel and customgrad_params_kernel.  No allocation, no synchronisation; every status is decided before
// the first launch.  The two tables lie in device memory: their contents are the caller's (the header).
#include <utility>
#include <vector>

#include "hk_customgrad_kernel.h"

using namespace hk;

namespace {

CustomgradShape shape_of(const hk_customgrad_desc& g) {
  CustomgradShape S = {};
  const hk_customnet_desc& q = g.net;
  S.batch = q.batch, S.m = q.m, S.d = q.d, S.e = q.e, S.nblocks = q.nblocks, S.actions = q.actions;
  for (int l = 0; l < HK_PVNET_MAX_BLOCKS; ++l) S.n[l] = g.n[l], S.kind[l] = g.kind[l];
  return S;
}

// the sizes alone: what the layout needs to be meaningful
int sizes(const hk_customgrad_desc& g) {
  const hk_customnet_desc& q = g.net;
  if (q.nblocks < 1 || q.nblocks > HK_PVNET_MAX_BLOCKS || q.m < 1 || q.m > HK_CUSTOMNET_MAX_POINTS || q.d < 2 || q.e < 0 ||
      (int64_t)q.m * q.d + q.e > HK_PVNET_MAX_WIDTH || q.actions < 1 || q.actions > HK_PVNET_MAX_WIDTH - 1)
    return HK_ERR_SHAPE;
  for (int l = 0; l < q.nblocks; ++l) {
    if (g.n[l] < 1 || g.n[l] > HK_PVNET_MAX_WIDTH) return HK_ERR_SHAPE;
    if (g.kind[l] != HK_PVNET_DENSE && g.kind[l] != HK_PVNET_RESIDUE) return HK_ERR_SHAPE;
    if (g.kind[l] == HK_PVNET_RESIDUE && !pvnet_normed_width(g.n[l])) return HK_ERR_SHAPE;
  }
  if (g.n[q.nblocks - 1] != q.n_last || (int64_t)q.n_last + q.e > HK_PVNET_MAX_WIDTH) return HK_ERR_SHAPE;
  return q.batch > HK_PVGRAD_MAX_BATCH ? HK_ERR_SHAPE : HK_OK;
}

uint64_t workspace_bytes(const CustomgradShape& S) {
  const uint64_t words = (uint64_t)customgrad_int_words(S) + (uint64_t)customgrad_float_words(S);
  return (words * 4 + 15) & ~(uint64_t)15;
}

int validate(const hk_customgrad_desc* g, bool backward) {
  if (!g) return HK_ERR_NULL;
  const hk_customnet_desc& q = g->net;
  {
    // everything hk_customnet_forward refuses but its own workspace's size, by asking it: without rows it launches nothing
    hk_customnet_desc probe = q;
    if (probe.batch > 0) probe.batch = 0;
    probe.workspace_bytes = ~(uint64_t)0;
    if (const int bad = hk_customnet_forward(&probe, nullptr)) return bad;
  }
  if (q.gate || (q.flags & (HK_CUSTOMNET_FORCE_TILE_SMALL | HK_CUSTOMNET_FORCE_TILE_LARGE))) return HK_ERR_UNSUPPORTED;
  if (const int bad = sizes(*g)) return bad;
  if (backward && (g->grad_policy_stride < q.actions || g->grad_value_stride < 1)) return HK_ERR_SHAPE;
  const CustomgradShape S = shape_of(*g);
  const uint64_t need = q.batch > 0 ? workspace_bytes(S) : 0;
  if (q.workspace_bytes < need) return HK_ERR_SHAPE;
  const uint64_t kh = (uint64_t)(q.n_last + q.e);
  if (backward) {
    if (!g->grad_table || !g->grads || !g->grad_policy || !g->grad_value) return HK_ERR_NULL;
    if (g->policy.d_weight < 0 || g->value.d_weight < 0) return HK_ERR_NULL;
    if (!aligned(g->grad_table, 8) || !all_aligned({g->grads, g->grad_policy, g->grad_value}, 4)) return HK_ERR_ALIGN;
    const std::pair<int64_t, uint64_t> heads[4] = {{g->policy.d_weight, kh * (uint64_t)q.actions},
                                                   {g->policy.d_bias, (uint64_t)q.actions},
                                                   {g->value.d_weight, kh},
                                                   {g->value.d_bias, 1}};
    for (const auto& h : heads)
      if (h.first >= 0 && (uint64_t)h.first + h.second > g->grad_floats) return HK_ERR_SHAPE;
  }
  if (q.batch == 0) return HK_OK;

  // what is written against what is read, and against each other
  std::vector<std::pair<const void*, uint64_t>> rd, wr;
  const uint64_t x_bytes = span_bytes(q.batch, q.x_stride, q.m * q.d + q.e, sizeof(float));
  const uint64_t policy_bytes = span_bytes(q.batch, q.policy_stride, q.actions, sizeof(float));
  const uint64_t value_bytes = span_bytes(q.batch, q.value_stride, 1, sizeof(float));
  const uint64_t gp_bytes = backward ? span_bytes(q.batch, g->grad_policy_stride, q.actions, sizeof(float)) : 1;
  const uint64_t gv_bytes = backward ? span_bytes(q.batch, g->grad_value_stride, 1, sizeof(float)) : 1;
  if (!x_bytes || !policy_bytes || !value_bytes || !gp_bytes || !gv_bytes) return HK_ERR_SHAPE;  // beyond 2^63 bytes
  const uint64_t records = (uint64_t)q.m * (uint64_t)q.nblocks;
  rd.emplace_back(q.x, x_bytes);
  rd.emplace_back(q.policy_weight, kh * (uint64_t)q.actions * sizeof(float));
  rd.emplace_back(q.value_weight, kh * sizeof(float));
  rd.emplace_back(q.policy_bias, (uint64_t)q.actions * sizeof(float));
  rd.emplace_back(q.value_bias, sizeof(float));
  rd.emplace_back(q.towers, records * sizeof(hk_pvnet_block));
  wr.emplace_back(q.workspace, need);
  if (backward) {
    rd.emplace_back(g->grad_table, records * sizeof(hk_customgrad_block));
    rd.emplace_back(q.value, value_bytes);
    rd.emplace_back(q.policy, policy_bytes);
    rd.emplace_back(g->grad_policy, gp_bytes);
    rd.emplace_back(g->grad_value, gv_bytes);
    wr.emplace_back(g->grads, g->grad_floats * sizeof(float));
  } else {
    wr.emplace_back(q.policy, policy_bytes);
    wr.emplace_back(q.value, value_bytes);
  }
  for (size_t i = 0; i < wr.size(); ++i) {
    for (const auto& r : rd)
      if (overlap(wr[i].first, wr[i].second, r.first, r.second)) return HK_ERR_UNSUPPORTED;
    for (size_t j = i + 1; j < wr.size(); ++j)
      if (overlap(wr[i].first, wr[i].second, wr[j].first, wr[j].second)) return HK_ERR_UNSUPPORTED;
  }
  return HK_OK;
}

const dim3 kRowBlock(kWave * mlp_waves(kPvgradTile));

int forward(const hk_customgrad_desc* g, hipStream_t stream) {
  const int bad = validate(g, false);
  if (bad != HK_OK) return bad;
  const hk_customnet_desc& q = g->net;
  if (q.batch == 0) return HK_OK;
  const CustomgradShape S = shape_of(*g);
  CustomgradGroupArgs a;
  a.x = static_cast<const float*>(q.x), a.ws = static_cast<int32_t*>(q.workspace), a.x_stride = q.x_stride;
  a.batch = q.batch, a.m = q.m, a.d = q.d;
  const int grouped = launch_kernel(customgrad_group_kernel, dim3(1), dim3(kCustomgradGroupThreads), 0, stream, a);
  if (grouped != HK_OK) return grouped;
  return launch_kernel_lds(customgrad_forward_kernel, 48 * 1024, dim3((unsigned)customgrad_max_tiles(q.batch, q.m)), kRowBlock,
                           mlp_lds_bytes(kPvgradTile), stream, q, S);
}

int backward(const hk_customgrad_desc* g, hipStream_t stream) {
  const int bad = validate(g, true);
  if (bad != HK_OK) return bad;
  const hk_customnet_desc& q = g->net;
  if (q.batch == 0) return HK_OK;
  {
    CustomgradRowsArgs a;
    a.q = q, a.S = shape_of(*g);
    a.grad_policy = static_cast<const float*>(g->grad_policy), a.grad_value = static_cast<const float*>(g->grad_value);
    a.grad_policy_stride = g->grad_policy_stride, a.grad_value_stride = g->grad_value_stride;
    const int status = launch_kernel_lds(customgrad_rows_kernel, 48 * 1024, dim3((unsigned)customgrad_max_tiles(q.batch, q.m)),
                                         kRowBlock, mlp_lds_bytes(kPvgradTile), stream, a);
    if (status != HK_OK) return status;
  }
  CustomgradParamsArgs a;
  a.S = shape_of(*g);
  a.towers = q.towers, a.table = g->grad_table, a.ws = static_cast<const int32_t*>(q.workspace);
  a.grads = static_cast<float*>(g->grads), a.policy = g->policy, a.value = g->value;
  a.tower_tiles = customgrad_tower_tiles(a.S);
  const int tiles = q.m * a.tower_tiles + customgrad_head_tiles(a.S);
  return launch_kernel(customgrad_params_kernel, dim3((unsigned)tiles), dim3(kPvgradParamThreads), 0, stream, a);
}

}  // namespace

extern "C" {

uint64_t hk_customgrad_workspace_bytes(const hk_customgrad_desc* g) {
  return g && g->net.batch > 0 && sizes(*g) == HK_OK ? workspace_bytes(shape_of(*g)) : 0;
}

int hk_customgrad_forward(const hk_customgrad_desc* g, void* stream) { return forward(g, (hipStream_t)stream); }

int hk_customgrad_backward(const hk_customgrad_desc* g, void* stream) { return backward(g, (hipStream_t)stream); }

}  // extern "C"
