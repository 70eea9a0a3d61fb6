// C ABI of hk_unified_expand and hk_unified_prior (include/hironaka_hip_unified.h, an addition within ABI 6): argument
// validation and launch of hk::unified_kind_kernel, hk::unified_expand_kernel and hk::unified_prior_kernel.  No
// allocation, no synchronisation; every status is decided before the first launch.  (hk_unified_pvnet_forward, the third
// entry of the header, lives with the kernel it gates: hk_pvnet.hip.)
#include "hk_unified_kernel.h"

using namespace hk;

extern "C" {

int hk_unified_expand(const hk_unified_expand_desc* q, void* stream) {
  if (!q) return HK_ERR_NULL;
  if (q->dtype != HK_F32) return HK_ERR_UNSUPPORTED;
  if (q->batch < 0 || q->num_nodes < 1 || q->max_points < 1 || q->dim < 2) return HK_ERR_SHAPE;
  if (q->dim > kUnifiedMaxDim) return HK_ERR_UNSUPPORTED;
  if (q->flags & ~(HK_UNIFIED_REPOSITION | HK_UNIFIED_SCALE_OBSERVATION)) return HK_ERR_UNSUPPORTED;
  // a parent state and the features of its successor share a slice; at least one slice has to fit
  const int64_t slice = (2 * (int64_t)q->max_points * q->dim + 2 * q->dim) | 1;
  if (slice * (int64_t)sizeof(float) > kSearchLdsBytes) return HK_ERR_UNSUPPORTED;
  if (q->batch == 0) return HK_OK;
  if (!q->embeddings || !q->parent || !q->action || !q->node || !q->kind || !q->net_in || !q->subset || !q->reward ||
      !q->discount_out)
    return HK_ERR_NULL;
  if (!all_aligned({q->embeddings, q->parent, q->action, q->node, q->kind, q->net_in, q->subset, q->reward,
                    q->discount_out}, 4))
    return HK_ERR_ALIGN;
  const int64_t len = (int64_t)q->max_points * q->dim + q->dim;
  const uint64_t games = (uint64_t)q->batch * sizeof(float);  // a [batch] array of 4-byte elements
  const uint64_t table = checked_mul(checked_mul((uint64_t)q->batch, (uint64_t)q->num_nodes), (uint64_t)len * sizeof(float));
  if (!table || table >> 63) return HK_ERR_SHAPE;
  // what a workgroup writes while others still read: no written range shares a byte with another range
  const void* written[6] = {q->embeddings, q->net_in, q->subset, q->reward, q->discount_out, q->kind};
  const uint64_t written_bytes[6] = {table, games * (uint64_t)len, games, games, games, sizeof(int32_t)};
  const void* read[3] = {q->parent, q->action, q->node};
  for (int i = 0; i < 6; ++i) {
    for (int j = i + 1; j < 6; ++j)
      if (overlap(written[i], written_bytes[i], written[j], written_bytes[j])) return HK_ERR_SHAPE;
    for (int j = 0; j < 3; ++j)
      if (overlap(written[i], written_bytes[i], read[j], games)) return HK_ERR_SHAPE;
  }
  UnifiedArgs a{};
  a.embeddings = static_cast<float*>(q->embeddings);
  a.parent = q->parent;
  a.action = q->action;
  a.node = q->node;
  a.kind = q->kind;
  a.net_in = static_cast<float*>(q->net_in);
  a.subset = q->subset;
  a.reward = static_cast<float*>(q->reward);
  a.discount_out = static_cast<float*>(q->discount_out);
  a.discount = q->discount;
  a.batch = q->batch;
  a.nodes = q->num_nodes;
  a.m = q->max_points;
  a.d = q->dim;
  a.reposition = (q->flags & HK_UNIFIED_REPOSITION) ? 1 : 0;
  a.scale = (q->flags & HK_UNIFIED_SCALE_OBSERVATION) ? 1 : 0;
  a.lds_stride = search_lds_stride(a.m, a.d);
  const LaneGeometry geo = lane_geometry(a.lds_stride, sizeof(float), a.batch);
  a.games_per_block = geo.per_block;
  const int st = launch_kernel(unified_kind_kernel<float>, dim3((unsigned)workgroups(a.batch, kUnifiedKindBlock)),
                               dim3(kUnifiedKindBlock), 0, (hipStream_t)stream, a, q->kind);
  if (st != HK_OK) return st;
  return launch_kernel(unified_expand_kernel<float>, dim3(geo.grid), dim3(kWave), geo.lds, (hipStream_t)stream, a);
}

int hk_unified_prior(const int32_t* kind, const void* agent_logits, const void* agent_value, const void* host_logits,
                     const void* host_value, const int32_t* subset, void* prior_out, void* value_out, int batch, int dim,
                     void* stream) {
  if (batch < 0 || dim < 2) return HK_ERR_SHAPE;
  if (dim > kUnifiedMaxDim) return HK_ERR_UNSUPPORTED;
  if (batch == 0) return HK_OK;
  if (!kind || !agent_logits || !agent_value || !host_logits || !host_value || !subset || !prior_out || !value_out)
    return HK_ERR_NULL;
  if (!all_aligned({kind, agent_logits, agent_value, host_logits, host_value, subset, prior_out, value_out}, 4))
    return HK_ERR_ALIGN;
  const int actions = (1 << dim) - dim - 1;
  const uint64_t games = (uint64_t)batch * sizeof(float);
  const void* read[6] = {kind, agent_logits, agent_value, host_logits, host_value, subset};
  const uint64_t read_bytes[6] = {sizeof(int32_t), games * (uint64_t)dim, games, games * (uint64_t)actions, games, games};
  for (int i = 0; i < 6; ++i)
    if (overlap(prior_out, games * (uint64_t)actions, read[i], read_bytes[i]) || overlap(value_out, games, read[i], read_bytes[i]))
      return HK_ERR_SHAPE;
  if (overlap(prior_out, games * (uint64_t)actions, value_out, games)) return HK_ERR_SHAPE;
  UnifiedPriorArgs a{kind, static_cast<const float*>(agent_logits), static_cast<const float*>(agent_value),
                     static_cast<const float*>(host_logits), static_cast<const float*>(host_value), subset,
                     static_cast<float*>(prior_out), static_cast<float*>(value_out), batch, dim, actions};
  return launch_kernel(unified_prior_kernel<float>, dim3((unsigned)workgroups((int64_t)batch * actions, 256)), dim3(256), 0,
                       (hipStream_t)stream, a);
}

}  // extern "C"
