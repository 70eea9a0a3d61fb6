// C ABI of hk_pv_loss (include/hironaka_hip_pvloss.h, an addition within ABI 6): argument validation and launch of
// hk::pv_loss_kernel.  No allocation, no synchronisation; every status is decided before the launch.
#include "hk_pvloss_kernel.h"

using namespace hk;

namespace {

uint64_t pvloss_tiles(int batch) { return ((uint64_t)batch + kPvLossTile - 1) / kPvLossTile; }

}  // namespace

extern "C" {

uint64_t hk_pv_loss_workspace_bytes(int batch) {
  if (batch < 0) return 0;
  const uint64_t slots = pvloss_tiles(batch) > 0 ? pvloss_tiles(batch) : 1;
  return checked_mul((uint64_t)kPvLossSlotOffset + slots, 8);
}

int hk_pv_loss(const hk_pv_loss_desc* q, void* stream) {
  if (!q) return HK_ERR_NULL;
  if (q->dtype != HK_F32 || q->flags != 0) return HK_ERR_UNSUPPORTED;
  if (q->batch < 0 || q->actions < 1 || q->actions > HK_PVLOSS_MAX_ACTIONS || q->num_samples < 0)
    return HK_ERR_SHAPE;
  const int64_t A = q->actions, B = q->batch, N = q->num_samples;
  if (q->logits_stride < A || q->target_policy_stride < A || q->dlogits_stride < A || q->value_stride < 1 ||
      q->dvalue_stride < 1)
    return HK_ERR_SHAPE;
  if (B == 0) return HK_OK;
  if (!q->logits || !q->value || !q->target_policy || !q->target_value || !q->dlogits || !q->dvalue || !q->loss ||
      !q->workspace || !q->status)
    return HK_ERR_NULL;
  if (N < 1 || (!q->index && N < B)) return HK_ERR_SHAPE;  // without an index row b takes sample b
  if (!all_aligned({q->logits, q->value, q->target_policy, q->target_value, q->weight, q->dlogits, q->dvalue,
                    q->row_loss, q->loss, q->status}, 4) ||
      !aligned(q->index, 8) || !aligned(q->workspace, 8))
    return HK_ERR_ALIGN;
  // what is read and what is written, with the bytes from its first to its last element (0: more than fits in 63 bits)
  const struct { const void* p; uint64_t bytes; } in[] = {
      {q->logits, span_bytes(B, q->logits_stride, A, 4)},
      {q->value, span_bytes(B, q->value_stride, 1, 4)},
      {q->target_policy, span_bytes(N, q->target_policy_stride, A, 4)},
      {q->target_value, span_bytes(N, 1, 1, 4)},
      {q->weight, span_bytes(N, 1, 1, 4)},
      {q->index, span_bytes(B, 1, 1, 8)},
  };
  const struct { const void* p; uint64_t bytes; } out[] = {
      {q->dlogits, span_bytes(B, q->dlogits_stride, A, 4)},
      {q->dvalue, span_bytes(B, q->dvalue_stride, 1, 4)},
      {q->row_loss, span_bytes(B, 1, 1, 4)},
      {q->loss, 4},
  };
  for (const auto& r : in)
    if (!r.bytes) return HK_ERR_SHAPE;
  for (const auto& w : out)
    if (!w.bytes) return HK_ERR_SHAPE;
  for (const auto& w : out)
    for (const auto& r : in)
      if (overlap(w.p, w.bytes, r.p, r.bytes)) return HK_ERR_UNSUPPORTED;
  PvLossArgs a{};
  a.logits = q->logits;
  a.value = q->value;
  a.target_policy = q->target_policy;
  a.target_value = q->target_value;
  a.weight = q->weight;
  a.index = q->index;
  a.dlogits = q->dlogits;
  a.dvalue = q->dvalue;
  a.row_loss = q->row_loss;
  a.loss = q->loss;
  a.ws = static_cast<unsigned long long*>(q->workspace);
  a.status = q->status;
  a.logits_stride = q->logits_stride;
  a.value_stride = q->value_stride;
  a.target_policy_stride = q->target_policy_stride;
  a.dlogits_stride = q->dlogits_stride;
  a.dvalue_stride = q->dvalue_stride;
  a.num_samples = N;
  a.batch = q->batch;
  a.actions = q->actions;
  int lg = 0;
  while (lg < 6 && (1 << lg) < q->actions) ++lg;
  a.lanes_log2 = lg;
  const dim3 grid((unsigned)pvloss_tiles(q->batch)), block(kPvLossThreads);
  return launch_kernel(pv_loss_kernel, grid, block, 0, (hipStream_t)stream, a);
}

}  // extern "C"
