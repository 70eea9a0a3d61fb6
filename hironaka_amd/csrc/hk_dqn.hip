// C ABI of hk_dqn_td / hk_polyak_update (include/hironaka_hip_dqn.h, additions within ABI 6): argument validation and
// launch of hk::dqn_td_kernel / hk::polyak_kernel.  No allocation, no synchronisation; every status is decided before
// the launch.
#include "hk_dqn_kernel.h"

using namespace hk;

namespace {

uint64_t dqn_tiles(int batch) { return ((uint64_t)batch + kDqnTile - 1) / kDqnTile; }

}  // namespace

extern "C" {

uint64_t hk_dqn_td_workspace_bytes(int batch) {
  if (batch < 0) return 0;
  const uint64_t slots = dqn_tiles(batch) > 0 ? dqn_tiles(batch) : 1;
  return ((uint64_t)kDqnSlotOffset + slots) * 8;
}

int hk_dqn_td(const hk_dqn_td_desc* q, void* stream) {
  if (!q) return HK_ERR_NULL;
  if (q->dtype != HK_F32 && q->dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (q->batch < 0 || q->num_actions < 1 || q->num_actions > HK_DQN_MAX_ACTIONS) return HK_ERR_SHAPE;
  const int64_t A = q->num_actions;
  if (q->q_stride < A || q->next_q_stride < A || q->dq_stride < A) return HK_ERR_SHAPE;
  if (q->batch == 0) return HK_OK;
  if (!q->q || !q->next_q || !q->actions || !q->rewards || !q->dones || !q->dq || !q->loss || !q->workspace ||
      !q->status)
    return HK_ERR_NULL;
  const size_t esz = elem_size(q->dtype);
  if (!aligned(q->q, esz) || !aligned(q->next_q, esz) || !aligned(q->dq, esz) || !aligned(q->loss, esz) ||
      !aligned(q->target, esz) || !aligned(q->row_loss, esz) || !aligned(q->actions, 4) || !aligned(q->rewards, 4) ||
      !aligned(q->status, 4) || !aligned(q->workspace, 8))
    return HK_ERR_ALIGN;
  const uint64_t q_bytes = span_bytes(q->batch, q->q_stride, q->num_actions, esz);
  const uint64_t nq_bytes = span_bytes(q->batch, q->next_q_stride, q->num_actions, esz);
  const uint64_t dq_bytes = span_bytes(q->batch, q->dq_stride, q->num_actions, esz);
  if (!q_bytes || !nq_bytes || !dq_bytes) return HK_ERR_SHAPE;
  if (overlap(q->dq, dq_bytes, q->q, q_bytes) || overlap(q->dq, dq_bytes, q->next_q, nq_bytes))
    return HK_ERR_UNSUPPORTED;
  DqnArgs a{};
  a.q = q->q;
  a.next_q = q->next_q;
  a.actions = q->actions;
  a.rewards = q->rewards;
  a.dones = q->dones;
  a.target = q->target;
  a.row_loss = q->row_loss;
  a.dq = q->dq;
  a.loss = q->loss;
  a.ws = static_cast<unsigned long long*>(q->workspace);
  a.status = q->status;
  a.q_stride = q->q_stride;
  a.next_q_stride = q->next_q_stride;
  a.dq_stride = q->dq_stride;
  a.gamma = (float)q->gamma;
  a.batch = q->batch;
  a.num_actions = q->num_actions;
  int lg = 0;
  while (lg < 6 && (1 << lg) < q->num_actions) ++lg;
  a.lanes_log2 = lg;
  const dim3 grid((unsigned)dqn_tiles(q->batch)), block(kDqnThreads);
  if (q->dtype == HK_F64) return launch_kernel(dqn_td_kernel<double>, grid, block, 0, (hipStream_t)stream, a);
  return launch_kernel(dqn_td_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
}

int hk_polyak_update(const hk_polyak_desc* q, void* stream) {
  if (!q) return HK_ERR_NULL;
  if (q->dtype != HK_F32 && q->dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (q->ntensors < 0 || q->ntensors > HK_POLYAK_MAX_TENSORS) return HK_ERR_SHAPE;
  const size_t esz = elem_size(q->dtype);
  for (int i = 0; i < q->ntensors; ++i) {
    const hk_polyak_tensor& t = q->tensor[i];
    if (t.numel < 0 || (uint64_t)t.numel > (UINT64_MAX >> 4)) return HK_ERR_SHAPE;
    if (t.numel > 0 && (!t.src || !t.dst)) return HK_ERR_NULL;
  }
  for (int i = 0; i < q->ntensors; ++i) {
    const hk_polyak_tensor& t = q->tensor[i];
    if (t.numel > 0 && (!aligned(t.src, esz) || !aligned(t.dst, esz))) return HK_ERR_ALIGN;
  }
  for (int i = 0; i < q->ntensors; ++i) {
    const hk_polyak_tensor& t = q->tensor[i];
    const uint64_t bytes = (uint64_t)t.numel * esz;
    for (int j = 0; j < q->ntensors; ++j) {
      const hk_polyak_tensor& u = q->tensor[j];
      const uint64_t other = (uint64_t)u.numel * esz;
      if (overlap(t.dst, bytes, u.src, other) || (j != i && overlap(t.dst, bytes, u.dst, other)))
        return HK_ERR_UNSUPPORTED;
    }
  }
  PolyakArgs a{};
  uint64_t blocks = 0;
  for (int i = 0; i < q->ntensors; ++i) {
    const hk_polyak_tensor& t = q->tensor[i];
    PolyakTensor& k = a.t[i];
    k.src = t.src;
    k.dst = t.dst;
    k.numel = t.numel;
    a.first[i] = (uint32_t)blocks;
    if (t.numel == 0) continue;
    const void* const ptr[2] = {t.dst, t.src};
    const ChunkPlan plan = chunk_plan<kPolyakThreads * kPolyakUnroll, kPolyakChunkBytes>(ptr, 2, t.numel, esz);
    k.head = plan.head;
    blocks += plan.chunks;
    if (blocks > 0x7FFFFFFFull) return HK_ERR_SHAPE;
  }
  for (int i = q->ntensors; i <= HK_POLYAK_MAX_TENSORS; ++i) a.first[i] = (uint32_t)blocks;
  if (blocks == 0) return HK_OK;
  a.tau = q->tau;
  a.rest = 1.0 - q->tau;
  a.ntensors = q->ntensors;
  const dim3 grid((unsigned)blocks), block(kPolyakThreads);
  if (q->dtype == HK_F64) return launch_kernel(polyak_kernel<double>, grid, block, 0, (hipStream_t)stream, a);
  return launch_kernel(polyak_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
}

}  // extern "C"
