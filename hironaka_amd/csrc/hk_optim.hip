// C ABI of hk_optim_prepare / hk_optim_apply (include/hironaka_hip_optim.h, additions within ABI 6): argument
// validation and launch of hk::optim_prepare_kernel / hk::optim_apply_kernel.  No allocation, no synchronisation; every
// status is decided before the launch.
#include "hk_optim_kernel.h"

using namespace hk;

namespace {

constexpr uint32_t kPrepareFlags = HK_OPTIM_LAST | HK_OPTIM_ADVANCE | HK_OPTIM_NO_CLIP;
constexpr uint32_t kApplyFlags = HK_OPTIM_KEEP_GRADS | HK_OPTIM_NESTEROV;
constexpr int kMaxUsed = 4;

// the pointers of an entry that the launch touches: prepare the gradient alone, apply what the kind uses
int used(const hk_optim_desc* q, const hk_optim_tensor& t, bool apply, const void* out[kMaxUsed]) {
  int n = 0;
  out[n++] = t.grad;
  if (!apply || q->kind == HK_OPTIM_SCALE) return n;
  out[n++] = t.param;
  if (q->kind == HK_OPTIM_ADAM || q->momentum != 0.0) out[n++] = t.state1;
  if (q->kind == HK_OPTIM_ADAM) out[n++] = t.state2;
  return n;
}

// the checks both entry points share; HK_OK: go on
int validate(const hk_optim_desc* q, bool apply) {
  if (!q) return HK_ERR_NULL;
  if (q->dtype != HK_F32 && q->dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (q->kind != HK_OPTIM_SCALE && q->kind != HK_OPTIM_SGD && q->kind != HK_OPTIM_ADAM) return HK_ERR_UNSUPPORTED;
  if (q->flags & ~(kPrepareFlags | kApplyFlags)) return HK_ERR_UNSUPPORTED;
  if (apply && q->kind == HK_OPTIM_SCALE && (q->flags & HK_OPTIM_KEEP_GRADS)) return HK_ERR_UNSUPPORTED;
  if (q->ntensors < 0 || q->ntensors > HK_OPTIM_MAX_TENSORS || q->slot_base < 0) return HK_ERR_SHAPE;
  const size_t esz = elem_size(q->dtype);
  const void* ptr[kMaxUsed];
  for (int i = 0; i < q->ntensors; ++i)
    if (q->tensor[i].numel < 0 || (uint64_t)q->tensor[i].numel > (UINT64_MAX >> 4)) return HK_ERR_SHAPE;
  if (!q->state || (!apply && !q->workspace)) return HK_ERR_NULL;
  for (int i = 0; i < q->ntensors; ++i) {
    const hk_optim_tensor& t = q->tensor[i];
    const int n = used(q, t, apply, ptr);
    for (int k = 0; k < n; ++k)
      if (t.numel > 0 && !ptr[k]) return HK_ERR_NULL;
  }
  if (!aligned(q->state, 8) || (!apply && (!aligned(q->workspace, 8) || !aligned(q->lr_dev, 8)))) return HK_ERR_ALIGN;
  for (int i = 0; i < q->ntensors; ++i) {
    const hk_optim_tensor& t = q->tensor[i];
    const int n = used(q, t, apply, ptr);
    for (int k = 0; k < n; ++k)
      if (t.numel > 0 && !aligned(ptr[k], esz)) return HK_ERR_ALIGN;
  }
  if (!apply) return HK_OK;  // prepare writes no tensor: its ranges may coincide
  const void* other[kMaxUsed];
  for (int i = 0; i < q->ntensors; ++i) {
    const hk_optim_tensor& t = q->tensor[i];
    const uint64_t bytes = (uint64_t)t.numel * esz;
    const int n = used(q, t, apply, ptr);
    for (int j = i; j < q->ntensors; ++j) {
      const hk_optim_tensor& u = q->tensor[j];
      const uint64_t bytes2 = (uint64_t)u.numel * esz;
      const int n2 = used(q, u, apply, other);
      for (int k = 0; k < n; ++k)
        for (int l = (j == i ? k + 1 : 0); l < n2; ++l)
          if (overlap(ptr[k], bytes, other[l], bytes2)) return HK_ERR_UNSUPPORTED;
    }
  }
  return HK_OK;
}

void scalars(const hk_optim_desc* q, OptimArgs& a) {
  a.state = static_cast<hk_optim_state*>(q->state);
  a.ws = static_cast<unsigned long long*>(q->workspace);
  a.lr_dev = q->lr_dev;
  a.lr = q->lr;
  a.beta1 = q->beta1;
  a.beta2 = q->beta2;
  a.eps = q->eps;
  a.weight_decay = q->weight_decay;
  a.momentum = q->momentum;
  a.dampening = q->dampening;
  a.max_norm = q->max_norm;
  a.ntensors = q->ntensors;
  a.slot_base = q->slot_base;
  a.flags = q->flags;
}

template <typename T, int KIND>
int launch_apply(const OptimArgs& a, hipStream_t stream) {
  return launch_kernel(optim_apply_kernel<T, KIND>, dim3(a.blocks), dim3(kOptimThreads), 0, stream, a);
}

template <typename T>
int launch_apply_kind(int kind, const OptimArgs& a, hipStream_t stream) {
  if (kind == HK_OPTIM_ADAM) return launch_apply<T, HK_OPTIM_ADAM>(a, stream);
  if (kind == HK_OPTIM_SGD) return launch_apply<T, HK_OPTIM_SGD>(a, stream);
  return launch_apply<T, HK_OPTIM_SCALE>(a, stream);
}

}  // namespace

extern "C" {

uint64_t hk_optim_workspace_bytes(int64_t total_workgroups) {
  if (total_workgroups < 0 || total_workgroups > 0x7FFFFFFFll) return 0;
  const uint64_t slots = total_workgroups > 0 ? (uint64_t)total_workgroups : 1;
  return ((uint64_t)kTicketSlotOffset + slots) * 8;
}

int hk_optim_prepare(const hk_optim_desc* q, void* stream) {
  const int bad = validate(q, false);
  if (bad != HK_OK) return bad;
  const size_t esz = elem_size(q->dtype);
  OptimArgs a{};
  uint64_t blocks = 0;
  for (int i = 0; i < q->ntensors; ++i) {
    a.t[i] = q->tensor[i];
    a.first[i] = (uint32_t)blocks;
    blocks += ((uint64_t)q->tensor[i].numel * esz + kOptimChunkBytes - 1) / kOptimChunkBytes;
    if (blocks + (uint64_t)q->slot_base > 0x7FFFFFFFull) return HK_ERR_SHAPE;
  }
  for (int i = q->ntensors; i <= HK_OPTIM_MAX_TENSORS; ++i) a.first[i] = (uint32_t)blocks;
  const bool reduce_only = blocks == 0 && (q->flags & HK_OPTIM_LAST) && q->slot_base > 0;
  if (blocks == 0 && !reduce_only) return HK_OK;
  scalars(q, a);
  a.blocks = (uint32_t)blocks;
  const dim3 grid(reduce_only ? 1u : (unsigned)blocks), block(kOptimThreads);
  if (q->dtype == HK_F64) return launch_kernel(optim_prepare_kernel<double>, grid, block, 0, (hipStream_t)stream, a);
  return launch_kernel(optim_prepare_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
}

int hk_optim_apply(const hk_optim_desc* q, void* stream) {
  const int bad = validate(q, true);
  if (bad != HK_OK) return bad;
  const size_t esz = elem_size(q->dtype);
  OptimArgs a{};
  uint64_t blocks = 0;
  const void* ptr[kMaxUsed];
  for (int i = 0; i < q->ntensors; ++i) {
    const hk_optim_tensor& t = q->tensor[i];
    a.t[i] = t;
    a.first[i] = (uint32_t)blocks;
    if (t.numel == 0) continue;
    const int n = used(q, t, true, ptr);
    const ChunkPlan plan = chunk_plan<kOptimThreads * kOptimUnroll, kOptimChunkBytes>(ptr, n, t.numel, esz);
    a.head[i] = (int8_t)plan.head;
    blocks += plan.chunks;
    if (blocks > 0x7FFFFFFFull) return HK_ERR_SHAPE;
  }
  for (int i = q->ntensors; i <= HK_OPTIM_MAX_TENSORS; ++i) a.first[i] = (uint32_t)blocks;
  if (blocks == 0) return HK_OK;
  scalars(q, a);
  a.blocks = (uint32_t)blocks;
  if (q->dtype == HK_F64) return launch_apply_kind<double>(q->kind, a, (hipStream_t)stream);
  return launch_apply_kind<float>(q->kind, a, (hipStream_t)stream);
}

}  // extern "C"
