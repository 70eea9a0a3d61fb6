// C ABI of hk_train_mlp_forward / hk_train_mlp_backward (include/hironaka_hip_mlp_train.h, an addition within ABI 6):
// argument validation and one launch per layer of hk::mlp_train_forward_kernel / hk::mlp_train_backward_kernel.  No
// allocation, no synchronisation; every status is decided before the first launch.
#include <utility>
#include <vector>

#include "hk_mlp_train_kernel.h"

using namespace hk;

namespace {

constexpr uint32_t kLayerFlags = HK_MLP_RELU | HK_MLP_TRAIN_BN;

// the byte ranges (pointer, bytes) that the launches read, or write
using Ranges = std::vector<std::pair<const void*, uint64_t>>;

bool is_bn(const hk_mlp_train_layer& L) { return L.flags & HK_MLP_TRAIN_BN; }

// two dz of [batch, the widest layer after the first]
uint64_t workspace_bytes(const hk_mlp_train_desc* q) {
  if (!q || q->nlayers < 2 || q->nlayers > HK_MLP_MAX_LAYERS || q->batch <= 0) return 0;
  int64_t widest = 0;
  for (int l = 1; l < q->nlayers; ++l) widest = q->layer[l].n > widest ? q->layer[l].n : widest;
  return widest > 0 ? (uint64_t)2 * (uint64_t)q->batch * (uint64_t)widest * sizeof(float) : 0;
}

int validate(const hk_mlp_train_desc* q, bool backward) {
  if (const int bad = mlp_check_desc(q, HK_MLP_INPUT_RELU)) return bad;
  if (q->batch > HK_MLP_TRAIN_MAX_BATCH || (backward && q->grad_stride < 0)) return HK_ERR_SHAPE;
  int64_t width = 0;
  if (const int bad = mlp_check_sizes(q, kLayerFlags, width)) return bad;
  bool any_bn = false;
  for (int l = 0; l < q->nlayers; ++l) any_bn = any_bn || is_bn(q->layer[l]);
  if (any_bn && q->batch == 1) return HK_ERR_SHAPE;
  if (backward && q->workspace_bytes < workspace_bytes(q)) return HK_ERR_SHAPE;
  if (mlp_input_missing(q)) return HK_ERR_NULL;
  if (backward && (!q->grad_out || (q->nlayers > 1 && !q->workspace))) return HK_ERR_NULL;
  for (int l = 0; l < q->nlayers; ++l) {
    const hk_mlp_train_layer& L = q->layer[l];
    if (!L.weight || !L.act) return HK_ERR_NULL;
    if (is_bn(L) && (!L.z || !L.mean || !L.inv || !L.running_mean || !L.running_var)) return HK_ERR_NULL;
    if (backward && !L.d_weight) return HK_ERR_NULL;
    if (!is_bn(L) && (L.bn_weight || L.bn_bias || L.running_mean || L.running_var || L.num_batches_tracked ||
                      L.d_bn_weight || L.d_bn_bias))
      return HK_ERR_UNSUPPORTED;
  }
  if (!all_aligned({q->x0, q->x1, q->grad_out, q->workspace}, 4)) return HK_ERR_ALIGN;
  for (int l = 0; l < q->nlayers; ++l) {
    const hk_mlp_train_layer& L = q->layer[l];
    if (!all_aligned({L.weight, L.bias, L.bn_weight, L.bn_bias, L.running_mean, L.running_var, L.z, L.act, L.mean, L.inv,
                      L.d_weight, L.d_bias, L.d_bn_weight, L.d_bn_bias}, 4) || !aligned(L.num_batches_tracked, 8))
      return HK_ERR_ALIGN;
  }
  // what is read and what is written
  Ranges rd, wr;
  const uint64_t B = (uint64_t)q->batch;
  uint64_t x0_bytes, x1_bytes;
  const uint64_t grad_bytes = backward ? span_bytes(q->batch, q->grad_stride, width, sizeof(float)) : 1;
  if (!mlp_input_spans(q, x0_bytes, x1_bytes) || (q->batch > 0 && !grad_bytes)) return HK_ERR_SHAPE;  // beyond 2^63 bytes
  rd.emplace_back(q->x0, x0_bytes);
  if (q->k1 > 0) rd.emplace_back(q->x1, x1_bytes);
  if (backward) {
    rd.emplace_back(q->grad_out, grad_bytes);
    wr.emplace_back(q->workspace, workspace_bytes(q));
  }
  for (int l = 0; l < q->nlayers; ++l) {
    const hk_mlp_train_layer& L = q->layer[l];
    const uint64_t vec = (uint64_t)L.n * sizeof(float);
    rd.emplace_back(L.weight, vec * (uint64_t)L.k);
    for (const void* p : {L.bias, L.bn_weight, L.bn_bias}) rd.emplace_back(p, vec);
    Ranges& saved = backward ? rd : wr;
    saved.emplace_back(L.act, vec * B);
    if (is_bn(L)) {
      saved.emplace_back(L.z, vec * B);
      saved.emplace_back(L.mean, vec);
      saved.emplace_back(L.inv, vec);
    }
    if (!backward) {
      wr.emplace_back(L.running_mean, vec);
      wr.emplace_back(L.running_var, vec);
      wr.emplace_back(L.num_batches_tracked, 8);
    } else {
      wr.emplace_back(L.d_weight, vec * (uint64_t)L.k);
      for (const void* p : {L.d_bias, L.d_bn_weight, L.d_bn_bias}) wr.emplace_back(p, vec);
    }
  }
  for (size_t i = 0; i < wr.size(); ++i) {
    for (const auto& r : rd)
      if (overlap(wr[i].first, wr[i].second, r.first, r.second)) return HK_ERR_UNSUPPORTED;
    for (size_t j = i + 1; j < wr.size(); ++j)
      if (overlap(wr[i].first, wr[i].second, wr[j].first, wr[j].second)) return HK_ERR_UNSUPPORTED;
  }
  return HK_OK;
}

template <int RT>
int launch_layer(bool backward, const TrainArgs& a, hipStream_t stream) {
  auto kernel = backward ? &mlp_train_backward_kernel<RT> : &mlp_train_forward_kernel<RT>;
  return launch_kernel_lds(kernel, 48 * 1024, dim3((unsigned)workgroups(a.L.n, kTrainCols)), dim3(kTrainThreads),
                           train_lds_bytes(RT), stream, a);
}

int run(const hk_mlp_train_desc* q, bool backward, hipStream_t stream) {
  const int bad = validate(q, backward);
  if (bad != HK_OK) return bad;
  if (q->batch == 0) return HK_OK;
  const bool large = train_rt(q->batch) == kTrainRtLarge;
  float* const ws0 = static_cast<float*>(q->workspace);
  float* ws[2] = {ws0, ws0 + workspace_bytes(q) / (2 * sizeof(float))};  // the workspace's halves
  for (int i = 0; i < q->nlayers; ++i) {
    const int l = backward ? q->nlayers - 1 - i : i;
    TrainArgs a = {};
    a.L = q->layer[l];
    a.a_in = l > 0 ? static_cast<const float*>(q->layer[l - 1].act) : nullptr;
    a.x0 = static_cast<const float*>(q->x0), a.x1 = static_cast<const float*>(q->x1);
    a.x0_stride = q->x0_stride, a.x1_stride = q->x1_stride;
    a.k0 = q->k0, a.input_relu = (q->flags & HK_MLP_INPUT_RELU) ? 1 : 0, a.batch = q->batch;
    if (backward) {
      if (l + 1 < q->nlayers) {
        a.n_next = q->layer[l + 1].n;
        a.w_next = static_cast<const float*>(q->layer[l + 1].weight);
        a.dz_next = ws[(l + 1) & 1];
      } else {
        a.grad = static_cast<const float*>(q->grad_out), a.grad_stride = q->grad_stride;
      }
      a.dz_out = l > 0 ? ws[l & 1] : nullptr;
    }
    const int status = large ? launch_layer<kTrainRtLarge>(backward, a, stream) : launch_layer<kTrainRtSmall>(backward, a, stream);
    if (status != HK_OK) return status;
  }
  return HK_OK;
}

}  // namespace

extern "C" {

int hk_train_mlp_rows(int64_t batch) { return train_rows(train_rt(batch)); }

uint64_t hk_train_mlp_workspace_bytes(const hk_mlp_train_desc* q) { return workspace_bytes(q); }

int hk_train_mlp_forward(const hk_mlp_train_desc* q, void* stream) { return run(q, false, (hipStream_t)stream); }

int hk_train_mlp_backward(const hk_mlp_train_desc* q, void* stream) { return run(q, true, (hipStream_t)stream); }

}  // extern "C"
