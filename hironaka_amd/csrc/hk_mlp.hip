// C ABI of hk_mlp_forward (include/hironaka_hip_mlp.h, an addition within ABI 6): argument validation and launch of
// hk::mlp_kernel.  No allocation, no synchronisation; every status is decided before the launch.
#include "hk_mlp_kernel.h"

using namespace hk;

namespace {

constexpr uint32_t kDescFlags = HK_MLP_INPUT_RELU | HK_MLP_FORCE_TILE_SMALL | HK_MLP_FORCE_TILE_LARGE;

// out's rows (`out_bytes` from first to last, n wide) share a byte with the rows of an input (`x_bytes`, k wide).  Rows of
// one stride that holds both widths are records side by side: they meet only where the windows meet inside a record (any
// two records apart: the batch is not looked at); everything else is judged by the spans from the first to the last element.
bool rows_overlap(const hk_mlp_desc* q, uint64_t out_bytes, int64_t n, const void* x, uint64_t x_bytes, int64_t stride,
                  int64_t k) {
  if (!overlap(q->out, out_bytes, x, x_bytes)) return false;
  if (q->batch == 1 || stride != q->out_stride || stride < k) return true;
  const int64_t diff = (int64_t)((reinterpret_cast<intptr_t>(q->out) - reinterpret_cast<intptr_t>(x)) / 4);
  const int64_t r = ((diff % stride) + stride) % stride;  // out's window starts r elements into x's record
  return r < k || r + n > stride;
}

bool has_bn(const hk_mlp_layer& L) { return L.bn_mean || L.bn_var || L.bn_weight || L.bn_bias; }
bool has_in_bn(const hk_mlp_desc* q) { return q->in_bn_mean || q->in_bn_var || q->in_bn_weight || q->in_bn_bias; }

int validate(const hk_mlp_desc* q) {
  if (const int bad = mlp_check_desc(q, kDescFlags)) return bad;
  if (mlp_forces_both_tiles(q->flags)) return HK_ERR_UNSUPPORTED;
  int64_t width = 0;
  if (const int bad = mlp_check_sizes(q, HK_MLP_RELU, width)) return bad;
  if (q->out_stride < width) return HK_ERR_SHAPE;
  if (mlp_input_missing(q) || !q->out) return HK_ERR_NULL;
  if (has_in_bn(q) && (!q->in_bn_mean || !q->in_bn_var)) return HK_ERR_NULL;
  for (int l = 0; l < q->nlayers; ++l) {
    const hk_mlp_layer& L = q->layer[l];
    if (!L.weight || (has_bn(L) && (!L.bn_mean || !L.bn_var))) return HK_ERR_NULL;
  }
  if (!all_aligned({q->x0, q->x1, q->out, q->in_bn_mean, q->in_bn_var, q->in_bn_weight, q->in_bn_bias}, 4))
    return HK_ERR_ALIGN;
  for (int l = 0; l < q->nlayers; ++l) {
    const hk_mlp_layer& L = q->layer[l];
    if (!all_aligned({L.weight, L.bias, L.bn_mean, L.bn_var, L.bn_weight, L.bn_bias}, 4)) return HK_ERR_ALIGN;
  }
  const uint64_t out_bytes = span_bytes(q->batch, q->out_stride, width, sizeof(float));
  uint64_t x0_bytes, x1_bytes;
  if (!mlp_input_spans(q, x0_bytes, x1_bytes) || (q->batch > 0 && !out_bytes)) return HK_ERR_SHAPE;  // beyond 2^63 bytes
  if (rows_overlap(q, out_bytes, width, q->x0, x0_bytes, q->x0_stride, q->k0)) return HK_ERR_UNSUPPORTED;
  if (q->k1 > 0 && rows_overlap(q, out_bytes, width, q->x1, x1_bytes, q->x1_stride, q->k1)) return HK_ERR_UNSUPPORTED;
  for (const void* p : {q->in_bn_mean, q->in_bn_var, q->in_bn_weight, q->in_bn_bias})
    if (overlap(q->out, out_bytes, p, (uint64_t)(q->k0 + q->k1) * sizeof(float))) return HK_ERR_UNSUPPORTED;
  for (int l = 0; l < q->nlayers; ++l) {
    const hk_mlp_layer& L = q->layer[l];
    const uint64_t vec = (uint64_t)L.n * sizeof(float);
    if (overlap(q->out, out_bytes, L.weight, vec * (uint64_t)L.k)) return HK_ERR_UNSUPPORTED;
    for (const void* p : {L.bias, L.bn_mean, L.bn_var, L.bn_weight, L.bn_bias})
      if (overlap(q->out, out_bytes, p, vec)) return HK_ERR_UNSUPPORTED;
  }
  return HK_OK;
}

}  // namespace

extern "C" {

int hk_mlp_row_tile(int64_t batch) { return mlp_row_tile(batch); }

int hk_mlp_forward(const hk_mlp_desc* q, void* stream) {
  const int bad = validate(q);
  if (bad != HK_OK) return bad;
  if (q->batch == 0) return HK_OK;
  return mlp_launch(mlp_kernel<HK_MLP_TILE_SMALL>, mlp_kernel<HK_MLP_TILE_LARGE>, *q, (hipStream_t)stream);
}

}  // extern "C"
