// C ABI of hk_tree_expand (include/hironaka_hip_tree.h, an addition within ABI 6): argument validation and launch of
// hk::tree_expand_kernel.  No allocation, no synchronisation; every status is decided before the launch.
#include "hk_tree_expand_kernel.h"

using namespace hk;

extern "C" {

int hk_tree_expand(const hk_tree_expand_desc* q, void* stream) {
  if (!q) return HK_ERR_NULL;
  if (q->dtype != HK_F32 && q->dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (q->n_parents < 0 || q->capacity < 0 || q->max_points < 1 || q->dim < 2) return HK_ERR_SHAPE;
  if (q->dim > kLaneGameMaxDim) return HK_ERR_UNSUPPORTED;
  if (q->sem != HK_SEM_JAX && q->sem != HK_SEM_LIST) return HK_ERR_UNSUPPORTED;
  if (q->flags & ~(HK_TREE_REPOSITION | HK_TREE_ZERO_TAIL)) return HK_ERR_UNSUPPORTED;
  const size_t es = elem_size(q->dtype);
  // a parent and its child share a slice; at least one slice has to fit
  const int64_t slice = (2 * (int64_t)q->max_points * q->dim + 2 * q->dim) | 1;
  if (slice * (int64_t)es > kSearchLdsBytes) return HK_ERR_UNSUPPORTED;
  if (q->n_parents == 0) return HK_OK;
  if (!q->parents_in || !q->class_id || !q->child_offset || !q->status) return HK_ERR_NULL;
  if (q->capacity > 0 && (!q->children_out || !q->child_parent || !q->child_axis || !q->child_num_points ||
                          !q->child_done))
    return HK_ERR_NULL;
  const int64_t n = (int64_t)q->max_points * q->dim;
  const int64_t len = n + ((q->flags & HK_TREE_ZERO_TAIL) ? q->dim : 0);
  if (q->in_stride < n || q->out_stride < len) return HK_ERR_SHAPE;
  // a workgroup writes children while others still stage parents: the two buffers do not overlap
  const uint64_t in_bytes = span_bytes(q->n_parents, q->in_stride, n, es);
  const uint64_t out_bytes = span_bytes(q->capacity, q->out_stride, len, es);
  if (!in_bytes || (q->capacity > 0 && !out_bytes)) return HK_ERR_SHAPE;  // a span beyond 2^63 bytes
  if (overlap(q->parents_in, in_bytes, q->children_out, out_bytes)) return HK_ERR_SHAPE;
  if (!all_aligned({q->class_id, q->child_parent, q->child_axis, q->child_num_points, q->status}, 4) ||
      !aligned(q->child_offset, 8) || !all_aligned({q->parents_in, q->children_out}, es))
    return HK_ERR_ALIGN;
  TreeExpandArgs a{};
  a.parents = q->parents_in;
  a.children = q->children_out;
  a.class_id = q->class_id;
  a.child_offset = q->child_offset;
  a.child_parent = q->child_parent;
  a.child_axis = q->child_axis;
  a.child_num_points = q->child_num_points;
  a.child_done = q->child_done;
  a.status = q->status;
  a.in_stride = q->in_stride;
  a.out_stride = q->out_stride;
  a.n_parents = q->n_parents;
  a.capacity = q->capacity;
  a.m = q->max_points;
  a.d = q->dim;
  a.list = q->sem == HK_SEM_LIST ? 1 : 0;
  a.reposition = (q->flags & HK_TREE_REPOSITION) ? 1 : 0;
  a.zero_tail = (q->flags & HK_TREE_ZERO_TAIL) ? 1 : 0;
  a.lds_stride = search_lds_stride(a.m, a.d);
  const LaneGeometry geo = lane_geometry(a.lds_stride, es, a.n_parents);
  a.parents_per_block = geo.per_block;
  const auto kernel = q->dtype == HK_F32 ? tree_expand_kernel<float> : tree_expand_kernel<double>;
  return launch_kernel(kernel, dim3(geo.grid), dim3(kWave), geo.lds, (hipStream_t)stream, a);
}

}  // extern "C"
