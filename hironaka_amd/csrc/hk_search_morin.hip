// C ABI of hk_search_morin_tree (include/hironaka_hip.h, an addition within ABI 6): argument validation and launch of
// hk::search_morin_kernel.  No allocation, no synchronisation; every status is decided before the launch.
#include "hk_search_morin_kernel.h"

using namespace hk;

namespace {

// dim 2..7 here, where the other fixed-host operators stop at kFixedHostMaxDim
int morin_spec(int batch, int m, int d, int dtype, int max_nodes, int stack_nodes) {
  if (dtype != HK_F32 && dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (batch < 0 || m < 1 || d < 2 || max_nodes < 1 || stack_nodes < 1) return HK_ERR_SHAPE;
  if (m > kFixedHostMaxPoints || d > kLaneGameMaxDim) return HK_ERR_UNSUPPORTED;
  return HK_OK;
}

// bytes of the record states of `batch` roots, then their int32 words; 0 when that overflows 64 bits
uint64_t morin_state_bytes(int batch, int m, int d, int dtype, int max_nodes) {
  return checked_mul((uint64_t)max_nodes * (uint64_t)m * d * elem_size(dtype), (uint64_t)batch);
}

uint64_t morin_workspace_bytes(int batch, int m, int d, int dtype, int max_nodes, int stack_nodes) {
  const uint64_t states = morin_state_bytes(batch, m, d, dtype, max_nodes);
  const uint64_t ints = checked_mul(4 * search_morin_int_words(max_nodes, stack_nodes, d), (uint64_t)batch);
  if (states == 0 || ints == 0 || ints > UINT64_MAX - states) return 0;
  return states + ints;
}

}  // namespace

extern "C" {

uint64_t hk_search_morin_tree_workspace_bytes(int batch, int max_points, int dim, int dtype, int max_nodes,
                                              int stack_nodes) {
  if (morin_spec(batch, max_points, dim, dtype, max_nodes, stack_nodes) != HK_OK) return 0;
  return morin_workspace_bytes(batch, max_points, dim, dtype, max_nodes, stack_nodes);
}

int hk_search_morin_tree(const void* points, const int32_t* weights, const int32_t* distinguished, int batch,
                         int max_points, int dim, int dtype, int host, int64_t expand_limit, int max_depth,
                         int max_nodes, int stack_nodes, void* workspace, uint64_t workspace_bytes, int32_t* parent_out,
                         int32_t* child_index_out, int32_t* axis_out, int32_t* depth_out, int32_t* num_points_out,
                         int32_t* host_class_out, int32_t* kind_out, int32_t* distinguished_out, int32_t* weights_out,
                         void* states_out, int32_t* count_out, int32_t* status_out, void* stream) {
  const int st = morin_spec(batch, max_points, dim, dtype, max_nodes, stack_nodes);
  if (st != HK_OK) return st;
  if (!fixed_host(host)) return HK_ERR_UNSUPPORTED;
  if (max_depth < 0) return HK_ERR_SHAPE;
  if (batch == 0) return HK_OK;
  if (!points || !weights || !distinguished || !workspace || !parent_out || !child_index_out || !axis_out ||
      !depth_out || !num_points_out || !host_class_out || !kind_out || !distinguished_out || !weights_out ||
      !count_out || !status_out)
    return HK_ERR_NULL;
  const uint64_t need = morin_workspace_bytes(batch, max_points, dim, dtype, max_nodes, stack_nodes);
  if (need == 0 || workspace_bytes < need) return HK_ERR_SHAPE;
  const size_t es = elem_size(dtype);
  const int32_t* ints[] = {weights,        distinguished,  parent_out, child_index_out,   axis_out,    depth_out,
                           num_points_out, host_class_out, kind_out,   distinguished_out, weights_out, count_out,
                           status_out};
  for (const int32_t* p : ints)
    if (!aligned(p, 4)) return HK_ERR_ALIGN;
  if (!aligned(points, es) || !aligned(workspace, es) || !aligned(states_out, es)) return HK_ERR_ALIGN;
  SearchMorinArgs a{};
  a.points = points;
  a.weights = weights;
  a.distinguished = distinguished;
  a.rec_states = workspace;
  a.rec_ints = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(workspace) +
                                          morin_state_bytes(batch, max_points, dim, dtype, max_nodes));
  a.parent_out = parent_out;
  a.child_index_out = child_index_out;
  a.axis_out = axis_out;
  a.depth_out = depth_out;
  a.num_points_out = num_points_out;
  a.host_class_out = host_class_out;
  a.kind_out = kind_out;
  a.distinguished_out = distinguished_out;
  a.weights_out = weights_out;
  a.states_out = states_out;
  a.count_out = count_out;
  a.status_out = status_out;
  a.expand_limit = expand_limit;
  a.rec_int_stride = search_morin_int_words(max_nodes, stack_nodes, dim);
  a.m = max_points;
  a.d = dim;
  a.max_depth = max_depth;
  a.max_nodes = max_nodes;
  a.stack_nodes = stack_nodes;
  return with_fixed_host(dtype, host, [&](auto t, auto h) {
    return launch_search<decltype(t)>(search_morin_kernel<decltype(t), h>, a, batch, (hipStream_t)stream,
                                      morin_lds_extra(dim));
  });
}

}  // extern "C"
