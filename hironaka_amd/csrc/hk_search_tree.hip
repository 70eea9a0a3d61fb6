// C ABI of hk_search_game_tree (include/hironaka_hip.h, an addition within ABI 6): argument validation and launch of
// hk::search_tree_kernel.  No allocation, no synchronisation; every status is decided before the launch.
#include "hk_search_tree_kernel.h"

using namespace hk;

namespace {

constexpr int kTreeMaxPoints = 64;
constexpr int kTreeMaxDim = 6;

int tree_spec(int batch, int m, int d, int dtype, int max_nodes, int stack_nodes) {
  if (dtype != HK_F32 && dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (batch < 0 || m < 1 || d < 2 || max_nodes < 1 || stack_nodes < 1) return HK_ERR_SHAPE;
  if (m > kTreeMaxPoints || d > kTreeMaxDim) return HK_ERR_UNSUPPORTED;
  return HK_OK;
}

// bytes of the record states of `batch` roots, then their int32 words; 0 when that overflows 64 bits
uint64_t tree_state_bytes(int batch, int m, int d, int dtype, int max_nodes) {
  const uint64_t per_root = (uint64_t)max_nodes * (uint64_t)m * d * (dtype == HK_F64 ? 8 : 4);
  return batch > 0 && per_root > UINT64_MAX / (uint64_t)batch ? 0 : per_root * (uint64_t)batch;
}

uint64_t tree_workspace_bytes(int batch, int m, int d, int dtype, int max_nodes, int stack_nodes) {
  const uint64_t states = tree_state_bytes(batch, m, d, dtype, max_nodes);
  const uint64_t per_root = 4 * search_tree_int_words(max_nodes, stack_nodes);
  if (states == 0 || per_root > (UINT64_MAX - states) / (uint64_t)batch) return 0;
  return states + per_root * (uint64_t)batch;
}

template <typename T, int HOST>
int launch_search_tree(SearchTreeArgs a, int batch, hipStream_t stream) {
  const int per_lane = a.lds_stride * (int)sizeof(T);
  a.lanes = kSearchTreeLdsBytes / per_lane < kWave ? kSearchTreeLdsBytes / per_lane : kWave;
  const size_t lds = (size_t)a.lanes * per_lane;
  launch_prepare();
  hipLaunchKernelGGL((search_tree_kernel<T, HOST>), dim3((unsigned)batch), dim3(kWave), lds, stream, a);
  return launch_status();
}

template <typename T>
int launch_search_tree(const SearchTreeArgs& a, int host, int batch, hipStream_t stream) {
  switch (host) {
    case HK_HOST_ALL_COORD: return launch_search_tree<T, HK_HOST_ALL_COORD>(a, batch, stream);
    case HK_HOST_ZEILLINGER: return launch_search_tree<T, HK_HOST_ZEILLINGER>(a, batch, stream);
    case HK_HOST_ZEILLINGER_LEX: return launch_search_tree<T, HK_HOST_ZEILLINGER_LEX>(a, batch, stream);
    case HK_HOST_WEAK_SPIVAKOVSKY: return launch_search_tree<T, HK_HOST_WEAK_SPIVAKOVSKY>(a, batch, stream);
    case HK_HOST_MIN_HITTING: return launch_search_tree<T, HK_HOST_MIN_HITTING>(a, batch, stream);
  }
  return HK_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" {

uint64_t hk_search_game_tree_workspace_bytes(int batch, int max_points, int dim, int dtype, int max_nodes,
                                             int stack_nodes) {
  if (tree_spec(batch, max_points, dim, dtype, max_nodes, stack_nodes) != HK_OK) return 0;
  return tree_workspace_bytes(batch, max_points, dim, dtype, max_nodes, stack_nodes);
}

int hk_search_game_tree(const void* points, int batch, int max_points, int dim, int dtype, int host,
                        int64_t expand_limit, int max_depth, int max_nodes, int stack_nodes, void* workspace,
                        uint64_t workspace_bytes, int32_t* parent_out, int32_t* child_index_out, int32_t* axis_out,
                        int32_t* depth_out, int32_t* num_points_out, int32_t* host_class_out, void* states_out,
                        int32_t* count_out, int32_t* status_out, void* stream) {
  const int st = tree_spec(batch, max_points, dim, dtype, max_nodes, stack_nodes);
  if (st != HK_OK) return st;
  if (host < HK_HOST_ALL_COORD || host > HK_HOST_MIN_HITTING) return HK_ERR_UNSUPPORTED;
  if (max_depth < 0) return HK_ERR_SHAPE;
  if (batch == 0) return HK_OK;
  if (!points || !workspace || !parent_out || !child_index_out || !axis_out || !depth_out || !num_points_out ||
      !host_class_out || !count_out || !status_out)
    return HK_ERR_NULL;
  const uint64_t need = tree_workspace_bytes(batch, max_points, dim, dtype, max_nodes, stack_nodes);
  if (need == 0 || workspace_bytes < need) return HK_ERR_SHAPE;
  const size_t es = dtype == HK_F64 ? 8 : 4;
  const int32_t* ints[] = {parent_out, child_index_out, axis_out, depth_out, num_points_out, host_class_out,
                           count_out, status_out};
  for (const int32_t* p : ints)
    if (reinterpret_cast<uintptr_t>(p) % 4) return HK_ERR_ALIGN;
  if ((reinterpret_cast<uintptr_t>(points) % es) || (reinterpret_cast<uintptr_t>(workspace) % es) ||
      (reinterpret_cast<uintptr_t>(states_out) % es))
    return HK_ERR_ALIGN;
  SearchTreeArgs a{};
  a.points = points;
  a.rec_states = workspace;
  a.rec_ints = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(workspace) +
                                          tree_state_bytes(batch, max_points, dim, dtype, max_nodes));
  a.parent_out = parent_out;
  a.child_index_out = child_index_out;
  a.axis_out = axis_out;
  a.depth_out = depth_out;
  a.num_points_out = num_points_out;
  a.host_class_out = host_class_out;
  a.states_out = states_out;
  a.count_out = count_out;
  a.status_out = status_out;
  a.expand_limit = expand_limit;
  a.rec_int_stride = search_tree_int_words(max_nodes, stack_nodes);
  a.m = max_points;
  a.d = dim;
  a.max_depth = max_depth;
  a.max_nodes = max_nodes;
  a.stack_nodes = stack_nodes;
  a.lds_stride = search_tree_lds_stride(max_points, dim);
  return dtype == HK_F32 ? launch_search_tree<float>(a, host, batch, (hipStream_t)stream)
                         : launch_search_tree<double>(a, host, batch, (hipStream_t)stream);
}

}  // extern "C"
