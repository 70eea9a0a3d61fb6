// C ABI of hk_search_depth (include/hironaka_hip.h, ABI 5; the hosts of ABI 6): argument validation and launch of
// hk::search_depth_kernel.  No allocation, no synchronisation; every status is decided before the launch.
#include "hk_search_depth_kernel.h"

using namespace hk;

namespace {

int search_spec(int batch, int m, int d, int dtype, int stack_nodes) {
  if (dtype != HK_F32 && dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (batch < 0 || m < 1 || d < 2 || stack_nodes < 1) return HK_ERR_SHAPE;
  if (m > kFixedHostMaxPoints || d > kFixedHostMaxDim) return HK_ERR_UNSUPPORTED;
  return HK_OK;
}

// bytes of the stacks of `batch` roots, 0 when that overflows 64 bits
uint64_t stack_bytes(int batch, int m, int d, int dtype, int stack_nodes) {
  return checked_mul((uint64_t)stack_nodes * ((uint64_t)m * d * elem_size(dtype) + 4), (uint64_t)batch);
}

}  // namespace

extern "C" {

uint64_t hk_search_depth_workspace_bytes(int batch, int max_points, int dim, int dtype, int stack_nodes) {
  if (search_spec(batch, max_points, dim, dtype, stack_nodes) != HK_OK) return 0;
  return stack_bytes(batch, max_points, dim, dtype, stack_nodes);
}

int hk_search_depth(const void* points, int batch, int max_points, int dim, int dtype, int host, int max_depth,
                    uint64_t max_nodes, int stack_nodes, void* workspace, uint64_t workspace_bytes, int32_t* depth_out,
                    uint64_t* nodes_out, int32_t* status_out, void* stream) {
  const int st = search_spec(batch, max_points, dim, dtype, stack_nodes);
  if (st != HK_OK) return st;
  if (!fixed_host(host)) return HK_ERR_UNSUPPORTED;
  if (max_depth < 0 || max_nodes < 1) return HK_ERR_SHAPE;
  if (batch == 0) return HK_OK;
  if (!points || !workspace || !depth_out || !nodes_out || !status_out) return HK_ERR_NULL;
  const uint64_t need = stack_bytes(batch, max_points, dim, dtype, stack_nodes);
  if (need == 0 || workspace_bytes < need) return HK_ERR_SHAPE;
  const size_t es = elem_size(dtype);
  if (!aligned(points, es) || !aligned(workspace, es) || !aligned(depth_out, 4) || !aligned(nodes_out, 8) ||
      !aligned(status_out, 4))
    return HK_ERR_ALIGN;
  SearchDepthArgs a{};
  a.points = points;
  a.stack = workspace;
  a.stack_depth = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(workspace) +
                                             (uint64_t)batch * stack_nodes * max_points * dim * es);
  a.depth_out = depth_out;
  a.nodes_out = reinterpret_cast<unsigned long long*>(nodes_out);
  a.status_out = status_out;
  a.max_nodes = max_nodes;
  a.m = max_points;
  a.d = dim;
  a.host = host;
  a.max_depth = max_depth;
  a.stack_nodes = stack_nodes;
  return with_fixed_host(dtype, host, [&](auto t, auto h) {
    return launch_search<decltype(t)>(search_depth_kernel<decltype(t), h>, a, batch, (hipStream_t)stream);
  });
}

}  // extern "C"
