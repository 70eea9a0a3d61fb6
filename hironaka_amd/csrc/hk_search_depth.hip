// C ABI of hk_search_depth (include/hironaka_hip.h, ABI 5; the hosts of ABI 6): argument validation and launch of
// hk::search_depth_kernel.  No allocation, no synchronisation; every status is decided before the launch.
#include "hk_search_depth_kernel.h"

using namespace hk;

namespace {

constexpr int kSearchMaxPoints = 64;
constexpr int kSearchMaxDim = 6;

int search_spec(int batch, int m, int d, int dtype, int stack_nodes) {
  if (dtype != HK_F32 && dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (batch < 0 || m < 1 || d < 2 || stack_nodes < 1) return HK_ERR_SHAPE;
  if (m > kSearchMaxPoints || d > kSearchMaxDim) return HK_ERR_UNSUPPORTED;
  return HK_OK;
}

// bytes of the stacks of `batch` roots, 0 when that overflows 64 bits
uint64_t stack_bytes(int batch, int m, int d, int dtype, int stack_nodes) {
  const uint64_t per_root = (uint64_t)stack_nodes * ((uint64_t)m * d * (dtype == HK_F64 ? 8 : 4) + 4);
  if (batch > 0 && per_root > UINT64_MAX / (uint64_t)batch) return 0;
  return per_root * (uint64_t)batch;
}

template <typename T, int HOST>
int launch_search_depth(SearchDepthArgs a, int batch, hipStream_t stream) {
  const int per_lane = a.lds_stride * (int)sizeof(T);
  a.lanes = kSearchDepthLdsBytes / per_lane < kWave ? kSearchDepthLdsBytes / per_lane : kWave;
  const size_t lds = (size_t)a.lanes * per_lane;
  launch_prepare();
  hipLaunchKernelGGL((search_depth_kernel<T, HOST>), dim3((unsigned)batch), dim3(kWave), lds, stream, a);
  return launch_status();
}

template <typename T>
int launch_search_depth(const SearchDepthArgs& a, int batch, hipStream_t stream) {
  switch (a.host) {
    case HK_HOST_ALL_COORD: return launch_search_depth<T, HK_HOST_ALL_COORD>(a, batch, stream);
    case HK_HOST_ZEILLINGER: return launch_search_depth<T, HK_HOST_ZEILLINGER>(a, batch, stream);
    case HK_HOST_ZEILLINGER_LEX: return launch_search_depth<T, HK_HOST_ZEILLINGER_LEX>(a, batch, stream);
    case HK_HOST_WEAK_SPIVAKOVSKY: return launch_search_depth<T, HK_HOST_WEAK_SPIVAKOVSKY>(a, batch, stream);
    case HK_HOST_MIN_HITTING: return launch_search_depth<T, HK_HOST_MIN_HITTING>(a, batch, stream);
  }
  return HK_ERR_UNSUPPORTED;
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
  if (host < HK_HOST_ALL_COORD || host > HK_HOST_MIN_HITTING) return HK_ERR_UNSUPPORTED;
  if (max_depth < 0 || max_nodes < 1) return HK_ERR_SHAPE;
  if (batch == 0) return HK_OK;
  if (!points || !workspace || !depth_out || !nodes_out || !status_out) return HK_ERR_NULL;
  const uint64_t need = stack_bytes(batch, max_points, dim, dtype, stack_nodes);
  if (need == 0 || workspace_bytes < need) return HK_ERR_SHAPE;
  const size_t es = dtype == HK_F64 ? 8 : 4;
  if ((reinterpret_cast<uintptr_t>(points) % es) || (reinterpret_cast<uintptr_t>(workspace) % es) ||
      (reinterpret_cast<uintptr_t>(depth_out) % 4) || (reinterpret_cast<uintptr_t>(nodes_out) % 8) ||
      (reinterpret_cast<uintptr_t>(status_out) % 4))
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
  a.lds_stride = search_depth_lds_stride(max_points, dim);
  return dtype == HK_F32 ? launch_search_depth<float>(a, batch, (hipStream_t)stream)
                         : launch_search_depth<double>(a, batch, (hipStream_t)stream);
}

}  // extern "C"
