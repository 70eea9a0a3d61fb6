// C ABI of hk_host_select (include/hironaka_hip.h, ABI 6): argument validation and launch of hk::host_select_kernel.
// No allocation, no synchronisation; every status is decided before the launch.
#include "hk_host_select_kernel.h"

using namespace hk;

namespace {

constexpr int kHostMaxPoints = 64;
constexpr int kHostMaxDim = 6;  // the hitting-set hosts keep one bit per possible support: 2^6

template <typename T, int HOST>
int launch_host(HostSelectArgs a, hipStream_t stream) {
  const unsigned grid = (unsigned)(((int64_t)a.batch + a.games_per_block - 1) / a.games_per_block);
  const size_t lds = HOST == HK_HOST_ALL_COORD ? 0 : (size_t)a.lds_stride * a.games_per_block * sizeof(T);
  launch_prepare();
  hipLaunchKernelGGL((host_select_kernel<T, HOST>), dim3(grid), dim3(kWave), lds, stream, a);
  return launch_status();
}

template <typename T>
int launch_host(const HostSelectArgs& a, int host, hipStream_t stream) {
  switch (host) {
    case HK_HOST_ALL_COORD: return launch_host<T, HK_HOST_ALL_COORD>(a, stream);
    case HK_HOST_ZEILLINGER: return launch_host<T, HK_HOST_ZEILLINGER>(a, stream);
    case HK_HOST_ZEILLINGER_LEX: return launch_host<T, HK_HOST_ZEILLINGER_LEX>(a, stream);
    case HK_HOST_WEAK_SPIVAKOVSKY: return launch_host<T, HK_HOST_WEAK_SPIVAKOVSKY>(a, stream);
    case HK_HOST_MIN_HITTING: return launch_host<T, HK_HOST_MIN_HITTING>(a, stream);
  }
  return HK_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" {

int hk_host_select(const void* points, int64_t stride, int32_t* class_out, int batch, int max_points, int dim,
                   int dtype, int host, void* stream) {
  if (batch < 0 || max_points < 1 || dim < 2) return HK_ERR_SHAPE;
  if (dtype != HK_F32 && dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (host < HK_HOST_ALL_COORD || host > HK_HOST_MIN_HITTING) return HK_ERR_UNSUPPORTED;
  if (max_points > kHostMaxPoints || dim > kHostMaxDim) return HK_ERR_UNSUPPORTED;
  if (batch == 0) return HK_OK;
  if (!points || !class_out) return HK_ERR_NULL;
  if (stride < (int64_t)max_points * dim) return HK_ERR_SHAPE;
  const size_t es = dtype == HK_F64 ? 8 : 4;
  if ((reinterpret_cast<uintptr_t>(points) % es) || (reinterpret_cast<uintptr_t>(class_out) % 4)) return HK_ERR_ALIGN;
  HostSelectArgs a{};
  a.points = points;
  a.class_out = class_out;
  a.stride = stride;
  a.batch = batch;
  a.m = max_points;
  a.d = dim;
  a.lds_stride = (max_points * dim) | 1;  // odd: the lanes' games start in different banks
  a.games_per_block = kWave;
  while (a.games_per_block > 1 && (size_t)a.lds_stride * a.games_per_block * es > (size_t)kHostSelectLdsBytes)
    a.games_per_block >>= 1;
  return dtype == HK_F32 ? launch_host<float>(a, host, (hipStream_t)stream)
                         : launch_host<double>(a, host, (hipStream_t)stream);
}

}  // extern "C"
