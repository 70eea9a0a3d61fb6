// C ABI of hk_host_select (include/hironaka_hip.h, ABI 6): argument validation and launch of hk::host_select_kernel.
// No allocation, no synchronisation; every status is decided before the launch.
#include "hk_host_select_kernel.h"

using namespace hk;

extern "C" {

int hk_host_select(const void* points, int64_t stride, int32_t* class_out, int batch, int max_points, int dim,
                   int dtype, int host, void* stream) {
  if (batch < 0 || max_points < 1 || dim < 2) return HK_ERR_SHAPE;
  if (dtype != HK_F32 && dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (!fixed_host(host)) return HK_ERR_UNSUPPORTED;
  if (max_points > kFixedHostMaxPoints || dim > kFixedHostMaxDim) return HK_ERR_UNSUPPORTED;
  if (batch == 0) return HK_OK;
  if (!points || !class_out) return HK_ERR_NULL;
  if (stride < (int64_t)max_points * dim) return HK_ERR_SHAPE;
  const size_t es = elem_size(dtype);
  if (!aligned(points, es) || !aligned(class_out, 4)) return HK_ERR_ALIGN;
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
  const unsigned grid = (unsigned)(((int64_t)a.batch + a.games_per_block - 1) / a.games_per_block);
  return with_fixed_host(dtype, host, [&](auto t, auto h) {
    using T = decltype(t);
    const size_t lds = h == HK_HOST_ALL_COORD ? 0 : (size_t)a.lds_stride * a.games_per_block * sizeof(T);
    return launch_kernel(host_select_kernel<T, h>, dim3(grid), dim3(kWave), lds, (hipStream_t)stream, a);
  });
}

}  // extern "C"
