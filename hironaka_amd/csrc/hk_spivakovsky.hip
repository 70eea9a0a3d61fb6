// C ABI of hk_spivakovsky_select (include/hironaka_hip_spivakovsky.h): argument validation and launch of
// hk::spivakovsky_select_kernel.  No allocation, no synchronisation; every status is decided before the launch, in
// hk_host_select's order.
#include "hk_spivakovsky_kernel.h"

using namespace hk;

namespace {

template <typename T, int HOST>
int launch(SpivakovskyArgs a, hipStream_t stream) {
  const size_t es = sizeof(SpivakovskySlice<T, HOST>);
  a.games_per_block = kWave;
  while (a.games_per_block > 1 && (size_t)a.lds_stride * a.games_per_block * es > (size_t)kHostSelectLdsBytes)
    a.games_per_block >>= 1;
  const unsigned grid = (unsigned)(((int64_t)a.batch + a.games_per_block - 1) / a.games_per_block);
  return launch_kernel(spivakovsky_select_kernel<T, HOST>, dim3(grid), dim3(kWave),
                       (size_t)a.lds_stride * a.games_per_block * es, stream, a);
}

}  // namespace

extern "C" {

int hk_spivakovsky_select(const void* points, int64_t stride, int32_t* mask_out, int batch, int max_points, int dim,
                          int dtype, int host, uint64_t seed, uint64_t game_offset, uint32_t step, void* stream) {
  if (batch < 0 || max_points < 1 || dim < 2) return HK_ERR_SHAPE;
  if (dtype != HK_F32 && dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (host != HK_HOST_SPIVAKOVSKY && host != HK_HOST_RANDOM_SPIVAKOVSKY) return HK_ERR_UNSUPPORTED;
  if (max_points > kFixedHostMaxPoints || dim > kFixedHostMaxDim) return HK_ERR_UNSUPPORTED;
  if (batch == 0) return HK_OK;
  if (!points || !mask_out) return HK_ERR_NULL;
  if (stride < (int64_t)max_points * dim) return HK_ERR_SHAPE;
  if (!aligned(points, elem_size(dtype)) || !aligned(mask_out, 4)) return HK_ERR_ALIGN;
  SpivakovskyArgs a{};
  a.points = points;
  a.mask_out = mask_out;
  a.stride = stride;
  a.seed = seed;
  a.game_offset = game_offset;
  a.step = step;
  a.batch = batch;
  a.m = max_points;
  a.d = dim;
  a.lds_stride = (max_points * dim) | 1;  // odd: the lanes' games start in different banks
  const hipStream_t s = (hipStream_t)stream;
  if (host == HK_HOST_SPIVAKOVSKY)
    return dtype == HK_F32 ? launch<float, HK_HOST_SPIVAKOVSKY>(a, s) : launch<double, HK_HOST_SPIVAKOVSKY>(a, s);
  return dtype == HK_F32 ? launch<float, HK_HOST_RANDOM_SPIVAKOVSKY>(a, s)
                         : launch<double, HK_HOST_RANDOM_SPIVAKOVSKY>(a, s);
}

}  // extern "C"
