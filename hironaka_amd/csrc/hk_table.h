// What the kernels over a table of tensors share (polyak_kernel in hk_dqn_kernel.h, the two of hk_optim_kernel.h): the host
// deals the workgroups to (tensor, chunk) pairs and the table travels as the kernel's argument; a workgroup finds its
// tensor by bisection over the tensors' first workgroups.  And the fused multiply-add by type, which their rules name
// explicitly under -ffp-contract=off.
#pragma once

#include "hk_common.h"

namespace hk {

// the last tensor whose first workgroup is <= block (tensors without elements have no workgroup)
__device__ __forceinline__ int table_find(const uint32_t* first, int ntensors, uint32_t block) {
  int lo = 0, hi = ntensors;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= block) lo = mid; else hi = mid;
  }
  return lo;
}

template <typename T>
__device__ __forceinline__ T hk_fma(T a, T b, T c);
template <>
__device__ __forceinline__ float hk_fma<float>(float a, float b, float c) {
  return fmaf(a, b, c);
}
template <>
__device__ __forceinline__ double hk_fma<double>(double a, double b, double c) {
  return fma(a, b, c);
}

}  // namespace hk
