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

// The chunks of a table entry of `numel` > 0 elements of `esz` bytes whose launch touches the `n` pointers `ptr`.  Where the
// pointers agree mod 16: `head` elements in front of the first 16-byte boundary, then chunks of `vecs_per_chunk` (lanes x
// transfers) 16-byte vectors, the tail with the last of them.  Where they disagree: head -1, element by element in chunks of
// `chunk_bytes`.
struct ChunkPlan {
  int32_t head;
  uint64_t chunks;
};
template <uint64_t vecs_per_chunk, uint64_t chunk_bytes>
ChunkPlan chunk_plan(const void* const* ptr, int n, int64_t numel, size_t esz) {
  static_assert(chunk_bytes == vecs_per_chunk * 16, "either way a chunk covers the same bytes: the families' constants agree");
  const uintptr_t mod = reinterpret_cast<uintptr_t>(ptr[0]) & 15u;
  bool together = true;
  for (int k = 1; k < n; ++k) together = together && (reinterpret_cast<uintptr_t>(ptr[k]) & 15u) == mod;
  if (!together) {
    const uint64_t per = chunk_bytes / esz;
    return ChunkPlan{-1, ((uint64_t)numel + per - 1) / per};
  }
  const int64_t to_boundary = (int64_t)(((16u - mod) & 15u) / esz);
  const int32_t head = (int32_t)(to_boundary < numel ? to_boundary : numel);
  const uint64_t nvec = (uint64_t)(numel - head) / (16 / esz);
  return ChunkPlan{head, nvec ? (nvec + vecs_per_chunk - 1) / vecs_per_chunk : 1};
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
