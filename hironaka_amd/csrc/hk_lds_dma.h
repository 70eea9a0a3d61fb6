// LDS-DMA requests and their completion, shared by the kernels that load a slab straight into its LDS image
// (hk_quad_kernel.h: quad_slab_load; hk_duo_kernel.h: duo_slab_dma).
#pragma once

namespace hk {

// the instruction's immediate offset is 12 bits unsigned here (it moves the LDS address too); what exceeds it goes
// into both base pointers
constexpr int kDmaImm = 4096;
template <int BYTES, int OFFSET>
__device__ __forceinline__ void lds_dma(const float* src, float* dst) {
  static_assert(BYTES == 16 || BYTES == 4, "request size");
  if constexpr (BYTES == 16) __builtin_amdgcn_global_load_lds(src, dst, 16, OFFSET, 0);
  else __builtin_amdgcn_global_load_lds(src, dst, 4, OFFSET, 0);
}

// completion of every LDS-DMA request (and load) of the wave
__device__ __forceinline__ void wait_vmem_all() { __builtin_amdgcn_s_waitcnt(0x0F70); }  // vmcnt(0)

}  // namespace hk
