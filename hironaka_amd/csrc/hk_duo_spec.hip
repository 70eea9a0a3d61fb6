// The two-lanes-per-game kernels hk::duo_kernel<HK_SPEC_M, HK_SPEC_D, *> of one shape per object file
// (Makefile: the same table as hk_fast_spec.hip), built beside the one-lane specialisations.
#define HK_SPEC_TU 1
#include "hk_duo_kernel.h"

namespace hk {
static_assert(HK_SPEC_M * HK_SPEC_D > 0, "build with -DHK_SPEC_M=<max_points> -DHK_SPEC_D=<dim>");
template int launch_duo_t<HK_SPEC_M, HK_SPEC_D>(Params, hipStream_t);
}  // namespace hk

#ifdef HK_DUO_PROBE
// dev builds: the probe's rows of this unit's kernels, copied to the host (scripts/probe_timeline.py)
extern "C" int hk_duo_probe_read(int32_t* dst, int waves) {
  if (waves < 0 || waves > hk::kDuoProbeWaves) return -1;
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(hk::duo_probe_rows), (size_t)waves * hk::kDuoProbeRow * sizeof(int32_t), 0,
                                  hipMemcpyDeviceToHost);
}
#endif
