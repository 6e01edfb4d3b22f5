// rtx_shade_rays.hip - the k_shade_rays instantiations (rtx_shade_kernels.h): bounce 0's shade kernels of a call or ray-frame step whose rays carry differentials
// (RT_FLAG_RAY_DIFFERENTIALS). A translation unit of its own, compiled beside the others, so that the code object of rtx_shade.hip - every k_shade form - is what it was.
#include <hip/hip_runtime.h>
#include "../../include/rtx_hip.h"
#include "rtx_shade_kernels.h"
#include "rtx_shade_launch.h"

namespace rtx {
void rtx_launch_shade_rays(int mode, bool general, unsigned grid, unsigned block, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, const RayDiffSrc& rd) {
#define RT_SR(M) do { if (general) hipLaunchKernelGGL((k_shade_rays<M, true>), dim3(grid), dim3(block), 0, stream, d, fp, p, rd); \
                      else hipLaunchKernelGGL((k_shade_rays<M, false>), dim3(grid), dim3(block), 0, stream, d, fp, p, rd); } while (0)
  switch (mode) {
    case 3: RT_SR(3); break;
    case 5: RT_SR(5); break;
    case 6: RT_SR(6); break;
    default: RT_SR(0); break;
  }
#undef RT_SR
}
void rtx_shade_rays_set_ewa_lut(const float* lut128) { (void)hipMemcpyToSymbol(HIP_SYMBOL(kEwaLut), lut128, 128 * sizeof(float)); }
}  // namespace rtx
