// rtx_rays.hip - the ray-generation kernels of rt_render_rays (rtx_raygen_rays.h) and their launchers. Compiled beside the other translation units.
#include <hip/hip_runtime.h>
#include "../../include/rtx_hip.h"
#include "rtx_raygen_rays.h"
#include "rtx_rays_launch.h"

namespace rtx {

void rtx_launch_rays_scan(unsigned grid, hipStream_t stream, const float* rays, unsigned long long n_rays, unsigned* any_skipped) {
  hipLaunchKernelGGL(k_rays_scan, dim3(grid), dim3(256), 0, stream, rays, n_rays, any_skipped);
}
void rtx_launch_raygen_rays(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const float4* rays, unsigned ray_s0, unsigned ray_ns, unsigned ts_log2,
                            float4* rad) {
  hipLaunchKernelGGL(k_raygen_rays, dim3(grid), dim3(256), 0, stream, fp, ps, SPtr<const float4>(rays), ray_s0, ray_ns, ts_log2, rad);
}

}  // namespace rtx
