// rtx_rays.hip - the ray-generation kernels of rt_render_rays and of ray frames, and rt_camera_rays' kernel (rtx_raygen_rays.h), and their launchers. Compiled beside the other translation units.
#include <hip/hip_runtime.h>
#include "../../include/rtx_hip.h"
#include "rtx_raygen_rays.h"
#include "rtx_rays_launch.h"

namespace rtx {

void rtx_launch_rays_scan(unsigned grid, hipStream_t stream, const float* rays, unsigned long long n_rays, unsigned rec_floats, unsigned* any_skipped) {
  hipLaunchKernelGGL(k_rays_scan, dim3(grid), dim3(256), 0, stream, rays, n_rays, rec_floats, any_skipped);
}
void rtx_launch_raygen_rays(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const float4* rays, unsigned ray_s0, unsigned ray_ns, unsigned rec4,
                            unsigned ts_log2, float4* rad) {
  hipLaunchKernelGGL(k_raygen_rays, dim3(grid), dim3(256), 0, stream, fp, ps, SPtr<const float4>(rays), ray_s0, ray_ns, rec4, ts_log2, rad);
}
void rtx_launch_rays_scan_owned(unsigned grid, hipStream_t stream, const FrameParams& fp, const float* rays, unsigned long long owned_pixels, unsigned ray_ns, unsigned rec_floats,
                                unsigned* any_skipped) {
  hipLaunchKernelGGL(k_rays_scan_owned, dim3(grid), dim3(256), 0, stream, fp, rays, owned_pixels, ray_ns, rec_floats, any_skipped);
}
void rtx_launch_raygen_rays_film(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const float4* rays, const float2* p_film, unsigned ray_s0,
                                 unsigned ray_ns, unsigned rec4, unsigned ts_log2, const unsigned char* active) {
  if (active) hipLaunchKernelGGL(k_raygen_rays_film_masked, dim3(grid), dim3(256), 0, stream, fp, ps, SPtr<const float4>(rays), SPtr<const float2>(p_film), ray_s0, ray_ns, rec4, ts_log2, active);
  else hipLaunchKernelGGL(k_raygen_rays_film, dim3(grid), dim3(256), 0, stream, fp, ps, SPtr<const float4>(rays), SPtr<const float2>(p_film), ray_s0, ray_ns, rec4, ts_log2);
}
void rtx_launch_camera_rays(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, unsigned ray_s0, unsigned ray_ns, unsigned rec4, float4* rays,
                            float2* p_film) {
  hipLaunchKernelGGL(k_camera_rays, dim3(grid), dim3(256), 0, stream, fp, ps, ray_s0, ray_ns, rec4, rays, p_film);
}
void rtx_launch_frame_sums_read(hipStream_t stream, const FrameParams& fp, const float4* film_acc, const float4* own_plane, float4* out, unsigned long long n) {
  hipLaunchKernelGGL(k_frame_sums_read, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fp, film_acc, own_plane, out, n);
}

}  // namespace rtx
