// rtx_rays_launch.h - bounce 0 from caller-supplied rays (rtx_rays.hip: k_rays_scan, k_raygen_rays): what the frame of rt_render_rays launches where the other frames
// launch k_raygen. A translation unit of its own, so that the code object of rtx_hip.hip - every kernel of the other frames - is what it was before ray frames existed.
// Included after rtx_kernels.h.
#pragma once
namespace rtx {
void rtx_launch_rays_scan(unsigned grid, hipStream_t stream, const float* rays, unsigned long long n_rays, unsigned* any_skipped);
void rtx_launch_raygen_rays(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const float4* rays, unsigned ray_s0, unsigned ray_ns, unsigned ts_log2,
                            float4* rad);
}
