// rtx_rays_launch.h - bounce 0 from caller-supplied rays (rtx_rays.hip: k_rays_scan, k_raygen_rays): what the frame of rt_render_rays launches where the other frames
// launch k_raygen, and what the step of a ray frame (rt_frame_advance_rays*) launches: k_rays_scan_owned on a shard, k_raygen_rays_film / _masked. A translation unit of
// its own, so that the code object of rtx_hip.hip - every kernel of the other frames - is what it was before ray frames existed.
// Included after rtx_kernels.h.
#pragma once
namespace rtx {
void rtx_launch_rays_scan(unsigned grid, hipStream_t stream, const float* rays, unsigned long long n_rays, unsigned rec_floats, unsigned* any_skipped);
void rtx_launch_raygen_rays(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const float4* rays, unsigned ray_s0, unsigned ray_ns, unsigned rec4,
                            unsigned ts_log2, float4* rad);
void rtx_launch_rays_scan_owned(unsigned grid, hipStream_t stream, const FrameParams& fp, const float* rays, unsigned long long owned_pixels, unsigned ray_ns, unsigned rec_floats,
                                unsigned* any_skipped);
// active == NULL: k_raygen_rays_film, else k_raygen_rays_film_masked. p_film may be NULL (pixel centres).
void rtx_launch_raygen_rays_film(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const float4* rays, const float2* p_film, unsigned ray_s0,
                                 unsigned ray_ns, unsigned rec4, unsigned ts_log2, const unsigned char* active);
// rt_camera_rays: k_camera_rays on the samples of a pass - records of rec4 float4 (2, or 5 with differentials) and film positions (p_film may be NULL) into the
// call's [pixel_index][ray_ns] arrays
void rtx_launch_camera_rays(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, unsigned ray_s0, unsigned ray_ns, unsigned rec4, float4* rays,
                            float2* p_film);
// rt_frame_read(RT_FRAME_SUMS): the frame's (sum w L).rgb and weight sum per cropped pixel, unresolved (k_frame_sums_read)
void rtx_launch_frame_sums_read(hipStream_t stream, const FrameParams& fp, const float4* film_acc, const float4* own_plane, float4* out, unsigned long long n);
}
