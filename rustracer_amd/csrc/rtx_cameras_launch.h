// rtx_cameras_launch.h - camera models beyond the perspective one (rtx_cameras.hip): pbrt-v3's orthographic and environment (lat-long) cameras, generated on the device
// from the pixel-keyed sampler's tables. The model travels as a kernel argument of its own (CameraModel): FrameParams and PassState are what they were, and so is the
// code object of every other translation unit. Included after rtx_kernels.h.
#pragma once
namespace rtx {
// rt_camera_model_rays' and a model frame's camera: RT_CAMERA_ORTHOGRAPHIC / RT_CAMERA_ENVIRONMENT, the affine camera-to-world matrix (row-major), the screen window
// (x0, x1, y0, y1), the thin lens and the film's full resolution
struct CameraModel { int model; float c2w[12]; float sw[4]; float lens_radius, focal_distance; float width, height; };
// k_camera_model_rays on the samples of a pass: records of rec4 float4 (2, or 5 with differentials) and film positions (p_film may be NULL) into [pixel_index][ray_ns]
// arrays - the caller's (rt_camera_model_rays) or the staging buffers of a model frame's step, which k_raygen_rays_film / k_shade_rays then read as a ray frame's.
// active != NULL: k_camera_model_rays_masked - the adaptive step of a model frame: a pixel whose byte is 0 gets no record (nothing reads it).
void rtx_launch_camera_model_rays(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const CameraModel& cm, unsigned ray_s0, unsigned ray_ns,
                                  unsigned rec4, float4* rays, float2* p_film, const unsigned char* active);
}
