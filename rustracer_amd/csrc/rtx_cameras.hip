// rtx_cameras.hip - the camera models of rt_camera_model_rays and of model frames (rt_frame_begin_model): pbrt-v3's orthographic and environment cameras generated on
// the device (rtx_camera_models.h), and their launcher. Compiled beside the other translation units, whose code objects stay what they were.
#include <hip/hip_runtime.h>
#include "../../include/rtx_hip.h"
#include "rtx_camera_models.h"

namespace rtx {

void rtx_launch_camera_model_rays(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const CameraModel& cm, unsigned ray_s0, unsigned ray_ns,
                                  unsigned rec4, float4* rays, float2* p_film, const unsigned char* active) {
  if (active) hipLaunchKernelGGL(k_camera_model_rays_masked, dim3(grid), dim3(256), 0, stream, fp, ps, cm, ray_s0, ray_ns, rec4, rays, p_film, active);
  else hipLaunchKernelGGL(k_camera_model_rays, dim3(grid), dim3(256), 0, stream, fp, ps, cm, ray_s0, ray_ns, rec4, rays, p_film);
}

}  // namespace rtx
