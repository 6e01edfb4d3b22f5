// rtx_camera_models.h - pbrt-v3's OrthographicCamera (cameras/orthographic.cpp, thin lens included) and EnvironmentCamera (cameras/environment.cpp) on the device:
// generate_model_ray, and k_camera_model_rays / k_camera_model_rays_masked (rtx_camera_model_rays.inl), which stand to it as k_camera_rays stands to
// generate_camera_ray. Included by rtx_cameras.hip alone (launcher: rtx_cameras_launch.h).
#pragma once
#include "rtx_kernels.h"
#include "rtx_cameras_launch.h"

namespace rtx {

// Camera-space ray of the model through the film position p (raster coordinates: x to the right, y downwards). DIFF: rx / ry as well - pbrt-v3's
// GenerateRayDifferential of each camera - before the world transform and the 1 / sqrt(spp) scaling.
struct ModelCamRay { f3 o, d, rx_o, ry_o, rx_d, ry_d; };
RT_DEV f3 environment_direction(const CameraModel& cm, float px, float py) {
  // theta = pi y / H, phi = 2 pi x / W; sinf / cosf, not the native approximations: a direction decides geometry
  const float theta = kPi * py / cm.height, phi = kTau * px / cm.width;
  const float st = sinf(theta);
  return mk3(st * cosf(phi), cosf(theta), st * sinf(phi));
}
template <bool DIFF>
RT_DEV ModelCamRay model_camera_space_ray(const CameraModel& cm, f2 p_film, f2 p_lens) {
  ModelCamRay r;
  if (cm.model == RT_CAMERA_ENVIRONMENT) {
    r.o = mk3(0.0f, 0.0f, 0.0f);
    r.d = environment_direction(cm, p_film.x, p_film.y);
    r.rx_o = r.o; r.ry_o = r.o; r.rx_d = r.d; r.ry_d = r.d;
    if (DIFF) {  // the base Camera::GenerateRayDifferential: the generator's own ray one raster pixel to the right and one down
      r.rx_d = environment_direction(cm, p_film.x + 1.0f, p_film.y);
      r.ry_d = environment_direction(cm, p_film.x, p_film.y + 1.0f);
    }
    return r;
  }
  // orthographic: the film position on the screen window of the plane z = 0 - raster y = 0 is the window's y1 -, the ray along +z
  const float x0 = cm.sw[0], x1 = cm.sw[1], y0 = cm.sw[2], y1 = cm.sw[3];
  const f3 p_cam = mk3(x0 + p_film.x / cm.width * (x1 - x0), y1 - p_film.y / cm.height * (y1 - y0), 0.0f);
  const f3 dx = mk3((x1 - x0) / cm.width, 0.0f, 0.0f), dy = mk3(0.0f, -(y1 - y0) / cm.height, 0.0f);
  r.o = p_cam; r.d = mk3(0.0f, 0.0f, 1.0f);
  if (cm.lens_radius > 0.0f) {  // pbrt-v3's thin lens: the ray leaves the lens point and passes through the pinhole ray's point on the plane of focus
    f2 pl = concentric_sample_disk(p_lens); pl.x = cm.lens_radius * pl.x; pl.y = cm.lens_radius * pl.y;
    float ft = cm.focal_distance / r.d.z;
    const f3 p_focus = p_cam + ft * r.d;
    r.o = mk3(pl.x, pl.y, 0.0f);
    r.d = normalize(p_focus - r.o);
    r.rx_o = r.o; r.ry_o = r.o; r.rx_d = r.d; r.ry_d = r.d;
    if (DIFF) {
      ft = cm.focal_distance / r.d.z;
      r.rx_d = normalize(p_cam + dx + mk3(0.0f, 0.0f, ft) - r.rx_o);
      r.ry_d = normalize(p_cam + dy + mk3(0.0f, 0.0f, ft) - r.ry_o);
    }
  } else {
    r.rx_o = r.o + dx; r.ry_o = r.o + dy; r.rx_d = r.d; r.ry_d = r.d;
  }
  return r;
}
// o_w = M o, d_w = normalize(M3x3 d): no origin nudge (rustracer_amd/cameras.py states the same in float64)
RT_DEV f3 model_point(const CameraModel& cm, f3 p) {
  const float* m = cm.c2w;
  return mk3(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7], m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]);
}
RT_DEV f3 model_direction(const CameraModel& cm, f3 v) {
  const float* m = cm.c2w;
  return normalize(mk3(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z));
}
// The model's world-space ray of a camera sample: p_film = pixel + 2D#0, p_lens = 2D#1 (read only where lens_radius > 0). The differentials are transformed as the
// main ray is and pulled toward it by diff_scale = 1 / sqrt(spp), as scale_differentials does; without DIFF they are the main ray's.
template <bool DIFF>
RT_DEV CameraRay generate_model_ray(const CameraModel& cm, f2 p_film, f2 p_lens, float diff_scale) {
  const ModelCamRay c = model_camera_space_ray<DIFF>(cm, p_film, p_lens);
  CameraRay r;
  r.o = model_point(cm, c.o); r.d = model_direction(cm, c.d);
  r.rx_o = r.o; r.ry_o = r.o; r.rx_d = r.d; r.ry_d = r.d;
  if (DIFF) {
    r.rx_o = model_point(cm, c.rx_o); r.ry_o = model_point(cm, c.ry_o);
    r.rx_d = model_direction(cm, c.rx_d); r.ry_d = model_direction(cm, c.ry_d);
    r.rx_o = r.o + (r.rx_o - r.o) * diff_scale; r.ry_o = r.o + (r.ry_o - r.o) * diff_scale;
    r.rx_d = r.d + (r.rx_d - r.d) * diff_scale; r.ry_d = r.d + (r.ry_d - r.d) * diff_scale;
  }
  return r;
}

// k_camera_rays for a model: one lane per (pixel, sample) of the pass with the SAMPLE running fastest, records into the [pixel_index][ray_ns] arrays.
static __global__ void __launch_bounds__(256) k_camera_model_rays(FrameParams fp, PassState ps, CameraModel cm, unsigned ray_s0, unsigned ray_ns, unsigned rec4,
                                                                  float4* __restrict__ rays, float2* __restrict__ p_film_out) {
#include "rtx_camera_model_rays.inl"
}
// ... of an adaptive step of a model frame: a pixel whose byte is 0 takes none of the step's samples, and no record of it is written.
static __global__ void __launch_bounds__(256) k_camera_model_rays_masked(FrameParams fp, PassState ps, CameraModel cm, unsigned ray_s0, unsigned ray_ns, unsigned rec4,
                                                                         float4* __restrict__ rays, float2* __restrict__ p_film_out,
                                                                         const unsigned char* __restrict__ active) {
#define RT_CAMERA_MODEL_MASKED
#include "rtx_camera_model_rays.inl"
#undef RT_CAMERA_MODEL_MASKED
}

}  // namespace rtx
