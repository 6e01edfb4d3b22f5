// rtx_light_eval.hip - rt_light_eval (rtx_hip.h): the light half of the shade stage per query. One lane per query runs what estimate_direct's light-sampling half runs
// at a vertex - the light pick of uniform_sample_one_light (integrator/mod.rs:186-220) over the scene's light-distribution tables, Light::sample_li, Light::pdf_li,
// Light::le and the segment of VisibilityTester::unoccluded (light/mod.rs:52-55) - with the device functions the shade kernels call (rtx_dev_shading.h,
// rtx_dev_sphere.h): light_sample_li_full<GENERAL>, light_pdf_li<GENERAL>, d1_sample_discrete, voxel_of, infinite_le, spawn_ray_to_interaction. No copy of them lives
// here. The segments are traced by the scene's production any-hit launch (rtx_hip.hip); k_light_eval_fold writes its answers into the records. A translation unit of
// its own, compiled beside the others: no other kernel's code object changes.
#include <hip/hip_runtime.h>
#include "../../include/rtx_hip.h"
#include "rtx_dev_shading.h"
#include "rtx_light_eval_launch.h"

namespace rtx {

// out: RT_LIGHT_OUT_FLOATS per query - light, pick pdf, Li rgb, wi, pdf, p1.p, p1.n, visibility (-1: not traced), pdf_li(wi query), le(wi query) rgb
template <bool GENERAL>
__global__ void __launch_bounds__(256) k_light_eval(DScene sc, LightEvalArgs a) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  const DScene& gsc = *sc.self;  // the out-of-line light functions take the scene record in device memory
  const float* r = a.ref + (size_t)RT_LIGHT_REF_FLOATS * i;
  Interaction ref;
  ref.p = mk3(r[0], r[1], r[2]); ref.n = mk3(r[3], r[4], r[5]); ref.p_error = mk3(r[6], r[7], r[8]); ref.wo = mk3(0, 0, 0);
  float* o = a.out + (size_t)RT_LIGHT_OUT_FLOATS * i;
  int light_num = a.light; float light_pdf = 1.0f;
  if (light_num < 0) {  // light_distribution.lookup(p) (path.rs:154-158), then Distribution1D::sample_discrete
    const float* ld_func = sc.ld_func; const float* ld_cdf = sc.ld_cdf; float ld_int;
    if (sc.ld_uniform) ld_int = sc.ld_int[0];
    else {
      const long slot = sc.ld_slot[voxel_of(sc, ref.p)];
      if (slot >= 0) { ld_func = sc.ld_func + slot * sc.n_lights; ld_cdf = sc.ld_cdf + slot * (sc.n_lights + 1); ld_int = sc.ld_int[slot]; }
      else ld_int = -1.0f;  // a voxel the eager build did not mark: no table row
    }
    if (ld_int < 0.0f) { light_num = -1; light_pdf = 0.0f; }
    else d1_sample_discrete(ld_func, ld_cdf, ld_int, sc.n_lights, a.u[3 * (size_t)i], light_num, light_pdf);
    if (light_pdf == 0.0f) {  // uniform_sample_one_light returns black (mod.rs:205-207): the pick and zeros
      o[0] = (float)light_num; o[1] = 0.0f;
      for (int k = 2; k < RT_LIGHT_OUT_FLOATS; ++k) o[k] = 0.0f;
      if (a.ray_o != nullptr) { a.ray_o[i] = make_float4(ref.p.x, ref.p.y, ref.p.z, 0.0f); a.ray_d[i] = make_float4(0.0f, 0.0f, 1.0f, 0.0f); }
      return;
    }
  }
  const DLight& light = sc.lights[light_num];
  const LiSample ls = light_sample_li_full<GENERAL>(gsc, light, ref, mk2(a.u[3 * (size_t)i + 1], a.u[3 * (size_t)i + 2]));
  o[0] = (float)light_num; o[1] = light_pdf;
  o[2] = ls.li.r; o[3] = ls.li.g; o[4] = ls.li.b;
  o[5] = ls.wi.x; o[6] = ls.wi.y; o[7] = ls.wi.z; o[8] = ls.pdf;
  o[9] = ls.p1.p.x; o[10] = ls.p1.p.y; o[11] = ls.p1.p.z;
  o[12] = ls.p1.n.x; o[13] = ls.p1.n.y; o[14] = ls.p1.n.z;
  o[15] = -1.0f;
  float pdf_q = 0.0f; rgb3 le_q = mkc(0, 0, 0);
  if (a.wi != nullptr) {
    const f3 wq = mk3(a.wi[3 * (size_t)i], a.wi[3 * (size_t)i + 1], a.wi[3 * (size_t)i + 2]);
    pdf_q = light_pdf_li<GENERAL>(gsc, light, ref, wq);
    if (light.kind == 3) le_q = infinite_le(sc, light, wq);  // Light::le: only an infinite light has one (light/mod.rs:30-32)
  }
  o[16] = pdf_q; o[17] = le_q.r; o[18] = le_q.g; o[19] = le_q.b;
  if (a.ray_o != nullptr) {  // VisibilityTester { p0: ref, p1 }: the segment estimate_direct would trace (integrator/mod.rs:252-262)
    if (ls.pdf > 0.0f && !is_black(ls.li)) {
      const Ray sr = spawn_ray_to_interaction(ref, ls.p1);
      a.ray_o[i] = make_float4(sr.o.x, sr.o.y, sr.o.z, sr.t_max); a.ray_d[i] = make_float4(sr.d.x, sr.d.y, sr.d.z, 0.0f);
    } else { a.ray_o[i] = make_float4(ref.p.x, ref.p.y, ref.p.z, 0.0f); a.ray_d[i] = make_float4(0.0f, 0.0f, 1.0f, 0.0f); }
  }
}

__global__ void __launch_bounds__(256) k_light_eval_fold(const unsigned* __restrict__ occluded, unsigned n, float* __restrict__ out) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  float* o = out + (size_t)RT_LIGHT_OUT_FLOATS * i;
  if (o[8] > 0.0f && !is_black(mkc(o[2], o[3], o[4]))) o[15] = occluded[i] != 0u ? 0.0f : 1.0f;
}

void rtx_launch_light_eval(bool general, hipStream_t stream, const DScene& d, const LightEvalArgs& a) {
  const unsigned grid = (a.n + 255u) / 256u;
  if (general) hipLaunchKernelGGL((k_light_eval<true>), dim3(grid), dim3(256), 0, stream, d, a);
  else hipLaunchKernelGGL((k_light_eval<false>), dim3(grid), dim3(256), 0, stream, d, a);
}
void rtx_launch_light_eval_fold(hipStream_t stream, const unsigned* occluded, unsigned n, float* out) {
  hipLaunchKernelGGL(k_light_eval_fold, dim3((n + 255u) / 256u), dim3(256), 0, stream, occluded, n, out);
}
void rtx_light_eval_set_ewa_lut(const float* lut128) { (void)hipMemcpyToSymbol(HIP_SYMBOL(kEwaLut), lut128, 128 * sizeof(float)); }
}  // namespace rtx
