// rtx_shade.hip - the k_shade instantiations (K3, rtx_kernels.h) and their launches: a translation unit of its own, compiled beside rtx_hip.hip.
#include <hip/hip_runtime.h>
#include "../../include/rtx_hip.h"
#include "rtx_shade_kernels.h"
#include "rtx_shade_launch.h"

namespace rtx {
// one shade launch of front-end MODE: the GENERAL form (quadric / instance hits, masked emitters), the LEAN form (area lights and constant textures only;
// front-ends 3 / 5 / 6), or the plain one
template <int MODE>
static void launch_shade_t(bool general, bool lean, bool bounced, unsigned grid, unsigned block, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, bool qlights = false, int lds = 0) {
  // sphere lights over constant textures: the front-end ranges hold triangle vertices only (quadric hits are binned into the generic range)
  // lds (LEAN / QLIGHTS forms): 1 = the scene's records, lights, materials and textures fit the kernel's LDS, 2 = its materials and textures do (k_shade's LDSREC)
  if constexpr (MODE != 0) {
    if (qlights) {
      if (lds == 1) hipLaunchKernelGGL((k_shade<MODE, false, true, false, true, 1>), dim3(grid), dim3(block), 0, stream, d, fp, p);
      else if (lds == 2) hipLaunchKernelGGL((k_shade<MODE, false, true, false, true, 2>), dim3(grid), dim3(block), 0, stream, d, fp, p);
      else hipLaunchKernelGGL((k_shade<MODE, false, true, false, true>), dim3(grid), dim3(block), 0, stream, d, fp, p);
      return;
    }
  }
  if (general) { hipLaunchKernelGGL((k_shade<MODE, true>), dim3(grid), dim3(block), 0, stream, d, fp, p); return; }
  if constexpr (MODE != 0) {
    if (lean) {
      if (lds == 2) hipLaunchKernelGGL((k_shade<MODE, false, true, false, false, 2>), dim3(grid), dim3(block), 0, stream, d, fp, p);
      else hipLaunchKernelGGL((k_shade<MODE, false, true>), dim3(grid), dim3(block), 0, stream, d, fp, p);
      return;
    }
  }
  // the Lambert front-end past the camera vertices: no differentials, bilinear image lookups, everything inline under a three-wave bound
  if constexpr (MODE == 3) {
    if (bounced) {
      if (lds == 3) hipLaunchKernelGGL((k_shade<3, false, false, true, false, 3>), dim3(grid), dim3(block), 0, stream, d, fp, p);
      else hipLaunchKernelGGL((k_shade<3, false, false, true>), dim3(grid), dim3(block), 0, stream, d, fp, p);
      return;
    }
  }
  if constexpr (MODE == 3 || MODE == 5 || MODE == 6) { if (lds == 3) { hipLaunchKernelGGL((k_shade<MODE, false, false, false, false, 3>), dim3(grid), dim3(block), 0, stream, d, fp, p); return; } }
  hipLaunchKernelGGL((k_shade<MODE, false>), dim3(grid), dim3(block), 0, stream, d, fp, p);
}

void rtx_launch_shade(int mode, bool general, bool lean, bool bounced, unsigned grid, unsigned block, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, bool qlights, int lds) {
  switch (mode) {
    case 3: launch_shade_t<3>(general, lean, bounced, grid, block, stream, d, fp, p, qlights, lds); break;
    case 5: launch_shade_t<5>(general, lean, bounced, grid, block, stream, d, fp, p, qlights, lds); break;
    case 6: launch_shade_t<6>(general, lean, bounced, grid, block, stream, d, fp, p, qlights, lds); break;
    default: launch_shade_t<0>(general, lean, bounced, grid, block, stream, d, fp, p, qlights, lds); break;
  }
}
void rtx_launch_shade_const(int ldsrec, unsigned grid, unsigned block, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, bool live_args) {
  if (ldsrec == 1 && live_args) hipLaunchKernelGGL(k_shade_const_live<1>, dim3(grid), dim3(block), 0, stream, d, fp, p);
  else if (ldsrec == 1) hipLaunchKernelGGL((k_shade<1, false, false, false, false, 1>), dim3(grid), dim3(block), 0, stream, d, fp, p);
  else if (ldsrec == 3) hipLaunchKernelGGL((k_shade<1, false, false, false, false, 3>), dim3(grid), dim3(block), 0, stream, d, fp, p);
  else hipLaunchKernelGGL(k_shade<1>, dim3(grid), dim3(block), 0, stream, d, fp, p);
}
void rtx_launch_shade_split(bool camera, unsigned grid, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, const unsigned long long* hit_mask, bool live_args) {
  if (live_args) {  // (RTX_SHADE_KARGS=0: the control)
    if (camera) hipLaunchKernelGGL(k_shade_split_live<RT_SPLIT_CAMERA>, dim3(grid), dim3(256), 0, stream, d, fp, p, hit_mask);
    else hipLaunchKernelGGL(k_shade_split_live<RT_SPLIT_BOUNCED>, dim3(grid), dim3(256), 0, stream, d, fp, p, hit_mask);
  }
  else if (camera) hipLaunchKernelGGL(k_shade_split<RT_SPLIT_CAMERA>, dim3(grid), dim3(256), 0, stream, d, fp, p, hit_mask);
  else hipLaunchKernelGGL(k_shade_split<RT_SPLIT_BOUNCED>, dim3(grid), dim3(256), 0, stream, d, fp, p, hit_mask);
}
void rtx_shade_karg_offsets(unsigned out[5]) { out[0] = RT_KARG_SC; out[1] = RT_KARG_FP; out[2] = RT_KARG_PS; out[3] = RT_KARG_HIT_MASK; out[4] = RT_KARG_RDIFF; }
// ---- rt_bsdf_eval (rtx_hip.h): the front-end structs above on hand-made surface records. One lane per query builds the Bsdf of the material at its record the way
// shade_vertex does (the generic front-end takes the scene record in device memory, the others the kernel argument) and evaluates f, pdf and sample_f over all lobes.
RT_DEV int front_end_lobes(const GenericBsdf& b) { return b.b.n; }
template <bool T, bool B> RT_DEV int front_end_lobes(const SingleLambertT<T, B>& b) { return b.has ? 1 : 0; }
template <bool W, bool C> RT_DEV int front_end_lobes(const SmallBsdfT<W, C>& b) { return b.n; }
// the register budgets of the shade kernels the front-ends live in: two waves for the generic one, four for the constant Lambert form (k_shade<1>), three for the others
template <int MODE, bool CONST_TEX>
__global__ void __launch_bounds__(256, MODE == 0 ? RT_SHADE0_MIN_WAVES : ((MODE == 3 && CONST_TEX) ? RT_SHADE_MIN_WAVES : RT_SHADE56_MIN_WAVES)) k_bsdf_eval(DScene sc, BsdfEvalArgs a) {
  const unsigned stride = gridDim.x * blockDim.x;
  const DScene& gsc = *sc.self;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    const f3 wo = mk3(a.wo[3 * (size_t)i], a.wo[3 * (size_t)i + 1], a.wo[3 * (size_t)i + 2]), wi = mk3(a.wi[3 * (size_t)i], a.wi[3 * (size_t)i + 1], a.wi[3 * (size_t)i + 2]);
    const f2 u = mk2(a.u[2 * (size_t)i], a.u[2 * (size_t)i + 1]);
    SurfaceInteraction si;
    si.hit.p = mk3(0, 0, 0); si.hit.p_error = mk3(0, 0, 0); si.hit.wo = wo; si.hit.n = mk3(0, 0, 1);
    si.uv = mk2(0.5f, 0.5f); si.dpdu = mk3(1, 0, 0); si.dpdv = mk3(0, 1, 0);
    si.dudx = si.dvdx = si.dudy = si.dvdy = 0.0f; si.dpdx = si.dpdy = mk3(0, 0, 0);
    si.sh_n = mk3(0, 0, 1); si.sh_dpdu = mk3(1, 0, 0); si.sh_dpdv = mk3(0, 1, 0); si.prim = 0;
    if (a.surface) {  // RT_BSDF_SURFACE_FLOATS = 40: ten 16-byte loads
      const float4* r = a.surface + 10 * (size_t)i;
      const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5], r6 = r[6], r7 = r[7], r8 = r[8], r9 = r[9];
      si.hit.p = mk3(r0.x, r0.y, r0.z); si.hit.n = mk3(r0.w, r1.x, r1.y); si.sh_n = mk3(r1.z, r1.w, r2.x);
      si.dpdu = mk3(r2.y, r2.z, r2.w); si.dpdv = mk3(r3.x, r3.y, r3.z);
      si.sh_dpdu = mk3(r3.w, r4.x, r4.y); si.sh_dpdv = mk3(r4.z, r4.w, r5.x);  // (r5.yzw, r6.xyz: dndu / dndv - zero for every primitive a bump map meets, bump_map)
      si.uv = mk2(r6.w, r7.x); si.dudx = r7.y; si.dvdx = r7.z; si.dudy = r7.w; si.dvdy = r8.x;
      si.dpdx = mk3(r8.y, r8.z, r8.w); si.dpdy = mk3(r9.x, r9.y, r9.z);
      si.prim = r9.w != 0.0f ? 1 : 0;  // the scene record's two stand-in primitives: orientation flag 0 / 1
    }
    si.ssb = normalize(si.sh_dpdu);  // the first axis of Bsdf::new's frame, as k_tri_records / the triangle fill leave it
    typename std::conditional<MODE == 3, SingleLambertT<!CONST_TEX, false>, typename std::conditional<MODE == 5, SmallBsdfT<false, CONST_TEX>,
                              typename std::conditional<MODE == 6, SmallBsdfT<true, CONST_TEX>, GenericBsdf>::type>::type>::type bsdf;
    if (MODE == 0) bsdf.build(gsc, a.material, si); else bsdf.build(sc, a.material, si);
    const rgb3 f = bsdf.f(wo, wi, BSDF_ALL);
    const float pdf = bsdf.pdf(wo, wi, BSDF_ALL);
    const LobeSample s = bsdf.sample_f(wo, u, BSDF_ALL);
    float* o = a.out + (size_t)RT_BSDF_OUT_FLOATS * i;
    o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = pdf;
    o[4] = s.f.r; o[5] = s.f.g; o[6] = s.f.b; o[7] = s.wi.x; o[8] = s.wi.y; o[9] = s.wi.z; o[10] = s.pdf; o[11] = (float)s.type; o[12] = (float)front_end_lobes(bsdf);
  }
}
void rtx_launch_bsdf_eval(int mode, bool const_tex, unsigned grid, hipStream_t stream, const DScene& d, const BsdfEvalArgs& a) {
#define RT_BE(M, C) hipLaunchKernelGGL((k_bsdf_eval<M, C>), dim3(grid), dim3(256), 0, stream, d, a)
  switch (mode) {
    case 3: if (const_tex) RT_BE(3, true); else RT_BE(3, false); break;
    case 5: if (const_tex) RT_BE(5, true); else RT_BE(5, false); break;
    case 6: if (const_tex) RT_BE(6, true); else RT_BE(6, false); break;
    default: RT_BE(0, false); break;
  }
#undef RT_BE
}
// k_feature_hits after bounce 0's shade launches of a frame or call that asked for first-hit features (general: the scene holds quadrics or object instances)
void rtx_launch_feature_hits(bool samples, bool general, unsigned grid, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, const FeatureOut& fo) {
#define RT_FH(S, G) hipLaunchKernelGGL((k_feature_hits<S, G>), dim3(grid), dim3(256), 0, stream, d, fp, p, fo)
  if (samples) { if (general) RT_FH(true, true); else RT_FH(true, false); }
  else { if (general) RT_FH(false, true); else RT_FH(false, false); }
#undef RT_FH
}
void rtx_shade_set_ewa_lut(const float* lut128) { (void)hipMemcpyToSymbol(HIP_SYMBOL(kEwaLut), lut128, 128 * sizeof(float)); }
}  // namespace rtx
