// rtx_shade_launch.h - the launches of the k_shade instantiations, which live in a translation unit of their own (rtx_shade.hip) so that the library's two halves
// compile side by side (a clean build: ~1 min instead of ~2). Included after rtx_kernels.h.
#pragma once
namespace rtx {
// one shade launch of front-end MODE (0 generic, 3 Lambert, 5 / 6 two-lobe): the GENERAL form (quadric / instance hits, masked emitters), the LEAN form (area lights and
// constant textures only), its QLIGHTS form (area lights on analytic spheres), the BOUNCED form of front-end 3, or the plain one; lds = k_shade's LDSREC
void rtx_launch_shade(int mode, bool general, bool lean, bool bounced, unsigned grid, unsigned block, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, bool qlights, int lds);
// k_shade<1> (constant matte, area lights): ldsrec 0 / 1 / 3. live_args (RTX_SHADE_KARGS=0, the control of S1's frames): the kernels of ldsrec 1 and the split kernels in
// the form that keeps the kernel arguments live through the vertex (k_shade_const_live, k_shade_split_live: rtx_shade_kernels.h, RT_SHADE_KARGS)
void rtx_launch_shade_const(int ldsrec, unsigned grid, unsigned block, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, bool live_args = false);
// the frames of k_shade<1, .., LDSREC = 1> whose closest hits come from k_trace: k_shade_split<1> (bounce 0 of a pass that traces every sample) or k_shade_split<2>
// (bounces >= 1), workgroups of 256 lanes; hit_mask: the words that bounce's k_trace launch wrote (TraceIO::hit_mask)
void rtx_launch_shade_split(bool camera, unsigned grid, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, const unsigned long long* hit_mask, bool live_args = false);
// the byte offsets of the shade kernels' arguments in their kernarg segments, as the vertex bodies read them (rt_shade_karg_offsets)
void rtx_shade_karg_offsets(unsigned out[5]);
// k_feature_hits (first-hit features: it builds the interaction with the shade kernels' fill routines, so it lives beside them)
void rtx_launch_feature_hits(bool samples, bool general, unsigned grid, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, const FeatureOut& fo);
void rtx_shade_set_ewa_lut(const float* lut128);  // kEwaLut of that translation unit
// rtx_shade_rays.hip: bounce 0's shade launch of front-end `mode` for rays that carry differentials - k_shade_rays<mode, general>, the plain / GENERAL form of k_shade<mode>
// with LDSREC = 0, whose camera vertices take their differentials from the caller's records (rd)
void rtx_launch_shade_rays(int mode, bool general, unsigned grid, unsigned block, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& p, const RayDiffSrc& rd);
void rtx_shade_rays_set_ewa_lut(const float* lut128);  // kEwaLut of that translation unit
// rt_bsdf_eval: one Bsdf front-end of k_shade - mode 0 GenericBsdf, 3 SingleLambertT, 5 SmallBsdfT<false>, 6 SmallBsdfT<true>; const_tex: the constant-texture form
// k_shade<1> and the LEAN forms use - on n queries, one lane each. Device pointers; surface NULL = the canonical hit. d.tri_p: record k carries orientation flag k (0, 1).
struct BsdfEvalArgs { int material; const float4* surface; const float* wo; const float* wi; const float* u; unsigned n; float* out; };
void rtx_launch_bsdf_eval(int mode, bool const_tex, unsigned grid, hipStream_t stream, const DScene& d, const BsdfEvalArgs& a);
}
