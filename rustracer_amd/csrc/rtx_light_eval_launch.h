// rtx_light_eval_launch.h - rt_light_eval (rtx_light_eval.hip: one lane per query over the light functions of the shade kernels): what the C ABI hands its kernels.
// Included after rtx_dev_shading.h.
#pragma once
namespace rtx {
// Device pointers. light >= 0: that light for every query; < 0: the pick of uniform_sample_one_light from the scene's light-distribution tables (DScene::ld_*).
// wi NULL: no pdf_li / le query. ray_o / ray_d NULL: no shadow segments are written; otherwise every query gets one - spawn_ray_to_interaction(ref, p1) where the
// record has pdf > 0 and a non-black Li, a ray of t_max = 0 (nothing can occlude it; its answer is not read) elsewhere - in the planar layout the trace launches read.
struct LightEvalArgs { int light; const float* ref; const float* u; const float* wi; unsigned n; float* out; float4* ray_o; float4* ray_d; };
void rtx_launch_light_eval(bool general, hipStream_t stream, const DScene& d, const LightEvalArgs& a);
// folds the any-hit answers (one word per query, 1 = occluded) into float 15 of the records whose segment was traced
void rtx_launch_light_eval_fold(hipStream_t stream, const unsigned* occluded, unsigned n, float* out);
void rtx_light_eval_set_ewa_lut(const float* lut128);  // kEwaLut of that translation unit
}
