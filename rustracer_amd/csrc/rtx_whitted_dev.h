// rtx_whitted_dev.h - what the tree-walking integrators' vertex kernels share (rtx_whitted.hip: k_whitted_vertex, rtx_direct.hip: k_direct_vertex): the draw convention
// and the interaction of a step's hit. Device code; included after rtx_shade_kernels.h.
#pragma once
namespace rtx {

// the k-th get_2d() of a camera sample after get_camera_sample (cur_2d = 2): the table value 2D#(2 + k) while 2 + k < dimensions, then two draws of the sample's keyed
// stream in (second, first) order (zerotwosequence.rs:168-180), as rt_render_rays_ao defines it
struct WhittedDraws {
  Tables tb; unsigned pix, s; Pcg32 rng; bool rng_used;
  RT_DEV f2 get(unsigned k) {
    if (2u + k < tb.dims && k < 8u) return table_2d(tb, pix, 2u + k, s);
    const float first = rng.next_f32(), second = rng.next_f32();
    rng_used = true;
    return mk2(second, first);
  }
  // the k-th get_1d() after the camera sample's time draw (cur_1d = 1): table 1D#(1 + k) while 1 + k < dimensions, then ONE draw of the same stream, in call order with
  // get()'s (zerotwosequence.rs:158-166)
  RT_DEV float get_1d(unsigned k) {
    if (1u + k < tb.dims && k < 8u) return table_1d(tb, pix, 1u + k, s);
    rng_used = true;
    return rng.next_f32();
  }
};

// The SurfaceInteraction of the hit `h4` (the frame loop's record: b2, prim, b0, b1) of the ray (ray_o, ray_d), as k_shade<0> fills it; returns the primitive whose
// records name the material and the emitter (inside an instance: the object's). depth 0 on a scene that reads differentials: the caller's, or the camera ray's.
template <bool GENERAL>
RT_DEV int whitted_interaction(const DScene& sc, const DScene& gsc, const FrameParams& fp, const PassState& ps, const RayDiffSrc& rdiff, const Tables& tb, unsigned pix, unsigned s,
                               unsigned pid, unsigned long long pixel_index, int depth, f3 ray_o, f3 ray_d, float4 h4, SurfaceInteraction& si) {
  int prim = __float_as_int(h4.y);
  TriHit th; th.t = 0.0f; th.b0 = h4.z; th.b1 = h4.w; th.b2 = h4.x;
  if (GENERAL && sc.n_instances != 0u && (unsigned)prim >= sc.n_top_prims)
    prim = sc.obj_general ? instance_fill_interaction<true>(gsc, (unsigned)prim, ray_o.x, ray_o.y, ray_o.z, ray_d.x, ray_d.y, ray_d.z, th.b0, th.b1, th.b2, si)
                          : instance_fill_interaction<false>(gsc, (unsigned)prim, ray_o.x, ray_o.y, ray_o.z, ray_d.x, ray_d.y, ray_d.z, th.b0, th.b1, th.b2, si);
  else if (GENERAL && (tri_flags(sc.tri_p, prim) & RT_FLAG_SPHERE)) {
    (void)sphere_fill_interaction(sc.spheres[prim_sphere_index(sc.tri_p, prim)], ray_o, ray_d, si);
    si.ssb = normalize(si.sh_dpdu);
    si.prim = prim;
  }
  else tri_fill_interaction(gsc, prim, ray_d, th, si);
  if (depth == 0 && sc.needs_differentials) {  // only the first vertex's ray carries differentials (interaction.rs:245-314)
    if (rdiff.rays != nullptr) {  // floats 8 - 19 of the caller's record: rx_o, ry_o, rx_d, ry_d, used as given (k_shade_rays)
      const float4* r = rdiff.rays + (size_t)((pixel_index * rdiff.ray_ns + (s - rdiff.ray_s0)) * rdiff.rec4) + 2;
      const float4 r0 = r[0], r1 = r[1], r2 = r[2];
      compute_differential_call(si, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w));
    } else {  // the perspective camera's, rebuilt from the film position (k_shade)
      const float2 t = sraw(ps.pfilm)[pid];
      const f2 pl = fp.lens_radius > 0.0f ? table_2d(tb, pix, 1, s) : mk2(0.0f, 0.0f);
      const CameraRay cr = generate_camera_ray(fp, mk2(t.x, t.y), pl, 1.0f / sqrtf((float)ps.spp));
      compute_differential_call(si, cr.rx_o, cr.ry_o, cr.rx_d, cr.ry_d);
    }
  }
  return prim;
}
}  // namespace rtx
