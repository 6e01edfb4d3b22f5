// rtx_shade_kernels.h - K3: the shade kernel k_shade<MODE, ...> and its Bsdf front-ends (split from rtx_kernels.h in round 6; compiled by rtx_shade.hip, and by rtx_shade_rays.hip for k_shade_rays).
#pragma once
#include "rtx_kernels.h"

namespace rtx {

// ================================================================================ K3 shade
struct PathSampler {  // ZeroTwoSequence::get_1d / get_2d (zerotwosequence.rs:158-180) for one (pixel, sample)
  Tables tb; unsigned pix, s; int c1, c2; Pcg32 rng;
  RT_DEV float get_1d() {
    if (c1 < (int)tb.dims) return table_1d(tb, pix, (unsigned)c1++, s);
    return rng.next_f32();
  }
  RT_DEV f2 get_2d() {
    if (c2 < (int)tb.dims) return table_2d(tb, pix, (unsigned)c2++, s);
    float x = rng.next_f32();
    float y = rng.next_f32();
    return mk2(y, x);  // (second draw, first draw), :174-179
  }
};

// ---- Bsdf front-ends. GenericBsdf is the tagged-lobe aggregate of rtx_dev_bsdf.h. SingleLambert is the
// same arithmetic specialised for the Bsdf a constant-texture matte material builds (one
// LambertianReflection lobe, or none when Kd is black): with one matching lobe the component choice,
// the u remap (u*1-0), the pdf average (/1) and the lobe sums (0+x) of Bsdf::{f,pdf,sample_f} are
// identities, so both front-ends return bit-identical values; the specialised one needs no lobe
// array in scratch and a fraction of the registers.
struct GenericBsdf {
  Bsdf b;
  RT_DEV void build(const DScene& sc, int mat, SurfaceInteraction& si) { build_bsdf(sc, mat, si, b); }  // a bump map rewrites si's shading geometry
  RT_DEV int num_nonspecular() const { return bsdf_num_components(b, BSDF_ALL & ~BSDF_SPECULAR); }
  RT_DEV rgb3 f(f3 wo, f3 wi, unsigned flags) const { return bsdf_f(b, wo, wi, flags); }
  RT_DEV float pdf(f3 wo, f3 wi, unsigned flags) const { return bsdf_pdf(b, wo, wi, flags); }
  RT_DEV LobeSample sample_f(f3 wo, f2 u, unsigned flags) const { return bsdf_sample_f(b, wo, u, flags); }
  RT_DEV float eta() const { return b.eta; }
};
template <bool TEXTURED, bool BOUNCED = false>  // TEXTURED: Kd may be any texture (evaluated out of line); false: constant Kd only, no call in the kernel; BOUNCED: the vertex is past the camera ray (no differentials: the inline level-0 bilinear lookup)
struct SingleLambertT {
  rgb3 r; bool has; f3 ns, ng, ss, ts;
  RT_DEV void build(const DScene& sc, int mat, SurfaceInteraction& si) {  // matte.rs:37-62 with sigma == 0 and no bump map
    const int kd = sc.materials[mat].slot[0];
    const DTexture& t = sc.textures[kd];
    if (TEXTURED && t.kind != RT_TEX_CONST && !RT_DBG(sc, 1)) r = clamp_pos(BOUNCED ? tex_eval_leaf_bounced(sc, kd, si) : tex_eval_leaf(sc, kd, si));
    else r = (TEXTURED && t.kind != RT_TEX_CONST) ? mkc(0.75f, 0.75f, 0.75f) : clamp_pos(mkc(t.v[0], t.v[1], t.v[2]));
    has = !is_black(r);
    ss = si.ssb; ns = si.sh_n; ng = si.hit.n; ts = cross(si.sh_n, ss);  // Bsdf::new, bsdf/mod.rs:77-91 (ssb = normalize(si.sh_dpdu))
  }
  RT_DEV f3 to_local(f3 v) const { return mk3(dot(v, ss), dot(v, ts), dot(v, ns)); }
  RT_DEV int num_nonspecular() const { return has ? 1 : 0; }
  RT_DEV rgb3 f(f3 wo_w, f3 wi_w, unsigned) const {
    f3 wo = to_local(wo_w);
    if (!has || wo.z == 0.0f) return mkc(0, 0, 0);
    bool refl = dot(wi_w, ng) * dot(wo_w, ng) > 0.0f;
    return refl ? r * kInvPi : mkc(0, 0, 0);
  }
  RT_DEV float pdf(f3 wo_w, f3 wi_w, unsigned) const {
    if (!has) return 0.0f;
    f3 wo = to_local(wo_w);
    if (wo.z == 0.0f) return 0.0f;
    f3 wi = to_local(wi_w);
    return default_pdf(wo, wi);
  }
  RT_DEV LobeSample sample_f(f3 wo_w, f2 u, unsigned) const {
    if (!has) return mk_ls(mkc(0, 0, 0), mk3(0, 0, 0), 0.0f, 0u);
    f2 ur = mk2(fminf(u.x * 1.0f - 0.0f, kOneMinusEpsilon), u.y);
    f3 wo = to_local(wo_w);
    if (wo.z == 0.0f) return mk_ls(mkc(0, 0, 0), mk3(0, 0, 0), 0.0f, BSDF_DIFFUSE | BSDF_REFLECTION);
    f3 wi = cosine_sample_hemisphere(ur);
    if (wo.z < 0.0f) wi.z *= -1.0f;
    float pdf = default_pdf(wo, wi);
    if (pdf == 0.0f) return mk_ls(mkc(0, 0, 0), mk3(0, 0, 0), 0.0f, 0u);
    f3 wi_w = mk3(ss.x * wi.x + ts.x * wi.y + ns.x * wi.z, ss.y * wi.x + ts.y * wi.y + ns.y * wi.z, ss.z * wi.x + ts.z * wi.y + ns.z * wi.z);
    bool refl = dot(wi_w, ng) * dot(wo_w, ng) > 0.0f;
    return mk_ls(refl ? r * kInvPi : mkc(0, 0, 0), wi_w, pdf, 0u);
  }
  RT_DEV float eta() const { return 1.0f; }
};
typedef SingleLambertT<false> SingleLambert;

// Register-resident front-end for the materials that build at most two lobes out of {Lambertian, Oren-Nayar, microfacet
// reflection, specular reflection}: matte (any sigma), plastic, metal, mirror, without bump map. Bsdf::{f, pdf, sample_f}
// (bsdf/mod.rs:94-251) restated over two named lobes; every lobe function is entered with its kind as a constant, so only that
// kind's code is instantiated. Same operations in the same order as GenericBsdf (sums start from the same zero, the same component
// choice and u remap), hence the same values.
// MULTI: compute_scattering_functions' allow_multiple_lobes, read by glass alone - true is the path integrator's (every shade kernel), false the Whitted integrator's form
// (build_bsdf<false>, rtx_dev_shading.h): smooth glass as SpecularReflection + SpecularTransmission
template <bool WIDE, bool CONST_TEX = false, bool MULTI = true>  // WIDE: + glass, substrate and the opaque uber form (FresnelSpecular, FresnelBlend, microfacet transmission; a Bsdf eta); CONST_TEX: every texture parameter is a constant (no out-of-line image lookup is instantiated)
struct SmallBsdfT {
  static RT_DEV rgb3 tc(const DScene& sc, int id, const SurfaceInteraction& si) { if (CONST_TEX) { const DTexture& t = sc.textures[id]; return mkc(t.v[0], t.v[1], t.v[2]); } return tex_eval_c(sc, id, si); }
  static RT_DEV float tcf(const DScene& sc, int id, const SurfaceInteraction& si) { return tc(sc, id, si).r; }
  f3 ns, ng, ss, ts; int n; Lobe l0, l1; float eta_;
  RT_DEV void add(const Lobe& l) { if (n == 0) l0 = l; else l1 = l; ++n; }
  RT_DEV void build(const DScene& sc, int mat, SurfaceInteraction& si) {
    const DMaterial& m = sc.materials[mat]; const int* s = m.slot;
    n = 0; l0 = lobe_zero(LB_LAMBERT_R); l1 = l0; eta_ = 1.0f;
    if (WIDE && m.kind == 4) {  // glass.rs:53-106, allow_multiple_lobes = MULTI (true: path.rs:145): one FresnelSpecular lobe, or microfacet reflection + transmission
      eta_ = tcf(sc, s[8], si);
      float ur = tcf(sc, s[6], si), vr = tcf(sc, s[7], si);
      rgb3 r = tc(sc, s[2], si), t = tc(sc, s[3], si);
      if (!is_black(r) || !is_black(t)) {
        if (MULTI && ur == 0.0f && vr == 0.0f) {
          Lobe l = lobe_zero(LB_FRESNEL_SPEC); l.r = r; l.t = t; l.eta_a = 1.0f; l.eta_b = eta_; add(l);
        } else if (!MULTI && ur == 0.0f && vr == 0.0f) {  // glass.rs:80-99: SpecularReflection over a dielectric Fresnel (1, eta), then SpecularTransmission
          if (!is_black(r)) { Lobe l = lobe_zero(LB_SPEC_R); l.r = r; l.fr_kind = FR_DIELECTRIC; l.fr_ei = 1.0f; l.fr_et = eta_; add(l); }
          if (!is_black(t)) add(mk_spec_t(t, 1.0f, eta_));
        } else {
          if (m.remap) { ur = tr_roughness_to_alpha(ur); vr = tr_roughness_to_alpha(vr); }
          if (!is_black(r)) add(mk_micro_r(r, ur, vr, FR_DIELECTRIC, 1.0f, eta_));
          if (!is_black(t)) add(mk_micro_t(r, ur, vr, 1.0f, eta_));  // passes `r` (glass.rs:97)
        }
      }
    } else if (WIDE && m.kind == 5) {  // uber.rs:63-126 where the host found opacity, Kr and Kt constant with 1 - opacity, Kr and Kt black: no specular lobe
      float e = tcf(sc, s[8], si);
      rgb3 op = clamp_pos(tc(sc, s[10], si));
      eta_ = e;
      rgb3 kd = op * clamp_pos(tc(sc, s[0], si));
      if (!is_black(kd)) add(mk_lambert(LB_LAMBERT_R, kd));
      rgb3 ks = op * clamp_pos(tc(sc, s[1], si));
      if (!is_black(ks)) {
        float ru = tcf(sc, s[6] >= 0 ? s[6] : s[5], si), rv = tcf(sc, s[7] >= 0 ? s[7] : s[5], si);
        if (m.remap) { ru = tr_roughness_to_alpha(ru); rv = tr_roughness_to_alpha(rv); }
        add(mk_micro_r(ks, ru, rv, FR_DIELECTRIC, 1.0f, e));
      }
    } else if (WIDE && m.kind == 6) {  // substrate.rs:43-71
      rgb3 d = clamp_pos(tc(sc, s[0], si)), sp = clamp_pos(tc(sc, s[1], si));
      float ru = tcf(sc, s[6], si), rv = tcf(sc, s[7], si);
      if (!is_black(d) || !is_black(sp)) {
        if (m.remap) { ru = tr_roughness_to_alpha(ru); rv = tr_roughness_to_alpha(rv); }
        Lobe l = lobe_zero(LB_FRESNEL_BLEND); l.r = d; l.t = sp; l.ax = ru; l.ay = rv; add(l);
      }
    } else if (m.kind == 0) {  // matte.rs:37-62
      rgb3 r = clamp_pos(tc(sc, s[0], si));
      float sigma = clampf(tcf(sc, s[4], si), 0.0f, 1.0f);
      if (!is_black(r)) {
        if (sigma == 0.0f) add(mk_lambert(LB_LAMBERT_R, r));
        else {  // OrenNayar::new, oren_nayar.rs:17-27
          Lobe l = lobe_zero(LB_OREN_NAYAR); l.r = r;
          float sigma_rad = sigma * (kPi / 180.0f);
          float sigma2 = sigma_rad * sigma_rad;
          l.ax = 1.0f - (sigma2 / (2.0f * (sigma2 + 0.33f)));
          l.ay = 0.45f * sigma2 / (sigma2 + 0.09f);
          add(l);
        }
      }
    } else if (m.kind == 1) {  // plastic.rs:45-75
      rgb3 kd = tc(sc, s[0], si), ks = tc(sc, s[1], si);
      if (!is_black(kd)) add(mk_lambert(LB_LAMBERT_R, kd));
      if (!is_black(ks)) {
        float rough = tcf(sc, s[5], si);
        if (m.remap) rough = tr_roughness_to_alpha(rough);
        add(mk_micro_r(ks, rough, rough, FR_DIELECTRIC, 1.5f, 1.0f));
      }
    } else if (m.kind == 2) {  // metal.rs:50-82
      float ur = tcf(sc, s[6] >= 0 ? s[6] : s[5], si), vr = tcf(sc, s[7] >= 0 ? s[7] : s[5], si);
      if (m.remap) { ur = tr_roughness_to_alpha(ur); vr = tr_roughness_to_alpha(vr); }
      Lobe l = mk_micro_r(mkc(1, 1, 1), ur, vr, FR_CONDUCTOR, 1.0f, 1.0f);
      l.t = tc(sc, s[8], si); l.k = tc(sc, s[9], si);
      add(l);
    } else {  // mirror.rs:30-48
      rgb3 R = clamp_pos(tc(sc, s[2], si));
      if (!is_black(R)) { Lobe l = lobe_zero(LB_SPEC_R); l.r = R; add(l); }
    }
    ss = si.ssb; ns = si.sh_n; ng = si.hit.n; ts = cross(si.sh_n, ss);  // Bsdf::new, bsdf/mod.rs:77-91 (ssb = normalize(si.sh_dpdu))
  }
  RT_DEV f3 to_local(f3 v) const { return mk3(dot(v, ss), dot(v, ts), dot(v, ns)); }
  // one lobe function entered with its kind as a compile-time constant
  template <class F> RT_DEV static auto with_kind(const Lobe& l, F fn) -> decltype(fn(l)) {
    Lobe c = l;
    switch (l.kind) {
      case LB_OREN_NAYAR: c.kind = LB_OREN_NAYAR; return fn(c);
      case LB_MICRO_R: c.kind = LB_MICRO_R; return fn(c);
      case LB_SPEC_R: c.kind = LB_SPEC_R; return fn(c);
      case LB_FRESNEL_SPEC: if (WIDE) { c.kind = LB_FRESNEL_SPEC; return fn(c); } break;
      case LB_FRESNEL_BLEND: if (WIDE) { c.kind = LB_FRESNEL_BLEND; return fn(c); } break;
      case LB_MICRO_T: if (WIDE) { c.kind = LB_MICRO_T; return fn(c); } break;
      case LB_SPEC_T: if (WIDE && !MULTI) { c.kind = LB_SPEC_T; return fn(c); } break;
      default: break;
    }
    c.kind = LB_LAMBERT_R; return fn(c);
  }
  RT_DEV static rgb3 lf(const Lobe& l, f3 wo, f3 wi) { return with_kind(l, [&](const Lobe& c) { return lobe_f_inner(c, wo, wi); }); }
  RT_DEV static float lp(const Lobe& l, f3 wo, f3 wi) { return with_kind(l, [&](const Lobe& c) { return lobe_pdf_inner(c, wo, wi); }); }
  RT_DEV static LobeSample lsamp(const Lobe& l, f3 wo, f2 u) { return with_kind(l, [&](const Lobe& c) { return lobe_sample_inner<false>(c, wo, u); }); }
  RT_DEV int num(unsigned flags) const { return (n > 0 && lobe_matches(l0.kind, flags) ? 1 : 0) + (n > 1 && lobe_matches(l1.kind, flags) ? 1 : 0); }
  RT_DEV int num_nonspecular() const { return num(BSDF_ALL & ~BSDF_SPECULAR); }
  RT_DEV static bool admits(const Lobe& l, unsigned flags, bool refl) {
    const unsigned ty = lobe_type(l.kind);
    return ((ty & flags) == ty) && ((refl && (ty & BSDF_REFLECTION)) || (!refl && (ty & BSDF_TRANSMISSION)));
  }
  RT_DEV rgb3 f(f3 wo_w, f3 wi_w, unsigned flags) const {  // :94-111
    f3 wi = to_local(wi_w), wo = to_local(wo_w);
    if (wo.z == 0.0f) return mkc(0, 0, 0);
    bool refl = dot(wi_w, ng) * dot(wo_w, ng) > 0.0f;
    rgb3 c = mkc(0, 0, 0);
    if (n > 0 && admits(l0, flags, refl)) c = c + lf(l0, wo, wi);
    if (n > 1 && admits(l1, flags, refl)) c = c + lf(l1, wo, wi);
    return c;
  }
  RT_DEV float pdf(f3 wo_w, f3 wi_w, unsigned flags) const {  // :113-136
    if (n == 0) return 0.0f;
    f3 wo = to_local(wo_w);
    if (wo.z == 0.0f) return 0.0f;
    f3 wi = to_local(wi_w);
    int matched = 0; float p = 0.0f;
    if (n > 0 && lobe_matches(l0.kind, flags)) { ++matched; p += lp(l0, wo, wi); }
    if (n > 1 && lobe_matches(l1.kind, flags)) { ++matched; p += lp(l1, wo, wi); }
    return matched == 0 ? 0.0f : p / (float)matched;
  }
  RT_DEV LobeSample sample_f(f3 wo_w, f2 u, unsigned flags) const {  // :138-251
    const bool m0 = n > 0 && lobe_matches(l0.kind, flags), m1 = n > 1 && lobe_matches(l1.kind, flags);
    const int m = (m0 ? 1 : 0) + (m1 ? 1 : 0);
    if (m == 0) return mk_ls(mkc(0, 0, 0), mk3(0, 0, 0), 0.0f, 0u);
    int comp_i = (int)f2u_sat(floorf(u.x * (float)m));
    if (comp_i > m - 1) comp_i = m - 1;
    const bool second = m0 ? (comp_i == 1) : true;  // the comp_i-th matching lobe
    const Lobe bx = second ? l1 : l0;
    const unsigned bty = lobe_type(bx.kind);
    f2 ur = mk2(fminf(u.x * (float)m - (float)comp_i, kOneMinusEpsilon), u.y);
    f3 wo = to_local(wo_w);
    if (wo.z == 0.0f) return mk_ls(mkc(0, 0, 0), mk3(0, 0, 0), 0.0f, bty);
    LobeSample s = lsamp(bx, wo, ur);
    if (s.pdf == 0.0f) return mk_ls(mkc(0, 0, 0), mk3(0, 0, 0), 0.0f, 0u);
    f3 wi = s.wi;
    f3 wi_w = mk3(ss.x * wi.x + ts.x * wi.y + ns.x * wi.z, ss.y * wi.x + ts.y * wi.y + ns.y * wi.z, ss.z * wi.x + ts.z * wi.y + ns.z * wi.z);
    float pdf = s.pdf;
    if (!(bty & BSDF_SPECULAR) && m > 1) pdf += second ? lp(l0, wo, wi) : lp(l1, wo, wi);  // the other matching lobe
    if (m > 1) pdf /= (float)m;
    rgb3 fv = s.f;
    if (!(bty & BSDF_SPECULAR)) {
      bool refl = dot(wi_w, ng) * dot(wo_w, ng) > 0.0f;
      fv = mkc(0, 0, 0);
      if (n > 0 && admits(l0, flags, refl)) fv = fv + lf(l0, wo, wi);
      if (n > 1 && admits(l1, flags, refl)) fv = fv + lf(l1, wo, wi);
    }
    return mk_ls(fv, wi_w, pdf, s.type);
  }
  RT_DEV float eta() const { return WIDE ? eta_ : 1.0f; }
};

// The SurfaceInteraction of a hit inside an object instance: the object-space interaction of the object's primitive, then SurfaceInteraction::transform
// (primitive_to_world), rc/interaction.rs:156-190. Returns the primitive's index in the scene's arrays (material, flags).
// OBJ_GENERAL: the object may hold quadrics (DScene::obj_general) - an instantiation of its own, so that scenes of plain objects keep the function they had (instances-10k:
// one function with both branches cost the generic shade launches 80 B of call frame and 12 %)
// The instance a hit id names (the last whose id_base <= hit_id)
RT_DEV const DInstance& instance_of_hit(const DScene& sc, unsigned hit_id) {
  unsigned lo = 0, hi = sc.n_instances;
  while (hi - lo > 1u) { const unsigned mid = (lo + hi) >> 1; if (sc.instances[mid].id_base <= hit_id) lo = mid; else hi = mid; }
  return sc.instances[lo];
}
// SurfaceInteraction::transform(primitive_to_world) of the object-space interaction `s` of instance `in` (rc/interaction.rs:156-190)
RT_DEV void instance_transform_interaction(const DInstance& in, const SurfaceInteraction& s, int gprim, SurfaceInteraction& si) {
  f3 perr;
  si.hit.p = xf34_point_with_error(in.o2w, s.hit.p, s.hit.p_error, perr); si.hit.p_error = perr;
  si.hit.wo = normalize(xf34_vector(in.o2w, s.hit.wo));
  si.hit.n = normalize(xf34_normal(in.w2o, s.hit.n));
  si.uv = s.uv;
  si.dpdu = xf34_vector(in.o2w, s.dpdu); si.dpdv = xf34_vector(in.o2w, s.dpdv);
  si.dudx = si.dvdx = si.dudy = si.dvdy = 0.0f; si.dpdx = si.dpdy = mk3(0, 0, 0);
  si.sh_n = normalize(xf34_normal(in.w2o, s.sh_n));
  si.sh_dpdu = xf34_vector(in.o2w, s.sh_dpdu); si.sh_dpdv = xf34_vector(in.o2w, s.sh_dpdv);
  si.sh_n = face_forward(si.sh_n, si.hit.n);
  si.ssb = normalize(si.sh_dpdu);
  si.prim = gprim;
}
template <bool OBJ_GENERAL>
RT_DEVN int instance_fill_interaction(const DScene& sc, unsigned hit_id, float ox, float oy, float oz, float dx, float dy, float dz, float b0, float b1, float b2,
                                      SurfaceInteraction& si) {
  const DInstance& in = instance_of_hit(sc, hit_id);
  const int gprim = (int)(in.prim_base + (hit_id - in.id_base));
  const f3 d_obj = xf34_vector(in.w2o, mk3(dx, dy, dz));  // Transform * Ray: the direction as a vector (the origin does not enter a triangle's interaction)
  TriHit th; th.t = 0.0f; th.b0 = b0; th.b1 = b1; th.b2 = b2;
  SurfaceInteraction s;
  if (OBJ_GENERAL && (tri_flags(sc.tri_p, gprim) & RT_FLAG_SPHERE)) {  // a quadric of the object (round 6): Sphere::intersect builds its interaction from the OBJECT-space ray, then SurfaceInteraction::transform
    (void)sphere_fill_interaction(sc.spheres[prim_sphere_index(sc.tri_p, gprim)], xf34_point(in.w2o, mk3(ox, oy, oz)), d_obj, s);
  } else tri_fill_interaction_inl(sc, gprim, d_obj, th, s);
  instance_transform_interaction(in, s, gprim, si);
  return gprim;
}
// The same interaction handed to `f` instead of stored: every branch - a triangle of the object, each kind of quadric - builds an interaction of its own, transforms it
// and returns f's value, all inline. For a kernel that reads a few fields (k_feature_hits): nothing is merged in a struct, so nothing of it lives in memory.
template <bool OBJ_GENERAL, class F>
RT_DEV auto instance_interaction_visit(const DScene& sc, unsigned hit_id, f3 o, f3 d, float b0, float b1, float b2, F f) {
  const DInstance& in = instance_of_hit(sc, hit_id);
  const int gprim = (int)(in.prim_base + (hit_id - in.id_base));
  const f3 d_obj = xf34_vector(in.w2o, d);
  if (OBJ_GENERAL && (tri_flags(sc.tri_p, gprim) & RT_FLAG_SPHERE))
    return quadric_interaction_visit(sc.spheres[prim_sphere_index(sc.tri_p, gprim)], xf34_point(in.w2o, o), d_obj,
                                     [&in, gprim, f](const SurfaceInteraction& s) { SurfaceInteraction w; instance_transform_interaction(in, s, gprim, w); return f(w); });
  TriHit th; th.t = 0.0f; th.b0 = b0; th.b1 = b1; th.b2 = b2;
  SurfaceInteraction s, w; tri_fill_interaction_inl(sc, gprim, d_obj, th, s);
  instance_transform_interaction(in, s, gprim, w);
  return f(w);
}

// MODE 0: any material / texture / light. MODE 1: every material is matte with constant Kd and
// sigma == 0 and every light is a DiffuseAreaLight (decided by the host from the material and light
// tables); no texture then reads the camera-ray differentials and the kernel makes no out-of-line call.
// MODE 3: matte materials with sigma == 0 and no bump map - Kd any texture - under any kind of light: the register-resident
// front-end with the generic light and texture functions. MODE 5: matte (any sigma), plastic, metal and mirror without bump map
// through SmallBsdfT<false>; MODE 6: glass, substrate and opaque uber as well, through SmallBsdfT<true> (the narrow kernel is 5 % faster on its classes).
// k_shade<1> is bound to FOUR waves per SIMD (round 4): with the vertex body a function of (entry, slot) it fits 128 VGPRs with nothing spilled (round 3: 84 B of
// scratch at four, 381 -> 404 ms). S1 shade 299 -> 264 ms, 1248 -> 1300 Msamples/s; S2 1403 -> 1432 (two interleaved rounds).
#ifndef RT_SHADE_MIN_WAVES
#define RT_SHADE_MIN_WAVES 4
#endif
#ifndef RT_SHADE0_MIN_WAVES
#define RT_SHADE0_MIN_WAVES 2
#endif
// Round 4: the plain forms of the textured front-ends are bound to THREE waves per SIMD. Round 3 measured that as a loss (k_shade<3> 207 -> 168 VGPRs with 40
// spilled: S4 shade 4074 -> 4166 ms); since the vertex body became a function of (entry, slot) the kernels need 187 / 207 / 214 VGPRs, and at 168 with 24 / 46 /
// 59 spilled dwords (48 / 112 / 128 B of scratch) the third wave now pays: S4 shade 3027 -> 2972 ms (k_shade<3>) and -> 2854 ms (k_shade<5 | 6>), 353.0 -> 356.3 /
// 363.1 Msamples/s, two interleaved rounds on one box (scripts/ab_bench.sh).
#ifndef RT_SHADE_GEN_MIN_WAVES  // the GENERAL forms of the register-resident front-ends (quadric / instance hits, masked emitters)
#define RT_SHADE_GEN_MIN_WAVES 2
#endif
#ifndef RT_SHADE_BOUNCED_MIN_WAVES
#define RT_SHADE_BOUNCED_MIN_WAVES 3
#endif
#ifndef RT_SHADE_LEAN_MIN_WAVES
#define RT_SHADE_LEAN_MIN_WAVES 3
#endif
#ifndef RT_SHADE56_MIN_WAVES  // the two-lobe front-ends under any light / texture (k_shade<5 | 6>, plain form)
#define RT_SHADE56_MIN_WAVES 3
#endif
#ifndef RT_SHADE3_MIN_WAVES  // the Lambert front-end under any light (k_shade<3>)
#define RT_SHADE3_MIN_WAVES 3
#endif
// GENERAL (generic front-end only): some emitter triangle carries an alpha mask, so Shape::pdf_wi's re-intersection evaluates it; such scenes shade
// every vertex through k_shade<0, true>, every other scene never instantiates the mask evaluator in a shade kernel.
// LEAN (front-ends 3 / 5 / 6): every light is a diffuse area light on a triangle and every texture a constant - what MODE 1 assumes, for the other material
// classes. No out-of-line light or texture evaluator is instantiated, so the kernel's allocation is its own: 155 / 168 / 168 VGPRs under a three-wave bound
// (4 / 12 spilled dwords in the two-lobe forms) instead of 208 / 230 / 236 at two waves.
// BOUNCED (front-end 3, launches of bounces >= 1): no vertex of the launch is a camera vertex, so no differentials exist, image maps are level-0 bilinear lookups
// (inline) and the light evaluators are taken inline too: 183 VGPRs of its own, 168 under the three-wave bound with 5 spilled dwords.
// QLIGHTS (with LEAN, round 4): the LEAN form for scenes whose area lights may sit on analytic spheres - what veach-mis.pbrt is. The launch holds vertices on
// TRIANGLES only (k_bin_count sends every quadric hit to the generic bin, DScene::route_quadric_hits) and the host has checked that no triangle reaches into
// an emitter sphere (rt_scene_create: sphere_lights_clear), so Sphere::sample_si and Sphere::pdf_wi only ever take their cone branches (sphere.rs:264-308,
// 325-333) - inlined here, no out-of-line evaluator, three waves per SIMD like the other LEAN forms. Round 3 shaded such scenes through the GENERAL forms:
// 256 VGPRs and 352 - 448 B of scratch.
// LDSREC: 0 = every table in HBM; 1 = the scene's shade / traversal records, lights, materials and textures in LDS (small scenes); 2 = materials and textures only;
// 3 = lights, materials, textures and image headers (the plain forms of scenes with few of each)
// SPLIT (rtx_shade_body.inl; k_shade itself is SPLIT 0): what a frame of k_shade<1, .., LDSREC = 1> whose closest hits come from k_trace knows about a launch at compile time.
//  RT_SPLIT_CAMERA  - k_shade_split<1>: bounce 0 of a pass that traces every sample. Entry = slot = path id (one ring), throughput (1, 1, 1 | 1), bounces 0, no specular
//                     bounce, sampler counters (1, 2), the RNG at its stream's first state: neither travelling record is read (k_raygen wrote neither), no Russian roulette.
//  RT_SPLIT_BOUNCED - k_shade_split<2>: the launches of bounces >= 1, without the emission block.
// Both take the hits of their entries from the mask words the bounce's k_trace launch left (TraceIO::hit_mask), not from the hit records.
#define RT_SPLIT_NONE 0
#define RT_SPLIT_CAMERA 1
#define RT_SPLIT_BOUNCED 2
// RT_SHADE_KARGS (round 10, rtx_shade_body.inl: KARGS): 1 - every shade kernel's vertex body re-reads the kernel's arguments from the kernarg segment; 0 (make
// EXTRA=-DRT_SHADE_KARGS=0) - the entry block's copies stay live through the vertex, as before. The kernels' arguments as the kernarg segment lays them out: each at the
// next multiple of its alignment, which is how a struct of the same members is laid out. rt_shade_karg_offsets (rtx_hip.h) exports the offsets and
// tests/test_shade_kargs_cpu.py holds them to the `.offset` entries of the built kernels' argument metadata.
#ifndef RT_SHADE_KARGS
#define RT_SHADE_KARGS 1
#endif
struct ShadeKArgs { DScene sc; FrameParams fp; PassState ps; };                                            // k_shade
struct ShadeSplitKArgs { DScene sc; FrameParams fp; PassState ps; const unsigned long long* hit_mask; };  // k_shade_split
struct ShadeRaysKArgs { DScene sc; FrameParams fp; PassState ps; RayDiffSrc rdiff; };                     // k_shade_rays
#define RT_KARG_SC ((unsigned)offsetof(ShadeKArgs, sc))
#define RT_KARG_FP ((unsigned)offsetof(ShadeKArgs, fp))
#define RT_KARG_PS ((unsigned)offsetof(ShadeKArgs, ps))
#define RT_KARG_HIT_MASK ((unsigned)offsetof(ShadeSplitKArgs, hit_mask))
#define RT_KARG_RDIFF ((unsigned)offsetof(ShadeRaysKArgs, rdiff))
static_assert(offsetof(ShadeSplitKArgs, ps) == offsetof(ShadeKArgs, ps) && offsetof(ShadeRaysKArgs, ps) == offsetof(ShadeKArgs, ps) && offsetof(ShadeSplitKArgs, fp) == offsetof(ShadeKArgs, fp) &&
              offsetof(ShadeRaysKArgs, fp) == offsetof(ShadeKArgs, fp), "the three signatures share their first three arguments");
#define RT_KARG_AS __attribute__((address_space(4)))
// the kernarg segment's address behind an empty asm: what is loaded through it cannot be hoisted over the asm, and stays a scalar load from the constant address space
// (the host pass only parses the kernels)
RT_DEV const RT_KARG_AS char* shade_kargs() {
#if defined(__HIP_DEVICE_COMPILE__)
  const RT_KARG_AS char* p = (const RT_KARG_AS char*)__builtin_amdgcn_kernarg_segment_ptr(); asm volatile("" : "+s"(p)); return p;
#else
  return nullptr;
#endif
}
// one argument out of the segment: word loads through the constant address space, unrolled (the words nothing reads are never loaded), then a bit cast
template <class T> RT_DEV T shade_karg(const RT_KARG_AS char* ka, unsigned offset) {
  static_assert(sizeof(T) % 4 == 0 && alignof(T) >= 4 && std::is_trivially_copyable<T>::value, "an argument is copied by words");
  struct Words { unsigned w[sizeof(T) / 4]; } r;
  const RT_KARG_AS unsigned* s = (const RT_KARG_AS unsigned*)(ka + offset);
#pragma unroll
  for (unsigned k = 0; k < sizeof(T) / 4; ++k) r.w[k] = s[k];
  return __builtin_bit_cast(T, r);
}
template <int MODE, bool GENERAL = false, bool LEAN = false, bool BOUNCED = false, bool QLIGHTS = false, int LDSREC = 0>
__global__ void __launch_bounds__(256, (MODE == 1 || LEAN || BOUNCED) ? ((LEAN || BOUNCED) ? (BOUNCED ? RT_SHADE_BOUNCED_MIN_WAVES : RT_SHADE_LEAN_MIN_WAVES) : RT_SHADE_MIN_WAVES) : (MODE == 3 && !GENERAL ? RT_SHADE3_MIN_WAVES : ((MODE == 5 || MODE == 6) && !GENERAL ? RT_SHADE56_MIN_WAVES : (MODE != 0 && GENERAL ? RT_SHADE_GEN_MIN_WAVES : RT_SHADE0_MIN_WAVES)))) k_shade(DScene sc, FrameParams fp, PassState ps) {
  constexpr int SPLIT = RT_SPLIT_NONE; const unsigned long long* const hit_mask = nullptr;
  constexpr bool RAYDIFF = false; constexpr RayDiffSrc rdiff{};
  constexpr bool KARGS = RT_SHADE_KARGS != 0;
#include "rtx_shade_body.inl"
}
// The control of S1's frames (RTX_SHADE_KARGS=0, read per render call): k_shade<1, .., LDSREC = 1> and the two split kernels below with the arguments kept live, as they
// were before round 10, under names of their own.
template <int LDSREC>
__global__ void __launch_bounds__(256, RT_SHADE_MIN_WAVES) k_shade_const_live(DScene sc, FrameParams fp, PassState ps) {
  constexpr int MODE = 1, SPLIT = RT_SPLIT_NONE; constexpr bool GENERAL = false, LEAN = false, BOUNCED = false, QLIGHTS = false; const unsigned long long* const hit_mask = nullptr;
  constexpr bool RAYDIFF = false; constexpr RayDiffSrc rdiff{}; constexpr bool KARGS = false;
#include "rtx_shade_body.inl"
}
// The two kernels of such a frame: the same body under the same four-wave bound, hit_mask = the words the bounce's k_trace launch wrote.
// k_shade_split<2> has no emission block (path.rs:127-136, `bounces == 0 || specular_bounce`): a vertex of bounce >= 1 has bounces >= 1 - its producer stored bounces + 1 -
// and its specular_bounce is the BSDF_SPECULAR bit of the type SingleLambert::sample_f returned at the previous vertex, which is 0 or BSDF_DIFFUSE | BSDF_REFLECTION on
// every return path of that function (mk_ls(.., 0u) three times, the wo.z == 0 return): the scene has no specular lobe, the condition is false at every vertex of these launches.
// Measured on the allocation and not kept (128 VGPRs, spilled dwords; k_shade<1, .., 1>: 4): k_shade_split<2> with the two records loaded without the launch-uniform
// select 25, with its queue view known at compile time 27, both 32; k_shade_split<1> without the scheduling barrier behind its record loads 27 - 31 (all with a per-lane
// n_shaded, which alone cost both kernels three dwords). As they stood: 3 and 4; with the arguments re-read per vertex (RT_SHADE_KARGS, round 10) 0 and 0, and of those forms
// the unconditional loads and the barrier-free camera kernel then fit with nothing spilled but measure no gain (MEASUREMENTS R10).
template <int SPLIT>
__global__ void __launch_bounds__(256, RT_SHADE_MIN_WAVES) k_shade_split(DScene sc, FrameParams fp, PassState ps, const unsigned long long* __restrict__ hit_mask) {
  constexpr int MODE = 1, LDSREC = 1; constexpr bool GENERAL = false, LEAN = false, BOUNCED = false, QLIGHTS = false;
  constexpr bool RAYDIFF = false; constexpr RayDiffSrc rdiff{}; constexpr bool KARGS = RT_SHADE_KARGS != 0;
#include "rtx_shade_body.inl"
}
template <int SPLIT>  // (the control, see k_shade_const_live)
__global__ void __launch_bounds__(256, RT_SHADE_MIN_WAVES) k_shade_split_live(DScene sc, FrameParams fp, PassState ps, const unsigned long long* __restrict__ hit_mask) {
  constexpr int MODE = 1, LDSREC = 1; constexpr bool GENERAL = false, LEAN = false, BOUNCED = false, QLIGHTS = false;
  constexpr bool RAYDIFF = false; constexpr RayDiffSrc rdiff{}; constexpr bool KARGS = false;
#include "rtx_shade_body.inl"
}
// Bounce 0 of a call or ray-frame step whose rays carry differentials (RT_FLAG_RAY_DIFFERENTIALS, rtx_shade_rays.hip): the plain / GENERAL, LDSREC = 0 form of k_shade<MODE>
// under its launch bound, with the one site that builds a camera vertex's differentials reading them from the caller's record of the vertex's ray (RayDiffSrc) instead
// of regenerating the perspective camera's. MODE 0, 3, 5, 6: the forms that can see a camera vertex and read differentials.
template <int MODE, bool GENERAL>
__global__ void __launch_bounds__(256, MODE == 3 && !GENERAL ? RT_SHADE3_MIN_WAVES : ((MODE == 5 || MODE == 6) && !GENERAL ? RT_SHADE56_MIN_WAVES : (MODE != 0 && GENERAL ? RT_SHADE_GEN_MIN_WAVES : RT_SHADE0_MIN_WAVES))) k_shade_rays(DScene sc, FrameParams fp, PassState ps, RayDiffSrc rdiff) {
  constexpr int SPLIT = RT_SPLIT_NONE, LDSREC = 0; constexpr bool LEAN = false, BOUNCED = false, QLIGHTS = false, RAYDIFF = true; const unsigned long long* const hit_mask = nullptr; constexpr bool KARGS = RT_SHADE_KARGS != 0;
#include "rtx_shade_body.inl"
}


// ================================================================================ first-hit features (FeatureOut, rtx_kernels.h)
// One lane per entry of bounce 0's queue, launched right after that bounce's shade launches and before bounce 1's trace overwrites ps.hit: the camera ray k_raygen wrote
// (ps.in.o / .d), its closest hit (ps.hit) and the SurfaceInteraction the shade kernels built from the two - by the fill routines they call, inline here so that the
// interaction stays in registers. The entry's path id is its slot where the pass traces every sample (ps.cnt_in == NULL: entry i is slot i is path i, and k_raygen left the
// state record out), else the state record's. Reads: three or four 16-byte records at consecutive slots of consecutive lanes, then the gathers of the fill routine.
// The normal is the interaction's shading normal BEFORE compute_scattering_functions (no bump map), negated where dot(n, d) > 0. A miss: prim = -1, every feature zero.
// GENERAL: the scene holds quadrics or object instances.
RT_DEV float4 feature_normal_depth(const SurfaceInteraction& si, f3 ray_o, f3 ray_d) {
  const f3 n = dot(si.sh_n, ray_d) > 0.0f ? -si.sh_n : si.sh_n;
  return make_float4(n.x, n.y, n.z, len(si.hit.p - ray_o));
}
template <bool SAMPLES, bool GENERAL>
__global__ void __launch_bounds__(256) k_feature_hits(DScene sc, FrameParams fp, PassState ps, FeatureOut fo) {
  QView qv; if (ps.cnt_in) qv.init(nullptr, ps.cnt_in, ps.shard_cap);
  const unsigned count = ps.cnt_in ? qv.total() : ps.cap, stride = gridDim.x * blockDim.x;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const unsigned slot = ps.cnt_in ? qv.get(i) : i;
    const float4 o4 = sraw(ps.in.o)[slot], d4 = sraw(ps.in.d)[slot], h4 = sraw(ps.hit)[slot];
    const unsigned pid = ps.cnt_in ? sraw(ps.in.st)[slot].y : slot;
    const f3 ray_o = mk3(o4.x, o4.y, o4.z), ray_d = mk3(d4.x, d4.y, d4.z);
    const int prim = __float_as_int(h4.y);
    float4 nd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (normal | depth); each branch takes it from an interaction of its own
    if (prim >= 0) {
      TriHit th; th.t = 0.0f; th.b0 = h4.z; th.b1 = h4.w; th.b2 = h4.x;  // the frame loop's hit record is (b2, prim, b0, b1)
      const auto take = [ray_o, ray_d](const SurfaceInteraction& si) { return feature_normal_depth(si, ray_o, ray_d); };
      if (GENERAL && sc.n_instances != 0u && (unsigned)prim >= sc.n_top_prims)
        nd = sc.obj_general ? instance_interaction_visit<true>(sc, (unsigned)prim, ray_o, ray_d, th.b0, th.b1, th.b2, take)
                            : instance_interaction_visit<false>(sc, (unsigned)prim, ray_o, ray_d, th.b0, th.b1, th.b2, take);
      else if (GENERAL && (tri_flags(sc.tri_p, prim) & RT_FLAG_SPHERE)) nd = quadric_interaction_visit(sc.spheres[prim_sphere_index(sc.tri_p, prim)], ray_o, ray_d, take);
      else { SurfaceInteraction si; tri_fill_interaction_inl<true>(sc, prim, ray_d, th, si); nd = feature_normal_depth(si, ray_o, ray_d); }  // (wo is not read)
    }
    const bool hit = prim >= 0;
    if (SAMPLES) {
      float4* o = fo.samples + feature_sample_at(fp, ps, fo, pid);
      o[0] = make_float4(ray_o.x, ray_o.y, ray_o.z, ray_d.x);
      o[1] = make_float4(ray_d.y, ray_d.z, __int_as_float(hit ? prim : -1), hit ? h4.z : 0.0f);
      o[2] = make_float4(hit ? h4.w : 0.0f, nd.w, nd.x, nd.y);
      o[3] = make_float4(nd.z, 0.0f, 0.0f, 0.0f);
    } else {
      fo.nd[pid] = nd;
      fo.ah[pid] = make_float4(0.0f, 0.0f, 0.0f, hit ? 1.0f : 0.0f);
    }
  }
}

}  // namespace rtx
