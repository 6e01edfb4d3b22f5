// The body of the shade kernels (rtx_shade_kernels.h includes it in k_shade<...> and in k_shade_split<SPLIT>). Shared as text, not as a function, like rtx_raygen_body.inl:
// the kernels' LDS arrays are then function-scope statics of each KERNEL, under the names they had, and k_shade<...> compiles to the code it had before the split kernels
// existed (as a __device__ template the same text gave k_shade<1, .., 1> and k_shade<1, .., 3> two more spilled dwords each: the arrays' names order the LDS layout).
// Expects: MODE, GENERAL, LEAN, BOUNCED, QLIGHTS, LDSREC, SPLIT (constants), sc, fp, ps (the kernel's arguments) and hit_mask (the split kernels' argument, else NULL);
// RAYDIFF (constant) and rdiff (RayDiffSrc): k_shade_rays takes a camera vertex's differentials from the caller's ray records; false and unread in every other kernel.
// KARGS (constant): the vertex body re-reads sc, fp, ps (and rdiff) from the kernarg segment instead of keeping the entry block's copies live (RT_SHADE_KARGS, below).
  static_assert(SPLIT == RT_SPLIT_NONE || (MODE == 1 && LDSREC == 1), "the split kernels are forms of k_shade<1, .., LDSREC = 1>");
  // LDSREC (MODE 1, round 5): a scene of <= RT_SMALL_TRIS triangles and <= RT_LDS_LIGHTS emitters keeps its shade records, traversal records and light table in LDS
  // for the launch. k_shade<1> is busy issuing VALU instructions half of the time and waits for memory two thirds of a wave's life (SQ counters), yet neither ~10 % fewer
  // instructions nor an earlier scan load moved it - what it waits for is the texture path's address processing: ~40 vector memory instructions per vertex, the
  // gathers among them (a vertex's triangle, the picked light, the light's triangle: every lane its own address) served a few lanes per clock. Read from LDS they
  // do not go there at all. Same values, same arithmetic.
  __shared__ float4 s_rec[LDSREC == 1 ? 8 * RT_SMALL_TRIS : 1];
  __shared__ float4 s_trip[LDSREC == 1 ? 3 * RT_SMALL_TRIS : 1];
  __shared__ unsigned s_lights[(LDSREC == 1 || LDSREC == 3) ? RT_LDS_LIGHTS * (sizeof(DLight) / 4) : 1];
  __shared__ unsigned s_imgs[LDSREC == 3 ? RT_LDS_IMAGES * (sizeof(DImage) / 4) : 1];
  __shared__ unsigned s_mats[LDSREC ? RT_LDS_MATERIALS * (sizeof(DMaterial) / 4) : 1];
  __shared__ unsigned s_texs[LDSREC ? RT_LDS_TEXTURES * (sizeof(DTexture) / 4) : 1];
  // (round 6 also kept ONE environment light's marginal distribution - cdf, func, guide: 10 KB - in LDS for the plain forms: S4 shade 2368 -> 2378 ms, not kept; commit ec235f5)
  if (LDSREC) {
    if (LDSREC == 1) {
      for (unsigned k = threadIdx.x; k < 8u * sc.n_tris; k += blockDim.x) s_rec[k] = sc.tri_rec[k];
      for (unsigned k = threadIdx.x; k < 3u * sc.n_tris; k += blockDim.x) s_trip[k] = sc.tri_p[k];
    }
    if (LDSREC == 1 || LDSREC == 3) {
      const unsigned nl = (unsigned)sc.n_lights_all * (unsigned)(sizeof(DLight) / 4);
      for (unsigned k = threadIdx.x; k < nl; k += blockDim.x) s_lights[k] = ((const unsigned*)sc.lights)[k];
    }
    if (LDSREC == 3) for (unsigned k = threadIdx.x; k < (unsigned)sc.n_images * (unsigned)(sizeof(DImage) / 4); k += blockDim.x) s_imgs[k] = ((const unsigned*)sc.images)[k];
    for (unsigned k = threadIdx.x; k < (unsigned)sc.n_materials * (unsigned)(sizeof(DMaterial) / 4); k += blockDim.x) s_mats[k] = ((const unsigned*)sc.materials)[k];
    for (unsigned k = threadIdx.x; k < (unsigned)sc.n_textures * (unsigned)(sizeof(DTexture) / 4); k += blockDim.x) s_texs[k] = ((const unsigned*)sc.textures)[k];
    __syncthreads();
    if (LDSREC == 1) { sc.tri_rec = (const float4*)s_rec; sc.tri_p = (const float4*)s_trip; }
    if (LDSREC == 1 || LDSREC == 3) sc.lights = (const DLight*)s_lights;
    sc.materials = (const DMaterial*)s_mats; sc.textures = (const DTexture*)s_texs;
  }
  // The kernel's once-through streams (path records in and out, shadow / MIS ray records) with or without the non-temporal hint (SPtr, RT_NT_STREAMS): with it where the launch
  // also GATHERS from tables larger than a cache (triangle records, texels, environment rows - the hint keeps the streams from evicting them: S4 shade 2489 -> 2325 ms, S2
  // 22.0 -> 20.6, S3 117.6 -> 114.3); without it where every table sits in LDS and the streams are all the launch reads (LDSREC == 1: S1 shade 219 -> 234 ms WITH the hint).
  constexpr bool NTK = LDSREC != 1;
  constexpr bool CAMERA = SPLIT == RT_SPLIT_CAMERA;
  QView qv; if (ps.cnt_in) qv.init(ps.q_in, ps.cnt_in, ps.shard_cap);
  unsigned first = 0, count = ps.cnt_in ? qv.total() : ps.cap;  // no counts: bounce 0 of a pass whose samples are all traced (entry i = slot i = path i)
  if (MODE != 1 && ps.range) { first = ps.range[0]; count = ps.range[1]; }
  const unsigned stride = gridDim.x * blockDim.x;
  unsigned n_shaded = 0, n_unreached = 0, n_tail = 0, n_no_walk = 0;
#ifdef RT_ABLATE
  unsigned long long stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, stamp_last = clock64();
#endif
  // one vertex per lane: entry i of the launch's queue, its records at slot rslot. Must be reached by every thread of the workgroup (the queue appends at its
  // end are workgroup-wide).
  // KARGS (RT_SHADE_KARGS, round 10): every vertex re-reads the kernel's arguments from the kernarg segment. Taken by value they are loaded in the entry block and
  // whatever a vertex reads of them - a few hundred scalars - is hoisted out of the persistent loop and live through the whole vertex body: the allocator parks
  // 123 - 337 of them in lanes of vector registers (v_writelane / v_readlane), and those three or more vector registers are what pushes vector values over the
  // kernel's register bound into scratch. Behind the empty asm the pointer is opaque, so the loads (scalar, constant address space: ~45 more s_load per 256-vertex
  // iteration) stay inside the vertex and each field lives from its reload to its last use. Same values, same arithmetic. The LDS overrides above are re-applied.
  const DScene& sc_k = sc; const FrameParams& fp_k = fp; const PassState& ps_k = ps; const RayDiffSrc& rdiff_k = rdiff;
  auto shade_vertex = [&](const bool lane_live, const unsigned i, const unsigned rslot) __attribute__((always_inline)) {  // (two call sites in the compacting forms: with the asm in it the inliner would leave it a function)
    RT_STAMP(7);  // loop overhead / previous iteration's tail
    // (k_shade_rays keeps the pass state live: with all four re-read its GENERAL forms of front-ends 3 and 5 take 232 / 255 VGPRs, one more than their k_shade siblings
    // - tests/test_ray_differentials_cpu.py bounds them by the sibling's count -, with ps live 230 / 253 and not a spilled dword more in any of the eight)
    constexpr bool KARGS_PS = KARGS && !RAYDIFF;
    DScene sc_r; FrameParams fp_r; PassState ps_r; RayDiffSrc rdiff_r{};
    if constexpr (KARGS) {
      const RT_KARG_AS char* ka = shade_kargs();
      sc_r = shade_karg<DScene>(ka, RT_KARG_SC); fp_r = shade_karg<FrameParams>(ka, RT_KARG_FP); if constexpr (KARGS_PS) ps_r = shade_karg<PassState>(ka, RT_KARG_PS);
      if constexpr (RAYDIFF) rdiff_r = shade_karg<RayDiffSrc>(ka, RT_KARG_RDIFF);  // (re-read at its one use instead, it costs k_shade_rays<6, true> 4 spilled dwords)
      if (LDSREC == 1) { sc_r.tri_rec = (const float4*)s_rec; sc_r.tri_p = (const float4*)s_trip; }
      if (LDSREC == 1 || LDSREC == 3) sc_r.lights = (const DLight*)s_lights;
      if (LDSREC) { sc_r.materials = (const DMaterial*)s_mats; sc_r.textures = (const DTexture*)s_texs; }
    }
    const DScene& sc = KARGS ? sc_r : sc_k; const FrameParams& fp = KARGS ? fp_r : fp_k; const PassState& ps = KARGS_PS ? ps_r : ps_k; const RayDiffSrc& rdiff = (KARGS && RAYDIFF) ? rdiff_r : rdiff_k;
    const DScene& gsc = *sc.self;  // what out-of-line functions get: the scene record in device memory, not a private copy of the kernel argument
    const auto in_o = sp<NTK>(ps.in.o), in_d = sp<NTK>(ps.in.d), in_beta = sp<NTK>(ps.in.beta); const auto in_st = sp<NTK>(ps.in.st); const auto pfilm_ = sp<NTK>(ps.pfilm);
    const auto out_o = sp<NTK>(ps.out.o), out_d = sp<NTK>(ps.out.d), out_beta = sp<NTK>(ps.out.beta); const auto out_st = sp<NTK>(ps.out.st);
    const auto sh_o = sp<NTK>(ps.sh.o), sh_d = sp<NTK>(ps.sh.d), sh_add = sp<NTK>(ps.sh.add);
    const auto mi_o = sp<NTK>(ps.mi.o), mi_d = sp<NTK>(ps.mi.d), mi_a = sp<NTK>(ps.mi.a), mi_b = sp<NTK>(ps.mi.b), mi_c = sp<NTK>(ps.mi.c); const auto mi_flags = sp<NTK>(ps.mi.flags);
    bool cont = false, want_shadow = false, want_mis = false, mis_occlusion_only = false, tail = false, no_walk = false;
    // what a continuing path takes to its slot in the next bounce's queue (stored after the append below has named the slot)
    f3 nr_o = mk3(0, 0, 0), nr_d = mk3(0, 0, 0); rgb3 beta = mkc(0, 0, 0); float eta_scale = 1.0f; unsigned st_out = 0u, pid = 0u; unsigned long long rng_out = 0ull;
    if (lane_live) {
      // the vertex's records: four 16-byte loads at consecutive slots of consecutive lanes, requested together
      const float4 d4 = in_d[rslot], h4 = sraw(ps.hit)[rslot];  // (hit: read twice in a launch - never with the non-temporal hint; once by the split kernels, whose scan reads mask words)
      float4 b4 = make_float4(1.0f, 1.0f, 1.0f, 1.0f); uint4 s4 = make_uint4(pack_state(0, false, 1, 2), rslot, 0u, 0u);
      // (fresh: bounce 0 of a pass whose samples are all traced - k_raygen left the record out, PassState::fresh; compiled out of the forms whose frames keep both)
      constexpr int FRESH = (MODE == 1 && LDSREC == 1) ? RT_FRESH_RECORDS_LDS : RT_FRESH_RECORDS;  // (rt_render: fresh_planes - the frames of exactly this kernel)
      if (!CAMERA) {  // (k_shade_split<1>: k_raygen wrote neither record)
        if (!((FRESH & 1) && RT_FRESH_BETA(ps))) b4 = in_beta[rslot];
        if (!((FRESH & 2) && RT_FRESH_ST(ps))) s4 = in_st[rslot];
      }
      if (SPLIT != RT_SPLIT_NONE) __builtin_amdgcn_sched_barrier(0);  // (the record loads stay in front of the arithmetic on them: without it the camera kernel spills 27 dwords)
      pid = s4.y;
      unsigned sl, pix; split_path_id(ps, pid, sl, pix); const unsigned s = ps.s0 + sl;
      f3 ray_d = mk3(d4.x, d4.y, d4.z);
      beta = mkc(b4.x, b4.y, b4.z); eta_scale = b4.w;
      const unsigned st = s4.x;
      int bounces = CAMERA ? 0 : (int)(st & 0xffu); bool specular_bounce = CAMERA ? false : ((st >> 8) & 1u);
      PathSampler smp; smp.tb = tables_of(ps); smp.pix = pix; smp.s = s; smp.c1 = CAMERA ? 1 : (int)((st >> 9) & 15u); smp.c2 = CAMERA ? 2 : (int)((st >> 13) & 15u);
      int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
      smp.rng.inc = ((pixel_index * (unsigned long long)ps.spp + s + (1ull << 32)) << 1u) | 1ull;
      smp.rng.state = (unsigned long long)s4.z | ((unsigned long long)s4.w << 32);
      if (CAMERA || ((FRESH & 2) && RT_FRESH_ST(ps))) smp.rng.state = (smp.rng.inc + 0x853c49e6748fea9bULL) * 0x5851f42d4c957f2dULL + smp.rng.inc;  // Pcg32::set_sequence (rng.rs:46-52) of the sample's keyed stream, as k_raygen leaves it
      int prim = __float_as_int(h4.y);
      const bool found = prim >= 0;
      // the frame loop's hit record is (b2, prim, b0, b1): the three barycentrics of the accepted test
      SurfaceInteraction si; TriHit th; th.t = 0.0f; th.b0 = h4.z; th.b1 = h4.w; th.b2 = h4.x;
      if (found) {
        if (GENERAL && sc.n_instances != 0u && (unsigned)prim >= sc.n_top_prims) {  // a hit inside an object instance: from here on `prim` is the object's primitive
          const float4 o4 = in_o[rslot];
          prim = sc.obj_general ? instance_fill_interaction<true>(gsc, (unsigned)prim, o4.x, o4.y, o4.z, ray_d.x, ray_d.y, ray_d.z, th.b0, th.b1, th.b2, si)
                                : instance_fill_interaction<false>(gsc, (unsigned)prim, o4.x, o4.y, o4.z, ray_d.x, ray_d.y, ray_d.z, th.b0, th.b1, th.b2, si);
        }
        else if (GENERAL && (tri_flags(sc.tri_p, prim) & RT_FLAG_SPHERE)) {  // Sphere::intersect builds its interaction from the ray: origin and direction of the path's ray
          const float4 o4 = in_o[rslot];
          (void)sphere_fill_interaction(sc.spheres[prim_sphere_index(sc.tri_p, prim)], mk3(o4.x, o4.y, o4.z), ray_d, si);
          si.ssb = normalize(si.sh_dpdu);
          si.prim = prim;
        }
        else if (MODE != 0) tri_fill_interaction_inl<MODE == 1 || MODE == 3>(sc, prim, ray_d, th, si);
        else tri_fill_interaction(gsc, prim, ray_d, th, si);
      }
      RT_STAMP(0);  // path state loads + SurfaceInteraction
      // path.rs:127-136 emitted light at the vertex / from the environment
      if (SPLIT != RT_SPLIT_BOUNCED && (bounces == 0 || specular_bounce)) {  // (k_shade_split<2>: bounces >= 1 and no specular lobe in the scene - never true)
        if (found) {
          int li = rec_light(sc.tri_rec, prim);
          // The path's radiance so far is not this kernel's business (round 4): it only adds what the vertex emits towards the path, where there is something to
          // add (rare), as a read-modify-write of lacc[pid] right here. The reference's order of a path's terms is kept: this one reaches lacc before the bounce's
          // direct-light terms (any-hit epilogue, k_resolve), after the previous bounce's.
          if (li >= 0) { const float4 l4 = ps.lacc[pid]; const rgb3 L = mkc(l4.x, l4.y, l4.z) + beta * area_light_l(sc.lights[li], si.hit.n, -ray_d); ps.lacc[pid] = make_float4(L.r, L.g, L.b, l4.w); }
        } else if ((MODE != 1 && !LEAN) && sc.n_infinite > 0) {
          const float4 l4 = ps.lacc[pid]; rgb3 L = mkc(l4.x, l4.y, l4.z);
          for (int k = 0; k < sc.n_infinite; ++k) L = L + beta * infinite_le<BOUNCED>(sc, sc.lights[k == 0 ? sc.infinite_ids[0] : (k == 1 ? sc.infinite_ids[1] : (k == 2 ? sc.infinite_ids[2] : sc.infinite_ids[3]))], ray_d);  // constant indices: the kernel argument stays in SGPRs
          ps.lacc[pid] = make_float4(L.r, L.g, L.b, l4.w);
        }
      }
      if (found && bounces < fp.max_depth) {  // path.rs:139
        if ((MODE != 1 && !LEAN && !BOUNCED) && bounces == 0 && sc.needs_differentials && !RT_DBG(sc, 16)) {  // only the camera ray carries differentials (interaction.rs:245-314)
          if constexpr (RAYDIFF) {  // k_shade_rays: the differentials the caller's record of this ray carries (floats 8 - 19: rx_o, ry_o, rx_d, ry_d), used as given
            int rx_, ry_; unsigned long long rpix; owned_pixel(fp, fp.chunk_first + pix, rx_, ry_, rpix);
            const float4* r = rdiff.rays + (size_t)((rpix * rdiff.ray_ns + (s - rdiff.ray_s0)) * rdiff.rec4) + 2;
            const float4 r0 = r[0], r1 = r[1], r2 = r[2];
            const f3 rx_o = mk3(r0.x, r0.y, r0.z), ry_o = mk3(r0.w, r1.x, r1.y), rx_d = mk3(r1.z, r1.w, r2.x), ry_d = mk3(r2.y, r2.z, r2.w);
            if (MODE == 0) compute_differential_call(si, rx_o, ry_o, rx_d, ry_d); else compute_differential(si, rx_o, ry_o, rx_d, ry_d);
          } else {
          f2 pf; { float2 t = pfilm_[pid]; pf = mk2(t.x, t.y); }
          const f2 pl = fp.lens_radius > 0.0f ? table_2d(smp.tb, pix, 1, s) : mk2(0.0f, 0.0f);
          CameraRay cr = generate_camera_ray(fp, pf, pl, 1.0f / sqrtf((float)ps.spp));
          if (MODE == 0) compute_differential_call(si, cr.rx_o, cr.ry_o, cr.rx_d, cr.ry_d); else compute_differential(si, cr.rx_o, cr.ry_o, cr.rx_d, cr.ry_d);
          }
        }
        typename std::conditional<MODE == 1, SingleLambert, typename std::conditional<MODE == 3, SingleLambertT<!LEAN, BOUNCED>,
                                  typename std::conditional<MODE == 5, SmallBsdfT<false, LEAN>, typename std::conditional<MODE == 6, SmallBsdfT<true, LEAN>, GenericBsdf>::type>::type>::type>::type bsdf;
        RT_STAMP(1);  // emission + differentials
        if (MODE == 0) bsdf.build(gsc, rec_material(sc.tri_rec, prim), si); else bsdf.build(sc, rec_material(sc.tri_rec, prim), si);
        RT_STAMP(2);  // material: textures + lobes
        // light_distribution.lookup(p) (path.rs:154-158)
        const float* ld_func; const float* ld_cdf; float ld_int; long ld_row = 0;
        float4 ld_r0 = make_float4(0, 0, 0, 0), ld_r1 = ld_r0;  // (DScene::ld_rows8: the voxel's whole distribution, scenes of <= 3 lights)
        const bool rows8 = sc.ld_rows8 != nullptr;
        if (sc.ld_uniform) { ld_func = sc.ld_func; ld_cdf = sc.ld_cdf; if (rows8) { ld_r0 = sc.ld_rows8[0]; ld_r1 = sc.ld_rows8[1]; ld_int = ld_r0.x; } else ld_int = sc.ld_int[0]; }
        else if (sc.ld_dense8 != nullptr) {  // (<= 3 lights, a grid of moderate size: the voxel's record directly, two loads in flight together and no slot before them)
          const long v = voxel_of(sc, si.hit.p);
          ld_r0 = sc.ld_dense8[2 * v]; ld_r1 = sc.ld_dense8[2 * v + 1]; ld_int = ld_r0.x; ld_func = sc.ld_func; ld_cdf = sc.ld_cdf;
        }
        else {
          const long slot = sc.ld_slot[voxel_of(sc, si.hit.p)];
          if (slot >= 0) {
            ld_func = sc.ld_func + slot * sc.n_lights; ld_cdf = sc.ld_cdf + slot * (sc.n_lights + 1); ld_row = slot;
            if (rows8) { ld_r0 = sc.ld_rows8[2 * slot]; ld_r1 = sc.ld_rows8[2 * slot + 1]; ld_int = ld_r0.x; } else ld_int = sc.ld_int[slot];
          }
          else { ld_func = sc.ld_func; ld_cdf = sc.ld_cdf; ld_int = -1.0f; }
        }
        const unsigned nonspec = BSDF_ALL & ~BSDF_SPECULAR;
        // voxels are built eagerly for every cell a surface point can fall into (k_lightdist_mark); the rest carry -1.
        // Looking one up would mean the marking missed a cell: count it (rt_render then fails the frame) and skip.
        const bool voxel_ok = !(ld_int < 0.0f);
        if (!voxel_ok) atomicAdd(&ps.stats[ST_UNBUILT_VOXEL], 1ull);
        if (voxel_ok && bsdf.num_nonspecular() > 0 && sc.n_lights > 0) {  // uniform_sample_one_light, integrator/mod.rs:186-220
          float su = smp.get_1d();
          int light_num; float light_pdf;
          if (RT_DBG(sc, 128)) { light_num = clampi((int)(su * (float)sc.n_lights), 0, sc.n_lights - 1); light_pdf = 1.0f / (float)sc.n_lights; }  // (measurement builds: no row search)
          else if (rows8) d1_sample_discrete_row8(ld_r0, ld_r1, sc.n_lights, su, light_num, light_pdf);
          else if (MODE != 1 && sc.ld_glog >= 0) d1_sample_discrete_guided(ld_func, ld_cdf, ld_int, sc.n_lights, su, sc.ld_guide + ld_row * ((1 << sc.ld_glog) + 1), sc.ld_glog, light_num, light_pdf);
          else d1_sample_discrete(ld_func, ld_cdf, ld_int, sc.n_lights, su, light_num, light_pdf);
          // Shadow sets (rtx_shadow_sets.h): the spare word of the voxel's record for the picked light (two lights) says EMPTY when no segment from
          // this voxel to the light can be occluded - the segment is then not cast and its answer, "unoccluded", is applied below as the any-hit kernel would apply it
          // (the constant-Kd Lambert front-end only, the one the scenes of two area lights in LDS reach most: the other forms keep their register budgets)
          const bool ld_empty = MODE == 1 && ps.shadow_sets && RT_SHADOW_KIND(__float_as_uint(light_num == 0 ? ld_r0.w : ld_r1.w)) == RT_SHADOW_EMPTY;
          RT_STAMP(3);  // light pick: voxel row + discrete search
          if (light_pdf != 0.0f) {
            f2 u_light = smp.get_2d();
            f2 u_scattering = smp.get_2d();
            const DLight& light = sc.lights[RT_DBG(sc, 256) ? 0 : light_num];  // (measurement builds, 256: one light's record for every lane - no gather)
            // ---- estimate_direct (integrator/mod.rs:222-318), light-sampling half
            rgb3 ld1 = mkc(0, 0, 0); f3 sh_dir = mk3(0, 0, 0);
            const bool q_light = QLIGHTS && (tri_flags(sc.tri_p, light.prim) & RT_FLAG_SPHERE) != 0u;  // the picked light sits on a sphere
            f3 q_center = mk3(0, 0, 0);
            LiSample ls;
            if (q_light) {  // DiffuseAreaLight::sample_li (diffuse.rs:59-70) over the cone branch of Sphere::sample_si, as light_sample_li_inl<true> assembles it
              const DSphere& sp = sc.spheres[prim_sphere_index(sc.tri_p, light.prim)];
              q_center = xf34_point(sp.o2w, mk3(0, 0, 0));
              float pdf; const SpherePoint pt = sphere_cone_sample_si(sp, q_center, si.hit, u_light, pdf);
              ls.p1.p = pt.p; ls.p1.p_error = pt.p_error; ls.p1.n = pt.n;
              ls.wi = normalize(pt.p - si.hit.p); ls.pdf = pdf; ls.li = area_light_l(light, pt.n, -ls.wi);
            } else ls = (MODE == 1 || LEAN) ? area_light_sample_li(sc, light, si.hit, u_light) : light_sample_li_full<GENERAL, false, BOUNCED>(gsc, light, si.hit, u_light);
            if (ls.pdf > 0.0f && !is_black(ls.li)) {
              rgb3 f = bsdf.f(si.hit.wo, ls.wi, nonspec) * fabsf(dot(ls.wi, si.sh_n));
              float scattering_pdf = ((MODE != 1 && !LEAN) && light_is_delta(light)) ? 0.0f : bsdf.pdf(si.hit.wo, ls.wi, nonspec);  // read by the power heuristic only: a delta light has none
              if (!is_black(f)) {
                Ray sr = spawn_ray_to_interaction(si.hit, ls.p1);  // VisibilityTester, light/mod.rs:52-55
                if (!ld_empty) sh_o[i] = make_float4(sr.o.x, sr.o.y, sr.o.z, sr.t_max);  // (shadow and MIS records sit at the vertex's position in THIS launch's queue, see PassState::sh)
                sh_dir = sr.d;
                want_shadow = true;
                if (light_is_delta(light)) ld1 = vdiv(f * ls.li, ls.pdf);
                else ld1 = vdiv(f * ls.li * power_heuristic1(ls.pdf, scattering_pdf), ls.pdf);
              }
            }
            RT_STAMP(4);  // light-sampling half: sample_li, f, pdf, shadow ray
            // ---- BSDF-sampling half
            rgb3 f2v = mkc(0, 0, 0); float w2 = 0.0f, spdf2 = 1.0f;
            if (!light_is_delta(light) && !RT_DBG(sc, 8)) {
              LobeSample bs = bsdf.sample_f(si.hit.wo, u_scattering, nonspec);
              rgb3 f = bs.f * fabsf(dot(bs.wi, si.sh_n));
              if (!is_black(f) && bs.pdf > 0.0f) {
                float weight = 1.0f; bool go = true;
                if (!(bs.type & BSDF_SPECULAR)) {
                  float lp;
                  if (q_light) lp = sphere_cone_pdf_wi(sc.spheres[prim_sphere_index(sc.tri_p, light.prim)], q_center, si.hit);
                  else if (RT_DBG(sc, 512)) lp = 1.0f;  // (measurement builds: no re-intersection of the emitter)
                  else lp = (MODE == 1 || LEAN) ? area_light_pdf_li<false>(sc, light, si.hit, bs.wi) : light_pdf_li<GENERAL, BOUNCED>(gsc, light, si.hit, bs.wi);
                  if (lp == 0.0f) go = false;  // `return ld`
                  else weight = power_heuristic1(bs.pdf, lp);
                  if ((GENERAL || QLIGHTS) && go && ps.skip_unreachable_mis && light.kind == 0 && (tri_flags(sc.tri_p, light.prim) & RT_FLAG_SPHERE)) {
                    const float4 b0 = sc.tri_p[3 * (size_t)light.prim], b1 = sc.tri_p[3 * (size_t)light.prim + 1];  // a quadric's leaf record: its world box
                    if (!ray_may_reach_box(mk3(b0.x, b0.y, b0.z), mk3(b1.x, b1.y, b1.z), si.hit.p, bs.wi)) { go = false; n_unreached += 1u; }
                  }
                }
                if (go) {
                  Ray mr = spawn_ray(si.hit, bs.wi);
                  mi_o[i] = make_float4(mr.o.x, mr.o.y, mr.o.z, kInf);
                  mi_d[i] = make_float4(mr.d.x, mr.d.y, mr.d.z, __uint_as_float(pid));  // the path the record belongs to
                  want_mis = true; f2v = f; w2 = weight; spdf2 = bs.pdf;
                  // An infinite light is never the emitter a ray hits (integrator/mod.rs:291-309): the term is `Le(ray)` if the ray leaves the
                  // scene and nothing otherwise, so occlusion is all this ray has to report.
                  mis_occlusion_only = (MODE != 1 && !LEAN) && ps.mis_any && light.kind == 3;
                }
              }
            }
            no_walk = want_shadow && ld_empty;
            if (want_mis) {  // both halves are combined by k_resolve once both rays are back
              mi_a[i] = make_float4(ld1.r, ld1.g, ld1.b, light_pdf);
              mi_b[i] = make_float4(f2v.r, f2v.g, f2v.b, w2);
              mi_c[i] = make_float4(beta.r, beta.g, beta.b, spdf2);
              mi_flags[i] = (want_shadow ? RT_PEND_SHADOW : 0u) | 2u | ((unsigned)light_num << 2) | (mis_occlusion_only ? RT_PEND_MIS_ANY : 0u);
              if (!want_shadow || no_walk) ps.occ_sh[i] = no_walk ? (unsigned char)0 : (unsigned char)1;  // no light-sampling term: as good as blocked (the any-hit kernel writes the byte of every other vertex)
            } else if (want_shadow) {  // L += beta * ((0 + Ld1) / pick_pdf) if unoccluded, applied by the any-hit kernel (trace_write_any) - or here, with the same sum
              rgb3 add = beta * vdiv(mkc(0, 0, 0) + ld1, light_pdf);
              if (no_walk) { const float4 l4 = ps.lacc[pid]; ps.lacc[pid] = make_float4(l4.x + add.r, l4.y + add.g, l4.z + add.b, l4.w); }
              else sh_add[i] = make_float4(add.r, add.g, add.b, 0.0f);
            }
            if (want_shadow && !no_walk) sh_d[i] = make_float4(sh_dir.x, sh_dir.y, sh_dir.z, __uint_as_float((want_mis ? 0u : 0x80000000u) | pid));  // bit 31: complete here (no MIS ray), bits 0-30: the path
            want_shadow = want_shadow && !no_walk;  // (from here on: a record in the shadow queue)
          }
        }
        RT_STAMP(5);  // BSDF-sampling half + records
        // ---- sample the BSDF for the next direction (path.rs:172-196)
        f3 wo = -ray_d;  // not normalised (reference quirk)
        LobeSample bs = bsdf.sample_f(wo, smp.get_2d(), BSDF_ALL);
        if (!(is_black(bs.f) || bs.pdf <= 0.0f)) {
          beta = vdiv(beta * bs.f * fabsf(dot(bs.wi, si.sh_n)), bs.pdf);
          specular_bounce = (bs.type & BSDF_SPECULAR) != 0u;
          if ((bs.type & BSDF_SPECULAR) && (bs.type & BSDF_TRANSMISSION)) {
            float eta = bsdf.eta();
            eta_scale *= dot(wo, si.hit.n) > 0.0f ? eta * eta : vdiv(1.0f, eta * eta);
          }
          cont = true;
          rgb3 rr_beta = beta * eta_scale;  // path.rs:201-209
          if (!CAMERA && max_component_value(rr_beta) < fp.rr_threshold && bounces > 3) {
            float q = fmaxf(1.0f - max_component_value(rr_beta), 0.05f);
            if (smp.get_1d() < q) cont = false;
            else beta = vdiv(beta, 1.0f - q);
          }
          if (cont) bounces += 1;
          // the next iteration would trace this ray, add what it reaches only after a specular bounce, and leave at bounces >= max_depth (path.rs:127-139)
          if (cont && ps.skip_dead_tail && bounces >= fp.max_depth && !specular_bounce) { cont = false; tail = true; }
          if (cont) { const Ray nr = spawn_ray(si.hit, bs.wi); nr_o = nr.o; nr_d = nr.d; }
        }
      }
      st_out = pack_state(bounces, specular_bounce, smp.c1, smp.c2); rng_out = smp.rng.state;
    }
    RT_STAMP(6);  // continuation sample, spawn, state stores
    // (a wave-uniform count, kept in a scalar register: a per-lane counter is one more live vector register in every form, and an atomic where the paths end
    // is ~7 M atomics on one word in the launch at the depth limit - k_shade<1> 271 -> 329 ms per S1 frame, measured)
    n_tail += (unsigned)__popcll(__ballot(tail));
    n_no_walk += (unsigned)__popcll(__ballot(no_walk));
    constexpr int NQ = (MODE == 1 || LEAN) ? 3 : 4;  // area lights only: every MIS ray needs its closest hit
    const int ci[4] = {0, 1, 2, 3}; const bool pr[4] = {cont, want_shadow, want_mis && !mis_occlusion_only, want_mis && mis_occlusion_only}; unsigned slot[4];
    block_push<NQ>(ps.cnt_out, ps.shard_cap, ci, pr, slot);
    if (cont) {  // the path's records for the next bounce, at its slot of that bounce's queue: a wave's stores are runs of consecutive slots
      out_o[slot[0]] = make_float4(nr_o.x, nr_o.y, nr_o.z, kInf);
      out_d[slot[0]] = make_float4(nr_d.x, nr_d.y, nr_d.z, 0.0f);
      out_beta[slot[0]] = make_float4(beta.r, beta.g, beta.b, eta_scale);
      out_st[slot[0]] = make_uint4(st_out, pid, (unsigned)rng_out, (unsigned)(rng_out >> 32));
    }
    if (want_shadow) ps.q_shadow[slot[1]] = i;  // the ray queues name RECORDS (= this launch's queue positions)
    if (pr[2]) ps.q_mis[slot[2]] = i;
    if (NQ == 4 && pr[3]) ps.q_misany[slot[3]] = i;
  };
  // slot = entry i of the sharded queue by the shard counts alone; on a material-sorted queue the sorted list names the slot
  if (MODE != 1) {
    for (unsigned base = first + blockIdx.x * blockDim.x; base < count; base += stride) {
      const unsigned i = base + threadIdx.x;
      const bool lane_live = i < count;
      n_shaded += lane_live ? 1u : 0u;
      shade_vertex(lane_live, i, lane_live ? (ps.cnt_in ? qv.get(i) : i) : 0u);
    }
  } else if constexpr (SPLIT != RT_SPLIT_NONE) {
    // The compaction below, fed by the mask words k_trace left (TraceIO::hit_mask: bit e & 63 of word e >> 6 = entry e found a hit; bits past the queue's end are zero)
    // instead of the hit records. An iteration's 256 entries are four consecutive words, the first a multiple of four; every wave reads all four with wave-uniform
    // loads - words at or past ceil(count / 64) were never written and count as zero - and has `before` and `total` from their popcounts: no load per entry, no exchange
    // through LDS and no barrier in front of the ring appends. Workgroups of 256 lanes (rtx_launch_shade_split).
    __shared__ unsigned s_ring_slot[512], s_ring_i[512];
    unsigned head = 0, n_pend = 0;  // (workgroup-uniform)
    const unsigned lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned n_words = (count + 63u) >> 6;
    for (unsigned base = blockIdx.x * 256u; base < count; base += stride) {
      const unsigned i = base + threadIdx.x;
      { const unsigned wb = base + 64u * wv; n_shaded += wb < count ? (count - wb < 64u ? count - wb : 64u) : 0u; }  // (the WAVE's entries, a scalar: a per-lane count is a vector register live through every vertex - 7 / 6 spilled dwords instead of 3 / 4)
      const unsigned w0 = base >> 6;
      unsigned before = 0, total = 0; unsigned long long m = 0ull;
      // (KARGS, measured on the allocation and not kept: hit_mask re-read here like the other arguments - the pointer is then no longer __restrict__ and the four
      // mask words become vector loads: k_shade_split<1> / <2> 49 / 66 more VALU instructions, 0 / 3 fewer spilled scalars, nothing else moves)
#pragma unroll
      for (unsigned w = 0; w < 4u; ++w) {
        const unsigned long long mw = w0 + w < n_words ? hit_mask[w0 + w] : 0ull;
        const unsigned c = (unsigned)__popcll(mw);
        before += w < wv ? c : 0u; total += c; m = w == wv ? mw : m;
      }
      if ((m >> lane) & 1ull) {
        const unsigned pos = (head + n_pend + before + (unsigned)__popcll(m & ((1ull << lane) - 1ull))) & 511u;
        if (!CAMERA) s_ring_slot[pos] = ps.cnt_in ? qv.get(i) : i;
        s_ring_i[pos] = i;
      }
      n_pend += total;
      __syncthreads();  // (the appends before the ring is read; the previous round's reads are behind shade_vertex's own barriers)
      if (n_pend >= 256u) {
        const unsigned pos = (head + threadIdx.x) & 511u;
        if (CAMERA) { const unsigned e = s_ring_i[pos]; shade_vertex(true, e, e); }  // (entry = slot: one ring)
        else shade_vertex(true, s_ring_i[pos], s_ring_slot[pos]);
        head = (head + 256u) & 511u; n_pend -= 256u;
      }
    }
    if (n_pend > 0u) {
      const unsigned pos = (head + threadIdx.x) & 511u;
      const bool lv = threadIdx.x < n_pend;
      if (CAMERA) { const unsigned e = lv ? s_ring_i[pos] : 0u; shade_vertex(lv, e, e); }
      else shade_vertex(lv, lv ? s_ring_i[pos] : 0u, lv ? s_ring_slot[pos] : 0u);
    }
  } else {
    // MODE 1 (area lights only: a ray that left the scene adds nothing and ends its path): the workgroup COMPACTS its entries before it shades them. A fifth of
    // S1's vertices are such misses (the box is open towards the camera) and their lanes sat through the ~4000 instructions of the others: 44 of 64 lanes per
    // VALU instruction. Each iteration the 256 threads look at the hit records of 256 entries, append the (entry, slot) pairs of the hits to a ring in LDS, and
    // whenever the ring holds 256 of them a full workgroup of vertices is shaded; the remainder at the end. Which lane shades a vertex is irrelevant (paths are
    // independent; a vertex's shadow / MIS records sit at its own entry number whoever writes them): same film, same counters.
    __shared__ unsigned s_ring_slot[512], s_ring_i[512], s_wave_hits[4];
    unsigned head = 0, n_pend = 0;  // (workgroup-uniform)
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (unsigned base = first + blockIdx.x * blockDim.x; base < count; base += stride) {
      const unsigned i = base + threadIdx.x;
      const bool lane_live = i < count;
      n_shaded += lane_live ? 1u : 0u;
      const unsigned rslot = lane_live ? (ps.cnt_in ? qv.get(i) : i) : 0u;
      const int hprim = lane_live ? __float_as_int(sraw(ps.hit)[rslot].y) : -1;
      const bool hit = hprim >= 0;
      const unsigned long long m = __ballot(hit);
      if (lane == 0u) s_wave_hits[wv] = (unsigned)__popcll(m);
      __syncthreads();
      unsigned before = 0, total = 0;
#pragma unroll
      for (unsigned w = 0; w < 4u; ++w) { const unsigned c = w < (blockDim.x >> 6) ? s_wave_hits[w] : 0u; before += w < wv ? c : 0u; total += c; }
      if (hit) { const unsigned pos = (head + n_pend + before + (unsigned)__popcll(m & ((1ull << lane) - 1ull))) & 511u; s_ring_slot[pos] = rslot; s_ring_i[pos] = i; }
      n_pend += total;
      __syncthreads();
      if (n_pend >= blockDim.x) {
        const unsigned pos = (head + threadIdx.x) & 511u;
        shade_vertex(true, s_ring_i[pos], s_ring_slot[pos]);
        head = (head + blockDim.x) & 511u; n_pend -= blockDim.x;
      }
    }
    if (n_pend > 0u) {
      const unsigned pos = (head + threadIdx.x) & 511u;
      const bool lv = threadIdx.x < n_pend;
      shade_vertex(lv, lv ? s_ring_i[pos] : 0u, lv ? s_ring_slot[pos] : 0u);
    }
  }
  if (GENERAL || QLIGHTS) {
    for (int off = 32; off > 0; off >>= 1) n_unreached += __shfl_down(n_unreached, off);
    if ((threadIdx.x & 63u) == 0u && n_unreached) atomicAdd(&ps.stats[ST_MIS_UNREACHED], (unsigned long long)n_unreached);
  }
  if ((threadIdx.x & 63u) == 0u && n_tail) atomicAdd(&ps.stats[ST_TAIL_UNCAST], (unsigned long long)n_tail);  // (the wave's count, the same in every lane)
  if ((threadIdx.x & 63u) == 0u && n_no_walk) atomicAdd(&ps.stats[ST_SHADOW_SETS], (unsigned long long)n_no_walk);
  if (SPLIT == RT_SPLIT_NONE) for (int off = 32; off > 0; off >>= 1) n_shaded += __shfl_down(n_shaded, off);  // (the split kernels hold the wave's count already)
  if ((threadIdx.x & 63u) == 0u && n_shaded) atomicAdd(&ps.stats[ST_SHADED + (MODE == 1 ? 0 : (MODE == 3 ? 1 : (MODE == 5 || MODE == 6 ? 2 : 3)))], (unsigned long long)n_shaded);
#ifdef RT_ABLATE
  if ((threadIdx.x & 63u) == 0u) for (int k = 0; k < 8; ++k) atomicAdd(&ps.stats[ST_STAMP + 8 * (MODE == 1 ? 0 : (MODE == 3 ? 1 : (MODE == 5 || MODE == 6 ? 2 : 3))) + k], stamp_acc[k]);
#endif
