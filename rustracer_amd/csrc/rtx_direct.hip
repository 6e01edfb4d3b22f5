// rtx_direct.hip - the direct-lighting integrator (rt_render_rays_direct, rt_render_direct: integrator/directlighting.rs:89-143, integrator/mod.rs:145-318). Its li is
// Whitted's tree walk - one NODE per camera sample and step, the pending stack, the state record (run_direct, rtx_hip.hip; rtx_whitted_dev.h) - with another estimator at
// each vertex: estimate_direct per light, a light sample and a BSDF sample combined by the power heuristic, the BSDF-sampled ray a closest-hit ray that counts only where
// it ends on THAT light. Under strategy "all" the samples of a vertex come from the sampler's 2-D ARRAYS, which ZeroTwoSequence::start_pixel generates from the pixel's
// stream after the 2 * dims tables: k_sampler_array_tables is that continuation, in its plain one-lane-per-pixel form.
// The two halves of estimate_direct stand here as estimate_light_half / estimate_bsdf_half, over the device functions the path kernels' statement calls (bsdf_f, bsdf_pdf,
// bsdf_sample_f, power_heuristic1, light_sample_li_full, light_pdf_li, spawn_ray*); rtx_shade_body.inl keeps its own interleaving of them with its front-ends' special
// cases, because no existing kernel's code object may change with this unit. A translation unit of its own, compiled beside the others.
#include <hip/hip_runtime.h>
#include "../../include/rtx_hip.h"
#include "rtx_shade_kernels.h"
#include "rtx_direct_launch.h"
#include "rtx_whitted_dev.h"

namespace rtx {

// ================================================================================ the array tables
// One lane per pixel of the batch. Seeds the pixel's stream as K0 does (pixel_index_of), walks the draws of the 2 * dims tables without storing anything - per table one
// (van_der_corput) or two (sobol_2d) scrambles, spp draws bounded(1), spp draws bounded(spp - i), every bounded draw with its retries (rng.rs:32-40) -, then writes the
// n_arrays array tables: sobol_2d(1, spp) each, so two scrambles and the Fisher-Yates shuffle of the sample order, replayed on a permutation staged in LDS
// ([lane][spp + 2] u16: an odd word stride, conflict-free) as k_sampler_tables does. In stream order: no dirty-pixel machinery.
static __global__ void k_sampler_array_tables(FrameParams fp, unsigned n_pixels, unsigned spp, unsigned dims, unsigned n_arrays, unsigned* __restrict__ scrambles,
                                              unsigned short* __restrict__ perms) {
  extern __shared__ unsigned short lds_perm[];
  const unsigned lane = threadIdx.x;
  unsigned short* const mine = lds_perm + (size_t)lane * (spp + 2u);
  const unsigned pix = blockIdx.x * blockDim.x + lane;
  if (pix >= n_pixels) return;
  Pcg32 rng; rng.set_sequence(pixel_index_of(fp, pix, 0ull, 0));
  for (unsigned t = 0; t < 2u * dims; ++t) {  // the tables K0 builds: their draws only
    (void)rng.next_u32();
    if (t >= dims) (void)rng.next_u32();
    for (unsigned i = 0; i < spp; ++i) (void)rng.bounded(1u);
    for (unsigned i = 0; i < spp; ++i) (void)rng.bounded(spp - i);
  }
  for (unsigned a = 0; a < n_arrays; ++a) {
    const unsigned s0 = rng.next_u32(), s1 = rng.next_u32();  // sobol_2d's scramble pair (lowdiscrepancy.rs:31)
    scrambles[(size_t)(2u * a) * n_pixels + pix] = s0;
    scrambles[(size_t)(2u * a + 1u) * n_pixels + pix] = s1;
    for (unsigned i = 0; i < spp; ++i) mine[i] = (unsigned short)i;
    for (unsigned i = 0; i < spp; ++i) (void)rng.bounded(1u);  // the per-pixel-sample shuffles of one element (:41-48)
    for (unsigned i = 0; i < spp; ++i) {                       // shuffle(samples, n_pixel_samples, 1) (:49, :114-124)
      const unsigned other = i + rng.bounded(spp - i);
      const unsigned short x = mine[i], y = mine[other];
      mine[i] = y; mine[other] = x;
    }
    unsigned short* const dst = perms + (size_t)a * spp * n_pixels + pix;
    for (unsigned i = 0; i < spp; ++i) dst[(size_t)i * n_pixels] = mine[i];
  }
}

// ================================================================================ estimate_direct (integrator/mod.rs:222-318), flags = ALL & !SPECULAR
#define RT_DIRECT_FLAGS (BSDF_ALL & ~BSDF_SPECULAR)
// Light half (:243-270): the visibility segment and the term it carries if it is clear - f li / pdf for a delta light, weighted by power_heuristic(1, pdf, 1, bsdf.pdf)
// for any other. ns: isect.shading.n after compute_scattering_functions.
template <bool GENERAL>
RT_DEV bool estimate_light_half(const DScene& gsc, const DLight& light, const SurfaceInteraction& si, const Bsdf& b, f3 ns, f2 u_light, Ray& segment, rgb3& ld) {
  const f3 wo = si.hit.wo;
  const LiSample ls = light_sample_li_full<GENERAL>(gsc, light, si.hit, u_light);
  if (!(ls.pdf > 0.0f) || is_black(ls.li)) return false;
  const rgb3 f = bsdf_f(b, wo, ls.wi, RT_DIRECT_FLAGS) * fabsf(dot(ls.wi, ns));
  if (is_black(f)) return false;
  segment = spawn_ray_to_interaction(si.hit, ls.p1);  // VisibilityTester, light/mod.rs:52-55
  if (light_is_delta(light)) ld = vdiv(f * ls.li, ls.pdf);
  else ld = vdiv(f * ls.li * power_heuristic1(ls.pdf, bsdf_pdf(b, wo, ls.wi, RT_DIRECT_FLAGS)), ls.pdf);
  return true;
}
// BSDF half (:272-315) of a non-delta light: the closest-hit ray and f |cos| weight / pdf, what the emitted radiance found at its end is multiplied by.
template <bool GENERAL>
RT_DEV bool estimate_bsdf_half(const DScene& gsc, const DLight& light, const SurfaceInteraction& si, const Bsdf& b, f3 ns, f2 u_scattering, Ray& probe, rgb3& term) {
  const LobeSample bs = bsdf_sample_f(b, si.hit.wo, u_scattering, RT_DIRECT_FLAGS);
  const rgb3 f = bs.f * fabsf(dot(bs.wi, ns));
  if (is_black(f) || !(bs.pdf > 0.0f)) return false;
  float weight = 1.0f;
  if (!(bs.type & BSDF_SPECULAR)) {
    const float lp = light_pdf_li<GENERAL>(gsc, light, si.hit, bs.wi);
    if (lp == 0.0f) return false;  // `return ld`
    weight = power_heuristic1(bs.pdf, lp);
  }
  probe = spawn_ray(si.hit, bs.wi);
  term = vdiv(f * weight, bs.pdf);
  return true;
}

// ================================================================================ the vertex kernel
// k_whitted_vertex's lane, queue, state record, pending stack and block_push (rtx_whitted.hip), with three queues: continuing samples, shadow records, probe records.
// Per-sample counters in wst[path]: k2 get_2d() draws, li invocations, k1 get_1d() draws, v vertices that reached uniform_sample_all_light.
// A light round writes the shadow record of ENTRY i exactly as Whitted's, and for a non-delta light the probe record of entry i: mi.o = (o | inf), mi.d = (d | path id),
// mi.a = (beta f |cos| weight / pdf [/ pick pdf] | light index).
// Everything that decides where a ray goes is IEEE; the radiance-only quotients are vdiv, as in Whitted. GENERAL: quadric or instance hits, quadric or masked emitters.
template <bool GENERAL>
__global__ void __launch_bounds__(256, RT_SHADE0_MIN_WAVES) k_direct_vertex(DScene sc, FrameParams fp, PassState ps, DirectArgs a) {
  QView qv; if (ps.cnt_in) qv.init(nullptr, ps.cnt_in, ps.shard_cap);
  const unsigned count = ps.cnt_in ? qv.total() : ps.cap, stride = gridDim.x * 256u;
  const DScene& gsc = *sc.self;  // what out-of-line functions get: the scene record in device memory
  const Tables tb = tables_of(ps);
  const bool last = a.round + 1u == a.n_rounds;
  const bool one = a.strategy == RT_DIRECT_ONE;
  const int light_rounds = one ? (a.n_lights > 0 ? 1 : 0) : a.n_lights;
  for (unsigned base = blockIdx.x * 256u; base < count; base += stride) {  // (uniform per workgroup: block_push holds barriers)
    const unsigned i = base + threadIdx.x;
    bool cont = false, want_shadow = false, want_probe = false;
    f3 nr_o = mk3(0, 0, 0), nr_d = mk3(0, 0, 0); rgb3 nbeta = mkc(0, 0, 0); unsigned nst = 0u, pid = 0u; unsigned long long rng_out = 0ull;
    if (i < count) {
      const unsigned slot = ps.cnt_in ? qv.get(i) : i;
      const float4 o4 = sraw(ps.in.o)[slot], d4 = sraw(ps.in.d)[slot], b4 = sraw(ps.in.beta)[slot];
      float4 h4 = sraw(ps.hit)[slot];
      uint4 st = sraw(ps.in.st)[slot];
      pid = st.y;
      f3 ray_o = mk3(o4.x, o4.y, o4.z), ray_d = mk3(d4.x, d4.y, d4.z);
      rgb3 beta = a.step == 0u ? mkc(1.0f, 1.0f, 1.0f) : mkc(b4.x, b4.y, b4.z);
      int depth = a.step == 0u ? 0 : (int)(st.x & 31u);
      unsigned pending = a.step == 0u ? 0u : (st.x >> 8) & 0xffffu;
      const uint4 w4 = a.step == 0u ? make_uint4(0u, 0u, 0u, 0u) : a.wst[pid];
      unsigned k2 = w4.x, k1 = w4.z, v = w4.w;  // what the sample has consumed before this node
      unsigned sl, pix; split_path_id(ps, pid, sl, pix); const unsigned s = ps.s0 + sl;
      int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
      WhittedDraws dr; dr.tb = tb; dr.pix = pix; dr.s = s; dr.rng_used = false;
      dr.rng.state = (unsigned long long)st.z | ((unsigned long long)st.w << 32);
      dr.rng.inc = ((pixel_index * (unsigned long long)ps.spp + s + (1ull << 32)) << 1u) | 1ull;  // set_sequence of the keyed per-sample stream (k_raygen)
      bool have_vertex = __float_as_int(h4.y) >= 0;
      bool fresh = true;  // the node the step traced (Le, its lights, its reflection); false: a popped vertex (its transmission only)
      if (!have_vertex && a.round == 0u && sc.n_infinite > 0) {  // a miss: the sum of the lights' le(ray) - only an infinite light has one (light/mod.rs:30-32)
        const float4 l4 = ps.lacc[pid]; rgb3 L = mkc(l4.x, l4.y, l4.z);
        for (int q = 0; q < sc.n_infinite; ++q) L = L + beta * infinite_le(sc, sc.lights[q == 0 ? sc.infinite_ids[0] : (q == 1 ? sc.infinite_ids[1] : (q == 2 ? sc.infinite_ids[2] : sc.infinite_ids[3]))], ray_d);
        ps.lacc[pid] = make_float4(L.r, L.g, L.b, l4.w);
      }
      for (;;) {
        if (have_vertex) {
          SurfaceInteraction si;
          const int prim = whitted_interaction<GENERAL>(sc, gsc, fp, ps, a.rdiff, tb, pix, s, pid, pixel_index, depth, ray_o, ray_d, h4, si);
          const f3 wo = si.hit.wo;
          Bsdf b;
          build_bsdf<false>(gsc, rec_material(sc.tri_rec, prim), si, b);
          const f3 ns = si.sh_n;  // isect.shading.n AFTER compute_scattering_functions: estimate_direct's cosine and the recursion's (a bump map has moved it)
          if (fresh && a.round == 0u) {  // colour += isect.le(wo)
            const int li = rec_light(sc.tri_rec, prim);
            if (li >= 0) { const float4 l4 = ps.lacc[pid]; const rgb3 L = mkc(l4.x, l4.y, l4.z) + beta * area_light_l(sc.lights[li], si.hit.n, wo); ps.lacc[pid] = make_float4(L.r, L.g, L.b, l4.w); }
          }
          if (fresh && (int)a.round < light_rounds) {
            int light_num = (int)a.round; float pick_pdf = 1.0f; f2 u_light, u_scattering;
            if (one) {  // uniform_sample_one_light(.., None), mod.rs:186-220
              const float s1 = dr.get_1d(k1);
              light_num = min(a.n_lights - 1, (int)(s1 * (float)a.n_lights));
              pick_pdf = 1.0f / (float)a.n_lights;
              u_light = dr.get(k2); u_scattering = dr.get(k2 + 1u);
            } else if (v < (unsigned)a.max_depth) {  // uniform_sample_all_light, mod.rs:145-184: the vertex's arrays, at the sample's index
              const unsigned t = 2u * (v * (unsigned)a.n_lights + a.round);
              u_light = table_2d(a.arr, pix, t, s); u_scattering = table_2d(a.arr, pix, t + 1u, s);
            } else {  // get_2d_array found the arrays exhausted: two plain draws per light
              u_light = dr.get(k2 + 2u * a.round); u_scattering = dr.get(k2 + 2u * a.round + 1u);
            }
            const DLight& light = sc.lights[light_num];
            Ray sr; rgb3 ld;
            if (estimate_light_half<GENERAL>(gsc, light, si, b, ns, u_light, sr, ld)) {
              const rgb3 add = beta * (one ? vdiv(ld, pick_pdf) : ld);
              sraw(ps.sh.o)[i] = make_float4(sr.o.x, sr.o.y, sr.o.z, sr.t_max);
              sraw(ps.sh.d)[i] = make_float4(sr.d.x, sr.d.y, sr.d.z, __uint_as_float(0x80000000u | pid));  // bit 31: the any-hit epilogue adds a clear record's term
              sraw(ps.sh.add)[i] = make_float4(add.r, add.g, add.b, 0.0f);
              want_shadow = true;
            }
            Ray pr; rgb3 term;
            if (!light_is_delta(light) && estimate_bsdf_half<GENERAL>(gsc, light, si, b, ns, u_scattering, pr, term)) {
              const rgb3 t3 = beta * (one ? vdiv(term, pick_pdf) : term);
              sraw(ps.mi.o)[i] = make_float4(pr.o.x, pr.o.y, pr.o.z, kInf);
              sraw(ps.mi.d)[i] = make_float4(pr.d.x, pr.d.y, pr.d.z, __uint_as_float(pid));
              sraw(ps.mi.a)[i] = make_float4(t3.r, t3.g, t3.b, __int_as_float(light_num));
              want_probe = true;
            }
          }
          if (!last) break;
          if (fresh && a.n_lights > 0) {
            if (one) { k1 += 1u; k2 += 2u; }
            else { if (v >= (unsigned)a.max_depth) k2 += 2u * (unsigned)a.n_lights; v += 1u; }
          }
          if (depth + 1 < a.max_depth) {  // directlighting.rs:126-131
            if (fresh) {  // specular_reflection (mod.rs:49-89): the draw is consumed whether or not a lobe matches
              const LobeSample bs = bsdf_sample_f(b, wo, dr.get(k2), BSDF_SPECULAR | BSDF_REFLECTION); k2 += 1u;
              const float c = fabsf(dot(bs.wi, ns));
              if (bs.pdf > 0.0f && !is_black(bs.f) && c != 0.0f) {
                // the vertex waits at its level for its transmission draw: (o | b2), (d | prim), (b0, b1), (beta)
                float4* const e = a.stack + (size_t)depth * a.stack_cap + pid; const size_t plane = (size_t)a.levels * a.stack_cap;
                e[0] = make_float4(ray_o.x, ray_o.y, ray_o.z, h4.x); e[plane] = make_float4(ray_d.x, ray_d.y, ray_d.z, h4.y);
                e[2 * plane] = make_float4(h4.z, h4.w, 0.0f, 0.0f); e[3 * plane] = make_float4(beta.r, beta.g, beta.b, 0.0f);
                pending |= 1u << depth;
                const Ray nr = spawn_ray(si.hit, bs.wi);
                nr_o = nr.o; nr_d = nr.d; nbeta = vdiv(beta * bs.f * c, bs.pdf); depth += 1; cont = true;
                break;
              }
            }
            // specular_transmission (mod.rs:92-142)
            const LobeSample bs = bsdf_sample_f(b, wo, dr.get(k2), BSDF_SPECULAR | BSDF_TRANSMISSION); k2 += 1u;
            const float c = fabsf(dot(bs.wi, ns));
            if (bs.pdf > 0.0f && !is_black(bs.f) && c != 0.0f) {
              const Ray nr = spawn_ray(si.hit, bs.wi);
              nr_o = nr.o; nr_d = nr.d; nbeta = vdiv(beta * bs.f * c, bs.pdf); depth += 1; cont = true;
              break;
            }
          }
        } else if (!last) break;
        // the subtree is finished: up to the pending transmission of the nearest ancestor
        if (pending == 0u) break;
        const int lvl = 31 - __clz((int)pending);
        pending &= ~(1u << lvl);
        const float4* const e = a.stack + (size_t)lvl * a.stack_cap + pid; const size_t plane = (size_t)a.levels * a.stack_cap;
        const float4 e0 = e[0], e1 = e[plane], e2 = e[2 * plane], e3 = e[3 * plane];
        ray_o = mk3(e0.x, e0.y, e0.z); ray_d = mk3(e1.x, e1.y, e1.z); h4 = make_float4(e0.w, e1.w, e2.x, e2.y); beta = mkc(e3.x, e3.y, e3.z);
        depth = lvl; have_vertex = true; fresh = false;
      }
      if (last) a.wst[pid] = make_uint4(k2, w4.y + 1u, k1, v);
      else if (dr.rng_used) { st.z = (unsigned)dr.rng.state; st.w = (unsigned)(dr.rng.state >> 32); sraw(ps.in.st)[slot] = st; }  // the next round's draw follows this one
      nst = (unsigned)depth | (pending << 8); rng_out = dr.rng.state;
    }
    const int qi[3] = {0, 1, 2}; const bool pr[3] = {cont, want_shadow, want_probe}; unsigned qs[3];
    block_push<3>(ps.cnt_out, ps.shard_cap, qi, pr, qs);
    if (cont) {  // the sample's next node, at its slot of the next step's queue: a wave's stores are runs of consecutive slots
      sraw(ps.out.o)[qs[0]] = make_float4(nr_o.x, nr_o.y, nr_o.z, kInf);
      sraw(ps.out.d)[qs[0]] = make_float4(nr_d.x, nr_d.y, nr_d.z, 0.0f);
      sraw(ps.out.beta)[qs[0]] = make_float4(nbeta.r, nbeta.g, nbeta.b, 1.0f);
      sraw(ps.out.st)[qs[0]] = make_uint4(nst, pid, (unsigned)rng_out, (unsigned)(rng_out >> 32));
    }
    if (want_shadow) ps.q_shadow[qs[1]] = i;
    if (want_probe) ps.q_mis[qs[2]] = i;
  }
}

// ================================================================================ probe resolution
// One lane per probe record of the round (ps.q_mis; the closest-hit launch has left the hit in ps.mi.hit): lacc[path] += term * le with le the emitter's L at the hit's
// geometric normal where the hit primitive's light IS the probe's light (mod.rs:293-307; a hit inside an object instance is in no light list), the infinite light's le on a
// miss, nothing otherwise - k_resolve's reading of the hit. One probe per path and round: ordinary loads and stores, no race.
template <bool GENERAL>
__global__ void __launch_bounds__(256) k_direct_probe(DScene sc, PassState ps) {
  QView qv; qv.init(ps.q_mis, ps.cnt_out + 2 * RT_QSHARDS * RT_CNT_STRIDE, ps.shard_cap);
  const unsigned count = qv.total(), stride = gridDim.x * blockDim.x;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const unsigned rec = qv.get(i);
    const float4 a4 = sraw(ps.mi.a)[rec], d4 = sraw(ps.mi.d)[rec], h4 = sraw(ps.mi.hit)[rec];
    const int light_num = __float_as_int(a4.w);
    const DLight& light = sc.lights[light_num];
    const f3 wi = mk3(d4.x, d4.y, d4.z);
    rgb3 li = mkc(0, 0, 0);
    const int prim = __float_as_int(h4.y);
    if (GENERAL && sc.n_instances != 0u && prim >= 0 && (unsigned)prim >= sc.n_top_prims) {
    } else if (prim >= 0) {
      if (tri_light(sc.tri_p, prim) == light_num) {
        const float4 o4 = sraw(ps.mi.o)[rec];
        if (GENERAL && (tri_flags(sc.tri_p, prim) & RT_FLAG_SPHERE)) {
          SurfaceInteraction lsi; (void)sphere_fill_interaction(sc.spheres[prim_sphere_index(sc.tri_p, prim)], mk3(o4.x, o4.y, o4.z), wi, lsi);
          li = area_light_l(light, lsi.hit.n, -wi);
        } else {
          f3 p0, p1, p2; load_tri(sc.tri_p, prim, p0, p1, p2);
          Ray r; r.o = mk3(o4.x, o4.y, o4.z); r.d = wi; r.t_max = kInf;
          TriHit th; (void)tri_test_call(p0, p1, p2, r, th);
          f3 p, n; tri_hit_point_normal(*sc.self, prim, th, p, n);
          li = area_light_l(light, n, -wi);
        }
      }
    } else if (light.kind == 3) li = infinite_le(sc, light, wi);  // light.le(ray)
    if (is_black(li)) continue;
    const rgb3 add = mkc(a4.x, a4.y, a4.z) * li;
    const unsigned pid = __float_as_uint(d4.w);
    const float4 l4 = ps.lacc[pid];
    ps.lacc[pid] = make_float4(l4.x + add.r, l4.y + add.g, l4.z + add.b, l4.w);
  }
}

// One lane per path of the pass: the four counters of every traced sample at its place in the caller's array. A skipped ray keeps the zeros the call began with.
static __global__ void __launch_bounds__(256) k_direct_info(FrameParams fp, PassState ps, DirectArgs a, int wx0, int wy0, int ww, uint4* __restrict__ info) {
  const unsigned stride = gridDim.x * 256u;
  for (unsigned pid = blockIdx.x * 256u + threadIdx.x; pid < ps.cap; pid += stride) {
    if (__float_as_uint(ps.lacc[pid].w) & RT_STATE_OUT_OF_BOUNDS) continue;
    unsigned sl, pix; split_path_id(ps, pid, sl, pix);
    int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
    const uint4 w4 = a.wst[pid];
    info[((size_t)(y - wy0) * (size_t)ww + (size_t)(x - wx0)) * ps.spp + ps.s0 + sl] = make_uint4(w4.y, w4.x, w4.z, w4.w);
  }
}

void rtx_launch_direct_vertex(bool general, unsigned grid, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& ps, const DirectArgs& a) {
  if (general) hipLaunchKernelGGL((k_direct_vertex<true>), dim3(grid), dim3(256), 0, stream, d, fp, ps, a);
  else hipLaunchKernelGGL((k_direct_vertex<false>), dim3(grid), dim3(256), 0, stream, d, fp, ps, a);
}
void rtx_launch_direct_probe(bool general, unsigned grid, hipStream_t stream, const DScene& d, const PassState& ps) {
  if (general) hipLaunchKernelGGL((k_direct_probe<true>), dim3(grid), dim3(256), 0, stream, d, ps);
  else hipLaunchKernelGGL((k_direct_probe<false>), dim3(grid), dim3(256), 0, stream, d, ps);
}
void rtx_launch_direct_info(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const DirectArgs& a, int wx0, int wy0, int ww, uint4* info) {
  hipLaunchKernelGGL(k_direct_info, dim3(grid), dim3(256), 0, stream, fp, ps, a, wx0, wy0, ww, info);
}
hipError_t rtx_launch_sampler_array_tables(hipStream_t stream, const FrameParams& fp, unsigned n_pixels, unsigned spp, unsigned dims, unsigned n_arrays, unsigned* scrambles,
                                           unsigned short* perms) {
  if (n_pixels == 0u || n_arrays == 0u) return hipSuccess;
  // lanes per block: the per-lane permutation (2 B * (spp + 2)) of a block should fill ~32 KB of LDS, as K0's
  unsigned lpb = (32u * 1024u) / ((spp + 2u) * 2u);
  lpb = lpb >= 64u ? 64u : (lpb >= 32u ? 32u : (lpb >= 16u ? 16u : (lpb >= 8u ? 8u : 4u)));
  const size_t lds = (size_t)lpb * (spp + 2u) * 2u;
  if (lds > 48u * 1024u) {
    const hipError_t e = hipFuncSetAttribute((const void*)k_sampler_array_tables, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_sampler_array_tables, dim3((n_pixels + lpb - 1u) / lpb), dim3(lpb), lds, stream, fp, n_pixels, spp, dims, n_arrays, scrambles, perms);
  return hipGetLastError();
}
void rtx_direct_set_ewa_lut(const float* lut128) { (void)hipMemcpyToSymbol(HIP_SYMBOL(kEwaLut), lut128, 128 * sizeof(float)); }
}  // namespace rtx
