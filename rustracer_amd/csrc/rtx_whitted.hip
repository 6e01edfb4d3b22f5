// rtx_whitted.hip - the Whitted integrator (rt_render_rays_whitted, rt_render_whitted: integrator/whitted.rs:41-99, integrator/mod.rs:49-142). Whitted::li branches:
// a vertex on glass continues as a reflected AND a transmitted ray, and the sampler's draws are consumed depth-first - the vertex's lights, the reflection draw, the whole
// reflection subtree, the transmission draw, the transmission subtree. The frame loop walks that tree one NODE per camera sample and step (run_whitted, rtx_hip.hip); this
// unit holds the kernel of a step, k_whitted_vertex: the hit's interaction through the fill routines the shade kernels call, the Bsdf through build_bsdf<false>
// (allow_multiple_lobes = false: smooth glass as SpecularReflection + SpecularTransmission), the light functions rt_light_eval runs, bsdf_f / bsdf_sample_f. No copy of
// them lives here. The form built is the exact one: a vertex whose reflection is followed waits as a 64-byte record (its incoming ray, its hit, its throughput) on a planar
// stack in HBM and is REBUILT when it is popped, where its transmission draw is taken - after its reflection subtree, as in the reference.
// Stated divergence: specular children carry no ray differentials (the reference propagates them, mod.rs:64-83, 107-136); every derivative at depth >= 1 is zero, as at the
// later vertices of the path frames. A translation unit of its own, compiled beside the others: no other kernel's code object changes.
#include <hip/hip_runtime.h>
#include "../../include/rtx_hip.h"
#include "rtx_shade_kernels.h"
#include "rtx_whitted_launch.h"
#include "rtx_whitted_dev.h"

namespace rtx {

// (WhittedDraws and whitted_interaction: rtx_whitted_dev.h, shared with the direct-lighting integrator's unit)

// One lane per entry of the step's queue (ps.in / ps.cnt_in; NULL counts: entry i is slot i is path i), a workgroup per run of 256 entries, grid-stride as k_ao_rays.
// Reads the ray, the hit, the throughput and the state record at consecutive slots of consecutive lanes, the path's two counters by path id, then the gathers of the fill
// routine, the material and the light. Writes, in a light round, the shadow record of ENTRY i - (o | t_max), (d | complete-here flag | path id), the weighted term - and
// appends i to the shadow queue; in the last round the sample's next node at its slot of the next step's queue (block_push: one atomic per queue, workgroup and
// iteration), the pending record of a vertex whose reflection is followed, and the counters. State record: st.x = depth | pending levels << 8, st.y = path id, st.zw = the
// RNG state of a path whose draws have left the tables.
// Everything that decides where a ray goes is IEEE: spawn_ray / offset_ray_origin, the specular directions and Fresnel's branch on total internal reflection inside
// bsdf_sample_f. The radiance-only quotients (the term / pdf, beta / pdf) are vdiv: v_rcp_f32 in the default build, correctly rounded under STRICT=1.
// GENERAL: quadric or instance hits, quadric or masked emitters.
template <bool GENERAL>
__global__ void __launch_bounds__(256, RT_SHADE0_MIN_WAVES) k_whitted_vertex(DScene sc, FrameParams fp, PassState ps, WhittedArgs a) {
  QView qv; if (ps.cnt_in) qv.init(nullptr, ps.cnt_in, ps.shard_cap);
  const unsigned count = ps.cnt_in ? qv.total() : ps.cap, stride = gridDim.x * 256u;
  const DScene& gsc = *sc.self;  // what out-of-line functions get: the scene record in device memory
  const Tables tb = tables_of(ps);
  const bool last = a.round + 1u == a.n_rounds;
  for (unsigned base = blockIdx.x * 256u; base < count; base += stride) {  // (uniform per workgroup: block_push holds barriers)
    const unsigned i = base + threadIdx.x;
    bool cont = false, want_shadow = false;
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
      unsigned k = w4.x;  // the draws the sample has consumed before this node
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
          const f3 n = si.sh_n, wo = si.hit.wo;  // isect.shading.n BEFORE compute_scattering_functions: what the light terms' cosine reads (whitted.rs:53, 79)
          Bsdf b;
          build_bsdf<false>(gsc, rec_material(sc.tri_rec, prim), si, b);  // (a bump map rewrites si's shading geometry: the recursion's ns)
          if (fresh && a.round == 0u) {  // colour += isect.le(wo)
            const int li = rec_light(sc.tri_rec, prim);
            if (li >= 0) { const float4 l4 = ps.lacc[pid]; const rgb3 L = mkc(l4.x, l4.y, l4.z) + beta * area_light_l(sc.lights[li], si.hit.n, wo); ps.lacc[pid] = make_float4(L.r, L.g, L.b, l4.w); }
          }
          if (fresh && (int)a.round < a.n_lights) {  // light `round` of the scene's list: its draw is consumed whatever the light is
            const f2 u = dr.get(k + a.round);
            const DLight& light = sc.lights[a.round];
            const LiSample ls = light_sample_li_full<GENERAL>(gsc, light, si.hit, u);
            if (ls.pdf > 0.0f && !is_black(ls.li)) {
              const rgb3 f = bsdf_f(b, wo, ls.wi, BSDF_ALL);
              if (!is_black(f)) {
                const Ray sr = spawn_ray_to_interaction(si.hit, ls.p1);  // VisibilityTester, light/mod.rs:52-55
                const rgb3 add = beta * vdiv(f * ls.li * fabsf(dot(ls.wi, n)), ls.pdf);
                sraw(ps.sh.o)[i] = make_float4(sr.o.x, sr.o.y, sr.o.z, sr.t_max);
                sraw(ps.sh.d)[i] = make_float4(sr.d.x, sr.d.y, sr.d.z, __uint_as_float(0x80000000u | pid));  // bit 31: the any-hit epilogue adds a clear record's term
                sraw(ps.sh.add)[i] = make_float4(add.r, add.g, add.b, 0.0f);
                want_shadow = true;
              }
            }
          }
          if (!last) break;
          if (fresh) k += (unsigned)a.n_lights;
          if (depth + 1 < a.max_depth) {  // whitted.rs:83-88
            const f3 ns = si.sh_n;
            if (fresh) {  // specular_reflection (mod.rs:49-89): the draw is consumed whether or not a lobe matches
              const LobeSample bs = bsdf_sample_f(b, wo, dr.get(k), BSDF_SPECULAR | BSDF_REFLECTION); k += 1u;
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
            const LobeSample bs = bsdf_sample_f(b, wo, dr.get(k), BSDF_SPECULAR | BSDF_TRANSMISSION); k += 1u;
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
      if (last) a.wst[pid] = make_uint4(k, w4.y + 1u, 0u, 0u);
      else if (dr.rng_used) { st.z = (unsigned)dr.rng.state; st.w = (unsigned)(dr.rng.state >> 32); sraw(ps.in.st)[slot] = st; }  // the next round's draw follows this one
      nst = (unsigned)depth | (pending << 8); rng_out = dr.rng.state;
    }
    const int qi[2] = {0, 1}; const bool pr[2] = {cont, want_shadow}; unsigned qs[2];
    block_push<2>(ps.cnt_out, ps.shard_cap, qi, pr, qs);
    if (cont) {  // the sample's next node, at its slot of the next step's queue: a wave's stores are runs of consecutive slots
      sraw(ps.out.o)[qs[0]] = make_float4(nr_o.x, nr_o.y, nr_o.z, kInf);
      sraw(ps.out.d)[qs[0]] = make_float4(nr_d.x, nr_d.y, nr_d.z, 0.0f);
      sraw(ps.out.beta)[qs[0]] = make_float4(nbeta.r, nbeta.g, nbeta.b, 1.0f);
      sraw(ps.out.st)[qs[0]] = make_uint4(nst, pid, (unsigned)rng_out, (unsigned)(rng_out >> 32));
    }
    if (want_shadow) ps.q_shadow[qs[1]] = i;
  }
}

// One lane per path of the pass: the two counters of every traced sample at its place in the caller's array. A skipped ray keeps the zeros the call began with.
static __global__ void __launch_bounds__(256) k_whitted_info(FrameParams fp, PassState ps, WhittedArgs a, int wx0, int wy0, int ww, uint2* __restrict__ info) {
  const unsigned stride = gridDim.x * 256u;
  for (unsigned pid = blockIdx.x * 256u + threadIdx.x; pid < ps.cap; pid += stride) {
    if (__float_as_uint(ps.lacc[pid].w) & RT_STATE_OUT_OF_BOUNDS) continue;
    unsigned sl, pix; split_path_id(ps, pid, sl, pix);
    int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
    const uint4 w4 = a.wst[pid];
    info[((size_t)(y - wy0) * (size_t)ww + (size_t)(x - wx0)) * ps.spp + ps.s0 + sl] = make_uint2(w4.y, w4.x);
  }
}

void rtx_launch_whitted_vertex(bool general, unsigned grid, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& ps, const WhittedArgs& a) {
  if (general) hipLaunchKernelGGL((k_whitted_vertex<true>), dim3(grid), dim3(256), 0, stream, d, fp, ps, a);
  else hipLaunchKernelGGL((k_whitted_vertex<false>), dim3(grid), dim3(256), 0, stream, d, fp, ps, a);
}
void rtx_launch_whitted_info(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const WhittedArgs& a, int wx0, int wy0, int ww, uint2* info) {
  hipLaunchKernelGGL(k_whitted_info, dim3(grid), dim3(256), 0, stream, fp, ps, a, wx0, wy0, ww, info);
}
void rtx_whitted_set_ewa_lut(const float* lut128) { (void)hipMemcpyToSymbol(HIP_SYMBOL(kEwaLut), lut128, 128 * sizeof(float)); }
}  // namespace rtx
