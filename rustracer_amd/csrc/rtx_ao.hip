// rtx_ao.hip - the ambient-occlusion and normal integrators (rt_render_rays_ao, rt_render_ao: integrator/ao.rs, integrator/normal.rs). One closest-hit ray per camera
// sample - bounce 0 of any frame, traced by the scene's closest-hit launch -, then n_samples rounds of "one occlusion ray per hit path": k_ao_rays builds the hit's
// interaction with the fill routines the shade kernels call (tri_fill_interaction_inl, quadric_interaction_visit, instance_interaction_visit: rtx_shade_kernels.h, no copy
// of them lives here), draws the round's get_2d(), and writes spawn_ray(hit, w) into the planar shadow-ray records; the scene's production any-hit launch traces them
// with shadow_masks = 1 (scene.intersect_p). No BSDF, no light. A translation unit of its own, compiled beside the others: no other kernel's code object changes.
#include <hip/hip_runtime.h>
#include "../../include/rtx_hip.h"
#include "rtx_shade_kernels.h"
#include "rtx_ao_launch.h"

namespace rtx {

struct AoHit { f3 p, p_error, n; };  // what AmbientOcclusion::li and Normal::li read of the SurfaceInteraction: hit.p, hit.p_error and the GEOMETRIC normal hit.n
RT_DEV AoHit ao_hit_of(const SurfaceInteraction& si) { AoHit h; h.p = si.hit.p; h.p_error = si.hit.p_error; h.n = si.hit.n; return h; }

// where sample s of pixel_index sits in the caller's ray records, in records (k_camera_rays' indexing)
RT_DEV size_t ao_ray_record(const AoArgs& a, unsigned long long pixel_index, unsigned s) { return (size_t)(pixel_index * a.ray_ns + (s - a.ray_s0)) * a.n_ao + a.round; }

// One lane per entry of bounce 0's queue (ps.in / ps.cnt_in; NULL counts: entry i is slot i), a workgroup per run of 256 entries. Reads the ray, the hit and the state
// record at consecutive slots of consecutive lanes, then the gathers of the fill routine and - while 2 + round < dimensions - the three words of the sampler tables.
// Writes, per hit path, the shadow record of ENTRY i (o | t_max), (d | flag | path id) - a wave's stores are one contiguous 1 KB run per plane - and appends i to the
// shadow queue (block_push: one atomic per workgroup and iteration); in round 0 also the add record (1, 0, 0, 0) - the entries are the same in every round - and aux.
// The RNG state of a path whose rounds have left the tables travels in its state record (st.zw), as between the bounces of a path.
// Everything that decides where the ray goes is IEEE: the division-free uniform_sample_sphere (sampling/mod.rs:14-20, in Sphere::sample's operation order,
// rtx_dev_sphere.h), the flip, offset_ray_origin. GENERAL: the scene holds quadrics or object instances.
template <bool GENERAL>
__global__ void __launch_bounds__(256) k_ao_rays(DScene sc, FrameParams fp, PassState ps, AoArgs a) {
  QView qv; if (ps.cnt_in) qv.init(nullptr, ps.cnt_in, ps.shard_cap);
  const unsigned count = ps.cnt_in ? qv.total() : ps.cap, stride = gridDim.x * 256u;
  const Tables tb = tables_of(ps);
  for (unsigned base = blockIdx.x * 256u; base < count; base += stride) {  // (uniform per workgroup: block_push holds barriers)
    const unsigned i = base + threadIdx.x;
    bool cast = false;
    if (i < count) {
      const unsigned slot = ps.cnt_in ? qv.get(i) : i;
      const float4 o4 = sraw(ps.in.o)[slot], d4 = sraw(ps.in.d)[slot], h4 = sraw(ps.hit)[slot];
      uint4 st = sraw(ps.in.st)[slot];
      const unsigned pid = st.y;
      const f3 ray_o = mk3(o4.x, o4.y, o4.z), ray_d = mk3(d4.x, d4.y, d4.z);
      const int prim = __float_as_int(h4.y);
      cast = prim >= 0;
      if (cast) {
        TriHit th; th.t = 0.0f; th.b0 = h4.z; th.b1 = h4.w; th.b2 = h4.x;  // the frame loop's hit record is (b2, prim, b0, b1)
        const auto take = [](const SurfaceInteraction& si) { return ao_hit_of(si); };
        AoHit h;
        if (GENERAL && sc.n_instances != 0u && (unsigned)prim >= sc.n_top_prims)
          h = sc.obj_general ? instance_interaction_visit<true>(sc, (unsigned)prim, ray_o, ray_d, th.b0, th.b1, th.b2, take)
                             : instance_interaction_visit<false>(sc, (unsigned)prim, ray_o, ray_d, th.b0, th.b1, th.b2, take);
        else if (GENERAL && (tri_flags(sc.tri_p, prim) & RT_FLAG_SPHERE)) h = quadric_interaction_visit(sc.spheres[prim_sphere_index(sc.tri_p, prim)], ray_o, ray_d, take);
        else { SurfaceInteraction si; tri_fill_interaction_inl<true>(sc, prim, ray_d, th, si); h = ao_hit_of(si); }  // (wo is not read)
        unsigned sl, pix; split_path_id(ps, pid, sl, pix); const unsigned s = ps.s0 + sl;
        int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
        f2 u;  // the round's get_2d() (zerotwosequence.rs:168-180), counters where get_camera_sample left them: cur_2d = 2
        if (2u + a.round < ps.dims) u = table_2d(tb, pix, 2u + a.round, s);
        else {
          Pcg32 rng; rng.state = (unsigned long long)st.z | ((unsigned long long)st.w << 32);
          rng.inc = ((pixel_index * (unsigned long long)ps.spp + s + (1ull << 32)) << 1u) | 1ull;  // set_sequence of the keyed per-sample stream (k_raygen)
          const float first = rng.next_f32(), second = rng.next_f32();
          u = mk2(second, first);
          st.z = (unsigned)rng.state; st.w = (unsigned)(rng.state >> 32);
          sraw(ps.in.st)[slot] = st;
        }
        const float z = 1.0f - 2.0f * u.x;  // uniform_sample_sphere
        const float r = sqrtf(fmaxf(1.0f - z * z, 0.0f));
        const float phi = 2.0f * kPi * u.y;
        float sn_phi, cs_phi; sincosf(phi, &sn_phi, &cs_phi);
        f3 w = mk3(r * cs_phi, r * sn_phi, z);
        if (dot(w, h.n) < 0.0f) w = -w;  // ao.rs:45-47
        Interaction it; it.p = h.p; it.p_error = h.p_error; it.n = h.n; it.wo = mk3(0, 0, 0);
        const Ray ar = spawn_ray(it, w);
        const float4 ro = make_float4(ar.o.x, ar.o.y, ar.o.z, a.max_distance), rd = make_float4(w.x, w.y, w.z, __uint_as_float(a.flag | pid));
        sraw(ps.sh.o)[i] = ro; sraw(ps.sh.d)[i] = rd;
        if (a.round == 0u) sraw(ps.sh.add)[i] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        if (a.rays_out) { float4* q = a.rays_out + 2u * ao_ray_record(a, pixel_index, s); q[0] = ro; q[1] = make_float4(w.x, w.y, w.z, 0.0f); }
        if (a.round == 0u && a.aux) a.aux[pid] = make_float4(fabsf(dot(ray_d, h.n)), len(h.p - ray_o), 0.0f, 0.0f);  // Normal::li (normal.rs:30-32); depth as the feature planes'
      } else if (a.round == 0u && a.aux) a.aux[pid] = make_float4(0.0f, 0.0f, 1.0f, 0.0f);  // a miss
    }
    const int qi[1] = {1}; const bool pr[1] = {cast}; unsigned qs[1];
    block_push<1>(ps.cnt_out, ps.shard_cap, qi, pr, qs);
    if (cast) ps.q_shadow[qs[0]] = i;
  }
}

// One lane per entry of the round's shadow queue: the record's answer (one byte, PassState::occ_sh) into the path's count and into the caller's copy of the record.
// One record per path and round, so the read-modify-write of lacc is race-free.
static __global__ void __launch_bounds__(256) k_ao_fold(FrameParams fp, PassState ps, AoArgs a) {
  QView qv; qv.init(ps.q_shadow, ps.cnt_out + RT_QSHARDS * RT_CNT_STRIDE, ps.shard_cap);
  const unsigned count = qv.total(), stride = gridDim.x * 256u;
  for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < count; j += stride) {
    const unsigned rec = qv.get(j);
    const bool occluded = ps.occ_sh[rec] != 0;
    const unsigned pid = __float_as_uint(sraw(ps.sh.d)[rec].w) & 0x7fffffffu;
    if (!occluded) { float4 l = ps.lacc[pid]; l.x += 1.0f; ps.lacc[pid] = l; }
    if (a.rays_out) {
      unsigned sl, pix; split_path_id(ps, pid, sl, pix);
      int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
      ((float*)(a.rays_out + 2u * ao_ray_record(a, pixel_index, ps.s0 + sl)))[7] = occluded ? 1.0f : 0.0f;
    }
  }
}

// One lane per path of the pass: lacc.x holds n_clear, exact in float32 (n_ao <= 1024); one IEEE divide (ao.rs:54). A sample outside pixel_bounds, a skipped ray: untouched.
static __global__ void __launch_bounds__(256) k_ao_finish(FrameParams fp, PassState ps, AoArgs a, int wx0, int wy0, int ww, float4* __restrict__ out) {
  const unsigned stride = gridDim.x * 256u;
  const float n = (float)a.n_ao;
  for (unsigned pid = blockIdx.x * 256u + threadIdx.x; pid < ps.cap; pid += stride) {
    const float4 l4 = ps.lacc[pid];
    if (__float_as_uint(l4.w) & RT_STATE_OUT_OF_BOUNDS) continue;
    const float ao = l4.x / n;
    if (!out) { ps.lacc[pid] = make_float4(ao, ao, ao, l4.w); continue; }  // Spectrum::grey(ao)
    unsigned sl, pix; split_path_id(ps, pid, sl, pix);
    int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
    const float4 x4 = a.aux[pid];
    out[((size_t)(y - wy0) * (size_t)ww + (size_t)(x - wx0)) * ps.spp + ps.s0 + sl] = make_float4(ao, x4.x, x4.y, x4.z);
  }
}

void rtx_launch_ao_rays(bool general, unsigned grid, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& ps, const AoArgs& a) {
  if (general) hipLaunchKernelGGL((k_ao_rays<true>), dim3(grid), dim3(256), 0, stream, d, fp, ps, a);
  else hipLaunchKernelGGL((k_ao_rays<false>), dim3(grid), dim3(256), 0, stream, d, fp, ps, a);
}
void rtx_launch_ao_fold(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const AoArgs& a) {
  hipLaunchKernelGGL(k_ao_fold, dim3(grid), dim3(256), 0, stream, fp, ps, a);
}
void rtx_launch_ao_finish(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const AoArgs& a, int wx0, int wy0, int ww, float4* out) {
  hipLaunchKernelGGL(k_ao_finish, dim3(grid), dim3(256), 0, stream, fp, ps, a, wx0, wy0, ww, out);
}
}  // namespace rtx
