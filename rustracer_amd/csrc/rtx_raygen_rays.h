// rtx_raygen_rays.h — bounce 0 from caller-supplied rays (rt_render_rays): the producer that stands where k_raygen stands when a frame's first rays do not come
// from the perspective camera - and from the caller's rays AND film positions for the step of a ray frame (k_raygen_rays_film, at the end of the file).
// And k_camera_rays, rt_camera_rays' kernel: the perspective camera's rays handed out. Included by rtx_rays.hip alone (launchers: rtx_rays_launch.h); k_raygen /
// k_raygen_masked (rtx_raygen_body.inl) are not touched.
#pragma once
#include "rtx_kernels.h"

namespace rtx {

// Does any ray of the call carry a t_max that is not > 0 (zero, negative, NaN: the ray is skipped)? One scan of the rays before the first pass, one word read back:
// the answer picks the route of every pass - none skipped: PassState::all_in_bounds with the fresh records, else the sharded bounce-0 queue of a cropped frame.
static __global__ void __launch_bounds__(256) k_rays_scan(const float* __restrict__ rays, unsigned long long n_rays, unsigned rec_floats, unsigned* __restrict__ any_skipped) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  bool skip = false;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_rays; i += stride) skip |= !(rays[i * rec_floats + 3ull] > 0.0f);
  if (__ballot(skip) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(any_skipped, 1u);
}

// One lane per ray of the pass. The caller's records are [pixel][sample of the call][8 floats] - pixel-major - and the pass's path ids are sample-major (local sample *
// n_pixels + batch pixel), so a workgroup takes a TILE of 2^tp_log2 pixels x 2^ts_log2 samples (256 rays): it reads the tile's records as 512 float4 - lane after lane,
// runs of 2 * TS float4 per pixel, contiguous over the tile where the pass holds all the call's samples; once-through, so with the non-temporal hint of the other streams -
// into LDS, and after a barrier every lane takes the ray of ITS path id, so that the record stores of a wave are the runs of neighbouring slots k_raygen's are.
// ts_log2 = log2(min(16, the pass's samples rounded up to a power of two)), tp_log2 = 8 - ts_log2.
// What it writes per ray is what rtx_raygen_body.inl writes per camera sample: lacc (zero | RT_STATE_OUT_OF_BOUNDS for a skipped ray), pfilm (the pixel centre: nothing
// reads it - the shade launches of caller-supplied rays rebuild no camera ray: no differentials, or the caller's, k_shade_rays), the ray at its slot with the caller's t_max in o.w, the throughput and state records unless the pass
// leaves them out (PassState::fresh), the shard push where rays are skipped, and ST_CAMERA. A skipped ray (t_max not > 0) gets no slot and its answer right here:
// rad[ray] = (0, 0, 0, 2.0) - k_sample_store passes over samples marked out of bounds.
// ray_s0 / ray_ns: first sample and samples per pixel of the CALL (the pass renders [ps.s0, ps.s0 + ps.n_samples) of them). rec4: float4 per record of the caller's array - 2,
// or 5 with RT_FLAG_RAY_DIFFERENTIALS; the kernel reads the first two of each (k_rays_scan / k_rays_scan_owned: rec_floats = 4 * rec4).
static __global__ void __launch_bounds__(256) k_raygen_rays(FrameParams fp, PassState ps, RT_SPTR_R(const float4) rays, unsigned ray_s0, unsigned ray_ns, unsigned rec4,
                                                            unsigned ts_log2, float4* __restrict__ rad) {
  __shared__ float4 s_ray[512 + 256];  // [tile pixel][2 * TS + 1]: one float4 of padding per pixel row
  const unsigned tp_log2 = 8u - ts_log2, TS = 1u << ts_log2, TP = 1u << tp_log2, row = 2u * TS + 1u;
  const unsigned n_ptiles = (ps.n_pixels + TP - 1u) >> tp_log2, n_stiles = (ps.n_samples + TS - 1u) >> ts_log2, n_tiles = n_ptiles * n_stiles;
  unsigned n_camera = 0;
  for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // (uniform per workgroup: barriers inside)
    const unsigned stile = tile / n_ptiles, ptile = tile - stile * n_ptiles;
    const unsigned pix0 = ptile << tp_log2, sl0 = stile << ts_log2;
#pragma unroll
    for (unsigned k = 0; k < 2u; ++k) {  // the tile's records, pixel-major as the caller laid them out
      const unsigned idx = threadIdx.x + 256u * k, lp = idx >> (ts_log2 + 1u), within = idx & (2u * TS - 1u);
      const unsigned pix = pix0 + lp, sl = sl0 + (within >> 1);
      if (pix < ps.n_pixels && sl < ps.n_samples) {
        int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
        s_ray[lp * row + within] = rays[(size_t)((pixel_index * ray_ns + (ps.s0 + sl - ray_s0)) * rec4 + (within & 1u))];
      }
    }
    __syncthreads();
    const unsigned lp = threadIdx.x & (TP - 1u), ls = threadIdx.x >> tp_log2;
    const unsigned pix = pix0 + lp, sl = sl0 + ls;
    const bool live = pix < ps.n_pixels && sl < ps.n_samples;
    const unsigned pid = sl * ps.n_pixels + pix;
    bool traced = false;
    float4 o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d4 = o4; unsigned long long rng_state = 0ull;
    if (live) {
      o4 = s_ray[lp * row + 2u * ls]; d4 = s_ray[lp * row + 2u * ls + 1u];
      traced = o4.w > 0.0f;  // (false for NaN)
      const unsigned s = ps.s0 + sl;
      int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
      Pcg32 rng; rng.set_sequence(pixel_index * (unsigned long long)ps.spp + s + (1ull << 32));  // keyed per-sample stream, as k_raygen
      rng_state = rng.state;
      ps.lacc[pid] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(traced ? 0u : RT_STATE_OUT_OF_BOUNDS));
      ps.pfilm[pid] = make_float2((float)x + 0.5f, (float)y + 0.5f);
      if (!traced) rad[(size_t)(pixel_index * ray_ns + (s - ray_s0))] = make_float4(0.0f, 0.0f, 0.0f, 2.0f);
    }
    n_camera += traced ? 1u : 0u;
    unsigned slot = pid;  // every ray traced: path i is entry i is slot i
    if (!ps.all_in_bounds) {
      const int ci[1] = {0}; const bool pr[1] = {traced}; unsigned sl_[1];
      block_push<1>(ps.cnt_out, ps.shard_cap, ci, pr, sl_);
      slot = sl_[0];
    }
    if (traced) {
      ps.out.o[slot] = o4;
      ps.out.d[slot] = make_float4(d4.x, d4.y, d4.z, 0.0f);
      if (!RT_FRESH_BETA(ps)) ps.out.beta[slot] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
      if (!RT_FRESH_ST(ps)) ps.out.st[slot] = make_uint4(pack_state(0, false, 1, 2), pid, (unsigned)rng_state, (unsigned)(rng_state >> 32));  // counters where get_camera_sample leaves them
    }
    __syncthreads();  // (the next tile's records overwrite s_ray)
  }
  for (int off = 32; off > 0; off >>= 1) n_camera += __shfl_down(n_camera, off);
  if ((threadIdx.x & 63u) == 0u && n_camera) atomicAdd(&ps.stats[ST_CAMERA], (unsigned long long)n_camera);
}

// ---- ray frames (rt_frame_begin_rays / rt_frame_advance_rays*): the step of a progressive frame whose rays and film positions come from the caller.
// k_rays_scan for the step of a SHARDED ray frame: the same question asked of the rays of the rank's own rows only - the rows of other ranks are never read. One lane per
// (owned pixel, sample of the step); fp.chunk_first is 0.
static __global__ void __launch_bounds__(256) k_rays_scan_owned(FrameParams fp, const float* __restrict__ rays, unsigned long long owned_pixels, unsigned ray_ns,
                                                                unsigned rec_floats, unsigned* __restrict__ any_skipped) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x, n = owned_pixels * ray_ns;
  bool skip = false;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned long long k = i / ray_ns;
    int x, y; unsigned long long pixel_index; owned_pixel(fp, k, x, y, pixel_index);
    skip |= !(rays[(pixel_index * ray_ns + (i - k * ray_ns)) * rec_floats + 3ull] > 0.0f);
  }
  if (__ballot(skip) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(any_skipped, 1u);
}
// Bounce 0 of a ray frame's step (rtx_raygen_rays_film.inl): k_raygen_rays with the film position of every sample, and no per-sample output. ray_s0 / ray_ns: first
// sample and samples per pixel of the STEP - rays and p_film hold [pixel_index][ray_ns] records.
static __global__ void __launch_bounds__(256) k_raygen_rays_film(FrameParams fp, PassState ps, RT_SPTR_R(const float4) rays, RT_SPTR_R(const float2) p_film, unsigned ray_s0,
                                                                 unsigned ray_ns, unsigned rec4, unsigned ts_log2) {
#include "rtx_raygen_rays_film.inl"
}
// ... of an adaptive step: a pixel whose byte is 0 takes none of the step's samples, and its rays are not read.
static __global__ void __launch_bounds__(256) k_raygen_rays_film_masked(FrameParams fp, PassState ps, RT_SPTR_R(const float4) rays, RT_SPTR_R(const float2) p_film,
                                                                        unsigned ray_s0, unsigned ray_ns, unsigned rec4, unsigned ts_log2, const unsigned char* __restrict__ active) {
#define RT_RAYGEN_RAYS_MASKED
#include "rtx_raygen_rays_film.inl"
#undef RT_RAYGEN_RAYS_MASKED
}
// rt_camera_rays: the perspective camera's rays of a pass, handed out instead of traced - what k_raygen computes per camera sample (film position from 2D#0, lens
// sample from 2D#1, generate_camera_ray with differentials scaled by 1 / sqrt(spp)) and, with rec4 = 5, the differentials bounce 0's shade kernels would rebuild from it.
// One lane per (pixel, sample) with the SAMPLE running fastest: lane i of the pass takes pixel i / n_samples, local sample i % n_samples, so consecutive lanes store
// consecutive records of the caller's [pixel_index][ray_ns] array. ray_s0 / ray_ns: first sample and samples per pixel of the CALL. p_film may be NULL.
static __global__ void __launch_bounds__(256) k_camera_rays(FrameParams fp, PassState ps, unsigned ray_s0, unsigned ray_ns, unsigned rec4, float4* __restrict__ rays,
                                                            float2* __restrict__ p_film_out) {
  const Tables tb = tables_of(ps);
  const unsigned stride = gridDim.x * blockDim.x;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < ps.cap; i += stride) {  // (ps.cap = n_pixels * n_samples <= 2^31 - 1)
    const unsigned pix = i / ps.n_samples, sl = i - pix * ps.n_samples, s = ps.s0 + sl;
    int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
    const f2 o = table_2d(tb, pix, 0, s);
    const f2 p_film = mk2((float)x + o.x, (float)y + o.y);
    const f2 p_lens = fp.lens_radius > 0.0f ? table_2d(tb, pix, 1, s) : mk2(0.0f, 0.0f);
    const CameraRay cr = generate_camera_ray(fp, p_film, p_lens, 1.0f / sqrtf((float)ps.spp));
    const size_t rec = (size_t)(pixel_index * ray_ns + (s - ray_s0));  // (< RT_RAYS_MAX: checked by rt_camera_rays)
    float4* r = rays + rec * rec4;
    r[0] = make_float4(cr.o.x, cr.o.y, cr.o.z, kInf);
    r[1] = make_float4(cr.d.x, cr.d.y, cr.d.z, 0.0f);
    if (rec4 == 5u) {
      r[2] = make_float4(cr.rx_o.x, cr.rx_o.y, cr.rx_o.z, cr.ry_o.x);
      r[3] = make_float4(cr.ry_o.y, cr.ry_o.z, cr.rx_d.x, cr.rx_d.y);
      r[4] = make_float4(cr.rx_d.z, cr.ry_d.x, cr.ry_d.y, cr.ry_d.z);
    }
    if (p_film_out) p_film_out[rec] = make_float2(p_film.x, p_film.y);
  }
}
// rt_frame_read(RT_FRAME_SUMS): k_frame_resolve's walk - one lane per cropped pixel, film sum + the pixel's own sum where this shard owns its row - with the sums stored as
// they are, (sum w L).rgb and the weight sum: no colour matrix, no division. A kernel of this translation unit, not a branch of frame_resolve_store, so that the code
// object of rtx_hip.hip stays what it was.
static __global__ void __launch_bounds__(256) k_frame_sums_read(FrameParams fp, const float4* __restrict__ film_acc, const float4* __restrict__ own_plane, float4* __restrict__ out,
                                                                unsigned long long n) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned cw = (unsigned)(fp.crop_x1 - fp.crop_x0);
  const int x = fp.crop_x0 + (int)(i % cw), y = fp.crop_y0 + (int)(i / cw);
  float4 a = film_acc[i];
  if (x >= fp.sb_x0 && x < fp.sb_x1 && y >= fp.sb_y0 && y < fp.sb_y1) {  // the inverse of owned_pixel
    const unsigned long long row = (unsigned long long)(y - fp.sb_y0), band = row >> fp.shard_log2;
    if (band % (unsigned long long)fp.world == (unsigned long long)fp.rank) {
      const unsigned long long j = ((band / (unsigned long long)fp.world) << fp.shard_log2) + (row & ((1ull << fp.shard_log2) - 1ull));
      const float4 o = own_plane[j * (unsigned long long)(fp.sb_x1 - fp.sb_x0) + (unsigned long long)(x - fp.sb_x0)];
      a = make_float4(a.x + o.x, a.y + o.y, a.z + o.z, a.w + o.w);
    }
  }
  out[i] = a;
}

}  // namespace rtx
