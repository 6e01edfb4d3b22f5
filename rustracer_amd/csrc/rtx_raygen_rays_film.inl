// The body of k_raygen_rays_film and of k_raygen_rays_film_masked (rtx_raygen_rays.h includes it once for each): k_raygen_rays' tile scheme - 2^tp_log2 pixels x 2^ts_log2
// samples = 256 rays per workgroup, the caller's records staged through LDS - for the step of a RAY FRAME (rt_frame_advance_rays*). Shared as text, not as a function, so
// that the unmasked kernel holds no trace of the mask. RT_RAYGEN_RAYS_MASKED: `active` is the byte mask of the adaptive step, by owned pixel.
// What differs from k_raygen_rays: the tile's film positions are staged as well - p_film[pixel][sample of the step] float2, one per lane, or the pixel centre where p_film
// is NULL - and written to ps.pfilm[path id], which the frame's film kernel reads; a ray that is not traced (t_max not > 0, or a pixel the mask leaves out) is marked out
// of bounds and nothing else: a frame has no per-sample output.
  __shared__ float4 s_ray[512 + 256];  // [tile pixel][2 * TS + 1]: one float4 of padding per pixel row
  __shared__ float2 s_pf[256 + 256];   // [tile pixel][TS + 1]
  const unsigned tp_log2 = 8u - ts_log2, TS = 1u << ts_log2, TP = 1u << tp_log2, row = 2u * TS + 1u, prow = TS + 1u;
  const unsigned n_ptiles = (ps.n_pixels + TP - 1u) >> tp_log2, n_stiles = (ps.n_samples + TS - 1u) >> ts_log2, n_tiles = n_ptiles * n_stiles;
  const bool has_pf = p_film != nullptr;
  unsigned n_camera = 0;
  for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // (uniform per workgroup: barriers inside)
    const unsigned stile = tile / n_ptiles, ptile = tile - stile * n_ptiles;
    const unsigned pix0 = ptile << tp_log2, sl0 = stile << ts_log2;
#pragma unroll
    for (unsigned k = 0; k < 2u; ++k) {  // the tile's records, pixel-major as the caller laid them out
      const unsigned idx = threadIdx.x + 256u * k, lp = idx >> (ts_log2 + 1u), within = idx & (2u * TS - 1u);
      const unsigned pix = pix0 + lp, sl = sl0 + (within >> 1);
      bool take = pix < ps.n_pixels && sl < ps.n_samples;
#ifdef RT_RAYGEN_RAYS_MASKED
      if (take) take = active[fp.chunk_first + pix] != 0;  // (the rays of an inactive pixel are not read)
#endif
      if (take) {
        int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
        s_ray[lp * row + within] = rays[(size_t)((pixel_index * ray_ns + (ps.s0 + sl - ray_s0)) * rec4 + (within & 1u))];
      }
    }
    if (has_pf) {  // ... and its film positions: one float2 per lane
      const unsigned lp = threadIdx.x >> ts_log2, within = threadIdx.x & (TS - 1u);
      const unsigned pix = pix0 + lp, sl = sl0 + within;
      if (pix < ps.n_pixels && sl < ps.n_samples) {
        int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
        s_pf[lp * prow + within] = p_film[(size_t)(pixel_index * ray_ns + (ps.s0 + sl - ray_s0))];
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
      int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
#ifdef RT_RAYGEN_RAYS_MASKED
      if (active[fp.chunk_first + pix] != 0)
#endif
      {
        o4 = s_ray[lp * row + 2u * ls]; d4 = s_ray[lp * row + 2u * ls + 1u];
        traced = o4.w > 0.0f;  // (false for NaN)
      }
      const unsigned s = ps.s0 + sl;
      Pcg32 rng; rng.set_sequence(pixel_index * (unsigned long long)ps.spp + s + (1ull << 32));  // keyed per-sample stream, as k_raygen
      rng_state = rng.state;
      ps.lacc[pid] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(traced ? 0u : RT_STATE_OUT_OF_BOUNDS));
      ps.pfilm[pid] = has_pf ? s_pf[lp * prow + ls] : make_float2((float)x + 0.5f, (float)y + 0.5f);
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
    __syncthreads();  // (the next tile's records overwrite s_ray and s_pf)
  }
  for (int off = 32; off > 0; off >>= 1) n_camera += __shfl_down(n_camera, off);
  if ((threadIdx.x & 63u) == 0u && n_camera) atomicAdd(&ps.stats[ST_CAMERA], (unsigned long long)n_camera);
