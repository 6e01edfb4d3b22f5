// The body of k_raygen and of k_raygen_masked (rtx_kernels.h includes it once for each): one lane per camera sample of the pass. Shared as text, not as a
// function, so that k_raygen compiles to the code it had before the masked kernel existed. RT_RAYGEN_MASKED: `active` is the byte mask of the adaptive step.
  const unsigned stride = gridDim.x * blockDim.x;
  const Tables tb = tables_of(ps);
  unsigned n_camera = 0;
  for (unsigned base = blockIdx.x * blockDim.x; base < ps.cap; base += stride) {
    const unsigned pid = base + threadIdx.x;
    bool in_bounds = false;
    CameraRay cr; unsigned long long rng_state = 0ull;
    if (pid < ps.cap) {
      unsigned sl, pix; split_path_id(ps, pid, sl, pix); const unsigned s = ps.s0 + sl;
      int x, y; unsigned long long pixel_index;
      owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
      in_bounds = y < fp.sb_y1 && x >= fp.pb_x0 && x < fp.pb_x1 && y >= fp.pb_y0 && y < fp.pb_y1;  // renderer.rs:103
#ifdef RT_RAYGEN_MASKED
      in_bounds &= active[fp.chunk_first + pix] != 0;
#endif
      // get_camera_sample (zerotwosequence.rs:182-192): 2D#0 film, 1D#0 time, 2D#1 lens
      f2 o = table_2d(tb, pix, 0, s);
      f2 p_film = mk2((float)x + o.x, (float)y + o.y);
      const f2 p_lens = fp.lens_radius > 0.0f ? table_2d(tb, pix, 1, s) : mk2(0.0f, 0.0f);  // (a pinhole camera never reads it, and a frame then does not build it: table_groups_frame)
      cr = generate_camera_ray(fp, p_film, p_lens, 1.0f / sqrtf((float)ps.spp));
      Pcg32 rng; rng.set_sequence(pixel_index * (unsigned long long)ps.spp + s + (1ull << 32));  // keyed per-sample stream
      rng_state = rng.state;
      ps.lacc[pid] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(in_bounds ? 0u : RT_STATE_OUT_OF_BOUNDS));
      ps.pfilm[pid] = make_float2(p_film.x, p_film.y);
    }
    n_camera += in_bounds ? 1u : 0u;
    unsigned slot = pid;  // every sample traced: path i is entry i is slot i
    if (!ps.all_in_bounds) {
      const int ci[1] = {0}; const bool pr[1] = {in_bounds}; unsigned sl_[1];
      block_push<1>(ps.cnt_out, ps.shard_cap, ci, pr, sl_);
      slot = sl_[0];
    }
    if (in_bounds) {  // the path's travelling records, at its slot of bounce 0's queue
      ps.out.o[slot] = make_float4(cr.o.x, cr.o.y, cr.o.z, kInf);
      ps.out.d[slot] = make_float4(cr.d.x, cr.d.y, cr.d.z, 0.0f);
      if (!RT_FRESH_BETA(ps)) ps.out.beta[slot] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);  // (left out: bounce 0 rebuilds the record from the slot, PassState::fresh)
      if (!RT_FRESH_ST(ps)) ps.out.st[slot] = make_uint4(pack_state(0, false, 1, 2), pid, (unsigned)rng_state, (unsigned)(rng_state >> 32));
    }
  }
  // camera samples actually generated: calls of PathIntegrator::li (samples outside pixel_bounds are skipped, renderer.rs:103)
  for (int off = 32; off > 0; off >>= 1) n_camera += __shfl_down(n_camera, off);
  if ((threadIdx.x & 63u) == 0u && n_camera) atomicAdd(&ps.stats[ST_CAMERA], (unsigned long long)n_camera);
