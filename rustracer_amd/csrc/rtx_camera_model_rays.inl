// The body of k_camera_model_rays and of k_camera_model_rays_masked (rtx_camera_models.h includes it once for each): k_camera_rays' loop with generate_model_ray in
// the place of generate_camera_ray. Shared as text, not as a function, so that the unmasked kernel holds no trace of the mask. RT_CAMERA_MODEL_MASKED: `active` is the
// byte mask of the adaptive step, by owned pixel.
// The camera sample is k_raygen's: p_film = pixel + 2D#0 of the pixel-keyed tables, p_lens = 2D#1 where the model has a lens. ray_s0 / ray_ns: first sample and samples
// per pixel of the arrays (the pass renders [ps.s0, ps.s0 + ps.n_samples) of them); rec4 = 5 stores the differentials, rec4 = 2 computes none. p_film_out may be NULL.
  const Tables tb = tables_of(ps);
  const unsigned stride = gridDim.x * blockDim.x;
  const float diff_scale = 1.0f / sqrtf((float)ps.spp);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < ps.cap; i += stride) {  // (ps.cap = n_pixels * n_samples <= 2^31 - 1)
    const unsigned pix = i / ps.n_samples, sl = i - pix * ps.n_samples, s = ps.s0 + sl;
#ifdef RT_CAMERA_MODEL_MASKED
    if (active[fp.chunk_first + pix] == 0) continue;
#endif
    int x, y; unsigned long long pixel_index; owned_pixel(fp, fp.chunk_first + pix, x, y, pixel_index);
    const f2 o = table_2d(tb, pix, 0, s);
    const f2 p_film = mk2((float)x + o.x, (float)y + o.y);
    const f2 p_lens = cm.lens_radius > 0.0f ? table_2d(tb, pix, 1, s) : mk2(0.0f, 0.0f);
    const size_t rec = (size_t)(pixel_index * ray_ns + (s - ray_s0));  // (< RT_RAYS_MAX: checked by the entry points)
    float4* r = rays + rec * rec4;
    if (rec4 == 5u) {
      const CameraRay cr = generate_model_ray<true>(cm, p_film, p_lens, diff_scale);
      r[0] = make_float4(cr.o.x, cr.o.y, cr.o.z, kInf);
      r[1] = make_float4(cr.d.x, cr.d.y, cr.d.z, 0.0f);
      r[2] = make_float4(cr.rx_o.x, cr.rx_o.y, cr.rx_o.z, cr.ry_o.x);
      r[3] = make_float4(cr.ry_o.y, cr.ry_o.z, cr.rx_d.x, cr.rx_d.y);
      r[4] = make_float4(cr.rx_d.z, cr.ry_d.x, cr.ry_d.y, cr.ry_d.z);
    } else {
      const CameraRay cr = generate_model_ray<false>(cm, p_film, p_lens, diff_scale);
      r[0] = make_float4(cr.o.x, cr.o.y, cr.o.z, kInf);
      r[1] = make_float4(cr.d.x, cr.d.y, cr.d.z, 0.0f);
    }
    if (p_film_out) p_film_out[rec] = make_float2(p_film.x, p_film.y);
  }
