// The body of k_trace and k_trace_spec (rtx_kernels.h), included where ANY, COUNT, BLOCK, DEPTH, GENERAL, MID and SPEC (the closest-hit link walk's form,
// closest_small_links) are compile-time constants and the kernel's arguments are in scope.
  // (plain loads and stores, no non-temporal hint: the scene is in LDS, the ray streams are all these launches read)
  const float4* __restrict__ ray_o = sraw(io.ray_o); const float4* __restrict__ ray_d = sraw(io.ray_d); const size_t rs = io.ray_stride;
  float4* __restrict__ hits = sraw(io.hits); const size_t hs = io.hit_stride; const bool hit_b2 = io.hit_b2 != 0;
  unsigned* __restrict__ occluded = io.occluded; const size_t os = io.occ_stride;
  float4* __restrict__ lacc = io.lacc; const size_t ls = io.lacc_stride; const float4* __restrict__ direct_add = sraw(io.direct_add); const size_t as = io.add_stride;
  // node indices of a tiny scene fit 16 bits: half the stack bytes => more resident waves per CU
  typedef unsigned short StackT;
  // LINKS: an LDS-resident scene's rays that do not count visits walk WITHOUT a stack over the link tables (closest_small_links, occluded_small_links[_rounds]) -
  // plain triangles, quadrics and masked triangles alike. Counting launches (the reference's walk, visit by visit) and HBM scenes keep the stack walk (traverse).
  constexpr bool LINKS = !COUNT;
  __shared__ StackT stack[LINKS ? 1 : DEPTH * BLOCK];
  constexpr int NN = MID ? RT_MID_NODES : RT_SMALL_NODES, NT = MID ? RT_MID_TRIS : RT_SMALL_TRIS;
  static_assert(!MID || (!COUNT && GENERAL == 0), "mid-size LDS scenes: plain triangles, no visit counts");
  constexpr bool MIDC = MID != 0 && !ANY;  // closest hit of a mid-size scene: six bound planes + eight link rows fill the LDS, the triangles stay in HBM
  typedef LdsSrcT<NN, NT> LdsS;
  __shared__ float s_nodes[(MIDC ? 6 : 8) * NN];
  __shared__ float s_tris[MIDC ? 1 : 10 * NT];
  QView qv; if (queue) qv.init(io.queue_is_slots ? nullptr : queue, shard_counts, shard_cap);
  const unsigned count = queue ? qv.total() : count_static;
  if (blockIdx.x * BLOCK >= count) return;  // short queues (MIS rays, late bounces): most blocks of the persistent grid have nothing to stage for
  __shared__ unsigned s_link[LINKS ? (ANY ? 1 : 8) * NN + 8 : 1];  // DScene::link8 (the tested nodes' links), rows NN apart, then the 8 start nodes
  stage_small_scene<BLOCK, NN, NT, MIDC>(sc, s_nodes, s_tris); __syncthreads();
  if (LINKS) {
    // DScene::link8: rows 0 - 7 (closest hit, by octant), their 8 starts, row 8 (occlusion rays), its start
    if (ANY) { for (unsigned k = threadIdx.x; k < sc.n_nodes; k += BLOCK) s_link[k] = sc.link8[8u * sc.n_nodes + 8u + k]; if (threadIdx.x == 0u) s_link[NN] = sc.link8[9u * sc.n_nodes + 8u]; }
    else {
      for (unsigned i = threadIdx.x; i < 8u * sc.n_nodes; i += BLOCK) { const unsigned o = i / sc.n_nodes, k = i - o * sc.n_nodes; s_link[o * NN + k] = sc.link8[i]; }
      if (threadIdx.x < 8u) s_link[8 * NN + threadIdx.x] = sc.link8[8u * sc.n_nodes + threadIdx.x];
    }
    __syncthreads();
  }
  const unsigned stride = gridDim.x * BLOCK;
  unsigned n_nodes = 0, n_tris = 0, n_rays = 0;
  auto trace_one = [&](unsigned pid) {
    float4 o4 = ray_o[pid * rs], d4 = ray_d[pid * rs];
    Ray ray; ray.o = mk3(o4.x, o4.y, o4.z); ray.d = mk3(d4.x, d4.y, d4.z); ray.t_max = o4.w;
    int prim = -1; TriHit h; h.t = kInf; h.b0 = h.b1 = h.b2 = 0.0f;
    bool found;
    constexpr int LM = ANY ? (MID ? RT_MID_LEAF_MIN_ANY : (GENERAL ? RT_LDS_LEAF_MIN_ANY_GENERAL : RT_LDS_LEAF_MIN_ANY)) : (MID ? RT_MID_LEAF_MIN_CLOSEST : (GENERAL ? RT_LDS_LEAF_MIN_CLOSEST_GENERAL : (SPEC ? RT_LDS_LEAF_MIN_SPEC : RT_LDS_LEAF_MIN_CLOSEST)));
    const GeneralCtx gen{sc.self, ANY && io.shadow_masks != 0};
    // Plain-triangle launches that do not count visits take the min / max node test (slab_test_finite) when every ray of the wave has a finite reciprocal
    // direction - all but a few hundred waves of a frame; a wave that holds one ray with a zero direction component walks with the reference's selects.
    constexpr bool FIN_FORMS = !COUNT;
    const bool fin = FIN_FORMS && __ballot(!inv_dir_finite(mk3(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z))) == 0ull;
    if (LINKS) {
      static_assert(!LINKS || ANY || (LM > 1 && LM < 64), "the closest-hit link walk tests its leaves in phases: 1 < LEAF_MIN < 64");
      if (!ANY) {
        if (fin) found = closest_small_links<NN, NT, true, LM, GENERAL, MIDC, SPEC>(s_nodes, s_tris, s_link, NN, (int)sc.n_nodes, ray, prim, h, gen, sc.tri_p);  // (s_link: 8 rows NN apart, the starts behind them)
        else found = closest_small_links<NN, NT, false, LM, GENERAL, MIDC>(s_nodes, s_tris, sc.link8_full, (int)sc.n_nodes, (int)sc.n_nodes, ray, prim, h, gen, sc.tri_p);
      } else if (LM > 1 && LM < 64) {
        found = fin ? occluded_small_links_rounds<NN, NT, true, LM, GENERAL>(s_nodes, s_tris, s_link, (int)sc.n_nodes, (int)s_link[NN], ray, gen)
                    : occluded_small_links_rounds<NN, NT, false, LM, GENERAL>(s_nodes, s_tris, sc.link8_full + 8u * sc.n_nodes + 8u, (int)sc.n_nodes, (int)sc.link8_full[9u * sc.n_nodes + 8u], ray, gen);
      } else {
        found = fin ? occluded_small_links<NN, NT, true, GENERAL>(s_nodes, s_tris, s_link, (int)sc.n_nodes, (int)s_link[NN], ray, gen)
                    : occluded_small_links<NN, NT, false, GENERAL>(s_nodes, s_tris, sc.link8_full + 8u * sc.n_nodes + 8u, (int)sc.n_nodes, (int)sc.link8_full[9u * sc.n_nodes + 8u], ray, gen);
      }
    }
    else {  // a frame that counts the reference's walk, visit by visit: the stack walk over the LDS copy
      LdsS src{s_nodes, s_tris};
      found = traverse<ANY, COUNT, LdsS, StackT, GENERAL>(src, ray, stack + threadIdx.x, BLOCK, prim, h, n_nodes, n_tris, gen);
    }
    n_rays += 1;
    if (ANY) trace_write_any(lacc, ls, direct_add, as, occluded, os, pid, d4.w, found);
    else hits[pid * hs] = make_float4(hit_b2 ? h.b2 : (found ? h.t : kInf), __int_as_float(found ? prim : -1), h.b0, h.b1);
    return found;
  };
  for (unsigned i = blockIdx.x * BLOCK + threadIdx.x; i < count; i += stride) {
    const bool found = trace_one(queue ? qv.get(i) : i);
    if constexpr (!ANY) {  // TraceIO::hit_mask: the wave's 64 entries (lanes past the queue's end are not here: their bits are zero), stored by its first lane
      if (io.hit_mask != nullptr) { const unsigned long long m = __ballot(found); if ((threadIdx.x & 63u) == 0u) io.hit_mask[i >> 6] = m; }
    } else (void)found;
  }
  if (stats) {
    // one atomic per wave and counter
    for (int off = 32; off > 0; off >>= 1) { n_rays += __shfl_down(n_rays, off); if (COUNT) { n_nodes += __shfl_down(n_nodes, off); n_tris += __shfl_down(n_tris, off); } }
    if ((threadIdx.x & 63u) == 0u) {
      if (n_rays) atomicAdd(&stats[st_rays], (unsigned long long)n_rays);
      if (COUNT) { atomicAdd(&stats[st_nodes], (unsigned long long)n_nodes); atomicAdd(&stats[st_tris], (unsigned long long)n_tris); }
    }
  }
