// Host side of scene creation (rt_scene_create / rt_multi_create; included by rtx_hip.hip): everything that is a function of the scene description alone - every
// check of the description, the host records behind each device buffer of rt_scene, the code classes of the materials and the route flags the launch code picks
// kernels by. Nothing here touches the device, so a faulty description is refused with the same code and message on a machine without one; what needs the device
// (the CU count, the occupancy test of the mid-size kernels, the traversal stacks) stays in scene_from_plan.
#pragma once
#include <map>
#include <string>
#include "rtx_link_tables.h"  // (and the standard headers it includes)
#include "rtx_shadow_sets.h"
// (after rtx_kernels.h and `using namespace rtx`: the D* records and the RT_* limits)

struct RtScenePlan {
  // one host vector per device buffer (nodes, tri_n / tri_uv / tri_s / tri_alpha and spheres are uploaded from the description as they are)
  std::vector<float> tri_p;  // 48-byte triangle records: coordinates + meta in the w lanes
  std::vector<DInstance> instances;
  std::vector<float> texels; std::vector<DImage> images;  // tiled float4 texels of every MIP level; DImage::texels is set by the upload
  std::vector<uint32_t> fourier; std::vector<uint64_t> fourier_at;  // the Fourier tables' words; per image its first word there, or ~0 (a MIP pyramid)
  std::vector<DTexture> textures;  // the n_textures records, then the side records (word blocks, graph programs)
  std::vector<DMaterial> materials; std::vector<int> mat_kind, mat_table, mat_class;
  unsigned n_code_classes = 0, n_lambert_classes = 0, n_small_classes = 0, n_wide_classes = 0;
  std::vector<uint16_t> prim_class;
  // DLight::cf / func_int / mfunc / mcdf and guide / mguide of an infinite light hold offsets into dist / guides (rt_blob_offset) until the upload rebases them
  std::vector<DLight> lights; std::vector<float> dist; std::vector<unsigned short> guides;
  int n_infinite = 0, infinite_ids[4] = {0, 0, 0, 0};
  std::vector<float> pairs, top_pairs, quads;  // child-pair, top-of-tree and four-wide records (empty: not built)
  RtLinkTables links; RtShadowSets shadow;     // links: of a small or mid scene
  uint32_t n_top_nodes = 0, n_top_prims = 0, n_all_lights = 0;
  int stack_depth = 64, quad_stack_depth = 0, needs_differentials = 0, obj_pairs = 0, route_quadric_hits = 0;
  // the route flags, named as in rt_scene. mid is a candidate: the upload withdraws it, and the link tables, where the kernels do not fit the device
  bool small = false, mid = false, general_prims = false, obj_general = false, has_masks = false, has_spheres = false, has_instances = false, masked_emitters = false;
  bool lambert_only = false, lambert_materials = false, lean_shade = false, lean_qlights = false, lds_records = false, lds_records_q = false, lds_tables = false, lds_mats = false;
  bool use_pairs = false, use_top = false, top_for_closest = false, use_quads = false, deep_column = false, shadow_sets = false;
};

static int rt_refuse(std::string& why, int code, const std::string& msg) { why = msg; return code; }
template <class T> static const T* rt_blob_offset(size_t n) { return reinterpret_cast<const T*>(n * sizeof(T)); }
template <class T> static void rt_blob_rebase(const T*& p, const void* blob) { p = reinterpret_cast<const T*>((const char*)blob + reinterpret_cast<uintptr_t>(p)); }
static bool is_const_texture(const rt_scene_desc* desc, int id) { return id >= 0 && (uint32_t)id < desc->n_textures && desc->textures[id].kind == RT_TEX_CONST; }
// Guide tables (environment-map rows, light-distribution rows) bracket a CDF search: bucket k of 2^glog holds the entries whose cdf lies in [k, k+1) / 2^glog.
// Density in quarters of an entry per bucket on average: 4 = as many buckets as entries (the search that follows is 0-2 dependent loads instead of the 4-5 of
// round 2's 16 entries per bucket; a 2048 x 1024 map's tables grow from 0.3 to 4 MB).
static long guide_quarters() { return 4; }

// Is every quadric that carries an area light a Sphere (kind 0) that no triangle of the scene reaches into? Then a path vertex on a triangle lies outside
// every emitter sphere, and Sphere::sample_si / Sphere::pdf_wi (rc/shapes/sphere.rs:246-334) take their cone branches for it: `distance_squared(p_origin,
// p_center) <= radius^2` - the reference's own inside test, world-space distance against the object-space radius - is false with a margin of 1e-3 radius
// (p_origin is the vertex moved by its error bounds, orders of magnitude less). Exact point-triangle distances in double; gives up (false) beyond 2e8 pairs.
static bool sphere_lights_clear(const rt_scene_desc* desc) {
  std::vector<uint32_t> emitters;
  for (uint32_t i = 0; i < desc->n_lights; ++i) {
    const rt_light& l = desc->lights[i];
    if (l.kind != RT_LIGHT_DIFFUSE_AREA || l.prim < 0 || (uint32_t)l.prim >= desc->n_tris) continue;
    if (!(desc->tri_meta[l.prim].flags & RT_PRIM_SPHERE)) continue;
    uint32_t k; memcpy(&k, &desc->tri_p[9 * (size_t)l.prim + 6], 4);  // a quadric's leaf record: its index in p2.x
    if (k >= desc->n_spheres || desc->spheres[k].kind != 0) return false;
    emitters.push_back(k);
  }
  if ((double)emitters.size() * (double)desc->n_tris > 2e8) return false;
  for (uint32_t k : emitters) {
    const rt_sphere& sp = desc->spheres[k];
    const double c[3] = {sp.o2w[3], sp.o2w[7], sp.o2w[11]};
    const double r = (double)sp.radius * 1.001 + 1e-6 * std::max(std::max(fabs(c[0]), fabs(c[1])), fabs(c[2])), r2 = r * r;
    for (uint32_t t = 0; t < desc->n_tris; ++t) {
      if (desc->tri_meta[t].flags & (RT_PRIM_SPHERE | RT_PRIM_INSTANCE)) continue;
      const float* q = desc->tri_p + 9 * (size_t)t;
      // closest point of triangle (a, b, c) to p (Ericson, Real-Time Collision Detection 5.1.5), relative to p
      double a[3], b[3], cc[3];
      for (int j = 0; j < 3; ++j) { a[j] = q[j] - c[j]; b[j] = q[3 + j] - c[j]; cc[j] = q[6 + j] - c[j]; }
      auto dot3 = [](const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
      double ab[3], ac[3]; for (int j = 0; j < 3; ++j) { ab[j] = b[j] - a[j]; ac[j] = cc[j] - a[j]; }
      double best[3];
      const double d1 = -dot3(ab, a), d2 = -dot3(ac, a);
      const double d3 = -dot3(ab, b), d4 = -dot3(ac, b), d5 = -dot3(ab, cc), d6 = -dot3(ac, cc);
      const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
      if (d1 <= 0 && d2 <= 0) { for (int j = 0; j < 3; ++j) best[j] = a[j]; }
      else if (d3 >= 0 && d4 <= d3) { for (int j = 0; j < 3; ++j) best[j] = b[j]; }
      else if (vc <= 0 && d1 >= 0 && d3 <= 0) { const double v = d1 / (d1 - d3); for (int j = 0; j < 3; ++j) best[j] = a[j] + v * ab[j]; }
      else if (d6 >= 0 && d5 <= d6) { for (int j = 0; j < 3; ++j) best[j] = cc[j]; }
      else if (vb <= 0 && d2 >= 0 && d6 <= 0) { const double w = d2 / (d2 - d6); for (int j = 0; j < 3; ++j) best[j] = a[j] + w * ac[j]; }
      else if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) { const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); for (int j = 0; j < 3; ++j) best[j] = b[j] + w * (cc[j] - b[j]); }
      else { const double den = 1.0 / (va + vb + vc), v = vb * den, w = vc * den; for (int j = 0; j < 3; ++j) best[j] = a[j] + ab[j] * v + ac[j] * w; }
      if (!(dot3(best, best) > r2)) return false;  // (a NaN vertex fails too)
    }
  }
  return true;
}

// The scenes the shadow sets serve (rtx_shadow_sets.h): LDS-resident plain triangles (plain: no quadric, instance or mask) whose sampled lights are exactly two
// area lights on triangles - the light-distribution records then have a spare word per light (ld_rows8, k_lightdist_rows8). One light: the distribution is
// uniform (build_light_distribution), its single record is shared by every voxel and carries no per-voxel word.
#define RT_SHADOW_PLAIN_FLAGS (RT_TRI_FLIP | RT_TRI_HAS_N | RT_TRI_HAS_UV | RT_TRI_HAS_S)
static bool shadow_sets_apply(const rt_scene_desc* desc, bool plain) {
  if (!plain || desc->n_lights != 2 || !desc->lights) return false;
  for (uint32_t k = 0; k < desc->n_lights; ++k) {
    const rt_light& l = desc->lights[k];
    if (l.kind != 0 || l.prim < 0 || (uint32_t)l.prim >= desc->n_tris || (desc->tri_meta[l.prim].flags & ~(uint32_t)RT_SHADOW_PLAIN_FLAGS)) return false;
  }
  return true;
}

// Fourier BSDF tables (an rt_image with n_levels == 0, rtx_hip.h): what is wrong with one, or "" - then `words` is its length. Everything the device lobe
// (fourier_f / fourier_pdf / fourier_sample_f in rtx_dev_bsdf.h) indexes is checked here, so that no table can make it read outside its words.
#define RT_FOURIER_MAX_WORDS (1ull << 28)
static std::string fourier_table_error(const rt_image& im, uint64_t& words) {
  if (!im.texels) return "Fourier BSDF table without words";
  if (im.n_texels > RT_FOURIER_MAX_WORDS) return "Fourier BSDF table larger than 2^28 words";
  const uint64_t cap = 3 * im.n_texels;
  if (cap < 5) return "Fourier BSDF table shorter than its header";
  const uint32_t* w = (const uint32_t*)im.texels;
  const uint64_t n_mu = w[0], m_max = w[1], n_ch = w[2], n_coeffs = w[3];
  float eta; memcpy(&eta, &w[4], 4);
  if (n_mu < 2 || n_mu > 8192) return "Fourier BSDF table: nMu must lie in [2, 8192]";
  if (n_ch != 1 && n_ch != 3) return "Fourier BSDF table: nChannels must be 1 or 3";
  if (n_coeffs > RT_FOURIER_MAX_WORDS) return "Fourier BSDF table: nCoeffs larger than 2^28";
  if (!std::isfinite(eta)) return "Fourier BSDF table: eta is not finite";
  words = 5 + n_mu + 3 * n_mu * n_mu + n_coeffs;
  if ((words + 2) / 3 != im.n_texels) return "Fourier BSDF table: sizes do not add up (" + std::to_string(words) + " words for " + std::to_string(im.n_texels) + " texels)";
  const float* mu = (const float*)(w + 5);
  for (uint64_t i = 0; i < n_mu; ++i) if (!std::isfinite(mu[i]) || (i > 0 && !(mu[i - 1] < mu[i]))) return "Fourier BSDF table: mu is not strictly ascending";
  const uint32_t* ol = w + 5 + n_mu + n_mu * n_mu;
  for (uint64_t c = 0; c < n_mu * n_mu; ++c) {
    const uint64_t off = ol[2 * c], len = ol[2 * c + 1];
    if (len > m_max) return "Fourier BSDF table: a cell's length exceeds mMax";
    if (off + len * n_ch > n_coeffs) return "Fourier BSDF table: a cell's coefficients run past nCoeffs";
  }
  return "";
}
// The Fourier half of a scene description's checks: the tables, and every reference to an image that is one
static bool tex_mapped(int kind) { return kind == RT_TEX_CHECKER_PLANAR || kind == RT_TEX_FBM_MAPPED; }
// per image: whether a mapped texture (RT_TEX_CHECKER_PLANAR / RT_TEX_FBM_MAPPED) names it as its word block
static std::vector<char> word_blocks(const rt_scene_desc* desc) {
  std::vector<char> b(desc->images ? desc->n_images : 0, 0);
  for (uint32_t i = 0; i < desc->n_textures && desc->textures; ++i) {
    const rt_texture& t = desc->textures[i];
    if (tex_mapped(t.kind) && t.image >= 0 && (size_t)t.image < b.size()) b[t.image] = 1;
  }
  return b;
}
static std::string fourier_desc_error(const rt_scene_desc* desc) {
  const std::vector<char> block = word_blocks(desc);
  auto is_block = [&](int id) { return id >= 0 && (size_t)id < block.size() && block[id]; };
  auto is_table = [&](int id) { return id >= 0 && (uint32_t)id < desc->n_images && desc->images && desc->images[id].n_levels == 0 && !is_block(id); };
  uint64_t total = 0;
  for (uint32_t i = 0; i < desc->n_images; ++i) {
    if (!desc->images || desc->images[i].n_levels != 0 || is_block((int)i)) continue;
    uint64_t words = 0;
    const std::string why = fourier_table_error(desc->images[i], words);
    if (!why.empty()) return "image " + std::to_string(i) + ": " + why;
    total += words;
    if (total > RT_FOURIER_MAX_WORDS) return "Fourier BSDF tables larger than 2^28 words in all";
  }
  for (uint32_t i = 0; i < desc->n_materials && desc->materials; ++i) {
    const rt_material& m = desc->materials[i];
    if (m.kind == RT_MAT_FOURIER && is_block(m.slot[RT_SLOT_M1]))
      return "material " + std::to_string(i) + ": a Fourier material names the word block of a mapped texture, not a Fourier BSDF table";
    if (m.kind == RT_MAT_FOURIER && !is_table(m.slot[RT_SLOT_M1]))
      return "material " + std::to_string(i) + ": a Fourier material must name a Fourier BSDF table (n_levels == 0) in slot M1, not a MIP pyramid";
  }
  for (uint32_t i = 0; i < desc->n_textures && desc->textures; ++i)
    if (desc->textures[i].kind == RT_TEX_IMAGE && is_table(desc->textures[i].image)) return "texture " + std::to_string(i) + ": an image texture names a Fourier BSDF table, not a MIP pyramid";
  for (uint32_t i = 0; i < desc->n_textures && desc->textures; ++i)
    if (desc->textures[i].kind == RT_TEX_IMAGE && is_block(desc->textures[i].image)) return "texture " + std::to_string(i) + ": an image texture names the word block of a mapped texture, not a MIP pyramid";
  for (uint32_t i = 0; i < desc->n_lights && desc->lights; ++i) {
    if (desc->lights[i].kind == RT_LIGHT_INFINITE && is_table(desc->lights[i].image)) return "light " + std::to_string(i) + ": an infinite light names a Fourier BSDF table, not a MIP pyramid";
    if (desc->lights[i].kind == RT_LIGHT_INFINITE && is_block(desc->lights[i].image)) return "light " + std::to_string(i) + ": an infinite light names the word block of a mapped texture, not a MIP pyramid";
  }
  return "";
}

// ---- texture graphs (rtx_dev_shading.h, tex_eval_q / tex_eval_prog). Roots of the shapes the two-level evaluator takes - combinators of combinators of
// leaves, kinds 0-6, mix amounts leaves - keep it; every other texture that is no leaf gets a post-order program in side records behind the textures.
static bool tex_comb(int kind) { return kind == RT_TEX_SCALE || kind == RT_TEX_MIX || kind == RT_TEX_CHECKER || kind == RT_TEX_CHECKER_PLANAR; }
static int tex_n_ops(int kind) { return kind == RT_TEX_MIX ? 3 : (tex_comb(kind) ? 2 : 0); }
static int tex_op(const rt_texture& t, int k) { return k == 0 ? t.tex1 : (k == 1 ? t.tex2 : t.amount); }
static bool tex_two_level(const rt_scene_desc* desc, int id) {
  auto leaf = [&](int i) { const int k = desc->textures[i].kind; return k == RT_TEX_CONST || k == RT_TEX_IMAGE || k == RT_TEX_UV || k == RT_TEX_FBM; };
  auto depth1 = [&](int i) {  // a leaf, or a combinator of kinds 1, 2, 4 over leaves
    const rt_texture& t = desc->textures[i];
    if (leaf(i)) return true;
    if (t.kind != RT_TEX_SCALE && t.kind != RT_TEX_MIX && t.kind != RT_TEX_CHECKER) return false;
    for (int k = 0; k < tex_n_ops(t.kind); ++k) if (!leaf(tex_op(t, k))) return false;
    return true;
  };
  const rt_texture& t = desc->textures[id];
  if (t.kind != RT_TEX_SCALE && t.kind != RT_TEX_MIX && t.kind != RT_TEX_CHECKER) return t.kind <= RT_TEX_FBM;
  return depth1(t.tex1) && depth1(t.tex2) && (t.kind != RT_TEX_MIX || leaf(t.amount));
}
#define RT_TEX_PROGRAM_WORDS (1ull << 24)  // 64 MB of programs per scene at most
// Every check of the texture table, and the programs: side words to append behind the n_textures records (DTexture::image of texture i = side_at[i] / 12 +
// n_textures, or -1), and per texture the value slots its program needs. Returns what is wrong, or "".
static std::string texture_programs(const rt_scene_desc* desc, std::vector<int32_t>& side, std::vector<int64_t>& side_at, std::vector<int>& slots_of) {
  const uint32_t nt = desc->n_textures;
  if (nt && !desc->textures) return "texture table missing";
  auto ok = [&](int id) { return id >= 0 && (uint32_t)id < nt; };
  for (uint32_t i = 0; i < nt; ++i) {
    const rt_texture& t = desc->textures[i];
    const std::string who = "texture " + std::to_string(i) + ": ";
    if (t.kind < RT_TEX_CONST || t.kind > RT_TEX_FBM_MAPPED) return who + "unknown texture kind";
    for (int k = 0; k < tex_n_ops(t.kind); ++k) if (!ok(tex_op(t, k))) return who + (k == 2 ? "mix amount out of range" : "texture operand out of range");
    if (tex_mapped(t.kind)) {
      const uint64_t need = t.kind == RT_TEX_CHECKER_PLANAR ? 8 : 16;
      if (t.image < 0 || (uint32_t)t.image >= desc->n_images || !desc->images) return who + "word block image index out of range";
      const rt_image& im = desc->images[t.image];
      if (im.n_levels != 0) return who + "a mapped texture names a MIP pyramid, not a word block (n_levels == 0)";
      if (!im.texels || 3 * im.n_texels < need) return who + "word block shorter than " + std::to_string(need) + " words";
    }
  }
  // cycles (a C caller can build one; the reference cannot): depth-first over the operand edges, iteratively
  std::vector<char> color(nt, 0);  // 0 new, 1 on the path, 2 done
  std::vector<std::pair<int, int>> st;
  for (uint32_t r = 0; r < nt; ++r) {
    if (color[r]) continue;
    st.push_back({(int)r, 0}); color[r] = 1;
    while (!st.empty()) {
      const int v = st.back().first; const int k = st.back().second;
      const rt_texture& t = desc->textures[v];
      if (k < tex_n_ops(t.kind)) {
        ++st.back().second;
        const int u = tex_op(t, k);
        if (color[u] == 1) return "texture " + std::to_string(u) + ": the texture graph has a cycle";
        if (color[u] == 0) { color[u] = 1; st.push_back({u, 0}); }
      } else { color[v] = 2; st.pop_back(); }
    }
  }
  // Sethi-Ullman numbers over the combinators (leaves are evaluated in place and hold no slot): operands are visited heavier first
  std::vector<int> su(nt, 0);
  for (uint32_t r = 0; r < nt; ++r) {  // post-order again (acyclic now)
    if (su[r]) continue;
    st.push_back({(int)r, 0});
    while (!st.empty()) {
      const int v = st.back().first; const int k = st.back().second;
      const rt_texture& t = desc->textures[v];
      if (k < tex_n_ops(t.kind)) { ++st.back().second; const int u = tex_op(t, k); if (tex_comb(desc->textures[u].kind) && !su[u]) st.push_back({u, 0}); continue; }
      st.pop_back();
      if (!tex_comb(t.kind)) { su[v] = -1; continue; }  // (-1: a leaf, done)
      int c[3] = {-8, -8, -8};  // (a leaf operand holds no slot)
      for (int q = 0; q < tex_n_ops(t.kind); ++q) c[q] = su[tex_op(t, q)] > 0 ? su[tex_op(t, q)] : -8;
      std::sort(c, c + 3, std::greater<int>());
      su[v] = std::max(std::max(1, c[0]), std::max(c[1] + 1, c[2] + 2));
    }
  }
  auto ordered_ops = [&](const rt_texture& t, int* o) {  // operand indices 0 .. n-1, heavier first (stable)
    const int n = tex_n_ops(t.kind);
    for (int q = 0; q < n; ++q) o[q] = q;
    std::stable_sort(o, o + n, [&](int a, int b) { return std::max(su[tex_op(t, a)], 0) > std::max(su[tex_op(t, b)], 0); });
    return n;
  };
  std::vector<int> seen(nt, -1), last(nt, -1), slot_of(nt, -1), order;
  uint64_t total_words = 0;
  for (uint32_t r = 0; r < nt; ++r) {
    const rt_texture& root = desc->textures[r];
    std::vector<int32_t> words;
    int peak_slots = 0;
    if (root.kind == RT_TEX_CHECKER_PLANAR) { const float* w = desc->images[root.image].texels; for (int k = 0; k < 8; ++k) { int32_t b; memcpy(&b, &w[k], 4); words.push_back(b); } }
    if (root.kind == RT_TEX_FBM_MAPPED) { const float* w = desc->images[root.image].texels; for (int k = 0; k < 16; ++k) { int32_t b; memcpy(&b, &w[k], 4); words.push_back(b); } }
    if (tex_comb(root.kind) && !tex_two_level(desc, (int)r)) {
      words.resize(8, 0);
      // the combinators of the graph in post-order, each once
      order.clear();
      st.push_back({(int)r, 0}); seen[r] = (int)r;
      while (!st.empty()) {
        const int v = st.back().first; const int k = st.back().second;
        const rt_texture& t = desc->textures[v];
        int o[3]; const int n = ordered_ops(t, o);
        if (k < n) {
          ++st.back().second;
          const int u = tex_op(t, o[k]);
          if (tex_comb(desc->textures[u].kind) && seen[u] != (int)r) { seen[u] = (int)r; st.push_back({u, 0}); }
        } else { order.push_back(v); st.pop_back(); }
      }
      for (size_t j = 0; j < order.size(); ++j) {
        const rt_texture& t = desc->textures[order[j]];
        for (int q = 0; q < tex_n_ops(t.kind); ++q) last[tex_op(t, q)] = (int)j;
      }
      // value slots by linear scan: an operand's slot is free again once its last reader has read it
      std::vector<char> busy(RT_TEX_SLOTS + 1, 0); int peak = 0;
      words.push_back((int32_t)order.size());
      for (size_t j = 0; j < order.size(); ++j) {
        const rt_texture& t = desc->textures[order[j]];
        int32_t ref[3] = {0, 0, 0};
        for (int q = 0; q < tex_n_ops(t.kind); ++q) { const int u = tex_op(t, q); ref[q] = tex_comb(desc->textures[u].kind) ? -1 - slot_of[u] : u; }
        for (int q = 0; q < tex_n_ops(t.kind); ++q) { const int u = tex_op(t, q); if (tex_comb(desc->textures[u].kind) && last[u] == (int)j) busy[slot_of[u]] = 0; }
        int d = 0; while (d < RT_TEX_SLOTS && busy[d]) ++d;
        if (d == RT_TEX_SLOTS) {  // count what it would need, for the message
          int live = 0; for (size_t q = 0; q < j; ++q) if (last[order[q]] > (int)j) ++live;
          peak = std::max(peak, live + 1);
          return "texture " + std::to_string(r) + ": its graph needs at least " + std::to_string(peak) + " value slots, more than the " + std::to_string(RT_TEX_SLOTS) +
                 " (RT_TEX_SLOTS) of the device evaluator";
        }
        busy[d] = 1; slot_of[order[j]] = d; peak = std::max(peak, d + 1); peak_slots = peak;
        words.push_back(order[j]); words.push_back(d); words.push_back(ref[0]); words.push_back(ref[1]); words.push_back(ref[2]);
      }
    }
    slots_of.push_back(tex_comb(root.kind) && !tex_two_level(desc, (int)r) ? (int)peak_slots : 0);
    if (words.empty()) { side_at.push_back(-1); continue; }
    // every such root has a program over its whole sub-graph, so a chain of n nested combinators costs ~n^2 / 2 instructions: bounded here, by name
    total_words += (words.size() + 11) / 12 * 12;
    if (total_words > RT_TEX_PROGRAM_WORDS)
      return "texture " + std::to_string(r) + ": the scene's texture programs would exceed " + std::to_string(RT_TEX_PROGRAM_WORDS) + " words (graphs nested that deep are not supported)";
    side_at.push_back((int64_t)side.size());
    side.insert(side.end(), words.begin(), words.end());
    side.resize((side.size() + 11) / 12 * 12, 0);  // whole 48-byte records
  }
  return "";
}

// ---- the stages of rt_plan_scene, in the order of their checks
static int plan_geometry(const rt_scene_desc* desc, const std::vector<int>& tex_slots, RtScenePlan& p, std::string& why) {
  p.tri_p.resize((size_t)desc->n_tris * 12);
  for (size_t i = 0; i < desc->n_tris; ++i) {
    const float* t = desc->tri_p + 9 * i; const rt_tri_meta& m = desc->tri_meta[i];
    float* q = &p.tri_p[12 * i];
    q[0] = t[0]; q[1] = t[1]; q[2] = t[2]; memcpy(&q[3], &m.material, 4);
    q[4] = t[3]; q[5] = t[4]; q[6] = t[5]; memcpy(&q[7], &m.light, 4);
    q[8] = t[6]; q[9] = t[7]; q[10] = t[8]; memcpy(&q[11], &m.flags, 4);
    if ((m.flags & RT_TRI_HAS_N) && !desc->tri_n) return rt_refuse(why, RT_ERR_INVALID, "tri flags need tri_n");
    if ((m.flags & RT_TRI_HAS_UV) && !desc->tri_uv) return rt_refuse(why, RT_ERR_INVALID, "tri flags need tri_uv");
    if ((m.flags & RT_TRI_HAS_S) && !desc->tri_s) return rt_refuse(why, RT_ERR_INVALID, "tri flags need tri_s");
    if (m.flags & RT_PRIM_INSTANCE) {
      uint32_t k; memcpy(&k, t + 6, 4);
      if (!desc->instances || k >= desc->n_instances || i >= desc->n_top_prims) return rt_refuse(why, RT_ERR_INVALID, "instance index out of range");
      if (m.flags != RT_PRIM_INSTANCE || m.light >= 0) return rt_refuse(why, RT_ERR_INVALID, "an instance primitive carries triangle attributes or a light");
      continue;
    }
    if (m.material < 0 || (uint32_t)m.material >= desc->n_materials) return rt_refuse(why, RT_ERR_INVALID, "material index out of range");
    if (m.light >= (int)(desc->n_lights + desc->n_unlisted_lights)) return rt_refuse(why, RT_ERR_INVALID, "light index out of range");
    if (m.flags & (RT_TRI_HAS_ALPHA | RT_TRI_HAS_SHADOW_ALPHA)) {
      if (!desc->tri_alpha) return rt_refuse(why, RT_ERR_INVALID, "tri flags need tri_alpha");
      for (int k = 0; k < 2; ++k)
        if ((m.flags & (k == 0 ? RT_TRI_HAS_ALPHA : RT_TRI_HAS_SHADOW_ALPHA)) && (desc->tri_alpha[2 * i + k] < 0 || (uint32_t)desc->tri_alpha[2 * i + k] >= desc->n_textures))
          return rt_refuse(why, RT_ERR_INVALID, "alpha texture out of range");
      for (int k = 0; k < 2; ++k) {
        const int a = desc->tri_alpha[2 * i + k];
        if ((m.flags & (k == 0 ? RT_TRI_HAS_ALPHA : RT_TRI_HAS_SHADOW_ALPHA)) && tex_slots[a] > RT_TEX_MASK_SLOTS)
          return rt_refuse(why, RT_ERR_UNSUPPORTED, "alpha texture " + std::to_string(a) + ": its graph needs " + std::to_string(tex_slots[a]) + " value slots, more than the " +
                                                    std::to_string(RT_TEX_MASK_SLOTS) + " (RT_TEX_MASK_SLOTS) a mask has");
      }
      p.general_prims = true; p.has_masks = true;
    }
  }
  static_assert(sizeof(rt_sphere) == sizeof(DSphere), "rt_sphere and DSphere are the same record");
  for (size_t i = 0; i < desc->n_tris; ++i)
    if (desc->tri_meta[i].flags & RT_PRIM_SPHERE) {
      uint32_t k; memcpy(&k, desc->tri_p + 9 * i + 6, 4);
      if (!desc->spheres || k >= desc->n_spheres) return rt_refuse(why, RT_ERR_INVALID, "sphere index out of range");
      if (desc->tri_meta[i].flags & (RT_TRI_HAS_N | RT_TRI_HAS_UV | RT_TRI_HAS_S | RT_TRI_HAS_ALPHA | RT_TRI_HAS_SHADOW_ALPHA)) return rt_refuse(why, RT_ERR_INVALID, "a sphere primitive carries triangle attributes");
      p.has_spheres = true;
    }
  if (p.has_spheres) p.general_prims = true;
  const uint32_t n_top_nodes = p.n_top_nodes = desc->n_instances ? desc->n_top_nodes : desc->n_nodes, n_top_prims = p.n_top_prims = desc->n_instances ? desc->n_top_prims : desc->n_tris;
  if (desc->n_instances) {  // rt_instance -> DInstance: + the first hit id of each instance
    if (!desc->instances || n_top_nodes == 0 || n_top_nodes > desc->n_nodes || n_top_prims == 0 || n_top_prims > desc->n_tris) return rt_refuse(why, RT_ERR_INVALID, "bad instance tables");
    p.instances.resize(desc->n_instances);
    uint64_t id = n_top_prims;
    for (uint32_t k = 0; k < desc->n_instances; ++k) {
      const rt_instance& in = desc->instances[k];
      if (in.n_prims == 0 || (uint64_t)in.prim_base + in.n_prims > desc->n_tris || in.prim_base < n_top_prims || (in.n_nodes == 0 && in.n_prims != 1) ||
          (in.n_nodes != 0 && ((uint64_t)in.node_base + in.n_nodes > desc->n_nodes || in.node_base < n_top_nodes))) return rt_refuse(why, RT_ERR_INVALID, "instance ranges out of bounds");
      // An object holds triangles (masked or not) and quadrics (round 6: TransformedPrimitive wraps whatever the object definition collected, primitive.rs:79-118) - not
      // another instance (the reference's ObjectInstance inside an object definition is an error, api.rs:1056-1059), and no light of the scene's list (an emitter inside
      // an object is never a listed light, api.rs:954-964)
      for (uint32_t t = in.prim_base; t < in.prim_base + in.n_prims; ++t) {
        if ((desc->tri_meta[t].flags & RT_PRIM_INSTANCE) || (desc->tri_meta[t].light >= 0 && (uint32_t)desc->tri_meta[t].light < desc->n_lights))
          return rt_refuse(why, RT_ERR_UNSUPPORTED, "an instanced object holds triangles and quadrics only, and no light of the scene's list");
        if (desc->tri_meta[t].flags & (RT_PRIM_SPHERE | RT_TRI_HAS_ALPHA | RT_TRI_HAS_SHADOW_ALPHA)) p.obj_general = true;
      }
      DInstance& di = p.instances[k];
      memcpy(di.o2w, in.o2w, 64); memcpy(di.w2o, in.w2o, 64);
      di.node_base = in.node_base; di.n_nodes = in.n_nodes; di.prim_base = in.prim_base; di.n_prims = in.n_prims; di.id_base = (unsigned)id;
      id += in.n_prims;
      if (id >= (1ull << 31)) return rt_refuse(why, RT_ERR_UNSUPPORTED, "more than 2^31 instanced primitives");
    }
    p.has_instances = true; p.general_prims = true;
  }
  return RT_OK;
}

// images: one blob of float4 texels, every level cut into tiles of 4 x 2 texels = one 128-byte line (mip_texel in rtx_dev_shading.h): a bilinear
// or EWA footprint then touches fewer lines than with 12-byte row-major texels, and a texel is one aligned 16-byte load. The layout changes no value.
static int plan_images(const rt_scene_desc* desc, RtScenePlan& p, std::string& why) {
  p.images.resize(desc->n_images);
  p.fourier_at.assign(desc->n_images, ~0ull);
  auto is_pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
  size_t total = 0;  // in float4 texels, levels padded to whole tiles
  uint64_t fourier_words = 0;
  const std::vector<char> block = word_blocks(desc);
  std::vector<uint64_t> table_words(desc->n_images, 0);
  for (uint32_t i = 0; i < desc->n_images; ++i) {
    const rt_image& im = desc->images[i];
    if (im.n_levels == 0 && block[i]) continue;  // a mapped texture's word block: its words go to the texture side records (texture_programs)
    if (im.n_levels == 0) {  // a Fourier BSDF table (rtx_hip.h)
      (void)fourier_table_error(im, table_words[i]);  // (checked by fourier_desc_error)
      p.fourier_at[i] = fourier_words; fourier_words += table_words[i];
      continue;
    }
    if (im.n_levels < 0 || im.n_levels > RT_MAX_MIP_LEVELS) return rt_refuse(why, RT_ERR_INVALID, "bad mip level count");
    for (int l = 0; l < im.n_levels; ++l) {
      // MIPMap::new resamples to powers of two and halves from there (rc/mipmap.rs:75-139), which is what lets Repeat wrap by a mask
      if (!is_pow2(im.width[l]) || !is_pow2(im.height[l])) return rt_refuse(why, RT_ERR_INVALID, "MIP level sizes must be powers of two (rc/mipmap.rs:75-139)");
      if ((uint64_t)im.offset[l] + (uint64_t)im.width[l] * im.height[l] > im.n_texels) return rt_refuse(why, RT_ERR_INVALID, "MIP level outside the texel array");
      total += (size_t)std::max(im.width[l], 4) * std::max(im.height[l], 2);
    }
  }
  p.texels.assign((total + 1) * 4, 0.0f);
  p.fourier.assign((size_t)fourier_words + 1, 0u);
  size_t base = 0;
  for (uint32_t i = 0; i < desc->n_images; ++i) {
    const rt_image& im = desc->images[i];
    DImage& d = p.images[i];
    d.n_levels = im.n_levels; d.trilinear = im.trilinear; d.max_aniso = im.max_anisotropy; d.wrap = im.wrap; d.texels = nullptr;
    for (int l = 0; l < 16; ++l) { d.w[l] = 0; d.h[l] = 0; d.off[l] = 0; d.tshift[l] = 0; }
    if (im.n_levels == 0 && block[i]) continue;
    if (im.n_levels == 0) {  // table words as they are; material_lobes finds them at fourier + off[0]
      memcpy(&p.fourier[(size_t)p.fourier_at[i]], im.texels, (size_t)table_words[i] * 4);
      d.off[0] = p.fourier_at[i];
      continue;
    }
    for (int l = 0; l < im.n_levels; ++l) {
      const int w = im.width[l], h = im.height[l], pw = std::max(w, 4), ph = std::max(h, 2);
      int ts = 0; while ((4 << ts) < pw) ++ts;  // tiles per row = 2^ts
      d.w[l] = w; d.h[l] = h; d.off[l] = base; d.tshift[l] = ts;
      const float* src = im.texels + 3 * (size_t)im.offset[l];
      for (int t = 0; t < h; ++t)
        for (int x = 0; x < w; ++x) {
          const size_t idx = base + ((((size_t)(t >> 1) << ts) + (size_t)(x >> 2)) << 3) + (size_t)((t & 1) << 2) + (size_t)(x & 3);
          const float* q = src + 3 * ((size_t)t * w + x);
          float* o = &p.texels[idx * 4]; o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
        }
      base += (size_t)pw * ph;
    }
  }
  return RT_OK;
}

// the n_textures records, then the side records of the mapped textures and graph programs (texture_programs checked the table)
static int plan_textures(const rt_scene_desc* desc, const std::vector<int32_t>& tex_side, const std::vector<int64_t>& tex_side_at, RtScenePlan& p, std::string& why) {
  p.textures.resize(desc->n_textures + tex_side.size() / 12);
  for (uint32_t i = 0; i < desc->n_textures; ++i) {
    const rt_texture& t = desc->textures[i]; DTexture& d = p.textures[i];
    d.kind = t.kind; d.v[0] = t.value[0]; d.v[1] = t.value[1]; d.v[2] = t.value[2];
    d.tex1 = t.tex1; d.tex2 = t.tex2; d.amount = t.amount; d.image = t.image;
    d.su = t.mapping[0]; d.sv = t.mapping[1]; d.du = t.mapping[2]; d.dv = t.mapping[3];
    if (t.kind == RT_TEX_IMAGE && (t.image < 0 || (uint32_t)t.image >= desc->n_images)) return rt_refuse(why, RT_ERR_INVALID, "image index out of range");
    if (tex_comb(t.kind) || tex_mapped(t.kind)) d.image = tex_side_at[i] < 0 ? -1 : (int)(desc->n_textures + tex_side_at[i] / 12);  // (tex_eval_q reads it)
  }
  if (!tex_side.empty()) memcpy(&p.textures[desc->n_textures], tex_side.data(), tex_side.size() * 4);
  return RT_OK;
}

// matte with a constant sigma <= 0 (clamp(sigma, 0, 1) == 0: Lambert, not Oren-Nayar, matte.rs:51) and no bump map: what every Lambert route asks of a material
static bool sigma_zero_matte(const rt_scene_desc* desc, const rt_material& m) {
  return m.kind == RT_MAT_MATTE && m.bump < 0 && is_const_texture(desc, m.slot[RT_SLOT_SIGMA]) && desc->textures[m.slot[RT_SLOT_SIGMA]].value[0] <= 0.0f;
}
static int plan_materials(const rt_scene_desc* desc, RtScenePlan& p, std::string& why) {
  std::vector<DMaterial>& hmat = p.materials; hmat.resize(desc->n_materials);
  p.mat_kind.assign(desc->n_materials, 0); p.mat_table.assign(desc->n_materials, -1);
  for (uint32_t i = 0; i < desc->n_materials; ++i) {
    const rt_material& m = desc->materials[i];
    p.mat_kind[i] = m.kind;
    if (m.kind == RT_MAT_FOURIER) p.mat_table[i] = m.slot[RT_SLOT_M1];  // the table's image (fourier_desc_error checked it); no texture slot is read
    hmat[i].kind = m.kind; hmat[i].remap = m.remap_roughness;
    hmat[i].bump = (m.kind != RT_MAT_MIX && m.bump >= 0) ? m.bump : -1;
    if (hmat[i].bump >= 0 && (uint32_t)hmat[i].bump >= desc->n_textures) return rt_refuse(why, RT_ERR_INVALID, "bump texture out of range");
    for (int k = 0; k < 16; ++k) hmat[i].slot[k] = m.slot[k];
    if (m.kind == RT_MAT_MIX) {
      for (int side = 0; side < 2; ++side) {
        int c = m.slot[RT_SLOT_M1 + side];
        if (c < 0 || (uint32_t)c >= desc->n_materials) return rt_refuse(why, RT_ERR_INVALID, "mix operand out of range");
        if (desc->materials[c].kind == RT_MAT_MIX)
          for (int q = 0; q < 2; ++q) { int g = desc->materials[c].slot[RT_SLOT_M1 + q]; if (g < 0 || (uint32_t)g >= desc->n_materials || desc->materials[g].kind == RT_MAT_MIX) return rt_refuse(why, RT_ERR_INVALID, "mix nesting deeper than 2"); }
      }
    }
  }
  // code classes: materials of one kind (and roughness remap / bump presence) whose slots hold textures of the same shape run the same code
  std::map<std::vector<int>, int> classes;
  std::function<void(int, int, std::vector<int>&)> tex_sig = [&](int id, int depth, std::vector<int>& sig) {
    if (id < 0 || (uint32_t)id >= desc->n_textures) { sig.push_back(-1); return; }
    const rt_texture& t = desc->textures[id];
    sig.push_back(t.kind);
    if (t.kind == RT_TEX_CONST) sig.push_back(t.value[0] == 0.0f ? 0 : 1);  // sigma == 0 (Lambert, not Oren-Nayar), roughness == 0 (specular lobes), ...
    if (t.kind == RT_TEX_IMAGE) { const rt_image& im = desc->images[t.image]; sig.push_back(im.trilinear ? 1 : 0); }
    if (t.kind == RT_TEX_CHECKER || t.kind == RT_TEX_CHECKER_PLANAR) sig.push_back(t.amount);
    if (tex_comb(t.kind) && depth < 3) {
      tex_sig(t.tex1, depth + 1, sig); tex_sig(t.tex2, depth + 1, sig);
      if (t.kind == RT_TEX_MIX) tex_sig(t.amount, depth + 1, sig);
    } else if (tex_comb(t.kind)) sig.push_back(id);  // a graph deeper than that (only programs reach here): the sub-graph itself, not its shape
  };
  // an uber material whose opacity, Kr and Kt are constants with 1 - opacity, Kr and Kt black builds Lambert + microfacet reflection only (uber.rs:76-121)
  auto uber_two_lobes = [&](const rt_material& m) {
    auto konst = [&](int id) -> const rt_texture* { return is_const_texture(desc, id) ? &desc->textures[id] : nullptr; };
    const rt_texture *op = konst(m.slot[RT_SLOT_OPACITY]), *kr = konst(m.slot[RT_SLOT_KR]), *kt = konst(m.slot[RT_SLOT_KT]);
    if (!op || !kr || !kt) return false;
    for (int c = 0; c < 3; ++c) {
      const float o = std::max(op->value[c], 0.0f);
      if (!(std::max(1.0f - o, 0.0f) == 0.0f) || !std::isfinite(o) || !(std::max(kr->value[c], 0.0f) == 0.0f) || !(std::max(kt->value[c], 0.0f) == 0.0f)) return false;
    }
    return true;
  };
  std::function<void(int, int, std::vector<int>&)> mat_sig = [&](int id, int depth, std::vector<int>& sig) {
    const rt_material& m = desc->materials[id];
    sig.push_back(1000 + m.kind); sig.push_back(m.remap_roughness ? 1 : 0);
    for (int k = 0; k < RT_SLOT_M1; ++k) tex_sig(m.slot[k], 0, sig);
    if (m.kind == RT_MAT_MIX) { if (depth < 2) { mat_sig(m.slot[RT_SLOT_M1], depth + 1, sig); mat_sig(m.slot[RT_SLOT_M2], depth + 1, sig); } }
    else { sig.push_back(m.kind == RT_MAT_DISNEY ? m.slot[RT_SLOT_M1] : 0); tex_sig(m.bump, 0, sig); }
    if (m.kind == RT_MAT_UBER) sig.push_back(uber_two_lobes(m) ? 1 : 0);
  };
  for (uint32_t i = 0; i < desc->n_materials; ++i) {
    std::vector<int> sig; mat_sig((int)i, 0, sig);
    auto it = classes.find(sig);
    if (it == classes.end()) it = classes.emplace(sig, (int)classes.size()).first;
    hmat[i].code_class = it->second;
  }
  p.n_code_classes = (unsigned)classes.size();
  // the register-resident front-ends evaluate constants in place and image maps through tex_image_q; a material with any other texture shape in a slot
  // (scale / mix / checkerboard / uv / fbm) is shaded by the generic kernel, whose evaluator handles them all
  auto leaf_slots = [&](const rt_material& m) {
    for (int k = 0; k < RT_SLOT_M1; ++k) {
      const int id = m.slot[k];
      if (id < 0 || (uint32_t)id >= desc->n_textures) continue;
      if (desc->textures[id].kind != RT_TEX_CONST && desc->textures[id].kind != RT_TEX_IMAGE) return false;
    }
    return true;
  };
  // classes the register-resident front-end can shade (matte, sigma == 0, no bump, Kd any texture: SingleLambertT) get the lowest ids, so that after binning they
  // are one contiguous range of the queue; then the classes of the two-lobe front-end (SmallBsdfT<false>): matte with sigma > 0, plastic, metal, mirror; then of
  // its wide form: glass, substrate, opaque uber; no bump map
  std::vector<int> lambert(classes.size(), 0), small(classes.size(), 0), wide(classes.size(), 0), remap(classes.size(), -1);
  for (uint32_t i = 0; i < desc->n_materials; ++i) {
    const rt_material& m = desc->materials[i]; const int c = hmat[i].code_class;
    lambert[c] = sigma_zero_matte(desc, m) && m.slot[RT_SLOT_KD] >= 0 && leaf_slots(m);
    small[c] = !lambert[c] && m.bump < 0 && leaf_slots(m) && (m.kind == RT_MAT_MATTE || m.kind == RT_MAT_PLASTIC || m.kind == RT_MAT_METAL || m.kind == RT_MAT_MIRROR);
    wide[c] = m.bump < 0 && leaf_slots(m) && (m.kind == RT_MAT_GLASS || m.kind == RT_MAT_SUBSTRATE || (m.kind == RT_MAT_UBER && uber_two_lobes(m)));
  }
  int next = 0;
  for (size_t c = 0; c < classes.size(); ++c) if (lambert[c]) remap[c] = next++;
  p.n_lambert_classes = (unsigned)next;
  for (size_t c = 0; c < classes.size(); ++c) if (small[c]) remap[c] = next++;
  p.n_small_classes = (unsigned)next - p.n_lambert_classes;
  for (size_t c = 0; c < classes.size(); ++c) if (wide[c]) remap[c] = next++;
  p.n_wide_classes = (unsigned)next - p.n_lambert_classes - p.n_small_classes;
  for (size_t c = 0; c < classes.size(); ++c) if (!lambert[c] && !small[c] && !wide[c]) remap[c] = next++;
  p.mat_class.resize(desc->n_materials);
  for (uint32_t i = 0; i < desc->n_materials; ++i) p.mat_class[i] = hmat[i].code_class = remap[hmat[i].code_class];
  // per primitive: the code class of its material (bit 15: a quadric) - what the vertex queue is binned by (k_bin_count), ONE two-byte gather instead of the primitive's
  // 128-byte shade record and then its material (round 6)
  p.prim_class.assign(desc->n_tris, 0);
  for (size_t i = 0; i < desc->n_tris; ++i) {
    const rt_tri_meta& m = desc->tri_meta[i];
    if (m.flags & RT_PRIM_INSTANCE) continue;
    const int c = (m.material >= 0 && (uint32_t)m.material < desc->n_materials) ? hmat[m.material].code_class : 0;
    p.prim_class[i] = (uint16_t)(std::min(c, 0x7ffe) | ((m.flags & RT_PRIM_SPHERE) ? 0x8000 : 0));
  }
  return RT_OK;
}

// lights: sampled lights, then the emitters no light list holds; the environment maps' distributions in one blob, the guide tables of their CDF searches
// (DLight::guide: 2^glog buckets per row, guide_quarters) in another
static int plan_lights(const rt_scene_desc* desc, RtScenePlan& p, std::string& why) {
  const uint32_t n_all_lights = p.n_all_lights = desc->n_lights + desc->n_unlisted_lights;
  p.lights.resize(n_all_lights);
  auto guide_log = [](int n) { const long q = guide_quarters(); int g = 0; while (g < 16 && (long)(2 << g) * q <= 4l * n) ++g; return g; };
  auto guide_row = [](const float* cdf, int n, int glog, unsigned short* out) {  // out[k] = #{i in [0, n] : cdf[i] <= k / 2^glog}
    const int G = 1 << glog; int i = 0;
    for (int k = 0; k <= G; ++k) { const float x = (float)k / (float)G; while (i <= n && cdf[i] <= x) ++i; out[k] = (unsigned short)i; }
  };
  size_t total = 0, guide_total = 0;
  for (uint32_t i = 0; i < n_all_lights; ++i) {
    const rt_light& l = desc->lights[i];
    if (l.kind != RT_LIGHT_INFINITE) continue;
    if (l.dist_nu < 1 || l.dist_nv < 1 || l.dist_nu > 65534 || l.dist_nv > 65534 || !l.dist_cdf || !l.marg_cdf) return rt_refuse(why, RT_ERR_INVALID, "infinite light tables missing or larger than 65534 entries per row");
    total += 2 * (size_t)l.dist_nv * (l.dist_nu + 1) + (size_t)l.dist_nv * 3 + 1;
    guide_total += (size_t)l.dist_nv * ((1u << guide_log(l.dist_nu)) + 1) + ((1u << guide_log(l.dist_nv)) + 1);
  }
  std::vector<float>& blob = p.dist; blob.assign(total + 4, 0.0f);
  std::vector<unsigned short>& gblob = p.guides; gblob.assign(guide_total + 1, 0);
  size_t base = 0, gbase = 0; int n_inf = 0;
  for (uint32_t i = 0; i < n_all_lights; ++i) {
    const rt_light& l = desc->lights[i]; DLight& d = p.lights[i];
    memset(&d, 0, sizeof(d));
    d.kind = l.kind; d.prim = l.prim; d.rgb[0] = l.rgb[0]; d.rgb[1] = l.rgb[1]; d.rgb[2] = l.rgb[2]; d.two_sided = l.two_sided;
    d.vec[0] = l.vec[0]; d.vec[1] = l.vec[1]; d.vec[2] = l.vec[2]; d.area = l.area; d.world_radius = l.world_radius; d.image = l.image;
    memcpy(d.l2w, l.l2w, 48); memcpy(d.w2l, l.w2l, 48);
    if (l.kind == RT_LIGHT_DIFFUSE_AREA && (l.prim < 0 || (uint32_t)l.prim >= desc->n_tris)) return rt_refuse(why, RT_ERR_INVALID, "area light prim out of range");
    if (i >= desc->n_lights && l.kind != RT_LIGHT_DIFFUSE_AREA) return rt_refuse(why, RT_ERR_INVALID, "an unlisted emitter must be a diffuse area light");
    if (l.kind != RT_LIGHT_INFINITE) continue;
    if (n_inf >= 4) return rt_refuse(why, RT_ERR_INVALID, "more than 4 infinite lights");
    if (l.image < 0 || (uint32_t)l.image >= desc->n_images) return rt_refuse(why, RT_ERR_INVALID, "infinite light image out of range");
    p.infinite_ids[n_inf++] = (int)i;
    d.nu = l.dist_nu; d.nv = l.dist_nv; d.mfunc_int = l.marg_func_int;
    d.cf = rt_blob_offset<float>(base);  // (cdf, func) pairs, nu + 1 per row
    for (int r = 0; r < l.dist_nv; ++r)
      for (int k = 0; k <= l.dist_nu; ++k) {
        blob[base++] = l.dist_cdf[(size_t)r * (l.dist_nu + 1) + k];
        blob[base++] = k < l.dist_nu ? l.dist_func[(size_t)r * l.dist_nu + k] : 0.0f;
      }
    memcpy(&blob[base], l.dist_func_int, (size_t)l.dist_nv * 4); d.func_int = rt_blob_offset<float>(base); base += l.dist_nv;
    memcpy(&blob[base], l.marg_func, (size_t)l.dist_nv * 4); d.mfunc = rt_blob_offset<float>(base); base += l.dist_nv;
    memcpy(&blob[base], l.marg_cdf, ((size_t)l.dist_nv + 1) * 4); d.mcdf = rt_blob_offset<float>(base); base += (size_t)l.dist_nv + 1;
    d.glog = guide_log(l.dist_nu); d.mglog = guide_log(l.dist_nv);
    const size_t gw = ((size_t)1 << d.glog) + 1;
    d.guide = rt_blob_offset<unsigned short>(gbase);
    for (int r = 0; r < l.dist_nv; ++r) guide_row(l.dist_cdf + (size_t)r * (l.dist_nu + 1), l.dist_nu, d.glog, &gblob[gbase + (size_t)r * gw]);
    gbase += (size_t)l.dist_nv * gw;
    d.mguide = rt_blob_offset<unsigned short>(gbase);
    guide_row(l.marg_cdf, l.dist_nv, d.mglog, &gblob[gbase]);
    gbase += ((size_t)1 << d.mglog) + 1;
  }
  p.n_infinite = n_inf;
  return RT_OK;
}

// which kernels a frame of this scene launches (launch_trace_c, shade_route, render_frame read these flags off rt_scene)
static void plan_route(const rt_scene_desc* desc, RtScenePlan& p) {
  bool all_const_textures = true, all_area_lights = true;
  for (uint32_t i = 0; i < desc->n_textures; ++i) {
    const rt_texture& t = desc->textures[i];
    if (t.kind != RT_TEX_CONST) all_const_textures = false;
    if (t.kind == RT_TEX_IMAGE || t.kind == RT_TEX_FBM || t.kind == RT_TEX_FBM_MAPPED || ((t.kind == RT_TEX_CHECKER || t.kind == RT_TEX_CHECKER_PLANAR) && t.amount != 0))
      p.needs_differentials = 1;
  }
  p.lambert_only = true;       // every material is matte{constant Kd, sigma == 0}
  p.lambert_materials = true;  // the same with Kd a constant or an image: what k_shade<3> evaluates (tex_eval_leaf)
  for (uint32_t i = 0; i < desc->n_materials; ++i) {
    const rt_material& m = desc->materials[i];
    if (m.kind != RT_MAT_MIX && m.bump >= 0) p.needs_differentials = 1;  // bump() reads dudx..
    const int kd = m.slot[RT_SLOT_KD];
    const bool kd_leaf = kd >= 0 && (uint32_t)kd < desc->n_textures && (desc->textures[kd].kind == RT_TEX_CONST || desc->textures[kd].kind == RT_TEX_IMAGE);
    if (!sigma_zero_matte(desc, m) || !is_const_texture(desc, kd)) p.lambert_only = false;
    if (!sigma_zero_matte(desc, m) || !kd_leaf) p.lambert_materials = false;
  }
  for (uint32_t i = 0; i < desc->n_lights; ++i) {
    if (desc->lights[i].kind != RT_LIGHT_DIFFUSE_AREA) all_area_lights = false;
    else if (desc->tri_meta[desc->lights[i].prim].flags & RT_TRI_HAS_ALPHA) p.masked_emitters = true;
  }
  if (p.has_spheres || p.has_instances) p.masked_emitters = true;  // quadric / instance hits, quadric emitters, masked emitters: the GENERAL instantiations of the shade kernels
  p.lean_shade = !p.masked_emitters && all_area_lights && all_const_textures;
  // The LEAN forms with sphere lights (QLIGHTS): constant textures, every light a diffuse area light on a triangle or on a Sphere that no triangle reaches
  // into, no masks, no instances. Vertices on quadrics are binned apart and shaded by the generic GENERAL kernel (route_quadric_hits), so the scene must be
  // one whose shade queue is binned (several material classes - rt_render checks that).
  p.lean_qlights = p.has_spheres && !p.has_instances && !p.has_masks && all_area_lights && all_const_textures && sphere_lights_clear(desc);
  // (the constant-matte kernel has no GENERAL form: such scenes shade through the Lambert front-end k_shade<3, true>)
  if (!all_area_lights || p.masked_emitters) p.lambert_only = false;
  p.route_quadric_hits = (p.lean_qlights && p.n_code_classes > 1 && !p.lambert_materials) ? 1 : 0;  // (the condition of rt_render's use_bins)
  p.small = desc->n_nodes <= RT_SMALL_NODES && desc->n_tris <= RT_SMALL_TRIS && !p.has_instances;  // quadrics and masked triangles: the GENERAL form of the LDS kernel
  // mid-size scenes (round 5): too large for the 256-node LDS kernels, small enough for one workgroup's 160 KB - occlusion rays walk link tables in LDS (k_trace<.., MID>)
  p.mid = !p.small && !p.general_prims && !p.has_instances && desc->n_nodes <= RT_MID_NODES && desc->n_tris <= RT_MID_TRIS;
  for (uint32_t i = 0; i < desc->n_nodes && p.mid; ++i) if (desc->nodes[i].n_prims > 15) p.mid = false;  // (the link word's count field)
  // what fits the shade kernels' LDS (RTX_SHADE_LDSREC=0, measurement knob read per scene: nothing): the material and texture tables (the LEAN forms); with them the
  // lights and image headers (the plain forms); the triangles, lights, materials and textures of a scene of quadric emitters (QLIGHTS forms with LDSREC = 1); the
  // shade / traversal records and the light table of an LDS-resident scene (k_shade<1, .., LDSREC>)
  const char* ldsrec = getenv("RTX_SHADE_LDSREC");
  p.lds_mats = desc->n_materials <= RT_LDS_MATERIALS && desc->n_textures <= RT_LDS_TEXTURES && !(ldsrec && ldsrec[0] == '0');
  p.lds_tables = p.lds_mats && p.n_all_lights <= RT_LDS_LIGHTS && desc->n_images <= RT_LDS_IMAGES;
  p.lds_records_q = p.lds_mats && p.n_all_lights <= RT_LDS_LIGHTS && desc->n_tris <= RT_SMALL_TRIS && !p.has_instances;
  p.lds_records = p.lds_records_q && p.small && !p.has_spheres;
}

// child-pair record of k_trace_pair: {A.min.xyz, A.max.x} {A.max.yz, code A, code B} {B.min.xyz, B.max.x} {B.max.yz, -, -}
static void pair_record(const rt_bvh_node& a, const rt_bvh_node& b, uint32_t ca, uint32_t cb, float* q) {
  q[0] = a.bmin[0]; q[1] = a.bmin[1]; q[2] = a.bmin[2]; q[3] = a.bmax[0]; q[4] = a.bmax[1]; q[5] = a.bmax[2]; memcpy(q + 6, &ca, 4); memcpy(q + 7, &cb, 4);
  q[8] = b.bmin[0]; q[9] = b.bmin[1]; q[10] = b.bmin[2]; q[11] = b.bmax[0]; q[12] = b.bmax[1]; q[13] = b.bmax[2];
}
// the trees: their checks and stack depths, the LDS walks' link tables and the shadow sets of the scenes that have them, the traversal records of the others
static int plan_trees(const rt_scene_desc* desc, RtScenePlan& p, std::string& why) {
  const uint32_t n_top_nodes = p.n_top_nodes, n_top_prims = p.n_top_prims;
  // tree height bounds the number of simultaneously pending stack entries
  // one tree: nodes [base, base + nn), child offsets relative to base, leaf ranges within its np primitives
  auto tree_depth = [&](uint32_t base, uint32_t nn, uint32_t np, int& maxd) -> bool {
    std::vector<int> depth(nn, 0); maxd = 0;
    for (uint32_t i = 0; i < nn; ++i) {
      const rt_bvh_node& n = desc->nodes[base + i];
      if (n.n_prims == 0) {
        if (i + 1 >= nn || n.offset >= nn || n.offset <= i) return false;
        depth[i + 1] = depth[i] + 1; depth[n.offset] = depth[i] + 1;
      } else if ((uint64_t)n.offset + n.n_prims > np) return false;
      if (depth[i] > maxd) maxd = depth[i];
    }
    return true;
  };
  int maxd = 0;
  if (!tree_depth(0, n_top_nodes, n_top_prims, maxd)) return rt_refuse(why, RT_ERR_INVALID, "malformed BVH");
  if (maxd + 1 > 64) return rt_refuse(why, RT_ERR_INVALID, "BVH deeper than the 64-entry traversal stack");
  int max_obj_depth = 0;
  for (uint32_t k = 0; k < desc->n_instances; ++k) {
    const rt_instance& in = desc->instances[k];
    int od = 0;
    if (in.n_nodes && (!tree_depth(in.node_base, in.n_nodes, in.n_prims, od) || od + 1 > 64)) return rt_refuse(why, RT_ERR_INVALID, "malformed or too deep object BVH");
    if (in.n_nodes) max_obj_depth = std::max(max_obj_depth, od + 1);
  }
  // an object's walk uses the entries of the lane's stack column above the top level's pending ones: the column holds both
  // The reference gives each BVH a 64-entry stack of its own (bvh/mod.rs:374), so a 36-deep top level over a 30-deep object is a valid scene: past 64 entries
  // in one column the scene is traced by the one-node-per-step kernel with a 128-entry column (k_trace_big<.., 64, 128>; no pair / four-wide records)
  p.stack_depth = maxd + 1 + max_obj_depth;
  p.deep_column = p.stack_depth > 64;
  // link tables (round 5: per octant and node where the stackless walk goes on, over all nodes and over the nodes a calibration on
  // synthetic path rays found worth testing): rtx_link_tables.h
  if (p.small || p.mid) rt_build_link_tables(desc, p.mid, false, p.links);
  const char* sets = getenv("RTX_SHADOW_SETS");  // (measurement knob, read per scene: 0 = every segment walks)
  if (shadow_sets_apply(desc, p.small && !p.general_prims && !p.has_instances) && !(sets && sets[0] == '0')) {
    int32_t lp[2] = {0, 0};
    for (uint32_t k = 0; k < desc->n_lights; ++k) lp[k] = desc->lights[k].prim;
    rt_build_shadow_sets(desc->tri_p, desc->n_tris, lp, (int)desc->n_lights, desc->nodes[0].bmin, desc->nodes[0].bmax, p.shadow);
    p.shadow_sets = p.shadow.empty > 0;
  }
  if (p.small || p.deep_column) return RT_OK;  // LDS-resident scenes keep the one-node-per-step loop: the pair form measured no faster there
  // With object instances the records cover the top-level tree (objects are walked one node per step, their child offsets are relative to the object).
  // A leaf of a GENERAL scene that holds anything but plain triangles carries RT_PAIR_GENERAL.
  const uint32_t n_pair_nodes = n_top_nodes;
  const bool gen = p.general_prims;
  auto general_leaf = [&](const rt_bvh_node& n) {
    for (uint32_t t = n.offset; t < n.offset + n.n_prims; ++t)
      if (desc->tri_meta[t].flags & (RT_TRI_HAS_ALPHA | RT_TRI_HAS_SHADOW_ALPHA | RT_PRIM_SPHERE | RT_PRIM_INSTANCE)) return true;
    return false;
  };
  // (a root that is itself a leaf - every centroid coincides - is never seen by a child code: its count must fit the 5-bit field too)
  bool ok = n_pair_nodes < (1u << 29) && n_top_prims < (gen ? (1u << 25) : (1u << 26)) && desc->nodes[0].n_prims <= 32;
  // a child's code: node `c` of the tree at `base` (0: the top level, whose leaves may be general; an object's codes are LOCAL to it - node indices and leaf ranges
  // are relative to the object's bases in its flattened tree already - and its records serve plain triangles: nested_pair_walk)
  auto code_of = [&](uint32_t base, uint32_t c, bool& good) -> uint32_t {
    const rt_bvh_node& n = desc->nodes[base + c];
    if (n.n_prims > 0) { if (n.n_prims > 32) good = false; return 0x80000000u | n.offset | ((uint32_t)(n.n_prims - 1) << 26) | (base == 0 && gen && general_leaf(n) ? RT_PAIR_GENERAL : 0u); }
    return c | ((uint32_t)n.axis << 29);
  };
  auto pair_tree = [&](uint32_t base, uint32_t nn, bool& good) {  // records at the nodes' global indices
    for (uint32_t i = 0; i < nn && good; ++i) {
      const rt_bvh_node& n = desc->nodes[base + i];
      if (n.n_prims != 0) continue;
      const uint32_t ca = code_of(base, i + 1, good), cb = code_of(base, n.offset, good);
      pair_record(desc->nodes[base + i + 1], desc->nodes[base + n.offset], ca, cb, p.pairs.data() + (size_t)(base + i) * 16);
    }
  };
  p.pairs.assign((size_t)(p.has_instances ? desc->n_nodes : n_pair_nodes) * 16, 0.0f);  // (with instances: the objects' records behind the top level's)
  pair_tree(0, n_pair_nodes, ok);
  bool obj_ok = ok && p.has_instances;  // the objects' trees as child pairs as well, each tree once
  if (obj_ok) {
    std::vector<char> done(desc->n_nodes, 0);
    for (uint32_t k = 0; k < desc->n_instances && obj_ok; ++k) {
      const rt_instance& in = desc->instances[k];
      if (in.n_nodes == 0 || done[in.node_base]) continue;
      done[in.node_base] = 1;
      if (in.n_nodes >= (1u << 29) || in.n_prims >= (1u << 26) || desc->nodes[in.node_base].n_prims > 32) { obj_ok = false; break; }
      pair_tree(in.node_base, in.n_nodes, obj_ok);
    }
  }
  if (!ok) { p.pairs.clear(); return RT_OK; }
  p.use_pairs = true;
  p.obj_pairs = (obj_ok && !p.obj_general) ? 1 : 0;  // (nested_pair_walk tests plain triangles only)
  if (n_pair_nodes < (1u << 28) && desc->nodes[0].n_prims == 0 && !p.has_instances) {  // (an object's walk needs a contiguous stack column: k_trace_pair)
    // the first levels of the tree, breadth first, for k_trace_top: up to RT_TOP_MAX interior nodes; a child that is itself one of them is named by its slot
    std::vector<uint32_t> top; std::vector<int> slot_of(n_pair_nodes, -1);
    top.push_back(0); slot_of[0] = 0;
    for (size_t head = 0; head < top.size(); ++head) {
      const uint32_t P = top[head]; const uint32_t kids[2] = {P + 1, desc->nodes[P].offset};
      for (uint32_t c : kids)
        if (desc->nodes[c].n_prims == 0 && top.size() < RT_TOP_MAX) { slot_of[c] = (int)top.size(); top.push_back(c); }
    }
    p.top_pairs.assign(top.size() * 16, 0.0f);
    for (size_t k = 0; k < top.size(); ++k) {
      uint32_t code[2]; memcpy(code, p.pairs.data() + (size_t)top[k] * 16 + 6, 8);
      for (int side = 0; side < 2; ++side)
        if (!(code[side] & 0x80000000u) && slot_of[code[side] & 0x0fffffffu] >= 0) code[side] = (code[side] & 0x60000000u) | RT_PAIR_TOP | (uint32_t)slot_of[code[side] & 0x0fffffffu];
      pair_record(desc->nodes[top[k] + 1], desc->nodes[desc->nodes[top[k]].offset], code[0], code[1], p.top_pairs.data() + 16 * k);
    }
    p.use_top = true;
    // Measured (scripts/ab_bench.sh, one box; k_trace_top vs k_trace_pair): shadow rays -9 % (S2) .. -12 % (S4); closest-hit rays -8 % on S4 (25 MB of
    // pair records), +2 % on S3 (83 KB: L1-resident either way) and +6 % on S2 (128 MB: a sixth wave per SIMD evicts more of the tree from L2 than
    // it hides). 64, 128 or 256 LDS-resident nodes measured the same: the top of the tree was already served by the CU's L1 - what the kernel
    // gains is its sixth wave per SIMD, and that pays where the tree fits the 32 MB of L2 without fitting an L1.
    const size_t pair_bytes = (size_t)n_pair_nodes * 64;
    p.top_for_closest = pair_bytes <= ((size_t)64 << 20);  // measured with the gated leaf phase: S3 (0.1 MB) 81 -> 78 ms, S4 (13 MB) 1743 -> 1659 ms, S2 (67 MB) 94 -> 102 ms
  }
  // four-wide records for the any-hit kernel (k_trace_quad): an interior node's grandchildren (a leaf child stands for itself), 128 B
  // per node: 24 floats = boxes of slots 0..3 (slots 0,1: first child's part, 2,3: second child's), 4 codes (0xffffffff = empty slot),
  // {axis of the first child | axis of the second child << 2}.
  std::vector<float>& qr = p.quads; qr.assign((size_t)n_pair_nodes * 32, 0.0f);
  std::vector<int> need(n_pair_nodes, 0);  // stack entries the four-wide walk can have pending below this node
  for (uint32_t i = n_pair_nodes; i-- > 0;) {
    const rt_bvh_node& n = desc->nodes[i];
    if (n.n_prims != 0) continue;
    float* q = qr.data() + (size_t)i * 32;
    uint32_t codes[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, axes = 0; int n_entries = 0, deepest = 0;
    const uint32_t child[2] = {i + 1, n.offset};
    for (int side = 0; side < 2; ++side) {
      const rt_bvh_node& c = desc->nodes[child[side]];
      uint32_t ids[2]; int cnt;
      if (c.n_prims != 0) { ids[0] = child[side]; cnt = 1; }
      else { ids[0] = child[side] + 1; ids[1] = c.offset; cnt = 2; axes |= (uint32_t)c.axis << (2 * side); }
      for (int k = 0; k < cnt; ++k) {
        const rt_bvh_node& g = desc->nodes[ids[k]];
        float* bq = q + 6 * (2 * side + k);
        bq[0] = g.bmin[0]; bq[1] = g.bmin[1]; bq[2] = g.bmin[2]; bq[3] = g.bmax[0]; bq[4] = g.bmax[1]; bq[5] = g.bmax[2];
        codes[2 * side + k] = code_of(0, ids[k], ok);
        n_entries += 1; if (need[ids[k]] > deepest) deepest = need[ids[k]];
      }
    }
    memcpy(q + 24, codes, 16); memcpy(q + 28, &axes, 4);
    { const uint32_t ca = code_of(0, child[0], ok), cb = code_of(0, child[1], ok); memcpy(q + 29, &ca, 4); memcpy(q + 30, &cb, 4); }  // the children themselves: what the closest-hit step pushes for the far side
    need[i] = deepest + n_entries - 1;
  }
  p.quad_stack_depth = need[0] + 1 + max_obj_depth;  // (+ the deepest object's walk above the pending entries)
  // (closest-hit rays through the same records - near side first, exact - were built in round 5 and measured slower: S2 91.0 -> 95.9 ms, S4 1371 -> 1554; MEASUREMENTS R5)
  p.use_quads = ok && p.quad_stack_depth <= 32;  // (any hit: beyond the 32-entry LDS stack the larger stack costs more residency than the wider step returns)
  if (!p.use_quads) p.quads.clear();
  return RT_OK;
}

// Every check of a scene description and everything scene creation derives from it alone: RT_OK, or RT_ERR_INVALID / RT_ERR_UNSUPPORTED and what is wrong
static int rt_plan_scene(const rt_scene_desc* desc, RtScenePlan& p, std::string& why) {
  std::vector<int32_t> tex_side; std::vector<int64_t> tex_side_at; std::vector<int> tex_slots;
  why = texture_programs(desc, tex_side, tex_side_at, tex_slots); if (!why.empty()) return RT_ERR_INVALID;
  why = fourier_desc_error(desc); if (!why.empty()) return RT_ERR_INVALID;
  if (desc->n_nodes == 0 || desc->n_tris == 0 || !desc->nodes || !desc->tri_p || !desc->tri_meta) return rt_refuse(why, RT_ERR_INVALID, "empty scene");
  int rc = plan_geometry(desc, tex_slots, p, why);
  if (rc == RT_OK) rc = plan_images(desc, p, why);
  if (rc == RT_OK) rc = plan_textures(desc, tex_side, tex_side_at, p, why);
  if (rc == RT_OK) rc = plan_materials(desc, p, why);
  if (rc == RT_OK) rc = plan_lights(desc, p, why);
  if (rc != RT_OK) return rc;
  plan_route(desc, p);
  return plan_trees(desc, p, why);
}
