// Host side of the shadow sets (rt_scene_create; included by rtx_hip.hip): for every voxel of the light distribution's grid and every sampled light of a scene with
// two triangle lights, whether ANY shadow segment that spawn_ray_to_interaction (rtx_dev_scene.h, rc/interaction.rs:69-74) can build from a surface point of the voxel
// to a point of the light can be occluded. A voxel / light pair whose segments provably hit no triangle is EMPTY: k_shade applies its light-sampling term without
// casting the segment. Everything else is WALK (today's any-hit walk). The argument and its margins: DESIGN.md §5.3. All tests in float64; when in doubt, WALK.
// Nothing here touches the device: rt_shadow_sets() exposes it to tests that run without one.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

// (after rtx_kernels.h: RT_SHADOW_WALK, RT_SHADOW_EMPTY - the kinds k_shade reads)

struct RtShadowSets {
  int nvox[3] = {1, 1, 1};
  int n_lights = 0;
  std::vector<uint32_t> word;     // [voxel * 2 + light]: the pair's kind (RT_SHADOW_*), 0 = WALK for voxels no surface reaches
  uint64_t pairs = 0, empty = 0;  // pairs of voxels that hold a surface point and lights, and of them EMPTY
};

namespace rtss {
struct D3 { double x, y, z; };
static inline D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static inline D3 crs(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static inline double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline double l1(D3 a) { return std::fabs(a.x) + std::fabs(a.y) + std::fabs(a.z); }
static inline D3 unit(D3 a) { const double l = std::sqrt(dot(a, a)); return l > 0.0 ? D3{a.x / l, a.y / l, a.z / l} : D3{0, 0, 0}; }
struct Box { D3 lo, hi; };
static inline double box_min(const Box& b, D3 a) { return (a.x < 0 ? b.hi.x : b.lo.x) * a.x + (a.y < 0 ? b.hi.y : b.lo.y) * a.y + (a.z < 0 ? b.hi.z : b.lo.z) * a.z; }
static inline double box_max(const Box& b, D3 a) { return (a.x < 0 ? b.lo.x : b.hi.x) * a.x + (a.y < 0 ? b.lo.y : b.hi.y) * a.y + (a.z < 0 ? b.lo.z : b.hi.z) * a.z; }
}  // namespace rtss

// The voxel grid of build_light_distribution (SpatialLightDistribution::new, lightdistrib.rs:62-81): 64 voxels along the widest axis of the world box.
static void rt_shadow_grid(const float wb_min[3], const float wb_max[3], int nvox[3]) {
  const float diag[3] = {wb_max[0] - wb_min[0], wb_max[1] - wb_min[1], wb_max[2] - wb_min[2]};
  const int ext = diag[0] > diag[1] ? (diag[0] > diag[2] ? 0 : 2) : (diag[1] > diag[2] ? 1 : 2);
  for (int i = 0; i < 3; ++i) {
    const float r = roundf(diag[i] / diag[ext] * 64.0f);
    const unsigned v = (r != r || r <= 0.0f) ? 0u : (unsigned)r;
    nvox[i] = (int)(v > 1u ? v : 1u);
  }
}

// tri_p: n_tris x 9 floats (leaf order); light_prims: the n_lights (2) emitting triangles; wb_min / wb_max: the world box (the root node's bounds)
static void rt_build_shadow_sets(const float* tri_p, uint32_t n_tris, const int32_t* light_prims, int n_lights, const float wb_min[3], const float wb_max[3], RtShadowSets& out) {
  using namespace rtss;
  rt_shadow_grid(wb_min, wb_max, out.nvox);
  out.n_lights = n_lights;
  const int nx = out.nvox[0], ny = out.nvox[1], nz = out.nvox[2];
  const size_t total = (size_t)nx * ny * nz;
  out.word.assign(total * 2, RT_SHADOW_WALK);
  out.pairs = out.empty = 0;
  if (n_lights != 2 || n_tris == 0) return;
  const D3 wmin{wb_min[0], wb_min[1], wb_min[2]}, wmax{wb_max[0], wb_max[1], wb_max[2]};
  const D3 ext = sub(wmax, wmin);
  const double scale = std::max(ext.x, std::max(ext.y, ext.z));
  // The float32 errors the margins cover grow with the coordinates, not with the extent: offset_ray_origin steps by dot(|n|, p_error) <= gamma(7) |p|_1 and the
  // watertight test rounds relative to |p - o|. The margins are fractions of MAG = max(extent, largest |coordinate|), and a scene further than 64 extents from
  // the origin gets no sets (its margins would swallow whole voxels).
  const double mag = std::max(scale, std::max(std::max(std::fabs(wmin.x), std::fabs(wmax.x)), std::max(std::max(std::fabs(wmin.y), std::fabs(wmax.y)), std::max(std::fabs(wmin.z), std::fabs(wmax.z)))));
  if (!(scale > 0.0) || !(mag <= 64.0 * scale)) return;
  // Margins: PAD_V >= the marking pad (k_lightdist_mark: every surface point voxel_of maps to a voxel lies in its box grown by 1e-4 of the extent
  // per axis; voxel_of's own rounding is below 1e-7 MAG); PAD_O adds the largest step of offset_ray_origin (< 1.3e-6 MAG) with room to spare; PAD_L bounds how
  // far the offset end of a segment leaves its light triangle; SEP: the gap a separating axis must show; COPLANAR: what counts as "in T's plane".
  const double PAD_V = 1e-4 * scale + 1e-5 * mag, PAD_O = 2e-4 * mag, PAD_L = 1e-4 * mag, SEP = 1e-4 * mag, COPLANAR = 1e-9 * mag;
  const double ONE_MINUS_TMAX = 0.99e-4;  // 1 - (1 - ShadowEpsilon) in float: 1.0001e-4; a little less
  const double T_GAP = 5e-5;              // shortest relative distance between t_max and the crossing of T's plane that rule (b) accepts
  auto vtx = [&](uint32_t t, int k) { const float* p = tri_p + 9 * (size_t)t + 3 * k; return D3{p[0], p[1], p[2]}; };
  std::vector<Box> tbox(n_tris);
  std::vector<D3> tn(n_tris);
  for (uint32_t t = 0; t < n_tris; ++t) {
    const D3 a = vtx(t, 0), b = vtx(t, 1), c = vtx(t, 2);
    tbox[t].lo = D3{std::min(a.x, std::min(b.x, c.x)), std::min(a.y, std::min(b.y, c.y)), std::min(a.z, std::min(b.z, c.z))};
    tbox[t].hi = D3{std::max(a.x, std::max(b.x, c.x)), std::max(a.y, std::max(b.y, c.y)), std::max(a.z, std::max(b.z, c.z))};
    tn[t] = unit(crs(sub(b, a), sub(c, a)));
  }
  // signed distance of x to T's plane (unit normal; 0 for a degenerate T)
  auto sdist = [&](uint32_t t, D3 x) { return dot(tn[t], sub(x, vtx(t, 0))); };
  auto coplanar = [&](uint32_t t, uint32_t s) {
    if (dot(tn[t], tn[t]) == 0.0) return false;
    for (int k = 0; k < 3; ++k) if (std::fabs(sdist(t, vtx(s, k))) > COPLANAR) return false;
    return true;
  };
  std::vector<uint32_t> surf;
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const size_t v = ((size_t)z * ny + y) * nx + x;
        Box vb;  // the voxel's box grown by the marking pad: every surface point voxel_of maps to v
        vb.lo = D3{wmin.x + ext.x * x / nx - PAD_V, wmin.y + ext.y * y / ny - PAD_V, wmin.z + ext.z * z / nz - PAD_V};
        vb.hi = D3{wmin.x + ext.x * (x + 1) / nx + PAD_V, wmin.y + ext.y * (y + 1) / ny + PAD_V, wmin.z + ext.z * (z + 1) / nz + PAD_V};
        surf.clear();
        for (uint32_t t = 0; t < n_tris; ++t) {
          const Box& b = tbox[t];
          if (b.lo.x <= vb.hi.x + PAD_O && b.hi.x >= vb.lo.x - PAD_O && b.lo.y <= vb.hi.y + PAD_O && b.hi.y >= vb.lo.y - PAD_O && b.lo.z <= vb.hi.z + PAD_O && b.hi.z >= vb.lo.z - PAD_O)
            surf.push_back(t);
        }
        if (surf.empty()) continue;  // no surface point can look this voxel up
        Box ob;  // every origin: a surface point in vb moved by offset_ray_origin
        ob.lo = D3{vb.lo.x - PAD_O, vb.lo.y - PAD_O, vb.lo.z - PAD_O}; ob.hi = D3{vb.hi.x + PAD_O, vb.hi.y + PAD_O, vb.hi.z + PAD_O};
        for (int l = 0; l < n_lights; ++l) {
          out.pairs += 1;
          const uint32_t lp = (uint32_t)light_prims[l];
          if (lp >= n_tris) continue;
          const D3 L[3] = {vtx(lp, 0), vtx(lp, 1), vtx(lp, 2)};
          // (a) a separating axis between T and the hull of the origin box and the light's (grown) triangle
          auto separated = [&](uint32_t t) {
            const D3 T[3] = {vtx(t, 0), vtx(t, 1), vtx(t, 2)};
            const D3 te[3] = {sub(T[1], T[0]), sub(T[2], T[1]), sub(T[0], T[2])}, le[3] = {sub(L[1], L[0]), sub(L[2], L[1]), sub(L[0], L[2])};
            const D3 ax3[3] = {D3{1, 0, 0}, D3{0, 1, 0}, D3{0, 0, 1}};
            const D3 oc{0.5 * (ob.lo.x + ob.hi.x), 0.5 * (ob.lo.y + ob.hi.y), 0.5 * (ob.lo.z + ob.hi.z)};
            const D3 lc{(L[0].x + L[1].x + L[2].x) / 3.0, (L[0].y + L[1].y + L[2].y) / 3.0, (L[0].z + L[1].z + L[2].z) / 3.0};
            auto test = [&](D3 a) {
              a = unit(a);
              if (dot(a, a) == 0.0) return false;
              double h0 = box_min(ob, a), h1 = box_max(ob, a);
              const double lpad = PAD_L * l1(a);
              for (int k = 0; k < 3; ++k) { const double p = dot(a, L[k]); h0 = std::min(h0, p - lpad); h1 = std::max(h1, p + lpad); }
              double t0 = dot(a, T[0]), t1 = t0;
              for (int k = 1; k < 3; ++k) { const double p = dot(a, T[k]); t0 = std::min(t0, p); t1 = std::max(t1, p); }
              return t1 < h0 - SEP || t0 > h1 + SEP;
            };
            for (int k = 0; k < 3; ++k) if (test(ax3[k])) return true;
            if (test(tn[t]) || test(tn[lp])) return true;
            for (int i = 0; i < 3; ++i) {
              for (int k = 0; k < 3; ++k) if (test(crs(te[i], ax3[k])) || test(crs(te[i], le[k]))) return true;
              if (test(crs(te[i], sub(lc, oc)))) return true;
              for (int k = 0; k < 3; ++k) if (test(crs(te[i], sub(L[k], oc)))) return true;
            }
            return false;
          };
          // (b) T's plane has every origin on its closed side and every shortened end strictly on that side, far enough from t_max
          auto behind = [&](uint32_t t) {
            if (dot(tn[t], tn[t]) == 0.0) return false;
            for (int sg = -1; sg <= 1; sg += 2) {
              auto s = [&](D3 p) { return sg * sdist(t, p); };
              // targets: a light coplanar with T is offset towards the origin's side (closed side); otherwise its grown vertices
              const bool l_in = coplanar(t, lp);
              double st_min = l_in ? 0.0 : std::min(s(L[0]), std::min(s(L[1]), s(L[2]))) - PAD_L * std::sqrt(3.0);
              if (!l_in && !(st_min > 0.0)) continue;
              double so_min = HUGE_VAL, so_max = -HUGE_VAL; bool ok = true;
              for (uint32_t si : surf) {
                if (coplanar(t, si)) {  // in T's plane: offset towards the light, which is on the positive side
                  if (l_in) { ok = false; break; }
                  so_min = std::min(so_min, 0.0); so_max = std::max(so_max, PAD_O);  // (an offset origin stays within PAD_O of the plane)
                  continue;
                }
                Box c;  // where surface si's points in this voxel can lie (its box grown, clipped to the origin box)
                c.lo = D3{std::max(tbox[si].lo.x - PAD_O, ob.lo.x), std::max(tbox[si].lo.y - PAD_O, ob.lo.y), std::max(tbox[si].lo.z - PAD_O, ob.lo.z)};
                c.hi = D3{std::min(tbox[si].hi.x + PAD_O, ob.hi.x), std::min(tbox[si].hi.y + PAD_O, ob.hi.y), std::min(tbox[si].hi.z + PAD_O, ob.hi.z)};
                const D3 a{sg * tn[t].x, sg * tn[t].y, sg * tn[t].z};
                const double off = sg * dot(tn[t], vtx(t, 0));
                const double mn = box_min(c, a) - off, mx = box_max(c, a) - off;
                if (!(mn >= 0.0)) { ok = false; break; }
                so_min = std::min(so_min, mn); so_max = std::max(so_max, mx);
              }
              if (!ok) continue;
              // shortened end e = (1 - t_max) o + t_max target: s(e) >= (1 - t_max) so_min + t_max st_min; the plane's crossing lies past t_max by s(e) / (s(o) - s(e))
              const double se_min = ONE_MINUS_TMAX * so_min + (1.0 - ONE_MINUS_TMAX) * st_min;
              if (se_min > 0.0 && se_min >= T_GAP * so_max) return true;
            }
            return false;
          };
          bool empty = true;
          for (uint32_t t = 0; t < n_tris && empty; ++t) if (!behind(t) && !separated(t)) empty = false;
          if (empty) { out.word[2 * v + l] = RT_SHADOW_EMPTY; out.empty += 1; }
        }
      }
}
