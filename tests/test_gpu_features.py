"""First-hit features on the GPU (rt_render_sample_features through HostScene.sample_features; RT_FLAG_FRAME_FEATURES / RT_FRAME_FEATURES through
HostScene.progressive(features=True)): the per-sample records are the frame loop's own camera ray, hit record, interaction and first throughput - held to
rt_trace_closest, to float64 models of the camera and of the scene description, to the materials' parameters -, the planes are the float64 sums of those records bit
for bit, and the flag moves nothing else. 32 x 32 x 16 scenes: (a) the Cornell box (k_shade<1> with its tables in LDS, identity slots, fresh records), (b) a small room
of matte-with-uv-texture, mirror, plastic, glass and a sphere (the binned queue), (c) = (b) under pixel_bounds strictly inside the film (real queue counts at bounce
0), (d) a two-level scene with one rigidly rotated and translated instance. Every measured figure is printed before it is asserted.

Record layout (RT_FEATURE_FLOATS = 16): o 0:3, d 3:6, prim 6 (int bits), b0 7, b1 8, depth 9, normal 10:13, albedo 13:16."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FLOOR = float(F(1e-3))
KD_UV = dict(su=0.8, sv=0.7, du=0.1, dv=0.15)   # u * su + du stays inside (0, 1) over the whole floor: the uv texture's fract() meets no edge
KR = (0.9, 0.8, 0.7)
KD_SPHERE = (0.2, 0.5, 0.8)
KD_WALL = (0.7, 0.6, 0.5)


def _cornell():
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(32, 32, 16)
    d.film.filter_kind, d.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)   # box filter, radius 0.5
    return d


def _room(pixel_bounds=None):
    """(b): floor = matte over a uv texture, back wall = mirror, left wall = plastic WITH vertex normals (interpolated shading normals), right wall = matte, a glass pane,
    a matte sphere, a ceiling over the back half only (camera rays through the front half leave the scene), one area light."""
    from rustracer_amd.scene_desc import SceneDesc
    s = SceneDesc()
    m_uv = s.matte(s.uv_tex(**KD_UV))
    m_mirror, m_plastic, m_glass = s.mirror(KR), s.plastic((0.3, 0.4, 0.2), (0.4, 0.4, 0.4), 0.2), s.glass()
    m_wall, m_sphere = s.matte(KD_WALL), s.matte(KD_SPHERE)
    s.add_mesh([(-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2)], [[0, 1, 2], [0, 2, 3]], m_uv, UV=[(0, 0), (1, 0), (1, 1), (0, 1)])
    s.add_quad((-2, 0, 2), (2, 0, 2), (2, 3, 2), (-2, 3, 2), m_mirror)
    tilt = np.float32([(1, 0.2, 0.1), (1, -0.1, 0.2), (1, 0.15, -0.2), (1, -0.2, -0.1)])
    s.add_mesh([(-2, 0, -2), (-2, 0, 2), (-2, 3, 2), (-2, 3, -2)], [[0, 1, 2], [0, 2, 3]], m_plastic, N=tilt / np.linalg.norm(tilt, axis=1, keepdims=True))
    s.add_quad((2, 0, 2), (2, 0, -2), (2, 3, -2), (2, 3, 2), m_wall)
    s.add_quad((-2, 3, 0), (2, 3, 0), (2, 3, 2), (-2, 3, 2), m_wall)
    s.add_quad((0.3, 0, 0.5), (1.3, 0, 0.5), (1.3, 1.5, 0.5), (0.3, 1.5, 0.5), m_glass)
    s.add_sphere((-0.8, 0.6, 0.3), 0.6, m_sphere)
    s.add_quad((-0.5, 2.99, 0.5), (0.5, 2.99, 0.5), (0.5, 2.99, 1.5), (-0.5, 2.99, 1.5), s.matte((0, 0, 0)), emission=(12, 12, 12))
    s.camera.pos, s.camera.look, s.camera.fov = (0.2, 1.5, -3.5), (0.0, 1.3, 0.0), 60.0
    s.film.xres, s.film.yres = 32, 32
    s.sampler.spp = 16
    s.integrator.pixel_bounds = pixel_bounds
    s.mats = dict(uv=m_uv, mirror=m_mirror, plastic=m_plastic, glass=m_glass, wall=m_wall, sphere=m_sphere)
    return s


def _rot(axis, angle):
    a = np.float64(axis) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


PYRAMID_P = np.float32([(0, 1, 0), (-0.6, 0, -0.6), (0.6, 0, -0.6), (0.6, 0, 0.6), (-0.6, 0, 0.6)])
PYRAMID_F = np.int32([(0, 2, 1), (0, 3, 2), (0, 4, 3), (0, 1, 4)])
INSTANCE_R, INSTANCE_T = _rot((1.0, 2.0, 0.5), 0.7), np.float64([0.3, 0.4, 0.2])


def _instanced():
    """(d): a floor, a light and ONE instance - a rotation and a translation - of an object of four flat triangles."""
    from rustracer_amd.scene_desc import SceneDesc
    s = SceneDesc()
    floor, red = s.matte((0.6, 0.5, 0.4)), s.matte((0.7, 0.2, 0.2))
    s.add_quad((-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3), floor)
    o = s.add_object([dict(P=PYRAMID_P, idx=PYRAMID_F, material=red)])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = INSTANCE_R, INSTANCE_T
    s.add_instance(o, m.astype(np.float32))
    s.add_quad((-1, 4, -1), (1, 4, -1), (1, 4, 1), (-1, 4, 1), s.matte((0, 0, 0)), emission=(10, 10, 10))
    s.camera.pos, s.camera.look, s.camera.fov = (0, 2.5, -5), (0.2, 0.6, 0), 40.0
    s.film.xres, s.film.yres = 32, 32
    s.sampler.spp = 16
    return s


BOUNDS_C = (5, 27, 6, 25)   # x0 x1 y0 y1: strictly inside the 32 x 32 film


@pytest.fixture(scope="module")
def scenes(gpu_host):
    """name -> dict(h, desc, feat): each scene, uploaded, with its per-sample records. Rendered once, left unchanged."""
    out = {}
    for name, d in (("a", _cornell()), ("b", _room()), ("c", _room(BOUNDS_C)), ("d", _instanced())):
        h = gpu_host.HostScene(d)
        feat = h.sample_features()
        feat.setflags(write=False)
        out[name] = dict(h=h, desc=d, feat=feat, window=h.samples_window())
    return out


def _prim(feat):
    return np.ascontiguousarray(feat[..., 6]).view(np.int32)


def _source(sc):
    """Per sample: the source primitive of a TOP-LEVEL hit (index into the description's triangles, then its spheres), -1 for a miss or a hit inside an instance."""
    ordered = np.asarray(sc["h"].bvh()["ordered"])
    prim = _prim(sc["feat"])
    top = (prim >= 0) & (prim < len(ordered))
    return np.where(top, ordered[np.clip(prim, 0, len(ordered) - 1)], -1)


def _tri_model_normals(P, idx, N, src, b0, b1, d):
    """float64 shading normals of triangle hits, turned against d: normalised interpolation of the vertex normals where N is given (per triangle: all or none), else
    +-normalize(cross)."""
    tri = idx[src]
    p0, p1, p2 = (P[tri[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(p0 - p2, p1 - p2)
    if N is not None:
        b2 = 1.0 - b0.astype(np.float64) - b1.astype(np.float64)
        n = N[tri[:, 0]].astype(np.float64) * b0[:, None].astype(np.float64) + N[tri[:, 1]].astype(np.float64) * b1[:, None].astype(np.float64) + N[tri[:, 2]].astype(np.float64) * b2[:, None]
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    flip = np.einsum("ij,ij->i", n, d.astype(np.float64)) > 0
    n[flip] *= -1
    return n


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_hits_are_the_kernels_hits(scenes, orc, name):
    """Each sample's (o, inf, d) through rt_trace_closest: prim, b0, b1 bit for bit; |depth - t| <= 1e-5 (|o|inf + |p|inf) - barycentric interpolation, one subtraction and
    a length are a handful of float32 roundings, ~1e-6 relative, times 10. (a) also through the oracle's trace, as the parity tests hold the two."""
    sc = scenes[name]
    f = sc["feat"].reshape(-1, 16)
    rays = np.zeros((len(f), 8), np.float32)
    rays[:, :3], rays[:, 3], rays[:, 4:7] = f[:, 0:3], np.inf, f[:, 3:6]
    r = sc["h"].trace(rays, count=False)
    prim = _prim(f)
    hit = prim >= 0
    same = [int((prim != r["prim"]).sum()), int((bits(f[hit, 7]) != bits(r["b0"][hit])).sum()), int((bits(f[hit, 8]) != bits(r["b1"][hit])).sum())]
    p = f[:, 0:3].astype(np.float64) + f[:, 3:6].astype(np.float64) * f[:, 9:10].astype(np.float64)
    bound = 1e-5 * (np.abs(f[:, 0:3]).max(1).astype(np.float64) + np.abs(p).max(1))
    err = np.abs(f[:, 9].astype(np.float64) - r["t"].astype(np.float64) * np.linalg.norm(f[:, 3:6].astype(np.float64), axis=1))
    worst = float((err[hit] / bound[hit]).max())
    print(f"\nFEATURES ({name}) {len(f)} samples, {int(hit.sum())} hits, {int((~hit).sum())} misses; differing prim / b0 / b1 words {same}; worst |depth - t| / bound {worst:.3e}")
    assert hit.any() and same == [0, 0, 0]
    assert worst <= 1.0
    if name == "b":
        assert (~hit).any(), "the room is open above its front half"
    if name == "d":
        assert (prim >= len(sc["h"].bvh()["ordered"])).sum() > 200, "hits inside the instance carry ids past the top level's"
    if name == "a":
        ro = orc.OracleScene(sc["desc"]).trace(rays)
        d = [int((prim != ro["prim"]).sum()), int((bits(f[hit, 7]) != bits(ro["b0"][hit])).sum()), int((bits(f[hit, 8]) != bits(ro["b1"][hit])).sum()), int((bits(r["t"]) != bits(ro["t"])).sum())]
        print(f"  against orc_trace: differing prim / b0 / b1 / t words {d}")
        assert d == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_rays_belong_to_their_film_positions(scenes, name):
    """d within 1e-6 per component of a float64 pinhole camera built from the camera description (raster_to_camera, camera_to_world; lens_radius = 0) at the film
    positions rt_render_samples reports for the same window; o at the camera position up to Ray::transform's error nudge."""
    sc = scenes[name]
    h = sc["h"]
    _, pf, _ = h.render_samples()
    st = h.setup()
    r2c = st["raster_to_camera"].astype(np.float64).reshape(4, 4)
    c2w = np.float64(list(st["params"].cam_to_world)).reshape(4, 4)
    assert st["params"].lens_radius == 0.0
    q = np.concatenate([pf.astype(np.float64), np.zeros(pf.shape[:-1] + (1,)), np.ones(pf.shape[:-1] + (1,))], -1) @ r2c.T
    pc = q[..., :3] / q[..., 3:4]
    dc = pc / np.linalg.norm(pc, axis=-1, keepdims=True)
    dw = dc @ c2w[:3, :3].T
    err_d = float(np.abs(sc["feat"][..., 3:6] - dw).max())
    pos = c2w[:3, 3]
    err_o = float(np.abs(sc["feat"][..., 0:3] - pos).max())
    print(f"\nFEATURES ({name}) rays against the float64 pinhole model: worst |d - model| {err_d:.3e} (bound 1e-6), worst |o - camera position| {err_o:.3e} (bound {1e-5 * (1 + np.abs(pos).max()):.3e})")
    assert pf.shape[:3] == sc["feat"].shape[:3]
    assert err_d <= 1e-6
    assert err_o <= 1e-5 * (1 + np.abs(pos).max())


# ---------------------------------------------------------------------------------------------- 3
def _check_normals(name, n, model, d):
    length = np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max()
    facing = float(np.einsum("ij,ij->i", n.astype(np.float64), d.astype(np.float64)).max())
    err = float(np.abs(n - model).max())
    print(f"  {name}: {len(n)} hits, worst | |n| - 1 | {length:.3e} (1e-6), largest dot(n, d) {facing:.3e} (<= 0), worst |n - model| {err:.3e} (1e-5)")
    assert len(n) > 0
    assert length <= 1e-6 and facing <= 0.0 and err <= 1e-5


def test_normals(scenes):
    """Unit length within 1e-6, dot(n, d) <= 0, components within 1e-5 of a float64 model from the scene description: flat triangles, interpolated vertex normals, the
    sphere's (p - c) / r at the record's own hit point, the instance's object-space normal under its rotation."""
    print("\nFEATURES normals")
    for name in ("a", "b"):
        sc = scenes[name]
        f = sc["feat"].reshape(-1, 16)
        src = _source(sc).reshape(-1)
        P, idx, N, UV, S, mat, light, flags = sc["desc"].arrays()
        tri = (src >= 0) & (src < len(idx))
        with_n = np.zeros(len(f), bool)
        with_n[tri] = (flags[src[tri]] & 2) != 0
        flat = tri & ~with_n
        _check_normals(f"({name}) flat triangles", f[flat, 10:13], _tri_model_normals(P, idx, None, src[flat], f[flat, 7], f[flat, 8], f[flat, 3:6]), f[flat, 3:6])
        if name == "b":
            _check_normals("(b) triangles with vertex normals", f[with_n, 10:13], _tri_model_normals(P, idx, N, src[with_n], f[with_n, 7], f[with_n, 8], f[with_n, 3:6]), f[with_n, 3:6])
            on = src >= len(idx)
            # (p - c) / r at the interaction's own point p = o + depth d. (Against the float64 root of the ray the float32 quadratic of Sphere::intersect places a grazing
            # hit up to 4e-5 further along the surface - measured: 6.6e-5 in the normal at dot(n, d) = -0.03 -, which is the intersection's error, not the normal's.)
            o, d = f[on, 0:3].astype(np.float64), f[on, 3:6].astype(np.float64)
            c, r = np.float64([-0.8, 0.6, 0.3]), 0.6
            p = o + d * f[on, 9:10].astype(np.float64)
            on_sphere = float(np.abs(np.linalg.norm(p - c, axis=1) - r).max())
            print(f"  (b) the sphere: worst | |p - c| - r | {on_sphere:.3e}")
            assert on_sphere <= 1e-5
            _check_normals("(b) the sphere", f[on, 10:13], (p - c) / r, f[on, 3:6])
    sc = scenes["d"]
    f = sc["feat"].reshape(-1, 16)
    inside = _prim(f) >= len(sc["h"].bvh()["ordered"])
    o, d = f[inside, 0:3].astype(np.float64), f[inside, 3:6].astype(np.float64)
    Pw = PYRAMID_P.astype(np.float64) @ INSTANCE_R.T + INSTANCE_T
    best_t, best_n = np.full(len(o), np.inf), np.zeros((len(o), 3))
    for tri in PYRAMID_F:   # float64 Moeller-Trumbore against the four world-space triangles: the nearest one's normal
        p0, e1, e2 = Pw[tri[0]], Pw[tri[1]] - Pw[tri[0]], Pw[tri[2]] - Pw[tri[0]]
        pv = np.cross(d, e2)
        det = pv @ e1
        tv = o - p0
        u = (tv * pv).sum(1) / det
        qv = np.cross(tv, e1)
        v = (d * qv).sum(1) / det
        t = qv @ e2 / det
        ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < best_t)
        n_obj = np.cross(PYRAMID_P[tri[0]].astype(np.float64) - PYRAMID_P[tri[2]], PYRAMID_P[tri[1]].astype(np.float64) - PYRAMID_P[tri[2]])
        n_w = INSTANCE_R @ (n_obj / np.linalg.norm(n_obj))
        best_t[ok], best_n[ok] = t[ok], n_w
    assert np.isfinite(best_t).all()
    flip = (best_n * d).sum(1) > 0
    best_n[flip] *= -1
    _check_normals("(d) the instance", f[inside, 10:13], best_n, f[inside, 3:6])
    worst = float(np.abs(f[inside, 9] - best_t * np.linalg.norm(d, axis=1)).max())
    print(f"  (d) depth against the float64 intersection: worst difference {worst:.3e}")
    assert worst <= 1e-5 * (np.abs(o).max() + 6.0)


# ---------------------------------------------------------------------------------------------- 4
def _rel_err(a, k):
    return np.abs(a.astype(np.float64) - k.astype(np.float64)) / np.maximum(np.abs(k.astype(np.float64)), 1e-30)


def test_albedo_of_matte_and_mirror_hits_and_misses(scenes):
    """Matte: f |cos| / pdf = (Kd / pi) cos / (cos / pi) = Kd, a chain of fewer than ten float32 roundings with a 1 - 2 ulp reciprocal: within 1e-5 relative. The uv
    texture's Kd is rt_texture_eval at the hit's uv. Mirror: Kr (Fresnel is 1 for Material "mirror"). Misses: all zero, prim = -1."""
    print("\nFEATURES albedo")
    for name in ("a", "b", "c"):
        sc = scenes[name]
        h, d = sc["h"], sc["desc"]
        f = sc["feat"].reshape(-1, 16)
        src = _source(sc).reshape(-1)
        P, idx, N, UV, S, mat, light, flags = d.arrays()
        prim = _prim(f)
        miss = prim < 0
        stray = int(np.count_nonzero(f[miss, 7:16])) + int((prim[miss] != -1).sum())
        print(f"  ({name}) {int(miss.sum())} misses, non-zero words among their b0 .. albedo {stray}")
        assert stray == 0
        tri = (src >= 0) & (src < len(idx))
        m_of = np.full(len(f), -1)
        m_of[tri] = mat[src[tri]]
        sph = src >= len(idx)
        m_of[sph] = np.int32([d.spheres[k - len(idx)].material for k in src[sph]])
        emitter = np.zeros(len(f), bool)
        emitter[tri] = light[src[tri]] >= 0
        for m, M in enumerate(d.materials):
            sel = (m_of == m) & ~emitter
            if not sel.any():
                continue
            kd_tex = d.textures[M.params["kd"]] if "kd" in M.params and M.kind == 0 else None
            if M.kind == 0 and kd_tex.kind == 0:     # matte, constant Kd
                want = np.broadcast_to(np.float32(kd_tex.value), (int(sel.sum()), 3))
            elif M.kind == 0:                        # matte over the uv texture
                b0, b1 = f[sel, 7].astype(np.float64), f[sel, 8].astype(np.float64)
                t = idx[src[sel]]
                uv = UV[t[:, 0]] * b0[:, None] + UV[t[:, 1]] * b1[:, None] + UV[t[:, 2]] * (1 - b0 - b1)[:, None]
                want = h.texture_eval(M.params["kd"], uv.astype(np.float32))
                assert want[:, :2].min() > 0.05 and not want[:, 2].any()
            elif M.kind == 3:                        # mirror
                want = np.broadcast_to(np.float32(d.textures[M.params["kr"]].value), (int(sel.sum()), 3))
            else:
                continue
            e = _rel_err(f[sel, 13:16], want)
            e[(want == 0) & (f[sel, 13:16] == 0)] = 0.0
            print(f"  ({name}) material {m} (kind {M.kind}): {int(sel.sum())} hits, worst relative |albedo - K| {float(e.max()):.3e} (1e-5)")
            assert e.max() <= 1e-5
        if name == "b":
            seen = {d.materials[m].kind for m in np.unique(m_of[m_of >= 0])}
            assert {0, 1, 3, 4} <= seen, seen   # matte, plastic, mirror and glass are all in view


def test_albedo_of_plastic_is_its_directional_albedo(gpu_host, orc):
    """256 spp on an 8 x 8 window of a narrow camera facing one plastic plane: the mean albedo against the deterministic quadrature of int f |cos| dw over orc_bsdf_probe
    (tests/test_invariants_cpu.py builds the same sum) at the window's central direction. Bound: 5 standard errors of the mean, from the samples themselves, + the
    quadrature's own error (the change when its step is halved). The camera's field of view is one degree, so the window's directions lie within 0.7 degrees of the central
    one; what the quadrature changes by over them is printed, not added to the bound."""
    import ctypes as C
    from rustracer_amd.scene_desc import SceneDesc

    def build():
        s = SceneDesc()
        m = s.plastic((0.4, 0.3, 0.2), (0.5, 0.5, 0.5), 0.4)
        s.add_quad((-50, -50, 0), (50, -50, 0), (50, 50, 0), (-50, 50, 0), m)
        s.add_quad((-1, -1, 90), (1, -1, 90), (1, 1, 90), (-1, 1, 90), s.matte((0, 0, 0)), emission=(5, 5, 5))
        return s, m
    theta = np.radians(40.0)
    wo_c = np.float64([np.sin(theta), 0.0, np.cos(theta)])
    s, m = build()
    s.camera.pos, s.camera.look, s.camera.up, s.camera.fov = tuple(10.0 * wo_c), (0, 0, 0), (0, 1, 0), 1.0
    s.film.xres, s.film.yres = 8, 8
    s.sampler.spp = 256
    feat = gpu_host.HostScene(s).sample_features().reshape(-1, 16)
    assert len(feat) == 64 * 256 and (_prim(feat) >= 0).all()
    a = feat[:, 13:16].astype(np.float64)
    mean, se = a.mean(0), a.std(0, ddof=1) / np.sqrt(len(a))
    sc = orc.OracleScene(build()[0])
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))

    def quadrature(wo, n_mu, n_phi):
        mu, w_mu = np.polynomial.legendre.leggauss(n_mu)
        phi = (np.arange(n_phi) + 0.5) * (2 * np.pi / n_phi)
        total = np.zeros(3)
        f, pdf, smp, u, wo32 = np.zeros(3, np.float32), C.c_float(), np.zeros(8, np.float32), np.float32([0.5, 0.5]), np.float32(wo)
        for c, wm in zip(mu, w_mu):
            sn = np.sqrt(max(0.0, 1 - c * c))
            for p in phi:
                wi = np.float32([sn * np.cos(p), sn * np.sin(p), c])
                orc.lib().orc_bsdf_probe(sc.h, m, fp(wo32), fp(wi), fp(u), fp(f), C.byref(pdf), fp(smp))
                total += f.astype(np.float64) * abs(c) * wm * (2 * np.pi / n_phi)
        return total
    wo_seen = -feat[:, 3:6].astype(np.float64)
    corner = wo_seen[np.argmax(np.linalg.norm(wo_seen - wo_c, axis=1))]
    q, q_half, q_corner = quadrature(wo_c, 64, 128), quadrature(wo_c, 32, 64), quadrature(corner / np.linalg.norm(corner), 32, 64)
    q_err = np.abs(q - q_half)
    print(f"\nFEATURES plastic: mean albedo {mean} +- {se} (standard error, {len(a)} samples); quadrature {q}, its error {np.abs(q - q_half)}, spread over the window {np.abs(q_corner - q_half)}; "
          f"|mean - quadrature| / (5 se + quadrature error) = {np.abs(mean - q) / (5 * se + q_err)}")
    assert (np.abs(mean - q) <= 5 * se + q_err).all()
    assert (se < 0.02).all() and (q > 0.1).all() and (q < 1.0).all()


# ---------------------------------------------------------------------------------------------- 5
def _criterion(n, sy, sy2, threshold, floor_y, min_samples):
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = sy / n
        var = np.maximum(0.0, sy2 - sy * mean) / (n - 1.0)
        se = np.sqrt(var / n)
        return (n < max(min_samples, 2)) | (se > threshold * np.maximum(mean, floor_y))


def _median_gap_threshold(n, sy, sy2, floor_y):
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = sy / n
        ratio = np.sqrt(np.maximum(0.0, sy2 - sy * mean) / (n - 1.0) / n) / np.maximum(mean, floor_y)
    r = np.sort(ratio[np.isfinite(ratio)].ravel())
    i = r.size // 2
    return float(F(0.5 * (float(r[i - 1]) + float(r[i])))), float(r[i - 1]), float(r[i])


def _planes(sc, taken):
    """The planes the records give: float64 sums, one term after the other in sample-index order from an explicit +0.0 (np.add.accumulate; np.sum is pairwise), over the
    samples marked in taken [window pixel, sample]; divided in float64, rounded to float32; laid into the cropped film."""
    h, feat = sc["h"], sc["feat"]
    x0, y0, x1, y1 = sc["window"]
    cropped = [int(v) for v in h.setup()["cropped"]]
    hit = _prim(feat) >= 0

    def total(v):
        v64 = np.where(taken, v.astype(np.float64), 0.0)
        return np.add.accumulate(np.concatenate([np.zeros(v64.shape[:-1] + (1,)), v64], -1), axis=-1)[..., -1]
    n = taken.sum(-1).astype(np.float64)
    hits = (taken & hit).sum(-1).astype(np.float64)
    win = np.zeros(feat.shape[:2] + (8,), np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, col in enumerate((13, 14, 15, 10, 11, 12)):
            win[..., k] = np.where(n > 0, total(feat[..., col]) / n, 0.0).astype(np.float32)
        win[..., 6] = np.where(hits > 0, total(np.where(hit, feat[..., 9], F(0))) / hits, 0.0).astype(np.float32)
        win[..., 7] = np.where(n > 0, hits / n, 0.0).astype(np.float32)
    out = np.zeros((cropped[3] - cropped[1], cropped[2] - cropped[0], 8), np.float32)
    out[y0 - cropped[1]:y1 - cropped[1], x0 - cropped[0]:x1 - cropped[0]] = win
    return out


def _window_of(sc, plane):
    """[window pixel] view of a [cropped pixel] array."""
    x0, y0, x1, y1 = sc["window"]
    cropped = [int(v) for v in sc["h"].setup()["cropped"]]
    return plane[y0 - cropped[1]:y1 - cropped[1], x0 - cropped[0]:x1 - cropped[0]]


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_planes_are_the_samples(scenes, name):
    sc = scenes[name]
    h = sc["h"]
    hh, ww, spp = sc["feat"].shape[:3]
    print(f"\nFEATURES ({name}) planes against the float64 sums of the records")
    with h.progressive(features=True) as fr:
        z = fr.features()
        assert z.shape[2] == 8 and z.dtype == np.float32 and not z.any(), "zeros before the first step"
        k = 0
        for step in (3, 5, 8):
            fr.advance(step)
            k += step
            taken = np.zeros((hh, ww, spp), bool)
            taken[..., :k] = True
            got, want = fr.features(), _planes(sc, taken)
            differ = int((bits(got) != bits(want)).sum())
            print(f"  after {k} samples: {differ} of {got.size} words differ; coverage spans [{got[..., 7].min():.3f}, {got[..., 7].max():.3f}]")
            assert differ == 0
        if name == "c":   # nothing outside pixel_bounds
            outside = np.ones(got.shape[:2], bool)
            _window_of(sc, outside)[...] = False
            assert outside.sum() == 32 * 32 - (BOUNDS_C[1] - BOUNDS_C[0]) * (BOUNDS_C[3] - BOUNDS_C[2]) and not got[outside].any()
        assert fr.state_bytes >= 32 * 32 * 64
    # features + statistics, one adaptive step: the indices each pixel took follow from the statistics plane and the criterion
    with h.progressive(features=True, pixel_stats=True) as fr:
        fr.advance(4)
        n, sy, sy2 = [_window_of(sc, a).copy() for a in fr.pixel_stats()]
        thr, lo, hi = _median_gap_threshold(n, sy, sy2, FLOOR)
        mask = _criterion(n, sy, sy2, thr, FLOOR, 4)
        fr.advance_adaptive(4, thr, FLOOR, min_samples=4)
        n8 = _window_of(sc, fr.pixel_stats()[0])
        taken = np.zeros((hh, ww, spp), bool)
        taken[..., :4] = True
        taken[..., 4:8] = mask[..., None]
        got, want = fr.features(), _planes(sc, taken)
        differ = int((bits(got) != bits(want)).sum())
        print(f"  4 samples, then an adaptive step of 4 at threshold {thr:.6g} (gap {(hi - lo) / hi:.3e}): {int(mask.sum())} of {mask.size} pixels active; {differ} words differ")
        assert (hi - lo) / hi > 1e-6 and 0 < mask.sum() < mask.size
        assert np.array_equal(n8, taken.sum(-1))
        assert differ == 0


def test_planes_of_a_shard_and_of_a_crop(gpu_host, scenes):
    """Rank 0 of 2 holds its own rows' planes and zeros elsewhere; a crop window reads the planes of its own pixels (whose samples are keyed by the cropped frame's pixel
    indices: other samples than the uncropped frame's)."""
    from rustracer_amd.distributed import owned_pixel_mask
    sc = scenes["b"]
    h = sc["h"]
    st = h.setup()
    cropped, sb = [int(v) for v in st["cropped"]], [int(v) for v in st["sample_bounds"]]
    taken = np.ones(sc["feat"].shape[:3], bool)
    want = _planes(sc, taken)
    print("\nFEATURES shards and crop")
    for r in range(2):
        with h.progressive(rank=r, world_size=2, features=True) as fr:
            fr.advance(16)
            got = fr.features()
        own = owned_pixel_mask(cropped, sb, r, 2)
        differ, stray = int((bits(got[own]) != bits(want[own])).sum()), int(np.count_nonzero(got[~own]))
        print(f"  rank {r} of 2: {int(own.sum())} own pixels, {differ} words differ from the unsharded planes, {stray} non-zero words in the other rank's rows")
        assert 0 < own.sum() < own.size and differ == 0 and stray == 0
    d = _room()
    d.film.crop = (0.25, 0.75, 0.125, 1.0)
    hc = gpu_host.HostScene(d)
    sc_c = dict(h=hc, feat=hc.sample_features(), window=hc.samples_window())
    with hc.progressive(features=True) as fr:
        fr.advance(16)
        got = fr.features()
    want_c = _planes(sc_c, np.ones(sc_c["feat"].shape[:3], bool))
    cc = [int(v) for v in hc.setup()["cropped"]]
    differ = int((bits(got) != bits(want_c)).sum())
    print(f"  crop {cc}: film {got.shape}, {differ} words differ from the records' sums; coverage spans [{got[..., 7].min():.3f}, {got[..., 7].max():.3f}]")
    assert got.shape == (cc[3] - cc[1], cc[2] - cc[0], 8) and got.shape[0] < 32 and differ == 0 and got[..., :3].any()


# ---------------------------------------------------------------------------------------------- 6
COUNTS = ("camera_rays", "rays_closest", "rays_shadow", "rays_mis", "rays_mis_any", "rays_mis_not_cast", "rays_tail_not_cast", "rays_shadow_not_cast", "paths_scrubbed", "n_passes",
          "vertices_lambert_const", "vertices_lambert", "vertices_two_lobe", "vertices_generic", "launches_trace_closest", "launches_trace_path", "launches_trace_shadow",
          "launches_trace_mis", "launches_trace_mis_any", "launches_shade")


@pytest.mark.parametrize("name", ["a", "b"])
def test_nothing_else_moves(gpu_host, scenes, name):
    sc = scenes[name]
    h = sc["h"]
    film0, st0 = h.render()
    with h.progressive(pixel_stats=True) as fr:
        plain_steps = [fr.advance(n) for n in (3, 5, 8)]
        plain = dict(film=fr.film(), stats=np.stack(fr.pixel_stats(), -1))
        with pytest.raises(gpu_host.BackendError) as e:
            fr.features()
        print(f"\nFEATURES ({name}) read without the flag refused: {e.value}")
        assert "RT_FLAG_FRAME_FEATURES" in str(e.value) and "(-1)" in str(e.value)
    with h.progressive(pixel_stats=True, features=True) as fr:
        steps = [fr.advance(n) for n in (3, 5, 8)]
        flagged = dict(film=fr.film(), stats=np.stack(fr.pixel_stats(), -1))
    film1, st1 = h.render()
    words = lambda a: np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)
    d = [int((words(plain[k]) != words(flagged[k])).sum()) for k in ("film", "stats")] + [int((bits(film0) != bits(film1)).sum()), int((bits(film0) != bits(flagged["film"])).sum())]
    moved = [k for k in COUNTS if st0[k] != st1[k]]
    step_moved = [k for k in COUNTS for a, b in zip(plain_steps, steps) if a[k] != b[k]]
    print(f"  words that differ - film with / without the flag {d[0]}, statistics plane {d[1]}, rt_render before / after the feature frame {d[2]}, rt_render / feature frame {d[3]}; "
          f"counters that moved between the two rt_render calls {moved}, between the frames' steps {step_moved}")
    assert d == [0, 0, 0, 0] and moved == [] and step_moved == []


def test_max_depth_moves_only_the_albedo(gpu_host, scenes):
    """max_depth 0, 1, 5: ray, hit, depth and normal keep every bit; max_depth 0 gives zero albedo, 1 gives max_depth 5's; the film at max_depth 1 is the same bytes with
    and without the flag (the feature frame casts the continuation rays nothing reads)."""
    print("\nFEATURES max_depth")
    for name in ("a", "b"):
        ref = scenes[name]["feat"]
        for depth in (0, 1):
            d = _cornell() if name == "a" else _room()
            d.integrator.max_depth = depth
            h = gpu_host.HostScene(d)
            f = h.sample_features()
            differ = int((bits(f[..., :13]) != bits(ref[..., :13])).sum())
            albedo = int(np.count_nonzero(f[..., 13:16])) if depth == 0 else int((bits(f[..., 13:16]) != bits(ref[..., 13:16])).sum())
            print(f"  ({name}) max_depth {depth}: {differ} words of o .. normal differ from max_depth 5's; albedo words {'non-zero' if depth == 0 else 'that differ'} {albedo}")
            assert differ == 0 and albedo == 0
            if depth == 1:
                film, st = h.render()
                with h.progressive(features=True) as fr:
                    a = fr.advance(16)
                    got, planes = fr.film(), fr.features()
                print(f"  ({name}) max_depth 1: film words that differ with the flag {int((bits(got) != bits(film)).sum())}; rays_tail_not_cast {st['rays_tail_not_cast']} -> {a['rays_tail_not_cast']}, "
                      f"rays_closest {st['rays_closest']} -> {a['rays_closest']}")
                assert int((bits(got) != bits(film)).sum()) == 0
                assert planes[..., :3].any() and a["rays_closest"] == st["rays_closest"] and a["rays_tail_not_cast"] < st["rays_tail_not_cast"]


# ---------------------------------------------------------------------------------------------- 7
_SEQUENCE = """
def sequence(h, thr, budget=None):
    with h.progressive(table_budget=budget, pixel_stats=True, features=True) as fr:
        a, b = fr.advance(2), fr.advance_adaptive(2, thr, float(np.float32(1e-3)), min_samples=2)
        return fr.features(), fr.tables_resident, (a["n_passes"], b["n_passes"]), fr.active_pixels
"""
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from rustracer_amd import host
from rustracer_amd.scenes import cornell_box
""" + _SEQUENCE + """
h = host.HostScene(cornell_box(320, 256, 4))
for out, budget, resident in ((sys.argv[3], None, True), (sys.argv[4], 1, False)):
    planes, res, passes, active = sequence(h, float(sys.argv[2]), budget)
    assert res == resident, (budget, res)
    # two batches of 2^16 and 2^14 pixels, the first in passes of one sample: more than one pass per step
    assert min(passes) >= 3, passes
    np.savez(out, planes=planes, active=active)
"""


def test_batches_passes_and_table_residency_change_no_byte(gpu_host, tmp_path):
    """The settings of test_gpu_adaptive's test of the same name (RTX_PASS_LOG2 = RTX_BATCH_LOG2 = 16 in a fresh child: two batches, one sample per pass; resident and
    rebuilt sampler tables): the planes are this process's, word for word."""
    from rustracer_amd.scenes import cornell_box
    ns = {"np": np}
    exec(_SEQUENCE, ns)
    h = gpu_host.HostScene(cornell_box(320, 256, 4))
    with h.progressive(pixel_stats=True) as fr:
        fr.advance(2)
        thr, lo, hi = _median_gap_threshold(*fr.pixel_stats(), FLOOR)
    assert (hi - lo) / hi > 1e-6
    planes, _, passes, active = ns["sequence"](h, thr)
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    out = [str(tmp_path / "resident.npz"), str(tmp_path / "rebuilt.npz")]
    env = dict(os.environ, RTX_PASS_LOG2="16", RTX_BATCH_LOG2="16")
    r = subprocess.run([sys.executable, str(script), ROOT, repr(thr)] + out, env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    resident, rebuilt = np.load(out[0]), np.load(out[1])
    d = [int((bits(resident["planes"]) != bits(rebuilt["planes"])).sum()), int((bits(resident["planes"]) != bits(planes)).sum())]
    print(f"\nFEATURES 320x256x4 in two batches, threshold {thr:.6g}: active here {active} / resident {int(resident['active'])} / rebuilt {int(rebuilt['active'])} (passes here {passes}); "
          f"plane words that differ - resident/rebuilt {d[0]}, resident/here {d[1]}")
    assert 0 < active < 320 * 256 and int(resident["active"]) == active and int(rebuilt["active"]) == active
    assert planes[..., 7].min() < 1.0 and planes[..., :3].any()
    assert d == [0, 0]
