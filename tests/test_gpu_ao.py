"""rt_render_rays_ao / rt_render_ao on the GPU (HostScene.render_rays_ao, HostScene.render_ao): the ambient-occlusion and normal integrators held to closed forms
(exact ones and zeros, the cone under a sphere), to the numpy model of tests/ao_model.py ray record by ray record, to the oracle's any-hit answer for every record,
and to the frame of rt_render for everything the two share. Scenes of 4 to 210 triangles, at most 16 x 16 x 4 rays except the one statistic; occlusion samples in
{1, 3, 8} at dimensions = 4, so that a sample's first two come from the tables and the rest from its RNG stream. Every measured figure is printed before it is asserted.

Origins of the occlusion rays: the float32 rebuild of (p, p_error) in the reference's order needs the third barycentric of the closest hit as the hit test computed it
(e2 * inv_det, not 1 - b0 - b1) and, on a sphere, the refined hit point; no exported hit record carries them (t, prim, b0, b1). So the origin is held to the second
form: p is rebuilt in float64 from the closest-hit record - b0 p0 + b1 p1 + (1 - b0 - b1) p2, a sphere's o + t d scaled onto the sphere - with the reference's p_error
evaluated in float64, and every origin must lie on w's side of the float64 plane through p with the hit's normal (on it: what offset_ray_origin gives where p_error's
component is 0, a plane through zero) and within 2 |p_error| + 2 ulp(|p|) of p in each of the three components (|p_error| the Euclidean length, ulp(|p|) that of
p's largest component). That is what offset_ray_origin's own arithmetic can promise per component - |offset_i| <= dot(|n|, p_error) <= |p_error|, the float32 p within
p_error_i of the float64 one, half an ulp for the sum and one for the step away - while the Euclidean distance of three such components can reach 2.6 ulp beyond
2 |p_error| in the reference itself. A sphere's ray point o + t d is taken in float32, as Sphere::intersect forms it (ao_model.Geometry.from_hit_records): p_error
bounds the scaling onto the sphere, not that rounding along it. No ray is set aside."""
import numpy as np
import pytest

import ao_model
from util import bits

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
DIMS = 4
INF = np.float32(np.inf)


# ---------------------------------------------------------------------------------------------- scenes
def _new(xres=8, yres=8, spp=4):
    from rustracer_amd.scene_desc import SceneDesc
    s = SceneDesc()
    s.film.xres, s.film.yres = xres, yres
    s.film.filter_kind, s.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)
    s.sampler.spp = spp
    s.camera.pos, s.camera.look, s.camera.fov = (0.0, 3.0, -6.0), (0.0, 0.5, 0.0), 40.0
    return s


def _hidden_light(s, y=-50.0):
    """An emitter no ray of these tests can see (below everything, facing down): the scene has a light list, the integrators never read it."""
    s.add_quad((-1, y, -1), (1, y, -1), (1, y, 1), (-1, y, 1), s.matte((0, 0, 0)), emission=(1, 1, 1))


def _ground(half=200.0, **kw):
    s = _new(**kw)
    s.add_quad((-half, 0, -half), (-half, 0, half), (half, 0, half), (half, 0, -half), s.matte((0.5, 0.5, 0.5)))
    _hidden_light(s)
    return s


def _cube(edge=2.0):
    s = _new()
    m, a = s.matte((0.5, 0.5, 0.5)), edge / 2
    c = [(-a, -a, -a), (a, -a, -a), (a, a, -a), (-a, a, -a), (-a, -a, a), (a, -a, a), (a, a, a), (-a, a, a)]
    for q in ((0, 1, 2, 3), (5, 4, 7, 6), (4, 0, 3, 7), (1, 5, 6, 2), (3, 2, 6, 7), (4, 5, 1, 0)):
        s.add_quad(*[c[i] for i in q], m)
    _hidden_light(s)
    return s


def _mesh():
    """A bumpy 10 x 10 height field over a ground quad, 200 triangles in three meshes: plain, wound the other way round through reverse_orientation, and with per-vertex
    normals that point DOWN - Triangle::intersect turns hit.n to the interpolated normal's side (mesh.rs:417-422), so on that mesh the occlusion rays leave downwards."""
    s = _new()
    m = s.matte((0.6, 0.6, 0.6))
    g = np.linspace(-2, 2, 11)
    X, Z = np.meshgrid(g, g, indexing="ij")
    Y = 0.5 + 0.35 * np.sin(2.1 * X + 0.3) * np.cos(1.7 * Z - 0.2)
    P = np.stack([X, Y, Z], axis=-1).reshape(-1, 3)
    N = np.stack([0.735 * np.cos(2.1 * X + 0.3) * np.cos(1.7 * Z - 0.2), -np.ones_like(X), -0.595 * np.sin(2.1 * X + 0.3) * np.sin(1.7 * Z - 0.2)], axis=-1).reshape(-1, 3)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    a, b, c = [], [], []
    for i in range(10):
        for j in range(10):
            v = i * 11 + j
            (a, b, c)[(i + 2 * j) % 3].extend([(v, v + 1, v + 12), (v, v + 12, v + 11)])
    s.add_mesh(P, a, m)
    s.add_mesh(P, b, m, reverse_orientation=True)
    s.add_mesh(P, c, m, N=N)
    s.add_quad((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4), m)
    _hidden_light(s)
    return s


def _sphere(r=0.5, h=1.0, **kw):
    s = _ground(half=6.0, **kw)
    s.add_sphere((0.0, h, 0.0), r, s.matte((0.3, 0.3, 0.8)))
    return s


def _instanced():
    """A floor and one rotated, translated instance of an object of four flat triangles ((d) of tests/test_gpu_render_rays.py): the two-level walk."""
    s = _new()
    floor, red = s.matte((0.6, 0.5, 0.4)), s.matte((0.7, 0.2, 0.2))
    s.add_quad((-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3), floor)
    P = np.float32([(0, 1, 0), (-0.6, 0, -0.6), (0.6, 0, -0.6), (0.6, 0, 0.6), (-0.6, 0, 0.6)])
    o = s.add_object([dict(P=P, idx=np.int32([(0, 2, 1), (0, 3, 2), (0, 4, 3), (0, 1, 4)]), material=red)])
    a = np.float64((1.0, 2.0, 0.5)) / np.linalg.norm((1.0, 2.0, 0.5))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K, (0.3, 0.4, 0.2)
    s.add_instance(o, m.astype(np.float32))
    _hidden_light(s)
    return s


def _rays(o, d, t_max=INF):
    """(H, W, ns, 8) records from origins and directions of shape (H, W, ns, 3) (broadcast)."""
    o, d = np.broadcast_arrays(np.asarray(o, np.float32), np.asarray(d, np.float32))
    r = np.zeros(o.shape[:-1] + (8,), np.float32)
    r[..., 0:3], r[..., 3], r[..., 4:7] = o, t_max, d
    return r


def _toward(eye, targets):
    t = np.asarray(targets, np.float64)
    d = t - np.float64(eye)
    return _rays(np.float32(eye), (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32))


def _upload(gpu_host, desc):
    h = gpu_host.HostScene(desc)
    h.upload(0)
    return h


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n_ao", [1, 3, 8])
def test_open_ground_is_exactly_one(gpu_host, n_ao):
    """Nothing above a ground quad: every occlusion ray is clear. A spawned ray that met its own surface, or left on the wrong side, would give ao < 1 - down to grazing
    incidence (89 degrees) and grazing occlusion rays. |d . n| is |d.y| here: products with exact zeros, 4 ulp allowed.
    t = length(p - o) is checked loosely: p carries the closest-hit kernel's float32 barycentrics, whose edge functions on this 400-unit quad are differences of
    products of ~4e4 rounded to 2^-24 each against a determinant of that order - ~1e-5 relative at grazing incidence, the scene's conditioning and not this integrator's;
    1e-4 relative catches a wrong point or a wrong origin."""
    h = _upload(gpu_host, _ground(xres=16, yres=4))
    ang = np.radians(np.concatenate([np.linspace(0, 80, 48), np.linspace(80, 89, 208)])).reshape(4, 16, 4)
    az = np.linspace(0, 2 * np.pi, 256).reshape(4, 16, 4)
    d = np.stack([np.sin(ang) * np.cos(az), -np.cos(ang), np.sin(ang) * np.sin(az)], axis=-1).astype(np.float32)
    d[1] *= np.float32(2.5)   # Normal::li takes ray.d as given, not normalised
    rays = _rays(np.float32((0.3, 1.0, -0.2)), d)
    out, st = h.render_rays_ao(rays, n_ao)
    want_dn = np.abs(d[..., 1].astype(np.float64))
    want_t = np.linalg.norm(d.astype(np.float64), axis=-1) * (1.0 / np.abs(d[..., 1].astype(np.float64)))
    ulp = np.abs(out[..., 1].astype(np.float64) - want_dn) / np.spacing(want_dn.astype(np.float32))
    print(f"\nAO 1 n = {n_ao}: ao in [{out[..., 0].min()}, {out[..., 0].max()}], status {np.unique(out[..., 3])}, |d.n| off by at most {ulp.max():.2f} ulp, "
          f"t relative {np.abs(out[..., 2] / want_t - 1).max():.2e}; rays {st['camera_rays']} / {st['rays_closest']} / {st['rays_shadow']}")
    assert np.array_equal(out[..., 0], np.ones_like(out[..., 0])) and not out[..., 3].any()
    assert ulp.max() <= 4
    assert np.abs(out[..., 2] / want_t - 1).max() < 1e-4
    assert (st["camera_rays"], st["rays_closest"], st["rays_shadow"]) == (256, 256, 256 * n_ao)


# ---------------------------------------------------------------------------------------------- 2
def test_sealed_cube_is_exactly_zero_and_max_distance_opens_it(gpu_host):
    edge = 2.0
    h = _upload(gpu_host, _cube(edge))
    rng = np.random.default_rng(5)
    o = rng.uniform(-0.8, 0.8, (8, 8, 2, 3)).astype(np.float32)
    d = rng.normal(size=(8, 8, 2, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    out, st = h.render_rays_ao(_rays(o, d), 8)
    print(f"\nAO 2 sealed cube: ao max {out[..., 0].max()}, status {np.unique(out[..., 3])}, occlusion rays {st['rays_shadow']}")
    assert not out[..., 0].any() and not out[..., 3].any() and st["rays_shadow"] == 8 * 128
    axes = np.float32([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]).reshape(2, 3, 1, 3)
    rays = _rays(np.zeros(3, np.float32), np.broadcast_to(axes, (2, 3, 4, 3)))
    near, _ = h.render_rays_ao(rays, 8, max_distance=1e-3 * edge)
    far, _ = h.render_rays_ao(rays, 8)
    print(f"AO 2 face centres: max_distance 1e-3 edge -> ao {np.unique(near[..., 0])}, inf -> {np.unique(far[..., 0])}, t {np.unique(near[..., 2])}")
    assert np.array_equal(near[..., 0], np.ones_like(near[..., 0])) and not far[..., 0].any()
    assert np.array_equal(near[..., 1:], far[..., 1:]) and np.abs(near[..., 2] - 1.0).max() <= 1e-6 and np.array_equal(near[..., 1], np.ones_like(near[..., 1]))


# ---------------------------------------------------------------------------------------------- 3
def test_status_of_misses_and_skipped_rays(gpu_host):
    h = _upload(gpu_host, _ground())
    o = np.float32((0.0, 2.0, 0.0))
    down, up = np.float32((0.1, -1.0, 0.2)), np.float32((0.1, 1.0, 0.2))
    rays = _rays(o, np.broadcast_to(down, (4, 4, 2, 3))).copy()
    rays[0, :, :, 4:7] = up                          # leaves the scene
    rays[1, :, 0, 3], rays[1, :, 1, 3] = 0.0, -1.0   # not traced
    rays[2, :, 0, 3] = np.nan                        # not traced
    rays[2, :, 1, 3] = 1.5                           # |d| = 1.02..: the ground is at t = 2, past t_max
    out, st = h.render_rays_ao(rays, 3)
    print(f"\nAO 3 status: miss {np.unique(out[0].reshape(-1, 4), axis=0)}, skipped {np.unique(out[1].reshape(-1, 4), axis=0)} {np.unique(out[2, :, 0], axis=0)}, "
          f"short {np.unique(out[2, :, 1], axis=0)}, hit status {np.unique(out[3, ..., 3])}; camera_rays {st['camera_rays']}, occlusion rays {st['rays_shadow']}")
    assert np.array_equal(np.unique(out[0].reshape(-1, 4), axis=0), np.float32([[0, 0, 0, 1]]))
    assert np.array_equal(np.unique(out[1].reshape(-1, 4), axis=0), np.float32([[0, 0, 0, 2]])) and np.array_equal(np.unique(out[2, :, 0], axis=0), np.float32([[0, 0, 0, 2]]))
    assert np.array_equal(np.unique(out[2, :, 1], axis=0), np.float32([[0, 0, 0, 1]]))
    assert np.array_equal(out[3, ..., 0], np.ones((4, 2), np.float32)) and not out[3, ..., 3].any()
    assert st["camera_rays"] == 32 - 12 and st["rays_closest"] == 20 and st["rays_shadow"] == 3 * 8


# ---------------------------------------------------------------------------------------------- 4
def _targets(lo, hi, seed, shape=(8, 8, 2)):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, shape + (3,))


RECORD_SCENES = {
    "mesh": (_mesh, (0.3, 4.0, -5.0), ((-2.6, 0.0, -2.6), (2.6, 0.6, 2.6))),
    "sphere": (lambda: _sphere(0.5, 1.0), (0.2, 2.5, -4.0), ((-1.0, 0.0, -1.0), (1.0, 1.4, 1.0))),
    "instanced": (_instanced, (0.0, 2.5, -5.0), ((-1.2, 0.0, -1.2), (1.5, 1.2, 1.5))),
}


@pytest.mark.parametrize("name", list(RECORD_SCENES))
def test_ray_records_against_the_model_and_the_oracle(gpu_host, orc, name):
    make, eye, (lo, hi) = RECORD_SCENES[name]
    desc = make()
    h = _upload(gpu_host, desc)
    W = H = 8
    ns, s0, spp, n_ao = 2, 1, 4, 8
    rays = _toward(eye, _targets(lo, hi, 11))
    out, recs, st = h.render_rays_ao(rays, n_ao, sample0=s0, spp=spp, with_rays=True)
    plain, st2 = h.render_rays_ao(rays, n_ao, sample0=s0, spp=spp)
    assert np.array_equal(bits(out), bits(plain)), "the any-hit epilogue's sum and k_ao_fold's agree"
    assert st["rays_shadow"] == st2["rays_shadow"] == n_ao * int((out[..., 3] == 0).sum())
    geo = ao_model.Geometry(desc)
    oracle = orc.OracleScene(desc)
    o, d = rays[..., 0:3].reshape(-1, 3).astype(np.float64), rays[..., 4:7].reshape(-1, 3).astype(np.float64)
    rec = oracle.trace(rays.reshape(-1, 8))   # (t, prim, b0, b1): the closest-hit record, which the project holds bit-equal to the device's
    hit = rec["prim"] >= 0
    p, n, perr3, residual, sin_theta = geo.from_hit_records(o, d, np.where(hit, rec["t"], 0.0), rec["b0"], rec["b1"])
    status, dn_dev = out[..., 3].reshape(-1), out[..., 1].reshape(-1).astype(np.float64)
    dn_err = np.abs(dn_dev - np.abs((d * n).sum(1)))
    flat_hit, quadric_hit = hit & (sin_theta == 1.0), hit & (sin_theta != 1.0)
    t_err = np.abs(out[..., 2].reshape(-1).astype(np.float64) - np.linalg.norm(p - o, axis=1))[hit]
    on_sphere = f" and {dn_err[quadric_hit].max():.2e} on the sphere (sin theta >= {sin_theta[quadric_hit].min():.3f})" if quadric_hit.any() else ""
    print(f"\nAO 4 {name}: {int(hit.sum())} of {hit.size} rays hit; the record's point lies within {residual[hit].max():.2e} of o + t d; |d.n| within "
          f"{dn_err[flat_hit].max():.2e} on triangles{on_sphere}, t within {t_err.max():.2e} of the model's; status agrees: {bool(np.array_equal(status == 0, hit))}")
    # no ray is set aside. The primitive is the one the record's own (t, b0, b1) name (ao_model.Geometry.from_hit_records); 1e-4: float32 t and barycentrics on scenes of
    # extent 8. |d.n| on a triangle: float32 products of a unit d with a float32-rounded n, three roundings of 2^-24 each and the normal's own -> 1e-6. On a sphere hit.n is
    # normalize(cross(dpdu, dpdv)) from the hit's float32 phi and theta (sphere.rs:178-214): some ten roundings of 2^-24, each amplified by at most 1 / sin(theta) - the
    # scene's hits keep sin(theta) >= 0.1 (asserted) -> 10 * 2^-24 / 0.1 = 6e-6 -> 1e-5. t = |p - o| <= 8 -> 2e-6
    assert np.array_equal(status == 0, hit) and np.array_equal(status == 1, ~hit) and hit.sum() >= 64
    assert residual[hit].max() < 1e-4 and dn_err[flat_hit].max() <= 1e-6 and t_err.max() <= 2e-6
    assert not quadric_hit.any() or (sin_theta[quadric_hit].min() >= 0.1 and dn_err[quadric_hit].max() <= 1e-5)
    assert quadric_hit.any() == (name == "sphere")
    recs = recs.reshape(-1, n_ao, 8)
    perr = np.linalg.norm(perr3, axis=1)
    worst_w, worst_o, worst_q, flips_skipped, wrong_side = 0.0, 0.0, 0.0, 0, 0
    for i in np.nonzero(hit)[0]:
        y, x, sl = np.unravel_index(i, (H, W, ns))
        u = ao_model.sample_u(orc, spp, DIMS, int(y * W + x), s0 + int(sl), n_ao)
        w, dn = ao_model.ao_directions(u, n[i])
        got_w = recs[i, :, 4:7]
        near = np.abs(dn) < 1e-6   # the float32 normal may put such a w on the other side
        flips_skipped += int(near.sum())
        diff = np.abs(got_w.astype(np.float64) - w.astype(np.float64)).max(axis=1)
        diff = np.where(near, np.minimum(diff, np.abs(got_w.astype(np.float64) + w.astype(np.float64)).max(axis=1)), diff)
        worst_w = max(worst_w, float(diff.max()))
        assert np.array_equal(recs[i, :, 3], np.full(n_ao, np.inf, np.float32))
        og = recs[i, :, 0:3].astype(np.float64)
        side = ((og - p[i]) @ n[i]) * np.sign(got_w.astype(np.float64) @ n[i])   # the float64 plane through p (a sphere: its tangent plane, which the sphere lies behind)
        wrong_side += int((side < 0).sum())
        bound = 2 * perr[i] + 2 * np.spacing(np.float32(np.abs(p[i]).max()))
        worst_o = max(worst_o, float((np.abs(og - p[i]).max(axis=1) / bound).max()))   # every component
        worst_q = max(worst_q, float((np.abs(og - p[i]).max(axis=1) / bound).max()) if quadric_hit[i] else 0.0)
    print(f"AO 4 {name}: directions within {worst_w / EPS:.2f} x 2^-24 of the model (4 allowed), {flips_skipped} near-tangent samples compared up to sign; "
          f"origins: {wrong_side} on the wrong side, worst distance from the float64 p {worst_o:.3f} of the bound 2 |p_error| + 2 ulp(|p|) (on the sphere: {worst_q:.3f})")
    assert worst_w <= 4 * EPS and wrong_side == 0 and worst_o <= 1.0
    # every record's answer is the oracle's any-hit answer for that record, and ao is their count
    cast = status == 0
    assert not recs[~cast].any(), "zeros for a miss"
    flat = recs[cast].reshape(-1, 8).copy()
    flags = flat[:, 7].copy()
    flat[:, 7] = 0
    occ = oracle.trace(flat, any_hit=True)["occluded"]
    print(f"AO 4 {name}: {int(occ.sum())} of {occ.size} records occluded (oracle), device flags differ in {int((occ != (flags == 1)).sum())}, values {np.unique(flags)}")
    assert np.isin(flags, (0.0, 1.0)).all() and np.array_equal(occ, flags == 1) and 0 < occ.sum() < occ.size
    want = ao_model.ao_value(flags.reshape(-1, n_ao) == 1)
    assert np.array_equal(bits(out[..., 0].reshape(-1)[cast]), bits(want))


# ---------------------------------------------------------------------------------------------- 5
def test_cone_under_a_sphere(gpu_host):
    """A sphere of radius r with its centre h above the hit point blocks the cone sin(theta) = r / h: the clear fraction of a uniformly sampled hemisphere is
    cos(theta) = sqrt(1 - r^2 / h^2). 4096 rays x 8 samples at the one point; 5 sigma of the binomial."""
    r, hgt, n_ao = 0.5, 1.0, 8
    h = _upload(gpu_host, _sphere(r, hgt, xres=64, yres=64, spp=1))
    rays = _rays(np.float32((0.0, 0.25, 0.0)), np.broadcast_to(np.float32((0.0, -1.0, 0.0)), (64, 64, 1, 3)))
    out, st = h.render_rays_ao(rays, n_ao, spp=1)
    p = np.sqrt(1 - (r / hgt) ** 2)
    N = 4096 * n_ao
    mean = float(out[..., 0].astype(np.float64).mean())
    print(f"\nAO 5 cone: mean ao {mean:.5f}, expected {p:.5f}, difference {abs(mean - p):.5f} (5 sigma = {5 * np.sqrt(p * (1 - p) / N):.5f})")
    assert not out[..., 3].any() and np.abs(out[..., 2] - 0.25).max() <= 1e-6
    assert abs(mean - p) <= 5 * np.sqrt(p * (1 - p) / N)


# ---------------------------------------------------------------------------------------------- 6
def test_masks(gpu_host):
    def scene(**mask):
        s = _ground(half=20.0)
        s.add_quad((-5, 1, -5), (-5, 1, 5), (5, 1, 5), (5, 1, -5), s.matte((0.5, 0.5, 0.5)), **mask)
        return s
    d = np.broadcast_to(np.float32((0.05, -1.0, 0.02)), (4, 4, 2, 3))
    # shadowalpha = 0: intersect_p passes the quad over - from below it occludes nothing (scene.intersect still meets it: from above it is the hit)
    h = _upload(gpu_host, scene(shadow_alpha=0.0))
    below, _ = h.render_rays_ao(_rays(np.float32((0.0, 0.5, 0.0)), d), 8)
    above, _ = h.render_rays_ao(_rays(np.float32((0.0, 2.0, 0.0)), d), 8)
    # alpha = 0: neither hit by the camera ray nor an occluder
    h2 = _upload(gpu_host, scene(alpha=0.0))
    through, _ = h2.render_rays_ao(_rays(np.float32((0.0, 2.0, 0.0)), d), 8)
    # no mask: the control - the ground under the quad is mostly occluded
    h3 = _upload(gpu_host, scene())
    ctrl, _ = h3.render_rays_ao(_rays(np.float32((0.0, 0.5, 0.0)), d), 8)
    tl = np.float64(np.linalg.norm(d[0, 0, 0].astype(np.float64)))
    print(f"\nAO 6 masks: shadowalpha below {np.unique(below[..., 0])} t {below[0, 0, 0, 2]:.4f}, above t {above[0, 0, 0, 2]:.4f}; alpha: ao {np.unique(through[..., 0])} "
          f"t {through[0, 0, 0, 2]:.4f}; unmasked control mean ao {ctrl[..., 0].mean():.3f}")
    assert np.array_equal(below[..., 0], np.ones_like(below[..., 0])) and abs(below[0, 0, 0, 2] - 0.5 * tl) < 1e-4
    assert abs(above[0, 0, 0, 2] - 1.0 * tl) < 1e-4 and np.array_equal(above[..., 0], np.ones_like(above[..., 0]))
    assert np.array_equal(through[..., 0], np.ones_like(through[..., 0])) and abs(through[0, 0, 0, 2] - 2.0 * tl) < 1e-4 and not through[..., 3].any()
    assert ctrl[..., 0].mean() < 0.2


# ---------------------------------------------------------------------------------------------- 7
@pytest.fixture(scope="module")
def sphere_call(gpu_host):
    desc = _sphere(0.5, 1.0)
    h = _upload(gpu_host, desc)
    rays = _toward((0.2, 2.5, -4.0), _targets((-1.5, 0.0, -1.5), (1.5, 1.4, 1.5), 3, (8, 8, 4)))
    out, st = h.render_rays_ao(rays, 3, spp=4)
    return h, rays, out, st


def test_sample_ranges_device_buffers_and_long_records(gpu_host, sphere_call):
    import torch
    h, rays, out, st = sphere_call
    a, _ = h.render_rays_ao(rays[:, :, 0:2], 3, sample0=0, spp=4)
    b, _ = h.render_rays_ao(rays[:, :, 2:4], 3, sample0=2, spp=4)
    assert np.array_equal(bits(np.concatenate([a, b], axis=2)), bits(out)) and 0 < out[..., 0].mean() < 1
    d_rays = torch.from_numpy(rays).cuda()
    d_out = torch.zeros((8, 8, 4, 4), dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((8, 8, 4, 3, 8), dtype=torch.float32, device="cuda")
    got, got_recs, _ = h.render_rays_ao(d_rays, 3, spp=4, with_rays=True, device_out=d_out, device_rays_out=d_recs)
    torch.cuda.synchronize()
    _, host_recs, _ = h.render_rays_ao(rays, 3, spp=4, with_rays=True)
    assert np.array_equal(bits(got.cpu().numpy()), bits(out)) and np.array_equal(bits(got_recs.cpu().numpy()), bits(host_recs))
    long = np.zeros((8, 8, 4, 20), np.float32)
    long[..., :8] = rays
    long[..., 8:] = np.random.default_rng(1).normal(size=(8, 8, 4, 12))   # differentials are not read
    c, _ = h.render_rays_ao(long, 3, spp=4)
    assert np.array_equal(bits(c), bits(out))
    print(f"\nAO 7 ranges, device buffers, 20-float records: all bit-identical; mean ao {out[..., 0].mean():.3f}, {st['rays_shadow']} occlusion rays")


def test_counters_and_timers(sphere_call):
    """RT_FLAG_COUNT_TRAVERSAL and RT_FLAG_TIME_KERNELS: the counting walks give the same samples and fill the nodes_ / tris_ counters of both kinds of ray; the timed call
    reports the three stages and nothing of the path integrator's."""
    h, rays, out, st = sphere_call
    counted, sc = h.render_rays_ao(rays, 3, spp=4, count_traversal=True)
    timed, tk = h.render_rays_ao(rays, 3, spp=4, time_kernels=True)
    print(f"\nAO 7 counters: nodes closest / occlusion {sc['nodes_closest']} / {sc['nodes_shadow']}, tris {sc['tris_closest']} / {sc['tris_shadow']}; uncounted call: "
          f"{st['nodes_closest']} / {st['nodes_shadow']}; timers closest {tk['ms_trace_closest']:.3f} any {tk['ms_trace_any']:.3f} shade {tk['ms_shade']:.3f} ms, "
          f"mis {tk['ms_trace_mis']:.3f} resolve {tk['ms_resolve']:.3f} lightdist {tk['ms_lightdist']:.3f}")
    assert np.array_equal(bits(counted), bits(out)) and np.array_equal(bits(timed), bits(out))
    assert min(sc["nodes_closest"], sc["nodes_shadow"], sc["tris_closest"], sc["tris_shadow"]) > 0 and st["nodes_closest"] == st["nodes_shadow"] == 0
    assert (sc["camera_rays"], sc["rays_closest"], sc["rays_shadow"], sc["rays_mis"]) == (st["camera_rays"], st["rays_closest"], st["rays_shadow"], 0)
    # one pass: one closest-hit launch (launches_trace_closest = path + MIS launches), one k_ao_rays and one any-hit launch per occlusion sample
    assert (st["launches_trace_closest"], st["launches_trace_path"], st["launches_trace_mis"], st["launches_trace_shadow"], st["launches_shade"], st["n_passes"]) == (1, 1, 0, 3, 3, 1)
    assert min(tk["ms_trace_closest"], tk["ms_trace_any"], tk["ms_shade"]) > 0 and tk["ms_trace_mis"] == tk["ms_resolve"] == 0   # (ms_lightdist: the stage is timed around nothing - no table is built)


def _splat(ao, pf, table, rx, ry, cropped):
    """FilmTile::add_sample (film.rs:298-361) for L = grey(ao) in float64, the footprint and table index in float32 in the device's order; XYZ as merge_film_tile."""
    f32 = np.float32
    x_lo, y_lo, x_hi, y_hi = cropped
    dx, dy = pf[..., 0] - f32(0.5), pf[..., 1] - f32(0.5)
    inv_rx, inv_ry = f32(1.0) / f32(rx), f32(1.0) / f32(ry)
    x0 = np.maximum(np.ceil(dx - f32(rx)), f32(x_lo)).astype(np.int64); y0 = np.maximum(np.ceil(dy - f32(ry)), f32(y_lo)).astype(np.int64)
    x1 = np.minimum(np.floor(dx + f32(rx) + f32(1.0)), f32(x_hi)).astype(np.int64); y1 = np.minimum(np.floor(dy + f32(ry) + f32(1.0)), f32(y_hi)).astype(np.int64)
    want = np.zeros((y_hi - y_lo, x_hi - x_lo, 2), np.float64)
    span = int(max((x1 - x0).max(), (y1 - y0).max()))
    for j in range(span):
        for i in range(span):
            yy, xx = y0 + j, x0 + i
            m = (yy < y1) & (xx < x1)
            fy = np.abs((yy.astype(f32) - dy) * inv_ry * f32(16.0)); fx = np.abs((xx.astype(f32) - dx) * inv_rx * f32(16.0))
            iy = np.minimum(np.floor(fy), f32(15.0)).astype(np.int64); ix = np.minimum(np.floor(fx), f32(15.0)).astype(np.int64)
            fw = table[np.clip(iy * 16 + ix, 0, 255)].astype(np.float64)
            np.add.at(want[..., 0], (yy[m] - y_lo, xx[m] - x_lo), ao[m].astype(np.float64) * fw[m])
            np.add.at(want[..., 1], (yy[m] - y_lo, xx[m] - x_lo), fw[m])
    c = lambda *v: sum(np.float64(np.float32(x)) for x in v)
    L = want[..., 0]
    return np.stack([c(0.412453, 0.357580, 0.180423) * L, c(0.212671, 0.715160, 0.072169) * L, c(0.019334, 0.119193, 0.950227) * L, want[..., 1]], axis=-1)


def _cornell(gpu_host, gaussian):
    from rustracer_amd.scene_desc import FILTER_GAUSSIAN
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(16, 16, 4)
    d.film.filter_kind, d.film.filter_params = (FILTER_GAUSSIAN, (1.5, 1.5, 2.0, 0.0)) if gaussian else (0, (0.5, 0.5, 0.0, 0.0))
    return _upload(gpu_host, d)


@pytest.fixture(scope="module")
def cornell(gpu_host):
    """Under the box filter (a sample reaches its own pixel only: the film kernel's sums have one order, so films compare bit for bit): rt_render, rt_render_ao, rt_render."""
    h = _cornell(gpu_host, False)
    before, _ = h.render()
    film, st = h.render_ao(3)
    after, _ = h.render()
    return h, before, film, st, after


def test_frame_is_the_splat_of_the_ray_entrys_samples(gpu_host, cornell):
    _, before, box_film, _, _ = cornell
    assert np.array_equal(bits(box_film[..., 3]), bits(before[..., 3])), "the weight plane is rt_render's"
    h = _cornell(gpu_host, True)   # a Gaussian of radius 1.5: sample bounds wider than the film, every sample reaches up to 16 pixels
    film, st = h.render_ao(3)
    setup = h.setup()
    cam_rays, pf = h.camera_rays()
    out, st_r = h.render_rays_ao(cam_rays, 3)
    sb = [int(v) for v in setup["sample_bounds"]]
    assert cam_rays.shape[:3] == (sb[3] - sb[1], sb[2] - sb[0], 4)
    want = _splat(out[..., 0], pf, setup["filter_table"].astype(np.float32), 1.5, 1.5, [int(v) for v in setup["cropped"]])
    err = float(np.linalg.norm(film.astype(np.float64) - want) / np.linalg.norm(want))
    print(f"\nAO 7 frame vs splat of rt_render_rays_ao over rt_camera_rays' records: relative L2 {err:.3e}; film mean Y {film[..., 1].mean():.4f}, "
          f"rays {st['camera_rays']} / {st['rays_shadow']} vs {st_r['camera_rays']} / {st_r['rays_shadow']}")
    assert err <= 1e-6 and film[..., 1].mean() > 0.05
    assert (st["camera_rays"], st["rays_closest"], st["rays_shadow"]) == (st_r["camera_rays"], st_r["rays_closest"], st_r["rays_shadow"])
    assert st["rays_shadow"] == 3 * int((out[..., 3] == 0).sum())


def test_two_shards_merge_to_the_unsharded_film_under_the_box_filter(gpu_host):
    from rustracer_amd.distributed import touched_rows
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(16, 16, 4)
    d.film.filter_kind, d.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)
    h = _upload(gpu_host, d)
    whole, _ = h.render_ao(3)
    parts = [h.render_ao(3, rank=r, world_size=2)[0] for r in range(2)]
    st = h.setup()
    rows = touched_rows([int(v) for v in st["cropped"]], [int(v) for v in st["sample_bounds"]], 1, 2, 0.5)   # distributed.merge_film's arithmetic without a process group
    merged = parts[0].copy()
    merged[rows] += parts[1][rows]
    differ = int((bits(merged) != bits(whole)).sum())
    print(f"\nAO 7 shards: merged film differs from the unsharded one in {differ} words; rank films non-zero: {[bool(p.any()) for p in parts]}")
    assert differ == 0 and all(p.any() for p in parts) and whole[..., 1].mean() > 0.05


# ---------------------------------------------------------------------------------------------- 8
def test_an_ao_call_leaves_the_path_frame_as_it_was(cornell):
    h, before, film, _, after = cornell
    differ = int((bits(before) != bits(after)).sum())
    print(f"\nAO 8: rt_render before / after rt_render_ao on the scene differ in {differ} words; the AO film differs from it in {int((bits(film) != bits(before)).sum())}")
    assert differ == 0 and not np.array_equal(film[..., :3], before[..., :3])
