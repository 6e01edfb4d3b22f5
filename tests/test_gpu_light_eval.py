"""rt_light_eval (HostScene.light_eval): light pick, Light::sample_li, Light::pdf_li, Light::le and the visibility segment PER QUERY, held to the float64 radiometric
model of tests/radiometry_model.py and to definitions - never to the code under test, never to the oracle.

Scenes, points and lights are tests/radiometry_cases.py's. The unbiasedness check uses the sample design of tests/light_eval_cases.py (B = 256 blocks of 8 x 8
jittered u_light per point and light; the statistic over the block means) on the points tests/test_light_eval_cpu.py fixes with its float64 stand-in. One device
call per case and light serves the per-query checks, the pdf_li check and the statistic. Every test prints its record before it asserts."""
import ctypes as C

import numpy as np
import pytest

import light_eval_cases as lc
import radiometry_cases as rc
import radiometry_model as rm

pytestmark = pytest.mark.gpu

F32_ULP = 2.0 ** -24
_SCENES, _RUNS = {}, {}


@pytest.fixture(autouse=True, scope="module")
def _a_device_error_ends_the_session(gpu_host):
    """A HIP error (RT_ERR_HIP, -3) from rt_light_eval ends the run there: nothing more is started on a device that has faulted."""
    orig = gpu_host.HostScene.light_eval

    def guarded(self, *a, **k):
        try:
            return orig(self, *a, **k)
        except gpu_host.BackendError as e:
            if "failed (-3)" in str(e):
                pytest.exit(f"device error, nothing more is started: {e}", returncode=3)
            raise
    gpu_host.HostScene.light_eval = guarded
    yield
    gpu_host.HostScene.light_eval = orig


def scene(gpu_host, name):
    if name not in _SCENES:
        c = lc.case(name) if name in lc.AREA_CASES else rc.case(name)
        h = gpu_host.HostScene(c.desc)
        h.upload(0)
        _SCENES[name] = (c, h)
    return _SCENES[name]


def run(gpu_host, name, k, visibility=False):
    """Light k of the case on the design: every point of the case x 16 384 u_light, and a second call that asks pdf_li / le about the returned wi. Kept: the
    first call's records (P, N, 20) and floats 16-19 of the second (P, N, 4), read-only; a test that is the last to need them drops them."""
    key = (name, k, visibility)
    if key not in _RUNS:
        c, h = scene(gpu_host, name)
        P = c.x.shape[0]
        u = np.zeros((P, lc.N, 3), np.float32)
        u[..., 1:] = lc.design(P).reshape(P, lc.N, 2)
        rep = lambda a: np.repeat(np.float32(a), lc.N, axis=0)
        r = h.light_eval(rep(c.x), rep(c.n), u.reshape(-1, 3), light=k, visibility=visibility)
        r2 = h.light_eval(rep(c.x), rep(c.n), u.reshape(-1, 3), light=k, wi=r["wi"])
        a, b = r["raw"].reshape(P, lc.N, 20), r2["raw"].reshape(P, lc.N, 20)
        assert np.array_equal(a[..., :15], b[..., :15]) and np.all(b[..., 15] == -1.0)      # the wi query changes nothing else
        b = b[..., 16:].copy()
        a.setflags(write=False)
        b.setflags(write=False)
        _RUNS[key] = (a, b)
    return _RUNS[key]


def estimator(c, raw, use_v):
    """Li max(0, n . wi) / pdf (x V) per query, green channel, float64 (P, N)."""
    wi, pdf = np.float64(raw[..., 5:8]), np.float64(raw[..., 8])
    cos = np.maximum((wi * c.n[:, None, :]).sum(-1), 0.0)
    e = np.where(pdf > 0, np.float64(raw[..., 3]) * cos / np.where(pdf > 0, pdf, 1.0), 0.0)
    return e * (raw[..., 15] == 1.0) if use_v else e


def block_means(e):
    return e.reshape(e.shape[0], lc.BLOCKS, lc.CELLS).mean(axis=2)


# ------------------------------------------------------------------------------------------------ 1. delta lights
def test_point_light_in_closed_form(gpu_host):
    c, h = scene(gpu_host, "point")
    l = c.lights[0]
    p, pos = np.float64(np.float32(c.x)), np.float64(np.float32(l.pos))
    r = h.light_eval(c.x, c.n, np.random.default_rng(1).random((p.shape[0], 3)), light=0)
    r2 = h.light_eval(c.x, c.n, np.zeros((p.shape[0], 3)), light=0, wi=r["wi"])
    w = pos - p
    d2 = (w * w).sum(-1)
    li = np.float64(np.float32(l.i)) / (4.0 * np.pi * d2)[:, None]          # I / (4 pi r^2): the reference's quirk (light/point.rs:50)
    wi = w / np.sqrt(d2)[:, None]
    dev_li, dev_wi = float(np.abs(r["li"] / li - 1.0).max()), float(np.abs(r["wi"] - wi).max())
    print(f"\nLIGHT_EVAL point: {p.shape[0]} queries, Li rel {dev_li:.2e}, wi abs {dev_wi:.2e}, p1 == pos {np.array_equal(r['p1'], np.tile(np.float32(l.pos), (p.shape[0], 1)))}, "
          f"pdf {np.unique(r['pdf'])}, pick pdf {np.unique(r['pick_pdf'])}, pdf_li {np.unique(r2['pdf_li'])}, visible {np.unique(r['visible'])}")
    assert dev_li <= 1e-6 and dev_wi <= 1e-6
    assert np.array_equal(r["p1"], np.tile(np.float32(l.pos), (p.shape[0], 1))) and np.all(r["n1"] == 0.0)
    assert np.all(r["pdf"] == 1.0) and np.all(r["pick_pdf"] == 1.0) and np.all(r["light"] == 0) and np.all(r["visible"] == -1)
    assert np.all(r2["pdf_li"] == 0.0) and np.all(r2["le"] == 0.0) and np.all(r["pdf_li"] == 0.0)
    assert np.array_equal(r["raw"][:, :16], r2["raw"][:, :16])            # a delta light reads no u


def test_distant_light_in_closed_form(gpu_host):
    c, h = scene(gpu_host, "distant")
    l = c.lights[0]
    p = np.float64(np.float32(c.x))
    r = h.light_eval(c.x, c.n, np.zeros((p.shape[0], 3)), light=0)
    r2 = h.light_eval(c.x, c.n, np.zeros((p.shape[0], 3)), light=0, wi=r["wi"])
    # p1 = p + wi * 2 * world radius; the world is the pyramid's box [-1, 1] x [0, 1] x [-1, 1], its bounding sphere has radius 1.5 (bounds.rs bounding_sphere)
    p1 = p + l.w * 3.0
    dev_li, dev_wi, dev_p1 = float(np.abs(r["li"] / l.l - 1.0).max()), float(np.abs(r["wi"] - l.w).max()), float((np.abs(r["p1"] - p1).max(axis=1) / np.abs(p1).max(axis=1)).max())
    print(f"\nLIGHT_EVAL distant: {p.shape[0]} queries, Li rel {dev_li:.2e}, wi abs {dev_wi:.2e}, p1 rel {dev_p1:.2e}, pdf {np.unique(r['pdf'])}, pdf_li {np.unique(r2['pdf_li'])}")
    assert dev_li <= 1e-6 and dev_wi <= 1e-6 and dev_p1 <= 1e-6
    assert np.all(r["pdf"] == 1.0) and np.all(r["pick_pdf"] == 1.0) and np.all(r2["pdf_li"] == 0.0) and np.all(r2["le"] == 0.0)


# ------------------------------------------------------------------------------------------------ 2. / 3. area emitters per query
def _on_emitter(l, y):
    """(distance of y (.., 3) float64 from the emitter's surface or outline, the emitter's extent), with the emitter's float32 parameters where the scene rounds them."""
    if isinstance(l, rm.Triangle):
        p = np.float64(np.float32(l.p))
        e1, e2 = p[1] - p[0], p[2] - p[0]
        ng = np.cross(e1, e2)
        ng /= np.linalg.norm(ng)
        q = y - p[0]
        off = np.abs((q * ng).sum(-1))
        m = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
        b = np.linalg.solve(m, np.stack([(q * e1).sum(-1).ravel(), (q * e2).sum(-1).ravel()])).T.reshape(q.shape[:-1] + (2,))
        ext = max(np.linalg.norm(e1), np.linalg.norm(e2), np.linalg.norm(e2 - e1))
        outside = np.maximum(0.0, np.max(np.stack([-b[..., 0], -b[..., 1], b[..., 0] + b[..., 1] - 1.0], axis=-1), axis=-1)) * ext
        return np.maximum(off, outside), ext
    shift = np.float64(np.float32(l.shift))
    q = (y - shift) @ np.float64(np.float32(l.rot))         # object space
    if isinstance(l, rm.Sphere):
        return np.abs(np.linalg.norm(q, axis=-1) - np.float64(np.float32(l.radius))), 2.0 * l.radius
    rho = np.hypot(q[..., 0], q[..., 1])
    if isinstance(l, rm.Disk):
        return np.maximum(np.abs(q[..., 2] - l.height), np.maximum(0.0, rho - np.float64(np.float32(l.radius)))), 2.0 * l.radius
    z0, z1 = np.float64(np.float32(l.z[0])), np.float64(np.float32(l.z[1]))
    phi = np.arctan2(q[..., 1], q[..., 0])
    phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
    sweep = np.maximum(0.0, phi - l.phi_max) * l.radius
    sweep = np.minimum(sweep, (2.0 * np.pi - phi) * l.radius)     # phi just below 0 reads as just below 2 pi
    return np.max(np.stack([np.abs(rho - np.float64(np.float32(l.radius))), np.maximum(0.0, z0 - q[..., 2]), np.maximum(0.0, q[..., 2] - z1), sweep], axis=-1), axis=-1), max(2.0 * l.radius, z1 - z0)


def _cylinder_first_hit(l, o, d):
    """The first intersection of the rays (o, d) (.., 3 float64, world) with the clipped cylinder, in float64: (distance, |n . d| there, the distance of the nearest
    root that decides it from a clip edge - z_min, z_max, phi = 0, phi_max -, whether there is one)."""
    q, dd = (o - np.float64(np.float32(l.shift))) @ np.float64(np.float32(l.rot)), d @ np.float64(np.float32(l.rot))
    rad, z0, z1 = np.float64(np.float32(l.radius)), np.float64(np.float32(l.z[0])), np.float64(np.float32(l.z[1]))
    qa, qb, qc = dd[:, 0] ** 2 + dd[:, 1] ** 2, 2.0 * (dd[:, 0] * q[:, 0] + dd[:, 1] * q[:, 1]), q[:, 0] ** 2 + q[:, 1] ** 2 - rad * rad
    disc = qb * qb - 4.0 * qa * qc
    sq = np.sqrt(np.maximum(disc, 0.0))
    res = []
    for t in ((-qb - sq) / (2.0 * qa), (-qb + sq) / (2.0 * qa)):
        h = q + t[:, None] * dd
        phi = np.arctan2(h[:, 1], h[:, 0])
        phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
        inside = (disc > 0) & (t > 0) & (h[:, 2] > z0) & (h[:, 2] < z1) & (phi < l.phi_max)
        edge = np.min(np.stack([np.abs(h[:, 2] - z0), np.abs(h[:, 2] - z1), np.abs(phi - l.phi_max) * rad, np.minimum(phi, 2.0 * np.pi - phi) * rad]), axis=0)
        cos = np.abs(h[:, 0] * dd[:, 0] + h[:, 1] * dd[:, 1]) / (rad * np.linalg.norm(dd, axis=1))
        res.append((t * np.linalg.norm(dd, axis=1), cos, edge, inside))
    (t0, c0, e0, i0), (t1, c1, e1, i1) = res
    # (a line that grazes the cylinder - its roots closer than 1e-3 of their mean - has no margin: whether it meets the wall at all is a matter of the last bit of wi)
    margin = np.where(disc > 1e-6 * qb * qb, np.where(i0, e0, np.minimum(e0, e1)), 0.0)
    return np.where(i0, t0, t1), np.where(i0, c0, c1), margin, i0 | i1


PER_QUERY_CASES = ("quad", "quad_two_sided", "quad_reversed", "quad_normals", "quad_overhead", "sphere_outside", "sphere_inside", "disk_tilted", "disk_overhead", "cylinder")


@pytest.mark.parametrize("name", PER_QUERY_CASES)
def test_area_emitters_per_query(gpu_host, name):
    """p1 on the emitter, wi = normalize(p1 - p), Li bit-exactly Le where the sample's normal faces p (or the emitter is two-sided) and exactly 0 elsewhere, and the
    pdf: r^2 / (|n_y . w| A) for the shapes sampled by area, 1 / (2 pi (1 - cos theta_max)) for a sphere seen from outside - relative 1e-4 (REL_FLOOR, the v_rcp
    allowance) where |n_y . w| >= 0.01, plus 4 x 2^-24 / (1 - cos theta_max) for the cone. Then pdf_li(returned wi) against that pdf, to 1e-4, on the samples
    tests/light_eval_cases.py's identity_subset picks in float64 from the sample's own distance and cosine; the share of the rest is capped (IDENTITY_CAP) and each of them
    held to a bound made of the number format; a re-intersection that misses (pdf_li = 0: a barycentric below the edge functions' float32 error) is counted, share
    <= 1e-3. The cylinder's samples that face away are held to the float64 first intersection of their ray."""
    c, h = scene(gpu_host, name)
    for k, l in enumerate(rc._flat(c.lights)):
        a, b = run(gpu_host, name, k)
        P = c.x.shape[0]
        p = np.float64(np.float32(c.x))[:, None, :]
        p1, n1, wi, pdf, li = np.float64(a[..., 9:12]), np.float64(a[..., 12:15]), np.float64(a[..., 5:8]), np.float64(a[..., 8]), a[..., 2:5]
        w = p1 - p
        r2 = (w * w).sum(-1)
        wn = w / np.sqrt(r2)[..., None]
        off, ext = _on_emitter(l, p1)
        cos_y = -(n1 * wn).sum(-1)
        le = np.float32(l.le)
        faces = np.ones_like(cos_y, bool) if l.two_sided else cos_y > 0
        sure = l.two_sided | (np.abs(cos_y) > 1e-6)
        li_ok = np.all(np.where(faces[..., None], li == le, li == 0.0), axis=-1)
        outside = lc.sphere_outside(l, c.x[0])
        if outside:
            d2 = ((np.float64(np.float32(l.shift)) - p) ** 2).sum(-1)
            cmax = np.sqrt(np.maximum(0.0, 1.0 - l.radius ** 2 / d2))
            want, allow, well = 1.0 / (2.0 * np.pi * (1.0 - cmax)), rm.REL_FLOOR + 4.0 * F32_ULP / (1.0 - cmax), np.ones_like(pdf, bool)
            want, allow = np.broadcast_to(want, pdf.shape), np.broadcast_to(allow, pdf.shape)
        else:
            well = np.abs(cos_y) >= lc.ILL_COS
            want, allow = r2 / (np.where(well, np.abs(cos_y), 1.0) * lc.area_of(l)), np.full(pdf.shape, rm.REL_FLOOR)
        if c.extra is not None:
            well = well & (c.extra == 0)[:, None]
        pdf_dev = np.where(well, np.abs(pdf / want - 1.0) / allow, 0.0)
        pdf_li = np.float64(b[..., 0])
        not_plane = np.ones_like(sure) if c.extra is None else np.broadcast_to((c.extra == 0)[:, None], sure.shape)
        r, cabs = np.sqrt(r2), np.abs(cos_y)
        # Shape::pdf_wi is the density at the FIRST intersection along wi: that is the sample where it faces p, or the emitter is two-sided (a planar emitter, the
        # inside of a sphere: one intersection). The identity is asked at 1e-4 on lc.identity_subset, decided in float64 from the sample; the rest is counted against
        # lc.IDENTITY_CAP and held to a bound made of the number format alone: two float32 dot products of unit vectors, 8 x 2^-24 / c, and the curved term.
        cand = (pdf > 0) & faces & sure & not_plane
        asked = cand & lc.identity_subset(l, c.x[0], r, cabs)
        left = cand & ~asked
        miss = cand & (pdf_li == 0.0)
        li_dev = np.where(cand & ~miss, np.abs(pdf_li / np.where(pdf > 0, pdf, 1.0) - 1.0), 0.0)
        is_curved = lc.curved(l, c.x[0])
        left_allow = 1e-4 + 8.0 * F32_ULP / np.maximum(cabs, 1e-30) + (lc.curved_term(l, r, cabs) if is_curved else 0.0)
        dev_asked = float(li_dev[asked].max())
        # (first-order, so a bound only while it is small: up to 0.1. Beyond - the silhouette of the cylinder, where the hit may land anywhere along the grazing ray -
        # all that binds the density of a hit on the emitter is that the hit is no nearer than the emitter: pdf_li = 0, a miss, or >= d_min^2 / A)
        lin = left & (left_allow <= 0.1)
        left_ratio = float((li_dev / left_allow)[lin].max()) if lin.any() else 0.0
        floor = np.zeros_like(pdf)
        if isinstance(l, rm.Cylinder):
            po = (p[:, 0, :] - np.float64(np.float32(l.shift))) @ np.float64(np.float32(l.rot))
            floor = np.broadcast_to((np.maximum(np.hypot(po[:, 0], po[:, 1]) - l.radius, 0.0) ** 2 / lc.area_of(l) * (1.0 - 1e-4))[:, None], pdf.shape)
        beyond = left & ~lin
        beyond_ok = bool(np.all((pdf_li[beyond] == 0.0) | (pdf_li[beyond] >= floor[beyond])))
        share, cap = left.sum() / max(1, int(cand.sum())), lc.IDENTITY_CAP["curved" if is_curved else "flat"]
        horizon = int((~sure & not_plane).sum())
        print(f"\nLIGHT_EVAL {name} light {k} ({type(l).__name__}{', from outside' if outside else ''}): {P * lc.N} queries; p1 off the emitter <= {off.max() / ext:.2e} of its extent; "
              f"|wi - normalize(p1 - p)| <= {np.abs(wi - wn).max():.2e}; Li exact {bool(li_ok[sure].all())} ({horizon} samples within 1e-6 of the horizon left out, {int((~sure).sum()) - horizon} "
              f"at points in the emitter's plane), emitting {faces.mean():.3f}; well-conditioned {well.mean():.4f}; pdf deviation <= {np.abs(np.where(well, pdf / want - 1.0, 0.0)).max():.2e} "
              f"({pdf_dev.max():.2f} of the allowance); pdf_li vs pdf on the {int(asked.sum())} samples asked <= {dev_asked:.2e}; left out {int(left.sum())} ({share:.2e}, cap {cap}), "
              f"the worst of the {int(lin.sum())} with a first-order bound at {left_ratio:.2f} of it ({float(li_dev[lin].max()) if lin.any() else 0.0:.2e}), {int(beyond.sum())} beyond it: a miss or no nearer than the emitter {beyond_ok}; re-intersection misses {int(miss.sum())} "
              f"({miss.sum() / max(1, int(cand.sum())):.2e})")
        assert off.max() <= 1e-6 * ext
        assert np.abs(wi - wn).max() <= 1e-6
        assert li_ok[sure].all() and horizon <= 1e-5 * sure.size
        assert np.all(a[..., 0] == k) and np.all(a[..., 1] == 1.0) and np.all(a[..., 15] == -1.0) and np.all(a[..., 16:] == 0.0)
        assert pdf_dev.max() <= 1.0
        assert np.all(b[..., 1:] == 0.0)
        assert cand.sum() >= 0.25 * (pdf > 0).sum()
        assert dev_asked <= 1e-4
        assert share <= cap
        assert left_ratio <= 1.0 and beyond_ok
        assert miss.sum() <= 1e-3 * max(1, int(cand.sum()))
        if isinstance(l, rm.Cylinder):
            # a sample that faces away lies behind the cylinder's own near wall: pdf_wi returns the density of that wall (or of whatever the ray meets first, or 0
            # through the gap). Held to the float64 intersection of the ray (p, wi) with the clipped cylinder, on the hits that stand 1e-4 of the extent off every clip edge
            back = (pdf > 0) & ~faces & sure
            pp = np.broadcast_to(p, wi.shape)[back]
            dist, ch, margin, hit = _cylinder_first_hit(l, pp, wi[back])
            clear = margin >= 1e-4 * ext
            ask_b = clear & hit & lc.identity_subset(l, c.x[0], dist, ch)
            d64 = dist ** 2 / (np.where(hit, ch, 1.0) * lc.area_of(l))
            got = pdf_li[back]
            dev_b = float(np.abs(got[ask_b] / d64[ask_b] - 1.0).max())
            none = clear & ~hit
            print(f"  back-facing samples {int(back.sum())}: first intersection in float64 for {int(hit.sum())}, asked {int(ask_b.sum())} ({ask_b.mean():.3f}), pdf_li vs its density <= {dev_b:.2e}; "
                  f"{int(none.sum())} rays meet nothing, pdf_li = 0 on all of them: {bool(np.all(got[none] == 0.0))}")
            assert ask_b.mean() >= 0.5 and dev_b <= 1e-4
            assert np.all(got[none] == 0.0) and np.all(got[clear & hit] > 0.0)
        if name not in lc.AREA_CASES:
            _RUNS.pop((name, k, False))


def test_infinite_light_pdf_li_agrees_with_sample_li(gpu_host):
    """env_map: pdf_li(returned wi) equals the sample's pdf to 1e-4, leaving out the samples within 4 degrees of a pole of the map (share <= 1e-3, each inside a bound
    made of the number format: see the body) and directions within 1e-4 of a texel width of a bin edge (decided in float64 from the
    sample's own wi; their share <= 1e-3); over the mid-points of the distribution's own 32 x 16 bins (twice the map's resolution) sum pdf_li sin(theta) dtheta dphi = 1 to 1e-5 (pdf sin(theta)
    is constant in each bin); Le at those mid-points is the model's bilinear value to 1e-5, but for the texels next to the sun's edge, where 2^-23 of
    phi x 16 times the thousandfold step is more than that (tests/test_gpu_radiometry.py, test_escaping_rays_see_the_map)."""
    c, h = scene(gpu_host, "env_map")
    env = c.lights[0]
    P = c.x.shape[0]
    u = np.zeros((P, 4096, 3), np.float32)
    u[..., 1:] = lc.design(P)[:, :64].reshape(P, 4096, 2)
    rep = lambda a: np.repeat(np.float32(a), 4096, axis=0)
    r = h.light_eval(rep(c.x), rep(c.n), u.reshape(-1, 3), light=0)
    r2 = h.light_eval(rep(c.x), rep(c.n), u.reshape(-1, 3), light=0, wi=r["wi"])
    wl = np.float64(r["wi"]) @ env.rot
    wl /= np.linalg.norm(wl, axis=1, keepdims=True)
    phi = np.arctan2(wl[:, 1], wl[:, 0])
    phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
    nu, nv = 2 * env.w, 2 * env.h                  # the distribution is tabulated at twice the map's resolution (light/infinite.rs:80)
    s, t = phi / (2.0 * np.pi) * nu, np.arccos(np.clip(wl[:, 2], -1.0, 1.0)) / np.pi * nv
    near = (np.abs(s - np.round(s)) < 1e-4) | (np.abs(t - np.round(t)) < 1e-4)
    pdf, pdf_li = np.float64(r["pdf"]), np.float64(r2["pdf_li"])
    ok = ~near & (pdf > 0)
    dev_all = np.where(ok, np.abs(pdf_li / np.where(pdf > 0, pdf, 1.0) - 1.0), 0.0)
    sin2 = 1.0 - wl[:, 2] ** 2
    wq = int(np.argmax(dev_all))
    print(f"\n  worst pdf_li sample {wq}: light-space theta {np.degrees(np.arccos(wl[wq, 2])):.5f} deg, pdf {pdf[wq]:.6e}, pdf_li {pdf_li[wq]:.6e}, deviation {dev_all[wq]:.3e}; deviations above 1e-4: "
          f"{int((dev_all > 1e-4).sum())}, the largest with sin^2 theta >= 0.01: {dev_all[sin2 >= 0.01].max():.3e}, largest deviation x sin^2 theta / 2^-24 = {(dev_all * sin2).max() / F32_ULP:.2f}")
    # pdf_li takes sin(theta) of theta = acos(w.z), w = w2l wi: the returned wi carries the roundings of l2w (three products and two sums per component) and of the
    # sines and cosines it was made of, w2l adds as many - delta z <= 8 x 2^-24 -, and d sin(theta) / sin(theta) = delta z cos(theta) / sin^2(theta): at a pole of the map the
    # identity is ill-conditioned in float32 whatever the code does. The identity is asked at 1e-4 where that term is at most 1e-4 (sin^2(theta) >= 4.8e-3: all but 4 degrees
    # around each pole), decided in float64 from the sample's own wi as the bin edges are; the polar samples are counted against the cap the issue gives the bin
    # edges, 1e-3, and each is held to 1e-4 plus the term
    polar = ok & (8.0 * F32_ULP / np.maximum(sin2, 1e-30) > 1e-4)
    asked = ok & ~polar
    dev = float(dev_all[asked].max())
    polar_ratio = float((dev_all / (1e-4 + 8.0 * F32_ULP / np.maximum(sin2, 1e-30)))[polar].max()) if polar.any() else 0.0
    norm = np.abs(np.linalg.norm(np.float64(r["wi"]), axis=1) - 1.0).max()
    far = np.abs(r["p1"] - (np.float64(rep(c.x)) + 3.0 * np.float64(r["wi"]))).max()
    th, ph = (np.arange(nv) + 0.5) * np.pi / nv, (np.arange(nu) + 0.5) * 2.0 * np.pi / nu
    tt, pp = np.meshgrid(th, ph, indexing="ij")
    mid = np.stack([np.sin(tt) * np.cos(pp), np.sin(tt) * np.sin(pp), np.cos(tt)], axis=-1).reshape(-1, 3) @ env.rot.T
    q = h.light_eval(np.zeros((mid.shape[0], 3)), None, np.zeros((mid.shape[0], 3)), light=0, wi=mid)
    total = float((np.float64(q["pdf_li"]) * np.sin(tt).reshape(-1)).sum() * (np.pi / nv) * (2.0 * np.pi / nu))
    img = np.float64(rc.env_image())
    ring = np.stack([np.roll(np.pad(img, ((1, 1), (0, 0), (0, 0)), mode="edge"), (dy, dx), axis=(0, 1))[1:-1] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    calm = np.repeat(np.repeat((ring.max(axis=0) / ring.min(axis=0)).max(axis=-1) < 2.0, 2, axis=0), 2, axis=1).reshape(-1)
    le_dev = np.abs(np.float64(q["le"]) / env.radiance(mid) - 1.0)[calm].max()
    print(f"\nLIGHT_EVAL env_map: {pdf.size} queries, {int(near.sum())} within 1e-4 texel of a bin edge ({near.mean():.2e}), pdf_li vs pdf on the {int(asked.sum())} asked <= {dev:.2e}, {int(polar.sum())} polar samples ({polar.mean():.2e}) left out, the worst at {polar_ratio:.2f} of its format bound ({float(dev_all[polar].max()) if polar.any() else 0.0:.2e}), | |wi| - 1 | <= {norm:.2e}, "
          f"|p1 - (p + 2 R wi)| <= {far:.2e}; sum over bin mid-points of pdf_li sin(theta) dtheta dphi = {total:.7f}; le at the mid-points vs the bilinear value <= {le_dev:.2e}")
    assert np.all(pdf > 0) and np.all(r["pick_pdf"] == 1.0) and np.all(r["visible"] == -1) and np.all(r["n1"] == 0.0)
    assert near.mean() <= 1e-3 and polar.mean() <= 1e-3
    assert dev <= 1e-4
    assert polar_ratio <= 1.0
    assert norm <= 1e-6 and far <= 1e-5
    assert abs(total - 1.0) <= 1e-5
    assert calm.sum() >= 100 and le_dev <= 1e-5


# ------------------------------------------------------------------------------------------------ 4. unbiased against the model
def _judge(c, name, k, e, model, keep, who):
    """e (P, N) per-query estimator of E, model (P,) E: the statistic over the block means on the judged points, scaled by rho / pi as `statistic` and the cases'
    `extra` expect; dark points of the model without an allowance must be 0.0 in every query."""
    bm = block_means(e) * c.rho / np.pi
    m = model * c.rho / np.pi
    extra = None if c.extra is None else c.extra[keep]
    st = rm.statistic(bm[keep], m[keep], extra)
    dark = (model == 0) & (True if c.extra is None else c.extra == 0)
    print("\n" + rm.line("light_eval", who, st) + f"; judged {int(keep.sum())} of {keep.size} points, {int(dark.sum())} dark")
    assert np.all(e[dark] == 0.0), f"{who}: {int((e[dark] != 0).sum())} non-zero queries at points the light does not reach"
    rm.require(st, who)


@pytest.mark.parametrize("name", [n for n in lc.AREA_CASES if n != "two_triangles_occluder"])
def test_unbiased_against_the_model(gpu_host, name):
    """Per light and point: the block means of Li max(0, n . wi) / pdf against rm.irradiance(light, x, n, occluders=None). On the receivers "instance" and "disk"
    the visibility flag multiplies the estimator (nothing occludes: the model is the same), so that other trace kernels answer the segments."""
    c, h = scene(gpu_host, name)
    use_v = name in ("quad_on_instance", "quad_on_disk")
    if use_v:
        assert not h.lds_resident()
    for k in range(len(lc.flat_lights(c))):
        a, _ = run(gpu_host, name, k, visibility=use_v)
        if use_v:
            traced = (a[..., 8] > 0) & (a[..., 2:5].max(axis=-1) > 0)
            assert np.all(a[..., 15][traced] >= 0.0) and np.all(a[..., 15][~traced] == -1.0)
        _judge(c, name, k, estimator(c, a, use_v), lc.model_e(name, k)[:, 1], lc.judged(name, k), f"{name} light {k}" + (" x V" if use_v else ""))
        _RUNS.pop((name, k, use_v))


def test_unbiased_with_visibility_against_the_occluded_model(gpu_host):
    """two_triangles_occluder (the `shadow` case), per light and point: the unoccluded estimator against the unoccluded model of the light, then Li max(0, n . wi) V /
    pdf against the OCCLUDED model of that light (tests/golden/light_eval_occluded.npz, from rm.irradiance(light, x, n, occluders)); the light's umbra must be 0.0 in
    every query. Last, the sum over the two lights against radiometry_cases' golden values of the case."""
    name = "two_triangles_occluder"
    c, h = scene(gpu_host, name)
    total = 0.0
    for k in range(len(lc.flat_lights(c))):
        a, _ = run(gpu_host, name, k, visibility=True)
        traced = (a[..., 8] > 0) & (a[..., 2:5].max(axis=-1) > 0)
        assert np.all(a[..., 15][traced] >= 0.0) and np.all(a[..., 15][~traced] == -1.0)
        print(f"\n{name} light {k}: traced {traced.mean():.4f}, unoccluded {(a[..., 15] == 1.0).mean():.4f}")
        _judge(c, name, k, estimator(c, a, False), lc.model_e(name, k)[:, 1], lc.judged(name, k), f"{name} light {k}, V ignored")
        m_k = lc.occluded_e(name, k)[:, 1]
        assert (m_k == 0).sum() >= 4 and (m_k > 0).sum() >= 30
        _judge(c, name, k, estimator(c, a, True), m_k, lc.judged_occluded_light(name, k), f"{name} light {k} x V, occluded model")
        total = total + estimator(c, a, True)
    m = lc.occluded_model(name)[:, 1] * np.pi / c.rho
    _judge(c, name, -1, total, m, lc.judged_occluded(name), f"{name} x V, both lights")


# ------------------------------------------------------------------------------------------------ 5. the pick
def _voxels(c, nv, p):
    """voxel_of (lightdistrib.rs:187-198) in float32 for floor points: the world's x and z bounds are the floor's +-6, y = 0 is the lower bound."""
    lo, hi = np.float32(-rc.FLOOR), np.float32(rc.FLOOR)
    p = np.float32(p)
    ix = np.clip((((p[:, 0] - lo) / (hi - lo)) * np.float32(nv[0])).astype(np.int64), 0, nv[0] - 1)
    iz = np.clip((((p[:, 2] - lo) / (hi - lo)) * np.float32(nv[2])).astype(np.int64), 0, nv[2] - 1)
    assert np.all(p[:, 1] == 0)
    return (iz * nv[1] + 0) * nv[0] + ix


def test_pick_spatial(gpu_host):
    """The index equals find_interval over the rows of HostScene.light_distribution() at the point's voxel, exactly; the pdf equals func[i] / (func_int n_lights)
    within 4 float32 ulp (one v_rcp quotient and one product); the rest of the record is the record of that light asked for by index. Before the tables hold every
    voxel, a point in free space whose voxel holds no surface gives light -1, pick pdf 0 and zeros."""
    c = rc.case("three_lights_spatial")
    h = gpu_host.HostScene(c.desc)
    h.upload(0)
    free = h.light_eval([(4.0, 1.4, 4.0)], None, [(0.3, 0.5, 0.5)])
    print(f"\nLIGHT_EVAL pick, a point in free space before light_distribution(): {free['raw'][0].tolist()}")
    assert free["light"][0] == -1 and free["pick_pdf"][0] == 0.0 and np.all(free["raw"][0, 2:] == 0.0)
    ld = h.light_distribution()
    nv, nl = [int(v) for v in ld["n_voxels"]], h.table("lights").shape[0]
    assert nl == 4 and min(nv) > 1
    P, K = c.x.shape[0], 256
    rng = np.random.default_rng(3)
    u = rng.random((P, K, 3)).astype(np.float32)
    vox = _voxels(c, nv, c.x)
    u[:, 0:nl + 1, 0] = ld["cdf"][vox][:, :nl + 1]                      # the row's own cdf entries as u_pick: the edges of the intervals
    u[:, nl + 1, 0] = np.float32(1.0) - np.float32(F32_ULP)
    u = np.minimum(u, np.float32(1.0) - np.float32(F32_ULP))
    rep = lambda a: np.repeat(np.float32(a), K, axis=0)
    r = h.light_eval(rep(c.x), rep(c.n), u.reshape(-1, 3))
    cdf, func, fint = ld["cdf"][vox], ld["func"][vox], ld["func_int"][vox]
    want = np.array([np.clip(np.searchsorted(cdf[p], u[p, :, 0], side="right") - 1, 0, nl - 1) for p in range(P)])
    want_pdf = np.float64(np.take_along_axis(func, want, axis=1)) / (np.float64(fint)[:, None] * nl)
    got, got_pdf = r["light"].reshape(P, K), np.float64(r["pick_pdf"]).reshape(P, K)
    ulp = np.abs(got_pdf - want_pdf) / (np.float64(np.spacing(np.float32(want_pdf))))
    print(f"LIGHT_EVAL pick spatial: {nv} voxels, {P} points x {K} u_pick, picks per light {np.bincount(got.ravel(), minlength=nl).tolist()}, wrong index {int((got != want).sum())}, "
          f"pdf within {ulp.max():.2f} ulp")
    assert np.array_equal(got, want) and len(np.unique(got)) == nl
    assert ulp.max() <= 4.0
    for k in range(nl):
        sel = r["light"] == k
        rk = h.light_eval(rep(c.x)[sel], rep(c.n)[sel], u.reshape(-1, 3)[sel], light=k)
        assert np.array_equal(r["raw"][sel][:, 2:], rk["raw"][:, 2:]) and np.all(rk["pick_pdf"] == 1.0)
    free = h.light_eval([(4.0, 1.4, 4.0)], None, [(0.3, 0.5, 0.5)])      # every voxel has a row now
    assert free["light"][0] >= 0 and free["pick_pdf"][0] > 0.0


def test_pick_uniform(gpu_host):
    """strategy "uniform": the index is min(n - 1, int(u n)) exactly and the pdf 1 / n exactly. n = 4: the cdf entries k / 4 and the product u x 4 are exact in
    float32, and so is the quotient by 4; the multiples of 1 / 4 themselves are among the u_pick values."""
    c = rc.case("three_lights_uniform")
    h = gpu_host.HostScene(c.desc)
    h.upload(0)
    nl = h.table("lights").shape[0]
    assert nl == 4
    P, K = c.x.shape[0], 256
    u = np.random.default_rng(4).random((P * K, 3)).astype(np.float32)
    u[0:4, 0] = np.float32([0.0, 0.25, 0.5, 0.75])
    u[4:7, 0] = np.nextafter(np.float32([0.25, 0.5, 0.75]), np.float32(0.0))
    u[7, 0] = np.float32(1.0) - np.float32(F32_ULP)
    rep = lambda a: np.repeat(np.float32(a), K, axis=0)
    r = h.light_eval(rep(c.x), rep(c.n), u, strategy="uniform")
    want = np.minimum(nl - 1, (np.float64(u[:, 0]) * nl).astype(np.int64))
    print(f"\nLIGHT_EVAL pick uniform: {nl} lights, {P * K} queries, picks {np.bincount(r['light'], minlength=nl).tolist()}, wrong index {int((r['light'] != want).sum())}, "
          f"the eight edge values pick {r['light'][:8].tolist()}, distinct pdfs {np.unique(r['pick_pdf']).tolist()}")
    assert np.array_equal(r["light"], want) and r["light"][:8].tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    assert np.all(r["pick_pdf"] == np.float32(0.25))
    one = gpu_host.HostScene(rc.case("sphere_outside").desc)                # one light: uniform whatever the strategy (path.rs:89)
    one.upload(0)
    r1 = one.light_eval(rc.case("sphere_outside").x, rc.case("sphere_outside").n, np.random.default_rng(5).random((rc.case("sphere_outside").x.shape[0], 3)), strategy="spatial")
    assert np.all(r1["light"] == 0) and np.all(r1["pick_pdf"] == 1.0)


# ------------------------------------------------------------------------------------------------ 6. shapes
def test_batch_sizes_and_the_general_instantiation(gpu_host):
    """n = 1, 63, 64, 65, 257 return the bytes the same queries return inside one larger batch (there are no chunks: device buffers are sized by n), picked lights,
    visibility and a wi query included; with and without RT_LIGHT_EVAL_GENERAL the bytes are the same on a scene whose emitters are all plain triangles."""
    c, h = scene(gpu_host, "two_triangles_occluder")
    rng = np.random.default_rng(6)
    big = 1000
    idx = rng.integers(0, c.x.shape[0], big)
    p, n, u = np.float32(c.x[idx]), np.float32(c.n[idx]), rng.random((big, 3)).astype(np.float32)
    wi = rng.normal(size=(big, 3))
    wi = np.float32(wi / np.linalg.norm(wi, axis=1, keepdims=True))
    wi[::2] = h.light_eval(p, n, u)["wi"][::2]
    full = h.light_eval(p, n, u, wi=wi, visibility=True)["raw"]
    gen = h.light_eval(p, n, u, wi=wi, visibility=True, general=True)["raw"]
    print(f"\nLIGHT_EVAL shapes: {big} queries, lights {np.bincount(full[:, 0].astype(int)).tolist()}, visible {np.unique(full[:, 15], return_counts=True)}, "
          f"pdf_li > 0 in {int((full[:, 16] > 0).sum())}; GENERAL bytes equal {np.array_equal(full.view(np.uint32), gen.view(np.uint32))}")
    assert len(np.unique(full[:, 0])) == 2 and {0.0, 1.0} <= set(np.unique(full[:, 15]).tolist()) and (full[:, 16] > 0).sum() > 100
    assert np.array_equal(full.view(np.uint32), gen.view(np.uint32))
    for k in (1, 63, 64, 65, 257):
        part = h.light_eval(p[:k], n[:k], u[:k], wi=wi[:k], visibility=True)["raw"]
        same = np.array_equal(part.view(np.uint32), full[:k].view(np.uint32))
        print(f"  n = {k}: bytes equal {same}")
        assert same


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_out_untouched(gpu_host):
    c, h = scene(gpu_host, "quad")
    L, hip = gpu_host.lib(), gpu_host.hip_lib()
    dev = C.c_void_p()
    assert L.rtxh_scene_device(h.h, C.byref(dev)) == 0
    bare = rc._scene()
    rc.add_floor(bare, bare.matte((0.5, 0.5, 0.5)))
    hb = gpu_host.HostScene(rc._finish(bare))
    hb.upload(0)
    dev_bare = C.c_void_p()
    assert L.rtxh_scene_device(hb.h, C.byref(dev_bare)) == 0
    n = 8
    ref, u, wi = np.zeros((n, 9), np.float32), np.full((n, 3), 0.5, np.float32), np.zeros((n, 3), np.float32)
    ref[:, 0], ref[:, 4] = 1.0, 1.0
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    cases = {
        "NULL scene": (None, 0, 0, n, ref, u, 0, True),
        "NULL ref": (dev, 0, 0, n, None, u, 0, True),
        "NULL u": (dev, 0, 0, n, ref, None, 0, True),
        "NULL out": (dev, 0, 0, n, ref, u, 0, False),
        "n == 0": (dev, 0, 0, 0, ref, u, 0, True),
        "n above RT_LIGHT_EVAL_MAX": (dev, 0, 0, gpu_host.RT_LIGHT_EVAL_MAX + 1, ref, u, 0, True),
        "light == n_lights": (dev, 2, 0, n, ref, u, 0, True),
        "light == -2": (dev, -2, 0, n, ref, u, 0, True),
        "a scene without lights": (dev_bare, -1, 0, n, ref, u, 0, True),
        "a scene without lights, light 0": (dev_bare, 0, 0, n, ref, u, 0, True),
        "strategy 2": (dev, -1, 2, n, ref, u, 0, True),
        "strategy -1 with a light index": (dev, 0, -1, n, ref, u, 0, True),
        "flag bit 4": (dev, 0, 0, n, ref, u, 4, True),
        "flag bit 31": (dev, 0, 0, n, ref, u, 1 << 31, True),
    }
    for what, (scn, light, strat, cnt, r_, u_, flags, with_out) in cases.items():
        out = np.full((n, 20), -7.5, np.float32)
        hip.rt_light_eval(dev, C.c_int32(0), C.c_int32(0), C.c_uint64(n), fp(ref), fp(u), fp(wi), C.c_uint32(0), fp(np.zeros((n, 20), np.float32)))   # a good call: the message is this call's
        rc_ = hip.rt_light_eval(scn, C.c_int32(light), C.c_int32(strat), C.c_uint64(cnt), fp(r_), fp(u_), fp(wi), C.c_uint32(flags), fp(out) if with_out else None)
        msg = hip.rt_last_error().decode(errors="replace")
        print(f"\nLIGHT_EVAL refusal, {what}: {rc_} \"{msg}\"")
        assert rc_ == -1 and "rt_light_eval" in msg and len(msg) > 20
        assert np.all(out == -7.5)
    good = h.light_eval(ref[:, 0:3], ref[:, 3:6], u, light=1)
    assert np.all(good["light"] == 1)


# ------------------------------------------------------------------------------------------------ 8. direct_irradiance
@pytest.mark.parametrize("name", ["quad_overhead", "env_map"])
def test_direct_irradiance(gpu_host, name):
    """E of all lights with visibility at every point of the case: within 5 of its own standard errors plus 1e-4 of the model's E, the standard errors inside the
    caps (se_p <= 0.03 E_p, sqrt(sum se^2) <= 0.002 sum E). quad_overhead: 256 blocks of 8 x 8, the design the CPU test holds to the caps. env_map: the map's sun
    takes 97.6 % of the light's samples, so a face that does not see it (or sees it edge-on) gets its irradiance from the 2.4 % that land in the sky - 256 blocks
    measured se_p = 0.065 E_p there; the case gets more blocks, not looser caps: 2048, which puts that point at 0.065 / sqrt(8) = 0.023."""
    c, h = scene(gpu_host, name)
    e, se = h.direct_irradiance(c.x, c.n, blocks=lc.BLOCKS if name == "quad_overhead" else 2048, grid=lc.GRID, seed=9)
    m = rc.model_radiance(c) * np.pi / c.rho
    lit = m[:, 1] > 0
    dev = np.abs(e - m)
    allow = rm.K_SIGMA * se + rm.REL_FLOOR * m
    pooled, cap = float(np.sqrt((se[lit, 1] ** 2).sum()) / m[lit, 1].sum()), float((se[lit, 1] / m[lit, 1]).max())
    worst = np.unravel_index(np.argmax(dev - allow), dev.shape)
    print(f"\nLIGHT_EVAL direct_irradiance {name}: {c.x.shape[0]} points ({int(lit.sum())} lit), sum E / sum model - 1 = {e[lit].sum() / m[lit].sum() - 1.0:+.2e}, pooled se / sum E = {pooled:.2e}, "
          f"largest se_p / E_p = {cap:.2e}, worst point {worst}: E {e[worst]:.6f}, model {m[worst]:.6f}, se {se[worst]:.2e}")
    assert e.shape == m.shape == se.shape
    assert np.all(e[~lit] == 0.0) and np.all(se[~lit] == 0.0)
    assert np.all(dev <= allow)
    assert pooled <= rm.CAP_POOLED and cap <= rm.CAP_POINT


def test_irradiance_probe_script(gpu_host, tmp_path):
    """scripts/irradiance_probe.py scene.pbrt points.npy out.npy on quad_overhead written out as a pbrt file: (P, 6) = E rgb and its standard error, each E within
    5 of its standard errors plus 1e-4 of the model's."""
    import os
    import subprocess
    import sys
    from rustracer_amd import pbrt_export
    c = rc.case("quad_overhead")
    pbrt_export.write_pbrt(c.desc, str(tmp_path / "scene.pbrt"))
    np.save(tmp_path / "points.npy", np.concatenate([c.x, c.n], axis=1))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "irradiance_probe.py"), str(tmp_path / "scene.pbrt"), str(tmp_path / "points.npy"), str(tmp_path / "out.npy"),
                        "--blocks", "64", "--seed", "3"], capture_output=True, text=True, timeout=300)
    print("\n" + r.stdout[-500:] + r.stderr[-1500:])
    assert r.returncode == 0
    out = np.load(tmp_path / "out.npy")
    m = rc.model_radiance(c) * np.pi / c.rho
    assert out.shape == (c.x.shape[0], 6) and out.dtype == np.float64
    e, se = out[:, :3], out[:, 3:]
    print(f"LIGHT_EVAL irradiance_probe quad_overhead: sum E / sum model - 1 = {e.sum() / m.sum() - 1.0:+.2e}, largest se / E {(se / m).max():.2e}, worst |E - model| / (5 se + 1e-4 model) = "
          f"{(np.abs(e - m) / (rm.K_SIGMA * se + rm.REL_FLOOR * m)).max():.2f}")
    assert np.all(se > 0) and np.all(np.abs(e - m) <= rm.K_SIGMA * se + rm.REL_FLOOR * m)
