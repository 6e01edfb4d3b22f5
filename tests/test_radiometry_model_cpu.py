"""tests/radiometry_model.py on the CPU: (a) the float64 model against closed forms it was not written from, (b) the oracle's per-sample radiance
(OracleScene.li_keyed, PathIntegrator::li in KEYED mode) against the model, with the statistic and the noise caps that tests/test_gpu_radiometry.py applies to
the HIP path, (c) the layout of every case: each ray meets the receiver at its own length, the model's two resolutions agree to 1e-4, the shadow case has EMPTY
shadow-set pairs. No GPU.

(b) looks straight down at a receiver point through a perspective camera of 0.002 degrees, one pixel, N samples: the pixel's footprint is 5e-5 wide; the model
is evaluated at its four corners too and their spread is added to the allowance."""
import numpy as np
import pytest

import radiometry_cases as rc
import radiometry_model as rm

L = 8.0


def _t(x=0.0, y=0.0, z=0.0):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


# ------------------------------------------------------------------------------------------------ (a) closed forms
def _close(lights, x, n, expect, tol=1e-9, **kw):
    e, d = rm.irradiance(lights, x, n, tol=tol, **kw)
    print(f"\nMODEL {e[1]:.12g} expected {expect:.12g}: relative {e[1] / expect - 1:+.2e}, two resolutions differ by {d / expect:.2e}")
    assert abs(e[1] / expect - 1.0) <= 1e-6 and d <= 1e-6 * expect
    assert np.allclose(e, expect, rtol=1e-6)       # a grey emitter: the three channels agree


def test_disk_form_factor():
    """The disk-to-element form factor tests/test_gpu_sphere.py quotes: a parallel disk of radius R at height h, a receiver at distance a from the axis."""
    R, h = 0.7, 3.0
    for a in (0.0, 1.3, 4.0):
        _close(rm.Disk(_t(z=h), R, L, two_sided=True), (a, 0, 0), (0, 0, 1), np.pi * L / 2 * (1 - (h * h + a * a - R * R) / np.sqrt((h * h + a * a + R * R) ** 2 - 4 * R * R * a * a)))


def test_sphere_above_the_horizon():
    """A sphere of radius r at distance D, all of it above the receiver's horizon: E = pi Le (r / D)^2 cos(theta), at 2.5 and at 1.01 radii."""
    for D, r, n in ((2.5, 0.8, (0.3, 0.0, 1.0)), (1.01, 1.0, (0.0, 0.0, 1.0)), (3.0, 0.5, (0.0, -0.4, 1.0))):
        _close(rm.Sphere(_t(z=D), r, L), (0, 0, 0), n, np.pi * L * (r / D) ** 2 / np.linalg.norm(n))


def test_inside_a_closed_emitting_sphere():
    for x, n in (((0.5, 0.2, 0.0), (0.3, 0.2, 1.0)), ((0.0, 0.0, 0.3), (0.0, 1.0, 0.0)), ((-1.2, 0.9, 0.4), (1.0, 0.0, 0.0))):
        _close(rm.Sphere(_t(z=0.3), 2.0, L, two_sided=True), x, n, np.pi * L, tol=1e-8)


def test_rectangle_from_a_point_on_its_axis():
    """A 2a x 2b rectangle parallel to the receiver at distance c, the receiver under its centre: four times the corner form factor
    1 / (2 pi) (A / sqrt(1 + A^2) atan(B / sqrt(1 + A^2)) + B / sqrt(1 + B^2) atan(A / sqrt(1 + B^2))), A = a / c, B = b / c."""
    a, b, c = 0.6, 0.9, 1.7
    A, B = a / c, b / c
    f = (A / np.sqrt(1 + A * A) * np.arctan(B / np.sqrt(1 + A * A)) + B / np.sqrt(1 + B * B) * np.arctan(A / np.sqrt(1 + B * B))) / (2 * np.pi)
    q = rm.quad((-a, -b, c), (-a, b, c), (a, b, c), (a, -b, c), L)
    _close(q, (0, 0, 0), (0, 0, 1), np.pi * L * 4 * f)


def test_constant_environment():
    for n in ((0.0, 0.0, 1.0), (0.3, 0.2, 1.0), (1.0, -1.0, -0.2)):
        _close(rm.Infinite(np.full((1, 1, 3), L, np.float32), rc._roty(25.0)), (0, 0, 0), n, np.pi * L, tol=1e-8)
    _close(rm.Infinite(np.full((8, 16, 3), L, np.float32)), (1, 2, 3), (0.3, 0.2, 1.0), np.pi * L, tol=1e-8)


def test_one_sided_emitters_from_behind_are_black():
    q = rm.quad((-1, -1, 2), (-1, 1, 2), (1, 1, 2), (1, -1, 2), L)
    front = rm.irradiance(q, (0, 0, 0), (0, 0, 1))[0][1]
    assert front > 0
    assert rm.irradiance(q, (0, 0, 4), (0, 0, -1))[0][1] == 0.0
    assert rm.irradiance(rm.quad((-1, -1, 2), (-1, 1, 2), (1, 1, 2), (1, -1, 2), L, reverse_orientation=True), (0, 0, 0), (0, 0, 1))[0][1] == 0.0
    both = rm.irradiance(rm.quad((-1, -1, 2), (-1, 1, 2), (1, 1, 2), (1, -1, 2), L, two_sided=True), (0, 0, 4), (0, 0, -1))[0][1]
    assert abs(both / front - 1.0) < 1e-9
    assert rm.irradiance(rm.Sphere(_t(z=2), 1.0, L, reverse_orientation=True), (0.3, 0, 0), (0, 0, 1))[0][1] == 0.0
    assert rm.irradiance(rm.Cylinder(_t(), 1.0, L), (0.2, 0.1, 0), (1, 0, 0))[0][1] == 0.0        # a cylinder emits outward: nothing inside it
    assert rm.irradiance(rm.Cylinder(_t(), 1.0, L), (3.0, 0, 0), (-1, 0, 0))[0][1] > 0


def test_point_and_distant_lights():
    e = rm.irradiance(rm.Point((0, 0, 2), (L, L, L)), (0, 0, 0), (0, 0, 1))[0][1]
    assert abs(e - L / (4 * np.pi * 4)) < 1e-15        # light/point.rs:50
    assert rm.irradiance(rm.Point((0, 0, -2), (L, L, L)), (0, 0, 0), (0, 0, 1))[0][1] == 0.0
    assert abs(rm.irradiance(rm.Distant((0, 3, 4), L), (5, 5, 5), (0, 0, 1))[0][1] - 0.8 * L) < 1e-15
    occ = [[(-1, -1, 1), (1, -1, 1), (0, 1, 1)]]
    assert rm.irradiance([rm.Point((0, 0, 2), L), rm.Distant((0, 0, 1), L)], (0, 0, 0), (0, 0, 1), occluders=occ)[0][1] == 0.0


def test_what_the_reference_does_not_render_physically_raises():
    scale = np.diag([2.0, 2.0, 2.0, 1.0])
    for make in (lambda: rm.Sphere(scale, 1.0, L), lambda: rm.Sphere(_t(), 1.0, L, z_max=0.5), lambda: rm.Sphere(_t(), 1.0, L, phi_max=180.0),
                 lambda: rm.Disk(_t(), 1.0, L, two_sided=True, inner_radius=0.3), lambda: rm.Disk(_t(), 1.0, L, two_sided=True, phi_max=270.0),
                 lambda: rm.Disk(scale, 1.0, L, two_sided=True), lambda: rm.Disk(_t(), 1.0, L),
                 lambda: rm.Cylinder(np.diag([1.0, 2.0, 1.0, 1.0]), 1.0, L),
                 lambda: rm.irradiance(rm.Sphere(_t(), 2.0, L, reverse_orientation=True), (0.1, 0, 0), (0, 0, 1))):
        with pytest.raises(rm.NotPhysical):
            make()


def test_an_occluder_needs_and_gets_the_finer_grid():
    """Half of a rectangle hidden behind an edge through its axis: half the irradiance, although the integrand jumps."""
    a, c = 0.7, 1.5
    q = rm.quad((-a, -a, c), (-a, a, c), (a, a, c), (a, -a, c), L)
    full = rm.irradiance(q, (0, 0, 0), (0, 0, 1))[0][1]
    occ = [[(0, -5, 0.5), (5, -5, 0.5), (5, 5, 0.5)], [(0, -5, 0.5), (5, 5, 0.5), (0, 5, 0.5)]]
    e, d = rm.irradiance(q, (0, 0, 0), (0, 0, 1), occluders=occ, tol=2e-4)
    print(f"\nMODEL half-hidden rectangle: {e[1] / full:.7f} of the whole, two resolutions differ by {d / e[1]:.2e}")
    assert abs(e[1] / full - 0.5) < 1e-4 and d <= 1e-4 * e[1]


def test_the_statistic_bites():
    rng = np.random.default_rng(0)
    M = np.array([1.0, 2.0, 0.0, 0.5])
    s = M[:, None] * (1.0 + 0.3 * rng.standard_normal((4, 16384)))
    good = rm.statistic(s, M)
    assert good["point_ok"].all() and good["pooled_ok"] and good["caps_ok"]
    rm.require(good)
    assert not rm.statistic(s * 1.01, M)["pooled_ok"]                       # a pooled bias of 1 %
    assert not rm.statistic(s, M * [1, 1.03, 1, 1])["point_ok"][1]         # one point off by 3 %
    t = s.copy(); t[2, 7] = 1e-6
    assert not rm.statistic(t, M)["point_ok"][2]                            # one sample of a black point not 0
    assert rm.statistic(t, M, np.array([0, 0, 1e-10, 0]))["point_ok"][2]   # ... inside the point's allowance (the mean is 6e-11)
    assert not rm.statistic(t, M, np.array([0, 0, 1e-11, 0]))["point_ok"][2]   # ... and outside it: 5 se of such samples is no allowance
    assert not rm.statistic(M[:, None] * (1.0 + 5.0 * rng.standard_normal((4, 16384))), M)["caps_ok"]   # too noisy to judge
    with pytest.raises(AssertionError):
        rm.require(rm.statistic(s * 1.01, M), "biased")


# ------------------------------------------------------------------------------------------------ (c) the cases' layout
@pytest.mark.parametrize("name", list(rc.CASES))
def test_case_layout(orc, name):
    """Every ray of the case meets the receiver first, at its own length; the model's two resolutions agree to 1e-4 of the value at every point; the case has
    lit points, and - where a receiver can be hidden from every light - points whose irradiance is 0."""
    c = rc.case(name)
    tr = orc.OracleScene(c.desc).trace(c.rays(1)[0, :, 0, :])
    assert np.all(np.abs(tr["t"] - c.h) <= 1e-4 * c.h), np.flatnonzero(np.abs(tr["t"] - c.h) > 1e-4 * c.h)
    m, rel = rc.compute_model_radiance(c)
    held = rc.model_radiance(c)
    assert np.allclose(held, m, rtol=1e-7, atol=0.0) and np.array_equal(held == 0, m == 0), "tests/golden/radiometry_model.npz is not this model's: python tests/radiometry_cases.py"
    lit = m[:, 1] > 0
    print(f"\nLAYOUT {name}: {c.x.shape[0]} points, {int(lit.sum())} lit, radiance {m[lit, 1].min():.3e} .. {m[lit, 1].max():.3e}, two resolutions differ by at most {rel[lit].max():.2e}")
    assert rel[lit].max() <= 1e-4 and np.all(rel[~lit] == 0.0)
    assert 32 <= c.x.shape[0] <= 64 and lit.sum() >= 12
    if name not in ("quad_overhead", "sphere_outside", "sphere_inside", "disk_tilted", "disk_overhead", "env_const", "env_map", "quad_two_sided", "three_lights_spatial", "three_lights_uniform"):
        assert (~lit).sum() >= 3
    for o, d, _ in c.probes:      # the max_depth = 0 rays: the emitter is the first thing each meets (its primitive comes after the receiver's)
        hit = orc.OracleScene(c.desc).trace(np.float32([[*o, np.inf, *d, 0.0]]))
        assert abs(float(hit["t"][0]) - 0.35) < 0.02, (o, d, hit["t"])


def test_the_shadow_case_has_empty_pairs(host):
    c = rc.case("two_triangles_occluder")
    ss = host.HostScene(c.desc).shadow_sets()
    m = rc.model_radiance(c)
    free = np.array([rm.irradiance(c.lights, x, n)[0][1] for x, n in zip(c.x, c.n)]) * c.rho / np.pi
    part = (m[:, 1] > 0) & (m[:, 1] < free * (1 - 1e-3))
    print(f"\nSHADOW SETS: {ss['pairs']} pairs, {ss['empty']} EMPTY; points: {int((m[:, 1] == 0).sum())} in the umbra, {int(part.sum())} partly shadowed, {int((m[:, 1] >= free * (1 - 1e-3)).sum())} lit")
    assert ss["empty"] > 0 and ss["empty"] < ss["pairs"]
    assert (m[:, 1] == 0).sum() >= 3 and part.sum() >= 6 and (m[:, 1] >= free * (1 - 1e-3)).sum() >= 6


# ------------------------------------------------------------------------------------------------ (b) the oracle against the model
ORACLE_LIT, ORACLE_DARK = 24, 4      # points per case (the cylinder, the overhead emitters and the uniform pick of three lights: all; the occluder, whose outline is slow to integrate: 14): enough for the pooled cap at N = 16384 (MEASUREMENTS.md, "Direct lighting against the float64 model")
FOV = 0.002


def oracle_samples(orc, c, pick):
    """(samples (len(pick), N, 3), footprint spread of the model's radiance (len(pick),)) of the case's points `pick`, each seen from 1.5 straight above it - or,
    where something is in the way there (the sphere over the points under it, the occluder over its shadow), along the case's own ray."""
    o = orc.OracleScene(c.desc)
    out, spread = np.zeros((len(pick), rc.N_SAMPLES, 3)), np.zeros(len(pick))
    tan_half = np.tan(np.radians(FOV) / 2)
    above = o.trace(np.float32([[*(c.x[p] + 1.5 * c.n[p]), np.inf, *(-c.n[p]), 0.0] for p in pick]))["t"]
    for k, p in enumerate(pick):
        x, n = c.x[p], c.n[p]
        d_in, h = (n, 1.5) if abs(above[k] - 1.5) < 1e-4 else (c.d_in[p], c.h[p])
        up, right = rc._tangent_frame(d_in)
        eye = x + h * d_in
        c.desc.camera.pos, c.desc.camera.look, c.desc.camera.up, c.desc.camera.fov = tuple(eye), tuple(x), tuple(up), FOV
        out[k] = o.li_keyed(0, 0, 0, n=rc.N_SAMPLES)
        centre = rm.irradiance(c.lights, x, n, c.occluders, tol=c.tol)[0][1]
        for a in (-1, 1):
            for b in (-1, 1):      # the pixel's corner rays, met with the receiver's plane
                w = -d_in + tan_half * (a * right + b * up)
                corner = eye + w * ((x - eye) @ n) / (w @ n)
                spread[k] = max(spread[k], c.rho / np.pi * abs(rm.irradiance(c.lights, corner, n, c.occluders, tol=c.tol)[0][1] - centre))
    return out, spread


def test_li_keyed_ranges_are_li_keyed(orc):
    c = rc.case("quad")
    c.desc.camera.pos, c.desc.camera.look, c.desc.camera.up, c.desc.camera.fov = (1.0, 1.5, 0.45), (1.0, 0.0, 0.45), (1.0, 0.0, 0.0), FOV
    o = orc.OracleScene(c.desc)
    block = o.li_keyed(0, 0, 3, n=5)
    assert np.array_equal(block, np.stack([o.li_keyed(0, 0, 3 + k) for k in range(5)])) and block.max() > 0


@pytest.mark.parametrize("name", list(rc.CASES))
def test_oracle_against_the_model(orc, name):
    """The oracle takes a subset of the case's points - up to 24 lit and 4 dark ones, spread over the case's list; all of the cylinder's, the overhead emitters' and the uniform
    pick's, 14 lit of the occluder's - because every point costs five evaluations of the model (the footprint's corners) where the device's costs none that is
    not recorded. The statistic and both caps are asserted on that subset; the device (tests/test_gpu_radiometry.py) leaves no point out."""
    c = rc.case(name)
    m = rc.model_radiance(c)
    lit, dark = np.flatnonzero(m[:, 1] > 0), np.flatnonzero(m[:, 1] == 0)
    few = lambda a, k: a[np.unique(np.linspace(0, a.size - 1, min(k, a.size)).round().astype(int))] if a.size else a
    pick = np.sort(np.concatenate([few(lit, 14 if c.occluders is not None else 64 if name in ("cylinder", "three_lights_uniform", "quad_overhead", "disk_overhead") else ORACLE_LIT), few(dark, ORACLE_DARK)]))
    s, spread = oracle_samples(orc, c, pick)
    extra = spread + (0.0 if c.extra is None else c.extra[pick])
    st = rm.statistic(s[..., 1], m[pick, 1], extra)
    print("\n" + rm.line("oracle", name, st) + f"; footprint spread at most {spread.max():.2e}")
    dark = (m[pick, 1] == 0) & (extra == 0)
    assert np.all(s[dark] == 0.0)
    rm.require(st, name)
