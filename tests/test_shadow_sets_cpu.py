"""Shadow sets (rt_shadow_sets) against the oracle's intersect_p, without a device: segments built as k_shade builds them
(surface point, offset_ray_origin at both ends, t_max = 1 - ShadowEpsilon) from every voxel / light pair marked EMPTY are unoccluded - on S1 and on random
soups and rooms with a two-triangle quad light in varied orientations, some scenes translated away from the origin. offset_ray_origin is the reference's
float32 arithmetic restated (test_gpu_parity checks the device's rt_offset_ray_origin bit for bit against the same restatement; test_gpu_shadow_sets builds
the segments with rt_offset_ray_origin itself)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import orc  # noqa: E402
from rustracer_amd import host  # noqa: E402
from rustracer_amd.scene_desc import SceneDesc  # noqa: E402
from rustracer_amd.scenes import cornell_box  # noqa: E402

F = np.float32
GAMMA7 = F(7 * np.finfo(np.float32).eps / 2 / (1 - 7 * np.finfo(np.float32).eps / 2))


def offset_ray_origin(p, p_error, n, w):
    """offset_ray_origin (rc/geometry/mod.rs:203-220) in float32, in the reference's order of operations: offset along n by dot(|n|, p_error), towards w,
    then each moved coordinate one ulp further (next_float_up / next_float_down)."""
    an = np.abs(n)
    d = ((an[:, 0] * p_error[:, 0]).astype(F) + (an[:, 1] * p_error[:, 1]).astype(F)).astype(F) + (an[:, 2] * p_error[:, 2]).astype(F)
    off = (d.astype(F)[:, None] * n).astype(F)
    dwn = ((w[:, 0] * n[:, 0]).astype(F) + (w[:, 1] * n[:, 1]).astype(F)).astype(F) + (w[:, 2] * n[:, 2]).astype(F)
    off = np.where((dwn < 0)[:, None], -off, off).astype(F)
    po = (p + off).astype(F)
    po = np.where(off > 0, np.nextafter(po, F(np.inf)), np.where(off < 0, np.nextafter(po, F(-np.inf)), po))
    return po.astype(F)


def surface_points(P, idx, tris, rng):
    """Uniform points on the given triangles with the error bound of Triangle::intersect's point (gamma(7) |b_i p_i|) and the geometric normal."""
    p0, p1, p2 = (P[idx[tris, k]].astype(F) for k in range(3))
    u, v = rng.random(len(tris)), rng.random(len(tris))
    s = np.sqrt(u)
    b0, b1 = (1 - s).astype(F), (s * (1 - v)).astype(F)
    b2 = (F(1) - b0 - b1).astype(F)
    p = (b0[:, None] * p0 + b1[:, None] * p1 + b2[:, None] * p2).astype(F)
    err = (GAMMA7 * (np.abs(b0[:, None] * p0) + np.abs(b1[:, None] * p1) + np.abs(b2[:, None] * p2))).astype(F)
    n = np.cross(p2 - p0, p1 - p0).astype(F)
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    return p, err, n


def voxel_of(p, wb_min, wb_max, nvox):
    o = ((p - wb_min) / (wb_max - wb_min)).astype(F)
    ix = [np.clip((o[:, k] * F(nvox[k])).astype(np.int64), 0, nvox[k] - 1) for k in range(3)]
    return ix[0], ix[1], ix[2]


def segments(desc, n, seed, offset=offset_ray_origin):
    """n shadow segments of the scene's sampled lights from area-weighted surface points (emitters included): (rays (n, 8), light index, surface point)."""
    rng = np.random.default_rng(seed)
    P, idx = desc.arrays()[:2]
    lights = np.asarray([lt.tri for lt in desc.lights])
    area = 0.5 * np.linalg.norm(np.cross(P[idx[:, 1]] - P[idx[:, 0]], P[idx[:, 2]] - P[idx[:, 0]]).astype(np.float64), axis=1)
    tris = rng.choice(len(idx), size=n, p=area / area.sum())
    p, perr, pn = surface_points(P, idx, tris, rng)
    li = rng.integers(0, len(lights), size=n)
    q, qerr, qn = surface_points(P, idx, lights[li], rng)
    o = offset(p, perr, pn, (q - p).astype(F))
    t = offset(q, qerr, qn, (o - q).astype(F))
    rays = np.zeros((n, 8), F)
    rays[:, :3], rays[:, 3], rays[:, 4:7] = o, F(1.0) - F(1e-4), (t - o).astype(F)
    return rays, li, p


def classify(desc, rays, li, p):
    """The shadow-set kind (1 = EMPTY) of each segment's voxel / light pair, and the sets."""
    h = host.HostScene(desc)
    ss = h.shadow_sets()
    b = h.bvh()["bounds"][0]
    vx, vy, vz = voxel_of(p, b[:3].astype(F), b[3:].astype(F), ss["nvox"])
    kind = ss["kind"][vz, vy, vx, li]
    assert set(np.unique(kind)) <= {0, 1}
    return kind, ss


def check_scene(desc, n=120_000, seed=1, offset=offset_ray_origin):
    rays, li, p = segments(desc, n, seed, offset)
    kind, ss = classify(desc, rays, li, p)
    occ = orc.OracleScene(desc).trace(rays, any_hit=True)["occluded"]
    empty = kind == 1
    assert not np.any(occ & empty), f"{int(np.sum(occ & empty))} occluded segments in EMPTY pairs"
    return ss, float(empty.mean()), float(occ.mean())


# ---- random scenes: each with ONE quad light (two triangles, two sampled lights)
def _frame(n):
    n = n / np.linalg.norm(n)
    a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    return a, np.cross(n, a)


def _quad(c, n, w, h):
    a, b = _frame(np.asarray(n, np.float64))
    c = np.asarray(c, np.float64)
    return [c - a * w - b * h, c + a * w - b * h, c + a * w + b * h, c - a * w + b * h]


def _box(s, m, lo, hi, rot=0.0, shift=(0.0, 0.0, 0.0)):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    P = np.array([[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])])
    c = 0.5 * (lo + hi)
    cr, sr = np.cos(rot), np.sin(rot)
    q = P - c
    P = np.stack([c[0] + cr * q[:, 0] - sr * q[:, 2], P[:, 1], c[2] + sr * q[:, 0] + cr * q[:, 2]], axis=1) + np.asarray(shift)
    idx = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]
    s.add_mesh(P.astype(F), idx, m)


def _finish(s, lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = 0.5 * (lo + hi)
    s.camera.pos = tuple(float(x) for x in (c[0], c[1], lo[2] + 0.02 * (hi[2] - lo[2])))
    s.camera.look = tuple(float(x) for x in c)
    s.camera.fov = 60.0
    s.film.xres, s.film.yres = 32, 32
    s.sampler.spp = 4
    return s


def random_room(seed, shift=(0.0, 0.0, 0.0), one_triangle_light=False):
    """A box room (floor, ceiling, three walls; open in front), 1 - 3 blocks resting on the floor or floating (some nearly touching), and one quad light:
    on the ceiling facing down, on a wall facing in, tilted in mid-air, or just above the floor facing up."""
    rng = np.random.default_rng(seed)
    s = SceneDesc()
    s.name = f"room{seed}"
    m = s.matte((0.6, 0.6, 0.6))
    W, H, D = rng.uniform(5, 600, 3)
    sh = np.asarray(shift, np.float64)
    v = lambda *p: tuple(float(x) for x in (np.asarray(p, np.float64) + sh))
    s.add_quad(v(0, 0, 0), v(0, 0, D), v(W, 0, D), v(W, 0, 0), m)        # floor
    s.add_quad(v(0, H, 0), v(W, H, 0), v(W, H, D), v(0, H, D), m)        # ceiling
    s.add_quad(v(0, 0, D), v(0, H, D), v(W, H, D), v(W, 0, D), m)        # back wall
    s.add_quad(v(0, 0, 0), v(0, H, 0), v(0, H, D), v(0, 0, D), m)        # left wall
    s.add_quad(v(W, 0, 0), v(W, 0, D), v(W, H, D), v(W, H, 0), m)        # right wall
    k = int(rng.integers(1, 4))
    x0 = None
    for j in range(k):
        sz = rng.uniform(0.08, 0.3, 3) * np.array([W, H, D])
        lo = rng.uniform(0.05, 0.6, 3) * np.array([W, H, D])
        if rng.random() < 0.6:
            lo[1] = 0.0  # resting on the floor: a face coplanar with it
        if x0 is not None and rng.random() < 0.5:
            lo[0] = x0 + float(rng.choice([0.0, 1e-3, 0.05])) * W  # next to the previous block: touching or a thin gap
        _box(s, m, lo, lo + sz, rot=float(rng.choice([0.0, rng.uniform(0, np.pi)])), shift=sh)
        x0 = lo[0] + sz[0]
    kind = int(rng.integers(0, 4))
    lw, lh = rng.uniform(0.05, 0.25) * W, rng.uniform(0.05, 0.25) * D
    if kind == 0:
        pts = _quad((W / 2, H * (1 - 1e-3), D / 2), (0, -1, 0), lw, lh)
    elif kind == 1:
        pts = _quad((W * (1 - 1e-3), H * 0.6, D / 2), (-1, 0, 0), lh, lw)
    elif kind == 2:
        n = rng.normal(size=3)
        pts = _quad(rng.uniform(0.3, 0.7, 3) * np.array([W, H, D]), n, lw, lh)
    else:
        pts = _quad((W / 2, H * 0.02, D / 2), (0, 1, 0), lw, lh)
    if one_triangle_light:
        s.add_mesh(np.array([v(*p) for p in pts[:3]], F), [[0, 1, 2]], m, emission=(5, 5, 5))
    else:
        s.add_quad(*[v(*p) for p in pts], m, emission=(5, 5, 5))
    return _finish(s, sh, sh + np.array([W, H, D]))


def random_soup_lit(seed, shift=(0.0, 0.0, 0.0)):
    """A random triangle soup (fuzz_lds_walks.py's generator, LDS-sized) with one quad light anywhere around it in any orientation."""
    from rustracer_amd.scenes import random_soup
    rng = np.random.default_rng(seed)
    n_tris = int(rng.integers(3, 110))
    base = random_soup(n_tris, seed=int(rng.integers(1 << 30)), max_prims=int(rng.choice([1, 2, 4, 8])))
    P, idx = base.arrays()[:2]
    P = P[idx[:n_tris].reshape(-1)].reshape(-1, 3).astype(np.float64) + np.asarray(shift)  # the soup's own triangles, without its light
    s = SceneDesc()
    s.name = f"soup{seed}"
    m = s.matte((0.6, 0.6, 0.6))
    s.add_mesh(P.astype(F), np.arange(3 * n_tris).reshape(-1, 3), m)
    s.max_prims_per_node = base.max_prims_per_node
    pts = _quad(np.asarray(shift) + rng.uniform(-20, 120, 3), rng.normal(size=3), rng.uniform(2, 30), rng.uniform(2, 30))
    s.add_quad(*[tuple(float(x) for x in p) for p in pts], m, emission=(5, 5, 5))
    return _finish(s, np.asarray(shift) - 20, np.asarray(shift) + 120)


SHIFTS = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1500.0, -700.0, 2300.0), (-40.0, 25.0, 90.0)]


def test_cornell_empty_pairs_are_unoccluded():
    ss, share, occluded = check_scene(cornell_box(64, 64, 16))
    assert ss["nvox"] == (64, 63, 64)
    assert 0 < ss["empty"] < ss["pairs"]
    # S1: 45 % of the area-weighted segments (ceiling and emitters included) need no walk; some segments elsewhere are occluded (the blocks' shadows)
    assert share > 0.35 and occluded > 0.05, (share, occluded)


@pytest.mark.parametrize("seed", [2, 3])
def test_cornell_more_segments(seed):
    check_scene(cornell_box(32, 32, 4), n=100_000, seed=seed)


@pytest.mark.parametrize("seed", range(8))
def test_random_rooms(seed):
    ss, share, _ = check_scene(random_room(100 + seed, SHIFTS[seed % 4]), n=100_000, seed=seed)
    assert ss["pairs"] > 0


@pytest.mark.parametrize("seed", range(8))
def test_random_soups(seed):
    ss, share, _ = check_scene(random_soup_lit(200 + seed, SHIFTS[seed % 4]), n=100_000, seed=seed)
    assert ss["pairs"] > 0


def test_random_scenes_have_empty_pairs():
    """The random scenes above are not vacuous: several rooms have EMPTY pairs (a light in mid-air or low in the room leaves few or none)."""
    rooms = [host.HostScene(random_room(100 + k, SHIFTS[k % 4])).shadow_sets()["empty"] for k in range(8)]
    assert sum(e > 0 for e in rooms) >= 3, rooms


def test_far_from_origin_gets_no_sets():
    """A scene further than 64 extents from the origin: its float32 errors would exceed the margins - no EMPTY pair."""
    ss = host.HostScene(random_room(7, (1e5, 0.0, 1e5))).shadow_sets()
    assert ss["empty"] == 0


def test_scenes_without_sets_are_refused():
    from rustracer_amd.scenes import mis_plates
    d = mis_plates(spp=4)
    assert len(d.lights) > 2
    with pytest.raises(host.BackendError):
        host.HostScene(d).shadow_sets()
    one = host.HostScene(random_room(3, one_triangle_light=True))  # one sampled light: the distribution is uniform, nothing carries a per-voxel word
    with pytest.raises(host.BackendError):
        one.shadow_sets()
