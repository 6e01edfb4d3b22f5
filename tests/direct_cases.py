"""The scenes and ray batches of the direct-lighting integrator's tests: tests/whitted_cases.py's construction (a whitted_model.Scene and a SceneDesc from one description,
40 x 24 pixels x 4 samples = 3840 rays - 15 workgroups of the vertex kernel, the last one partial -, jittered targets, the `settled` loop) over the cases of this
integrator, each run under both light strategies. tests/test_direct_cpu.py asserts the margins of the model alone, tests/test_gpu_direct.py then compares EVERY sample."""
import os

import numpy as np

import direct_model as dm
import whitted_cases as wc
from whitted_cases import GREY, H, NS, N_SALTS, SPP, W, Both, jittered, model_rays, toward

EMIT = ("matte", 0.0)


# ---- floor: Whitted's - a matte floor, one point light, misses and skipped rays. A delta light has no probe, yet its arrays are consumed
def case_floor(salt=None):
    return wc.case_floor(salt)


# ---- area: a matte floor and a matte wall under a two-triangle emitter that faces down, with a matte blocker quad between the emitter and the floor: the light half,
# probes that end on the emitter, on the wall, on the blocker or nowhere, and the MIS weights
def case_area(salt=None):
    b = Both()
    b.quad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6), GREY)
    b.quad((-6, 0, 6), (6, 0, 6), (6, 12, 6), (-6, 12, 6), ("matte", (0.7, 0.5, 0.3)))          # the wall, normal -z
    b.quad((-1.5, 3.0, -1.0), (1.5, 3.0, -1.0), (1.5, 3.0, 2.0), (-1.5, 3.0, 2.0), EMIT, emission=(30.0, 28.0, 24.0))   # normal -y
    b.quad((0.2, 1.5, -0.6), (0.2, 1.5, 0.9), (1.4, 1.5, 0.9), (1.4, 1.5, -0.6), ("matte", 0.5))  # the blocker, normal +y
    tg = jittered(-3.5, 3.5, -3.0, 4.0, 71, salt=salt)
    tg[16:] = jittered(-3.5, 3.5, 0.3, 1.5, 72, y=6.0, axis="z", salt=salt)[16:]                  # onto the wall, low enough for the emitter to be seen well off its plane
    return b, toward((0.3, 2.4, -6.5), tg)


# ---- glass: Whitted's glass scene (slab and sphere: the GENERAL kernel) under its two-triangle area light; the last four rows of pixels see the bare floor, whose one
# vertex leaves the arrays far from exhausted, while the trees through the glass exhaust them
def _floor_rows(tg, seed, salt):
    tg[20:] = jittered(3.0, 4.6, -3.2, -1.6, seed, salt=salt)[20:]
    return tg


def case_glass(salt=None):
    b = wc._glass_scene("area")
    t = jittered(-2.4, -0.8, -1.0, 0.2, 81, y=0.9, salt=salt)
    sp = jittered(-0.3, 0.3, -0.3, 0.3, 82, y=0.9, salt=salt)
    sp[..., 0] += 1.3
    t[12:] = sp[12:]
    return b, toward((-0.9, 4.0, -2.2), _floor_rows(t, 83, salt))


def case_glass_triangles(salt=None):
    """The slab alone: no quadric, the plain kernel."""
    t = jittered(-2.4, -0.8, -1.0, 0.2, 85, y=0.9, salt=salt)
    return wc._glass_scene("area", sphere=False), toward((-0.9, 4.0, -2.2), _floor_rows(t, 86, salt))


# ---- mix: a mix of matte and mirror (one diffuse lobe scaled by the amount, one specular lobe the estimator's flags exclude) under a point light and a constant
# infinite light: a probe that leaves the scene takes le, the infinite light's pdf_li, and the reflection is followed
def case_mix(salt=None):
    b = Both()
    b.quad((-40, 0, -40), (-40, 0, 40), (40, 0, 40), (40, 0, -40), ("mix", ("matte", (0.7, 0.6, 0.5)), ("mirror", (0.9, 0.9, 0.9)), 0.6))
    b.quad((-40, -1, 4), (40, -1, 4), (40, 9, 4), (-40, 9, 4), GREY)   # a back wall through the floor, normal -z
    b.point((0.0, 3.0, 0.0), (30.0, 30.0, 30.0))
    b.infinite((0.4, 0.5, 0.7))
    return b, toward((0.0, 2.0, -5.0), jittered(-2.5, 2.5, -2.5, 2.5, 91, salt=salt))


# ---- many: Whitted's 48 listed lights over a mirror floor before a matte wall, at max_depth 3: 288 arrays
def case_many(salt=None):
    return wc.case_many(salt)


CASES = dict(many=case_many, floor=case_floor, area=case_area, glass=case_glass, glass_triangles=case_glass_triangles, mix=case_mix)
# (max_depth, dimensions) each case is rendered at, under both strategies
RUNS = dict(many=[(3, 4)], floor=[(5, 4)], area=[(5, 2), (5, 8)], glass=[(5, 4)], glass_triangles=[(5, 4)], mix=[(5, 4)])
STRATEGIES = (("all", dm.ALL), ("one", dm.ONE))
MARGIN = wc.MARGIN   # scene units, and |1 - sin^2(theta_t)|
GRAZING = 0.1        # |cos| at an emitter: the relative error of 1 / |cos| is the direction's error (~1e-5) over |cos| - 1e-4, half the flat scenes' tolerance
PICK = 1e-6          # the pick is taken from the float32 product s n, which the model forms in float32 too: any distance from an integer will do
SALTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct_salts.npz")

_cache = {}


def violations(res):
    return (res.edge < MARGIN) | (res.shadow < MARGIN) | (res.sin2 < MARGIN) | (res.grazing < GRAZING) | (res.pick < PICK)


def n_arrays(b, max_depth, strategy):
    return 2 * max_depth * len(b.model.lights) if strategy == dm.ALL else 0


def tables(orc, dims, na):
    """(the rays' draws as plain arrays, the replayed tables) of the batch at `dims` dimensions with `na` arrays, replayed once per session."""
    if ("T", dims, na) not in _cache:
        dr, tb = dm.draws_for(orc, SPP, dims, W, H, NS, 0, na)
        _cache[("T", dims, na)] = ((dr.T1, dr.T2, dr.ARR, dr.R), tb)
    return _cache[("T", dims, na)]


def _render(orc, b, rays, max_depth, dims, strategy):
    o, d = model_rays(rays)
    (T1, T2, ARR, R), _ = tables(orc, dims, n_arrays(b, max_depth, strategy))
    return dm.render(b.model, o, d, max_depth, strategy, dm.Draws(T1, T2, ARR, R, dims), rays.reshape(-1, 8)[:, 3] > 0)


def settled(orc, name):
    """whitted_cases.settled over this module's cases and both strategies: every ray whose tree, in any run, comes within a margin of a decision is moved to its next
    jitter until none does (at most N_SALTS - 1 times). Returns (Both, rays)."""
    if name not in _cache:
        salt = np.zeros((H, W, NS), int)
        if os.path.exists(SALTS):
            with np.load(SALTS) as z:
                salt = z[name].astype(int) if name in z.files else salt
        for _ in range(N_SALTS - 1):
            b, rays = CASES[name](salt)
            bad, runs = np.zeros(H * W * NS, bool), {}
            for md, dims in RUNS[name]:
                for sname, st in STRATEGIES:
                    runs[(name, md, dims, sname)] = _render(orc, b, rays, md, dims, st)
                    bad |= violations(runs[(name, md, dims, sname)])
            if not bad.any():
                _cache.update(runs)
                break
            salt = salt + bad.reshape(H, W, NS)
        _cache[name] = CASES[name](salt)
        _cache[("salt", name)] = salt
    return _cache[name]


def reference(orc, name, max_depth, dims, sname):
    """(the model's Result of a run, computed once per session; the case (Both, rays))."""
    key = (name, max_depth, dims, sname)
    if key not in _cache:
        b, rays = settled(orc, name)
        _cache[key] = _render(orc, b, rays, max_depth, dims, dict(STRATEGIES)[sname])
    return _cache[key], _cache[name]
