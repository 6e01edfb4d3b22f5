"""The scenes and ray batches of the Whitted integrator's tests, each built twice from one description: as the model's own world-space triangles and spheres
(whitted_model.Scene) and as a SceneDesc for the backend. Ray batches are 40 x 24 pixels x 4 samples = 3840 rays - 15 workgroups of the vertex kernel, the last one
partial - aimed by `toward` at chosen points, so that every li ray and every visibility segment keeps its distance from edges, silhouettes, shadow boundaries and the
critical angle: tests/test_whitted_cpu.py asserts that of the model alone, tests/test_gpu_whitted.py then compares EVERY sample.

The targets of a batch are a jittered grid inside a rectangle (a fixed seed), never on a grid line of the scene: a quad's outline, a slab's outline, a shadow's edge."""
import os

import numpy as np

import whitted_model as wm

W, H, NS = 40, 24, 4
SPP = 4


class Both:
    """A whitted_model.Scene and the calls that rebuild it as a SceneDesc."""

    def __init__(self):
        self.model = wm.Scene()
        self.calls = []

    def quad(self, p0, p1, p2, p3, mat, emission=None):
        self.model.add_quad(p0, p1, p2, p3, mat, emission)
        self.calls.append(("quad", (p0, p1, p2, p3), mat, emission))

    def sphere(self, c, r, mat):
        self.model.add_sphere(c, r, mat)
        self.calls.append(("sphere", (c, r), mat, None))

    def point(self, pos, I):
        self.model.lights.append(("point", pos, I))
        self.calls.append(("point", pos, I, None))

    def distant(self, w_light, L):
        self.model.lights.append(("distant", w_light, L))
        self.calls.append(("distant", w_light, L, None))

    def infinite(self, L, rows=8):
        self.model.lights.append(("infinite", L, rows))
        self.calls.append(("infinite", L, rows, None))

    def box(self, lo, hi, mat):
        """An axis-aligned box of six outward-facing quads (normal (p0 - p2) x (p1 - p2))."""
        x0, y0, z0 = lo
        x1, y1, z1 = hi
        c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
        for q in ((0, 3, 2, 1), (4, 5, 6, 7), (0, 4, 7, 3), (1, 2, 6, 5), (3, 7, 6, 2), (0, 1, 5, 4)):
            self.quad(*[c[i] for i in q], mat)

    def desc(self, dims=4):
        from rustracer_amd.scene_desc import SceneDesc
        s = SceneDesc()
        s.film.xres, s.film.yres = 32, 32
        s.film.filter_kind, s.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)
        s.sampler.spp, s.sampler.dims = SPP, dims
        s.camera.pos, s.camera.look, s.camera.fov = (0.0, 2.2, -5.0), (0.0, 0.6, 0.0), 40.0

        def mat(m):
            if m[0] == "matte":
                return s.matte(m[1])
            if m[0] == "mirror":
                return s.mirror(m[1])
            if m[0] == "glass":
                return s.glass(m[1], m[2], m[3])
            return s.mix(mat(m[1]), mat(m[2]), m[3])
        cache = {}
        for kind, a, b, em in self.calls:
            if kind == "quad":
                cache.setdefault(repr(b), mat(b))
                s.add_quad(*a, cache[repr(b)], emission=em)
            elif kind == "sphere":
                cache.setdefault(repr(b), mat(b))
                s.add_sphere(a[0], a[1], cache[repr(b)])
            elif kind == "point":
                s.point_light(a, b)
            elif kind == "distant":
                s.distant_light(a, (0.0, 0.0, 0.0), b)
            else:
                s.infinite_light(s.add_mip(np.tile(np.float32(a), (b // 2, b, 1))))  # the sampling distribution has twice the map's rows (infinite.rs:80)
        return s


N_SALTS = 12


def jittered(x0, x1, z0, z1, seed, y=0.0, axis="y", salt=None):
    """(H, W, NS, 3) targets on a jittered H x (W * NS) grid inside the rectangle, in the plane `axis` = y. salt (H, W, NS) ints < N_SALTS: which of the seed's
    jitters each ray takes (`settled` moves a ray whose tree comes close to a decision to its next one)."""
    rnd = np.random.default_rng(seed).random((N_SALTS, 2, H, W * NS))
    k = np.zeros((1, H, W * NS), int) if salt is None else np.asarray(salt).reshape(1, H, W * NS)
    rx, rz = np.take_along_axis(rnd[:, 0], k, 0)[0], np.take_along_axis(rnd[:, 1], k, 0)[0]
    gx = (np.arange(W * NS) + 0.2 + 0.6 * rx) / (W * NS)
    gz = (np.arange(H)[:, None] + 0.2 + 0.6 * rz) / H
    a, b = x0 + (x1 - x0) * gx, z0 + (z1 - z0) * gz
    t = np.stack([a, np.full_like(a, y), b], axis=-1) if axis == "y" else np.stack([a, b, np.full_like(a, y)], axis=-1)
    return t.reshape(H, W, NS, 3)


def toward(eye, targets, t_max=np.inf):
    """(H, W, NS, 8) float32 ray records from `eye` (a point, or per-ray origins) toward the targets, unit directions; and the same rays in float64 as the records hold them."""
    t = np.asarray(targets, np.float64)
    e = np.broadcast_to(np.asarray(eye, np.float64), t.shape)
    d = t - e
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    r = np.zeros(t.shape[:-1] + (8,), np.float32)
    r[..., 0:3], r[..., 3], r[..., 4:7] = e, t_max, d
    return r


def model_rays(rays):
    """The origins and directions the records hold, as float64 (n, 3) each."""
    r = np.asarray(rays, np.float32).reshape(-1, rays.shape[-1]).astype(np.float64)
    return r[:, 0:3], r[:, 4:7]


GREY = ("matte", 0.6)


# Every case is a function of the salt: (Both, rays).
# ---- 1: a matte floor under one point light; a third of the rays leave above the floor's far edge, one column of pixels and one more ray are skipped
def case_floor(salt=None):
    b = Both()
    b.quad((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4), GREY)
    b.point((0.5, 3.0, -0.5), (40.0, 36.0, 30.0))
    tg = jittered(-3.0, 3.0, -3.0, 3.0, 11, salt=salt)
    tg[16:] = jittered(-3.0, 3.0, 5.0, 9.0, 12, y=6.0, salt=salt)[16:]  # the sky: a miss
    rays = toward((0.3, 2.5, -6.0), tg)
    rays[:, 7, :, 3] = 0.0   # t_max not > 0: skipped
    rays[3, 9, 2, 3] = -1.0
    return b, rays


# ---- 2: two facing mirrors, one unit apart, that end at a lit matte wall: a ray bounces between them until the depth limit or the wall
def case_mirrors(salt=None):
    b = Both()
    mir = ("mirror", 0.9)
    b.quad((-0.5, 0, -2), (-0.5, 0, 12), (-0.5, 3, 12), (-0.5, 3, -2), mir)   # normal +x
    b.quad((0.5, 0, -2), (0.5, 3, -2), (0.5, 3, 12), (0.5, 0, 12), mir)       # normal -x
    b.quad((-0.5, 0, 12), (0.5, 0, 12), (0.5, 3, 12), (-0.5, 3, 12), GREY)    # the end wall, normal -z
    b.point((0.1, 1.5, 1.0), (30.0, 30.0, 30.0))
    b.distant((0.05, 0.3, -1.0), (1.5, 1.2, 1.0))
    # from between the mirrors toward the left one, 0.3 - 1.5 units further in z: z advances by that per 0.7 in x, so the wall is reached after 6 - 28 crossings
    g = jittered(0.3, 1.5, 1.45, 1.55, 21, salt=salt)
    tg = np.stack([np.full(g.shape[:-1], -0.5), g[..., 2], g[..., 0]], axis=-1)
    return b, toward((0.2, 1.5, 0.0), tg)


# ---- 3: a glass slab (a closed box) and a glass sphere over a matte floor, in front of a matte wall the reflections see; the light stands above the slab, so the floor
# seen through it lies well inside its shadow
GLASS = ("glass", 1.0, 1.0, 1.5)
SLAB = ((-3.0, 0.6, -1.5), (-0.2, 0.9, 1.5))


def _glass_scene(light="point", sphere=True):
    b = Both()
    b.quad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6), GREY)
    b.quad((-6, 0, 6), (6, 0, 6), (6, 12, 6), (-6, 12, 6), ("matte", (0.7, 0.5, 0.3)))   # the wall, normal -z
    b.box(*SLAB, GLASS)
    if sphere:
        b.sphere((1.3, 0.9, 0.0), 0.5, GLASS)
    if light == "point":
        b.point((-1.2, 5.0, -0.4), (2000.0, 1800.0, 1500.0))
    else:  # a two-triangle area light facing down: two lights, two draws per vertex
        b.quad((-1.8, 5.0, -1.0), (-0.6, 5.0, -1.0), (-0.6, 5.0, 0.2), (-1.8, 5.0, 0.2), ("matte", 0.0), emission=(40.0, 40.0, 40.0))
    return b


def _glass_rays(seed, salt, sphere=True):
    tg = jittered(-2.4, -0.8, -1.0, 0.2, seed, y=0.9, salt=salt)           # onto the slab's top face
    if sphere:
        sp = jittered(-0.3, 0.3, -0.3, 0.3, seed + 1, y=0.9, salt=salt)   # into the sphere's disc as seen from above: well inside its silhouette
        sp[..., 0] += 1.3
        tg[12:] = sp[12:]
    return toward((-0.9, 4.0, -2.2), tg)


def case_glass(salt=None):
    return _glass_scene("point"), _glass_rays(31, salt)


def case_glass_triangles(salt=None):
    """The slab without the sphere: no quadric, the plain kernel."""
    return _glass_scene("point", sphere=False), _glass_rays(33, salt, sphere=False)


def case_glass_inside(salt=None):
    """Rays that start INSIDE the slab and meet its top face beyond the critical angle (41.8 degrees at eta 1.5), 50 - 60 degrees from the normal: no transmission child."""
    b = _glass_scene("point")
    tg = jittered(-2.7, -2.3, -1.0, 1.0, 35, y=0.9, salt=salt)
    ang = np.radians(50.0 + 10.0 * (tg[..., 2] + 1.0) / 2.0)
    eye = tg.copy()
    eye[..., 1] = 0.75
    eye[..., 0] = tg[..., 0] - 0.15 * np.tan(ang)
    return b, toward(eye, tg)


# ---- 4: draw order - the glass scene under the two-triangle area light
def case_area(salt=None):
    return _glass_scene("area"), _glass_rays(41, salt)


# ---- 5: a mix of two mirrors (two SPEC_R lobes: u[0] chooses), and a constant infinite light
def case_mix(salt=None):
    b = Both()
    b.quad((-40, 0, -40), (-40, 0, 40), (40, 0, 40), (40, 0, -40), ("mix", ("mirror", (0.9, 0.5, 0.2)), ("mirror", (0.2, 0.5, 0.9)), 0.3))
    b.quad((-40, -1, 4), (40, -1, 4), (40, 9, 4), (-40, 9, 4), GREY)   # a back wall through the floor, normal -z: no outline near a ray that skims the floor
    b.point((0.0, 3.0, 0.0), (30.0, 30.0, 30.0))
    b.infinite((0.4, 0.5, 0.7))
    return b, toward((0.0, 2.0, -5.0), jittered(-2.5, 2.5, -2.5, 2.5, 51, salt=salt))


# ---- 6: many lights - 24 separate emitting quads (48 listed lights: 48 rounds per step) over a mirror floor before a matte wall: every ray meets the mirror (48 draws, no
# term), then the wall (48 terms). The quads stand apart, so no visibility segment that ends on one passes its neighbour's outline
def case_many(salt=None):
    b = Both()
    b.quad((-6, 0, -6), (-6, 0, 3), (6, 0, 3), (6, 0, -6), ("mirror", 0.8))
    b.quad((-30, -1, 3), (30, -1, 3), (30, 40, 3), (-30, 40, 3), GREY)   # the wall through the floor's far edge, normal -z
    for i in range(6):
        for j in range(4):
            x, z = -2.7 + 0.9 * i, -4.0 + 0.9 * j
            b.quad((x, 6.0, z), (x + 0.6, 6.0, z), (x + 0.6, 6.0, z + 0.6), (x, 6.0, z + 0.6), ("matte", 0.0), emission=(3.0 + 0.2 * i, 3.0, 3.0 + 0.3 * j))
    return b, toward((0.0, 2.0, -5.5), jittered(-2.0, 2.0, -2.5, 1.5, 61, salt=salt))


CASES = dict(many=case_many, floor=case_floor, mirrors=case_mirrors, glass=case_glass, glass_triangles=case_glass_triangles, glass_inside=case_glass_inside, area=case_area, mix=case_mix)
# (max_depth, dimensions) each case is rendered at
RUNS = dict(many=[(3, 4)], floor=[(1, 4), (5, 4)], mirrors=[(1, 4), (2, 4), (5, 4), (16, 4)], glass=[(5, 4)], glass_triangles=[(5, 4)], glass_inside=[(5, 4)],
            area=[(5, 2), (5, 8)], mix=[(5, 4)])
N_DRAWS = 160  # more than any sample of these cases consumes (asserted by the model's own indexing)

MARGIN = 1e-3  # scene units, and |1 - sin^2(theta_t)|
SALTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "whitted_salts.npz")

_cache = {}


def violations(res):
    return (res.edge < MARGIN) | (res.shadow < MARGIN) | (res.sin2 < MARGIN)


def _draws(orc, dims):
    if ("U", dims) not in _cache:
        _cache[("U", dims)] = wm.draws_for(orc, SPP, dims, W, H, NS, 0, N_DRAWS)
    return _cache[("U", dims)]


def _render(orc, b, rays, max_depth, dims):
    o, d = model_rays(rays)
    return wm.render(b.model, o, d, max_depth, _draws(orc, dims), rays.reshape(-1, 8)[:, 3] > 0)


def settled(orc, name):
    """The case with every ray whose tree, in any of the case's runs, comes within MARGIN of a decision moved to its next jitter, until none does (at most N_SALTS - 1
    times; tests/test_whitted_cpu.py asserts the result). Deterministic: the jitters are functions of the case's seed. Returns (Both, rays)."""
    if name not in _cache:
        salt = np.zeros((H, W, NS), int)
        if os.path.exists(SALTS):  # where an earlier settling ended (tests/golden): nothing moves again unless a case was edited
            with np.load(SALTS) as z:
                salt = z[name].astype(int) if name in z.files else salt
        for _ in range(N_SALTS - 1):
            b, rays = CASES[name](salt)
            bad, runs = np.zeros(H * W * NS, bool), {}
            for md, dims in RUNS[name]:
                runs[(name, md, dims)] = _render(orc, b, rays, md, dims)
                bad |= violations(runs[(name, md, dims)])
            if not bad.any():
                _cache.update(runs)   # (the settled case's runs: `reference` need not render them again)
                break
            salt = salt + bad.reshape(H, W, NS)
        _cache[name] = CASES[name](salt)
        _cache[("salt", name)] = salt
    return _cache[name]


def reference(orc, name, max_depth, dims):
    """(the model's Result of a run, computed once per session; the case (Both, rays))."""
    key = (name, max_depth, dims)
    if key not in _cache:
        b, rays = settled(orc, name)
        _cache[key] = _render(orc, b, rays, max_depth, dims)
    return _cache[key], _cache[name]
