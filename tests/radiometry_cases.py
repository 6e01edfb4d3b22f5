"""The direct-lighting cases of tests/test_radiometry_model_cpu.py (oracle) and tests/test_gpu_radiometry.py (HIP path): for each, the SceneDesc - a Lambertian
receiver, the lights, nothing else -, the same lights as tests/radiometry_model.py describes them, receiver points with their normals, and one ray per point.

The world is y-up. Receivers: `floor` (the quad |x|, |z| <= 6 of the plane y = 0; as two triangles, as a disk quadric, or as two triangles inside a rotated
object instance that lands on the same plane) and `pyramid` (the four side faces of the pyramid with apex (0, 1, 0) over the square |x|, |z| <= 1: a convex
body, so that no face sees another and a face that looks away from a light is black). Every point's ray comes from 1 - 2 units away, from a direction that
leans away from the emitter (so that it does not cross it; tests/test_radiometry_model_cpu.py traces every ray of every case and requires the receiver at the
ray's own length), at polar angles between 8 and 80 degrees.
"""
import os
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import radiometry_model as rm

FLOOR = 6.0
N_SAMPLES = 16384
FRONT_ENDS = ("const", "image", "plastic", "uber", "mix")
# front end -> the one vertex counter of rt_stats that may be non-zero. The constant-matte kernel exists for scenes of plain triangles whose lights are all
# triangle emitters (rtx_scene_plan.h: "the constant-matte kernel has no GENERAL form"): with a quadric, an instance or another kind of light in the scene a
# constant matte shades through the Lambert front end, see `counter`.
COUNTER = dict(const="vertices_lambert_const", image="vertices_lambert", plastic="vertices_two_lobe", uber="vertices_two_lobe", mix="vertices_generic")
CONST_KERNEL_CASES = ("quad", "quad_two_sided", "quad_reversed", "quad_normals", "quad_overhead", "two_triangles_occluder")
VERTEX_COUNTERS = ("vertices_lambert_const", "vertices_lambert", "vertices_two_lobe", "vertices_generic")


def counter(case_name, front_end):
    return "vertices_lambert" if front_end == "const" and case_name not in CONST_KERNEL_CASES else COUNTER[front_end]


@dataclass
class Case:
    name: str
    desc: object
    lights: list
    rho: float
    x: np.ndarray            # (P, 3) receiver points
    n: np.ndarray            # (P, 3) their unit normals (the side the rays come from)
    d_in: np.ndarray         # (P, 3) unit, from the point to its ray's origin
    h: np.ndarray            # (P,) length of the ray up to the point
    occluders: object = None
    extra: np.ndarray = None  # (P,) absolute allowance on the radiance, for points in an emitter's plane (see _in_plane_allowance)
    tol: float = 2e-6         # of the model's quadrature
    probes: list = field(default_factory=list)   # (origin, direction, expected rgb) of max_depth = 0 rays aimed at the emitters
    mat: int = 0              # the receiver's material

    def rays(self, n_samples=N_SAMPLES):
        """(1, P, n_samples, 8) float32: every sample of "pixel" p is the same ray."""
        r = np.zeros((1, self.x.shape[0], n_samples, 8), np.float32)
        o = self.x + self.h[:, None] * self.d_in
        r[0, :, :, 0:3], r[0, :, :, 3], r[0, :, :, 4:7] = o[:, None, :], np.inf, -self.d_in[:, None, :]
        return r


# ------------------------------------------------------------------------------------------------ the model's values, once per case
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "radiometry_model.npz")
_MODEL = {}


def compute_model_radiance(case):
    """(M (P, 3) = rho / pi * E, the quadrature's two-resolution difference relative to the value (P,)). What does not depend on the point - an environment or a
    distant light without occluders - is integrated once per normal."""
    m, rel, seen = np.zeros((case.x.shape[0], 3)), np.zeros(case.x.shape[0]), {}
    everywhere = case.occluders is None and all(isinstance(l, (rm.Infinite, rm.Distant)) for l in _flat(case.lights))
    for k, (x, n) in enumerate(zip(case.x, case.n)):
        key = tuple(n) if everywhere else k
        if key not in seen:
            seen[key] = rm.irradiance(case.lights, x, n, case.occluders, tol=case.tol)
        e, d = seen[key]
        m[k], rel[k] = case.rho / np.pi * e, (d / e.max() if e.max() > 0 else d)
    return m, rel


def model_radiance(case):
    """M (P, 3) of the case: from tests/golden/radiometry_model.npz where that holds the case with these very points and normals (the quadrature of an occluder's
    outline takes a minute: tests/test_radiometry_model_cpu.py recomputes every case and holds the file to it; `python tests/radiometry_cases.py` writes it),
    computed otherwise."""
    if case.name not in _MODEL:
        m = None
        if os.path.exists(GOLDEN):
            with np.load(GOLDEN) as g:
                if case.name + "/M" in g and np.array_equal(g[case.name + "/x"], case.x) and np.array_equal(g[case.name + "/n"], case.n):
                    m = g[case.name + "/M"].copy()
        m = compute_model_radiance(case)[0] if m is None else m
        m.setflags(write=False)
        _MODEL[case.name] = m
    return _MODEL[case.name]


# ------------------------------------------------------------------------------------------------ receivers and their materials
RHO = 0.6


def receiver_material(s, front_end, rho=RHO):
    """Five materials whose BSDF is f = rho / pi, one per shade front end."""
    if front_end == "const":
        return s.matte((rho,) * 3)
    if front_end == "image":      # a matte whose Kd is an image map of one value
        return s.matte(s.image_tex(s.add_mip(np.full((4, 4, 3), rho, np.float32))))
    if front_end == "plastic":
        return s.plastic(kd=(rho,) * 3, ks=0.0)
    if front_end == "uber":       # opaque, no gloss, no specular lobes
        return s.uber(kd=(rho,) * 3, ks=0.0, kr=0.0, kt=0.0, opacity=1.0)
    if front_end == "mix":        # MixMaterial scales its first material by `amount` and the second by 1 - amount (material/mixmat.rs:41-56)
        a, r1 = 0.25, 0.9
        return s.mix(s.matte((r1,) * 3), s.matte(((rho - a * r1) / (1 - a),) * 3), amount=a)
    raise ValueError(front_end)


def _roty(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s, -s, c
    return m


def add_floor(s, mat, how="tris", half=FLOOR):
    q = np.float32([(-half, 0, -half), (-half, 0, half), (half, 0, half), (half, 0, -half)])
    if how == "tris":
        s.add_mesh(q, [[0, 1, 2], [0, 2, 3]], mat, UV=[(0, 0), (0, 1), (1, 1), (1, 0)])
    elif how == "disk":       # a disk quadric: object z is the world's y
        o2w = np.float32([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]])
        s.add_disk(o2w, radius=1.5 * half, material=mat)
        # a small scene of quadrics still walks in LDS (the GENERAL form of that kernel); one instance of a triangle, out of everyone's sight 5 below the disk,
        # makes it a scene for the other trace kernels
        under = s.add_object([dict(P=np.float32([(-0.1, 0, -0.1), (0.1, 0, -0.1), (0, 0, 0.1)]), idx=np.int32([[0, 1, 2]]), material=mat)])
        m = np.eye(4, dtype=np.float32)
        m[1, 3] = -5.0
        s.add_instance(under, m)
    elif how == "instance":   # the same quad, defined in an object and placed by a rotation about y and a shift in the plane
        m = _roty(30.0)
        m[:3, 3] = (0.3, 0.0, -0.2)
        inv = np.linalg.inv(m)
        o = s.add_object([dict(P=(np.float64(q) * 1.5) @ inv[:3, :3].T + inv[:3, 3], idx=np.int32([[0, 1, 2], [0, 2, 3]]), material=mat)])
        s.add_instance(o, m.astype(np.float32))
    else:
        raise ValueError(how)


APEX = np.array([0.0, 1.0, 0.0])
BASE = np.array([(1.0, 0.0, 1.0), (1.0, 0.0, -1.0), (-1.0, 0.0, -1.0), (-1.0, 0.0, 1.0)])


def add_pyramid(s, mat):
    s.add_mesh(np.float32([APEX, *BASE]), [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], mat, UV=[(0.5, 0.5), (0, 0), (1, 0), (1, 1), (0, 1)])


def pyramid_points(per_face=10, seed=5):
    rng = np.random.default_rng(seed)
    xs, ns = [], []
    for k in range(4):
        a, b = BASE[k], BASE[(k + 1) % 4]
        n = np.cross(a - APEX, b - APEX)
        n /= np.linalg.norm(n)
        n = n if n[1] > 0 else -n
        w = rng.dirichlet((1.5, 1.5, 1.5), per_face) * 0.94 + 0.02     # barycentrics that stay 2 % off every edge
        xs.append(w @ np.array([APEX, a, b]))
        ns.append(np.tile(n, (per_face, 1)))
    return np.concatenate(xs), np.concatenate(ns)


def _tangent_frame(n):
    t = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.6 else [0.0, 0.0, 1.0])
    t /= np.linalg.norm(t)
    return t, np.cross(n, t)


POLAR = (8.0, 30.0, 55.0, 78.0)
LENGTH = (1.0, 1.3, 1.7, 2.0)
SWING = (0.0, 50.0, -35.0, 20.0, -50.0)


def lean_away(x, n, centre, polar=POLAR):
    """Per point a unit direction in n's hemisphere whose part in the receiver's plane points away from `centre` (swung by up to 50 degrees; along +x for a
    point right under it), at a polar angle from `polar` in turn, and a length from LENGTH."""
    d, h = np.zeros_like(x), np.zeros(x.shape[0])
    for k in range(x.shape[0]):
        away = x[k] - np.asarray(centre, np.float64)
        away = away - (away @ n[k]) * n[k]
        if np.linalg.norm(away) < 1e-6:
            away = np.array([1.0, 0.0, 0.0]) - n[k][0] * n[k]
        away /= np.linalg.norm(away)
        side = np.cross(n[k], away)
        sw, po = np.radians(SWING[k % len(SWING)]), np.radians(polar[k % len(polar)])
        flat = np.cos(sw) * away + np.sin(sw) * side
        d[k], h[k] = np.cos(po) * n[k] + np.sin(po) * flat, LENGTH[(k // 2) % len(LENGTH)]
    return d, h


def floor_points(xs, zs):
    x = np.array([(a, 0.0, b) for a in xs for b in zs], np.float64)
    return x, np.tile([0.0, 1.0, 0.0], (x.shape[0], 1))


def _finish(s, strategy="spatial"):
    s.film.xres = s.film.yres = 1
    s.film.filter_kind, s.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)
    s.sampler.spp, s.integrator.max_depth, s.integrator.light_strategy = N_SAMPLES, 1, strategy
    return s


def _scene():
    from rustracer_amd.scene_desc import SceneDesc
    return SceneDesc()


def _rigid(rot, shift):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rot, shift
    return m


def _rot_from_to(a, b, twist=0.0):
    """The rotation that takes unit a to unit b, followed by a rotation by `twist` about b."""
    def rodrigues(k, ang):
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    k = np.cross(a, b)
    r = rodrigues(k / np.linalg.norm(k), np.arctan2(np.linalg.norm(k), a @ b))
    return rodrigues(b, twist) @ r


def _emitter_probes(lights, keep):
    """max_depth = 0 rays at points of each emitter, from 0.35 in front of it (expect Le) and from 0.35 behind (Le if two-sided, else 0); `keep(origin)`
    says whether a ray from there reaches the emitter before anything else."""
    out = []
    for l in lights:
        point, (ue, ve) = l.param(np.zeros(3) + 100.0)
        for fu, fv in ((0.3, 0.6), (0.7, 0.2), (0.55, 0.85)):
            u, v = np.array(ue[0] + fu * (ue[-1] - ue[0])), np.array(ve[0] + fv * (ve[-1] - ve[0]))
            y, ny, _ = point(u, v)
            skew = np.cross(ny, [0.3, 0.5, 0.8])
            for side in (1.0, -1.0):
                o = y + side * 0.35 * ny + 0.05 * skew
                if keep(o) and keep(y):
                    out.append((o, (y - o) / np.linalg.norm(y - o), l.le if (side > 0 or l.two_sided) else np.zeros(3)))
    return out


def _flat(lights):
    out = []
    for l in lights:
        out.extend(l if isinstance(l, (list, tuple)) else [l])
    return out


# ------------------------------------------------------------------------------------------------ the cases
QUAD_LE = (8.0, 10.0, 6.0)
QUAD_Y0 = 0.6      # the height of its lower edge. (At 0.1 the nearest receivers see it over a steradian and the BSDF-sampled half carries weight, but their noise breaks the pooled cap: 3.4e-3.)
QUAD_P = [(0.0, QUAD_Y0, 0.5), (0.0, QUAD_Y0, -0.5), (0.0, QUAD_Y0 + 1.0, -0.5), (0.0, QUAD_Y0 + 1.0, 0.5)]   # in the plane x = 0; (p0 - p2) x (p1 - p2) points along +x


def _in_plane_allowance(x, le, rho):
    """A receiver in the plane of the emitter gets E = 0, but its float32 hit point is off that plane by up to a few ulp of the receiver's size, d = 8 * 2^-24 *
    FLOOR, and so may see the emitter at the cosine d / r: E <= Le d int y / (y^2 + z^2)^2 dA <= Le d int_y0^inf pi / (2 y^2) dy = Le d pi / (2 y0), y0 the height
    of the emitter's lower edge."""
    d = 8.0 * 2.0 ** -24 * FLOOR
    return np.where(np.abs(x[:, 0]) < 1e-9, rho / np.pi * le * d * np.pi / (2.0 * QUAD_Y0), 0.0)


def quad_case(front_end="const", receiver="tris", two_sided=False, reverse=False, normals=False):
    """A 1 x 1 emitter standing in the plane x = 0, 0.6 above the floor: receivers in front of it, behind it and in its plane."""
    s = _scene()
    mat = receiver_material(s, front_end)
    add_floor(s, mat, receiver)
    nrm = None
    if normals:   # vertex normals on the far side of the geometric normal: the emitter's normal is turned to their side (mesh.rs:418, 623)
        nrm = np.array([(-1.0, 0.2, 0.1), (-1.0, -0.1, 0.2), (-1.0, 0.15, -0.2), (-1.0, -0.2, -0.1)])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    s.add_mesh(QUAD_P, [[0, 1, 2], [0, 2, 3]], s.matte((0.0, 0.0, 0.0)), N=nrm, reverse_orientation=reverse, emission=QUAD_LE, two_sided=two_sided)
    lights = rm.quad(*QUAD_P, QUAD_LE, two_sided=two_sided, reverse_orientation=reverse, normals=nrm)
    x, n = floor_points((-4.0, -2.0, -1.0, -0.5, -0.15, 0.0, 0.15, 0.5, 1.0, 2.0, 4.0), (0.0, 0.45, 1.2, 3.0))
    d, h = lean_away(x, n, (0.0, 0.0, 0.0))
    name = "quad" + ("_two_sided" if two_sided else "") + ("_reversed" if reverse else "") + ("_normals" if normals else "")
    name += ("" if receiver == "tris" else "_on_" + receiver)
    c = Case(name, _finish(s), lights, RHO, x, n, d, h, extra=_in_plane_allowance(x, QUAD_LE[1], RHO), mat=mat)
    c.probes = _emitter_probes(lights, lambda o: o[1] > 0.05)
    return c


SPHERE_LE = (20.0, 25.0, 15.0)


def sphere_outside_case(front_end="const"):
    """A sphere of radius 0.5 whose lowest point is 0.005 above the floor: the receiver under it is at 1.01 radii from its centre."""
    s = _scene()
    mat = receiver_material(s, front_end)
    add_floor(s, mat)
    c0, r = (0.0, 0.505, 0.0), 0.5
    s.add_sphere(c0, r, s.matte((0.0, 0.0, 0.0)), emission=SPHERE_LE)
    lights = [rm.Sphere(_rigid(np.eye(3), c0), r, SPHERE_LE)]
    ring = [(rad * np.cos(a), rad * np.sin(a)) for k, rad in enumerate((0.3, 0.6, 1.0, 1.5, 2.5, 4.0)) for a in np.radians(np.arange(6) * 60.0 + 11.0 * k)]
    x = np.array([(0.0, 0.0, 0.0)] + [(a, 0.0, b) for a, b in ring])
    n = np.tile([0.0, 1.0, 0.0], (x.shape[0], 1))
    d, h = lean_away(x, n, (0.0, 0.0, 0.0))
    under = np.hypot(x[:, 0], x[:, 2]) < 0.7      # under the sphere or next to it: only a grazing ray passes below it
    flat = np.array([(1.0, 0.0, 0.0) if np.hypot(p[0], p[2]) < 1e-9 else (p[0], 0.0, p[2]) / np.hypot(p[0], p[2]) for p in x])
    graze = np.radians(84.0)
    d[under] = np.cos(graze) * n[under] + np.sin(graze) * flat[under]
    c = Case("sphere_outside", _finish(s), lights, RHO, x, n, d, h, mat=mat)
    c.probes = _emitter_probes(lights, lambda o: o[1] > 0.05)
    return c


def sphere_inside_case():
    """A two-sided sphere of radius 3 around a small floor: E = pi Le at every point."""
    s = _scene()
    add_floor(s, receiver_material(s, "const"), half=2.0)
    c0, r, le = (0.0, 0.5, 0.0), 3.0, (1.5, 2.0, 1.0)
    s.add_sphere(c0, r, s.matte((0.0, 0.0, 0.0)), emission=le, two_sided=True)
    lights = [rm.Sphere(_rigid(np.eye(3), c0), r, le, two_sided=True)]
    x, n = floor_points((-1.7, -0.9, -0.2, 0.3, 1.0, 1.8), (-1.5, -0.8, -0.1, 0.5, 1.1, 1.9))
    d, h = lean_away(x, n, (9.0, 0.0, 7.0))
    h = np.minimum(h, 1.0)
    c = Case("sphere_inside", _finish(s), lights, RHO, x, n, d, h)
    c.probes = _emitter_probes(lights, lambda o: o[1] > 0.05)      # from inside and from outside: the floor lies inside the sphere, below both ends
    return c


def disk_case():
    """A two-sided disk of radius 0.6 at (0, 1.5, 0) whose normal is 35 degrees off straight down: the floor beyond x = -2.14 sees its other side. (Two-sided: the
    reference's one-sided disk emits to one side when sampled and to the other when hit, see tests/radiometry_model.py.)"""
    s = _scene()
    add_floor(s, receiver_material(s, "const"))
    t = np.radians(35.0)
    nz = np.array([np.sin(t), -np.cos(t), 0.0])
    rot = np.stack([np.array([np.cos(t), np.sin(t), 0.0]), np.cross(nz, [np.cos(t), np.sin(t), 0.0]), nz], axis=1)
    o2w, le = _rigid(rot, (0.0, 1.5, 0.0)), (9.0, 12.0, 7.0)
    s.add_disk(o2w.astype(np.float32), 0.6, s.matte((0.0, 0.0, 0.0)), emission=le, two_sided=True)
    lights = [rm.Disk(o2w, 0.6, le, two_sided=True)]
    x, n = floor_points((-4.5, -3.0, -1.5, -0.6, 0.0, 0.5, 1.1, 2.0, 3.2, 5.0), (0.0, 0.5, 1.4, 3.0))
    d, h = lean_away(x, n, (0.0, 0.0, 0.0), polar=(30.0, 55.0, 78.0, 65.0))
    c = Case("disk_tilted", _finish(s), lights, RHO, x, n, d, h)
    c.probes = _emitter_probes(lights, lambda o: o[1] > 0.05)
    return c


OVERHEAD_Y = 0.7
OVERHEAD_POLAR = (72.0, 76.0, 80.0, 78.0)     # a ray of length 2 at 72 degrees starts 0.62 above the floor: every ray stays under the emitter


def _overhead_points():
    x, n = floor_points((-2.5, -1.4, -0.8, -0.3, 0.2, 0.7, 1.2, 1.8, 3.0), (-1.6, -0.6, 0.1, 0.9, 2.2))
    return (x, n) + lean_away(x, n, (0.0, 0.0, 0.0), polar=OVERHEAD_POLAR)


def quad_overhead_case():
    """A 2 x 2 one-sided emitter 0.7 above the floor and parallel to it, receivers under and around it. Under it the light's solid-angle density r^2 / (A cos) is
    0.1 - 0.3 against the BSDF's cos / pi of 0.3: the BSDF-sampled half of the estimator carries about half of the weight, so this is the case that holds the
    light's pdf in that half (area_light_pdf_li: the re-intersection, its normal, the quotient by the area). The upright 1 x 1 quad leaves it a per cent."""
    s = _scene()
    mat = receiver_material(s, "const")
    add_floor(s, mat)
    q = [(-1.0, OVERHEAD_Y, -1.0), (1.0, OVERHEAD_Y, -1.0), (1.0, OVERHEAD_Y, 1.0), (-1.0, OVERHEAD_Y, 1.0)]
    le = (2.0, 2.5, 1.5)
    s.add_mesh(q, [[0, 1, 2], [0, 2, 3]], s.matte((0.0, 0.0, 0.0)), emission=le)
    lights = rm.quad(*q, le)
    assert rm.irradiance(lights, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))[0][1] > 0     # it faces the floor
    x, n, d, h = _overhead_points()
    c = Case("quad_overhead", _finish(s), lights, RHO, x, n, d, h, mat=mat)
    c.probes = _emitter_probes(lights, lambda o: o[1] > 0.05)
    return c


def disk_overhead_case():
    """A two-sided disk of radius 1.2, 0.7 above the floor and parallel to it: as quad_overhead, for Shape::pdf_wi's default form (disk and cylinder)."""
    s = _scene()
    add_floor(s, receiver_material(s, "const"))
    rot = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])      # object z is the world's y
    o2w, le = _rigid(rot, (0.0, OVERHEAD_Y, 0.0)), (2.0, 2.5, 1.5)
    s.add_disk(o2w.astype(np.float32), 1.2, s.matte((0.0, 0.0, 0.0)), emission=le, two_sided=True)
    lights = [rm.Disk(o2w, 1.2, le, two_sided=True)]
    x, n, d, h = _overhead_points()
    c = Case("disk_overhead", _finish(s), lights, RHO, x, n, d, h)
    c.probes = _emitter_probes(lights, lambda o: o[1] > 0.05)
    return c


def cylinder_case():
    """A one-sided cylinder of radius 0.3 standing on the axis x = z = 0 from y = 0.3 to y = 1.4, phi_max = 200 degrees: the floor facing the gap from near by, and
    the floor under it, see only its inside and are dark."""
    s = _scene()
    add_floor(s, receiver_material(s, "const"))
    rot = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])      # object z is the world's y
    o2w, le = _rigid(rot, (0.0, 0.7, 0.0)), (9.0, 12.0, 7.0)
    s.add_cylinder(o2w.astype(np.float32), 0.3, s.matte((0.0, 0.0, 0.0)), z_min=-0.4, z_max=0.7, phi_max=200.0, emission=le)
    lights = [rm.Cylinder(o2w, 0.3, le, z_min=-0.4, z_max=0.7, phi_max=200.0)]
    # lit points from 5 radii away: nearer, half of the area samples of a cylinder face away and the rest vary so much that one point's noise uses up the case's cap
    polar = [(rad, a) for rad in (1.5, 1.7, 1.9, 2.1, 2.4, 2.7, 3.0, 3.5) for a in (10.0, 55.0, 100.0, 145.0, 190.0, 235.0, 325.0)] + [(0.6, 280.0), (0.9, 280.0), (1.2, 280.0)]
    obj = [(rad * np.cos(np.radians(a)), rad * np.sin(np.radians(a)), 0.0) for rad, a in polar]
    x = np.array([(0.0, 0.0, 0.0), (0.1, 0.0, -0.15)] + [tuple(rot @ np.array(p)) for p in obj])
    n = np.tile([0.0, 1.0, 0.0], (x.shape[0], 1))
    d, h = lean_away(x, n, (0.0, 0.0, 0.0))
    under = np.hypot(x[:, 0], x[:, 2]) < 0.3       # under the cylinder: only a flat ray gets there
    graze = np.radians(80.0)
    d[under] = np.cos(graze) * n[under] + np.sin(graze) * np.array([0.6, 0.0, 0.8])
    c = Case("cylinder", _finish(s), lights, RHO, x, n, d, h)
    c.probes = _emitter_probes(lights, lambda o: o[1] > 0.05)
    return c


def _pyramid_case(front_end="const"):
    s = _scene()
    s.receiver_mat = receiver_material(s, front_end)
    add_pyramid(s, s.receiver_mat)
    x, n = pyramid_points()
    d, h = lean_away(x, n, (0.0, -5.0, 0.0))
    return s, x, n, d, h


def point_case():
    s, x, n, d, h = _pyramid_case()
    pos, i = (1.5, 2.0, 0.7), (30.0, 40.0, 20.0)
    s.point_light(pos, i)
    return Case("point", _finish(s), [rm.Point(pos, i)], RHO, x, n, d, h)


def distant_case():
    s, x, n, d, h = _pyramid_case()
    frm, l = (2.0, 0.5, 0.6), (3.0, 4.0, 2.0)     # above the pyramid's +x and +z faces, under the horizon of the other two
    s.distant_light(frm, (0.0, 0.0, 0.0), l)
    return Case("distant", _finish(s), [rm.Distant(frm, l)], RHO, x, n, d, h)


def env_const_case():
    s, x, n, d, h = _pyramid_case()
    img = np.tile(np.float32([1.5, 2.0, 1.0]), (2, 2, 1))
    s.infinite_light(s.add_mip(img))
    return Case("env_const", _finish(s), [rm.Infinite(img)], RHO, x, n, d, h)


def env_image():
    """16 x 8: a sky that is not uniform (0.6 .. 1) and a 2 x 2 sun a thousand times brighter."""
    rng = np.random.default_rng(11)
    img = (0.6 + 0.4 * rng.random((8, 16, 3))).astype(np.float32)
    img[2:4, 5:7] *= 1000.0
    return img


SUN_L = (np.radians(67.5), np.radians(135.0))     # light-space theta, phi of the middle of the sun's four texels (rows 2-3, columns 5-6)


def env_l2w():
    th, ph = SUN_L
    sun_l = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    return _rigid(_rot_from_to(sun_l, np.array([1.0, 0.3, -0.3]), twist=0.6), (0.0, 0.0, 0.0))


def env_map_case(front_end="const"):
    """The sun of `env_image` (light-space phi = 135, theta = 67.5 degrees) is turned to (1, 0.3, -0.3): above the pyramid's +x and -z faces, in the plane of its +z
    face, under the horizon of its -x face."""
    s, x, n, d, h = _pyramid_case(front_end)
    s.matte((0.0, 0.0, 0.0))   # a second material class, as every scene with an emitter has one: a scene of one class is not binned and shades through the generic kernel
    img, l2w = env_image(), env_l2w()
    s.infinite_light(s.add_mip(img), l2w.astype(np.float32))
    return Case("env_map", _finish(s), [rm.Infinite(img, l2w)], RHO, x, n, d, h, mat=s.receiver_mat)


def three_lights_case(strategy):
    """A quad facing down at (-1.5, 2.4, 0), a sphere at (1.5, 2.4, 0) and a point light at (0, 1.2, 0.8) over the floor: no segment from the floor to one light
    passes another (both emitters lie above every ray's origin, far apart, and the point light below them)."""
    s = _scene()
    add_floor(s, receiver_material(s, "const"))
    q = [(-2.0, 2.4, -0.5), (-1.0, 2.4, -0.5), (-1.0, 2.4, 0.5), (-2.0, 2.4, 0.5)]
    s.add_mesh(q, [[0, 1, 2], [0, 2, 3]], s.matte((0.0, 0.0, 0.0)), emission=QUAD_LE)
    s.add_sphere((1.5, 2.4, 0.0), 0.4, s.matte((0.0, 0.0, 0.0)), emission=SPHERE_LE)
    s.point_light((0.0, 1.2, 0.8), (6.0, 8.0, 4.0))
    lights = [rm.quad(*q, QUAD_LE), rm.Sphere(_rigid(np.eye(3), (1.5, 2.4, 0.0)), 0.4, SPHERE_LE), rm.Point((0.0, 1.2, 0.8), (6.0, 8.0, 4.0))]
    assert rm.irradiance(lights[0], (-1.5, 0.0, 0.0), (0.0, 1.0, 0.0))[0][1] > 0     # the quad faces the floor
    x, n = floor_points((-4.0, -2.5, -1.5, -0.6, 0.0, 0.7, 1.5, 2.4, 4.0), (-2.0, -0.5, 0.0, 0.9, 3.0))
    d, h = lean_away(x, n, (0.0, 0.0, 0.0))
    return Case("three_lights_" + strategy, _finish(s, strategy), lights, RHO, x, n, d, h)


def shadow_case():
    """Two triangle lights (a 0.6 x 0.6 quad facing down at y = 2.4) over a 1.2 x 1.2 occluder at y = 1.2: the floor within |x|, |z| < 0.9 is in the umbra, beyond
    1.5 fully lit, in between partly shadowed. Rays arrive at 55 degrees and flatter: their origins stay under the occluder's height."""
    s = _scene()
    add_floor(s, receiver_material(s, "const"))
    q = [(-0.3, 2.4, -0.3), (0.3, 2.4, -0.3), (0.3, 2.4, 0.3), (-0.3, 2.4, 0.3)]
    o = [(-0.6, 1.2, -0.6), (0.6, 1.2, -0.6), (0.6, 1.2, 0.6), (-0.6, 1.2, 0.6)]
    le = (40.0, 50.0, 30.0)
    s.add_mesh(q, [[0, 1, 2], [0, 2, 3]], s.matte((0.0, 0.0, 0.0)), emission=le)
    s.add_mesh(o, [[0, 1, 2], [0, 2, 3]], s.matte((0.3, 0.3, 0.3)))
    lights = rm.quad(*q, le)
    assert rm.irradiance(lights, (3.0, 0.0, 0.0), (0.0, 1.0, 0.0))[0][1] > 0
    occ = np.array([[o[0], o[1], o[2]], [o[0], o[2], o[3]]], np.float64)
    x, n = floor_points((-3.0, -1.35, -1.1, -0.5, 0.0, 0.7, 1.0, 1.25, 1.45, 2.0, 4.0), (0.0, 0.6, 1.2, 2.5))
    d, h = lean_away(x, n, (0.0, 0.0, 0.0), polar=(55.0, 62.0, 70.0, 78.0))
    return Case("two_triangles_occluder", _finish(s), lights, RHO, x, n, d, h, occluders=occ, tol=2e-4)


CASES = {
    "quad": quad_case,
    "quad_two_sided": lambda: quad_case(two_sided=True),
    "quad_reversed": lambda: quad_case(reverse=True),
    "quad_normals": lambda: quad_case(normals=True),
    "quad_overhead": quad_overhead_case,
    "sphere_outside": sphere_outside_case,
    "sphere_inside": sphere_inside_case,
    "disk_tilted": disk_case,
    "disk_overhead": disk_overhead_case,
    "cylinder": cylinder_case,
    "point": point_case,
    "distant": distant_case,
    "env_const": env_const_case,
    "env_map": env_map_case,
    "three_lights_spatial": lambda: three_lights_case("spatial"),
    "three_lights_uniform": lambda: three_lights_case("uniform"),
    "two_triangles_occluder": shadow_case,
}
FRONT_END_CASES = {"quad": quad_case, "sphere_outside": sphere_outside_case, "env_map": env_map_case}


@lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {}
    for name_ in CASES:
        c_ = case(name_)
        out[name_ + "/M"], rel_ = compute_model_radiance(c_)
        out[name_ + "/x"], out[name_ + "/n"] = c_.x, c_.n
        print(f"{name_}: {c_.x.shape[0]} points, two resolutions differ by at most {rel_.max():.2e}")
    np.savez_compressed(GOLDEN, **out)
