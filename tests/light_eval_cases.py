"""What tests/test_light_eval_cpu.py and tests/test_gpu_light_eval.py share: the sample design of the unbiasedness check of rt_light_eval, a float64 stand-in
for the device's light sampling, and the list of points the GPU test judges.

Design: per point and light B = 256 independent blocks, each an 8 x 8 jittered grid of u_light, N = 16 384; the statistic is radiometry_model.statistic over the
BLOCK MEANS, shape (P, 256). Its caps are conditions on the samples (pooled se <= 0.002 sum M, se_p <= 0.03 M_p), so whether a point can be judged at this N is
decided here, without the device: the stand-in maps the same u_light onto each emitter the way the reference's sampling does - uniformly by area through the
model's own `point` parametrisation (triangle, disk, cylinder, a sphere seen from inside), uniformly in the cone a sphere subtends seen from outside - and
evaluates the model's integrand, numpy and tests/radiometry_model.py only. A lit point is kept when the stand-in's se_p is at most KEEP x 0.03 M_p: the
standard error of a standard deviation estimated from 256 block means is 1 / sqrt(2 x 255) = 4.4 % of it, so KEEP = 2 / 3 leaves a point that is kept more than
seven of those deviations inside the cap on any other draw of the jitter. At least three quarters of a case's lit points must remain (the CPU test asserts it)."""
import os
from functools import lru_cache

import numpy as np

import radiometry_cases as rc
import radiometry_model as rm

BLOCKS, GRID = 256, 8
CELLS = GRID * GRID
N = BLOCKS * CELLS
KEEP = 2.0 / 3.0
ILL_COS = 0.01          # |n_y . w| below this: the pdf identity r^2 / (|n_y . w| A) is ill-conditioned in float32
ILL_SHARE = 0.02

# the area-light cases of the unbiasedness check -> (case, occluded?). The receivers "instance" and "disk" put other trace kernels behind the segments.
AREA_CASES = ("quad", "quad_overhead", "sphere_outside", "sphere_inside", "disk_tilted", "disk_overhead", "cylinder", "two_triangles_occluder",
              "quad_on_instance", "quad_on_disk")


@lru_cache(maxsize=None)
def case(name):
    if name == "quad_on_instance":
        return rc.quad_case(receiver="instance")
    if name == "quad_on_disk":
        return rc.quad_case(receiver="disk")
    return rc.case(name)


def flat_lights(c):
    return rc._flat(c.lights)


@lru_cache(maxsize=None)
def design(points, seed=2024):
    """u_light (points, BLOCKS, CELLS, 2) float32 in [0, 1): every block an independent jittered GRID x GRID set."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(GRID), np.arange(GRID), indexing="ij")
    jit = rng.random((points, BLOCKS, CELLS, 2))
    u = np.stack([(gx.reshape(-1) + jit[..., 0]) / GRID, (gy.reshape(-1) + jit[..., 1]) / GRID], axis=-1)
    u = np.minimum(u, 1.0 - 2.0 ** -24).astype(np.float32)
    u.setflags(write=False)
    return u


def area_of(l):
    if isinstance(l, rm.Triangle):
        return 0.5 * l.area2
    if isinstance(l, rm.Sphere):
        return 4.0 * np.pi * l.radius ** 2
    if isinstance(l, rm.Disk):
        return np.pi * l.radius ** 2
    if isinstance(l, rm.Cylinder):
        return l.radius * (l.z[1] - l.z[0]) * l.phi_max
    raise TypeError(l)


def sphere_outside(l, x):
    return isinstance(l, rm.Sphere) and np.linalg.norm(np.asarray(x, np.float64) - l.shift) > l.radius


def standin(l, x, n, u, occluders=None):
    """Per sample of u (..., 2) at the point x with normal n: (the estimator of E, green channel, in float64; |n_y . w| of the sample; its distance r; whether it
    emits toward x)."""
    u1, u2 = np.float64(u[..., 0]), np.float64(u[..., 1])
    if sphere_outside(l, x):       # uniform in the cone the sphere subtends (Sphere::sample_si, sphere.rs:267-299): pdf = 1 / (2 pi (1 - cos theta_max))
        a = l.shift - x
        d = np.linalg.norm(a)
        a = a / d
        t1, t2 = rc._tangent_frame(a)
        cos_max = np.sqrt(max(0.0, 1.0 - (l.radius / d) ** 2))
        ct = (1.0 - u1) + u1 * cos_max
        st_, ph = np.sqrt(np.maximum(0.0, 1.0 - ct * ct)), 2.0 * np.pi * u2
        w = (st_ * np.cos(ph))[..., None] * t1 + (st_ * np.sin(ph))[..., None] * t2 + ct[..., None] * a
        est = l.le[1] * np.maximum((w * n).sum(-1), 0.0) * 2.0 * np.pi * (1.0 - cos_max)
        if occluders is not None and len(occluders):
            est = np.where(rm._blocked(np.broadcast_to(x, w.shape), w, np.full(w.shape[:-1], d), occluders), 0.0, est)
        return est, np.ones_like(est), np.full(est.shape, d), np.ones(est.shape, bool)
    point, _ = l.param(x)
    if isinstance(l, rm.Triangle):        # uniform by area over (b1, b2) = (pu, pv (1 - pu)): the density of pu is 2 (1 - pu)
        pu, pv = 1.0 - np.sqrt(1.0 - u1), u2
    elif isinstance(l, rm.Disk):
        pu, pv = l.radius * np.sqrt(u1), 2.0 * np.pi * u2
    elif isinstance(l, rm.Cylinder):
        pu, pv = l.z[0] + u1 * (l.z[1] - l.z[0]), u2 * l.phi_max
    else:                                  # a sphere seen from inside: uniform over the whole sphere (sphere.rs:246-266)
        pu, pv = np.arccos(np.clip(1.0 - 2.0 * u1, -1.0, 1.0)), 2.0 * np.pi * u2
    y, ny, _ = point(pu, pv)
    w = y - x
    r2 = (w * w).sum(-1)
    r = np.sqrt(r2)
    w = w / r[..., None]
    cos_y = -(ny * w).sum(-1)
    emit = np.abs(cos_y) if l.two_sided else np.maximum(cos_y, 0.0)
    est = l.le[1] * np.maximum((w * n).sum(-1), 0.0) * emit / r2 * area_of(l)
    if occluders is not None and len(occluders):
        est = np.where(rm._blocked(np.broadcast_to(x, w.shape), w, r, occluders), 0.0, est)
    return est, np.abs(cos_y), r, emit > 0


@lru_cache(maxsize=None)
def model_e(name, k):
    """E (P, 3) of light k of the case alone, without occluders, from the float64 model."""
    c = case(name)
    l = flat_lights(c)[k]
    e = np.array([rm.irradiance(l, x, n, None, tol=c.tol)[0] for x, n in zip(c.x, c.n)])
    e.setflags(write=False)
    return e


def occluded_model(name):
    """rho / pi * E (P, 3) of ALL lights of an occluded case: the golden values of radiometry_cases."""
    return rc.model_radiance(case(name))


@lru_cache(maxsize=None)
def standin_blocks(name, k, occluded=False):
    """(block means (P, BLOCKS) of the stand-in for light k, the share of ill-conditioned samples per point (P,))."""
    c = case(name)
    l = flat_lights(c)[k]
    u = design(c.x.shape[0])
    bm, ill = np.zeros((c.x.shape[0], BLOCKS)), np.zeros(c.x.shape[0])
    for p, (x, n) in enumerate(zip(c.x, c.n)):
        est, cy, _, _ = standin(l, x, n, u[p], c.occluders if occluded else None)
        bm[p], ill[p] = est.mean(axis=-1), float((cy < ILL_COS).mean())
    return bm, ill


# ------------------------------------------------------------------------------------------------ where pdf_li(sample's wi) is asked to equal the sample's pdf to 1e-4
# Decided in float64 from the sample itself - its distance r and its cosine c = |n_y . w| - never from what the device returns for it.
#   every emitter: c >= ILL_COS, the line the issue draws for the density's own definition (a float32 dot product of unit vectors is good to 2e-7 absolute).
#   a curved emitter that Shape::pdf_wi re-intersects (the cylinder, a sphere from inside): the root of the float32 quadric - about thirty operations on quantities of
#   the size of r^2 - leaves the hit point off by e <= CURVED_OPS x 2^-24 r across the ray; at the cosine c the ray meets the surface e / c further along it, where
#   the normal has turned by e / (c R), R the radius of curvature: a relative change of c, and so of the density, of e / (R c^2). The identity is asked where that is
#   at most 1e-4.
# The share of the emitting samples that this leaves out is capped per kind of emitter (IDENTITY_CAP); tests/test_light_eval_cpu.py holds the float64 stand-in to the
# caps without a device, tests/test_gpu_light_eval.py the device's samples.
CURVED_OPS = 32.0
# flat emitters and the cone: the issue's share of ill-conditioned samples. Curved: the stand-in leaves out 27.3 % of the cylinder's emitting samples (the case's
# points stand 5 - 12 radii away, where the term passes 1e-4 below c = 0.3 - 0.5) and none of the sphere's from inside; rounded up to the next 5 %.
IDENTITY_CAP = dict(flat=ILL_SHARE, curved=0.30)


def curved(l, x):
    return isinstance(l, rm.Cylinder) or (isinstance(l, rm.Sphere) and not sphere_outside(l, x))


def curved_term(l, r, c):
    """e / (R c^2) with e = CURVED_OPS x 2^-24 r."""
    return CURVED_OPS * 2.0 ** -24 * r / l.radius / np.maximum(c * c, 1e-30)


def identity_subset(l, x, r, c):
    """Boolean mask over samples (distance r, cosine c = |n_y . w|, float64): the pdf_li identity is asked at 1e-4 there."""
    ok = c >= ILL_COS
    return ok & (curved_term(l, r, c) <= 1e-4) if curved(l, x) else ok


@lru_cache(maxsize=None)
def standin_identity_share(name, k):
    """The share of the stand-in's emitting samples that identity_subset leaves out, over the points of the case that are not in the emitter's plane."""
    c = case(name)
    l = flat_lights(c)[k]
    u = design(c.x.shape[0])
    out = tot = 0
    for p, (x, n) in enumerate(zip(c.x, c.n)):
        if c.extra is not None and c.extra[p] > 0:
            continue
        _, cy, r, emits = standin(l, x, n, u[p])
        out, tot = out + int((emits & ~identity_subset(l, x, r, cy)).sum()), tot + int(emits.sum())
    return out / max(1, tot)


# ------------------------------------------------------------------------------------------------ the occluded model, per light
OCCLUDED_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "light_eval_occluded.npz")


def compute_occluded_e(name, k, points=None):
    """E (P, 3) of light k alone WITH the case's occluders from the float64 model (the quadrature of an occluder's outline: a third of a second per point)."""
    c = case(name)
    l = flat_lights(c)[k]
    idx = range(c.x.shape[0]) if points is None else points
    return np.array([rm.irradiance(l, c.x[p], c.n[p], c.occluders, tol=c.tol)[0] for p in idx])


@lru_cache(maxsize=None)
def occluded_e(name, k):
    """The same from tests/golden/light_eval_occluded.npz (`python tests/light_eval_cases.py` writes it; tests/test_light_eval_cpu.py recomputes a sample of its points
    and holds the sum over the lights to radiometry_cases' golden values), which must hold the case with these very points and normals."""
    c = case(name)
    with np.load(OCCLUDED_GOLDEN) as g:
        assert np.array_equal(g[name + "/x"], c.x) and np.array_equal(g[name + "/n"], c.n), "tests/golden/light_eval_occluded.npz is stale: rewrite it"
        e = g[f"{name}/E{k}"].copy()
    e.setflags(write=False)
    return e


@lru_cache(maxsize=None)
def judged(name, k):
    """The points of light k of the case that the GPU test judges, as a boolean mask (P,): every dark point of the model (it must be 0.0 in every query) and every
    lit point whose stand-in noise is at most KEEP of the per-point cap."""
    m = model_e(name, k)[:, 1]
    bm, _ = standin_blocks(name, k)
    se = bm.std(axis=1, ddof=1) / np.sqrt(BLOCKS)
    return (m == 0) | (se <= KEEP * rm.CAP_POINT * m)


@lru_cache(maxsize=None)
def judged_occluded_light(name, k):
    """The same for light k with the case's occluders, against the occluded model of that light."""
    m = occluded_e(name, k)[:, 1]
    bm, _ = standin_blocks(name, k, True)
    se = bm.std(axis=1, ddof=1) / np.sqrt(BLOCKS)
    return (m == 0) | (se <= KEEP * rm.CAP_POINT * m)


@lru_cache(maxsize=None)
def judged_occluded(name):
    """The same for the sum over the lights of an occluded case, against the occluded model."""
    c = case(name)
    m = occluded_model(name)[:, 1] * np.pi / c.rho
    bm = sum(standin_blocks(name, k, True)[0] for k in range(len(flat_lights(c))))
    se = bm.std(axis=1, ddof=1) / np.sqrt(BLOCKS)
    return (m == 0) | (se <= KEEP * rm.CAP_POINT * m)


if __name__ == "__main__":
    out_ = {}
    for name_ in AREA_CASES:
        c_ = case(name_)
        if c_.occluders is None:
            continue
        out_[name_ + "/x"], out_[name_ + "/n"] = c_.x, c_.n
        for k_ in range(len(flat_lights(c_))):
            out_[f"{name_}/E{k_}"] = compute_occluded_e(name_, k_)
            print(f"{name_} light {k_}: {int((out_[f'{name_}/E{k_}'][:, 1] > 0).sum())} of {c_.x.shape[0]} points lit")
    np.savez_compressed(OCCLUDED_GOLDEN, **out_)
