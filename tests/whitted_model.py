"""A float64 model of the Whitted integrator, written from the reference's integrator/whitted.rs:41-99 and integrator/mod.rs:49-142 (specular_reflection,
specular_transmission), bsdf/mod.rs (Bsdf::f, Bsdf::sample_f's choice among matching lobes), bsdf/fresnel.rs (fr_dielectric, SpecularReflection,
SpecularTransmission with the eta^2 scaling under TransportMode::RADIANCE), material/glass.rs:73-100 (allow_multiple_lobes = false: two lobes), material/mixmat.rs,
light/point.rs (I / (4 pi r^2)), light/distant.rs, light/diffuse.rs + shapes/mesh.rs:610-634 (uniform_sample_triangle, pdf = r^2 / (|cos| area)) and
light/infinite.rs (Distribution2D over luminance * sin(theta), le). Not from the device code and not from oracle/.

  li(ray, depth):  miss -> sum of light.le(ray)                                    (nothing drawn)
                   hit  -> L = isect.le(wo)
                           for light in scene.lights: u = get_2d(); (li, wi, pdf, vis) = light.sample_li(hit, u); skip if li black or pdf == 0
                                                      f = bsdf.f(wo, wi, ALL); if f not black and vis.unoccluded: L += f li |wi . n| / pdf
                           if depth + 1 < max_depth:  L += specular_reflection + specular_transmission, each sample_f(wo, get_2d(), SPECULAR | R or T) - the draw is
                                                      taken whether or not a lobe matches - and f li(spawn_ray(wi), depth + 1) |wi . ns| / pdf where pdf > 0, f not black

The scene is the model's own: world-space triangles and spheres with a brute-force closest hit and occlusion test (`Scene`); tests mirror it into a SceneDesc. The
recursion runs over BATCHES of rays (numpy), every ray with its own draw counter, so the draws are consumed per ray exactly in the reference's depth-first order.
Sampler values: ao_model.sample_u (the k-th get_2d() after the camera sample).

Per sample it returns L, the number of li invocations, the number of draws, and three MARGINS that say how far the sample's tree is from a decision float32 could take
differently: `edge` - the smallest distance between any li ray (up to its hit) and a boundary edge of a surface or the silhouette of a sphere; `shadow` - the same for
every visibility segment (the emitter's own outline excepted: a segment ends before it); `sin2` - the smallest |1 - sin^2(theta_t)| of any refraction (total internal
reflection is decided there). A test compares every sample only where these are large (tests/test_whitted_cpu.py)."""
import numpy as np

import ao_model

F = np.float32
INF = np.inf
T_EPS = 1e-7  # spawn_ray: a ray leaves the surface it starts on


# ------------------------------------------------------------------------------------------------ scene
class Scene:
    """Triangles (p0, p1, p2, material, surface id, emission), spheres (centre, radius, material) and lights. A material is ("matte", kd), ("mirror", kr),
    ("glass", kr, kt, eta) or ("mix", m1, m2, amount) with m1, m2 of those. A light is ("point", pos, I), ("distant", w_light (towards the light), L),
    ("tri", triangle index) - one per emitting triangle, in triangle order, as the reference lists them - or ("infinite", L, rows): a constant map of `rows` rows."""

    def __init__(self):
        self.tris, self.spheres, self.lights = [], [], []
        self._surf = 0

    def add_tri(self, p0, p1, p2, mat, surf=None, emission=None):
        if surf is None:
            surf = self._new_surface()
        self.tris.append((np.float64(p0), np.float64(p1), np.float64(p2), mat, surf, None if emission is None else np.float64(emission)))
        if emission is not None:
            self.lights.append(("tri", len(self.tris) - 1))
        return len(self.tris) - 1

    def _new_surface(self):
        self._surf += 1
        return self._surf

    def add_quad(self, p0, p1, p2, p3, mat, emission=None):
        """Two triangles (p0 p1 p2), (p0 p2 p3) of one surface: their shared diagonal is no boundary."""
        s = self._new_surface()
        self.add_tri(p0, p1, p2, mat, s, emission)
        self.add_tri(p0, p2, p3, mat, s, emission)

    def add_sphere(self, c, r, mat):
        self.spheres.append((np.float64(c), float(r), mat))

    def boundary_edges(self):
        """[(a, b, surface)]: the triangle edges that no second triangle of the same surface shares."""
        seen = {}
        for p0, p1, p2, _, s, _ in self.tris:
            for a, b in ((p0, p1), (p1, p2), (p2, p0)):
                key = (s,) + tuple(sorted([tuple(np.round(a, 9)), tuple(np.round(b, 9))]))
                seen.setdefault(key, []).append((a, b, s))
        return [v[0] for v in seen.values() if len(v) == 1]


def _norm(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dot(a, b):
    return (a * b).sum(-1)


def intersect(sc, o, d, t_max=None):
    """Closest hit of rays o + t d, t in (T_EPS, t_max): (t, kind, index, n) with kind 0 miss / 1 triangle / 2 sphere; n the geometric (= shading) normal
    (p0 - p2) x (p1 - p2) of a triangle, the outward normal of a sphere."""
    nr = o.shape[0]
    best = np.full(nr, INF) if t_max is None else np.array(t_max, np.float64, copy=True)
    kind, index, nrm = np.zeros(nr, int), np.full(nr, -1), np.zeros((nr, 3))
    for k, (p0, p1, p2, _, _, _) in enumerate(sc.tris):
        e1, e2 = p1 - p0, p2 - p0
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o - p0
            b1 = _dot(tv, pv) * inv
            qv = np.cross(tv, e1)
            b2 = _dot(d, qv) * inv
            t = (qv @ e2) * inv
            ok = (np.abs(det) > 0) & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1) & (t > T_EPS) & (t < best)
        n = _norm(np.cross(p0 - p2, p1 - p2))
        best, kind, index = np.where(ok, t, best), np.where(ok, 1, kind), np.where(ok, k, index)
        nrm = np.where(ok[:, None], n, nrm)
    for k, (c, r, _) in enumerate(sc.spheres):
        oc = o - c
        a, b = _dot(d, d), 2.0 * _dot(d, oc)
        disc = b * b - 4 * a * (_dot(oc, oc) - r * r)
        sq = np.sqrt(np.maximum(disc, 0.0))
        t0, t1 = (-b - sq) / (2 * a), (-b + sq) / (2 * a)
        t = np.where(t0 > T_EPS, t0, t1)
        ok = (disc >= 0) & (t > T_EPS) & (t < best)
        n = (oc + t[:, None] * d) / r
        best, kind, index = np.where(ok, t, best), np.where(ok, 2, kind), np.where(ok, k, index)
        nrm = np.where(ok[:, None], n, nrm)
    return best, kind, index, nrm


# ------------------------------------------------------------------------------------------------ margins
def _seg_seg(p, u, q, v):
    """Smallest distance between the segments p + s u, q + t v, s, t in [0, 1]; p, u: (n, 3), q, v: (3,)."""
    w = p - q
    a, b, c, dd, e = _dot(u, u), u @ v, float(v @ v), _dot(u, w), w @ v
    den = a * c - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.clip(np.where(den > 1e-300, (b * e - c * dd) / den, 0.0), 0.0, 1.0)
    t = np.clip((b * s + e) / c, 0.0, 1.0)
    s = np.clip(np.where(a > 0, (b * t - dd) / np.where(a > 0, a, 1.0), 0.0), 0.0, 1.0)
    t = np.clip((b * s + e) / c, 0.0, 1.0)
    return np.linalg.norm(w + s[:, None] * u - t[:, None] * v, axis=1)


def clearance(sc, o, d, t, skip_surface=None, own_sphere=None, hit_sphere=None, far=50.0):
    """How far the segments o + s d, s in [0, t] (t = inf: `far` scene units) stay from every boundary edge and every sphere's silhouette: (n,). skip_surface (n,): a
    surface whose edges do not count (the emitter a segment ends short of). own_sphere (n,): the sphere a segment starts on - its silhouette is met at the start; what
    counts there is how far the direction is from tangent, r |d . n| / |d|. hit_sphere (n,): the sphere a segment ends on - what counts is how far the whole half-line
    passes from its outline, | distance to the centre - r |, not the end point, which lies on it."""
    length = np.where(np.isfinite(t), t, far / np.maximum(np.linalg.norm(d, axis=1), 1e-300))
    u = d * length[:, None]
    m = np.full(o.shape[0], INF)
    for a, b, s in sc.boundary_edges():
        dist = _seg_seg(o, u, a, b - a)
        if skip_surface is not None:
            dist = np.where(skip_surface == s, INF, dist)
        m = np.minimum(m, dist)
    for k, (c, r, _) in enumerate(sc.spheres):
        uu = _dot(u, u)
        s = _dot(c - o, u) / np.where(uu > 0, uu, 1.0)
        s = np.clip(s, 0.0, np.where(hit_sphere == k, INF, 1.0) if hit_sphere is not None else 1.0)
        dist = np.abs(np.linalg.norm(o + s[:, None] * u - c, axis=1) - r)
        if own_sphere is not None:
            own = own_sphere == k
            n = (o - c) / r
            dist = np.where(own, r * np.abs(_dot(_norm(d), n)), dist)
        m = np.minimum(m, dist)
    return m


# ------------------------------------------------------------------------------------------------ BSDF
def fr_dielectric(cos_i, eta_i, eta_t):
    """fresnel.rs:33-58: the unpolarised Fresnel reflectance of a dielectric interface; 1 under total internal reflection. The lobes reach it through
    FresnelDielectric::evaluate, which passes |cos| (fresnel.rs:125): seen from inside the glass the interface is evaluated as (1, eta) too - the reference's, restated."""
    cos_i = np.clip(cos_i, -1.0, 1.0)
    ent = cos_i > 0
    ei, et = np.where(ent, eta_i, eta_t), np.where(ent, eta_t, eta_i)
    ci = np.abs(cos_i)
    sin_t = ei / et * np.sqrt(np.maximum(0.0, 1.0 - ci * ci))
    ct = np.sqrt(np.maximum(0.0, 1.0 - sin_t * sin_t))
    with np.errstate(divide="ignore", invalid="ignore"):
        rl = (et * ci - ei * ct) / (et * ci + ei * ct)
        rp = (ei * ci - et * ct) / (ei * ci + et * ct)
    return np.where(sin_t >= 1.0, 1.0, (rl * rl + rp * rp) / 2.0)


def lobes(mat, scale=1.0):
    """[(kind, colour (3,), eta, scale)] of compute_scattering_functions(allow_multiple_lobes = false): kind "diffuse", "spec_r" (eta 0: no Fresnel), "spec_t"."""
    k = mat[0]
    if k == "matte":
        return [("diffuse", np.float64(mat[1]) * np.ones(3), 0.0, scale)] if np.any(np.float64(mat[1]) != 0) else []
    if k == "mirror":
        return [("spec_r", np.float64(mat[1]) * np.ones(3), 0.0, scale)] if np.any(np.float64(mat[1]) != 0) else []
    if k == "glass":
        kr, kt, eta = np.float64(mat[1]) * np.ones(3), np.float64(mat[2]) * np.ones(3), float(mat[3])
        out = []
        if np.any(kr != 0):
            out.append(("spec_r", kr, eta, scale))
        if np.any(kt != 0):
            out.append(("spec_t", kt, eta, scale))
        return out
    if k == "mix":  # mixmat.rs:34-64: m1's lobes scaled by amount, m2's by 1 - amount
        return lobes(mat[1], scale * float(mat[3])) + lobes(mat[2], scale * (1.0 - float(mat[3])))
    raise ValueError(k)


def bsdf_f(lb, wo, wi, n):
    """Bsdf::f(wo, wi, ALL) (bsdf/mod.rs:94-111): the specular lobes' f is black; a Lambertian reflection counts where wi and wo lie on one side of the surface."""
    f = np.zeros(wo.shape)
    refl = _dot(wi, n) * _dot(wo, n) > 0
    for kind, col, _, sc_ in lb:
        if kind == "diffuse":
            f = f + np.where(refl[:, None], col * sc_ / np.pi, 0.0)
    return np.where((_dot(wo, n) == 0)[:, None], 0.0, f)


def sample_specular(lb, want, wo, n, u, signed_fresnel=False):
    """Bsdf::sample_f(wo, u, SPECULAR | want) (bsdf/mod.rs:138-251) at normal n: (weight f |wi . n| / pdf (n, 3), wi (n, 3), valid (n,), |1 - sin^2 theta_t| (n,)).
    Among m matching lobes u[0] picks floor(u[0] m) and the pdf is 1 / m. signed_fresnel: evaluate the interface with the cosine's sign (the physical reflectance, under
    which a vertex conserves energy) instead of the reference's |cos| - for the model's own tests."""
    cosine = (lambda c: c) if signed_fresnel else np.abs
    match = [l for l in lb if l[0] == want]
    nr = wo.shape[0]
    weight, wi, valid, gap = np.zeros((nr, 3)), np.zeros((nr, 3)), np.zeros(nr, bool), np.full(nr, INF)
    m = len(match)
    if m == 0:
        return weight, wi, valid, gap
    comp = np.minimum(np.floor(np.asarray(u[:, 0], np.float64) * m).astype(int), m - 1)
    cos_o = _dot(wo, n)
    for j, (kind, col, eta, sc_) in enumerate(match):
        sel = (comp == j) & (cos_o != 0)
        if kind == "spec_r":  # wi = (-wo.x, -wo.y, wo.z) in the shading frame; f = Fr R / |cos|, pdf 1
            w = -wo + 2.0 * cos_o[:, None] * n
            fr = fr_dielectric(cosine(_dot(w, n)), 1.0, eta) if eta != 0.0 else np.ones(nr)  # FresnelDielectric::evaluate takes |cos| (fresnel.rs:125): (1, eta) from either side
            wt, ok, g = (fr[:, None] * col) * sc_ * m, sel, np.full(nr, INF)
        else:
            ent = cos_o > 0
            ei, et = np.where(ent, 1.0, eta), np.where(ent, eta, 1.0)
            nn = np.where(ent[:, None], n, -n)  # face_forward((0, 0, 1), wo)
            r = ei / et
            ci = _dot(nn, wo)
            sin2t = r * r * np.maximum(0.0, 1.0 - ci * ci)
            ct = np.sqrt(np.maximum(0.0, 1.0 - sin2t))
            w = -wo * r[:, None] + (r * ci - ct)[:, None] * nn  # refract (geometry.rs)
            ft = (1.0 - fr_dielectric(cosine(_dot(w, n)), 1.0, eta))[:, None] * col * (ei * ei / (et * et))[:, None]
            wt, ok, g = ft * sc_ * m, sel & (sin2t < 1.0), np.where(sel, np.abs(1.0 - sin2t), INF)
        ok = ok & np.any(wt != 0, axis=1) & (_dot(w, n) != 0)
        weight, wi, valid = np.where(ok[:, None], wt, weight), np.where(ok[:, None], w, wi), valid | ok
        gap = np.minimum(gap, g)
    return weight, wi, valid, gap


# ------------------------------------------------------------------------------------------------ lights
def infinite_sample(rows, u):
    """InfiniteAreaLight::sample_li over a CONSTANT map of `rows` rows (infinite.rs:60-100, 143-181; distribution2d.rs): the conditional rows are uniform, the marginal is
    piecewise constant with weights sin(pi (v + 0.5) / rows). Returns (wi in light space = world space (n, 3), pdf (n,))."""
    func = np.sin(np.pi * (np.arange(rows) + 0.5) / rows)
    cdf = np.concatenate([[0.0], np.cumsum(func) / rows])
    func_int = cdf[-1]
    cdf = cdf / func_int
    u0, u1 = np.asarray(u[:, 0], np.float64), np.asarray(u[:, 1], np.float64)
    off = np.clip(np.searchsorted(cdf, u1, side="right") - 1, 0, rows - 1)
    du = (u1 - cdf[off]) / (cdf[off + 1] - cdf[off])
    d1, pdf1 = (off + du) / rows, func[off] / func_int
    theta, phi = d1 * np.pi, u0 * 2.0 * np.pi
    wi = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1)
    with np.errstate(divide="ignore"):
        pdf = np.where(np.sin(theta) == 0, 0.0, pdf1 / (2.0 * np.pi * np.pi * np.sin(theta)))
    return wi, pdf


def sample_light(sc, light, p, u, world_radius=1e3):
    """Light::sample_li(hit, u): (li (n, 3), wi (n, 3), pdf (n,), distance to the sampled point (n,), the emitter's surface id or -1)."""
    nr = p.shape[0]
    if light[0] == "point":
        v = np.float64(light[1]) - p
        r2 = _dot(v, v)
        return np.float64(light[2]) / (4.0 * np.pi * r2)[:, None], _norm(v), np.ones(nr), np.sqrt(r2), -1
    if light[0] == "distant":
        w = _norm(np.float64(light[1]))
        return np.broadcast_to(np.float64(light[2]), (nr, 3)), np.broadcast_to(w, (nr, 3)), np.ones(nr), np.full(nr, 2.0 * world_radius), -1
    if light[0] == "infinite":
        wi, pdf = infinite_sample(light[2], u)
        return np.broadcast_to(np.float64(light[1]), (nr, 3)), wi, pdf, np.full(nr, 2.0 * world_radius), -1
    p0, p1, p2, _, surf, em = sc.tris[light[1]]
    su0 = np.sqrt(np.asarray(u[:, 0], np.float64))  # uniform_sample_triangle
    b0, b1 = 1.0 - su0, np.asarray(u[:, 1], np.float64) * su0
    q = b0[:, None] * p0 + b1[:, None] * p1 + (1.0 - b0 - b1)[:, None] * p2
    n = _norm(np.cross(p0 - p2, p1 - p2))
    area = 0.5 * np.linalg.norm(np.cross(p1 - p0, p2 - p0))
    v = q - p
    r2 = _dot(v, v)
    wi = _norm(v)
    cos_l = _dot(n, -wi)
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = np.where((r2 == 0) | (cos_l == 0), 0.0, r2 / (np.abs(cos_l) * area))
    li = np.where((cos_l > 0)[:, None], em, 0.0)  # one-sided (diffuse.rs:91-97)
    return li, wi, pdf, np.sqrt(r2), surf


# ------------------------------------------------------------------------------------------------ the integrator
class Result:
    def __init__(self, n):
        self.L = np.zeros((n, 3))
        self.nodes = np.zeros(n, np.int64)
        self.draws = np.zeros(n, np.int64)
        self.edge = np.full(n, INF)
        self.shadow = np.full(n, INF)
        self.sin2 = np.full(n, INF)


def _material(sc, kind, index):
    return sc.tris[index][3] if kind == 1 else sc.spheres[index][2]


def _li(sc, res, ids, o, d, depth, max_depth, U, beta, own=None):
    """Whitted::li for the rays `ids` of the batch (their own draw counters in res.draws); adds beta * L into res.L. own (n,): the sphere each ray starts on, or -1."""
    if ids.size == 0:
        return
    res.nodes[ids] += 1
    t, kind, index, n = intersect(sc, o, d)
    res.edge[ids] = np.minimum(res.edge[ids], clearance(sc, o, d, t, own_sphere=own, hit_sphere=np.where(kind == 2, index, -1)))
    miss = kind == 0
    for light in sc.lights:  # the sum of light.le(ray): an infinite light's alone
        if light[0] == "infinite":
            res.L[ids[miss]] += beta[miss] * np.float64(light[1])
    groups = {}
    for j in np.nonzero(~miss)[0]:
        groups.setdefault((int(kind[j]), int(index[j])), []).append(j)
    for (kd, ix), js in groups.items():  # the rays of one primitive share its material
        js = np.array(js)
        g, p, nn, wo, b = ids[js], o[js] + t[js, None] * d[js], n[js], -_norm(d[js]), beta[js]
        lb = lobes(_material(sc, kd, ix))
        if kd == 1 and sc.tris[ix][5] is not None:  # isect.le(wo): one-sided
            res.L[g] += b * np.where((_dot(nn, wo) > 0)[:, None], sc.tris[ix][5], 0.0)
        own_sphere = np.full(js.size, ix if kd == 2 else -1)
        for light in sc.lights:
            u = U[g, res.draws[g]]
            res.draws[g] += 1
            li, wi, pdf, dist, surf = sample_light(sc, light, p, u)
            f = bsdf_f(lb, wo, wi, nn)
            live = np.any(li != 0, axis=1) & (pdf != 0) & np.any(f != 0, axis=1)
            if not live.any():
                continue
            side = np.where((_dot(wi, nn) > 0)[:, None], nn, -nn)  # spawn_ray: off the surface on wi's side
            so = p + side * T_EPS
            tt, hk, _, _ = intersect(sc, so[live], wi[live], t_max=np.maximum(dist[live] * (1.0 - 1e-6) - T_EPS, 0.0))
            clear = hk == 0
            res.shadow[g[live]] = np.minimum(res.shadow[g[live]], clearance(sc, p[live], wi[live], np.minimum(dist[live], 50.0), skip_surface=np.full(int(live.sum()), surf), own_sphere=own_sphere[live]))
            with np.errstate(divide="ignore", invalid="ignore"):
                term = f[live] * li[live] * np.abs(_dot(wi[live], nn[live]))[:, None] / pdf[live][:, None]
            res.L[g[live][clear]] += b[live][clear] * term[clear]
        if depth + 1 < max_depth:
            for want in ("spec_r", "spec_t"):
                u = U[g, res.draws[g]]
                res.draws[g] += 1
                weight, wi, valid, gap = sample_specular(lb, want, wo, nn, u)
                res.sin2[g] = np.minimum(res.sin2[g], gap)
                v = np.nonzero(valid)[0]
                side = np.where((_dot(wi[v], nn[v]) > 0)[:, None], nn[v], -nn[v])
                _li(sc, res, g[v], p[v] + side * T_EPS, wi[v], depth + 1, max_depth, U, b[v] * weight[v], own_sphere[v])


def render(sc, o, d, max_depth, U, active=None):
    """Whitted::li(ray, 0) for the rays o, d (n, 3) with the draws U (n, K, 2) (ao_model.sample_u per ray): a Result. active (n,) bool: the rays that are traced."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    res = Result(o.shape[0])
    ids = np.arange(o.shape[0]) if active is None else np.nonzero(active)[0]
    _li(sc, res, ids, o[ids], d[ids], 0, max_depth, U, np.ones((ids.size, 3)))
    return res


def draws_for(orc, spp, dims, width, height, ns, sample0, n_draws):
    """U (height * width * ns, n_draws, 2) float32: the get_2d() values after the camera sample of every ray of an (H, W, ns) batch over its virtual film."""
    U = np.zeros((height, width, ns, n_draws, 2), F)
    for y in range(height):
        for x in range(width):
            for sl in range(ns):
                U[y, x, sl] = ao_model.sample_u(orc, spp, dims, y * width + x, sample0 + sl, n_draws)
    return U.reshape(-1, n_draws, 2)
