"""A float64 model of the direct-lighting integrator, written from the reference's integrator/directlighting.rs:89-143 (li), integrator/mod.rs:145-318
(uniform_sample_all_light, uniform_sample_one_light, estimate_direct), sampling/mod.rs (cosine_sample_hemisphere, concentric_sample_disk, power_heuristic), bsdf/mod.rs
(Bsdf::pdf, Bsdf::sample_f's lobe choice and u remap under ALL & !SPECULAR), bsdf/lambertian.rs, shapes/mod.rs:59-68 + shapes/mesh.rs (Shape::pdf_wi of a triangle, the
shading frame of a triangle without uvs: ss = -normalize(p1 - p0) after mesh.rs:402-406 re-orthogonalises it), light/infinite.rs:183-196 (pdf_li), and, for the sampler's arrays,
sampler/zerotwosequence.rs:67-180, sampler/lowdiscrepancy.rs (sobol_2d, van_der_corput, gray_code_sample, shuffle) and rng.rs:32-40 (the bounded draw's retry). Not from the
device code and not from oracle/. Scene, intersection, lights, specular lobes and the margin code are tests/whitted_model.py's.

  li(ray, depth):  miss -> sum of light.le(ray)
                   hit  -> L = isect.le(wo)
                           if lights: "all": for light j: (u_light, u_scattering) = the sample's next two arrays, or two get_2d() once they are exhausted; L += estimate_direct
                                      "one": s = get_1d(); j = min(n - 1, floor(s n)); u_light = get_2d(); u_scattering = get_2d(); L += n estimate_direct
                           if depth + 1 < max_depth: specular_reflection + specular_transmission as Whitted takes them

Per sample it returns L, the four info words (li invocations, get_2d() draws, get_1d() draws, vertices that reached uniform_sample_all_light), the visibility segments and
probe rays cast, and the margins: Whitted's `edge` - now also over every probe ray up to its hit and, toward a triangle light, over the probe's whole half-line against that
triangle's three edges (pdf_li and the probe's hit decide on them) -, `shadow` and `sin2`; `grazing`, the smallest |cos| at an emitter of any live light sample, pdf_li hit or
probe hit; `pick`, under "one" the distance of s n from an integer."""
import numpy as np

import whitted_model as wm
from whitted_model import INF, T_EPS, _dot, _norm

F = np.float32
ONE_MINUS_EPS = F(np.nextafter(F(1.0), F(0.0)))
ALL, ONE = 0, 1
# switches for the model's own tests (test_direct_cpu.py): one half of estimate_direct alone, the weights forced to 1
LIGHT_HALF, BSDF_HALF, MIS = True, True, True


# ------------------------------------------------------------------------------------------------ the sampler's tables, replayed
def _sobol_columns():
    c0 = [1 << (31 - j) for j in range(32)]
    c1 = [0x80000000]
    for _ in range(31):
        c1.append(c1[-1] ^ (c1[-1] >> 1))
    assert c1[:8] == [0x80000000, 0xc0000000, 0xa0000000, 0xf0000000, 0x88000000, 0xcc000000, 0xaa000000, 0xff000000] and c1[16] == 0x80008000  # lowdiscrepancy.rs:167-173
    return np.array(c0, np.uint32), np.array(c1, np.uint32)


C0, C1 = _sobol_columns()


def _unit(v):
    return np.minimum(v.astype(F) * F(2.3283064365386963e-10), ONE_MINUS_EPS)


class _Stream:
    """The raw u32 draws of many pixels' streams, walked in lockstep: every pixel has its own position, so a retried bounded draw shifts that pixel alone."""

    def __init__(self, orc, pixel_indices, n):
        self.raw = np.stack([orc.rng_stream(int(p), n)[0] for p in pixel_indices])
        self.rows = np.arange(len(pixel_indices))
        self.pos = np.zeros(len(pixel_indices), np.int64)
        self.retries = 0

    def u32(self):
        v = self.raw[self.rows, self.pos]
        self.pos += 1
        return v

    def bounded(self, b):  # rng.rs:32-40
        threshold = ((~b + 1) & b) & 0xffffffff
        r = self.u32().copy()
        while True:
            bad = r < threshold
            if not bad.any():
                return r % np.uint32(b)
            self.retries += int(bad.sum())
            r[bad] = self.raw[self.rows[bad], self.pos[bad]]
            self.pos[bad] += 1


def _shuffled(st, vals, spp):
    """The two shuffles that end van_der_corput / sobol_2d (lowdiscrepancy.rs:14-22, 41-49) on vals (P, spp, ...)."""
    for i in range(spp):
        st.bounded(1)
    for i in range(spp):
        other = i + st.bounded(spp - i).astype(np.int64)
        a, b = vals[st.rows, i].copy(), vals[st.rows, other].copy()
        vals[st.rows, i], vals[st.rows, other] = b, a
    return vals


def _gray(cols, scramble, spp):
    out = np.zeros((scramble.shape[0], spp), np.uint32)
    v = scramble.copy()
    for i in range(spp):
        out[:, i] = v
        tz = (i + 1 & -(i + 1)).bit_length() - 1
        v = v ^ cols[tz]
    return out


def replay_tables(orc, pixel_indices, spp, dims, n_arrays):
    """ZeroTwoSequence::start_pixel for the keyed pixels: (t1 (P, dims, spp), t2 (P, dims, spp, 2), arrays (P, n_arrays, spp, 2)) float32, and the retries met."""
    n_pix = len(pixel_indices)
    st = _Stream(orc, pixel_indices, (2 * dims + n_arrays) * (2 + 2 * spp) + 64)
    t1, t2, arr = np.zeros((n_pix, dims, spp), F), np.zeros((n_pix, dims, spp, 2), F), np.zeros((n_pix, n_arrays, spp, 2), F)
    for t in range(dims):
        t1[:, t] = _shuffled(st, _unit(_gray(C0, st.u32(), spp)), spp)

    def sobol_2d():
        sx, sy = st.u32(), st.u32()
        return _shuffled(st, np.stack([_unit(_gray(C0, sx, spp)), _unit(_gray(C1, sy, spp))], axis=-1), spp)
    for t in range(dims):
        t2[:, t] = sobol_2d()
    for a in range(n_arrays):
        arr[:, a] = sobol_2d()
    return t1, t2, arr, st.retries


# ------------------------------------------------------------------------------------------------ a sample's draws
class Draws:
    """Per ray: its table values (1-D and 2-D, at its sample index), its arrays, the floats of its keyed stream, and the three counters."""

    def __init__(self, T1, T2, ARR, R, dims):
        n = T1.shape[0]
        self.T1, self.T2, self.ARR, self.R, self.dims = T1, T2, ARR, R, dims
        self.k1, self.k2, self.pos, self.v = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)

    def get_2d(self, ids):  # zerotwosequence.rs:168-180
        k = self.k2[ids]
        tab = 2 + k < self.dims
        p = self.pos[ids]
        out = np.where(tab[:, None], self.T2[ids, np.minimum(2 + k, self.dims - 1)], np.stack([self.R[ids, p + 1], self.R[ids, p]], axis=-1))
        self.pos[ids] += np.where(tab, 0, 2)
        self.k2[ids] += 1
        return out

    def get_1d(self, ids):  # :158-166
        k = self.k1[ids]
        tab = 1 + k < self.dims
        p = self.pos[ids]
        out = np.where(tab, self.T1[ids, np.minimum(1 + k, self.dims - 1)], self.R[ids, p])
        self.pos[ids] += np.where(tab, 0, 1)
        self.k1[ids] += 1
        return out


def draws_for(orc, spp, dims, width, height, ns, sample0, n_arrays, n_stream=512):
    """A Draws for the rays of an (H, W, ns) batch over its virtual film (pixel y * W + x, sample sample0 + sl), and the replayed tables themselves."""
    spp_r = 1
    while spp_r < spp:
        spp_r *= 2
    t1, t2, arr, retries = replay_tables(orc, np.arange(width * height), spp_r, dims, n_arrays)
    pix = np.repeat(np.arange(width * height), ns)
    s = np.tile(sample0 + np.arange(ns), width * height)
    R = np.stack([orc.rng_stream(int(p) * spp_r + int(k) + (1 << 32), n_stream)[1] for p, k in zip(pix, s)])
    return Draws(t1[pix, :, s], t2[pix, :, s], arr[pix, :, s], R, dims), (t1, t2, arr, retries)


# ------------------------------------------------------------------------------------------------ the diffuse lobes and pdf_li
def concentric_sample_disk(u):
    """sampling/mod.rs:28-47, evaluated in float64 on the float32 draws."""
    ox, oy = 2.0 * u[:, 0].astype(np.float64) - 1.0, 2.0 * u[:, 1].astype(np.float64) - 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.abs(ox) > np.abs(oy)
        r = np.where(first, ox, oy)
        theta = np.where(first, np.pi / 4 * (oy / ox), np.pi / 2 - np.pi / 4 * (ox / oy))
    zero = (ox == 0) & (oy == 0)
    return np.where(zero, 0.0, r * np.cos(theta)), np.where(zero, 0.0, r * np.sin(theta))


def power_heuristic(f, g):
    if not MIS:
        return np.ones_like(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (f * f) / (f * f + g * g)


def diffuse_lobes(lb):
    return [l for l in lb if l[0] == "diffuse"]


def bsdf_pdf(lb, wo, wi, n):
    """Bsdf::pdf(wo, wi, ALL & !SPECULAR): the mean of the matching lobes' pdfs; a Lambertian lobe's is |cos| / pi on wo's side."""
    if not diffuse_lobes(lb):
        return np.zeros(wo.shape[0])
    same = _dot(wi, n) * _dot(wo, n) > 0
    return np.where(same & (_dot(wo, n) != 0), np.abs(_dot(wi, n)) / np.pi, 0.0)


def sample_diffuse(lb, wo, n, ss, u):
    """Bsdf::sample_f(wo, u, ALL & !SPECULAR) at normal n with tangent ss: (f (n, 3), wi (n, 3), pdf (n,)). m matching lobes: u[0] picks floor(u[0] m) and is remapped;
    every Lambertian lobe has the same pdf, so the mean is that pdf; f is the sum of the lobes on wo's side."""
    dl = diffuse_lobes(lb)
    nr = wo.shape[0]
    if not dl:
        return np.zeros((nr, 3)), np.zeros((nr, 3)), np.zeros(nr)
    m = len(dl)
    um = (u[:, 0].astype(F) * F(m)).astype(F)
    comp = np.minimum(np.floor(um), m - 1)
    u0 = np.minimum((um - comp.astype(F)).astype(F), ONE_MINUS_EPS)
    dx, dy = concentric_sample_disk(np.stack([u0, u[:, 1].astype(F)], axis=-1))
    z = np.sqrt(np.maximum(0.0, 1.0 - dx * dx - dy * dy))
    ts = np.cross(n, ss)
    cos_o = _dot(wo, n)
    z = np.where(cos_o < 0, -z, z)
    wi = dx[:, None] * ss + dy[:, None] * ts + z[:, None] * n
    pdf = np.where(cos_o != 0, np.abs(z) / np.pi, 0.0)
    f = sum(col * sc_ / np.pi for _, col, _, sc_ in dl) * np.ones((nr, 1))
    f = np.where(((pdf > 0) & (_dot(wi, n) * cos_o > 0))[:, None], f, 0.0)
    return f, wi, pdf


def _tri_hit(tri, o, d):
    """Shape::intersect of ONE triangle: (t or inf, |cos| between its normal and d)."""
    p0, p1, p2 = tri[0], tri[1], tri[2]
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
        ok = (np.abs(det) > 0) & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1) & (t > T_EPS)
    n = _norm(np.cross(p0 - p2, p1 - p2))
    return np.where(ok, t, INF), np.abs(d @ n) / np.linalg.norm(d, axis=1)


def pdf_li(sc, light, p, so, wi):
    """Light::pdf_li(hit, wi): (pdf (n,), |cos| at the emitter where it is hit, else inf). so: the spawned origin."""
    nr = p.shape[0]
    if light[0] == "tri":
        tri = sc.tris[light[1]]
        t, cos_l = _tri_hit(tri, so, wi)
        area = 0.5 * np.linalg.norm(np.cross(tri[1] - tri[0], tri[2] - tri[0]))
        q = so + np.where(np.isfinite(t), t, 0.0)[:, None] * wi
        with np.errstate(divide="ignore", invalid="ignore"):
            pdf = np.where(np.isfinite(t), _dot(q - p, q - p) / (cos_l * area), 0.0)
        return pdf, np.where(np.isfinite(t), cos_l, INF)
    if light[0] == "infinite":  # infinite.rs:183-196 over the constant map's distribution (whitted_model.infinite_sample)
        rows = light[2]
        func = np.sin(np.pi * (np.arange(rows) + 0.5) / rows)
        func_int = func.sum() / rows
        w = _norm(wi)
        theta = np.arccos(np.clip(w[:, 2], -1.0, 1.0))
        iv = np.clip((theta / np.pi * rows).astype(int), 0, rows - 1)
        with np.errstate(divide="ignore"):
            pdf = np.where(np.sin(theta) == 0, 0.0, func[iv] / func_int / (2.0 * np.pi * np.pi * np.sin(theta)))
        return pdf, np.full(nr, INF)
    return np.zeros(nr), np.full(nr, INF)


# ------------------------------------------------------------------------------------------------ the integrator
class Result(wm.Result):
    def __init__(self, n):
        super().__init__(n)
        self.draws1 = np.zeros(n, np.int64)
        self.verts = np.zeros(n, np.int64)
        self.grazing = np.full(n, INF)
        self.pick = np.full(n, INF)
        self.n_shadow = 0
        self.n_probe = 0

    def info(self):
        return np.stack([self.nodes, self.draws, self.draws1, self.verts], axis=1)


def _is_delta(light):
    return light[0] in ("point", "distant")


def _spawn(p, n, w):
    return p + np.where((_dot(w, n) > 0)[:, None], n, -n) * T_EPS


def _light_edges(sc, light):
    tri = sc.tris[light[1]]
    return [(tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])]


def _estimate(sc, res, g, p, n, ss, wo, beta, lb, j, u_l, u_s, scale, own_sphere):
    """estimate_direct (mod.rs:222-318) for the rays g at their hits (p, n, ss) toward light j; adds beta * scale * ld into res.L, light half first."""
    light = sc.lights[j]
    # ---- light half
    li, wi, pdf, dist, surf = wm.sample_light(sc, light, p, u_l)
    f = wm.bsdf_f(lb, wo, wi, n) * np.abs(_dot(wi, n))[:, None]
    live = np.any(li != 0, axis=1) & (pdf > 0) & np.any(f != 0, axis=1)
    if live.any() and LIGHT_HALF:
        so = _spawn(p, n, wi)
        _, hk, _, _ = wm.intersect(sc, so[live], wi[live], t_max=np.maximum(dist[live] * (1.0 - 1e-6) - T_EPS, 0.0))
        clear = hk == 0
        res.n_shadow += int(live.sum())
        res.shadow[g[live]] = np.minimum(res.shadow[g[live]], wm.clearance(sc, p[live], wi[live], np.minimum(dist[live], 50.0), skip_surface=np.full(int(live.sum()), surf), own_sphere=own_sphere[live]))
        if light[0] == "tri":
            ln = _norm(np.cross(sc.tris[light[1]][0] - sc.tris[light[1]][2], sc.tris[light[1]][1] - sc.tris[light[1]][2]))
            res.grazing[g[live]] = np.minimum(res.grazing[g[live]], np.abs(wi[live] @ ln))
        with np.errstate(divide="ignore", invalid="ignore"):
            term = f[live] * li[live] / pdf[live][:, None]
            if not _is_delta(light):
                term = term * power_heuristic(pdf[live], bsdf_pdf(lb, wo[live], wi[live], n[live]))[:, None]
        res.L[g[live][clear]] += beta[live][clear] * term[clear] * scale
    if _is_delta(light) or not BSDF_HALF:
        return
    # ---- BSDF half
    f, wi, spdf = sample_diffuse(lb, wo, n, ss, u_s)
    f = f * np.abs(_dot(wi, n))[:, None]
    go = np.any(f != 0, axis=1) & (spdf > 0)
    if not go.any():
        return
    so = _spawn(p, n, wi)
    lp, cos_l = pdf_li(sc, light, p, so, wi)
    if light[0] == "tri":  # pdf_li and the probe's hit decide on the triangle's own edges, the diagonal it shares with its neighbour included
        for a, b in _light_edges(sc, light):
            res.edge[g[go]] = np.minimum(res.edge[g[go]], wm._seg_seg(so[go], _norm(wi[go]) * 50.0, a, b - a))
    go = go & (lp != 0)
    if not go.any():
        return
    res.grazing[g[go]] = np.minimum(res.grazing[g[go]], cos_l[go])
    res.n_probe += int(go.sum())
    t, kind, index, hn = wm.intersect(sc, so[go], wi[go])
    res.edge[g[go]] = np.minimum(res.edge[g[go]], wm.clearance(sc, so[go], wi[go], t, own_sphere=own_sphere[go], hit_sphere=np.where(kind == 2, index, -1)))
    le = np.zeros((int(go.sum()), 3))
    if light[0] == "tri":
        on = (kind == 1) & (index == light[1])
        le = np.where((on & (_dot(hn, -wi[go]) > 0))[:, None], sc.tris[light[1]][5], 0.0)
    elif light[0] == "infinite":
        le = np.where((kind == 0)[:, None], np.float64(light[1]), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = f[go] * le * (power_heuristic(spdf[go], lp[go]) / spdf[go])[:, None]
    res.L[g[go]] += beta[go] * np.where(np.any(le != 0, axis=1)[:, None], term, 0.0) * scale


def _li(sc, res, dr, ids, o, d, depth, max_depth, strategy, beta, own=None):
    if ids.size == 0:
        return
    res.nodes[ids] += 1
    t, kind, index, n = wm.intersect(sc, o, d)
    res.edge[ids] = np.minimum(res.edge[ids], wm.clearance(sc, o, d, t, own_sphere=own, hit_sphere=np.where(kind == 2, index, -1)))
    miss = kind == 0
    for light in sc.lights:
        if light[0] == "infinite":
            res.L[ids[miss]] += beta[miss] * np.float64(light[1])
    groups = {}
    for j in np.nonzero(~miss)[0]:
        groups.setdefault((int(kind[j]), int(index[j])), []).append(j)
    nl = len(sc.lights)
    for (kd, ix), js in groups.items():
        js = np.array(js)
        g, p, nn, wo, b = ids[js], o[js] + t[js, None] * d[js], n[js], -_norm(d[js]), beta[js]
        lb = wm.lobes(wm._material(sc, kd, ix))
        assert kd == 1 or not diffuse_lobes(lb), "the model samples diffuse lobes on triangles only (their tangent runs along p1 - p0)"
        # mesh.rs:396-413: ss0 = normalize(dpdu) = normalize(p1 - p0) (default uvs), ts = ss0 x ns, then ss = ts x ns = (ss0 x ns) x ns = -ss0 for ss0 normal to ns:
        # the shading tangent the Bsdf is built on points from p1 to p0
        ss = np.broadcast_to(-_norm(sc.tris[ix][1] - sc.tris[ix][0]), nn.shape) if kd == 1 else np.zeros(nn.shape)
        if kd == 1 and sc.tris[ix][5] is not None:
            res.L[g] += b * np.where((_dot(nn, wo) > 0)[:, None], sc.tris[ix][5], 0.0)
        own_sphere = np.full(js.size, ix if kd == 2 else -1)
        if nl > 0 and strategy == ALL:  # uniform_sample_all_light
            have = dr.v[g] < max_depth
            base = 2 * dr.v[g] * nl
            dr.v[g] += 1
            for j in range(nl):
                u_l, u_s = np.zeros((js.size, 2), F), np.zeros((js.size, 2), F)
                if have.any():
                    u_l[have], u_s[have] = dr.ARR[g[have], base[have] + 2 * j], dr.ARR[g[have], base[have] + 2 * j + 1]
                if (~have).any():  # get_2d_array returned None: u_light = get_2d(), then u_scattering = get_2d()
                    u_l[~have] = dr.get_2d(g[~have])
                    u_s[~have] = dr.get_2d(g[~have])
                _estimate(sc, res, g, p, nn, ss, wo, b, lb, j, u_l, u_s, 1.0, own_sphere)
        elif nl > 0:  # uniform_sample_one_light(.., None)
            s1 = dr.get_1d(g).astype(F)
            sn = (s1 * F(nl)).astype(F)
            pick = np.minimum(nl - 1, np.floor(sn).astype(int))
            res.pick[g] = np.minimum(res.pick[g], np.abs(sn.astype(np.float64) - np.round(sn.astype(np.float64))) if nl > 1 else INF)
            u_l, u_s = dr.get_2d(g), dr.get_2d(g)
            for j in range(nl):
                sel = pick == j
                if sel.any():
                    _estimate(sc, res, g[sel], p[sel], nn[sel], ss[sel], wo[sel], b[sel], lb, j, u_l[sel], u_s[sel], float(nl), own_sphere[sel])
        if depth + 1 < max_depth:
            for want in ("spec_r", "spec_t"):
                u = dr.get_2d(g)
                weight, wi, valid, gap = wm.sample_specular(lb, want, wo, nn, u)
                res.sin2[g] = np.minimum(res.sin2[g], gap)
                v = np.nonzero(valid)[0]
                _li(sc, res, dr, g[v], _spawn(p[v], nn[v], wi[v]), wi[v], depth + 1, max_depth, strategy, b[v] * weight[v], own_sphere[v])


def render(sc, o, d, max_depth, strategy, dr, active=None):
    """DirectLightingIntegrator::li(ray, 0) for the rays o, d (n, 3) with the draws `dr` (a fresh Draws): a Result."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    res = Result(o.shape[0])
    ids = np.arange(o.shape[0]) if active is None else np.nonzero(active)[0]
    _li(sc, res, dr, ids, o[ids], d[ids], 0, max_depth, strategy, np.ones((ids.size, 3)))
    res.draws, res.draws1, res.verts = dr.k2.copy(), dr.k1.copy(), dr.v.copy() if strategy == ALL else np.zeros_like(dr.v)
    return res
