"""An independent model of the reference's MIPMap (rustracer-core/src/mipmap.rs), ImageTexture::evaluate (texture/imagemap.rs:232-235) and UVMapping2D::map
(texture/mod.rs:52-60), written from those sources in plain numpy - not from oracle/orc_mipmap.h and not from the device code.

Inputs are the float32 values the device gets; the UV mapping is the reference's own float32 expression (two IEEE operations, the same everywhere), everything
after it is float64. Texel indices are int64 with a true modulo, so neither the two's-complement mask of the device's Repeat wrap nor any 32-bit saturation of a
float -> integer conversion is shared with the code under test. `dtype=np.float32` runs the same code in single precision: a diagnostic that tells a rounding
difference from a defect; no assertion rests on it.

What a single-precision evaluation may differ by
------------------------------------------------
`lookup_diff` returns (value, widened, unit), all per channel:

* `unit` bounds the error of a float32 evaluation of everything that is continuous in the inputs. E = 2^-24 is float32's unit roundoff.
    - triangle: s = st * size - 0.5 carries 2 roundings at magnitude |s| + 1, so ds and dt are off by 2 E (|s| + 1) and 2 E (|t| + 1); the bilinear value moves
      by at most the level's texel range per unit of ds or dt; 8 roundings in the combination at the texels' magnitude. A floor that lands on the other side
      only renames the taps (bilinear interpolation is continuous).
    - the blend between two levels: the level is n - 1 + log2(x) with a float32 log2 good to a few ulp, E (2 n + 4 |log2 x| + 8) in all, times the finer
      level's texel range (an upper bound of the difference of the two levels' values).
    - EWA: weights come from a table, so the only continuous errors are the accumulation of the taps, 2 E (taps + 8) at the texels' magnitude, and the table's
      own single-precision entries (in that 8).
* `widened` covers the two things that are not continuous.
    - The EWA table index floor(r2 * 128). For every tap whose r2 * 128 lies within delta of an integer the weight may be the neighbouring entry; the result
      sum(w t) / sum(w) then moves by |dw| |t - mean| / sumWts. delta is this model's bound of the float32 error of r2 * 128 at that tap, from the magnitudes of
      r2's three terms, rounding by rounding: a scaled derivative carries 2 E (the mapping's product, the level's size), the clamped minor axis 9 E (two lengths,
      their quotient with max_aniso, the product); A0, B0 and C0 what their products and sums add to that, B0 measured against 2 (|x0 y0| + |x1 y1|) since it can
      cancel; F = A0 C0 - B0^2 / 4 cancels too and carries C0 dA + A0 dC + |B0| dB / 2 and its own three roundings; the offsets ss = is - s carry
      2 E (|s| + 1) + E |ss| (and E |is| once `is` no longer fits float32's 24 bits).
      A tap at r2 = 1 enters or leaves with the last entry, exp(-2) - exp(-2) = 0, so the ellipse's edge and its bounding box need nothing.
    - Under Black, `lookup` jumps at level = n - 1 from triangle(n - 1, st) - a 1 x 1 level blended with black - to that level's texel. Where the level is
      within its error of n - 1 the difference of the two is allowed.
  No query is dropped.

ENVELOPE_K is the largest (|oracle - model| - widened) / unit measured on the CPU (tests/test_mipmap_model_cpu.py); if `unit` is the bound it is meant to be,
it is below 1.
"""
import numpy as np

WRAP_REPEAT, WRAP_BLACK, WRAP_CLAMP = 0, 1, 2  # rustracer_amd.scene_desc
E = 2.0 ** -24
F32 = np.float32

# Measured by tests/test_mipmap_model_cpu.py::test_lookups_oracle_against_the_model over every (shape, wrap, filter) of CASES and the query sets below: the
# largest (|oracle - model| - widened) / unit. The tests assert 4 x this. (MEASUREMENTS.md, "Image maps against a float64 model".)
ENVELOPE_K = 0.96
# Pyramids: the largest |level texel - model| / max texel measured over SHAPES x wraps, oracle and host alike; the gate is 4 x this and has to stay below 1e-5
# (8 single-precision taps whose weights come from sinf).
PYRAMID_ENVELOPE = 3.5e-7
PYRAMID_CEILING = 1.0e-5

SHAPES = [(1, 1), (2, 8), (5, 3), (2, 1), (1, 2), (4, 2), (8, 2), (64, 4), (4, 64), (16, 16), (3, 1), (1, 5), (24, 20), (33, 17)]  # (w, h); see scene order
FILTERS = [("trilinear", True, 8.0), ("ewa1", False, 1.0), ("ewa2", False, 2.0), ("ewa8", False, 8.0)]
WRAPS = [("repeat", WRAP_REPEAT), ("black", WRAP_BLACK), ("clamp", WRAP_CLAMP)]
MAPPINGS = [(1.0, 1.0, 0.0, 0.0), (2.0, 0.5, 0.25, -0.5)]  # su sv du dv: the identity, and one whose products are exact


def image(w, h, seed=3):
    """(h, w, 3) float32, not symmetric under transposition or mirroring: a crop of a noisy checkerboard with near-black cells (so that the Lanczos zoom rings
    below zero and the clamp at zero acts) plus two ramps."""
    from rustracer_amd.scenes.procedural import checker_fbm_image
    base = checker_fbm_image(96, seed, (0.9, 0.5, 0.2), (0.01, 0.02, 0.03), 24).astype(np.float64)
    img = base[5:5 + h, 9:9 + w].copy()
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img[..., 0] += 0.30 * x / max(w, 1)
    img[..., 1] += 0.25 * y / max(h, 1)
    img[..., 2] += 0.05 * ((3 * x + 5 * y) % 7)
    return img.astype(F32)


# ---------------------------------------------------------------- pyramid (mipmap.rs:67-194, 362-408)
def _lanczos(x):  # :395-408
    x = np.abs(x)
    px = np.where(x < 1e-5, 1.0, x) * np.pi
    v = np.sin(2.0 * px) / (2.0 * px) * (np.sin(px) / px)
    return np.where(x < 1e-5, 1.0, np.where(x > 1.0, 0.0, v))


def _resample_weights(old, new, f):  # :362-393
    i = np.arange(new).astype(f)
    center = (i + f(0.5)) * f(old) / f(new)
    first = np.floor((center - f(2.0)) + f(0.5))
    pos = first[:, None] + np.arange(4).astype(f)[None, :] + f(0.5)
    w = _lanczos((pos - center[:, None]) / f(2.0)).astype(f)
    w = w * (f(1.0) / w.sum(axis=1, keepdims=True))
    return first.astype(np.int64), w


def _wrap_index(i, n, wrap):
    if wrap == WRAP_REPEAT:
        return np.mod(i, n)
    if wrap == WRAP_CLAMP:
        return np.clip(i, 0, n - 1)
    return i


def _zoom(img, wrap, f):  # :75-139
    ry, rx = img.shape[:2]
    px, py = 1 << (rx - 1).bit_length(), 1 << (ry - 1).bit_length()
    first, w = _resample_weights(rx, px, f)
    o = _wrap_index(first[:, None] + np.arange(4)[None, :], rx, wrap)  # (px, 4)
    ok = (o >= 0) & (o < rx)
    out = np.zeros((py, px, 3), f)
    out[:ry] = (img[:, np.clip(o, 0, rx - 1)] * (w * ok)[None, :, :, None]).sum(axis=2)  # only the first res.y rows are filled (:89-110)
    first, w = _resample_weights(ry, py, f)
    o = _wrap_index(first[:, None] + np.arange(4)[None, :], ry, wrap)  # (py, 4)
    ok = (o >= 0) & (o < ry)
    col = (out[np.clip(o, 0, ry - 1)] * (w * ok)[:, :, None, None]).sum(axis=1)  # (py, px, 3): reads rows below res.y only
    return np.maximum(col, f(0.0))  # Clampable::clamp(0, inf) (:134-136)


class MipModel:
    def __init__(self, img, trilinear=False, max_aniso=8.0, wrap=WRAP_REPEAT, dtype=np.float64):
        self.f = f = dtype
        self.trilinear, self.max_aniso, self.wrap = bool(trilinear), f(F32(max_aniso)), int(wrap)
        img = np.asarray(img, F32).astype(f)
        h, w = img.shape[:2]
        if (w & (w - 1)) or (h & (h - 1)):
            img = _zoom(img, self.wrap, f)
            h, w = img.shape[:2]
        self.levels = [img]
        n_levels = 1 + (max(w, h).bit_length() - 1)  # 1 + floor(log2(max)) (:159); exact for a power of two
        for i in range(1, n_levels):  # :168-187
            v, u = self.levels[i - 1].shape[:2]
            t, s = np.meshgrid(np.arange(max(1, v // 2)), np.arange(max(1, u // 2)), indexing="ij")
            self.levels.append((self.texel(i - 1, 2 * s, 2 * t) + self.texel(i - 1, 2 * s + 1, 2 * t) + self.texel(i - 1, 2 * s, 2 * t + 1)
                                + self.texel(i - 1, 2 * s + 1, 2 * t + 1)) * f(0.25))
        self.lut = (np.exp(-2.0 * (np.arange(128) / 127.0)) - np.exp(-2.0)).astype(f)  # :33-44
        lo = [np.minimum(L.min(axis=(0, 1)), 0.0) if self.wrap == WRAP_BLACK else L.min(axis=(0, 1)) for L in self.levels]
        self.rng = [np.asarray(L.max(axis=(0, 1)) - a, np.float64) for L, a in zip(self.levels, lo)]  # per level and channel (Black reads zeros too)
        self.mx = [np.asarray(np.abs(L).max(axis=(0, 1)), np.float64) for L in self.levels]

    def n(self):
        return len(self.levels)

    def texel(self, level, s, t):  # :208-225; s, t int64 arrays
        L = self.levels[level]
        v, u = L.shape[:2]
        s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
        if self.wrap == WRAP_REPEAT:
            return L[np.mod(t, v), np.mod(s, u)]
        if self.wrap == WRAP_CLAMP:
            return L[np.clip(t, 0, v - 1), np.clip(s, 0, u - 1)]
        inside = (s >= 0) & (s < u) & (t >= 0) & (t < v)
        return np.where(inside[..., None], L[np.clip(t, 0, v - 1), np.clip(s, 0, u - 1)], self.f(0.0))

    def triangle(self, level, st):  # :285-308 -> value, unit
        f = self.f
        level = min(max(level, 0), self.n() - 1)
        v, u = self.levels[level].shape[:2]
        s, t = st[0] * f(u) - f(0.5), st[1] * f(v) - f(0.5)
        s0, t0 = int(np.floor(s)), int(np.floor(t))
        ds, dt = s - f(s0), t - f(t0)
        tx = self.texel(level, np.array([s0, s0, s0 + 1, s0 + 1]), np.array([t0, t0 + 1, t0, t0 + 1]))
        val = tx[0] * (f(1) - ds) * (f(1) - dt) + tx[1] * (f(1) - ds) * dt + tx[2] * ds * (f(1) - dt) + tx[3] * ds * dt
        unit = self.rng[level] * 2.0 * E * (abs(float(s)) + abs(float(t)) + 2.0) + 8.0 * E * self.mx[level]
        return val, unit

    def lookup(self, st, width):  # :227-245 -> value, widened, unit
        f, n = self.f, self.n()
        x = max(width, f(1e-8))
        lg = np.log2(x)
        level = f(n) - f(1) + lg
        err = E * (2.0 * n + 4.0 * abs(float(lg)) + 8.0)
        last = self.texel(n - 1, 0, 0)
        wid = np.zeros(3)
        if self.wrap == WRAP_BLACK and abs(float(level) - (n - 1.0)) <= err:  # the jump between triangle(n - 1) and the last texel
            wid = np.abs(np.asarray(self.triangle(n - 1, st)[0], np.float64) - last)
        if level < 0:
            val, unit = self.triangle(0, st)
            return val, wid, unit
        if level >= f(n) - f(1):
            return last, wid, 2.0 * E * self.mx[n - 1]
        il = int(np.floor(level))
        delta = level - f(il)
        a, ua = self.triangle(il, st)
        b, ub = self.triangle(il + 1, st)
        return a * (f(1) - delta) + b * delta, wid, ua + ub + err * self.rng[il] + 3.0 * E * self.mx[il]

    def ewa(self, level, st, d0, d1, e1=2.0 * E):  # :310-360 -> value, widened, unit, (taps, flagged); e1: relative error of a float32 d1
        f, n = self.f, self.n()
        if level >= n:
            return self.texel(n - 1, 0, 0), np.zeros(3), 2.0 * E * self.mx[n - 1], (0, 0)
        v, u = self.levels[level].shape[:2]
        s, t = st[0] * f(u) - f(0.5), st[1] * f(v) - f(0.5)
        x0, y0, x1, y1 = d0[0] * f(u), d0[1] * f(v), d1[0] * f(u), d1[1] * f(v)
        A0 = y0 * y0 + y1 * y1 + f(1)
        B0 = f(-2) * (x0 * y0 + x1 * y1)
        C0 = x0 * x0 + x1 * x1 + f(1)
        F = A0 * C0 - B0 * B0 * f(0.25)
        inv_f = f(1) / F
        A, B, C = A0 * inv_f, B0 * inv_f, C0 * inv_f
        det = -B * B + f(4) * A * C
        inv_det = f(1) / det
        us, vs = np.sqrt(det * C), np.sqrt(A * det)
        s0, s1 = int(np.ceil(s - f(2) * inv_det * us)), int(np.floor(s + f(2) * inv_det * us))
        t0, t1 = int(np.ceil(t - f(2) * inv_det * vs)), int(np.floor(t + f(2) * inv_det * vs))
        assert (s1 - s0 + 1) * (t1 - t0 + 1) <= 1 << 20, "a footprint of a million texels is a slow kernel, not a test"
        it, is_ = np.meshgrid(np.arange(t0, t1 + 1, dtype=np.int64), np.arange(s0, s1 + 1, dtype=np.int64), indexing="ij")
        tt, ss = it.astype(f) - t, is_.astype(f) - s
        T1, T2, T3 = A * ss * ss, B * ss * tt, C * tt * tt
        r2 = T1 + T2 + T3
        inside = r2 < 1
        x = r2 * f(128)
        idx = np.minimum(np.floor(np.where(inside, x, 0)).astype(np.int64), 127)
        wt = np.where(inside, self.lut[idx], f(0))
        tx = self.texel(level, is_, it)
        sum_w = wt.sum()
        val = (tx * wt[..., None]).sum(axis=(0, 1)) / sum_w
        # -- delta: the float32 error of r2 * 128 per tap (module docstring)
        x0, y0, x1, y1, Af, Bf, Cf, Ff = (abs(float(q)) for q in (x0, y0, x1, y1, A0, B0, C0, F))
        e0 = 2.0 * E  # d0: the mapping's product, the scaling by the level's size
        Bm = 2.0 * (x0 * y0 + x1 * y1)
        dA = y0 * y0 * (2.0 * e0 + E) + y1 * y1 * (2.0 * e1 + E) + 2.0 * E * Af
        dC = x0 * x0 * (2.0 * e0 + E) + x1 * x1 * (2.0 * e1 + E) + 2.0 * E * Cf
        dB = 2.0 * (x0 * y0 * (2.0 * e0 + E) + x1 * y1 * (2.0 * e1 + E)) + 2.0 * E * Bm
        dF = Cf * dA + Af * dC + E * Af * Cf + 0.5 * Bf * dB + 2.0 * E * 0.25 * Bf * Bf + E * Ff
        rel_f = dF / Ff
        rel_a, rel_c = dA / Af + rel_f + 2.0 * E, dC / Cf + rel_f + 2.0 * E
        ass, att = np.abs(ss).astype(np.float64), np.abs(tt).astype(np.float64)
        e_ss = 2.0 * E * (abs(float(s)) + 1.0) + E * (np.abs(is_) * (np.abs(is_) >= 2 ** 24) + ass)
        e_tt = 2.0 * E * (abs(float(t)) + 1.0) + E * (np.abs(it) * (np.abs(it) >= 2 ** 24) + att)
        a1, a2, a3 = np.abs(T1).astype(np.float64), np.abs(T2).astype(np.float64), np.abs(T3).astype(np.float64)
        Aa, Ba, Ca = abs(float(A)), abs(float(B)), abs(float(C))
        err = (a1 * (rel_a + 2.0 * E) + 2.0 * Aa * ass * e_ss
               + a2 * (rel_f + 4.0 * E) + ass * att * (dB / Ff) + Ba * (att * e_ss + ass * e_tt)
               + a3 * (rel_c + 2.0 * E) + 2.0 * Ca * att * e_tt
               + 2.0 * E * (a1 + a2 + a3))
        delta = 128.0 * err
        xf = x.astype(np.float64)
        lo = np.clip(np.floor(xf - delta), 0, 128).astype(np.int64)
        hi = np.clip(np.floor(xf + delta), 0, 128).astype(np.int64)
        lut = np.append(np.asarray(self.lut, np.float64), 0.0)  # entry 128: outside the ellipse
        cur = np.where(inside, idx, 128)
        dw = np.maximum(lut[lo] - lut[cur], lut[cur] - lut[hi])
        flagged = dw > 0
        wid = (dw[..., None] * np.abs(np.asarray(tx, np.float64) - np.asarray(val, np.float64))).sum(axis=(0, 1)) / float(sum_w)
        taps = int(inside.sum())
        unit = 2.0 * E * (taps + 8.0) * self.mx[level]
        return val, wid, unit, (taps, int(flagged.sum()))

    def lookup_diff(self, st, d0, d1, info=None):  # :247-283 -> value, widened, unit
        f = self.f
        st, d0, d1 = [f(q) for q in st], [f(q) for q in d0], [f(q) for q in d1]
        if self.trilinear:
            width = max(abs(d0[0]), abs(d0[1]), abs(d1[0]), abs(d1[1]))
            return self.lookup(st, f(2) * width)
        if d0[0] * d0[0] + d0[1] * d0[1] < d1[0] * d1[0] + d1[1] * d1[1]:
            d0, d1 = d1, d0
        major = np.sqrt(d0[0] * d0[0] + d0[1] * d0[1])
        minor = np.sqrt(d1[0] * d1[0] + d1[1] * d1[1])
        e1 = 2.0 * E
        if minor * self.max_aniso < major and minor > 0:
            e1 = 9.0 * E  # two lengths (2 E each), their quotient with the product by max_aniso (3 E), the product with d1, then as d0
            scale = major / (minor * self.max_aniso)
            d1 = [d1[0] * scale, d1[1] * scale]
            minor = minor * scale
        if minor == 0:
            val, unit = self.triangle(0, st)
            return val, np.zeros(3), unit
        n = self.n()
        lg = np.log2(minor)
        lod = max(f(0), f(n) - f(1) + lg)
        ilod = int(np.floor(lod))
        fr = lod - f(ilod)
        a, wa, ua, ia = self.ewa(ilod, st, d0, d1, e1)
        b, wb, ub, ib = self.ewa(ilod + 1, st, d0, d1, e1)
        if info is not None:
            info.update(ilod=ilod, taps=ia[0] + ib[0], flagged=ia[1] + ib[1])
        err = E * (2.0 * n + 4.0 * abs(float(lg)) + 8.0)
        frf = float(fr)
        return (a * (f(1) - fr) + b * fr, (1.0 - frf) * wa + frf * wb + err * (wa + wb),
                ua + ub + err * self.rng[min(ilod, n - 1)] + 3.0 * E * self.mx[min(ilod, n - 1)])

    def table_step_cap(self, ilod):
        """one table step (the largest, at the table's start) times the level's texel range: what no widened allowance may exceed"""
        return float(self.lut[0] - self.lut[1]) * self.rng[min(max(ilod, 0), self.n() - 1)]


def image_tex(model, mapping, uv, duv, info=None):
    """ImageTexture::evaluate: UVMapping2D::map in the reference's float32 (texture/mod.rs:52-60), then lookup_diff (imagemap.rs:232-235)."""
    su, sv, du, dv = (F32(q) for q in mapping)
    uv, duv = np.asarray(uv, F32), np.asarray(duv, F32)
    st = (su * uv[0] + du, sv * uv[1] + dv)
    return model.lookup_diff(st, (su * duv[0], sv * duv[1]), (su * duv[2], sv * duv[3]), info)


def evaluate(model, mapping, q):
    """every query of q = dict(uv (n, 2), duv (n, 4)) -> value, widened, unit (n, 3) float64, and the per-query tap statistics"""
    n = q["uv"].shape[0]
    val, wid, unit = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    infos = []
    for i in range(n):
        info = {}
        v, w, u = image_tex(model, mapping, q["uv"][i], q["duv"][i], info)
        val[i], wid[i], unit[i] = v, w, u
        infos.append(info)
    return val, wid, unit, infos


# ---------------------------------------------------------------- query sets
def level_sizes(w, h):
    w, h = 1 << (w - 1).bit_length(), 1 << (h - 1).bit_length()
    out = [(w, h)]
    while max(w, h) > 1:
        w, h = max(1, w // 2), max(1, h // 2)
        out.append((w, h))
    return out


def queries(w, h, seed, n_a=48, n_b=8):
    """the query sets (a), (b) and (c) for an image of w x h texels: dict(uv (n, 2), duv (n, 4) = dudx dvdx dudy dvdy) in float32, and the set of each query"""
    rng = np.random.default_rng(seed)
    sizes = level_sizes(w, h)
    nl = len(sizes)
    uv, duv, kind = [], [], []
    # (a) anywhere, every level
    a_uv = rng.normal(0.0, 3.0, (n_a, 2))
    a_uv[::3] = -np.abs(a_uv[::3])
    a_d = rng.choice([-1.0, 1.0], (n_a, 4)) * 10.0 ** rng.uniform(-4.0, 0.5, (n_a, 4))
    uv.append(a_uv); duv.append(a_d); kind += ["a"] * n_a
    # (b) per level: within 2 texels of the borders 0 and 1, on texel centres and on texel edges, with a footprint that selects that level
    for l, (lw, lh) in enumerate(sizes):
        d = 2.0 ** (l - (nl - 1)) * rng.uniform(0.6, 1.4, n_b)
        b_uv = np.stack([rng.choice([0.0, 1.0], n_b) + rng.uniform(-2, 2, n_b) / lw, rng.choice([0.0, 1.0], n_b) + rng.uniform(-2, 2, n_b) / lh], 1)
        i, j = rng.integers(-2, lw + 3, n_b), rng.integers(-2, lh + 3, n_b)
        b_uv[1::3] = np.stack([(i + 0.5) / lw, (j + 0.5) / lh], 1)[1::3]
        b_uv[2::3] = np.stack([i / lw, j / lh], 1)[2::3]
        b_d = np.stack([d, np.zeros(n_b), np.zeros(n_b), 0.8 * d], 1)
        uv.append(b_uv); duv.append(b_d); kind += ["b"] * n_b
    # (c) degenerate footprints
    m = 10.0 ** rng.uniform(-3.0, -0.5, 12)
    x, y = m * 0.8, m * 0.6
    c_d = np.zeros((12, 4))
    c_d[1] = [x[1], y[1], 0, 0]; c_d[2] = [0, 0, x[2], y[2]]       # one of the two zero
    c_d[3] = [x[3], y[3], x[3], y[3]]; c_d[4] = [x[4], -y[4], x[4], -y[4]]  # dst0 = dst1
    c_d[5] = [x[5], y[5], -y[5], x[5]]; c_d[6] = [x[6], y[6], y[6], x[6]]  # |dst0| = |dst1| exactly
    c_d[7] = [m[7], 0, 0, 0.5 * m[7]]; c_d[8] = [0, 0.3 * m[8], m[8], 0]  # axis-aligned, B = 0
    c_d[9] = [m[9], 0.2 * m[9], 0.002 * m[9], -0.01 * m[9]]; c_d[10] = [0.003 * m[10], 0.01 * m[10], 0.5 * m[10], -m[10]]  # 100 : 1
    c_d[11] = [m[11], 0, 0.01 * m[11], 0]  # 100 : 1 and parallel
    uv.append(rng.normal(0.0, 1.5, (12, 2))); duv.append(c_d); kind += ["c"] * 12
    return dict(uv=np.concatenate(uv).astype(F32), duv=np.concatenate(duv).astype(F32)), np.array(kind)


def far_queries(w, h, seed, n=24):
    """st * size from 2^31 up to 2^40 (both signs), derivatives small enough for level 0 and a footprint of a texel or two: trilinear and EWA alike then read
    level 0 only. Far inside 64 bits: at 2^63 the reference's own `t0..(t1 + 1)` overflows."""
    rng = np.random.default_rng(seed)
    pw, ph = level_sizes(w, h)[0]
    mag = 2.0 ** rng.uniform(31.0, 40.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    uv = mag / np.array([pw, ph])
    uv[::4, 1] = rng.uniform(-2, 2, len(uv[::4]))  # one axis far, the other near
    d = rng.choice([-1.0, 1.0], (n, 4)) * 10.0 ** rng.uniform(-4.0, -3.0, (n, 4)) / max(pw, ph)
    d[::5] = 0.0
    return dict(uv=uv.astype(F32), duv=d.astype(F32))


def add_cases(d):
    """every (shape, wrap, filter) as an image and an image texture of scene description `d`, the 1 x 1, the 2 x 8 and the resampled 5 x 3 first (SHAPES' order),
    so that the texel array's running base and every level's offset and tile shift differ from image to image"""
    cases = []
    for w, h in SHAPES:
        img = image(w, h)
        for wrap_name, wrap in WRAPS:
            for filter_name, trilinear, aniso in FILTERS:
                mip = d.add_mip(img, trilinear=trilinear, max_aniso=aniso, wrap=wrap)
                mapping = MAPPINGS[len(cases) % 2]
                cases.append(dict(name=f"{w}x{h} {wrap_name} {filter_name}", shape=(w, h), wrap_name=wrap_name, wrap=wrap, filter=filter_name, trilinear=trilinear,
                                  aniso=aniso, img=img, mip=mip, tex=d.image_tex(mip, *mapping), mapping=mapping, seed=1000 * w + 10 * h + wrap))
    return cases


def model_of(case, dtype=np.float64):
    return MipModel(case["img"], case["trilinear"], case["aniso"], case["wrap"], dtype)


WIDENED_FLOOR = 1e-3  # a query counts as widened where `widened` exceeds this share of `unit` (below it, it is arithmetic dust of the model itself)


def judge(model, case, q, got):
    """got (n, 3) against the model on queries q -> ratio (n,) = the largest (|got - model| - widened) / unit per query, the share of widened queries, and
    whether any widened allowance exceeds one table step of its level's range"""
    val, wid, unit, infos = evaluate(model, case["mapping"], q)
    ratio = ((np.abs(np.asarray(got, np.float64) - val) - wid) / unit).max(axis=1)
    widened = (wid > WIDENED_FLOOR * unit).any(axis=1)
    over = [i for i in range(len(infos)) if (wid[i] > model.table_step_cap(infos[i].get("ilod", 0)) + WIDENED_FLOOR * unit[i]).any()]
    return dict(val=val, wid=wid, unit=unit, infos=infos, ratio=ratio, share=float(widened.mean()), over=over)


def outside_queries(rng, n):
    """one coordinate 4 to 6 outside [0, 1] - beyond 2 texels of the coarsest level plus any footprint of derivatives up to 0.05 - the other anywhere"""
    uv = rng.normal(0.0, 1.0, (n, 2))
    axis = rng.integers(0, 2, n)
    uv[np.arange(n), axis] = np.where(rng.random(n) < 0.5, 1.0 + rng.uniform(4.0, 6.0, n), -rng.uniform(4.0, 6.0, n))
    duv = rng.choice([-1.0, 1.0], (n, 4)) * 10.0 ** rng.uniform(-4.0, -1.3, (n, 4))
    duv[::6] = 0.0
    return dict(uv=uv.astype(F32), duv=duv.astype(F32))


def periodic_queries(rng, n):
    """coordinates on a grid of 1 / 1024 in [-4, 4] and the same shifted by integers up to 8: st, the shifted st and st * size - 0.5 are exact in float32"""
    uv = rng.integers(-4096, 4097, (n, 2)) / 1024.0
    shift = rng.integers(-8, 9, (n, 2))
    duv = (rng.choice([-1.0, 1.0], (n, 4)) * 10.0 ** rng.uniform(-4.0, 0.3, (n, 4))).astype(F32)
    duv[::6] = 0.0
    return dict(uv=uv.astype(F32), duv=duv), dict(uv=(uv + shift).astype(F32), duv=duv)
