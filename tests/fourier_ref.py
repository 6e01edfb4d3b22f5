"""Tabulated Fourier BSDFs for the tests: a .bsdf writer and an independent numpy restatement of the reader and of FourierBSDF's f / pdf / sample_f.

Written from the file format and the algorithm (pbrt-v3's FourierBSDF as the reference states it: rc/bsdf/fourier.rs, rc/interpolation.rs), all in float32
and in the reference's operation order, vectorised over queries. The two Newton-bisection loops stop after 64 steps, as the device's do. Not a test module.
"""
import struct

import numpy as np

F = np.float32
MAGIC = b"SCATFUN\x01"
MAX_ITER = 64


# ---------------------------------------------------------------- file format
def write_bsdf(path, mu, cdf, offsets, lengths, a, m_max, n_channels, eta, flags=1, n_bases=1, magic=MAGIC):
    """A .bsdf file: magic, nine u32 (flags nMu nCoeffs mMax nChannels nBases nMetadataBytes nParameters nParameterValues), five f32 (eta alpha[2]
    unused[2]), mu[nMu], cdf[nMu^2], {offset, length}[nMu^2], a[nCoeffs]."""
    mu, cdf, a = (np.asarray(x, F).ravel() for x in (mu, cdf, a))
    ol = np.stack([np.asarray(offsets, np.uint32).ravel(), np.asarray(lengths, np.uint32).ravel()], 1).ravel()
    with open(path, "wb") as f:
        f.write(magic)
        f.write(struct.pack("<9I", flags, mu.size, a.size, m_max, n_channels, n_bases, 0, 0, 0))
        f.write(struct.pack("<5f", eta, 0.0, 0.0, 0.0, 0.0))
        f.write(mu.astype("<f4").tobytes() + cdf.astype("<f4").tobytes() + ol.astype("<u4").tobytes() + a.astype("<f4").tobytes())
    return str(path)


class Table:
    def __init__(self, mu, cdf, offset, length, a, m_max, n_channels, eta):
        self.mu, self.cdf, self.a = np.asarray(mu, F), np.asarray(cdf, F), np.asarray(a, F)
        self.offset, self.length = np.asarray(offset, np.int64), np.asarray(length, np.int64)
        self.m_max, self.n_channels, self.eta, self.n_mu = int(m_max), int(n_channels), F(eta), len(mu)
        self.a0 = np.where(self.length > 0, self.a[np.minimum(self.offset, max(self.a.size - 1, 0))] if self.a.size else F(0), F(0)).astype(F)


def read_bsdf(path):
    """FourierBSDFTable::read."""
    b = open(path, "rb").read()
    if b[:8] != MAGIC:
        raise ValueError(f"BSDF file {path} has an invalid header")
    flags, n_mu, n_coeffs, m_max, n_ch, n_bases = struct.unpack_from("<6I", b, 8)
    eta = struct.unpack_from("<f", b, 44)[0]
    if flags != 1 or n_ch not in (1, 3) or n_bases != 1:
        raise ValueError(f"Unsupported BSDF file {path}")
    o = 64
    mu = np.frombuffer(b, "<f4", n_mu, o); o += 4 * n_mu
    cdf = np.frombuffer(b, "<f4", n_mu * n_mu, o); o += 4 * n_mu * n_mu
    ol = np.frombuffer(b, "<u4", 2 * n_mu * n_mu, o); o += 8 * n_mu * n_mu
    a = np.frombuffer(b, "<f4", n_coeffs, o)
    return Table(mu, cdf, ol[0::2], ol[1::2], a, m_max, n_ch, eta)


# ---------------------------------------------------------------- synthetic tables
def integrate_catmull_rom(x, values):
    """Running integral of the Catmull-Rom spline through (x, values) (IntegrateCatmullRom): cdf[0] = 0."""
    x, values = np.asarray(x, np.float64), np.asarray(values, np.float64)
    n = len(x)
    cdf = np.zeros(n)
    for i in range(n - 1):
        x0, x1, f0, f1 = x[i], x[i + 1], values[i], values[i + 1]
        w = x1 - x0
        d0 = w * (f1 - values[i - 1]) / (x1 - x[i - 1]) if i > 0 else f1 - f0
        d1 = w * (values[i + 2] - f0) / (x[i + 2] - x0) if i + 2 < n else f1 - f0
        cdf[i + 1] = cdf[i] + ((d0 - d1) * (1.0 / 12.0) + (f0 + f1) * 0.5) * w
    return cdf


def make_table(mu, coeffs, n_channels, eta):
    """coeffs(mu_i, mu_o) -> None or an array (n_channels, m) of Fourier coefficients for the cell (row mu_o, column mu_i). cdf rows integrate a0 over mu_i."""
    mu = np.asarray(mu, F)
    n = len(mu)
    offs, lens, a, m_max = [], [], [], 0
    for o in range(n):
        for i in range(n):
            c = coeffs(float(mu[i]), float(mu[o]))
            if c is None or np.asarray(c).shape[1] == 0:
                offs.append(len(a)); lens.append(0)
                continue
            c = np.asarray(c, F)
            offs.append(len(a)); lens.append(c.shape[1]); a.extend(c.ravel()); m_max = max(m_max, c.shape[1])
    a = np.asarray(a, F)
    t = Table(mu, np.zeros(n * n, F), offs, lens, a, max(m_max, 1), n_channels, eta)
    cdf = np.concatenate([integrate_catmull_rom(mu, t.a0[o * n:(o + 1) * n]) for o in range(n)]).astype(F)
    return Table(mu, cdf, offs, lens, a, max(m_max, 1), n_channels, eta)


def write_table(path, t, **kw):
    return write_bsdf(path, t.mu, t.cdf, t.offset, t.length, t.a, t.m_max, t.n_channels, t.eta, **kw)


def nonuniform_mu(n):
    """n nodes on [-1, 1], denser near 0 and +-1, with -1, 0 and 1 among them."""
    h = np.sin(np.linspace(0.0, np.pi / 2, n // 2 + 1)) if n % 2 else np.sin(np.linspace(0.0, np.pi / 2, n // 2))
    h = np.asarray(h, np.float64) ** 1.3
    return np.unique(np.concatenate([-h, h]).astype(F))


def glossy_table(n_mu=11, m=8, n_channels=1, eta=1.0, varying=True, empty_cells=False):
    """A smooth glossy table: a_k = c (|mu_i mu_o| + 0.1) g^k / (1 + k) with g < 1, non-negative series; the order varies from cell to cell (varying) and some
    cells are empty (empty_cells)."""
    mu = nonuniform_mu(n_mu)

    def coeffs(mi, mo):
        k = np.arange(m if not varying else max(1, int(m - (abs(mi) + abs(mo)) * (m - 1) / 2)))
        if empty_cells and mi * mo > 0 and abs(mi) > 0.6:
            return None
        refl = mi * mo < 0
        base = (abs(mi * mo) + 0.1) * (0.6 if refl else 0.2) * 0.5 ** k / (1.0 + k)
        chans = [base]
        if n_channels == 3:
            chans += [base * 1.2, base * 0.7]
        return np.asarray(chans, F)
    return make_table(mu, coeffs, n_channels, eta)


def lambert_table(rho_rgb, n_mu=41):
    """k = 0 only, a = rho / pi |mu_i| on the reflection side (mu_i mu_o < 0): f = rho / pi there. Three channels: Y such that G comes out as rho_g."""
    mu = np.unique(np.concatenate([nonuniform_mu(n_mu), np.float32([-1e-2, 1e-2])]).astype(F))
    r, g, b = (float(x) for x in rho_rgb)
    y = (g + 0.100913 * b + 0.297375 * r) / 1.39829

    def coeffs(mi, mo):
        if not mi * mo < 0:
            return None
        s = abs(mi) / np.pi
        return np.asarray([[y * s], [r * s], [b * s]], F)
    return make_table(mu, coeffs, 3, 1.0)


# ---------------------------------------------------------------- the restatement (vectorised over n queries)
def find_interval_nodes(nodes, x):
    """find_interval(size, |i| nodes[i] <= x) for ascending nodes."""
    return np.clip(np.searchsorted(nodes, x, side="right") - 1, 0, len(nodes) - 2)


def catmull_rom_weights(nodes, x):
    """-> ok (n,), offset (n,), w (4, n)."""
    x = np.asarray(x, F)
    size = len(nodes)
    ok = (x >= nodes[0]) & (x <= nodes[size - 1])
    idx = find_interval_nodes(nodes, x)
    x0, x1 = nodes[idx], nodes[idx + 1]
    with np.errstate(all="ignore"):
        t = (x - x0) / (x1 - x0)
        t2 = t * t
        t3 = t2 * t
        w = np.zeros((4,) + x.shape, F)
        w[1] = F(2) * t3 - F(3) * t2 + F(1)
        w[2] = F(-2) * t3 + F(3) * t2
        first = idx > 0
        xm1 = nodes[np.maximum(idx - 1, 0)]
        w0a = (t3 - F(2) * t2 + t) * (x1 - x0) / (x1 - xm1)
        w0b = t3 - F(2) * t2 + t
        w[0] = np.where(first, -w0a, F(0))
        w[2] = np.where(first, w[2] + w0a, w[2] + w0b)
        w[1] = np.where(first, w[1], w[1] - w0b)
        last = idx + 2 < size
        xp2 = nodes[np.minimum(idx + 2, size - 1)]
        w3a = (t3 - t2) * (x1 - x0) / (xp2 - x0)
        w3b = t3 - t2
        w[1] = np.where(last, w[1] - w3a, w[1] - w3b)
        w[2] = np.where(last, w[2], w[2] + w3b)
        w[3] = np.where(last, w3a, F(0))
    return ok, idx - 1, w


class Cells:
    """The 16 cells of each query's (mu_i, mu_o) stencil, j = 4 b + a; ak(c, k) as the reference accumulates ak[c mMax + k]."""

    def __init__(self, t, mu_i, mu_o):
        oki, offi, wi = catmull_rom_weights(t.mu, mu_i)
        oko, offo, wo = catmull_rom_weights(t.mu, mu_o)
        self.ok = oki & oko
        self.wo, self.off_o = wo, offo
        n = t.n_mu
        self.w, self.off, self.m = [], [], []
        for b in range(4):
            for a in range(4):
                w = (wi[a] * wo[b]).astype(F)
                use = self.ok & (w != 0)
                cell = np.clip((offo + b) * n + (offi + a), 0, n * n - 1)
                self.w.append(np.where(use, w, F(0)))
                self.off.append(np.where(use, t.offset[cell], 0))
                self.m.append(np.where(use, t.length[cell], 0))
        self.m_max = np.max(np.stack(self.m), 0)
        self.a = t.a

    def ak(self, c, k):
        s = np.zeros(self.m_max.shape, F)
        for w, off, m in zip(self.w, self.off, self.m):
            use = k < m
            if use.any():
                v = self.a[np.where(use, off + c * m + k, 0)]
                s = np.where(use, s + w * v, s)
        return s


def fourier_series(cl, c, cos_phi):
    value = np.zeros(cos_phi.shape, F)
    cos_km1, cos_k = cos_phi.astype(F), np.ones(cos_phi.shape, F)
    for k in range(int(cl.m_max.max(initial=0))):
        value = np.where(k < cl.m_max, value + cl.ak(c, k) * cos_k, value)
        cos_kp1 = F(2) * cos_phi * cos_k - cos_km1
        cos_km1, cos_k = cos_k, cos_kp1
    return value


def cos_d_phi(wa, wb):
    with np.errstate(all="ignore"):
        v = (wa[:, 0] * wb[:, 0] + wa[:, 1] * wb[:, 1]) / np.sqrt((wa[:, 0] * wa[:, 0] + wa[:, 1] * wa[:, 1]) * (wb[:, 0] * wb[:, 0] + wb[:, 1] * wb[:, 1]))
    return np.where(v < F(-1), F(-1), np.where(v > F(1), F(1), v)).astype(F)


def _scale(t, mu_i, mu_o):
    with np.errstate(all="ignore"):
        s = np.where(mu_i != 0, F(1) / np.abs(mu_i), F(0)).astype(F)
        e = np.where(mu_i > 0, F(1) / t.eta, t.eta).astype(F)
    return np.where(mu_i * mu_o > 0, s * (e * e), s).astype(F)


def _rgb(t, cl, y, scale, cos_phi):
    if t.n_channels == 1:
        return np.repeat((y * scale)[:, None], 3, 1)
    r, b = fourier_series(cl, 1, cos_phi), fourier_series(cl, 2, cos_phi)
    g = F(1.39829) * y - F(0.100913) * b - F(0.297375) * r
    out = np.stack([r * scale, g * scale, b * scale], 1)
    return np.where(out < 0, F(0), out).astype(F)  # Spectrum::clamp (NaN stays)


def f(t, wo, wi):
    wo, wi = np.asarray(wo, F), np.asarray(wi, F)
    mu_i, mu_o = -wi[:, 2], wo[:, 2]
    cp = cos_d_phi(-wi, wo)
    cl = Cells(t, mu_i, mu_o)
    y = np.fmax(F(0), fourier_series(cl, 0, cp))
    out = _rgb(t, cl, y, _scale(t, mu_i, mu_o), cp)
    return np.where(cl.ok[:, None], out, F(0)).astype(F)


def pdf(t, wo, wi):
    wo, wi = np.asarray(wo, F), np.asarray(wi, F)
    mu_i, mu_o = -wi[:, 2], wo[:, 2]
    cp = cos_d_phi(-wi, wo)
    cl = Cells(t, mu_i, mu_o)
    rho = np.zeros(mu_o.shape, F)
    n = t.n_mu
    for o in range(4):
        row = np.clip(cl.off_o + o, 0, n - 1)
        rho = np.where(cl.wo[o] != 0, rho + cl.wo[o] * t.cdf[row * n + n - 1] * (F(2) * F(np.pi)), rho)
    y = fourier_series(cl, 0, cp)
    with np.errstate(all="ignore"):
        out = np.where((rho > 0) & (y > 0), y / rho, F(0))
    return np.where(cl.ok, out, F(0)).astype(F)


def sample_catmull_rom_2d(t, alpha, u):
    n = t.n_mu
    ok, off, w = catmull_rom_weights(t.mu, alpha)

    def interp(arr, idx):
        v = np.zeros(alpha.shape, F)
        for i in range(4):
            cell = np.clip((off + i) * n + idx, 0, n * n - 1)
            v = np.where(w[i] != 0, v + arr[cell] * w[i], v)
        return v
    with np.errstate(all="ignore"):
        maximum = interp(t.cdf, np.full(alpha.shape, n - 1))
        u = u * maximum
        first, ln = np.zeros(alpha.shape, np.int64), np.full(alpha.shape, n, np.int64)
        while (ln > 0).any():
            act = ln > 0
            half = ln >> 1
            middle = first + half
            pred = interp(t.cdf, np.minimum(middle, n - 1)) <= u
            first = np.where(act & pred, middle + 1, first)
            ln = np.where(act, np.where(pred, ln - half - 1, half), ln)
        idx = np.clip(first - 1, 0, n - 2)
        f0, f1 = interp(t.a0, idx), interp(t.a0, idx + 1)
        x0, x1 = t.mu[idx], t.mu[idx + 1]
        width = x1 - x0
        u = (u - interp(t.cdf, idx)) / width
        d0 = np.where(idx > 0, width * (f1 - interp(t.a0, np.maximum(idx - 1, 0))) / (x1 - t.mu[np.maximum(idx - 1, 0)]), f1 - f0)
        d1 = np.where(idx + 2 < n, width * (interp(t.a0, np.minimum(idx + 2, n - 1)) - f0) / (t.mu[np.minimum(idx + 2, n - 1)] - x0), f1 - f0)
        tt = np.where(f0 != f1, (f0 - np.sqrt(np.fmax(F(0), f0 * f0 + F(2) * u * (f1 - f0)))) / (f0 - f1), u / f0).astype(F)
        a, b = np.zeros(alpha.shape, F), np.ones(alpha.shape, F)
        Fh, fh = np.zeros(alpha.shape, F), np.zeros(alpha.shape, F)
        done = np.zeros(alpha.shape, bool)
        for it in range(MAX_ITER):
            tt = np.where(~done & ~((tt >= a) & (tt <= b)), F(0.5) * (a + b), tt)
            Fn = tt * (f0 + tt * (F(0.5) * d0 + tt * (F(1.0 / 3.0) * (F(-2) * d0 - d1) + f1 - f0 + tt * (F(0.25) * (d0 + d1) + F(0.5) * (f0 - f1)))))
            fn = f0 + tt * (d0 + tt * (F(-2) * d0 - d1 + F(3) * (f1 - f0) + tt * (d0 + d1 + F(2) * (f0 - f1))))
            Fh, fh = np.where(done, Fh, Fn), np.where(done, fh, fn)
            stop = (np.abs(Fh - u) < F(1e-6)) | (b - a < F(1e-6)) | (it + 1 >= MAX_ITER)
            go = ~done & ~stop
            a = np.where(go & (Fh - u < 0), tt, a)
            b = np.where(go & ~(Fh - u < 0), tt, b)
            tt = np.where(go, tt - (Fh - u) / fh, tt)
            done = done | stop
        x = x0 + width * tt
        p = fh / maximum
    return np.where(ok, x, F(0)).astype(F), np.where(ok, p, F(0)).astype(F)


def sample_fourier(cl, u):
    flip = u >= F(0.5)
    u = np.where(flip, F(1) - F(2) * (u - F(0.5)), u * F(2)).astype(F)
    ak0 = cl.ak(0, 0)
    mm = int(cl.m_max.max(initial=0))
    aks = [cl.ak(0, k) for k in range(mm)]
    a, b = np.zeros(u.shape, F), np.full(u.shape, F(np.pi))
    phi = np.full(u.shape, F(0.5) * F(np.pi))
    Fv, fv = np.zeros(u.shape, F), np.zeros(u.shape, F)
    done = np.zeros(u.shape, bool)
    with np.errstate(all="ignore"):
        for it in range(MAX_ITER):
            cos_phi = np.cos(phi).astype(F)
            sin_phi = np.sqrt(np.fmax(F(0), F(1) - cos_phi * cos_phi))
            cp, cc, sp, sc = cos_phi, np.ones(u.shape, F), -sin_phi, np.zeros(u.shape, F)
            Fn, fn = ak0 * phi, ak0.copy()
            for k in range(1, mm):
                sn = F(2) * cos_phi * sc - sp
                cn = F(2) * cos_phi * cc - cp
                sp, sc, cp, cc = sc, sn, cc, cn
                use = k < cl.m_max
                Fn = np.where(use, Fn + aks[k] * (F(1) / F(k)) * sn, Fn)
                fn = np.where(use, fn + aks[k] * cn, fn)
            Fn = Fn - u * ak0 * F(np.pi)
            Fv, fv = np.where(done, Fv, Fn), np.where(done, fv, fn)
            b = np.where(~done & (Fv > 0), phi, b)
            a = np.where(~done & ~(Fv > 0), phi, a)
            stop = (np.abs(Fv) < F(1e-6)) | (b - a < F(1e-6)) | (it + 1 >= MAX_ITER)
            go = ~done & ~stop
            nphi = phi - Fv / fv
            nphi = np.where(~((nphi > a) & (nphi < b)), F(0.5) * (a + b), nphi)
            phi = np.where(go, nphi, phi).astype(F)
            done = done | stop
        phi = np.where(flip, F(2) * F(np.pi) - phi, phi).astype(F)
        p = F(0.15915494309189533577) * fv / ak0
    return fv, p, phi


def sample_f(t, wo, u):
    """-> f (n, 3), wi (n, 3), pdf (n,)."""
    wo, u = np.asarray(wo, F), np.asarray(u, F)
    mu_o = wo[:, 2]
    mu_i, pdf_mu = sample_catmull_rom_2d(t, mu_o, u[:, 1])
    cl = Cells(t, mu_i, mu_o)
    y, pdf_phi, phi = sample_fourier(cl, u[:, 0])
    with np.errstate(all="ignore"):
        p = np.fmax(F(0), pdf_phi * pdf_mu)
        sin2_i = np.fmax(F(0), F(1) - mu_i * mu_i)
        norm = np.sqrt(sin2_i / np.fmax(F(1) - mu_o * mu_o, F(0)))
        norm = np.where(np.isinf(norm), F(0), norm).astype(F)
        sn, cs = np.sin(phi).astype(F), np.cos(phi).astype(F)
        wi = -np.stack([norm * (cs * wo[:, 0] - sn * wo[:, 1]), norm * (sn * wo[:, 0] + cs * wo[:, 1]), mu_i], 1)
        wi = wi / np.sqrt((wi * wi).sum(1, dtype=F))[:, None]
        fv = _rgb(t, cl, y, _scale(t, mu_i, mu_o), cs)
    ok = cl.ok
    return (np.where(ok[:, None], fv, F(0)).astype(F), np.where(ok[:, None], wi, F(0)).astype(F), np.where(ok, p, F(0)).astype(F))
