"""Float64 numpy model of the code between a hit and the BSDF's local frame: the shading frame of Bsdf::new, material::bump with set_shading_geometry, and
Bsdf::f / pdf / sample_f over lobes whose value is a closed form (Lambert reflection and transmission, perfect mirror, FresnelSpecular, specular transmission).
Written from the reference's definitions (rustracer-core/src: material/mod.rs, interaction.rs, bsdf/mod.rs, bsdf/bxdf.rs, bsdf/lambertian.rs, bsdf/fresnel.rs,
sampling/mod.rs, material/mixmat.rs), not from oracle/ or the device headers. Everything is vectorised over n queries; records are the 40-float surface records of
rt_bsdf_eval (include/rtx_hip.h), directions are world space.

Reference quirks the model carries (file:line of the reference):
  - bsdf/mod.rs:82-88    the frame is ss = normalize(shading.dpdu), ns = shading.n as given, ts = cross(ns, ss): no re-orthogonalisation, ns is not normalised.
  - bsdf/mod.rs:253-263  world_to_local is three dot products, local_to_world the combination ss x + ts y + ns z: for a record whose shading dpdu is not
                         perpendicular to its shading n (or whose ns is not unit) local_to_world IS NOT THE INVERSE of world_to_local, and local vectors of unit
                         world directions are not unit.
  - bsdf/mod.rs:100,230  reflection or transmission is chosen by the GEOMETRIC normal (dot(wi, ng) dot(wo, ng) > 0) while every lobe works in the shading frame.
  - bsdf/mod.rs:97,118,181  wo_local.z == 0: f and pdf are 0, sample_f returns no sample but the chosen lobe's type flags.
  - bsdf/mod.rs:202-208  a sampled pdf of 0 returns type flags 0.
  - bsdf/mod.rs:213-226  a specular sample's pdf is not summed with the other lobes' but still divided by the number of matching lobes; its f is not re-summed.
  - bsdf/bxdf.rs:18-25   the default BxDF::sample_f reports BxDFType::empty(): a sampled Lambert lobe carries type flags 0.
  - bsdf/lambertian.rs:39-47  LambertianTransmission overrides neither sample_f nor pdf: it samples wo's own hemisphere and its pdf is non-zero on wo's side only.
  - bsdf/fresnel.rs:19-30  refract does not clamp cos_theta_i; fr_dielectric (:33-58) does.
  - bsdf/fresnel.rs:202-229  SpecularTransmission at eta_a = eta_b = 1 (uber below full opacity, material/uber.rs:83) passes straight through: wi_local = -wo_local.
  - bsdf/fresnel.rs:315-322  FresnelSpecular whose refraction fails returns pdf 0 - no sample.
  - material/mod.rs:55-73  the bump shift is du = 0.5 (|dudx| + |dudy|), 0.0005 where that is zero (dv likewise); the shifted lookups keep the record's differentials.
  - material/mod.rs:83-88  the slopes push along shading.n AS GIVEN, which need not be normalize(cross(shading.dpdu, shading.dpdv)).
  - interaction.rs:227-235  the bumped normal is normalize(cross(dpdu', dpdv')), negated under reverse_orientation ^ swaps_handedness, then turned to n_geom's side:
                         a constant displacement replaces the record's own shading n by +-normalize(cross(shading.dpdu, shading.dpdv)).
  - material/mixmat.rs:43-63  mix(A, B): B works on a clone taken before A; the Bsdf (frame, eta) is A's - the interaction after A's bump -, B's bump reaches nothing
                         but the textures B reads (which read uv and p, not the shading geometry: nothing).
"""
import numpy as np

REFLECTION, TRANSMISSION, DIFFUSE, GLOSSY, SPECULAR = 1, 2, 4, 8, 16
ONE_MINUS_EPSILON = float(np.float32(1.0) - np.float32(2.0 ** -24))   # lib.rs: f32::EPSILON-based 1 - 2^-24
# columns of a surface record
P, NG, NS, DPDU, DPDV, SDU, SDV = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), slice(12, 15), slice(15, 18), slice(18, 21)
UV, DPDX, DPDY = slice(27, 29), slice(33, 36), slice(36, 39)
DUDX, DVDX, DUDY, DVDY, FLIP = 29, 30, 31, 32, 39


def dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def unit(v):
    return v / np.sqrt(dot(v, v))[..., None]


# ---------------------------------------------------------------------------------------------- the frame (Bsdf::new)
def frame(record):
    """Bsdf::new of a record: dict(ss, ts, ns, ng) in float64. ss = normalize(sh_dpdu), ns = sh_n as given, ts = cross(ns, ss) - not re-orthogonalised, ns not
    normalised: for a record whose sh_dpdu is not perpendicular to sh_n, local_to_world below is NOT the inverse of world_to_local (bsdf/mod.rs:253-263)."""
    r = np.asarray(record, np.float64)
    ss = unit(r[..., SDU])
    ns = r[..., NS]
    return dict(ss=ss, ts=np.cross(ns, ss), ns=ns, ng=r[..., NG])


def world_to_local(fr, w):
    return np.stack([dot(w, fr["ss"]), dot(w, fr["ts"]), dot(w, fr["ns"])], -1)


def local_to_world(fr, v):
    return fr["ss"] * v[..., 0:1] + fr["ts"] * v[..., 1:2] + fr["ns"] * v[..., 2:3]


# ---------------------------------------------------------------------------------------------- material::bump
def bump_lookups(record):
    """Where material::bump looks its displacement up, in float32 as the device forms it (each quantity is one rounding): dict(du, dv (n,), uv (n, 2) the record's
    own, uv_u = uv + (du, 0), uv_v = uv + (0, dv)). The shifted lookups keep the record's differentials."""
    r = np.asarray(record, np.float32)
    half, tiny = np.float32(0.5), np.float32(0.0005)
    du = half * (np.abs(r[..., DUDX]) + np.abs(r[..., DUDY]))
    dv = half * (np.abs(r[..., DVDX]) + np.abs(r[..., DVDY]))
    du = np.where(du == 0, tiny, du).astype(np.float32)
    dv = np.where(dv == 0, tiny, dv).astype(np.float32)
    uv = r[..., UV]
    uv_u = np.stack([uv[..., 0] + du, uv[..., 1]], -1).astype(np.float32)
    uv_v = np.stack([uv[..., 0], uv[..., 1] + dv], -1).astype(np.float32)
    return dict(du=du, dv=dv, uv=uv, uv_u=uv_u, uv_v=uv_v)


def bump(record, d, d_u, d_v):
    """material::bump + set_shading_geometry(.., false) in float64: d, d_u, d_v the displacement at the record's uv and at the two shifted lookups of bump_lookups
    (analytic, or read from a texture evaluator at those points). Returns (the record with sh_n, sh_dpdu, sh_dpdv replaced - float64 -, dot(n', n_geom) before
    face_forward: the side decision)."""
    r = np.array(record, np.float64)
    lk = bump_lookups(record)
    du, dv = lk["du"].astype(np.float64), lk["dv"].astype(np.float64)
    d, d_u, d_v = (np.asarray(x, np.float64) for x in (d, d_u, d_v))
    ns = r[..., NS]
    dpdu = r[..., SDU] + ((d_u - d) / du)[..., None] * ns      # dndu = dndv = 0
    dpdv = r[..., SDV] + ((d_v - d) / dv)[..., None] * ns
    n = unit(np.cross(dpdu, dpdv))
    n = np.where((r[..., FLIP] != 0)[..., None], -n, n)
    side = dot(n, r[..., NG])
    n = np.where((side < 0)[..., None], -n, n)                  # face_forward_n(shading.n, hit.n)
    r[..., NS], r[..., SDU], r[..., SDV] = n, dpdu, dpdv
    return r, side


# ---------------------------------------------------------------------------------------------- lobes
class Lobe:
    """kind: "lambert_r", "lambert_t", "mirror" (SpecularReflection, FresnelNoOp), "spec_t" (SpecularTransmission), "fresnel_spec". r, t: rgb, (3,) or (n, 3)."""

    def __init__(self, kind, r=None, t=None, eta_a=1.0, eta_b=1.0):
        self.kind, self.eta_a, self.eta_b = kind, float(eta_a), float(eta_b)
        self.r = None if r is None else np.asarray(r, np.float64)
        self.t = None if t is None else np.asarray(t, np.float64)
        self.type = {"lambert_r": DIFFUSE | REFLECTION, "lambert_t": DIFFUSE | TRANSMISSION, "mirror": SPECULAR | REFLECTION, "spec_t": SPECULAR | TRANSMISSION,
                     "fresnel_spec": SPECULAR | REFLECTION | TRANSMISSION}[kind]


def fr_dielectric(cos_i, eta_i, eta_t):
    """fresnel.rs:33-58, float64, vectorised over cos_i."""
    c = np.clip(np.asarray(cos_i, np.float64), -1.0, 1.0)
    leaving = c <= 0
    ei, et = np.where(leaving, eta_t, eta_i), np.where(leaving, eta_i, eta_t)
    c = np.abs(c)
    sin_i = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    sin_t = ei / et * sin_i
    cos_t = np.sqrt(np.maximum(0.0, 1.0 - sin_t * sin_t))
    with np.errstate(divide="ignore", invalid="ignore"):
        r_parl = (et * c - ei * cos_t) / (et * c + ei * cos_t)
        r_perp = (ei * c - et * cos_t) / (ei * c + et * cos_t)
    return np.where(sin_t >= 1.0, 1.0, 0.5 * (r_parl * r_parl + r_perp * r_perp))


def refract(i, n, eta):
    """fresnel.rs:19-30: (wi (n, 3), ok (n,), the discriminant 1 - sin^2 theta_t)."""
    cos_i = dot(n, i)
    sin2_t = eta * eta * np.maximum(0.0, 1.0 - cos_i * cos_i)
    disc = 1.0 - sin2_t
    cos_t = np.sqrt(np.maximum(disc, 0.0))
    return np.asarray(eta)[..., None] * -i + (eta * cos_i - cos_t)[..., None] * n, sin2_t < 1.0, disc


def concentric_sample_disk(u):
    """sampling/mod.rs:28-47 in float64."""
    o = 2.0 * np.asarray(u, np.float64) - 1.0
    x, y = o[..., 0], o[..., 1]
    wide = np.abs(x) > np.abs(y)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(wide, x, y)
        theta = np.where(wide, np.pi / 4 * (y / x), np.pi / 2 - np.pi / 4 * (x / y))
    d = np.stack([r * np.cos(theta), r * np.sin(theta)], -1)
    return np.where(((x == 0) & (y == 0))[..., None], 0.0, d)


def cosine_sample_hemisphere(u):
    d = concentric_sample_disk(u)
    z = np.sqrt(np.maximum(0.0, 1.0 - d[..., 0] ** 2 - d[..., 1] ** 2))
    return np.concatenate([d, z[..., None]], -1)


def _rgb(c, n):
    return np.broadcast_to(c, (n, 3)).astype(np.float64)


def lobe_f(l, wo, wi):
    n = wo.shape[0]
    if l.kind == "lambert_r":
        return _rgb(l.r, n) / np.pi
    if l.kind == "lambert_t":
        return _rgb(l.t, n) / np.pi
    return np.zeros((n, 3))


def lobe_pdf(l, wo, wi):
    if l.kind in ("lambert_r", "lambert_t"):   # the default BxDF::pdf, bxdf.rs:38-44
        return np.where(wo[:, 2] * wi[:, 2] > 0, np.abs(wi[:, 2]) / np.pi, 0.0)
    return np.zeros(wo.shape[0])


def lobe_sample_f(l, wo, u):
    """BxDF::sample_f in the local frame: (f (n, 3), wi (n, 3), pdf (n,), type (n,) int, disc (n,) - the refraction discriminant where one is taken, else +inf)."""
    n = wo.shape[0]
    inf = np.full(n, np.inf)
    if l.kind in ("lambert_r", "lambert_t"):
        wi = cosine_sample_hemisphere(u)
        wi[:, 2] = np.where(wo[:, 2] < 0, -wi[:, 2], wi[:, 2])
        return lobe_f(l, wo, wi), wi, lobe_pdf(l, wo, wi), np.zeros(n, np.int64), inf
    mirror_wi = wo * np.array([-1.0, -1.0, 1.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        if l.kind == "mirror":
            return _rgb(l.r, n) / np.abs(mirror_wi[:, 2:3]), mirror_wi, np.ones(n), np.full(n, l.type), inf
        entering = wo[:, 2] > 0
        eta_i, eta_t = np.where(entering, l.eta_a, l.eta_b), np.where(entering, l.eta_b, l.eta_a)
        nrm = np.zeros((n, 3))
        nrm[:, 2] = np.where(wo[:, 2] < 0, -1.0, 1.0)          # face_forward((0, 0, 1), wo)
        wt, ok, disc = refract(wo, nrm, eta_i / eta_t)
        scale = (eta_i * eta_i) / (eta_t * eta_t)                # TransportMode::RADIANCE
        if l.kind == "spec_t":
            ft = _rgb(l.t, n) * (1.0 - fr_dielectric(np.abs(wt[:, 2]), l.eta_a, l.eta_b))[:, None] * scale[:, None]
            f = np.where(ok[:, None], ft / np.abs(wt[:, 2:3]), 1.0)
            return f, np.where(ok[:, None], wt, 0.0), np.where(ok, 1.0, 0.0), np.where(ok, l.type, 0), disc
        fr = fr_dielectric(wo[:, 2], l.eta_a, l.eta_b)
        refl = np.asarray(u, np.float64)[:, 0] < fr.astype(np.float32).astype(np.float64)   # the choice on the float32 F
        f_r = fr[:, None] * _rgb(l.r, n) / np.abs(mirror_wi[:, 2:3])
        f_t = np.where(ok[:, None], _rgb(l.t, n) * (1.0 - fr)[:, None] * scale[:, None] / np.abs(wt[:, 2:3]), 0.0)
        f = np.where(refl[:, None], f_r, f_t)
        wi = np.where(refl[:, None], mirror_wi, np.where(ok[:, None], wt, 0.0))
        pdf = np.where(refl, fr, np.where(ok, 1.0 - fr, 0.0))
        typ = np.where(refl, SPECULAR | REFLECTION, np.where(ok, SPECULAR | TRANSMISSION, 0))
        return f, wi, pdf, typ, np.where(refl | (fr >= 1.0), np.inf, disc)


# ---------------------------------------------------------------------------------------------- Bsdf::f / pdf / sample_f (flags = ALL: every lobe matches)
def bsdf_f(fr, lobes, wo_w, wi_w):
    wo_w, wi_w = np.asarray(wo_w, np.float64), np.asarray(wi_w, np.float64)
    wo, wi = world_to_local(fr, wo_w), world_to_local(fr, wi_w)
    reflect = dot(wi_w, fr["ng"]) * dot(wo_w, fr["ng"]) > 0
    f = np.zeros((wo.shape[0], 3))
    for l in lobes:
        use = np.where(reflect, (l.type & REFLECTION) != 0, (l.type & TRANSMISSION) != 0)
        f = f + np.where(use[:, None], lobe_f(l, wo, wi), 0.0)
    return np.where((wo[:, 2] == 0)[:, None], 0.0, f)


def bsdf_pdf(fr, lobes, wo_w, wi_w):
    wo, wi = world_to_local(fr, np.asarray(wo_w, np.float64)), world_to_local(fr, np.asarray(wi_w, np.float64))
    if not lobes:
        return np.zeros(wo.shape[0])
    pdf = sum(lobe_pdf(l, wo, wi) for l in lobes) / len(lobes)
    return np.where(wo[:, 2] == 0, 0.0, pdf)


def bsdf_sample_f(fr, lobes, wo_w, u):
    """Bsdf::sample_f: dict(f (n, 3), wi (n, 3) world, pdf (n,), type (n,), wi_local (n, 3), disc (n,)). u float32 values: u.x * m is exact for m in 1, 2, 4."""
    wo_w = np.asarray(wo_w, np.float64)
    u = np.asarray(u, np.float64)
    n, m = wo_w.shape[0], len(lobes)
    zero = dict(f=np.zeros((n, 3)), wi=np.zeros((n, 3)), pdf=np.zeros(n), type=np.zeros(n, np.int64), wi_local=np.zeros((n, 3)), disc=np.full(n, np.inf),
                chosen=np.zeros(n, np.int64))
    if m == 0:
        return zero
    assert m in (1, 2, 4)
    comp = np.minimum(np.floor(u[:, 0] * m).astype(np.int64), m - 1)
    ur = np.stack([np.minimum(u[:, 0] * m - comp, ONE_MINUS_EPSILON), u[:, 1]], -1)
    wo = world_to_local(fr, wo_w)
    out = zero
    for k, l in enumerate(lobes):
        f, wi, pdf, typ, disc = lobe_sample_f(l, wo, ur)
        live = pdf != 0                             # the SAMPLED lobe's own pdf == 0: no sample, type flags 0
        wi_w = local_to_world(fr, wi)
        specular = (l.type & SPECULAR) != 0
        if not specular:
            pdf = pdf + sum(lobe_pdf(o, wo, wi) for j, o in enumerate(lobes) if j != k)
            reflect = dot(wi_w, fr["ng"]) * dot(wo_w, fr["ng"]) > 0
            f = np.zeros((n, 3))
            for o in lobes:
                use = np.where(reflect, (o.type & REFLECTION) != 0, (o.type & TRANSMISSION) != 0)
                f = f + np.where(use[:, None], lobe_f(o, wo, wi), 0.0)
        pdf = pdf / m
        mine = comp == k
        flat = wo[:, 2] == 0                        # no sample, the chosen lobe's type flags
        sel = mine & live & ~flat
        out = dict(f=np.where(sel[:, None], f, out["f"]), wi=np.where(sel[:, None], wi_w, out["wi"]), pdf=np.where(sel, pdf, out["pdf"]),
                   type=np.where(sel, typ, np.where(mine & flat, l.type, out["type"])), wi_local=np.where(sel[:, None], wi, out["wi_local"]),
                   disc=np.where(mine, disc, out["disc"]), chosen=np.where(mine, l.type, out["chosen"]))
    return out


def evaluate(record, lobes, wo_w, wi_w, u):
    """The 13 columns of rt_bsdf_eval from the model: f rgb, pdf, sampled f rgb, wi xyz, pdf, type flags, lobe count - float64 - and the sample dict."""
    fr = frame(record)
    s = bsdf_sample_f(fr, lobes, wo_w, u)
    n = np.asarray(wo_w).shape[0]
    out = np.concatenate([bsdf_f(fr, lobes, wo_w, wi_w), bsdf_pdf(fr, lobes, wo_w, wi_w)[:, None], s["f"], s["wi"], s["pdf"][:, None],
                          s["type"][:, None].astype(np.float64), np.full((n, 1), float(len(lobes)))], -1)
    return out, s
