"""rt_bsdf_eval and rt_render_samples on the GPU: the shade stage held to the oracle query by query and sample by sample, not only through filtered films.

BSDF: the oracle's orc_bsdf_probe (canonical hit) against HostScene.bsdf_eval on the same SceneDesc; the register-resident front-ends against the generic one bit
for bit; surface records against rt_texture_eval and under rigid rotations. Samples: OracleScene.li_keyed against HostScene.render_samples, and the samples against
the frame rt_render makes of them. Every figure is printed before it is asserted (MEASUREMENTS.md records them)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from util import bits, tables_from_perm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSDF_SPECULAR = 16
N_QUERIES = 2048

KAT = ["matte", "oren", "plastic", "metal", "mirror", "glass", "rough_glass", "uber", "substrate", "translucent", "disney", "disney_cc", "disney_thin", "mix"]
ALPHAS = ["plastic_a0.02", "plastic_a0.054", "plastic_a1", "metal_a0.02", "metal_a0.054", "metal_a1"]
SHARP = ["plastic_a0.02", "plastic_a0.001", "plastic_a0.0001", "metal_a0.02", "metal_a0.001", "metal_a0.0001"]


def _material_desc():
    """The materials of tests/test_oracle_kat.py::material_scene, in its order, plus plastic and metal with un-remapped microfacet roughness (alpha itself)."""
    from rustracer_amd.scene_desc import SceneDesc
    s = SceneDesc()
    mats = dict(
        matte=s.matte((0.8, 0.6, 0.4)), oren=s.matte((0.8, 0.6, 0.4), sigma=20.0), plastic=s.plastic((0.3, 0.3, 0.3), (0.4, 0.4, 0.4), 0.1),
        metal=s.metal(roughness=0.05), mirror=s.mirror(0.9), glass=s.glass(), rough_glass=s.glass(urough=0.1, vrough=0.1),
        uber=s.uber(kr=0.2, kt=0.1), substrate=s.substrate(), translucent=s.translucent(),
        disney=s.disney((0.7, 0.4, 0.3), roughness=0.4, sheen=0.5), disney_cc=s.disney((0.5, 0.5, 0.6), metallic=0.7, roughness=0.3, anisotropic=0.5, clearcoat=1.0, clearcoatgloss=0.6),
        disney_thin=s.disney((0.6, 0.6, 0.4), thin=True, flatness=0.5, spectrans=0.4, roughness=0.3))
    mats["mix"] = s.mix(mats["matte"], mats["plastic"], 0.3)
    for a in (0.02, 0.054, 1.0, 0.001, 0.0001):
        mats[f"plastic_a{a:g}"] = s.plastic((0.3, 0.3, 0.3), (0.4, 0.4, 0.4), a, remap=False)
        mats[f"metal_a{a:g}"] = s.metal(roughness=a, remap=False)
    s.add_quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), mats["matte"])
    return s, mats


@pytest.fixture(scope="module")
def pair(gpu_host, orc):
    s, mats = _material_desc()
    h = gpu_host.HostScene(s)
    h.upload(0)
    return orc.OracleScene(s), h, mats


def _dirs(rng, n):
    """Unit vectors over the whole sphere, both hemispheres; the first 3/16 grazing, |cos| in {1e-3, 3e-3, 1e-2}."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    g = 3 * n // 16
    z = np.resize(np.array([1e-3, -1e-3, 3e-3, -3e-3, 1e-2, -1e-2]), g)
    phi = rng.uniform(0, 2 * np.pi, g)
    r = np.sqrt(1 - z * z)
    d[:g] = np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)
    return np.ascontiguousarray(d, np.float32)


def _us(rng, n):
    u = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    u = np.minimum(u, np.float32(0.99999994))
    edge = np.float32([0.0, 0.99999994, 0.5, 0.49999997, 5.9604645e-08])
    k = n // 8
    u[:k, 0] = np.resize(edge, k)
    u[k:2 * k, 1] = np.resize(edge, k)
    u[2 * k:2 * k + 25] = np.stack(np.meshgrid(edge, edge), -1).reshape(-1, 2)
    return u


def _oracle(orc, osc, mat, wo, wi, u):
    n = wo.shape[0]
    out = np.zeros((n, 13), np.float32)
    f, smp, pdf = np.zeros(3, np.float32), np.zeros(8, np.float32), C.c_float()
    fp, sp = f.ctypes.data_as(C.POINTER(C.c_float)), smp.ctypes.data_as(C.POINTER(C.c_float))
    probe = orc.lib().orc_bsdf_probe
    P = C.POINTER(C.c_float)
    for i in range(n):
        nl = probe(osc.h, mat, wo[i].ctypes.data_as(P), wi[i].ctypes.data_as(P), u[i].ctypes.data_as(P), fp, C.byref(pdf), sp)
        out[i, 0:3], out[i, 3], out[i, 4:12], out[i, 12] = f, pdf.value, smp, nl
    return out


def _within(dev, ref, rtol, atol=0.0):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    both_nan = np.isnan(dev) & np.isnan(ref)
    return both_nan | (np.abs(dev - ref) <= rtol * np.abs(ref) + atol)


def _excess(dev, ref, rtol, atol=0.0):
    """For the printed tables: (the largest |dev - ref| / (|ref| + atol / rtol) - the relative difference the bound `rtol |ref| + atol` compares with rtol -, the
    largest absolute difference). rtol == 0: an absolute bound, the first figure is 0."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    d = np.abs(dev - ref)
    d = np.where(np.isnan(dev) & np.isnan(ref), 0.0, d)
    if not d.size:
        return 0.0, 0.0
    if rtol == 0:
        return 0.0, float(np.max(d))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(d == 0, 0.0, d / (np.abs(ref) + atol / rtol))
    return float(np.max(rel)), float(np.max(d))


# ---------------------------------------------------------------------------------------------- item 4: oracle parity, query by query
def _cases(names, findings):
    """Parametrised cases; a case named in `findings` is a measured finding of these comparisons (MEASUREMENTS.md): it keeps its bound and is expected to miss it."""
    return [pytest.param(n, marks=pytest.mark.xfail(strict=True, reason=findings[n])) if n in findings else n for n in names]


def _queries(names, name):
    rng = np.random.default_rng(1000 + names.index(name))
    return _dirs(rng, N_QUERIES), _dirs(rng, N_QUERIES)[::-1].copy(), _us(rng, N_QUERIES)


# The rim of the cosine-sampled disk (MEASUREMENTS.md "Per-query BSDF and per-sample radiance"). cosine_sample_hemisphere returns z = sqrt(1 - x^2 - y^2): towards the rim
# the difference cancels, and a last bit or two of sinf / cosf - x^2 + y^2 off by a few ulp of 1 - moves wi.z by 6e-8 / |wi.z|: past the issue's 1e-6
# below |wi.z| = 0.06, and across zero at the rim itself (u.x = 0: one side draws z = 0, pdf 0, no sample; the other z = sqrt(2^-23) = 3.4e-4, a sample). So the sample
# comparison PARTITIONS the queries by the smaller |wi.z| either side sampled (canonical frame: world z is the lobe's z):
#   |wi.z| >= RIM_Z - the issue's bounds: type flags equal, wi within 1e-6, f and pdf within 1e-4 relative;
#   below (the rim set, ~270 of 2048 queries) - type flags equal and wi.xy within 1e-6 all the same; z^2 within RIM_Z2 = 5e-7 (4 ulp of 1: two last bits in each of
#   sinf and cosf - measured 2.4e-7); f and pdf within 1e-4 + 4 |dz| / |z| relative (the lobes are rational in cos(theta_i) of degree <= 2 either way: 1 / (4 cos cos),
#   G1's tan^2, the cosine pdf; measured <= 0.7 of it); sampled by one side only solely where the sampling side's z^2 <= RIM_Z2 (measured 3.5e-4 = sqrt(2^-23)).
RIM_Z, RIM_Z2 = 0.06, 5e-7
_AT_002S = "alpha = 0.02 is not BELOW the sharp-lobe threshold of rtx_dev_bsdf.h (v_rsq_f32 normalisation of the half vector): "
SAMPLE_FINDINGS = {
    "plastic_a0.02": _AT_002S + "sampled f 5.1e-4 relative off in 8 of 2048 queries away from the rim (bound 1e-4); wi, pdf and type flags agree",
    "metal_a0.02": _AT_002S + "sampled f 5.8e-4 relative off in 13 of 2048 queries (bound 1e-4); wi within 3e-8, pdf within 6.5e-7",
    "rough_glass": "sampled f 1.2e-4 relative off in 4 of 2048 queries (bound 1e-4, no absolute term), all at u.x next to 1 where f is 5e-7 and wi.z = -0.6 / -0.7; wi to the last bit, pdf 4.8e-7",
}
VALUE_FINDINGS = {"plastic_a0.054": "pdf(wo, wi) 1.46e-5 relative off in 1 of 2048 queries (bound 1e-5 + 1e-7); f within 3.5e-6"}


@pytest.mark.parametrize("name", _cases(KAT + ALPHAS, VALUE_FINDINGS))
def test_bsdf_values_match_the_oracle_query_by_query(pair, orc, name):
    """Lobe count equal, f and pdf within 1e-5 relative + 1e-7: generic front-end, canonical hit, 2048 queries over the whole sphere with grazing directions."""
    osc, h, mats = pair
    wo, wi, u = _queries(KAT + ALPHAS, name)
    ref = _oracle(orc, osc, mats[name], wo, wi, u)
    dev = h.bsdf_eval(mats[name], wo, wi, u, front_end="generic")["raw"]
    fig = dict(f=_excess(dev[:, 0:3], ref[:, 0:3], 1e-5, 1e-7), pdf=_excess(dev[:, 3], ref[:, 3], 1e-5, 1e-7))
    print(f"\nBSDF-VALUES {name:16s} " + " ".join(f"{k}: rel {v[0]:.2e} abs {v[1]:.2e}" for k, v in fig.items()) + f" lobes_differ {int((dev[:, 12] != ref[:, 12]).sum())}")
    assert np.array_equal(dev[:, 12], ref[:, 12]), "lobe counts"
    assert _within(dev[:, 0:3], ref[:, 0:3], 1e-5, 1e-7).all(), ("f", fig["f"])
    assert _within(dev[:, 3], ref[:, 3], 1e-5, 1e-7).all(), ("pdf", fig["pdf"])


def _rel64(d, r):
    d, r = np.asarray(d, np.float64), np.asarray(r, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == r, 0.0, np.abs(d - r) / np.abs(r))


def _check_samples(tag, name, dev, ref, values=True):
    """The partitioned sample comparison described above; values=False: direction and type flags only. Prints the figures, then asserts."""
    d, r = dev.astype(np.float64), ref.astype(np.float64)
    sd, sr = d[:, 10] > 0, r[:, 10] > 0
    zmin = np.minimum(np.where(sd, np.abs(d[:, 9]), np.inf), np.where(sr, np.abs(r[:, 9]), np.inf))
    rim = zmin < RIM_Z
    out, one, both = ~rim, rim & (sd != sr), rim & sd & sr
    dw = np.abs(d[:, 7:10] - r[:, 7:10])
    relf, relp = _rel64(d[:, 4:7], r[:, 4:7]).max(1), _rel64(d[:, 10], r[:, 10])
    z2 = np.abs(d[:, 9] ** 2 - r[:, 9] ** 2)
    dz, zm = dw[:, 2], np.minimum(np.abs(d[:, 9]), np.abs(r[:, 9]))
    tol = np.where(zm > 0, 1e-4 + 4.0 * dz / np.maximum(zm, 1e-300), np.inf)   # (z = 0 on a side that sampled: only among the one-sided queries)
    one_z2 = np.where(sd, d[:, 9], r[:, 9]) ** 2
    mx = lambda v, m: float(v[m].max()) if m.any() else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):   # (inf / inf among the one-sided queries, which the masks leave out)
        f_of, p_of = relf / tol, relp / tol
    print(f"\n{tag} {name:16s} away from the rim {int(out.sum())}: wi {mx(dw.max(1), out):.2e} f {mx(relf, out):.2e} pdf {mx(relp, out):.2e} types differ {int((d[out, 11] != r[out, 11]).sum())} | "
          f"rim both-sided {int(both.sum())}: wi.xy {mx(dw[:, :2].max(1), both):.2e} z^2 {mx(z2, both):.2e} wi.z {mx(dz, both):.2e} f / its bound {mx(f_of, both):.2f} pdf / its bound {mx(p_of, both):.2f} | "
          f"one-sided {int(one.sum())}: z^2 {mx(one_z2, one):.2e}")
    assert out.sum() > dev.shape[0] // 2
    # away from the rim: the issue's bounds
    assert np.array_equal(d[out, 11], r[out, 11]), "sampled type flags"
    assert (dw[out] <= 1e-6).all(), ("sampled wi", mx(dw.max(1), out))
    if values:
        assert (relf[out] <= 1e-4).all(), ("sampled f", mx(relf, out))
        assert (relp[out] <= 1e-4).all(), ("sampled pdf", mx(relp, out))
    # the rim set
    assert np.array_equal(d[both, 11], r[both, 11]), "sampled type flags at the rim"
    assert (dw[both, :2] <= 1e-6).all() and (z2[both] <= RIM_Z2).all() and (np.sign(d[both, 9]) == np.sign(r[both, 9])).all(), ("sampled wi at the rim", mx(dw[:, :2].max(1), both), mx(z2, both))
    assert (one_z2[one] <= RIM_Z2).all(), ("sampled by one side only away from z = 0", mx(one_z2, one))
    if values:
        assert (relf[both] <= tol[both]).all(), ("sampled f at the rim", mx(f_of, both))
        assert (relp[both] <= tol[both]).all(), ("sampled pdf at the rim", mx(p_of, both))


@pytest.mark.parametrize("name", _cases(KAT + ALPHAS, SAMPLE_FINDINGS))
def test_bsdf_samples_match_the_oracle_query_by_query(pair, orc, name):
    """sample_f on the same 2048 queries, u in [0, 1)^2 including 0 and values next to 1 (and next to 1/2): sampled type flags equal, wi within 1e-6 per component,
    f and pdf within 1e-4 relative of the oracle's sampled values - on every query whose sampled direction keeps |wi.z| >= 0.06; the stated looser bounds on the rest
    (the rim of the cosine-sampled disk, see RIM_Z above)."""
    osc, h, mats = pair
    wo, wi, u = _queries(KAT + ALPHAS, name)
    ref = _oracle(orc, osc, mats[name], wo, wi, u)
    dev = h.bsdf_eval(mats[name], wo, wi, u, front_end="generic")["raw"]
    _check_samples("BSDF-SAMPLES", name, dev, ref)


# ---------------------------------------------------------------------------------------------- item 5: the sharp-lobe rule, per query
def _sharp_queries(name):
    alpha = float(name.split("_a")[1])
    rng = np.random.default_rng(2000 + SHARP.index(name))
    n = N_QUERIES
    wo = rng.normal(size=(n, 3))
    wo[:, 2] = np.abs(wo[:, 2]) + 0.05
    wo[n // 2:, 2] *= -1                                  # both sides
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    wi = wo * np.array([-1.0, -1.0, 1.0]) + rng.normal(size=(n, 3)) * (2.0 * alpha)   # the mirror direction, a few alpha around it
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    return np.ascontiguousarray(wo, np.float32), np.ascontiguousarray(wi, np.float32), _us(rng, n)


_AT_002 = "alpha = 0.02 is not BELOW the sharp-lobe threshold (rtx_dev_bsdf.h sharp_lobe): near the mirror direction one ulp in the half vector's length moves D by 1e-7 / alpha^2; "
SHARP_VALUE_FINDINGS = {"plastic_a0.02": _AT_002 + "f and pdf 4.3e-4 relative off (bound 1e-5)", "metal_a0.02": _AT_002 + "f and pdf 4.3e-4 relative off (bound 1e-5)"}
SHARP_F_AT_FINDINGS = {"plastic_a0.02": _AT_002 + "sampled f 5.8e-4 relative off the oracle's f at the device's wi (bound 1e-5)",
                       "metal_a0.02": _AT_002 + "sampled f 5.2e-4 relative off the oracle's f at the device's wi (bound 1e-5)"}
# MicrofacetReflection::sample_f reports the pdf of the half vector it DREW; pdf(wo, wi) recomputes the half vector from the wi that was rounded to f32, and across a lobe
# this sharp one rounding of wi is a large step. The issue's comparison - the device's sampled pdf against the oracle's pdf(wo, wi_dev), 1e-5 - is therefore asserted where it is
# conditioned (alpha 0.02 misses it by the threshold finding: expected failure) and, for alpha 1e-3 / 1e-4, replaced by one that can pass and would catch a wrong pdf: the
# device's sampled pdf against the oracle's SAMPLED pdf at the same u (test_sharp_lobes_sampled_pdf_is_the_oracles_sampled_pdf). What pdf(wo, wi_dev) gives there is printed
# beside the oracle's own sample_f pdf against its own pdf(wo, wi_oracle) on the same queries - neither is a bound (MEASUREMENTS.md).
SHARP_PDF_AT_FINDINGS = {"plastic_a0.02": _AT_002 + "sampled pdf 5.8e-4 relative off the oracle's pdf at the device's wi (bound 1e-5)",
                         "metal_a0.02": _AT_002 + "sampled pdf 6.0e-4 relative off the oracle's pdf at the device's wi (bound 1e-5)"}


@pytest.mark.parametrize("name", _cases(SHARP, SHARP_VALUE_FINDINGS))
def test_sharp_lobes_agree_per_query_at_given_directions(pair, orc, name):
    """Un-remapped alpha 0.02 / 1e-3 / 1e-4, wi within a few alpha of the mirror direction: f and pdf within 1e-5 relative + 1e-7 (same inputs, same operations)."""
    osc, h, mats = pair
    wo, wi, u = _sharp_queries(name)
    ref = _oracle(orc, osc, mats[name], wo, wi, u)
    dev = h.bsdf_eval(mats[name], wo, wi, u, front_end="generic")["raw"]
    fig = dict(f=_excess(dev[:, 0:3], ref[:, 0:3], 1e-5, 1e-7), pdf=_excess(dev[:, 3], ref[:, 3], 1e-5, 1e-7))
    print(f"\nBSDF-SHARP-VALUES {name:16s} " + " ".join(f"{k}: rel {v[0]:.2e} abs {v[1]:.2e}" for k, v in fig.items()) + f" on the lobe {int((ref[:, 0] > 1.0).sum())}")
    assert (ref[:, 0] > 1.0).sum() > N_QUERIES // 4       # the queries do sit on the lobe
    assert np.array_equal(dev[:, 12], ref[:, 12])
    assert _within(dev[:, 0:3], ref[:, 0:3], 1e-5, 1e-7).all(), ("f", fig["f"])
    assert _within(dev[:, 3], ref[:, 3], 1e-5, 1e-7).all(), ("pdf", fig["pdf"])


def _sharp_samples(pair, orc, name):
    osc, h, mats = pair
    wo, wi, u = _sharp_queries(name)
    ref = _oracle(orc, osc, mats[name], wo, wi, u)
    dev = h.bsdf_eval(mats[name], wo, wi, u, front_end="generic")["raw"]
    at = _oracle(orc, osc, mats[name], wo, np.ascontiguousarray(dev[:, 7:10]), u)   # the oracle's f / pdf at the direction the DEVICE sampled
    return dev, ref, at, dev[:, 10] > 0


@pytest.mark.parametrize("name", SHARP)
def test_sharp_lobes_sample_the_oracles_direction(pair, orc, name):
    """The sampled wi within 1e-6 per component of the oracle's, the sampled type flags equal (plastic's diffuse lobe at the rim of its disk: the partition of RIM_Z);
    every sample of the glossy lobe within 1e-6 whatever its wi.z."""
    dev, ref, _, _ = _sharp_samples(pair, orc, name)
    _check_samples("BSDF-SHARP-WI", name, dev, ref, values=False)
    glossy = ((dev[:, 11].astype(int) & 8) != 0) & ((ref[:, 11].astype(int) & 8) != 0)
    e = _excess(dev[glossy, 7:10], ref[glossy, 7:10], 0, 1e-6)
    print(f"BSDF-SHARP-WI {name:16s} glossy lobe: {int(glossy.sum())} samples, wi abs {e[1]:.2e}")
    assert glossy.sum() > N_QUERIES // 4 and e[1] <= 1e-6, e


@pytest.mark.parametrize("name", SHARP)
def test_sharp_lobes_sampled_pdf_is_the_oracles_sampled_pdf(pair, orc, name):
    """The sampled pdf of the glossy lobe against the oracle's SAMPLED pdf at the same u - the pdf of the half vector drawn, well conditioned in u at any alpha -
    within 1e-4 relative (the issue's bound for sampled values)."""
    dev, ref, _, _ = _sharp_samples(pair, orc, name)
    glossy = ((dev[:, 11].astype(int) & 8) != 0) & ((ref[:, 11].astype(int) & 8) != 0) & (dev[:, 10] > 0) & (ref[:, 10] > 0)
    rel = _rel64(dev[glossy, 10], ref[glossy, 10])
    print(f"\nBSDF-SHARP-SPDF {name:16s} glossy lobe: {int(glossy.sum())} samples, sampled pdf vs the oracle's sampled pdf rel {float(rel.max()):.2e}")
    assert glossy.sum() > N_QUERIES // 4 and (rel <= 1e-4).all(), float(rel.max())


@pytest.mark.parametrize("name", _cases(SHARP, SHARP_F_AT_FINDINGS))
def test_sharp_lobes_sampled_f_is_the_oracles_f_at_the_device_direction(pair, orc, name):
    """One ulp in wi is a large step across such a lobe, so the oracle's own sampled values are no reference: the device's sampled f against the oracle's f(wo, wi_dev)
    - a second probe at the direction the device sampled - within 1e-5 relative + 1e-7."""
    dev, _, at, live = _sharp_samples(pair, orc, name)
    e = _excess(dev[live, 4:7], at[live, 0:3], 1e-5, 1e-7)
    print(f"\nBSDF-SHARP-F-AT {name:16s} rel {e[0]:.2e} abs {e[1]:.2e} live samples {int(live.sum())}")
    assert live.sum() > N_QUERIES // 2
    assert _within(dev[live, 4:7], at[live, 0:3], 1e-5, 1e-7).all(), e


@pytest.mark.parametrize("name", _cases(["plastic_a0.02", "metal_a0.02"], SHARP_PDF_AT_FINDINGS))
def test_sharp_lobes_sampled_pdf_is_the_oracles_pdf_at_the_device_direction(pair, orc, name):
    """... and the sampled pdf against the oracle's pdf(wo, wi_dev), within 1e-5 relative + 1e-7: alpha 0.02, where a rounding of wi is still a small step across the lobe."""
    dev, _, at, live = _sharp_samples(pair, orc, name)
    e = _excess(dev[live, 10], at[live, 3], 1e-5, 1e-7)
    print(f"\nBSDF-SHARP-PDF-AT {name:16s} rel {e[0]:.2e} abs {e[1]:.2e} live samples {int(live.sum())}")
    assert _within(dev[live, 10], at[live, 3], 1e-5, 1e-7).all(), e


@pytest.mark.parametrize("name", ["plastic_a0.001", "plastic_a0.0001", "metal_a0.001", "metal_a0.0001"])
def test_sharp_lobes_pdf_of_the_rounded_direction_is_no_reference(pair, orc, name):
    """Why alpha 1e-3 / 1e-4 are not in the test above: pdf(wo, wi) of a wi rounded to f32 is not the pdf of the half vector that was drawn, in the reference itself. Asserted:
    the ORACLE's own sample_f pdf misses its own pdf(wo, wi_oracle) by more than 1e-3 relative on these queries (measured 0.38 / 331 for plastic, 0.38 / 342 for metal at alpha
    1e-3 / 1e-4 - to three digits the device's figures against pdf(wo, wi_dev); so no f32 implementation can meet 1e-5 against it), while the
    device's sampled f - which Bsdf::sample_f does recompute from wi - is the oracle's f(wo, wi_dev) within 1e-5 (the test above this group) and its sampled pdf the oracle's
    sampled pdf within 1e-4 (test_sharp_lobes_sampled_pdf_is_the_oracles_sampled_pdf). The device's figure against pdf(wo, wi_dev) is printed for MEASUREMENTS.md."""
    osc, _, mats = pair
    dev, ref, at, live = _sharp_samples(pair, orc, name)
    wo, _, u = _sharp_queries(name)
    own = _oracle(orc, osc, mats[name], wo, np.ascontiguousarray(ref[:, 7:10]), u)   # the oracle's pdf at the direction the ORACLE sampled
    glossy_o = (ref[:, 10] > 0) & ((ref[:, 11].astype(int) & 8) != 0)
    glossy_d = live & ((dev[:, 11].astype(int) & 8) != 0)
    eo, e = _rel64(ref[glossy_o, 10], own[glossy_o, 3]), _rel64(dev[glossy_d, 10], at[glossy_d, 3])
    print(f"\nBSDF-SHARP-PDF-ROUNDED {name:16s} oracle sampled pdf vs oracle pdf(wo, wi_oracle): max {float(eo.max()):.2e} median {float(np.median(eo)):.2e}; "
          f"device sampled pdf vs oracle pdf(wo, wi_dev): max {float(e.max()):.2e} median {float(np.median(e)):.2e}")
    assert float(eo.max()) > 1e-3


# ---------------------------------------------------------------------------------------------- item 6: register-resident front-ends == generic
def _front_end_scene(textured):
    """Materials of the kinds of test_register_resident_front_ends_equal_the_generic_one that a register-resident front-end serves, with constant slots (the scene then
    has constant textures and area lights only: the constant-texture forms) or with image maps in their colour slots (the plain forms)."""
    from rustracer_amd.scene_desc import SceneDesc, WRAP_REPEAT
    from rustracer_amd.scenes.procedural import checker_fbm_image
    s = SceneDesc()
    if textured:
        img = s.add_mip(checker_fbm_image(32, 5, (0.9, 0.3, 0.2), (0.2, 0.3, 0.9), 4), trilinear=False, max_aniso=8.0, wrap=WRAP_REPEAT)
        tri = s.add_mip(checker_fbm_image(16, 6), trilinear=True, wrap=WRAP_REPEAT)
        c1, c2 = s.image_tex(img, 3, 2, 0.1, 0.2), s.image_tex(tri, 2, 2)
    else:
        c1, c2 = (0.6, 0.5, 0.4), (0.4, 0.4, 0.4)
    mats = {
        "matte": (s.matte(c1), "lambert"), "oren_nayar": (s.matte(c1, sigma=30.0), "two_lobe"), "plastic": (s.plastic(c1, c2, 0.15), "two_lobe"),
        "plastic_noremap": (s.plastic(c1, (0.4, 0.4, 0.4), 0.2, remap=False), "two_lobe"), "metal": (s.metal(roughness=0.05), "two_lobe"),
        "metal_aniso": (s.metal(roughness=0.1, urough=0.02, vrough=0.3), "two_lobe"), "mirror": (s.mirror(c2), "two_lobe"),
        "glass": (s.glass(index=1.5), "two_lobe_wide"), "glass_rough": (s.glass(kr=c2, kt=0.8, index=1.33, urough=0.1, vrough=0.2), "two_lobe_wide"),
        "substrate": (s.substrate(kd=c1, ks=c2, urough=0.05, vrough=0.2), "two_lobe_wide"), "uber_opaque": (s.uber(kd=c1, ks=(0.25, 0.25, 0.25), roughness=0.2), "two_lobe_wide"),
        # ... and kinds no register-resident front-end serves
        "uber": (s.uber(kd=(0.3, 0.4, 0.2), ks=(0.3, 0.3, 0.3), kr=(0.1, 0.1, 0.1), kt=(0.2, 0.2, 0.2), roughness=0.1, opacity=(0.8, 0.7, 0.9)), None),
        "translucent": (s.translucent(), None), "disney": (s.disney((0.6, 0.3, 0.2)), None),
    }
    mats["matte_bump"] = (s.set_bump(s.matte((0.6, 0.5, 0.4)), s.const_tex(0.05)) if not textured else s.set_bump(s.matte(c1), s.scale_tex(c2, s.const_tex(0.05))), None)
    mats["mix"] = (s.mix(mats["plastic"][0], mats["metal"][0], 0.35), None)
    s.add_quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), mats["matte"][0])
    s.add_quad((0, 0, 2), (1, 0, 2), (1, 1, 2), (0, 1, 2), mats["matte"][0], emission=(5.0, 5.0, 5.0))
    return s, mats


def _random_surfaces(gpu_host, rng, n):
    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    ng = unit(rng.normal(size=(n, 3)))
    ns = unit(ng + 0.3 * rng.normal(size=(n, 3)))
    t = unit(np.cross(ng, rng.normal(size=(n, 3))))
    b = np.cross(ng, t)
    dpdu = t * rng.uniform(0.5, 2.0, (n, 1)) + 0.1 * rng.normal(size=(n, 3))
    dpdv = b * rng.uniform(0.5, 2.0, (n, 1)) + 0.1 * rng.normal(size=(n, 3))
    sdu = dpdu + 0.2 * rng.normal(size=(n, 3))
    sdv = dpdv + 0.2 * rng.normal(size=(n, 3))
    return gpu_host.surface_records(n, p=rng.uniform(-3, 3, (n, 3)), n_geom=ng, n_shading=ns, dpdu=dpdu, dpdv=dpdv, sh_dpdu=sdu, sh_dpdv=sdv, uv=rng.uniform(-1, 2, (n, 2)),
                                    duv=rng.normal(size=(n, 4)) * 0.02, dpdx=rng.normal(size=(n, 3)) * 0.01, dpdy=rng.normal(size=(n, 3)) * 0.01, flip=rng.integers(0, 2, (n, 1)))


@pytest.mark.parametrize("textured", [False, True], ids=["constant_slots", "image_slots"])
def test_register_resident_front_ends_are_bit_equal_to_the_generic_one(gpu_host, textured):
    s, mats = _front_end_scene(textured)
    h = gpu_host.HostScene(s)
    h.upload(0)
    rng = np.random.default_rng(31 + textured)
    n = 1536
    wo, wi, u = _dirs(rng, n), _dirs(rng, n)[::-1].copy(), _us(rng, n)
    surf = _random_surfaces(gpu_host, rng, n)
    names = ("lambert", "two_lobe", "two_lobe_wide")
    launched = set()
    for name, (m, fe) in mats.items():
        for surface in (None, surf):
            gen = h.bsdf_eval(m, wo, wi, u, surface=surface, front_end="generic")["raw"]
            assert h.scene_query(gpu_host.RT_QUERY_BSDF_LAUNCHED) == 1   # k_bsdf_eval<0, false>
            auto = h.bsdf_eval(m, wo, wi, u, surface=surface, front_end="auto")["raw"]
            assert (gen[:, 12] >= 1).all(), name   # every material here builds a lobe
            # the kernel AUTO launched (RT_QUERY_BSDF_LAUNCHED = 1 + 2 * mode + const_tex): the register-resident one of the material's class, in the constant-texture form
            # on the scene of constants and in the plain form on the image-mapped one - not the generic kernel
            want_kernel = 1 + (2 * {"lambert": 3, "two_lobe": 5, "two_lobe_wide": 6}[fe] + (0 if textured else 1) if fe is not None else 0)
            assert h.scene_query(gpu_host.RT_QUERY_BSDF_LAUNCHED) == want_kernel, (name, h.scene_query(gpu_host.RT_QUERY_BSDF_LAUNCHED), want_kernel)
            launched.add(want_kernel)
            assert np.array_equal(bits(auto), bits(gen)), (name, "auto", surface is not None, int((bits(auto) != bits(gen)).any(axis=1).sum()))
            if fe is not None:
                own = h.bsdf_eval(m, wo, wi, u, surface=surface, front_end=fe)["raw"]
                assert h.scene_query(gpu_host.RT_QUERY_BSDF_LAUNCHED) == want_kernel
                assert np.array_equal(bits(own), bits(gen)), (name, fe, surface is not None, int((bits(own) != bits(gen)).any(axis=1).sum()))
        for other in names:   # a front-end asked for a material it does not serve is refused, with a message
            if other != fe:
                with pytest.raises(gpu_host.BackendError, match="front-end"):
                    h.bsdf_eval(m, wo[:4], wi[:4], u[:4], front_end=other)
    with pytest.raises(gpu_host.BackendError, match="out of range"):
        h.bsdf_eval(len(s.materials), wo[:4], wi[:4], u[:4])
    assert launched == ({1, 7, 11, 13} if textured else {1, 8, 12, 14}), launched   # k_bsdf_eval<0>, <3>, <5>, <6>: the plain forms / the constant-texture forms, each has run


# ---------------------------------------------------------------------------------------------- item 7: surface records mean what they say
def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def test_surface_records_drive_textures_and_rotate_rigidly(gpu_host):
    s, mats = _front_end_scene(True)
    h = gpu_host.HostScene(s)
    h.upload(0)
    rng = np.random.default_rng(77)
    n = 1024
    uv, duv = rng.uniform(-1, 2, (n, 2)).astype(np.float32), (rng.normal(size=(n, 4)) * 0.02).astype(np.float32)
    p, dpdx, dpdy = rng.uniform(-3, 3, (n, 3)).astype(np.float32), (rng.normal(size=(n, 3)) * 0.01).astype(np.float32), (rng.normal(size=(n, 3)) * 0.01).astype(np.float32)
    surf = gpu_host.surface_records(n, p=p, uv=uv, duv=duv, dpdx=dpdx, dpdy=dpdy)
    wo, wi = _dirs(rng, n), _dirs(rng, n)
    wo[:, 2], wi[:, 2] = np.abs(wo[:, 2]), np.abs(wi[:, 2])   # on the normal's side
    u = _us(rng, n)
    m = mats["matte"][0]
    kd_tex = s.materials[m].slots()[0]
    tex = h.texture_eval(int(kd_tex), uv, p=p, duv=duv, dpdx=dpdx, dpdy=dpdy)
    want = np.maximum(tex, np.float32(0.0)) * np.float32(1.0 / np.pi)   # LambertianReflection::f = R * INV_PI in f32
    assert len(np.unique(bits(want))) > n // 2   # the records do reach the texture: about as many values as records
    for fe in ("generic", "auto"):
        got = h.bsdf_eval(m, wo, wi, u, surface=surf, front_end=fe)
        assert np.array_equal(bits(got["f"]), bits(want)), fe
    # a rigid rotation of the whole record and of wo, wi: f and pdf stay (1e-5: a few roundings of the frame's dot products), the sampled wi turns with it
    R = _rotation(rng)
    rot = lambda v: np.ascontiguousarray(np.asarray(v, np.float64) @ R.T, np.float32)
    ng = rng.normal(size=(n, 3))
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    t = np.cross(ng, rng.normal(size=(n, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(ng, t)
    wo_l, wi_l = _dirs(rng, n).astype(np.float64), _dirs(rng, n).astype(np.float64)
    wo_l[:n // 2, 2], wi_l[:n // 2, 2] = np.abs(wo_l[:n // 2, 2]) + 0.05, np.abs(wi_l[:n // 2, 2]) + 0.05   # away from grazing where a rounding flips a side
    wo_l /= np.linalg.norm(wo_l, axis=1, keepdims=True)
    wi_l /= np.linalg.norm(wi_l, axis=1, keepdims=True)
    world = lambda v: v[:, :1] * t + v[:, 1:2] * b + v[:, 2:3] * ng
    wo_w, wi_w = world(wo_l), world(wi_l)
    # matte: 1e-5. The microfacet and Disney lobes: 1e-4 - the rotated wo, wi and frame are ROUNDED to f32 again, and a last bit in a direction moves a lobe of width
    # alpha by about 1e-7 theta / alpha^2 of its value (1e-5 per rounding at alpha = 0.1: the bound sampled values get for the same reason)
    for name, tol in (("matte", 1e-5), ("plastic", 1e-4), ("substrate", 1e-4), ("disney", 1e-4)):
        m = mats[name][0]
        a = h.bsdf_eval(m, np.float32(wo_w), np.float32(wi_w), u, surface=gpu_host.surface_records(n, p=p, n_geom=ng, dpdu=t, dpdv=b, uv=uv, duv=duv, dpdx=dpdx, dpdy=dpdy))
        r = h.bsdf_eval(m, rot(wo_w), rot(wi_w), u, surface=gpu_host.surface_records(n, p=rot(p), n_geom=rot(ng), dpdu=rot(t), dpdv=rot(b), uv=uv, duv=duv, dpdx=rot(dpdx), dpdy=rot(dpdy)))
        ok = (np.abs(wo_l[:, 2]) > 0.04) & (np.abs(wi_l[:, 2]) > 0.04)
        fe, pe = _excess(r["f"][ok], a["f"][ok], tol, 1e-7), _excess(r["pdf"][ok], a["pdf"][ok], tol, 1e-7)
        same = (a["stype"] == r["stype"]) & (a["spdf"] > 0) & (r["spdf"] > 0) & (np.abs(np.einsum("ij,ij->i", a["swi"], np.float32(ng))) >= 0.1)
        we = float(np.abs(r["swi"][same].astype(np.float64) - rot(a["swi"][same])).max())
        print(f"\nBSDF-ROTATION {name:12s} f rel {fe[0]:.2e} pdf rel {pe[0]:.2e} sampled wi abs {we:.2e} compared {int(same.sum())} / {n}")
        assert _within(r["f"][ok], a["f"][ok], tol, 1e-7).all() and _within(r["pdf"][ok], a["pdf"][ok], tol, 1e-7).all(), (name, fe, pe)
        assert same.sum() > 0.6 * (a["spdf"] > 0).sum() and we <= 1e-5, (name, we)   # (samples at least 0.1 off the tangent plane: below, a rounding of the input moves wi.z by 6e-8 / |wi.z|)


# ---------------------------------------------------------------------------------------------- item 8: sample_f is consistent with f and pdf
@pytest.mark.parametrize("name", ["matte", "oren", "plastic", "metal", "substrate", "mix", "uber", "translucent", "disney", "disney_cc", "disney_thin"])
def test_sample_f_is_reproduced_by_f_and_pdf(pair, name):
    """tests/test_oracle_kat.py::test_bsdf_sampling_is_consistent on the device, with its bounds: f(wo, wi_sampled) within 2e-4 relative (+ 1e-6), pdf within
    2e-4 max(1, pdf); the mix material's pdf excepted (reference quirk 10)."""
    _, h, mats = pair
    rng = np.random.default_rng(5)
    n = 4000
    wo = np.float32([0.3, -0.2, 0.93])
    wo = np.tile(wo / np.linalg.norm(wo), (n, 1)).astype(np.float32)
    u = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    a = h.bsdf_eval(mats[name], wo, wo, u)
    live = (a["spdf"] > 0) & ((a["stype"] & BSDF_SPECULAR) == 0)
    assert live.sum() > 100
    wi = np.ascontiguousarray(a["swi"][live])
    b = h.bsdf_eval(mats[name], wo[live], wi, u[live])
    fe = float(np.max(np.abs(b["f"].astype(np.float64) - a["sf"][live]) / (2e-4 * np.abs(a["sf"][live]) + 1e-6)))
    pe = float(np.max(np.abs(b["pdf"].astype(np.float64) - a["spdf"][live]) / (2e-4 * np.maximum(1.0, a["spdf"][live]))))
    print(f"\nBSDF-CONSISTENCY {name:12s} f {fe:.3f} of its bound, pdf {pe:.3f} of its bound, {int(live.sum())} samples")
    assert np.allclose(b["f"], a["sf"][live], rtol=2e-4, atol=1e-6), fe
    if name != "mix":
        assert (np.abs(b["pdf"].astype(np.float64) - a["spdf"][live]) <= 2e-4 * np.maximum(1.0, a["spdf"][live])).all(), pe


# ---------------------------------------------------------------------------------------------- item 9: per-sample radiance against the oracle
def _scrub_flags(L):
    L = np.asarray(L, np.float32)
    lum = np.float32(0.212671) * L[..., 0] + np.float32(0.715160) * L[..., 1] + np.float32(0.072169) * L[..., 2]
    with np.errstate(invalid="ignore"):
        return np.isnan(L).any(-1) | (lum < np.float32(-1e-5)) | np.isinf(lum)


def _compare_samples(gpu_host, orc, d, tol, cap, tag):
    W, H = d.film.xres, d.film.yres
    d.integrator.pixel_bounds = (0, W, 0, H)
    h = gpu_host.HostScene(d)
    rad, pf, st = h.render_samples()
    assert rad.shape[:2] == (H, W) and h.samples_window() == (0, 0, W, H)
    spp = rad.shape[2]
    o = orc.OracleScene(d)
    ref = np.zeros((H, W, spp, 3), np.float32)
    for y in range(H):
        for x in range(W):
            for s in range(spp):
                ref[y, x, s] = o.li_keyed(x, y, s)
    mean = float(np.nanmean(np.abs(ref[np.isfinite(ref)])))
    with np.errstate(invalid="ignore"):
        ratio = (np.abs(rad[..., :3].astype(np.float64) - ref) / np.maximum(np.abs(ref), mean)).max(-1)   # per channel: |difference| / max(|reference channel|, frame mean), then the largest
        bad = ~(ratio <= tol)
        ten = float((~(ratio <= 0.1 * tol)).mean())
    share = float(bad.mean())
    print(f"\nSAMPLES {tag:44s} {bad.size} samples: {int(bad.sum())} ({100 * share:.3f} %) beyond {tol:g}, {100 * ten:.3f} % beyond {0.1 * tol:g}; frame mean {mean:.4f}, "
          f"worst {float(np.nanmax(ratio)):.2e}; scrubbed {int(rad[..., 3].sum())}")
    assert np.array_equal(rad[..., 3] != 0, _scrub_flags(ref)), "scrub flags"
    assert st["camera_rays"] == W * H * spp and st["paths_scrubbed"] == int(rad[..., 3].sum())
    assert share <= cap, (share, cap)


def test_samples_match_the_oracle_cornell(gpu_host, orc):
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(24, 24, 16)
    d.integrator.max_depth = 3   # Russian roulette (bounces > 3) never runs: the number of draws of a path cannot flip
    _compare_samples(gpu_host, orc, d, 1e-4, 0.002, "cornell 24x24x16")


@pytest.mark.parametrize("material,light", [("plastic", "area"), ("metal", "point"), ("glass_rough", "infinite"), ("disney_metal_aniso_clearcoat", "area"),
                                            ("matte_bump_fbm", "distant"), ("glass", "area_two_sided"), ("substrate", "area"), ("mix_nested", "area")])
def test_samples_match_the_oracle_zoo(gpu_host, orc, material, light):
    from test_gpu_materials import _zoo
    d = _zoo(material, light, res=(20, 16), spp=4, max_depth=3)
    _compare_samples(gpu_host, orc, d, 1e-3, 0.005, f"zoo {material} / {light} 20x16x4")


# ---------------------------------------------------------------------------------------------- item 10: the samples are the frame's
def _film_from_samples(rad, pf, window, cropped, radius, max_lum):
    """FilmTile::add_sample + merge (film.rs:298-361, :177-194) for a box filter (every table entry 1) in numpy f32, samples in order; RGB -> XYZ as merge_film_tile."""
    x0, y0, x1, y1 = window
    H, W, spp, _ = rad.shape
    ch, cw = cropped[3] - cropped[1], cropped[2] - cropped[0]
    acc = np.zeros((ch, cw, 4), np.float32)
    for s in range(spp):
        c = rad[:, :, s, :3].copy()
        c[rad[:, :, s, 3] != 0] = 0
        lum = np.float32(0.212671) * c[..., 0] + np.float32(0.715160) * c[..., 1] + np.float32(0.072169) * c[..., 2]
        over = lum > np.float32(max_lum)
        if over.any():
            c[over] = c[over] * np.float32(max_lum) / lum[over][:, None]
        dx, dy = pf[:, :, s, 0] - np.float32(0.5), pf[:, :, s, 1] - np.float32(0.5)
        px0, py0 = np.ceil(dx - np.float32(radius)).astype(np.int64), np.ceil(dy - np.float32(radius)).astype(np.int64)
        px1, py1 = np.floor(dx + np.float32(radius) + np.float32(1.0)).astype(np.int64), np.floor(dy + np.float32(radius) + np.float32(1.0)).astype(np.int64)
        for oy in range(2):
            for ox in range(2):
                xx, yy = px0 + ox, py0 + oy
                ok = (xx < np.minimum(px1, cropped[2])) & (yy < np.minimum(py1, cropped[3])) & (xx >= cropped[0]) & (yy >= cropped[1])
                np.add.at(acc, (yy[ok] - cropped[1], xx[ok] - cropped[0]), np.concatenate([c[ok], np.ones((int(ok.sum()), 1), np.float32)], -1))
    out = np.zeros_like(acc)
    r, g, b = acc[..., 0], acc[..., 1], acc[..., 2]
    out[..., 0] = np.float32(0.412453) * r + np.float32(0.357580) * g + np.float32(0.180423) * b
    out[..., 1] = np.float32(0.212671) * r + np.float32(0.715160) * g + np.float32(0.072169) * b
    out[..., 2] = np.float32(0.019334) * r + np.float32(0.119193) * g + np.float32(0.950227) * b
    out[..., 3] = acc[..., 3]
    return out


def test_samples_are_the_frames(gpu_host):
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(32, 32, 16)
    d.film.filter_kind, d.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)   # box filter, radius 0.5
    h = gpu_host.HostScene(d)
    film, st_f = h.render()
    rad, pf, st = h.render_samples()
    assert rad.shape == (32, 32, 16, 4) and pf.shape == (32, 32, 16, 2) and np.isfinite(rad).all()
    setup = h.setup()
    rebuilt = _film_from_samples(rad, pf, h.samples_window(), [int(v) for v in setup["cropped"]], 0.5, d.film.max_sample_luminance)
    assert np.array_equal(rebuilt[..., 3], film[..., 3]), "filter weight sums"
    err = float(np.max(np.abs(rebuilt[..., :3].astype(np.float64) - film[..., :3]) / np.maximum(np.abs(film[..., :3]), 1e-30)))
    print(f"\nSAMPLES-FILM xyz of the film rebuilt from the samples vs rt_render: worst relative difference {err:.2e}")
    assert np.allclose(rebuilt[..., :3], film[..., :3], rtol=2e-5, atol=1e-7), err
    for k in ("camera_rays", "rays_closest", "rays_shadow", "rays_mis", "paths_scrubbed", "n_passes"):
        assert st[k] == st_f[k], k
    # a second call returns the same bytes
    rad2, pf2, _ = h.render_samples()
    assert np.array_equal(bits(rad2), bits(rad)) and np.array_equal(bits(pf2), bits(pf))
    # a cropped window returns the values the full frame has for its pixels
    d2 = cornell_box(32, 32, 16)
    d2.film.filter_kind, d2.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)
    d2.integrator.pixel_bounds = (5, 21, 9, 30)   # x0 x1 y0 y1
    h2 = gpu_host.HostScene(d2)
    radc, pfc, stc = h2.render_samples()
    assert h2.samples_window() == (5, 9, 21, 30) and radc.shape == (21, 16, 16, 4) and stc["camera_rays"] == 21 * 16 * 16
    assert np.array_equal(bits(radc), bits(rad[9:30, 5:21])) and np.array_equal(bits(pfc), bits(pf[9:30, 5:21]))
    # film positions: pixel + the (0, 2) value of 2D table 0 at the sample's shuffled index (get_camera_sample, zerotwosequence.rs:182-192)
    sc, pm = gpu_host.sampler_tables(16, 4, 0, 32 * 32)
    want = np.zeros_like(pf)
    for y in range(32):
        for x in range(32):
            _, t2 = tables_from_perm(sc[y * 32 + x], pm[y * 32 + x], 4)
            want[y, x, :, 0] = np.float32(x) + t2[0, :, 0]
            want[y, x, :, 1] = np.float32(y) + t2[0, :, 1]
    assert np.array_equal(bits(pf), bits(want))
    # p_film may be left out
    rad3, none, _ = h.render_samples(with_p_film=False)
    assert none is None and np.array_equal(bits(rad3), bits(rad))


# ---------------------------------------------------------------------------------------------- item 11: across batches and passes
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from rustracer_amd import host
from rustracer_amd.scenes import cornell_box
rad, pf, st = host.HostScene(cornell_box(320, 256, 4)).render_samples()
assert st["n_passes"] == 5, st["n_passes"]   # a batch of 2^16 pixels in four passes of one sample, then one of 2^14 pixels in one pass of four
np.save(sys.argv[2], rad)
np.save(sys.argv[3], pf)
"""


def test_batches_and_passes_change_no_byte(gpu_host, tmp_path):
    """RTX_PASS_LOG2 / RTX_BATCH_LOG2 are read once per process: a fresh child renders the window in two batches and one sample per pass (both knobs at 16)."""
    from rustracer_amd.scenes import cornell_box
    env = dict(os.environ, RTX_PASS_LOG2="16", RTX_BATCH_LOG2="16")
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    out = [str(tmp_path / "rad.npy"), str(tmp_path / "pf.npy")]
    r = subprocess.run([sys.executable, str(script), ROOT] + out, env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rad, pf, st = gpu_host.HostScene(cornell_box(320, 256, 4)).render_samples()
    assert rad.shape == (256, 320, 4, 4) and st["n_passes"] == 1
    assert np.array_equal(bits(np.load(out[0])), bits(rad)) and np.array_equal(bits(np.load(out[1])), bits(pf))
