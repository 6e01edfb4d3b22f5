"""tests/shading_frame_model.py against closed forms it was not written from, the oracle (orc_bsdf_probe_surface) against that model on the query sets of
tests/shading_frame_cases.py with the bounds the GPU file uses, and the query sets against their own conditions. No GPU."""
import numpy as np
import pytest

import shading_frame_cases as K
import shading_frame_model as M


@pytest.fixture(scope="module")
def world(host, orc):
    s, mats, plan, tex = K.scene()
    osc = orc.OracleScene(s)

    def tex_eval(t, uv, duv):
        return np.stack([osc.tex_probe(int(t), uv=uv[i], duv=duv[i]) for i in range(uv.shape[0])])
    return dict(host=host, osc=osc, mats=mats, plan=plan, tex=tex, tex_eval=tex_eval)


def _orthonormal(host, rng, n):
    ng = K._unit(rng.normal(size=(n, 3)))
    t = K._unit(np.cross(ng, rng.normal(size=(n, 3))))
    return host.surface_records(n, n_geom=ng, dpdu=t, dpdv=np.cross(ng, t)), ng.astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------- the model against closed forms
def test_model_reduces_to_closed_forms_on_an_orthonormal_frame(host):
    rng = np.random.default_rng(1)
    n = 512
    surf, ng = _orthonormal(host, rng, n)
    wo, wi = K._random_unit32(rng, n).astype(np.float64), K._random_unit32(rng, n).astype(np.float64)
    u = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    kd = np.array([0.8, 0.6, 0.4])
    out, _ = M.evaluate(surf, [M.Lobe("lambert_r", r=kd)], wo, wi, u)
    co, ci = M.dot(wo, ng), M.dot(wi, ng)
    same = co * ci > 0
    assert np.allclose(out[same, 0:3], kd / np.pi, rtol=1e-12) and (out[~same, 0:3] == 0).all()
    assert np.allclose(out[:, 3], np.where(same, np.abs(ci) / np.pi, 0.0), rtol=1e-6, atol=1e-9)   # (the record is orthonormal to float32)
    out, s = M.evaluate(surf, [M.Lobe("mirror", r=np.full(3, 0.9))], wo, wi, u)
    assert np.allclose(s["wi"], -wo + 2.0 * co[:, None] * ng, atol=1e-6) and (s["type"] == 17).all() and (s["pdf"] == 1).all()
    assert np.allclose(s["f"], 0.9 / np.abs(co)[:, None], rtol=1e-5)
    out, s = M.evaluate(surf, [M.Lobe("fresnel_spec", r=np.ones(3), t=np.ones(3), eta_a=1.0, eta_b=1.5)], wo, wi, np.full((n, 2), 0.99999, np.float32))
    t = s["type"] == 18                                          # Snell's law in world space: eta_i sin theta_i = eta_t sin theta_t, wi in the plane of wo and n, other side
    assert t.sum() > n // 2
    eta_i, eta_t = np.where(co > 0, 1.0, 1.5), np.where(co > 0, 1.5, 1.0)
    sin_i, sin_t = np.linalg.norm(np.cross(ng, wo), axis=1), np.linalg.norm(np.cross(ng, s["wi"]), axis=1)
    assert np.allclose((eta_i * sin_i)[t], (eta_t * sin_t)[t], atol=1e-6)
    assert (np.abs(M.dot(np.cross(ng, wo), s["wi"]))[t] < 1e-6).all() and ((M.dot(s["wi"], ng) * co)[t] < 0).all()
    assert np.allclose(np.linalg.norm(s["wi"][t], axis=1), 1.0, atol=1e-6)
    # uber's index-matched pass-through: wi = -wo, f = T / |cos|
    out, s = M.evaluate(surf, [M.Lobe("spec_t", t=np.full(3, 0.2))], wo, wi, u)
    assert np.allclose(s["wi"], -wo, atol=1e-6) and np.allclose(s["f"], 0.2 / np.abs(co)[:, None], rtol=1e-5)


def test_model_bump_of_a_linear_displacement_is_the_slope(host):
    """d linear in (u, v) with slopes (a, b): the bumped frame is sh_dpdu + a n, sh_dpdv + b n whatever du and dv are."""
    rng = np.random.default_rng(2)
    surf, _ = K.group_b_queries(host, "matte_lin")
    n = surf.shape[0]
    a, b, d0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    lk = M.bump_lookups(surf)
    assert len(np.unique(lk["du"])) > n // 4 and (lk["du"] == np.float32(0.0005)).sum() > n // 4   # both rules of the shift
    rec, side = M.bump(surf, d0, d0 + a * lk["du"].astype(np.float64), d0 + b * lk["dv"].astype(np.float64))
    s64 = surf.astype(np.float64)
    want_u, want_v = s64[:, M.SDU] + a[:, None] * s64[:, M.NS], s64[:, M.SDV] + b[:, None] * s64[:, M.NS]
    assert np.allclose(rec[:, M.SDU], want_u, rtol=0, atol=1e-12) and np.allclose(rec[:, M.SDV], want_v, rtol=0, atol=1e-12)
    nn = M.unit(np.cross(want_u, want_v))
    nn = np.where((s64[:, M.FLIP] != 0)[:, None], -nn, nn)
    assert np.allclose(side, M.dot(nn, s64[:, M.NG]), atol=1e-12)
    assert np.allclose(rec[:, M.NS], np.where((side < 0)[:, None], -nn, nn), atol=1e-12) and (M.dot(rec[:, M.NS], s64[:, M.NG]) >= 0).all()


def test_model_bump_of_a_constant_replaces_the_records_own_normal(host):
    """A constant displacement gives n' = +-normalize(cross(sh_dpdu, sh_dpdv)) on n_geom's side - NOT the record's own sh_n where the two differ (interaction.rs:227)."""
    surf, _ = K.group_b_queries(host, "matte_chk")
    s64 = surf.astype(np.float64)
    c = np.full(surf.shape[0], 0.37)
    rec, _ = M.bump(surf, c, c, c)
    nn = M.unit(np.cross(s64[:, M.SDU], s64[:, M.SDV]))
    nn = np.where((M.dot(nn, s64[:, M.NG]) < 0)[:, None], -nn, nn)
    assert np.allclose(rec[:, M.NS], nn, atol=1e-12)
    assert (np.linalg.norm(rec[:, M.NS] - M.unit(s64[:, M.NS]), axis=1) > 0.05).mean() > 0.9   # the records' own normals are somewhere else
    assert np.array_equal(rec[:, M.SDU], s64[:, M.SDU]) and np.array_equal(rec[:, M.SDV], s64[:, M.SDV])


def test_model_frame_is_not_inverted_by_local_to_world(host):
    """The quirk the frame carries: on a record whose sh_dpdu is not perpendicular to sh_n, local_to_world(world_to_local(w)) != w; on an orthonormal one it is w."""
    rng = np.random.default_rng(3)
    surf, _ = K.group_b_queries(host, "matte_img")
    w = K._random_unit32(rng, surf.shape[0]).astype(np.float64)
    fr = M.frame(surf)
    assert np.allclose(np.linalg.norm(fr["ss"], axis=1), 1.0) and np.array_equal(fr["ns"], surf[:, M.NS].astype(np.float64))
    assert np.allclose(fr["ts"], np.cross(surf[:, M.NS].astype(np.float64), fr["ss"]))
    back = M.local_to_world(fr, M.world_to_local(fr, w))
    assert (np.linalg.norm(back - w, axis=1) > 1e-2).mean() > 0.9
    osurf, _ = _orthonormal(host, rng, 64)
    fo = M.frame(osurf)
    assert np.allclose(M.local_to_world(fo, M.world_to_local(fo, w[:64])), w[:64], atol=1e-6)


@pytest.mark.parametrize("flip_wo", [False, True])
def test_model_lambert_samples_have_density_pdf(host, flip_wo):
    """Chi-square of the sampled world directions against bsdf_pdf on a 16 x 32 (cos theta, phi) grid, p > 0.01, fixed seed; a tilted orthonormal frame."""
    from scipy import stats
    rng = np.random.default_rng(17)
    surf = K._tilted(host, rng, 1, 20.0, 70.0)
    n, nt, nphi, sub = 1 << 17, 16, 32, 4
    fr = M.frame(surf)
    wo = -fr["ns"] * 0.8 + fr["ss"] * 0.6 if flip_wo else fr["ns"] * 0.5 + fr["ts"] * np.sqrt(0.75)
    lobes = [M.Lobe("lambert_r", r=np.full(3, 0.5))]
    rep = lambda a, k: np.repeat(a, k, 0)
    s = M.bsdf_sample_f(M.frame(rep(surf, n)), lobes, rep(wo, n), rng.random((n, 2)).astype(np.float32))
    w = s["wi"][s["pdf"] > 0]
    phi = np.mod(np.arctan2(w[:, 1], w[:, 0]), 2 * np.pi)
    obs, _, _ = np.histogram2d(np.clip(w[:, 2], -1, 1), phi, bins=[nt, nphi], range=[[-1, 1], [0, 2 * np.pi]])
    ct = -1 + (np.arange(nt * sub) + 0.5) * (2.0 / (nt * sub))
    ph = (np.arange(nphi * sub) + 0.5) * (2 * np.pi / (nphi * sub))
    Cc, Pp = np.meshgrid(ct, ph, indexing="ij")
    st = np.sqrt(1 - Cc * Cc)
    wi = np.stack([st * np.cos(Pp), st * np.sin(Pp), Cc], -1).reshape(-1, 3)
    p = M.bsdf_pdf(M.frame(rep(surf, wi.shape[0])), lobes, rep(wo, wi.shape[0]), wi).reshape(nt * sub, nphi * sub)
    e = (p.reshape(nt, sub, nphi, sub).sum((1, 3)) * (2.0 / (nt * sub)) * (2 * np.pi / (nphi * sub)) * n).ravel()
    o = obs.ravel()
    big = e >= 5
    chi2 = np.sum((o[big] - e[big]) ** 2 / e[big]) + ((o[~big].sum() - e[~big].sum()) ** 2 / e[~big].sum() if e[~big].sum() > 0 else 0.0)
    dof = int(big.sum()) + (1 if (~big).any() else 0) - 1
    pval = stats.chi2.sf(chi2, dof)
    print(f"\nSHADING-FRAME-CHI2 flip_wo={flip_wo}: chi2 {chi2:.1f} dof {dof} p {pval:.3f}")
    assert pval > 0.01, (chi2, dof, pval)


# ---------------------------------------------------------------------------------------------- the query sets keep their own conditions
def test_rim_constants_are_the_projects():
    import test_gpu_shade_entry as E
    assert (K.RIM_Z, K.RIM_Z2, K.N) == (E.RIM_Z, E.RIM_Z2, E.N_QUERIES)


@pytest.mark.parametrize("name", K.GROUP_A)
def test_group_a_query_sets_hold_their_shares(world, name):
    plan = world["plan"][name]
    surf, wo, wi, u = K.group_a_queries(world["host"], name, plan["specular"])
    cls = np.bincount(K.classes(surf, wo, wi), minlength=4)
    mc = K.model_case(plan, surf, wo, wi, u)
    share = float((mc["skip"] | mc["skip_sample"]).mean())
    print(f"\nSHADING-FRAME-SETS {name:12s} classes {cls.tolist()} skipped {100 * share:.2f} %")
    assert (cls >= K.N / 5).all(), cls
    assert share <= K.SKIP_CAP
    s64 = surf.astype(np.float64)
    cosn = M.dot(M.unit(s64[:, M.NS]), s64[:, M.NG])
    (a0, a1), (b0, b1), (c0, c1), (d0, d1) = K.FAMILIES
    assert np.allclose(cosn[a0:a1], 1.0, atol=1e-6)
    assert (cosn[b0:b1] < np.cos(np.radians(19.9))).all() and (cosn[b0:b1] > np.cos(np.radians(70.1))).all()
    assert (np.abs(M.dot(M.unit(s64[c0:c1, M.SDU]), s64[c0:c1, M.NS])) > 1e-3).mean() > 0.9 and (np.abs(np.linalg.norm(s64[c0:c1, M.SDU], axis=1) - 1) > 1e-3).mean() > 0.9
    assert (cosn[d0:d1] < 0).all()
    if plan["specular"]:
        assert (np.abs(M.dot(wo.astype(np.float64), s64[:, M.NS])) >= 0.05).all()


def test_group_b_records_cross_their_factors(world):
    surf, _ = K.group_b_queries(world["host"], "matte_lin")
    s64 = surf.astype(np.float64)
    side = M.dot(np.cross(s64[:, M.SDU], s64[:, M.SDV]), s64[:, M.NG]) > 0
    flip = s64[:, M.FLIP] != 0
    lk = M.bump_lookups(surf)
    kind = np.where((lk["du"] == np.float32(0.0005)) & (lk["dv"] == np.float32(0.0005)), 0, np.where(lk["du"] == np.float32(0.0005), 2, 1))
    for sv in (False, True):
        for fv in (False, True):
            for k in range(3):
                assert ((side == sv) & (flip == fv) & (kind == k)).sum() >= K.N // 16, (sv, fv, k)


# ---------------------------------------------------------------------------------------------- the oracle against the model
@pytest.mark.parametrize("name", K.GROUP_A)
def test_oracle_matches_the_model_on_frames_and_sides(world, name):
    plan = world["plan"][name]
    surf, wo, wi, u = K.group_a_queries(world["host"], name, plan["specular"])
    got = world["osc"].bsdf_probe_surface(world["mats"][name], surf, wo, wi, u)
    K.compare("SHADING-FRAME-ORACLE-A", name, got, K.model_case(plan, surf, wo, wi, u))


@pytest.mark.parametrize("name", K.GROUP_B)
def test_oracle_matches_the_model_on_bump_maps(world, name):
    plan, surf, wo, wi, u, pre = K.bump_case(world["host"], world["plan"], name, world["tex_eval"])
    got = world["osc"].bsdf_probe_surface(world["mats"][name], surf, wo, wi, u)
    K.compare("SHADING-FRAME-ORACLE-B", name, got, K.model_case(plan, surf, wo, wi, u, pre=pre))


def test_oracle_matches_the_model_where_only_flip_decides(world):
    plan, surf, wo, wi, u, pre = K.flip_edge_case(world["host"], world["plan"], world["tex_eval"])
    got = world["osc"].bsdf_probe_surface(world["mats"]["matte_chk"], surf, wo, wi, u)
    K.compare("SHADING-FRAME-ORACLE-FLIP", "matte_chk", got, K.model_case(plan, surf, wo, wi, u, pre=pre, exact_side=True))
    # ... and the bit does act there: the records with flip = 1 answer differently from the same records with flip = 0
    unflipped = surf.copy()
    unflipped[:, M.FLIP] = 0
    other = world["osc"].bsdf_probe_surface(world["mats"]["matte_chk"], unflipped, wo, wi, u)
    on = (surf[:, M.FLIP] != 0) & (got[:, 10] > 0)
    assert on.sum() > 64 and (np.abs(other[on, 7:10] - got[on, 7:10]).max(1) > 1e-3).mean() > 0.9


def test_probe_surface_with_null_is_the_canonical_probe(world, orc):
    import ctypes as C
    rng = np.random.default_rng(9)
    wo, wi, u = K._random_unit32(rng, 64), K._random_unit32(rng, 64), K._us(rng, 64)
    osc, m = world["osc"], world["mats"]["uber"]
    a = osc.bsdf_probe_surface(m, None, wo, wi, u)
    b = osc.bsdf_probe_surface(m, world["host"].surface_records(64), wo, wi, u)
    f, smp, pdf = np.zeros(3, np.float32), np.zeros(8, np.float32), C.c_float()
    P = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    for i in range(64):
        nl = orc.lib().orc_bsdf_probe(osc.h, m, P(wo[i]), P(wi[i]), P(u[i]), P(f), C.byref(pdf), P(smp))
        want = np.concatenate([f, [pdf.value], smp, [nl]]).astype(np.float32)
        assert np.array_equal(a[i].view(np.uint32), want.view(np.uint32)) and np.array_equal(b[i].view(np.uint32), want.view(np.uint32))
