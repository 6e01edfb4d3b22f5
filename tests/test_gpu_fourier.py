"""Material "fourier" on the GPU: the shade kernel's Fourier lobe against the numpy restatement (tests/fourier_ref.py), its sampling against its own pdf,
and frames that depend on it. The oracle has no Fourier BSDF: no scene here is handed to it."""
import numpy as np
import pytest

from rustracer_amd import host
from rustracer_amd import scene_desc as sd
from rustracer_amd.pbrt_export import write_pbrt
from rustracer_amd.scenes import cornell_box

import fourier_ref as fr

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not host.device_available():
        pytest.fail("no gfx950 device visible")


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _away_from_nodes(v, nodes, sign=1.0):
    """keep directions whose cosine is more than 2e-5 away from every mu node (the interval search may go either way on a node)"""
    z = sign * v[:, 2].astype(np.float64)
    return np.min(np.abs(z[:, None] - nodes[None, :].astype(np.float64)), 1) > 2e-5


def _plane_scene(t_path, n=2, bump=None, mix=False):
    d = sd.SceneDesc()
    m = d.fourier(t_path)
    if bump is not None:
        d.set_bump(m, bump)
    if mix:
        m = d.mix(m, d.matte(0.5), 0.4)
    d.add_quad((-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0), m)
    d.point_light((0.0, 0.6, 1.5), (20.0, 20.0, 20.0))
    d.camera.pos, d.camera.look, d.camera.up, d.camera.fov = (0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 30.0
    d.film.xres = d.film.yres = 32
    d.sampler.spp = 256
    d.integrator.max_depth = 1
    return d, m


def _tables(tmp_path):
    narrow = fr.glossy_table(n_channels=1)
    narrow = fr.make_table((narrow.mu * F(0.93) + F(0.02)).astype(F), lambda mi, mo: np.asarray([[0.3 + 0.1 * abs(mi)] + [0.05] * 3], F), 1, 1.0)
    ts = {"glossy1": fr.glossy_table(n_channels=1, m=6),
          "glossy3_eta": fr.glossy_table(n_channels=3, m=9, eta=1.33, empty_cells=True),
          "narrow": narrow,
          "lambert": fr.lambert_table((0.65, 0.05, 0.05), n_mu=21)}
    return {k: (fr.write_table(str(tmp_path / f"{k}.bsdf"), t), t) for k, t in ts.items()}


def _eval(path, wo, wi, u):
    d, m = _plane_scene(path)
    h = host.HostScene(d)
    return h.fourier_eval(m, wo, wi, u)


@pytest.mark.parametrize("name", ["glossy1", "glossy3_eta", "narrow", "lambert"])
def test_kernel_parity_with_the_restatement(tmp_path, name):
    path, t = _tables(tmp_path)[name]
    rng = np.random.default_rng(7)
    n = 1 << 16
    wo, wi, u = _unit(rng, 2 * n), _unit(rng, 2 * n), rng.random((2 * n, 2)).astype(F)
    keep = _away_from_nodes(wo, t.mu) & _away_from_nodes(wi, t.mu, -1.0)
    wo, wi, u = wo[keep][:n], wi[keep][:n], u[keep][:n]
    got = _eval(path, wo, wi, u)
    for k in ("f", "pdf", "sf", "swi", "spdf"):
        assert np.all(np.isfinite(got[k])), k
    ref_f, ref_pdf = fr.f(t, wo, wi), fr.pdf(t, wo, wi)
    assert np.all(np.abs(got["f"] - ref_f) <= 1e-5 * np.abs(ref_f) + 1e-7), np.max(np.abs(got["f"] - ref_f))
    assert np.all(np.abs(got["pdf"] - ref_pdf) <= 1e-5 * np.abs(ref_pdf) + 1e-7), np.max(np.abs(got["pdf"] - ref_pdf))
    sf, swi, spdf = fr.sample_f(t, wo, u)
    tol = lambda r: 1e-4 * np.maximum(1.0, np.abs(r))
    assert np.all(np.abs(got["sf"] - sf) <= tol(sf)), np.max(np.abs(got["sf"] - sf))
    assert np.all(np.abs(got["swi"] - swi) <= tol(swi)), np.max(np.abs(got["swi"] - swi))
    assert np.all(np.abs(got["spdf"] - spdf) <= tol(spdf)), np.max(np.abs(got["spdf"] - spdf))
    if name == "narrow":  # cosines outside [mu[0], mu[n - 1]]: black, pdf 0
        out = (wo[:, 2] > t.mu[-1]) | (wo[:, 2] < t.mu[0]) | (-wi[:, 2] > t.mu[-1]) | (-wi[:, 2] < t.mu[0])
        assert out.sum() > 1000
        assert np.all(got["f"][out] == 0) and np.all(got["pdf"][out] == 0)
    assert np.count_nonzero(got["f"]) > n // 4


def test_sampled_pdf_is_the_pdf_of_the_sampled_direction(tmp_path):
    path, t = _tables(tmp_path)["glossy3_eta"]
    rng = np.random.default_rng(3)
    n = 1 << 15
    wo, u = _unit(rng, n), rng.random((n, 2)).astype(F)
    s = _eval(path, wo, wo, u)
    ok = s["spdf"] > 0
    back = _eval(path, wo[ok], s["swi"][ok], u[ok])
    assert ok.sum() > n // 2
    scale = s["spdf"][ok].max()
    assert np.all(np.abs(back["pdf"] - s["spdf"][ok]) <= 1e-4 * np.abs(s["spdf"][ok]) + 1e-6 * scale), np.max(np.abs(back["pdf"] - s["spdf"][ok]))


@pytest.mark.parametrize("wo_z", [0.9, 0.3, -0.6])
def test_chi2_of_sampled_directions_against_pdf(tmp_path, wo_z):
    from scipy import stats
    path, t = _tables(tmp_path)["glossy1"]
    wo = np.float32([np.sqrt(1 - wo_z * wo_z), 0.0, wo_z])
    n, nt, nphi, sub = 1 << 18, 10, 20, 8
    rng = np.random.default_rng(11)
    s = _eval(path, np.repeat(wo[None], n, 0), np.repeat(wo[None], n, 0), rng.random((n, 2)).astype(F))
    ok = s["spdf"] > 0
    w = s["swi"][ok]
    phi = np.mod(np.arctan2(w[:, 1], w[:, 0]), 2 * np.pi)
    obs, _, _ = np.histogram2d(np.clip(w[:, 2], -1, 1), phi, bins=[nt, nphi], range=[[-1, 1], [0, 2 * np.pi]])
    # expected: n x the pdf integrated over each (cos theta, phi) bin (midpoint rule, sub x sub points a bin)
    ct = -1 + (np.arange(nt * sub) + 0.5) * (2.0 / (nt * sub))
    ph = (np.arange(nphi * sub) + 0.5) * (2 * np.pi / (nphi * sub))
    C, P = np.meshgrid(ct, ph, indexing="ij")
    st = np.sqrt(1 - C * C)
    wi = np.stack([st * np.cos(P), st * np.sin(P), C], -1).reshape(-1, 3).astype(F)
    p = _eval(path, np.repeat(wo[None], wi.shape[0], 0), wi, np.zeros((wi.shape[0], 2), F))["pdf"].reshape(nt * sub, nphi * sub).astype(np.float64)
    exp = p.reshape(nt, sub, nphi, sub).sum((1, 3)) * (2.0 / (nt * sub)) * (2 * np.pi / (nphi * sub)) * n
    o, e = obs.ravel(), exp.ravel()
    big = e >= 5
    chi2 = np.sum((o[big] - e[big]) ** 2 / e[big]) + ((o[~big].sum() - e[~big].sum()) ** 2 / e[~big].sum() if e[~big].sum() > 0 else 0.0)
    dof = int(big.sum()) + (1 if (~big).any() else 0) - 1
    pval = stats.chi2.sf(chi2, dof)
    assert pval > 0.01, (chi2, dof, pval)


def test_direct_term_of_a_plane_under_a_point_light(tmp_path):
    path, t = _tables(tmp_path)["glossy3_eta"]
    t = fr.read_bsdf(fr.write_table(str(tmp_path / "g.bsdf"), fr.glossy_table(n_channels=3, m=9, eta=1.0)))
    d, m = _plane_scene(str(tmp_path / "g.bsdf"))
    film, _ = host.HostScene(d).render()
    rgb = host.film_to_rgb(film).astype(np.float64)
    W = d.film.xres
    tanh = np.tan(np.radians(d.camera.fov) / 2)
    ys, xs = np.mgrid[0:W, 0:W]
    sx, sy = -1 + 2 * (xs + 0.5) / W, 1 - 2 * (ys + 0.5) / W
    o = np.array(d.camera.pos, np.float64)
    dirs = np.stack([sx * tanh, sy * tanh, -np.ones_like(sx)], -1)  # looking down -z with +y up; the scene is mirror-symmetric in x
    tt = -o[2] / dirs[..., 2]
    p = o + tt[..., None] * dirs
    inside = (np.abs(p[..., 0]) < 0.9) & (np.abs(p[..., 1]) < 0.9)
    L = np.array([0.0, 0.6, 1.5])
    wi = L - p
    r2 = (wi ** 2).sum(-1)
    wi /= np.sqrt(r2)[..., None]
    wo = -dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)
    fv = fr.f(t, wo.reshape(-1, 3).astype(F), wi.reshape(-1, 3).astype(F)).reshape(W, W, 3).astype(np.float64)
    want = fv * (20.0 / (4 * np.pi * r2))[..., None] * np.abs(wi[..., 2])[..., None]
    got, ref = rgb[inside], want[inside]
    assert np.all(np.isfinite(rgb)) and ref.max() > 0
    rel = np.abs(got - ref) / np.maximum(ref, 1e-3 * ref.max())
    assert np.max(rel) < 0.01, np.max(rel)


def test_cornell_red_wall_as_a_lambert_table_matches_matte(tmp_path):
    path = fr.write_table(str(tmp_path / "lam.bsdf"), fr.lambert_table((0.65, 0.05, 0.05), n_mu=41))
    a = cornell_box(128, 128, 256)
    b = cornell_box(128, 128, 256)
    b.materials[1] = b.materials.pop(b.fourier(path))  # the red wall (material 1) as the matching Lambert table
    fa, _ = host.HostScene(a).render()
    fb, st = host.HostScene(b).render()
    ra, rb = host.film_to_rgb(fa).astype(np.float64), host.film_to_rgb(fb).astype(np.float64)
    assert np.all(np.isfinite(rb)) and st["vertices_generic"] > 0
    blocks = lambda r: r.reshape(8, 16, 8, 16, 3).mean((1, 3))  # the means of an 8 x 8 grid of blocks (16 x 16 pixels, 65536 samples each)
    lum = lambda x: x @ np.array([0.2126, 0.7152, 0.0722])
    rel = np.abs(lum(blocks(ra)) - lum(blocks(rb))) / lum(blocks(ra))
    assert np.max(rel) < 0.01, np.max(rel)


def test_frames_are_plumbing_invariant(tmp_path):
    path, t = _tables(tmp_path)["glossy3_eta"]
    d = cornell_box(48, 48, 16)
    d.materials[1] = d.materials.pop(d.fourier(path))  # the red wall: Fourier; the green wall: mix(Fourier, white)
    d.materials[2] = d.materials.pop(d.mix(d.fourier(path), 0, 0.3))
    h = host.HostScene(d)
    film, _ = h.render()
    assert np.all(np.isfinite(film)) and film[..., :3].max() > 0
    pb = str(tmp_path / "c.pbrt")
    write_pbrt(d, pb)
    fp, _ = host.PbrtScene(pb).render()
    assert np.array_equal(fp, film)
    multi, _, _ = h.render_multi([0])
    assert np.array_equal(multi, film)
    shards = [h.render(rank=r, world_size=2)[0] for r in range(2)]
    assert np.array_equal(shards[0] + shards[1], film)


def test_mix_and_bump_render_finite_films(tmp_path):
    path, t = _tables(tmp_path)["glossy3_eta"]
    for kw in (dict(mix=True), dict(bump=0.05)):
        d, m = _plane_scene(path, **kw)
        d.integrator.max_depth = 3
        film, _ = host.HostScene(d).render()
        assert np.all(np.isfinite(film)) and film[..., :3].max() > 0, kw
