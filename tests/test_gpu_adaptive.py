"""Frame statistics and adaptive steps on the GPU (RT_FLAG_FRAME_STATS, RT_FRAME_STATS, rt_frame_advance_adaptive through HostScene.progressive(pixel_stats=True)):
the moments are the samples' - bit for bit -, the flag changes no film byte, the mask of an adaptive step is the stated criterion, the film is the film of the
samples taken, and batches, passes, table residency, shards and pixel bounds change nothing of that. Every measured figure is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FLOOR = float(F(1e-3))


def _cornell(filter_kind=0, filter_params=(0.5, 0.5, 0.0, 0.0)):
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(32, 32, 16)
    d.film.filter_kind, d.film.filter_params = filter_kind, filter_params   # default: box filter, radius 0.5
    return d


def _clamped(rad, max_lum):
    """(c, y): what the film splats of every sample - scrubbed samples as 0, the max_sample_luminance clamp in float32 as the device applies it - and its float32
    luminance, left to right."""
    c = rad[..., :3].copy()
    c[rad[..., 3] != 0] = 0
    lum = F(0.212671) * c[..., 0] + F(0.715160) * c[..., 1] + F(0.072169) * c[..., 2]
    over = lum > F(max_lum)
    if over.any():
        c[over] = c[over] * F(max_lum) / lum[over][:, None]
    y = F(0.212671) * c[..., 0] + F(0.715160) * c[..., 1] + F(0.072169) * c[..., 2]
    assert c.dtype == np.float32 and y.dtype == np.float32
    return c, y


def _moments(y, taken):
    """(n, sum_y, sum_y2) of the taken samples: sequential float64 sums in sample-index order (cumsum adds one term after the other)."""
    y64 = np.where(taken, y.astype(np.float64), 0.0)   # (adding +0.0 changes no bit of a non-negative sum; a scrubbed or black sample adds +0.0 on the device too)
    return taken.sum(-1).astype(np.float64), np.cumsum(y64, -1)[..., -1], np.cumsum(y64 * y64, -1)[..., -1]


def _criterion(n, sy, sy2, threshold, floor_y, min_samples):
    """The activity criterion of rt_frame_advance_adaptive in float64, operation for operation."""
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = sy / n
        var = np.maximum(0.0, sy2 - sy * mean) / (n - 1.0)
        se = np.sqrt(var / n)
        return (n < max(min_samples, 2)) | (se > threshold * np.maximum(mean, floor_y))


def _ratio(n, sy, sy2, floor_y):
    mean = sy / n
    return np.sqrt(np.maximum(0.0, sy2 - sy * mean) / (n - 1.0) / n) / np.maximum(mean, floor_y)


def _median_gap_threshold(ratio):
    """The midpoint of the two adjacent sorted ratios nearest the median, as the float32 the entry point takes, and the relative gap between the two."""
    r = np.sort(ratio.ravel())
    i = r.size // 2
    lo, hi = float(r[i - 1]), float(r[i])
    thr = float(F(0.5 * (lo + hi)))
    return thr, lo, hi


def _film_taken(rad, pf, taken, cropped, radius, table, max_lum):
    """FilmTile::add_sample + merge (film.rs:298-361, :177-194) of the samples marked in `taken` [window pixel, sample] with float64 sums: pixel ranges and filter
    table indices from the float32 film positions as the device computes them, the table's float32 weights, RGB -> XYZ in float64."""
    ch, cw = cropped[3] - cropped[1], cropped[2] - cropped[0]
    acc = np.zeros((ch, cw, 4), np.float64)
    c_all, _ = _clamped(rad, max_lum)
    r, inv_r = F(radius), F(1.0) / F(radius)
    span = int(np.ceil(2 * radius)) + 1
    table = np.asarray(table, np.float32).ravel()
    for s in range(rad.shape[2]):
        t = taken[:, :, s]
        if not t.any():
            continue
        c = c_all[:, :, s]
        dx, dy = pf[:, :, s, 0] - F(0.5), pf[:, :, s, 1] - F(0.5)
        x0, y0 = np.maximum(np.ceil(dx - r).astype(np.int64), cropped[0]), np.maximum(np.ceil(dy - r).astype(np.int64), cropped[1])
        x1, y1 = np.minimum(np.floor(dx + r + F(1.0)).astype(np.int64), cropped[2]), np.minimum(np.floor(dy + r + F(1.0)).astype(np.int64), cropped[3])
        for oy in range(span):
            yy = y0 + oy
            iy = np.minimum(np.floor(np.abs((yy.astype(np.float32) - dy) * inv_r * F(16.0))), F(15.0)).astype(np.int64)
            for ox in range(span):
                xx = x0 + ox
                ix = np.minimum(np.floor(np.abs((xx.astype(np.float32) - dx) * inv_r * F(16.0))), F(15.0)).astype(np.int64)
                ok = t & (xx < x1) & (yy < y1)
                fw = table[iy[ok] * 16 + ix[ok]].astype(np.float64)
                np.add.at(acc, (yy[ok] - cropped[1], xx[ok] - cropped[0]), np.concatenate([c[ok].astype(np.float64) * fw[:, None], fw[:, None]], -1))
    out = np.zeros_like(acc)
    r_, g_, b_ = acc[..., 0], acc[..., 1], acc[..., 2]
    out[..., 0] = float(F(0.412453)) * r_ + float(F(0.357580)) * g_ + float(F(0.180423)) * b_
    out[..., 1] = float(F(0.212671)) * r_ + float(F(0.715160)) * g_ + float(F(0.072169)) * b_
    out[..., 2] = float(F(0.019334)) * r_ + float(F(0.119193)) * g_ + float(F(0.950227)) * b_
    out[..., 3] = acc[..., 3]
    return out


def _taken(spp, *steps):
    """steps: (first index, end index, boolean [pixel] or None for every pixel) -> boolean [pixel..., sample]."""
    shape = next(m.shape for _, _, m in steps if m is not None)
    t = np.zeros(shape + (spp,), bool)
    for a, b, m in steps:
        t[..., a:b] = True if m is None else m[..., None]
    return t


@pytest.fixture(scope="module")
def cornell(gpu_host):
    """The 32 x 32 x 16 Cornell box under the box filter: the scene, its whole-frame film, its samples (render_samples: parent-commit code held to the oracle by
    tests/test_gpu_shade_entry.py) and what the film splats of them. Rendered once, left unchanged."""
    h = gpu_host.HostScene(_cornell())
    film, st = h.render()
    rad, pf, _ = h.render_samples()
    _, y = _clamped(rad, h.desc.film.max_sample_luminance)
    for a in (film, rad, pf, y):
        a.setflags(write=False)
    return dict(h=h, film=film, st=st, rad=rad, pf=pf, y=y)


@pytest.fixture(scope="module")
def case3(cornell):
    """advance(4), the read-out, the threshold between the two ratios nearest the median - and the frame's state after one adaptive step of 4 at that threshold."""
    h = cornell["h"]
    with h.progressive(pixel_stats=True) as fr:
        first = fr.advance(4)
        n, sy, sy2 = [a.copy() for a in fr.pixel_stats()]
        ratio = _ratio(n, sy, sy2, FLOOR)
        thr, lo, hi = _median_gap_threshold(ratio)
        mask = _criterion(n, sy, sy2, thr, FLOOR, 4)
        step = fr.advance_adaptive(4, thr, FLOOR, min_samples=4)
        out = dict(first=first, n4=n, ratio=ratio, thr=thr, lo=lo, hi=hi, mask=mask, step=step, n8=fr.pixel_stats()[0].copy(), film=fr.film(), active=fr.active_pixels,
                   taken=fr.samples_taken, done=fr.samples_done)
    return out


# ---------------------------------------------------------------------------------------------- 1
def test_moments_are_the_samples(cornell):
    """n == k exactly; sum_y and sum_y2 bit for bit: every term is exact in double (a float32 squared has 48 bits) and the additions run in index order."""
    h, y = cornell["h"], cornell["y"]
    with h.progressive(pixel_stats=True) as fr:
        z = fr.pixel_stats()
        assert all(a.shape == (32, 32) and a.dtype == np.float64 and not a.any() for a in z), "zeros before the first step"
        k = 0
        for step in (1, 3, 8):
            fr.advance(step)
            k += step
            n, sy, sy2 = fr.pixel_stats()
            wn, wsy, wsy2 = _moments(y, _taken(16, (0, k, np.ones((32, 32), bool))))
            d = [int((a.view(np.uint64) != b.view(np.uint64)).sum()) for a, b in ((np.ascontiguousarray(sy), wsy), (np.ascontiguousarray(sy2), wsy2))]
            print(f"\nADAPTIVE moments at k = {k}: n == k everywhere {bool((n == k).all())}; sum_y words that differ {d[0]}, sum_y2 {d[1]} (largest sum_y {sy.max():.6g})")
            assert (n == k).all() and np.array_equal(n, wn)
            assert d == [0, 0]
        mean, se = fr.noise()
        assert np.array_equal(mean, sy / 12) and (se >= 0).all() and np.isfinite(se).all()
        assert fr.state_bytes >= 32 * 32 * (16 * 2 + 32) + 1024


# ---------------------------------------------------------------------------------------------- 2
def test_the_flag_changes_no_film_byte_and_refusals(gpu_host, cornell):
    h, film = cornell["h"], cornell["film"]
    with h.progressive(pixel_stats=True) as fr:
        stats = [fr.advance(n) for n in (1, 3, 4, 8)]
        differ = int((bits(fr.film()) != bits(film)).sum())
        print(f"\nADAPTIVE stats frame stepped [1, 3, 4, 8] with plain advance: {differ} film words differ from rt_render's; samples taken {fr.samples_taken}")
        assert differ == 0
        assert fr.samples_taken == sum(s["camera_rays"] for s in stats) == cornell["st"]["camera_rays"] and fr.active_pixels == 0
    with h.progressive() as fr:   # no flag
        fr.advance(2)
        for call, word in ((lambda: fr.pixel_stats(), "RT_FLAG_FRAME_STATS"), (lambda: fr.advance_adaptive(2, 0.1), "RT_FLAG_FRAME_STATS")):
            with pytest.raises(gpu_host.BackendError) as e:
                call()
            print(f"  refused: {e.value}")
            assert word in str(e.value)
        assert fr.samples_done == 2
    with h.progressive(pixel_stats=True) as fr:
        seen = set()
        for kw, word in ((dict(n=4, threshold=-0.5), "threshold"), (dict(n=4, threshold=float("nan")), "threshold"), (dict(n=0, threshold=0.1), "n_samples"),
                         (dict(n=4, threshold=0.1, floor_y=-1.0), "floor_y"), (dict(n=4, threshold=0.1, floor_y=float("nan")), "floor_y"),
                         (dict(n=4, threshold=0.1, min_samples=-1), "min_samples")):
            with pytest.raises(gpu_host.BackendError) as e:
                fr.advance_adaptive(**kw)
            print(f"  refused {kw}: {e.value}")
            assert word in str(e.value) and "(-1)" in str(e.value)
            seen.add((word, str(e.value)))
        assert len({m for _, m in seen}) == 4   # one message per kind of refusal
        assert fr.samples_done == 0 and fr.samples_taken == 0 and not fr.film().any()


# ---------------------------------------------------------------------------------------------- 3
def test_the_mask_is_the_criterion_and_the_film_is_the_film_of_the_samples_taken(cornell, case3):
    h, c = cornell["h"], case3
    gap = (c["hi"] - c["lo"]) / c["hi"]
    print(f"\nADAPTIVE threshold {c['thr']:.9g} between ratios {c['lo']:.9g} and {c['hi']:.9g} (relative gap {gap:.3e}); ratios span [{c['ratio'].min():.3g}, {c['ratio'].max():.3g}]")
    assert gap > 1e-6 and c["lo"] < c["thr"] < c["hi"]
    assert (c["n4"] == 4).all()
    mask = c["ratio"] > c["thr"]
    assert np.array_equal(mask, c["mask"])   # (the ratio form and the product form agree: no pixel sits within rounding of the decision)
    count = int(mask.sum())
    want_n = np.where(mask, 8.0, 4.0)
    print(f"  active pixels {c['active']} (mask {count}); camera rays of the step {c['step']['camera_rays']}; samples taken {c['taken']}; n differs in {int((c['n8'] != want_n).sum())} pixels")
    assert 0 < count < 1024
    assert np.array_equal(c["n8"], want_n)
    assert c["active"] == count and c["step"]["camera_rays"] == 4 * count and c["taken"] == 4 * 1024 + c["step"]["camera_rays"] and c["done"] == 8
    cropped = [int(v) for v in h.setup()["cropped"]]
    want = _film_taken(cornell["rad"], cornell["pf"], _taken(16, (0, 4, None), (4, 8, mask)), cropped, 0.5, h.setup()["filter_table"], h.desc.film.max_sample_luminance)
    got = c["film"]
    rtol = ((want_n + 4) * 2.0 ** -23)[..., None]
    err = np.abs(got[..., :3].astype(np.float64) - want[..., :3])
    worst = float(np.max(err / np.maximum(np.abs(want[..., :3]), 1e-30)))
    over = int((err > 1e-7 + rtol * np.abs(want[..., :3])).sum())
    print(f"  weights equal {np.array_equal(got[..., 3], want[..., 3])}; worst relative XYZ difference {worst:.3e} (bound (k + 4) * 2^-23 = {rtol.max():.3e} + 1e-7), {over} values over")
    assert np.array_equal(got[..., 3].astype(np.float64), want[..., 3]), "filter weight sums"
    assert over == 0, worst


# ---------------------------------------------------------------------------------------------- 4
def test_threshold_infinity_takes_nothing(cornell):
    h = cornell["h"]
    with h.progressive(pixel_stats=True) as fr:
        fr.advance(4)
        film, stats = fr.film(), [a.copy() for a in fr.pixel_stats()]
        st = fr.advance_adaptive(4, float("inf"), FLOOR, min_samples=4)
        zero = all(v == 0 for k, v in st.items() if k != "shade_section_cycles") and not any(st["shade_section_cycles"])
        differ = int((bits(fr.film()) != bits(film)).sum())
        print(f"\nADAPTIVE threshold +inf: active pixels {fr.active_pixels}, stats all zero {zero}, film words changed {differ}, done {fr.samples_done}, taken {fr.samples_taken}")
        assert fr.active_pixels == 0 and zero and differ == 0 and fr.samples_done == 8 and fr.samples_taken == 4 * 1024
        assert all(np.array_equal(a, b) for a, b in zip(stats, fr.pixel_stats()))


def test_min_samples_spp_is_rt_renders_frame(cornell):
    """Every step all-active through the masked ray generation: it must reproduce the unmasked route bit for bit."""
    h, film = cornell["h"], cornell["film"]
    with h.progressive(pixel_stats=True) as fr:
        steps = [fr.advance_adaptive(n, 0.0, 0.0, min_samples=16) for n in (1, 3, 4, 8)]
        actives = fr.active_pixels
        differ = int((bits(fr.film()) != bits(film)).sum())
        print(f"\nADAPTIVE min_samples = spp: camera rays per step {[s['camera_rays'] for s in steps]}, active {actives}, {differ} film words differ from rt_render's")
        assert [s["camera_rays"] for s in steps] == [1024, 3072, 4096, 8192] and actives == 1024 and fr.samples_done == 16
        assert differ == 0
        for k in ("rays_closest", "rays_shadow", "rays_mis", "paths_scrubbed"):
            assert sum(s[k] for s in steps) == cornell["st"][k], k
        assert (fr.pixel_stats()[0] == 16).all()


def test_threshold_zero_drops_exactly_the_pixels_without_variance(gpu_host):
    """A camera further back sees the black background around the box: those pixels have var == 0 and drop out at threshold 0; every other pixel goes on."""
    d = _cornell()
    d.camera.pos = (278.0, 273.0, -1600.0)
    h = gpu_host.HostScene(d)
    with h.progressive(pixel_stats=True) as fr:
        fr.advance(4)
        n, sy, sy2 = [a.copy() for a in fr.pixel_stats()]
        var0 = np.maximum(0.0, sy2 - sy * (sy / n)) == 0.0
        st = fr.advance_adaptive(4, 0.0, 0.0, min_samples=4)
        n8 = fr.pixel_stats()[0]
        print(f"\nADAPTIVE threshold 0: {int(var0.sum())} pixels with var == 0, {int((~var0).sum())} with var > 0; active {fr.active_pixels}; n == 4 on {int((n8 == 4).sum())}, n == 8 on {int((n8 == 8).sum())}")
        assert var0.any() and (~var0).any()
        assert np.array_equal(n8, np.where(var0, 4.0, 8.0)) and fr.active_pixels == int((~var0).sum()) and st["camera_rays"] == 4 * fr.active_pixels


# ---------------------------------------------------------------------------------------------- 5
def test_wide_filter(gpu_host, case3):
    """Gaussian, radius 2: the sample window is wider than the film, so which samples were taken is derived from render_samples' moments with the criterion itself
    (and checked against the read-out inside the film). The bound is test_wide_filter's: n_taps * 2^-23 + 1e-7 with n_taps = 16 * 5 * 5, on all four channels."""
    from rustracer_amd.scene_desc import FILTER_GAUSSIAN
    h = gpu_host.HostScene(_cornell(FILTER_GAUSSIAN, (2.0, 2.0, 2.0, 0.0)))
    rad, pf, _ = h.render_samples()
    _, y = _clamped(rad, h.desc.film.max_sample_luminance)
    x0, y0, x1, y1 = h.samples_window()
    cropped = [int(v) for v in h.setup()["cropped"]]
    inside = (slice(cropped[1] - y0, cropped[3] - y0), slice(cropped[0] - x0, cropped[2] - x0))
    thr = case3["thr"]
    steps = [(0, 4, np.ones(y.shape[:2], bool))]
    with h.progressive(pixel_stats=True) as fr:
        fr.advance(4)
        for a in (4, 8):
            m = _criterion(*_moments(y, _taken(16, *steps)), thr, FLOOR, 4)
            st = fr.advance_adaptive(4, thr, FLOOR, min_samples=4)
            print(f"\nADAPTIVE gaussian r = 2, offer [{a}, {a + 4}): active {fr.active_pixels} (criterion on render_samples' moments {int(m.sum())}), camera rays {st['camera_rays']}")
            assert fr.active_pixels == int(m.sum()) and st["camera_rays"] == 4 * int(m.sum())
            steps.append((a, a + 4, m))
        taken = _taken(16, *steps)
        assert np.array_equal(fr.pixel_stats()[0], taken.sum(-1)[inside])
        got = fr.film()
    want = _film_taken(rad, pf, taken, cropped, 2.0, h.setup()["filter_table"], h.desc.film.max_sample_luminance)
    n = 16 * 5 * 5
    err = np.abs(got.astype(np.float64) - want)
    worst = float(np.max(err / np.maximum(np.abs(want), 1e-30)))
    over = int((err > 1e-7 + n * 2.0 ** -23 * np.abs(want)).sum())
    print(f"  worst relative difference to the float64 film of the samples taken {worst:.3e} (bound {n * 2.0 ** -23:.3e} + 1e-7), {over} values over")
    assert over == 0, worst


# ---------------------------------------------------------------------------------------------- 6
_SEQUENCE = """
def sequence(h, thr, budget=None):
    with h.progressive(table_budget=budget, pixel_stats=True) as fr:
        a, b = fr.advance(2), fr.advance_adaptive(2, thr, float(np.float32(1e-3)), min_samples=2)
        return fr.film(), np.stack(fr.pixel_stats(), -1), fr.tables_resident, (a["n_passes"], b["n_passes"]), fr.active_pixels
"""
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from rustracer_amd import host
from rustracer_amd.scenes import cornell_box
""" + _SEQUENCE + """
h = host.HostScene(cornell_box(320, 256, 4))
for out, budget, resident in ((sys.argv[3], None, True), (sys.argv[4], 1, False)):
    film, stats, res, passes, active = sequence(h, float(sys.argv[2]), budget)
    assert res == resident, (budget, res)
    # two batches of 2^16 and 2^14 pixels, the first in passes of one sample: more than one pass per step
    assert min(passes) >= 3, passes
    np.savez(out, film=film, stats=stats, active=active)
"""


def test_batches_passes_and_table_residency_change_no_byte(gpu_host, tmp_path):
    """RTX_PASS_LOG2 / RTX_BATCH_LOG2 are read once per process: a fresh child runs advance(2), advance_adaptive(2) in two batches and one sample per pass (both knobs
    at 16), with resident and with rebuilt sampler tables; films and stats read-outs are this process's, word for word."""
    from rustracer_amd.scenes import cornell_box
    ns = {"np": np}
    exec(_SEQUENCE, ns)
    h = gpu_host.HostScene(cornell_box(320, 256, 4))
    with h.progressive(pixel_stats=True) as fr:   # the threshold, from a first run at default knobs
        fr.advance(2)
        thr, lo, hi = _median_gap_threshold(_ratio(*fr.pixel_stats(), FLOOR))
    assert (hi - lo) / hi > 1e-6
    film, stats, _, passes, active = ns["sequence"](h, thr)
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    out = [str(tmp_path / "resident.npz"), str(tmp_path / "rebuilt.npz")]
    env = dict(os.environ, RTX_PASS_LOG2="16", RTX_BATCH_LOG2="16")
    r = subprocess.run([sys.executable, str(script), ROOT, repr(thr)] + out, env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    resident, rebuilt = np.load(out[0]), np.load(out[1])
    words = lambda a: np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)
    d = [int((words(a[k]) != words(b[k])).sum()) for k in ("film", "stats") for a, b in ((resident, rebuilt), (resident, dict(film=film, stats=stats)))]
    print(f"\nADAPTIVE 320x256x4 in two batches, threshold {thr:.6g}: active here {active} / resident {int(resident['active'])} / rebuilt {int(rebuilt['active'])} (passes here {passes}); "
          f"words that differ - film resident/rebuilt {d[0]}, resident/here {d[1]}, stats resident/rebuilt {d[2]}, resident/here {d[3]}")
    assert 0 < active < 320 * 256 and int(resident["active"]) == active and int(rebuilt["active"]) == active
    assert d == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- 7
def test_shards(cornell, case3):
    """Ranks 0 and 1 of 2 on one GPU run the adaptive sequence of case 3; merged as test_gpu_progressive.test_shards merges, the film is the unsharded adaptive film in
    every word (the criterion reads a pixel's own moments only), and a rank's stats are zero in the other rank's rows."""
    from rustracer_amd.distributed import owned_pixel_mask, touched_rows
    h = cornell["h"]
    st = h.setup()
    cropped, sb = [int(v) for v in st["cropped"]], [int(v) for v in st["sample_bounds"]]
    parts, stats, active = [], [], []
    for r in range(2):
        with h.progressive(rank=r, world_size=2, pixel_stats=True) as fr:
            fr.advance(4)
            fr.advance_adaptive(4, case3["thr"], FLOOR, min_samples=4)
            parts.append(fr.film())
            stats.append(np.stack(fr.pixel_stats(), -1))
            active.append(fr.active_pixels)
    merged = parts[0].copy()
    rows = touched_rows(cropped, sb, 1, 2, 0.5)
    merged[rows] += parts[1][rows]
    differ = int((bits(merged) != bits(case3["film"])).sum())
    stray = [int(np.count_nonzero(stats[r][owned_pixel_mask(cropped, sb, 1 - r, 2)])) for r in range(2)]
    n_sum = stats[0][..., 0] + stats[1][..., 0]
    print(f"\nADAPTIVE 2 shards: merged film differs from the unsharded adaptive film in {differ} words; active {active} (unsharded {case3['active']}); "
          f"non-zero stats in the other rank's rows {stray}")
    assert differ == 0 and stray == [0, 0] and sum(active) == case3["active"]
    assert np.array_equal(n_sum, case3["n8"])


# ---------------------------------------------------------------------------------------------- 8
def test_pixel_bounds_and_crop(gpu_host):
    """The description of test_gpu_progressive.test_pixel_bounds_and_crop: pixels outside pixel_bounds keep n == 0 and are never counted active."""
    d = _cornell()
    d.integrator.pixel_bounds = (5, 21, 9, 30)     # x0 x1 y0 y1
    d.film.crop = (0.25, 0.75, 0.125, 1.0)
    h = gpu_host.HostScene(d)
    film, st = h.render()
    x0, y0, x1, y1 = h.samples_window()
    cropped = [int(v) for v in h.setup()["cropped"]]
    inside = np.zeros(film.shape[:2], bool)
    inside[y0 - cropped[1]:y1 - cropped[1], x0 - cropped[0]:x1 - cropped[0]] = True
    with h.progressive(pixel_stats=True) as fr:
        a = fr.advance(4)
        n4 = fr.pixel_stats()[0].copy()
        b = fr.advance_adaptive(4, 0.0, 0.0, min_samples=8)    # every pixel inside the bounds holds fewer than 8 samples: all of them, and only them
        all_active = fr.active_pixels
        n, sy, sy2 = [v.copy() for v in fr.pixel_stats()]
        thr, lo, hi = _median_gap_threshold(_ratio(n[inside], sy[inside], sy2[inside], FLOOR))
        mask = _criterion(n, sy, sy2, thr, FLOOR, 4) & inside
        c = fr.advance_adaptive(8, thr, FLOOR, min_samples=4)
        n16 = fr.pixel_stats()[0]
        print(f"\nADAPTIVE pixel bounds + crop, film {film.shape}, window {(x0, y0, x1, y1)}: {int(inside.sum())} pixels inside; active {all_active} then {fr.active_pixels} "
              f"(mask {int(mask.sum())}, threshold {thr:.6g}, gap {(hi - lo) / hi:.3e}); camera rays {a['camera_rays']}, {b['camera_rays']}, {c['camera_rays']}")
        assert film.shape == (28, 16, 4) and int(inside.sum()) == (x1 - x0) * (y1 - y0)
        assert np.array_equal(n4, np.where(inside, 4.0, 0.0)) and np.array_equal(n, np.where(inside, 8.0, 0.0))
        assert all_active == int(inside.sum()) and a["camera_rays"] == b["camera_rays"] == 4 * all_active
        assert (hi - lo) / hi > 1e-6
        assert fr.active_pixels == int(mask.sum()) and c["camera_rays"] == 8 * int(mask.sum())
        assert np.array_equal(n16, np.where(mask, 16.0, np.where(inside, 8.0, 0.0))) and not n16[~inside].any()
