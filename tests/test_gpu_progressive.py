"""Progressive frames on the GPU (rt_frame_* through HostScene.progressive): a frame rendered in steps is rt_render's frame - bit for bit under the box filter,
whatever the steps, batches, passes, table residency, shards and neighbours on the scene are -, its film part-way is the film of the samples so far, and the RGB /
8-bit read-outs are Film::write_image's and the PNG writer's pixels. Every measured figure is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("camera_rays", "rays_closest", "rays_shadow", "rays_mis", "paths_scrubbed")


def _cornell(filter_kind=0, filter_params=(0.5, 0.5, 0.0, 0.0)):
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(32, 32, 16)
    d.film.filter_kind, d.film.filter_params = filter_kind, filter_params   # default: box filter, radius 0.5
    return d


@pytest.fixture(scope="module")
def cornell(gpu_host):
    """The 32 x 32 x 16 Cornell box under the box filter: the scene, its whole-frame film and stats (rendered once, left unchanged)."""
    h = gpu_host.HostScene(_cornell())
    film, st = h.render()
    film.setflags(write=False)
    return h, film, st


def _step(h, steps, **kw):
    """The film after `steps`, the per-step stats, and the frame's tables_resident."""
    with h.progressive(**kw) as fr:
        stats = [fr.advance(n) for n in steps]
        return fr.film(), stats, fr.tables_resident


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("steps", [[16], [1] * 16, [1, 3, 4, 8]], ids=["16", "1x16", "1-3-4-8"])
def test_the_finished_frame_is_rt_renders(cornell, steps):
    """Every pixel's sum is its own samples in index order; under the box filter at most one edge splat joins it, and a two-term float addition commutes: bit-equal."""
    h, film, st = cornell
    with h.progressive() as fr:
        assert fr.spp == 16 and fr.samples_done == 0
        stats = [fr.advance(n) for n in steps]
        assert fr.samples_done == 16
        got = fr.film()
        differ = int((bits(got) != bits(film)).sum())
        print(f"\nPROGRESSIVE steps {steps}: {differ} film words differ from rt_render's; tables resident: {fr.tables_resident}")
        assert differ == 0
        for k in COUNTS:
            total = sum(s[k] for s in stats)
            print(f"  {k}: steps {total}, frame {st[k]}")
            assert total == st[k], k
        extra = fr.advance(4)   # a finished frame: zero stats, no device work, the same bytes
        assert all(v == 0 for k, v in extra.items() if k != "shade_section_cycles") and not any(extra["shade_section_cycles"]), extra
        assert fr.samples_done == 16 and np.array_equal(bits(fr.film()), bits(film))


# ---------------------------------------------------------------------------------------------- 2
def _film_f64(rad, pf, k, window, cropped, radius, max_lum):
    """FilmTile::add_sample + merge (film.rs:298-361, :177-194) of samples [0, k) under a box filter (every table entry 1) with float64 sums; the scrub flags of
    render_samples are honoured; pixel ranges from the float32 film positions as the device computes them; RGB -> XYZ in float64."""
    ch, cw = cropped[3] - cropped[1], cropped[2] - cropped[0]
    acc = np.zeros((ch, cw, 4), np.float64)
    f = np.float32
    for s in range(k):
        c = rad[:, :, s, :3].copy()
        c[rad[:, :, s, 3] != 0] = 0
        lum = f(0.212671) * c[..., 0] + f(0.715160) * c[..., 1] + f(0.072169) * c[..., 2]
        over = lum > f(max_lum)
        if over.any():
            c[over] = c[over] * f(max_lum) / lum[over][:, None]
        dx, dy = pf[:, :, s, 0] - f(0.5), pf[:, :, s, 1] - f(0.5)
        px0, py0 = np.ceil(dx - f(radius)).astype(np.int64), np.ceil(dy - f(radius)).astype(np.int64)
        px1, py1 = np.floor(dx + f(radius) + f(1.0)).astype(np.int64), np.floor(dy + f(radius) + f(1.0)).astype(np.int64)
        for oy in range(2):
            for ox in range(2):
                xx, yy = px0 + ox, py0 + oy
                ok = (xx < np.minimum(px1, cropped[2])) & (yy < np.minimum(py1, cropped[3])) & (xx >= cropped[0]) & (yy >= cropped[1])
                np.add.at(acc, (yy[ok] - cropped[1], xx[ok] - cropped[0]), np.concatenate([c[ok].astype(np.float64), np.ones((int(ok.sum()), 1))], -1))
    out = np.zeros_like(acc)
    r, g, b = acc[..., 0], acc[..., 1], acc[..., 2]
    out[..., 0] = float(f(0.412453)) * r + float(f(0.357580)) * g + float(f(0.180423)) * b
    out[..., 1] = float(f(0.212671)) * r + float(f(0.715160)) * g + float(f(0.072169)) * b
    out[..., 2] = float(f(0.019334)) * r + float(f(0.119193)) * g + float(f(0.950227)) * b
    out[..., 3] = acc[..., 3]
    return out


def test_the_film_part_way_is_the_film_of_the_samples_so_far(cornell):
    """After k samples per pixel the film is FilmTile::add_sample over samples [0, k): weight sums exact (integers under the box filter), XYZ within
    (k + 4) * 2^-23 relative - k float32 additions of non-negative terms plus the three-term colour transform, each at most half an ulp of a partial sum no larger
    than the result - plus 1e-7 absolute."""
    h, _, _ = cornell
    rad, pf, _ = h.render_samples()
    cropped = [int(v) for v in h.setup()["cropped"]]
    with h.progressive() as fr:
        for n, k in ((1, 1), (3, 4), (8, 12)):
            fr.advance(n)
            assert fr.samples_done == k
            got = fr.film()
            want = _film_f64(rad, pf, k, h.samples_window(), cropped, 0.5, h.desc.film.max_sample_luminance)
            rtol = (k + 4) * 2.0 ** -23
            err = np.abs(got[..., :3].astype(np.float64) - want[..., :3])
            worst = float(np.max(err / np.maximum(np.abs(want[..., :3]), 1e-30)))
            over = int((err > 1e-7 + rtol * np.abs(want[..., :3])).sum())
            print(f"\nPROGRESSIVE k = {k}: weights equal {np.array_equal(got[..., 3], want[..., 3])}, worst relative XYZ difference {worst:.3e} (bound {rtol:.3e} + 1e-7), {over} values over")
            assert np.array_equal(got[..., 3].astype(np.float64), want[..., 3]), "filter weight sums"
            assert over == 0, worst


# ---------------------------------------------------------------------------------------------- 3
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from rustracer_amd import host
from rustracer_amd.scenes import cornell_box
h = host.HostScene(cornell_box(320, 256, 4))
for out, budget, resident in ((sys.argv[2], None, True), (sys.argv[3], 1, False)):
    with h.progressive(table_budget=budget) as fr:
        assert fr.tables_resident == resident, (budget, fr.tables_resident)
        a, b = fr.advance(1), fr.advance(3)
        # two batches of 2^16 and 2^14 pixels: the first in passes of one sample, the second in one pass per step
        assert (a["n_passes"], b["n_passes"]) == (2, 4), (a["n_passes"], b["n_passes"])
        np.save(out, fr.film())
"""


def test_batches_passes_and_table_residency_change_no_byte(gpu_host, tmp_path):
    """RTX_PASS_LOG2 / RTX_BATCH_LOG2 are read once per process: a fresh child steps the frame [1, 3] in two batches and one sample per pass (both knobs at 16), once
    with resident sampler tables and once rebuilding them in every step; both films are this process's whole-frame render."""
    from rustracer_amd.scenes import cornell_box
    env = dict(os.environ, RTX_PASS_LOG2="16", RTX_BATCH_LOG2="16")
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    out = [str(tmp_path / "resident.npy"), str(tmp_path / "rebuilt.npy")]
    r = subprocess.run([sys.executable, str(script), ROOT] + out, env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    film, _ = gpu_host.HostScene(cornell_box(320, 256, 4)).render()
    resident, rebuilt = np.load(out[0]), np.load(out[1])
    d = [int((bits(a) != bits(b)).sum()) for a, b in ((resident, rebuilt), (resident, film), (rebuilt, film))]
    print(f"\nPROGRESSIVE 320x256x4 in two batches: words that differ resident/rebuilt {d[0]}, resident/rt_render {d[1]}, rebuilt/rt_render {d[2]}")
    assert d == [0, 0, 0]


# ---------------------------------------------------------------------------------------------- 4
def test_wide_filter(gpu_host):
    """Gaussian, radius 2: every sample splats onto 5 x 5 pixels through float atomics whose order differs between any two launches. All weights are positive, so
    every partial sum is bounded by the result: n * 2^-23 relative with n = 16 * 5 * 5 taps at most per pixel, plus 1e-7 absolute."""
    from rustracer_amd.scene_desc import FILTER_GAUSSIAN
    h = gpu_host.HostScene(_cornell(FILTER_GAUSSIAN, (2.0, 2.0, 2.0, 0.0)))
    film, _ = h.render()
    got, _, _ = _step(h, [3, 5, 8])
    n = 16 * 5 * 5
    err = np.abs(got.astype(np.float64) - film)
    worst = float(np.max(err / np.maximum(np.abs(film), 1e-30)))
    over = int((err > 1e-7 + n * 2.0 ** -23 * np.abs(film)).sum())
    print(f"\nPROGRESSIVE gaussian r = 2, steps [3, 5, 8]: worst relative difference to rt_render {worst:.3e} (bound {n * 2.0 ** -23:.3e} + 1e-7), {over} values over")
    assert over == 0, worst


# ---------------------------------------------------------------------------------------------- 5
def test_pixel_bounds_and_crop(gpu_host):
    """pixel_bounds inside the sample bounds (the route where not every generated sample is traced) on a cropped film."""
    d = _cornell()
    d.integrator.pixel_bounds = (5, 21, 9, 30)     # x0 x1 y0 y1
    d.film.crop = (0.25, 0.75, 0.125, 1.0)
    h = gpu_host.HostScene(d)
    film, st = h.render()
    got, stats, _ = _step(h, [8, 8])
    differ = int((bits(got) != bits(film)).sum())
    print(f"\nPROGRESSIVE pixel bounds + crop, film {film.shape}: {differ} words differ; camera rays {sum(s['camera_rays'] for s in stats)} / {st['camera_rays']}")
    assert film.shape == (28, 16, 4) and film[..., 3].any()
    assert differ == 0 and sum(s["camera_rays"] for s in stats) == st["camera_rays"]


# ---------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("scene", ["room_env", "mis_plates"])
def test_other_routes_through_shade(gpu_host, scene):
    """room_env: the binned front-ends and the infinite light's occlusion-only MIS queue; mis_plates with analytic spheres: the QLIGHTS forms. Steps [2, 6]; the
    16-sample scene then takes its remaining 8 in a third step - a frame equals render() only once it is finished."""
    from rustracer_amd.scenes import mis_plates, room_env
    d = room_env(64, 36, 8, detail=2, tex_size=32, env_size=32) if scene == "room_env" else mis_plates(96, 54, 16, analytic_spheres=True)
    assert d.film.filter_kind == 0 and tuple(d.film.filter_params[:2]) == (0.5, 0.5)   # the default box filter
    h = gpu_host.HostScene(d)
    film, st = h.render()
    got, stats, _ = _step(h, [2, 6] if scene == "room_env" else [2, 6, 8])
    differ = int((bits(got) != bits(film)).sum())
    print(f"\nPROGRESSIVE {scene}: {differ} words differ from rt_render's; rays_mis_any {sum(s['rays_mis_any'] for s in stats)} / {st['rays_mis_any']}")
    assert differ == 0
    for k in COUNTS:
        assert sum(s[k] for s in stats) == st[k], k


# ---------------------------------------------------------------------------------------------- 7
def test_frames_do_not_share_state(cornell):
    """Two frames with different cameras and a plain render interleaved on one scene: each is the render of its own description."""
    h, film_a, _ = cornell
    pos_a, pos_b = tuple(h.desc.camera.pos), (250.0, 300.0, -780.0)
    try:
        h.desc.camera.pos = pos_b
        film_b, _ = h.render()
        b = h.progressive()
        h.desc.camera.pos = pos_a
        a = h.progressive()
        a.advance(4)
        b.advance(8)
        mid, _ = h.render()
        a.advance(12)
        b.advance(8)
        got_a, got_b = a.film(), b.film()
        a.close()
        b.close()
    finally:
        h.desc.camera.pos = pos_a
    d = [int((bits(x) != bits(y)).sum()) for x, y in ((got_a, film_a), (got_b, film_b), (mid, film_a))]
    print(f"\nPROGRESSIVE two frames + rt_render on one scene: words that differ A {d[0]}, B {d[1]}, the render in between {d[2]}; A and B differ in {int((bits(film_a) != bits(film_b)).sum())}")
    assert not np.array_equal(bits(film_a), bits(film_b))
    assert d == [0, 0, 0]


# ---------------------------------------------------------------------------------------------- 8
def test_shards(cornell):
    """Two ranks on one GPU with different steps. The merge is distributed.merge_film's arithmetic without a process group: rank 0 adds the rows rank 1 can have
    touched (distributed.touched_rows), in rank order; every other row of a rank's film is zero."""
    from rustracer_amd.distributed import owned_pixel_mask, touched_rows
    h, film, _ = cornell
    st = h.setup()
    cropped, sb = [int(v) for v in st["cropped"]], [int(v) for v in st["sample_bounds"]]
    parts = [_step(h, steps, rank=r, world_size=2)[0] for r, steps in ((0, [5, 11]), (1, [2, 2, 12]))]
    merged = parts[0].copy()
    rows = touched_rows(cropped, sb, 1, 2, 0.5)
    merged[rows] += parts[1][rows]
    differ = int((bits(merged) != bits(film)).sum())
    stray = []
    for r in range(2):
        untouched = np.setdiff1d(np.arange(film.shape[0]), touched_rows(cropped, sb, r, 2, 0.5))
        stray.append((int(np.count_nonzero(parts[r][untouched])), int(np.count_nonzero(parts[r][owned_pixel_mask(cropped, sb, 1 - r, 2)]))))
    print(f"\nPROGRESSIVE 2 shards: merged film differs from rt_render's in {differ} words; non-zero words outside a rank's touched rows / in the other rank's rows: {stray}")
    assert differ == 0 and stray == [(0, 0), (0, 0)]


# ---------------------------------------------------------------------------------------------- 9
def test_read_outs(gpu_host, cornell):
    import torch
    h, _, _ = cornell
    host = gpu_host
    scale = 1.75
    with h.progressive() as fr:
        for name, a in (("film", fr.film()), ("rgb", fr.rgb()), ("display", fr.display())):   # before the first step
            assert not a.any(), name
        assert fr.film().shape == (32, 32, 4) and fr.rgb().dtype == np.float32 and fr.display().shape == (32, 32, 3) and fr.display().dtype == np.uint8
        for n, k in ((4, 4), (12, 16)):
            fr.advance(n)
            film = fr.film()
            for sc, rgb in ((h.desc.film.scale, fr.rgb()), (scale, fr.rgb(scale=scale))):
                want = host.film_to_rgb(film, sc)
                differ = int((bits(rgb) != bits(want)).sum())
                print(f"\nPROGRESSIVE read-outs at k = {k}, scale {sc}: rgb words that differ from film_to_rgb {differ}")
                assert differ == 0
                disp = fr.display(scale=sc)
                want8 = host.rgb_to_png8(want)
                v = np.asarray(want, np.float32)
                c = np.float32
                with np.errstate(invalid="ignore"):
                    g = np.where(v <= c(0.0031308), c(12.92) * v, c(1.055) * np.power(np.maximum(v, c(0.0)), c(1.0) / c(2.4), dtype=np.float32) - c(0.055)).astype(np.float32)
                q = (c(255.0) * g + c(0.5)).astype(np.float64)
                off = disp != want8
                step = np.abs(disp.astype(np.int32) - want8.astype(np.int32))
                near = np.abs(q - np.rint(q)) <= 1e-3
                print(f"  display bytes that differ from rgb_to_png8: {int(off.sum())} of {off.size} (largest step {int(step.max())}), of them on a rounding boundary: {int((off & near).sum())}")
                assert step.max() <= 1 and not (off & ~near).any()
            assert np.array_equal(fr.display(), fr.display(scale=h.desc.film.scale))   # the default scale is the film's own
            dev_film = fr.film(device_out=torch.empty((32, 32, 4), dtype=torch.float32, device="cuda"))
            dev_rgb = fr.rgb(scale=scale, device_out=torch.empty((32, 32, 3), dtype=torch.float32, device="cuda"))
            dev_disp = fr.display(scale=scale, device_out=torch.empty((32, 32, 3), dtype=torch.uint8, device="cuda"))
            torch.cuda.synchronize()
            assert np.array_equal(bits(dev_film.cpu().numpy()), bits(film))
            assert np.array_equal(bits(dev_rgb.cpu().numpy()), bits(fr.rgb(scale=scale)))
            assert np.array_equal(dev_disp.cpu().numpy(), fr.display(scale=scale))
        assert fr.state_bytes >= 32 * 32 * 16 * 2 + 1024
