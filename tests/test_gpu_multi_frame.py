"""Progressive and adaptive frames across several workers of one process (rt_multi_frame_* through HostScene.progressive_multi), with the workers [0], [0, 0] and
[0, 0, 0] on the one GPU. One worker is rt_frame in every read-out, bit for bit; several workers give the single-device frame's statistics plane, active pixels,
samples taken and - under the box filter - its film, bit for bit at every step; a wide filter stays inside the bound of test_gpu_progressive.test_wide_filter.
Films are compared as bit patterns; every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

from util import bits

pytestmark = pytest.mark.gpu

STEPS = [3, 5, 8]
SCALE = 1.75
COUNTS = ("camera_rays", "rays_closest", "rays_shadow", "rays_mis", "vertices_lambert_const", "vertices_lambert", "vertices_two_lobe", "vertices_generic")
WORKERS = {"2": [0, 0], "3": [0, 0, 0]}


def _cornell(w=32, h=32, filter_kind=0, filter_params=(0.5, 0.5, 0.0, 0.0)):
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(w, h, 16)
    d.film.filter_kind, d.film.filter_params = filter_kind, filter_params   # default: box filter, radius 0.5
    return d


def _read_outs(fr):
    """XYZW, RGB at the film's scale and at another, the 8-bit pixels."""
    return dict(film=fr.film(), rgb=fr.rgb(), rgb_scaled=fr.rgb(scale=SCALE), display=fr.display())


def _differ(a, b):
    if a.dtype == np.uint8:
        return int((a != b).sum())
    return int((bits(a) != bits(b)).sum())


def _zero(st):
    return all(v == 0 for k, v in st.items() if k != "shade_section_cycles") and not any(st["shade_section_cycles"])


@pytest.fixture(scope="module")
def cornell(gpu_host):
    """The 32 x 32 x 16 Cornell box under the box filter: the scene, its whole-frame film and stats, and a single-device frame's read-outs (and statistics) after
    each of STEPS - rendered once, left unchanged."""
    h = gpu_host.HostScene(_cornell())
    film, st = h.render()
    film.setflags(write=False)
    single = []
    with h.progressive(pixel_stats=True) as fr:
        for n in STEPS:
            fr.advance(n)
            r = _read_outs(fr)
            r["stats"] = np.stack(fr.pixel_stats(), -1)
            single.append(r)
    return dict(h=h, film=film, st=st, single=single)


# ---------------------------------------------------------------------------------------------- 1
def test_one_worker_is_rt_frame(cornell):
    h = cornell["h"]
    with h.progressive_multi([0], pixel_stats=True) as fr:
        assert fr.spp == 16 and fr.samples_done == 0 and not fr.film().any()
        done = 0
        for n, want in zip(STEPS, cornell["single"]):
            total, per = fr.advance(n)
            done += n
            got = _read_outs(fr)
            got["stats"] = np.stack(fr.pixel_stats(), -1)
            d = {k: (int((got[k] != want[k]).sum()) if k == "stats" else _differ(got[k], want[k])) for k in want}
            print(f"\nMULTI FRAME [0] after {done} samples: words / bytes that differ from rt_frame's {d}; camera rays {total['camera_rays']} = {per[0]['camera_rays']}")
            assert fr.samples_done == done and len(per) == 1 and total["camera_rays"] == per[0]["camera_rays"] == 32 * 32 * n
            assert all(v == 0 for v in d.values()), d
        assert np.array_equal(bits(fr.film()), bits(cornell["film"]))
        assert fr.tables_resident and fr.state_bytes >= 32 * 32 * (16 * 2 + 32) + 1024


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("workers", list(WORKERS), ids=lambda w: w + " workers")
def test_several_workers_give_the_single_device_film(cornell, workers):
    """Box filter: a pixel's sum is its own samples in index order on its owner, every other contribution is zero or one edge splat - bit-equal at every step."""
    h, st = cornell["h"], cornell["st"]
    dev = WORKERS[workers]
    sums = {k: 0 for k in COUNTS}
    with h.progressive_multi(dev) as fr:
        done = 0
        for n, want in zip(STEPS, cornell["single"]):
            total, per = fr.advance(n)
            done += n
            got = _read_outs(fr)
            d = {k: _differ(got[k], want[k]) for k in got}
            print(f"\nMULTI FRAME {dev} after {done} samples: words / bytes that differ from the single-device frame's {d}; camera rays per worker {[p['camera_rays'] for p in per]}")
            assert len(per) == len(dev) and fr.samples_done == done
            assert all(v == 0 for v in d.values()), d
            for k in COUNTS:
                assert total[k] == sum(p[k] for p in per), k
                sums[k] += total[k]
            assert all(p["camera_rays"] > 0 for p in per) and total["ms_total"] > 0
        differ = int((bits(fr.film()) != bits(cornell["film"])).sum())
        print(f"  finished: {differ} words differ from rt_render's; counters {sums} / rt_render {[st[k] for k in COUNTS]}")
        assert differ == 0
        for k in COUNTS:
            assert sums[k] == st[k], k
        assert fr.samples_taken == st["camera_rays"]


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("workers", list(WORKERS), ids=lambda w: w + " workers")
def test_statistics_and_adaptive_steps(cornell, workers):
    """advance(4), then three adaptive steps of 4 at a threshold that leaves part of the image active (the median ratio after the first step). Both sides run the
    same IEEE double arithmetic on the same plane, pixel by pixel: equal, no allowance."""
    h = cornell["h"]
    dev = WORKERS[workers]
    floor_y = 1e-3
    with h.progressive(pixel_stats=True) as one, h.progressive_multi(dev, pixel_stats=True) as fr:
        one.advance(4)
        total, per = fr.advance(4)
        mean, se = one.noise()
        thr = float(np.float32(np.median(se / np.maximum(mean, floor_y))))
        calls = [None, thr, thr, thr]
        for i, t in enumerate(calls):
            if t is not None:
                st1 = one.advance_adaptive(4, t, floor_y=floor_y)
                total, per = fr.advance_adaptive(4, t, floor_y=floor_y)
                assert total["camera_rays"] == st1["camera_rays"] == sum(p["camera_rays"] for p in per)
            a, b = np.stack(one.pixel_stats(), -1), np.stack(fr.pixel_stats(), -1)
            film_differ = int((bits(one.film()) != bits(fr.film())).sum())
            print(f"\nMULTI FRAME {dev} call {i} (threshold {t}): statistics equal {np.array_equal(a, b)}, active {fr.active_pixels} / {one.active_pixels}, "
                  f"taken {fr.samples_taken} / {one.samples_taken}, film words that differ {film_differ}")
            assert np.array_equal(a, b)
            assert fr.active_pixels == one.active_pixels and fr.samples_taken == one.samples_taken and fr.samples_done == one.samples_done
            assert film_differ == 0
            if i == 1:
                assert 0 < one.active_pixels < 32 * 32, "the threshold leaves part of the image active"
        mean2, se2 = fr.noise()
        assert np.array_equal(mean2, one.noise()[0]) and np.array_equal(se2, one.noise()[1])


# ---------------------------------------------------------------------------------------------- 4
def test_wide_filter(gpu_host):
    """Gaussian, radius 2, two workers: test_gpu_progressive.test_wide_filter's bound against rt_render, unchanged - all weights are positive, every partial sum is
    bounded by the result, and the only difference is the order of the additions: n * 2^-23 relative with n = 16 * 5 * 5 taps at most per pixel, plus 1e-7."""
    from rustracer_amd.scene_desc import FILTER_GAUSSIAN
    h = gpu_host.HostScene(_cornell(filter_kind=FILTER_GAUSSIAN, filter_params=(2.0, 2.0, 2.0, 0.0)))
    film, _ = h.render()
    with h.progressive_multi([0, 0]) as fr:
        for n in STEPS:
            fr.advance(n)
        got = fr.film()
    n = 16 * 5 * 5
    err = np.abs(got.astype(np.float64) - film)
    worst = float(np.max(err / np.maximum(np.abs(film), 1e-30)))
    over = int((err > 1e-7 + n * 2.0 ** -23 * np.abs(film)).sum())
    print(f"\nMULTI FRAME gaussian r = 2, [0, 0], steps {STEPS}: worst relative difference to rt_render {worst:.3e} (bound {n * 2.0 ** -23:.3e} + 1e-7), {over} values over")
    assert over == 0, worst


# ---------------------------------------------------------------------------------------------- 5
def _finish(h, dev, steps):
    """The finished film, the per-worker sums of camera_rays and whether every step of a worker was all zero."""
    with h.progressive_multi(dev) as fr:
        rays, all_zero = [0] * len(dev), [True] * len(dev)
        for n in steps:
            _, per = fr.advance(n)
            for k, p in enumerate(per):
                rays[k] += p["camera_rays"]
                all_zero[k] = all_zero[k] and _zero(p)
        assert fr.samples_done == fr.spp
        return fr.film(), rays, all_zero


@pytest.mark.parametrize("height,workers", [(4, "2"), (4, "3"), (6, "2"), (6, "3")])
def test_few_rows(gpu_host, height, workers):
    """4 rows are one band of RT_SHARD_ROWS = 4: every worker but the first owns nothing; 6 rows are a full band and a partial one: the third worker owns nothing."""
    dev = WORKERS[workers]
    h = gpu_host.HostScene(_cornell(32, height))
    film, st = h.render()
    got, rays, all_zero = _finish(h, dev, [8, 8])
    differ = int((bits(got) != bits(film)).sum())
    n_bands = (height + 3) // 4
    print(f"\nMULTI FRAME {height} rows, {dev}: {differ} words differ from rt_render's; camera rays per worker {rays} / {st['camera_rays']}; all-zero step stats {all_zero}")
    assert differ == 0 and sum(rays) == st["camera_rays"]
    assert all_zero == [k >= n_bands for k in range(len(dev))]


@pytest.mark.parametrize("pixel_bounds,idle", [((5, 21, 9, 30), None), ((5, 21, 8, 12), 0)], ids=["every worker traces", "worker 0 has nothing to trace"])
def test_pixel_bounds_and_crop(gpu_host, pixel_bounds, idle):
    """The cropped film of test_gpu_progressive.test_pixel_bounds_and_crop (sample rows 4 .. 32: bands of 4 rows from row 4 on). Its own pixel_bounds reach both
    workers; rows 8 .. 12 are one band of worker 1, so worker 0 has nothing to trace: it raises no error and its step stats are zero."""
    d = _cornell()
    d.integrator.pixel_bounds = pixel_bounds     # x0 x1 y0 y1
    d.film.crop = (0.25, 0.75, 0.125, 1.0)
    h = gpu_host.HostScene(d)
    film, st = h.render()
    got, rays, all_zero = _finish(h, [0, 0], [8, 8])
    differ = int((bits(got) != bits(film)).sum())
    print(f"\nMULTI FRAME pixel bounds {pixel_bounds} + crop, film {film.shape}: {differ} words differ; camera rays per worker {rays} / {st['camera_rays']}; all-zero step stats {all_zero}")
    assert film.shape == (28, 16, 4) and film[..., 3].any()
    assert differ == 0 and sum(rays) == st["camera_rays"]
    assert all_zero == [k == idle for k in range(2)]


# ---------------------------------------------------------------------------------------------- 6
def test_other_routes_through_shade(gpu_host):
    """room_env: the binned front-ends and the infinite light's occlusion-only MIS queue, through two workers."""
    from rustracer_amd.scenes import room_env
    d = room_env(64, 36, 8, detail=2, tex_size=32, env_size=32)
    assert d.film.filter_kind == 0 and tuple(d.film.filter_params[:2]) == (0.5, 0.5)   # the default box filter
    h = gpu_host.HostScene(d)
    film, st = h.render()
    with h.progressive_multi([0, 0]) as fr:
        stats = [fr.advance(n)[0] for n in (2, 6)]
        got = fr.film()
    differ = int((bits(got) != bits(film)).sum())
    print(f"\nMULTI FRAME room_env [0, 0]: {differ} words differ from rt_render's; rays_mis_any {sum(s['rays_mis_any'] for s in stats)} / {st['rays_mis_any']}")
    assert differ == 0
    for k in COUNTS + ("rays_mis_any",):
        assert sum(s[k] for s in stats) == st[k], k


# ---------------------------------------------------------------------------------------------- 7
def test_device_output_and_an_interleaved_render_multi(cornell):
    import torch
    h = cornell["h"]
    with h.progressive_multi([0, 0], pixel_stats=True) as fr:
        fr.advance(3)
        mid, _, _ = h.render_multi([0, 0])   # the same replicas, between two steps
        before = _read_outs(fr)
        fr.advance(5)
        host_out = _read_outs(fr)
        host_stats = np.stack(fr.pixel_stats(), -1)
        dev_film = fr.film(device_out=torch.empty((32, 32, 4), dtype=torch.float32, device="cuda:0"))
        dev_rgb = fr.rgb(scale=SCALE, device_out=torch.empty((32, 32, 3), dtype=torch.float32, device="cuda:0"))
        dev_disp = fr.display(device_out=torch.empty((32, 32, 3), dtype=torch.uint8, device="cuda:0"))
        dev_stats = torch.empty((32, 32, 3), dtype=torch.float64, device="cuda:0")
        fr.pixel_stats(device_out=dev_stats)
        torch.cuda.synchronize()
        d_dev = [_differ(dev_film.cpu().numpy(), host_out["film"]), _differ(dev_rgb.cpu().numpy(), host_out["rgb_scaled"]), _differ(dev_disp.cpu().numpy(), host_out["display"]),
                 int((dev_stats.cpu().numpy() != host_stats).sum())]
        d_mid = int((bits(mid) != bits(cornell["film"])).sum())
        d_before = {k: _differ(before[k], cornell["single"][0][k]) for k in before}
        d_after = {k: _differ(host_out[k], cornell["single"][1][k]) for k in host_out}
        print(f"\nMULTI FRAME device read-outs differ from the host's in {d_dev}; render_multi between two steps differs from rt_render in {d_mid} words; "
              f"the frame before / after it differs from the single-device frame in {d_before} / {d_after}")
        assert d_dev == [0, 0, 0, 0] and d_mid == 0
        assert all(v == 0 for v in d_before.values()) and all(v == 0 for v in d_after.values())
        assert np.array_equal(host_stats, cornell["single"][1]["stats"])


# ---------------------------------------------------------------------------------------------- 8
def test_refusals(gpu_host, cornell):
    host, h = gpu_host, cornell["h"]
    # RT_FLAG_REF_STREAM has no keyword: through the host layer's entry point itself
    st = h.setup()
    p = st["params"]
    p.flags = host.RT_FLAG_REF_STREAM
    dev = np.array([0, 0], np.int32)
    out = C.c_void_p(0x1234)
    rc = host.lib().rtxh_multi_frame_begin(h.h, C.byref(p), dev.ctypes.data_as(C.POINTER(C.c_int32)), 2, C.c_uint64(0), C.byref(out))
    msg = host.lib().rtxh_last_error().decode()
    print(f"\nMULTI FRAME refusals: RT_FLAG_REF_STREAM -> {rc}, {msg!r}")
    assert rc == -1 and out.value is None and "reference-stream" in msg
    with h.progressive_multi([0, 0]) as fr:   # no statistics flag
        fr.advance(2)
        for call, word in ((lambda: fr.pixel_stats(), "RT_FLAG_FRAME_STATS"), (lambda: fr.advance_adaptive(2, 0.1), "RT_FLAG_FRAME_STATS"), (lambda: fr.advance(0), "n_samples"),
                           (lambda: fr.advance(-3), "n_samples")):
            with pytest.raises(host.BackendError) as e:
                call()
            print(f"  refused: {e.value}")
            assert word in str(e.value) and "(-1)" in str(e.value)
        assert fr.samples_done == 2
    with h.progressive_multi([0, 0], pixel_stats=True) as fr:
        for kw, word in ((dict(n=4, threshold=float("nan")), "threshold"), (dict(n=0, threshold=0.1), "n_samples"), (dict(n=4, threshold=-1.0), "threshold"),
                         (dict(n=4, threshold=0.1, floor_y=float("nan")), "floor_y"), (dict(n=4, threshold=0.1, min_samples=-1), "min_samples")):
            with pytest.raises(host.BackendError) as e:
                fr.advance_adaptive(**kw)
            print(f"  refused {kw}: {e.value}")
            assert word in str(e.value) and "(-1)" in str(e.value)
        assert fr.samples_done == 0 and fr.samples_taken == 0 and not fr.film().any()
        fr.advance(16)
        film = fr.film()
        for total, per in (fr.advance(4), fr.advance_adaptive(4, 0.1)):   # a finished frame: RT_OK, zero stats, the same bytes
            assert _zero(total) and all(_zero(p) for p in per), (total, per)
        assert fr.samples_done == 16 and np.array_equal(bits(fr.film()), bits(film)) and np.array_equal(bits(film), bits(cornell["film"]))
