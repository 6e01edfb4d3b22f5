"""What adaptive steps buy (MEASUREMENTS "Adaptive steps").

    python scripts/adaptive_report.py [--scenes room,cornell] [--res N] [--spp 256] [--step 16] [--thresholds 0.2,0.1] [--ref-spp 4096] [--out results/adaptive_report.json]

For the bench workload of each scene at --spp samples per pixel, in steps of --step: the uniformly stepped frame (every pixel takes every step; a stats frame), then
for each threshold the adaptive frame (rt_frame_advance_adaptive, floor 1e-3, min_samples = one step) until no pixel is active or the frame is finished:
samples taken / the full frame's, wall time / the full frame's, and the relative L2 distance to a --ref-spp render (Film::write_image's RGB) of (a) the adaptive
film and (b) a uniform frame of the nearest equal budget (round(samples taken / pixels) samples per pixel) - and, beside the L2 distance (which bright pixels and
fireflies dominate), the mean over the pixels of |Y - Y_ref| / max(Y_ref, 1e-3), the per-pixel relative error the criterion aims at. Last, what an INACTIVE sample
costs: ray generation + film time (RT_FLAG_TIME_KERNELS) of a step in which only the pixels of the largest ratio are active (threshold = the float32 just below
it; pixels with one non-zero sample so far all tie at ratio 1) against those of a full step.
Measurements, no pass mark."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOOR = 1e-3


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def rel_mean(a, b):
    """mean per-pixel relative luminance error"""
    lum = lambda v: 0.212671 * v[..., 0].astype(np.float64) + 0.715160 * v[..., 1] + 0.072169 * v[..., 2]
    return float(np.mean(np.abs(lum(a) - lum(b)) / np.maximum(lum(b), FLOOR)))


def main():
    import bench
    from rustracer_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="room,cornell")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--thresholds", default="0.2,0.1")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    host.build()
    thresholds = [float(v) for v in a.thresholds.split(",")]
    report = []
    for scene in a.scenes.split(","):
        ref_h = host.HostScene(bench.make_desc(scene, a.ref_spp, a.res)[0])
        ref_h.upload(0)
        ref = host.film_to_rgb(ref_h.render()[0], 1.0)
        del ref_h
        h = host.HostScene(bench.make_desc(scene, a.spp, a.res)[0])
        h.upload(0)
        whole = h.render()[1]["ms_total"]   # warm-up: workspace, light distribution
        whole = h.render()[1]["ms_total"]

        def uniform(k, stats=True):
            with h.progressive(pixel_stats=stats) as fr:
                t0 = time.perf_counter()
                while fr.samples_done < k:
                    fr.advance(min(a.step, k - fr.samples_done))
                ms = (time.perf_counter() - t0) * 1e3
                return host.film_to_rgb(fr.film(), 1.0), ms, fr.samples_taken

        uniform(a.step)   # the first stepped frame builds the resident sampler tables' buffers
        full_rgb, full_ms, full_taken = uniform(a.spp)
        _, plain_ms, _ = uniform(a.spp, stats=False)
        res = dict(scene=scene, shape=list(ref.shape), spp=a.spp, step=a.step, ref_spp=a.ref_spp, rt_render_ms=whole, full_stepped_ms=full_ms, full_stepped_without_stats_ms=plain_ms,
                   full_samples=full_taken, full_rel_l2=rel_l2(full_rgb, ref), full_rel_mean=rel_mean(full_rgb, ref), runs=[])
        print(f"{scene} {ref.shape[1]}x{ref.shape[0]}x{a.spp} in steps of {a.step}: rt_render {whole:.1f} ms, stepped with stats {full_ms:.1f} ms (without {plain_ms:.1f}), "
              f"to {a.ref_spp} spp: relative L2 {res['full_rel_l2']:.4e}, mean relative error {res['full_rel_mean']:.4e}", flush=True)
        for thr in thresholds:
            with h.progressive(pixel_stats=True) as fr:
                t0 = time.perf_counter()
                active = []
                while fr.samples_done < fr.spp:
                    fr.advance_adaptive(a.step, thr, FLOOR, min_samples=a.step)
                    active.append(fr.active_pixels)
                    if active[-1] == 0:
                        break
                ms = (time.perf_counter() - t0) * 1e3
                rgb, taken, n = host.film_to_rgb(fr.film(), 1.0), fr.samples_taken, fr.pixel_stats()[0]
            k = int(min(a.spp, max(1, round(taken / max(int(np.count_nonzero(n)), 1)))))
            uni_rgb, uni_ms, uni_taken = uniform(k)
            run = dict(threshold=thr, samples_taken=taken, samples_ratio=taken / full_taken, ms=ms, ms_ratio=ms / full_ms, steps=len(active), active_per_step=active,
                       rel_l2_adaptive=rel_l2(rgb, ref), uniform_spp=k, uniform_samples=uni_taken, uniform_ms=uni_ms, rel_l2_uniform=rel_l2(uni_rgb, ref),
                       rel_mean_adaptive=rel_mean(rgb, ref), rel_mean_uniform=rel_mean(uni_rgb, ref),
                       samples_per_pixel=dict(min=float(n.min()), median=float(np.median(n)), max=float(n.max())))
            res["runs"].append(run)
            print(f"  threshold {thr}: samples {taken} / {full_taken} = {run['samples_ratio']:.3f}, wall {ms:.1f} / {full_ms:.1f} ms = {run['ms_ratio']:.3f}, {len(active)} steps, "
                  f"relative L2 adaptive {run['rel_l2_adaptive']:.4e}, uniform {k} spp ({uni_taken} samples, {uni_ms:.1f} ms) {run['rel_l2_uniform']:.4e}; "
                  f"mean relative error adaptive {run['rel_mean_adaptive']:.4e}, uniform {run['rel_mean_uniform']:.4e}; "
                  f"samples per pixel min / median / max {n.min():.0f} / {np.median(n):.0f} / {n.max():.0f}", flush=True)
        # an inactive sample: a step in which only the pixels of the largest ratio are active against a full step, per-stage HIP-event times
        with h.progressive(pixel_stats=True, time_kernels=True) as fr:
            fr.advance(a.step)
            full = fr.advance(a.step)
            n, sy, sy2 = fr.pixel_stats()
            mean = sy / n
            ratio = np.sort((np.sqrt(np.maximum(0.0, sy2 - sy * mean) / (n - 1.0) / n) / np.maximum(mean, FLOOR)).ravel())
            thr1 = float(np.nextafter(np.float32(ratio[-1]), np.float32(0.0)))
            one = fr.advance_adaptive(a.step, thr1, FLOOR, min_samples=2)
            one_active = fr.active_pixels
            t0 = time.perf_counter()
            none = fr.advance_adaptive(a.step, float("inf"), FLOOR, min_samples=2)
            none_ms = (time.perf_counter() - t0) * 1e3
            assert fr.active_pixels == 0 and none["camera_rays"] == 0
        res["inactive"] = dict(active_pixels=one_active, camera_rays=one["camera_rays"], raygen_ms=one["ms_raygen"], film_ms=one["ms_film"], total_ms=one["ms_total"],
                               full_raygen_ms=full["ms_raygen"], full_film_ms=full["ms_film"], full_total_ms=full["ms_total"], no_active_pixel_call_ms=none_ms)
        i = res["inactive"]
        print(f"  a step with {one_active} active pixel(s): raygen {i['raygen_ms']:.2f} + film {i['film_ms']:.2f} ms, whole step {i['total_ms']:.2f} ms; a full step: raygen "
              f"{i['full_raygen_ms']:.2f} + film {i['full_film_ms']:.2f} ms, whole step {i['full_total_ms']:.2f} ms -> inactive samples cost "
              f"{(i['raygen_ms'] + i['film_ms']) / i['full_total_ms']:.3%} of a full step (the whole step {i['total_ms'] / i['full_total_ms']:.3%}); a step with no active pixel returns in {none_ms:.2f} ms", flush=True)
        report.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
