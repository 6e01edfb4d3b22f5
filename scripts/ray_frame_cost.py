"""What a ray frame costs beside the camera's frame (MEASUREMENTS "Ray frames").

    python scripts/ray_frame_cost.py [--film] [--res N] [--spp N] [--rounds N] [--out results/ray_frame_cost.json]

The benchmark's Cornell box cut to one RT_RAYS_MAX call (1024 x 1024 pixels x 128 samples = 2^27 rays by default). The camera's own rays are collected on the device
(rt_render_sample_features, window by window, RT_FLAG_FILM_ON_DEVICE) and laid out as rt_render_rays takes them; then, interleaved for --rounds rounds after a warm-up
of each: rt_render_rays over those device-resident rays into a device-resident radiance buffer, and rt_render_samples over the same pixels and samples, its radiance
device-resident too. Wall time
(a host clock around the device-synchronised call) and stats.ms_raygen (RT_FLAG_TIME_KERNELS, in rounds of their own so that the events do not sit in the wall times)
of both, medians; the difference is the price of streaming 32 B per ray in instead of computing the ray. The two radiance arrays are compared word for word."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def film_mode(a, h, rays, out):
    """--film: one step of a ray frame over all the call's samples (rt_frame_advance_rays, device-resident rays; p_film NULL, and an explicit device-resident p_film of
    pixel centres) beside rt_render_rays over the same rays, interleaved for --rounds rounds after a warm-up of each: ms_total of the call, and - in rounds of their own
    under RT_FLAG_TIME_KERNELS - ms_film and ms_raygen, medians. Every step is the first of a fresh frame begun with table_budget=1: its sampler tables are not resident,
    so the step builds them inside the timed call as rt_render_rays does; rt_frame_begin_rays itself (allocation, zeroing) is outside it. With RTX_LIB_DIR naming a library from before ray frames (MEASUREMENTS "Ray frames with a film": the parent commit's), only
    rt_render_rays is measured - run the two builds in alternating processes."""
    import torch
    from rustracer_amd import host
    n, spp = a.res, a.spp
    have_frames = hasattr(host.lib(), "rtxh_frame_begin_rays")
    pf = None
    if have_frames:
        ys, xs = torch.meshgrid(torch.arange(n, dtype=torch.float32, device="cuda") + 0.5, torch.arange(n, dtype=torch.float32, device="cuda") + 0.5, indexing="ij")
        pf = torch.stack([xs, ys], dim=-1)[:, :, None, :].expand(n, n, spp, 2).contiguous()

    def rays_call(timed):
        return h.render_rays(rays, device_out=out, time_kernels=timed)[1]

    def step(p_film, timed):
        with h.progressive_rays(n, n, spp=spp, table_budget=1, time_kernels=timed) as fr:
            st = fr.advance(rays, p_film)
            torch.cuda.synchronize()
            return st

    kinds = {"render_rays": rays_call}
    if have_frames:
        kinds["step"] = lambda timed: step(None, timed)
        kinds["step_p_film"] = lambda timed: step(pf, timed)
    for f in kinds.values():
        f(False)
    total = {k: [] for k in kinds}
    film = {k: [] for k in kinds}
    raygen = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for k, f in kinds.items():
            total[k].append(f(False)["ms_total"])
    for _ in range(a.rounds):
        for k, f in kinds.items():
            st = f(True)
            film[k].append(st["ms_film"]), raygen[k].append(st["ms_raygen"])
    med = lambda v: float(np.median(v))
    res = dict(mode="film", lib_dir=os.environ.get("RTX_LIB_DIR") or "", res=n, spp=spp, rays=n * n * spp, rounds=a.rounds,
               ms_total={k: med(v) for k, v in total.items()}, ms_film={k: med(v) for k, v in film.items()}, ms_raygen={k: med(v) for k, v in raygen.items()},
               all=dict(ms_total=total, ms_film=film, ms_raygen=raygen))
    print(f"cornell {n}x{n}x{spp} = {n * n * spp} device-resident rays, medians of {a.rounds}: " +
          "; ".join(f"{k} {res['ms_total'][k]:.2f} ms (ms_film {res['ms_film'][k]:.3f}, ms_raygen {res['ms_raygen'][k]:.3f})" for k in kinds))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--film", action="store_true", help="measure one ray-frame step (rt_frame_advance_rays, with and without p_film) beside rt_render_rays")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from rustracer_amd import host
    host.build()
    if not host.device_available():
        raise SystemExit("ray_frame_cost.py measures on an MI355X: no device visible")
    n, spp = a.res, a.spp
    if n * n * spp > host.RT_RAYS_MAX:
        raise SystemExit("one call holds at most RT_RAYS_MAX rays")
    d = bench.make_desc("cornell", spp, n)[0]
    d.film.filter_kind, d.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)   # box filter, radius 0.5: the sample bounds are the pixel bounds
    h = host.HostScene(d)
    h.upload(0)
    # the camera's rays, in bands of at most RT_FEATURE_SAMPLES_MAX samples
    rays = torch.zeros((n, n, spp, 8), dtype=torch.float32, device="cuda")
    rays[..., 3] = float("inf")
    rows = max(1, host.RT_FEATURE_SAMPLES_MAX // (n * spp))
    for y0 in range(0, n, rows):
        y1 = min(n, y0 + rows)
        d.integrator.pixel_bounds = (0, n, y0, y1)   # x0 x1 y0 y1
        feat = torch.empty((y1 - y0, n, spp, host.RT_FEATURE_FLOATS), dtype=torch.float32, device="cuda")
        h.sample_features(device_out=feat)
        rays[y0:y1, :, :, 0:3], rays[y0:y1, :, :, 4:7] = feat[..., 0:3], feat[..., 3:6]
        del feat
    d.integrator.pixel_bounds = None
    torch.cuda.synchronize()
    out = torch.empty((n, n, spp, 4), dtype=torch.float32, device="cuda")
    if a.film:
        return film_mode(a, h, rays, out)

    def ray_frame(timed):
        t0 = time.perf_counter()
        _, st = h.render_rays(rays, device_out=out, time_kernels=timed)
        return (time.perf_counter() - t0) * 1e3, st

    import ctypes as C
    out_cam = torch.empty((n, n, spp, 4), dtype=torch.float32, device="cuda")

    def camera_frame(timed):   # rt_render_samples with a device-resident radiance buffer as well (HostScene.render_samples copies to the host: 2 GiB here)
        p = h.setup()["params"]
        p.flags = host.RT_FLAG_FILM_ON_DEVICE | (host.RT_FLAG_TIME_KERNELS if timed else 0)
        st = host.Stats()
        L = host.lib()
        L.rtxh_render_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        t0 = time.perf_counter()
        rc = L.rtxh_render_samples(h.h, C.byref(p), None, C.c_void_p(out_cam.data_ptr()), None, C.byref(st))
        ms = (time.perf_counter() - t0) * 1e3
        if rc != 0:
            raise RuntimeError(f"rtxh_render_samples failed ({rc}): {L.rtxh_last_error()}")
        return ms, st.as_dict(), out_cam

    ray_frame(False)
    _, _, rad = camera_frame(False)
    differ = int((out.view(torch.int32) != rad.view(torch.int32)).sum().item())
    wall = {"rays": [], "samples": []}
    call = {"rays": [], "samples": []}
    raygen = {"rays": [], "samples": []}
    for _ in range(a.rounds):
        ms, st = ray_frame(False)
        wall["rays"].append(ms), call["rays"].append(st["ms_total"])
        ms, st, _ = camera_frame(False)
        wall["samples"].append(ms), call["samples"].append(st["ms_total"])
    for _ in range(a.rounds):
        raygen["rays"].append(ray_frame(True)[1]["ms_raygen"])
        raygen["samples"].append(camera_frame(True)[1]["ms_raygen"])
    med = lambda v: float(np.median(v))
    res = dict(res=n, spp=spp, rays=n * n * spp, rounds=a.rounds, radiance_words_differ=differ,
               wall_ms_rays=med(wall["rays"]), wall_ms_samples=med(wall["samples"]), call_ms_rays=med(call["rays"]), call_ms_samples=med(call["samples"]),
               raygen_ms_rays=med(raygen["rays"]), raygen_ms_samples=med(raygen["samples"]), all=dict(wall=wall, call=call, raygen=raygen))
    print(f"cornell {n}x{n}x{spp} = {n * n * spp} rays, medians of {a.rounds}: rt_render_rays (device rays, device radiance) {res['call_ms_rays']:.2f} ms in the call "
          f"({res['wall_ms_rays']:.2f} ms around the Python call); rt_render_samples (device radiance) {res['call_ms_samples']:.2f} ms ({res['wall_ms_samples']:.2f}); "
          f"ms_raygen {res['raygen_ms_rays']:.3f} vs {res['raygen_ms_samples']:.3f}; radiance words that differ {differ}")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
