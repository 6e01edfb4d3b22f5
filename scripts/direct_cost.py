"""What a direct-lighting frame costs (rt_render_direct) beside a Whitted frame, for MEASUREMENTS.md.

    python scripts/direct_cost.py [--res 256] [--spp 16] [--depth 5] [--reps 5] [--json out.json]

The Cornell box, rendered three ways into a device buffer: rt_render_whitted, rt_render_direct under strategy "one" and under strategy "all". Per way the wall time
(median of --reps calls after one warm-up call) and, from one more call under RT_FLAG_TIME_KERNELS, the HIP-event times of its stages: ms_trace_closest (the li rays),
ms_trace_any (the visibility segments), ms_trace_mis (the BSDF-sampled probe rays), ms_vertex (k_whitted_vertex / k_direct_vertex: ms_shade less the array tables),
ms_array_tables (k_sampler_array_tables, "all" only: rt_stats::ms_shade_bin of such a call), ms_probe (k_direct_probe: ms_resolve), ms_sampler (K0), ms_raygen, ms_film.
Prints one JSON line per way. No threshold: the array-table figure is what decides whether a segmented form of that kernel is worth building."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from rustracer_amd import host
    from rustracer_amd.scenes import cornell_box
    host.build()
    h = host.HostScene(cornell_box(a.res, a.res, a.spp))
    h.upload(0)
    cr = h.setup()["cropped"]
    out = torch.zeros((int(cr[3] - cr[1]), int(cr[2] - cr[0]), 4), dtype=torch.float32, device="cuda")

    def wall(call):
        call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    ways = (("whitted", lambda **kw: h.render_whitted(a.depth, device_out=out, **kw)),
            ("direct one", lambda **kw: h.render_direct(a.depth, "one", device_out=out, **kw)),
            ("direct all", lambda **kw: h.render_direct(a.depth, "all", device_out=out, **kw)))
    rows = []
    for name, call in ways:
        w = wall(call)
        _, k = call(time_kernels=True)
        r3 = lambda v: round(float(v), 3)
        row = dict(way=name, res=a.res, spp=a.spp, max_depth=a.depth, wall_ms_median=r3(w[0]), wall_ms_min=r3(w[1]), wall_ms_max=r3(w[2]),
                   ms_trace_closest=r3(k["ms_trace_closest"]), ms_trace_any=r3(k["ms_trace_any"]), ms_trace_mis=r3(k["ms_trace_mis"]),
                   ms_vertex=r3(k["ms_shade"] - k["ms_shade_bin"]), ms_array_tables=r3(k["ms_shade_bin"]), ms_probe=r3(k["ms_resolve"]), ms_sampler=r3(k["ms_sampler"]),
                   ms_raygen=r3(k["ms_raygen"]), ms_film=r3(k["ms_film"]), ms_total_timed_call=r3(k["ms_total"]), camera_rays=k["camera_rays"], rays_closest=k["rays_closest"],
                   rays_shadow=k["rays_shadow"], rays_mis=k["rays_mis"], launches_vertex=k["launches_shade"], launches_probe=k["launches_trace_mis"], n_passes=k["n_passes"],
                   mean_film_y=round(float(out[..., 1].mean() / out[..., 3].mean()), 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
