"""What an ambient-occlusion frame costs (rt_render_ao), for MEASUREMENTS.md.

    python scripts/ao_cost.py [--res 256] [--spp 4] [--ao 8] [--reps 5] [--scenes cornell,room] [--json out.json]

Per scene: the wall time of HostScene.render_ao into a device buffer (median of --reps calls after one warm-up call) and, from one more call under
RT_FLAG_TIME_KERNELS, the HIP-event times of its stages - ms_trace_closest (the camera rays), ms_trace_any (the occlusion rays: the scene's own any-hit launches, the
yardstick) and ms_shade (k_ao_rays, once per occlusion sample, plus k_ao_finish). For comparison the same scene's rt_render frame. Prints one JSON line per scene."""
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
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--ao", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="cornell,room")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from rustracer_amd import host
    from rustracer_amd.scenes import cornell_box, room_env
    host.build()
    make = dict(cornell=lambda: cornell_box(a.res, a.res, a.spp), room=lambda: room_env(a.res, a.res, a.spp))
    rows = []
    for name in a.scenes.split(","):
        h = host.HostScene(make[name]())
        h.upload(0)
        st = h.setup()
        cr = st["cropped"]
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

        ao_wall = wall(lambda: h.render_ao(a.ao, device_out=out))
        _, k = h.render_ao(a.ao, device_out=out, time_kernels=True)
        path_wall = wall(lambda: h.render(device_out=out))
        row = dict(scene=name, res=a.res, spp=a.spp, ao_samples=a.ao, ao_wall_ms_median=round(ao_wall[0], 3), ao_wall_ms_min=round(ao_wall[1], 3), ao_wall_ms_max=round(ao_wall[2], 3),
                   ms_trace_closest=round(k["ms_trace_closest"], 3), ms_trace_any=round(k["ms_trace_any"], 3), ms_shade=round(k["ms_shade"], 3), ms_raygen=round(k["ms_raygen"], 3),
                   ms_sampler=round(k["ms_sampler"], 3), ms_film=round(k["ms_film"], 3), ms_total_timed_call=round(k["ms_total"], 3), camera_rays=k["camera_rays"],
                   rays_shadow=k["rays_shadow"], mean_film_y=round(float(out[..., 1].mean() / out[..., 3].mean()), 4), path_wall_ms_median=round(path_wall[0], 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
