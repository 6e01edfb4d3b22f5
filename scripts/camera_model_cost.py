"""What generating a camera model's rays on the device buys (MEASUREMENTS "Camera models on the device").

    python scripts/camera_model_cost.py [--scene room] [--res 512] [--spp 16] [--step 4] [--rounds 5] [--out results/camera_model_cost.json]

The bench workload of that name at --res x --res, --spp samples per pixel in steps of --step, through three frames, interleaved for --rounds rounds after a warm-up round
of each:
  model        the environment camera through HostScene.progressive_model (rt_frame_begin_model): rays generated on the device, with differentials;
  host rays    the same records and film positions (camera_model_rays' output, in host memory) through HostScene.progressive_rays: every step uploads them;
  perspective  the scene's own camera through HostScene.progressive.
Per frame the first step is dropped (it builds the frame's sampler tables) unless it is the only one. Step time is ms_total of the advance call - a host clock around device-synchronised work,
the upload of a host-fed step included; ms_raygen comes from frames of their own begun with RT_FLAG_TIME_KERNELS. Medians over all timed steps, the two ratios, and - for
scale - the time numpy takes to compute one step's rays with rustracer_amd/cameras.py, which a host-fed frame pays on top. The model frame's sums are compared with the
host-fed frame's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="room")
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--step", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="results/camera_model_cost.json")
    a = ap.parse_args()
    import bench
    from rustracer_amd import cameras, host
    host.build()
    d = bench.make_desc(a.scene, a.spp, a.res)[0]
    d.film.xres = d.film.yres = a.res   # (make_desc sizes only the cornell box by `res`)
    h = host.HostScene(d)
    h.upload(0)
    cam = h.camera_model_params("environment")
    rays, pf = h.camera_model_rays("environment", cam, differentials=True)
    steps = [(s0, min(a.step, a.spp - s0)) for s0 in range(0, a.spp, a.step)]
    cuts = [(np.ascontiguousarray(rays[:, :, s0:s0 + n]), np.ascontiguousarray(pf[:, :, s0:s0 + n])) for s0, n in steps]

    def run(kind, time_kernels):
        if kind == "model":
            fr = h.progressive_model("environment", cam, differentials=True, time_kernels=time_kernels)
        elif kind == "host rays":
            fr = h.progressive_rays(a.res, a.res, time_kernels=time_kernels)
        else:
            fr = h.progressive(time_kernels=time_kernels)
        with fr:
            st = [fr.advance(r, p) if kind == "host rays" else fr.advance(n) for (r, p), (_, n) in zip(cuts, steps)]
            return st, fr.sums()

    kinds = ("model", "host rays", "perspective")
    wall, raygen, sums = {k: [] for k in kinds}, {k: [] for k in kinds}, {}
    for rnd in range(a.rounds + 1):   # round 0 warms every path up (workspace, light distribution, code objects)
        for k in kinds:
            st, sums[k] = run(k, False)
            tk, _ = run(k, True)
            if rnd:
                wall[k] += [s["ms_total"] for s in (st[1:] or st)]   # (a frame of one step has only that one: its time holds the table build)
                raygen[k] += [s["ms_raygen"] for s in (tk[1:] or tk)]
    t0 = time.perf_counter()
    p = np.asarray(cuts[0][1], np.float64)
    cameras.environment(np.float32(cam[:16]).reshape(4, 4), a.res, a.res, p, differentials=True, spp=a.spp)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    med = {k: float(np.median(v)) for k, v in wall.items()}
    med_rg = {k: float(np.median(v)) for k, v in raygen.items()}
    res = dict(scene=a.scene, res=a.res, spp=a.spp, step=a.step, rounds=a.rounds, steps_timed=len(wall["model"]), step_ms=med, ms_raygen=med_rg,
               spread_ms={k: [float(np.min(v)), float(np.max(v))] for k, v in wall.items()},
               model_over_perspective=med["model"] / med["perspective"], model_over_host_rays=med["model"] / med["host rays"],
               upload_bytes_per_step=int(cuts[0][0].nbytes + cuts[0][1].nbytes), numpy_ms_per_step=numpy_ms,
               sum_bytes_differing_model_vs_host_rays=int((sums["model"].view(np.uint8) != sums["host rays"].view(np.uint8)).sum()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"{a.scene} {a.res}x{a.res}, steps of {a.step} samples ({res['steps_timed']} timed per path), median step ms (min .. max) / ms_raygen:")
    for k in kinds:
        print(f"  {k:12s} {med[k]:8.2f} ({res['spread_ms'][k][0]:.2f} .. {res['spread_ms'][k][1]:.2f}) / {med_rg[k]:.3f}")
    print(f"  model / perspective {res['model_over_perspective']:.3f}; model / host rays {res['model_over_host_rays']:.3f}; a host-fed step uploads "
          f"{res['upload_bytes_per_step'] / 2**20:.0f} MiB and numpy takes {numpy_ms:.0f} ms to compute its rays; sum bytes differing model / host rays "
          f"{res['sum_bytes_differing_model_vs_host_rays']}")


if __name__ == "__main__":
    main()
