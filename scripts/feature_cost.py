"""What the first-hit feature planes cost (MEASUREMENTS "First-hit feature planes").

    python scripts/feature_cost.py [--scenes cornell,room] [--res N] [--spp N] [--step N] [--rounds N] [--parent-build DIR [--bench-steps K] [--bench-warmup W]]
                                   [--out results/feature_cost.json]

1. Per scene (the bench workload of that name): a frame of --spp samples per pixel stepped --step samples at a time, begun without and with RT_FLAG_FRAME_FEATURES, the two
   interleaved for --rounds rounds after a warm-up frame of each: the median step time (ms_total of rt_frame_advance: a host clock around device-synchronised work) of
   either, their ratio, one rt_frame_read(RT_FRAME_FEATURES), the state bytes; the two films are compared word for word.
2. --parent-build DIR: the default `bench.py --gpus 1` line of THIS build against the parent commit's libraries (DIR holds its librtx_hip.so and librtx_host.so), each in a
   process of its own (with --bench-args: by default the headline workload's timed frames alone), interleaved this / parent for --rounds rounds; medians of Msamples/s and
   their ratio. That path launches nothing new: a difference beyond the
   box's spread (README: +-2 % box to box) is a defect to find. The parent's process loads its libraries from DIR (RTX_LIB_DIR); nothing in the tree is touched."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames(a, res):
    import bench
    from rustracer_amd import host
    for scene in a.scenes.split(","):
        h = host.HostScene(bench.make_desc(scene, a.spp, a.res)[0])
        h.upload(0)
        times, films, extra = {False: [], True: []}, {}, {}
        for rnd in range(a.rounds + 1):   # round 0 warms both up (workspace, light distribution, code objects)
            for feat in (False, True):
                with h.progressive(features=feat) as fr:
                    ms = []
                    while fr.samples_done < fr.spp:
                        ms.append(fr.advance(a.step)["ms_total"])
                    if rnd:
                        times[feat] += ms[1:] if len(ms) > 1 else ms   # (a frame's first step builds its sampler tables)
                    films[feat] = fr.film()
                    if feat:
                        import time
                        fr.features()
                        t0 = time.perf_counter()
                        planes = fr.features()
                        extra = dict(read_ms=(time.perf_counter() - t0) * 1e3, state_bytes=fr.state_bytes, mean_coverage=float(planes[..., 7].mean()))
                    else:
                        extra_plain = fr.state_bytes
        med = {k: float(np.median(v)) for k, v in times.items()}
        differ = int((films[False].view(np.uint32) != films[True].view(np.uint32)).sum())
        run = dict(scene=scene, res=a.res, spp=a.spp, step=a.step, rounds=a.rounds, steps_timed=len(times[True]), step_ms_plain=med[False], step_ms_features=med[True],
                   ratio=med[True] / med[False], spread_plain=[float(np.min(times[False])), float(np.max(times[False]))], spread_features=[float(np.min(times[True])), float(np.max(times[True]))],
                   film_words_differ=differ, state_bytes_plain=extra_plain, **extra)
        res["frames"].append(run)
        print(f"{scene} {a.res}x{a.res}, steps of {a.step} samples ({len(times[True])} timed per variant): {med[False]:.2f} ms without, {med[True]:.2f} ms with the planes = {run['ratio']:.4f} x "
              f"(without: {run['spread_plain'][0]:.2f} .. {run['spread_plain'][1]:.2f} ms, with: {run['spread_features'][0]:.2f} .. {run['spread_features'][1]:.2f}); read {extra['read_ms']:.2f} ms; "
              f"state {extra_plain / 2**20:.1f} -> {extra['state_bytes'] / 2**20:.1f} MiB; film words that differ {differ}; mean coverage {extra['mean_coverage']:.3f}", flush=True)


def bench_lines(a, res):
    rates = {"this": [], "parent": []}
    for rnd in range(a.rounds):
        for which in ("this", "parent"):
            env = dict(os.environ)
            if which == "parent":
                env["RTX_LIB_DIR"] = os.path.abspath(a.parent_build)   # (host.py loads the libraries from there; nothing in the tree is touched)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)] + a.bench_args.split(),
                               capture_output=True, text=True, cwd=ROOT, timeout=900, env=env)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py ({which}) failed: {r.stderr[-1000:]}")
            line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            rate = float(line["value"])   # Msamples/s of the timed frames
            rates[which].append(rate)
            print(f"  bench.py round {rnd + 1}, {which}: {rate:.1f}", flush=True)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    res["bench"] = dict(rates=rates, median_this=med["this"], median_parent=med["parent"], ratio=med["this"] / med["parent"], steps=a.bench_steps, warmup=a.bench_warmup)
    print(f"bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}: this build {med['this']:.1f}, parent {med['parent']:.1f} (medians of {a.rounds}) = {res['bench']['ratio']:.4f} x", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,room")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--step", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-build", default=None)
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--bench-args", default="--headline-only --no-cpu-baseline", help="further bench.py arguments (default: the timed frames of the headline workload alone)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from rustracer_amd import host
    host.build()
    if not host.device_available():
        raise SystemExit("feature_cost.py measures on an MI355X: no device visible")
    res = dict(frames=[])
    frames(a, res)
    if a.parent_build:
        bench_lines(a, res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
