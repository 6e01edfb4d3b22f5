"""What rendering a frame in steps costs (MEASUREMENTS "Progressive frames").

    python scripts/progressive_cost.py [--scene cornell|room|...] [--res N] [--spp N] [--steps 8,64] [--out results/progressive_cost.json]

For the bench workload of the scene: rt_render's ms_total (median of --frames frames after a warm-up), then the frame stepped in each of --steps equal steps, with
resident sampler tables and with table_budget = 1 (every step rebuilds them): the sum of the steps' ms_total, its ratio to rt_render's, the first step's share, one
rt_frame_read of each kind, RT_FRAME_STATE_BYTES; and, for the first step count with resident tables, the per-stage HIP-event times (RT_FLAG_TIME_KERNELS) of the
stepped frame beside rt_render's. Every stepped film is compared with rt_render's bytes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("ms_sampler", "ms_raygen", "ms_trace_closest", "ms_trace_any", "ms_trace_mis", "ms_shade", "ms_resolve", "ms_film")


def main():
    import bench
    from rustracer_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--steps", default="8,64")
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    host.build()
    spp = a.spp or {"cornell": 1024, "blob": 256, "mis": 512, "room": 1024}.get(a.scene, 1024)
    h = host.HostScene(bench.make_desc(a.scene, spp, a.res)[0])
    h.upload(0)
    film, _ = h.render()                                    # warm-up: workspace, light distribution
    whole = sorted(h.render()[1]["ms_total"] for _ in range(a.frames))[a.frames // 2]
    timed = h.render(time_kernels=True)[1]
    res = dict(scene=a.scene, spp=spp, shape=list(film.shape), rt_render_ms=whole, rt_render_stages={k: timed[k] for k in STAGES}, runs=[])
    print(f"{a.scene} {film.shape[1]}x{film.shape[0]}x{spp}: rt_render {whole:.1f} ms", flush=True)
    again, _ = h.render()
    res["rt_render_words_differ_between_calls"] = int((again.view(np.uint32) != film.view(np.uint32)).sum())
    with h.progressive() as fr:   # does the default budget (a quarter of the free memory, the workspace being allocated) hold the tables?
        default_resident = fr.tables_resident
    res["default_budget_resident"] = default_resident
    print(f"  two rt_render calls differ in {res['rt_render_words_differ_between_calls']} words; tables resident under the default budget: {default_resident}", flush=True)
    first = True
    for n_steps in [int(v) for v in a.steps.split(",")]:
        for resident in (True, False):
            budget = 1 if not resident else (None if default_resident else 1 << 36)
            with h.progressive(table_budget=budget) as fr:
                assert fr.tables_resident == resident, fr.tables_resident
                n = max(1, fr.spp // n_steps)
                ms = []
                while fr.samples_done < fr.spp:
                    ms.append(fr.advance(n)["ms_total"])
                reads = {}
                for name, call in (("xyzw", fr.film), ("rgb", fr.rgb), ("rgb8", fr.display)):
                    call()
                    t0 = time.perf_counter()
                    got = call()
                    reads[name] = (time.perf_counter() - t0) * 1e3
                    if name == "xyzw":   # against rt_render's film: words that differ, and by how much (a pixel that receives two or more edge splats sums them in another order)
                        differ = int((got.view(np.uint32) != film.view(np.uint32)).sum())
                        worst = float(np.max(np.abs(got.astype(np.float64) - film) / np.maximum(np.abs(film), 1e-30)))
                run = dict(steps=len(ms), resident=resident, sum_ms=float(sum(ms)), ratio=float(sum(ms) / whole), first_step_ms=ms[0], other_steps_median_ms=float(np.median(ms[1:])) if len(ms) > 1 else None,
                           read_ms=reads, state_bytes=fr.state_bytes, film_words_differ=differ, film_worst_relative=worst)
            res["runs"].append(run)
            print(f"  {len(ms):3d} steps, tables {'resident' if resident else 'rebuilt '}: sum {run['sum_ms']:.1f} ms = {run['ratio']:.3f} x rt_render (first step {ms[0]:.1f} ms), "
                  f"read xyzw / rgb / rgb8 {reads['xyzw']:.2f} / {reads['rgb']:.2f} / {reads['rgb8']:.2f} ms, state {run['state_bytes'] / 2**20:.1f} MiB, film words that differ from rt_render's: {differ} of {film.size} (worst relative {worst:.2e})", flush=True)
            if first and resident:   # where the time goes: the stepped frame's stages beside rt_render's
                first = False
                with h.progressive(time_kernels=True, table_budget=budget) as fr:
                    tot = {k: 0.0 for k in STAGES}
                    while fr.samples_done < fr.spp:
                        st = fr.advance(n)
                        for k in STAGES:
                            tot[k] += st[k]
                res["stepped_stages"] = dict(steps=n_steps, **tot)
                print("  stage ms, stepped / rt_render: " + ", ".join(f"{k[3:]} {tot[k]:.1f} / {timed[k]:.1f}" for k in STAGES), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
