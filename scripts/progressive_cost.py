"""What rendering a frame in steps costs (MEASUREMENTS "Progressive frames").

    python scripts/progressive_cost.py [--scene cornell|room|...] [--res N] [--spp N] [--steps 8,64] [--devices 0:0,0:0,0,0] [--out results/progressive_cost.json]

For the bench workload of the scene: rt_render's ms_total (median of --frames frames after a warm-up), then the frame stepped in each of --steps equal steps, with
resident sampler tables and with table_budget = 1 (every step rebuilds them): the sum of the steps' ms_total, its ratio to rt_render's, the first step's share, one
rt_frame_read of each kind, RT_FRAME_STATE_BYTES; and, for the first step count with resident tables, the per-stage HIP-event times (RT_FLAG_TIME_KERNELS) of the
stepped frame beside rt_render's. Every stepped film is compared with rt_render's bytes.
--devices: worker lists separated by ':' (0:0,0:0,0,0 = one, two and three workers on GPU 0). Per list, the frame across those workers (rt_multi_frame_*) in the first
step count of --steps with resident tables: the steps' wall time, the slowest worker's share of a step (median over the steps), one read of each kind (median of
--frames), the bytes the film rows of a read hold - touched_rows x cw x 16 per worker, of which the workers on other devices send theirs over the links -, the state
bytes, and the film against rt_render's. Beside the one-worker list stands the rt_frame with the same steps. Workers that share a GPU share its compute units: such a
list measures the cost of the mechanism, not scaling."""
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
    ap.add_argument("--devices", default=None)
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
    if a.devices:
        from rustracer_amd.distributed import touched_rows
        st = h.setup()
        cropped, sb = [int(v) for v in st["cropped"]], [int(v) for v in st["sample_bounds"]]
        cw = cropped[2] - cropped[0]
        ry = float(h.desc.film.filter_params[1])
        n_steps = int(a.steps.split(",")[0])
        budget = None if default_resident else 1 << 36
        res["multi"] = []

        def timed_reads(fr):
            reads = {}
            for name, call in (("xyzw", fr.film), ("rgb", fr.rgb), ("rgb8", fr.display)):
                call()
                ts = []
                for _ in range(a.frames):
                    t0 = time.perf_counter()
                    got = call()
                    ts.append((time.perf_counter() - t0) * 1e3)
                reads[name] = float(np.median(ts))
                if name == "xyzw":
                    reads["film"] = got
            return reads

        for devs in [[int(v) for v in part.split(",")] for part in a.devices.split(":")]:
            rows = [len(touched_rows(cropped, sb, k, len(devs), ry)) for k in range(len(devs))]
            with h.progressive_multi(devs, table_budget=budget) as fr:
                n = max(1, fr.spp // n_steps)
                wall, share = [], []
                while fr.samples_done < fr.spp:
                    t0 = time.perf_counter()
                    total, per = fr.advance(n)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    share.append(max(p["ms_total"] for p in per) / max(total["ms_total"], 1e-9))
                reads = timed_reads(fr)
                got = reads.pop("film")
                run = dict(devices=devs, steps=len(wall), sum_ms=float(sum(wall)), ratio=float(sum(wall) / whole), first_step_ms=wall[0],
                           other_steps_median_ms=float(np.median(wall[1:])) if len(wall) > 1 else None, slowest_worker_share=float(np.median(share)), read_ms=reads,
                           touched_rows=rows, read_bytes=[r * cw * 16 for r in rows], link_bytes=int(sum(r * cw * 16 for r, d in zip(rows, devs) if d != devs[0])),
                           state_bytes=fr.state_bytes, film_words_differ=int((got.view(np.uint32) != film.view(np.uint32)).sum()))
            if len(devs) == 1:   # the rt_frame with the same steps, timed the same way
                with h.progressive(table_budget=budget) as fr:
                    wall1 = []
                    while fr.samples_done < fr.spp:
                        t0 = time.perf_counter()
                        fr.advance(n)
                        wall1.append((time.perf_counter() - t0) * 1e3)
                    reads1 = timed_reads(fr)
                    reads1.pop("film")
                run["rt_frame"] = dict(sum_ms=float(sum(wall1)), other_steps_median_ms=float(np.median(wall1[1:])) if len(wall1) > 1 else None, read_ms=reads1)
            res["multi"].append(run)
            print(f"  workers {devs}: {run['steps']} steps sum {run['sum_ms']:.1f} ms = {run['ratio']:.3f} x rt_render (first {wall[0]:.1f}, others median {run['other_steps_median_ms']}), slowest worker's share "
                  f"{run['slowest_worker_share']:.3f}; read xyzw / rgb / rgb8 {reads['xyzw']:.2f} / {reads['rgb']:.2f} / {reads['rgb8']:.2f} ms; rows per worker {rows} = {run['read_bytes']} bytes, "
                  f"{run['link_bytes']} over links; state {run['state_bytes'] / 2**20:.1f} MiB; film words that differ from rt_render's: {run['film_words_differ']}", flush=True)
            if "rt_frame" in run:
                r1 = run["rt_frame"]
                print(f"    rt_frame, same steps: sum {r1['sum_ms']:.1f} ms (others median {r1['other_steps_median_ms']}), read xyzw / rgb / rgb8 "
                      f"{r1['read_ms']['xyzw']:.2f} / {r1['read_ms']['rgb']:.2f} / {r1['read_ms']['rgb8']:.2f} ms", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
