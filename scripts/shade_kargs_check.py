#!/usr/bin/env python3
"""The shade front-ends that have no run-time knob (every kernel but a Cornell-box frame's three: RTX_SHADE_KARGS, tests/test_gpu_shade_kargs.py) compared across two
BUILDS: this tree's libraries and a second build with EXTRA=-DRT_SHADE_KARGS=0 (every shade kernel keeps its arguments live through the vertex) in a directory of
its own, rustracer_amd/csrc/_build_kargs0. Each build renders, in a child process of its own (RTX_LIB_DIR), one small box-filter frame of each workload - S1 to
S4, mis-spheres, instances-10k, 96 x 80 at 16 spp - and runs scripts/fuzz_shading.py 100 1; the parent prints the sha256 of each film's bits with the integer
stats and requires them equal, and both fuzz runs clean.

  python scripts/shade_kargs_check.py --build     (no GPU needed: compiles the second build, ~1 min)
  python scripts/shade_kargs_check.py             (GPU box, repo root; every GPU step under its own time limit, nothing started after one fails)"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rustracer_amd", "csrc")
BUILDS = {"kargs": os.path.join(CSRC, "_build"), "kargs0": os.path.join(CSRC, "_build_kargs0")}
WORKLOADS = ["cornell", "blob", "mis", "room", "mis-spheres", "instances-10k"]
RES, SPP = (96, 80), 16


def build_second():
    subprocess.run(["make", "-C", CSRC, "all", "OUT=_build_kargs0", "EXTRA=-DRT_SHADE_KARGS=0"], check=True)


def make_desc(name):
    from rustracer_amd.scenes import blob_scene, cornell_box, forest, mis_plates, room_env
    if name == "cornell":
        return cornell_box(RES[0], RES[1], SPP)
    if name == "blob":
        return blob_scene(xres=RES[0], yres=RES[1], spp=SPP)
    if name == "mis":
        return mis_plates(RES[0], RES[1], SPP)
    if name == "room":
        return room_env(RES[0], RES[1], SPP)
    if name == "mis-spheres":
        return mis_plates(RES[0], RES[1], SPP, analytic_spheres=True)
    return forest(100, 3, SPP, res=RES)


def child(name):
    """one frame of workload `name` with the libraries RTX_LIB_DIR names: a JSON line {sha256 of the film's bits, integer stats}"""
    sys.path.insert(0, ROOT)
    import numpy as np
    from rustracer_amd import host
    film, st = host.HostScene(make_desc(name)).render()
    ints = {n: int(st[n]) for n, t in host.Stats._fields_ if t is ctypes.c_uint64}
    print(json.dumps({"workload": name, "sha256": hashlib.sha256(np.ascontiguousarray(film, dtype=np.float32).tobytes()).hexdigest(), "stats": ints}))


def run(cmd, lib_dir, limit):
    env = dict(os.environ, RTX_LIB_DIR=lib_dir)
    return subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)


def main():
    for tag, d in BUILDS.items():
        if not os.path.exists(os.path.join(d, "librtx_hip.so")):
            sys.exit(f"{d}/librtx_hip.so missing: run `python scripts/shade_kargs_check.py --build` (and the product build) first")
    bad = 0
    for name in WORKLOADS:
        got = {}
        for tag, d in BUILDS.items():
            r = run([sys.executable, os.path.abspath(__file__), "--child", name], d, 240)
            if r.returncode != 0:  # a fault, an abort or a time limit: nothing more is started on this GPU
                sys.exit(f"{name} / {tag}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            got[tag] = json.loads(r.stdout.strip().splitlines()[-1])
        a, b = got["kargs"], got["kargs0"]
        same = a["sha256"] == b["sha256"] and a["stats"] == b["stats"]
        bad += 0 if same else 1
        diff = {k: (a["stats"][k], b["stats"][k]) for k in a["stats"] if a["stats"][k] != b["stats"].get(k)}
        print(f"{name:14s} {RES[0]}x{RES[1]} {SPP}spp  kargs {a['sha256'][:16]}  kargs0 {b['sha256'][:16]}  vertices {sum(v for k, v in a['stats'].items() if k.startswith('vertices_'))}"
              f"  {'EQUAL' if same else 'DIFFERENT ' + json.dumps(diff)}", flush=True)
    for tag, d in BUILDS.items():
        r = run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_shading.py"), "100", "1"], d, 420)
        last = (r.stdout.strip().splitlines() or ["(no output)"])[-1]
        print(f"fuzz_shading.py 100 1 / {tag}: exit {r.returncode}: {last}", flush=True)
        if r.returncode not in (0, 1):
            sys.exit(r.stderr[-2000:])
        bad += r.returncode
    print("all equal" if bad == 0 else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    if "--build" in sys.argv:
        build_second()
    elif "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 1])
    else:
        sys.exit(main())
