"""Direct irradiance of a pbrt-v3 scene's lights at arbitrary points (a light probe, a lightmap bake): no surface, no BSDF, no path.

    python scripts/irradiance_probe.py scene.pbrt points.npy out.npy [--blocks B] [--grid G] [--seed N]

points.npy: (P, 6) = position xyz and unit normal xyz per point, world space. out.npy: (P, 6) float64 = E rgb and its standard error. Every light of the file's
light list is sampled per point through rt_light_eval (HostScene.direct_irradiance): the shade kernels' own Light::sample_li, the segment to the sample traced by
the scene's any-hit kernels, Li max(0, n . wi) / pdf. A point or distant light takes one query per point; an area or environment light --blocks (64)
independent jittered --grid x --grid (8 x 8) sets of samples, and the standard error is that of the block means."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import numpy as np
    from rustracer_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("points")
    ap.add_argument("out")
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    pts = np.load(a.points)
    if pts.ndim != 2 or pts.shape[1] != 6:
        raise SystemExit(f"{a.points}: expected an array of shape (P, 6) = position and normal, got {pts.shape}")
    host.build()
    s = host.PbrtScene(a.scene)
    e, se = s.direct_irradiance(pts[:, 0:3], pts[:, 3:6], blocks=a.blocks, grid=a.grid, seed=a.seed)
    np.save(a.out, np.concatenate([e, se], axis=1))
    print(f"{pts.shape[0]} points, {s.n_lights()} lights: mean E {e.mean(axis=0)}, largest standard error {se.max():.3e}")


if __name__ == "__main__":
    main()
