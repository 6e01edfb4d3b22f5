"""Render a pbrt-v3 scene file on the GPU.

    python scripts/render_pbrt.py scene.pbrt [out.png|out.pfm] [--spp N] [--samples out.npy] [--preview-every N]
                                  [--adaptive T [--min-samples M] [--noise-floor F] [--sample-map out.npy]] [--devices 0,1,...] [--features out.npy]
                                  [--camera-model orthographic|environment [--seed N] [--ray-frame] [--ray-differentials] [--device-camera]]
                                  [--ao N [--ao-distance D]] [--whitted [MAXDEPTH]] [--direct [MAXDEPTH] [--direct-strategy all|one]]

What `rustracer scene.pbrt` does, with the C++ host's parser (rtxh_pbrt_load) in front of the HIP path. Without an output
name the image goes where the reference writes it: "rt-" + the Film's filename, or image.png (rc/film.rs:118-123), as an
8-bit sRGB PNG with write_image_png's quantisation (rc/imageio.rs:52-74). A .pfm name gets the linear film values.
--samples out.npy: instead of an image, the radiance of every sample of the integrator's pixel bounds (rt_render_samples), float32
[height, width, spp, 6] = L rgb as PathIntegrator::li returned it, 1.0 where the renderer scrubs the sample, the sample's film position.
--preview-every N: the frame is rendered in steps of N samples per pixel (rt_frame_*) and the output image rewritten after each, as the reference's
-p / --display shows the image while it renders; the last image written is the one the run without the flag writes.
--adaptive T: the frame is rendered in steps of --preview-every samples (4 if not given) that only the pixels still noisier than T take (rt_frame_advance_adaptive:
the standard error of a pixel's mean luminance over max(mean, --noise-floor), every pixel at least --min-samples), until no pixel is active or the sampler's count is
reached; prints samples taken / samples of the full frame; --sample-map out.npy gets the per-pixel sample counts (float64 [height, width]). Such an image is no longer
the one the run without the flag writes.
--devices 0,1,...: with --preview-every or --adaptive, the frame lives on these GPUs of this process (rt_multi_frame_*; an index may repeat): every step runs on all
of them at once and the image written is the merged frame; prints the slowest worker's share of each step.
--features out.npy: beside the image, the guide images a denoiser takes (RT_FLAG_FRAME_FEATURES): float32 [height, width, 8] = per pixel the means over its own samples of
the first-hit albedo rgb and shading normal xyz, the mean depth of the samples that hit, and the coverage hits / samples - unfiltered. The frame is then rendered through
rt_frame_* (in one step unless --preview-every / --adaptive cut it; on --devices if given): the image is the one the run without the flag writes.
--camera-model orthographic|environment [--seed N]: the scene along the rays of a camera the reference does not have (rustracer_amd/cameras.py, pbrt-v3's definitions)
through rt_render_rays, in place of the file's perspective camera - whose camera-to-world and screen window it keeps -: film positions pixel + 0.5 + a seeded jitter of
the script's own, sample ranges of at most RT_RAYS_MAX rays, the radiance box-filtered (each pixel the mean of its own samples, scrubbed samples black). A choice of
this command line, not a file directive: the loader refuses Camera "orthographic" / "environment" as the reference does.
--ray-frame (with --camera-model): the same rays and film positions through a ray frame (rt_frame_begin_rays / rt_frame_advance_rays*) - filtered on the device with the
file's PixelFilter, clamp and film scale, no sample travels back. Honours --preview-every N (steps of N samples, the image rewritten after each), --adaptive T with
--min-samples / --noise-floor / --sample-map, and --features; the PNG is RT_FRAME_RGB8's bytes, a .pfm the frame's sums over their weights (RT_FRAME_SUMS). Without the flag --camera-model renders as before.
--ray-differentials (with --camera-model, with or without --ray-frame): the rays carry the camera model's differentials (records of 20 floats, RT_FLAG_RAY_DIFFERENTIALS;
pbrt-v3's GenerateRayDifferential of each camera, scaled by 1 / sqrt(spp)), so image maps, checkerboards, fbm and bump maps are filtered at the first hit as under the
file's perspective camera. Opt-in: without it the rays have none and textures are looked up at zero width, as before.
--device-camera (with --camera-model): the camera's rays are generated on the device (rt_frame_begin_model) from the file's ZeroTwoSequence tables - film positions
pixel + the sampler's 2D#0 instead of the script's seeded jitter (--seed is unused), the orthographic camera's "lensradius" / "focaldistance" as a thin lens from 2D#1 -
and rendered through a model frame: nothing per sample crosses the host bus. Filtered as under --ray-frame (the file's PixelFilter, clamp and film scale; the PNG is
RT_FRAME_RGB8's bytes, a .pfm the frame's sums over their weights); honours --preview-every, --adaptive with its options, --features and --ray-differentials.
--ao N [--ao-distance D]: the file's camera, film, filter and sampler with the reference's ambient-occlusion integrator (rt_render_ao; integrator/ao.rs) in place of the
file's Integrator: every camera sample's value is the clear fraction of N occlusion rays over the hemisphere of the first hit's geometric normal, rays of length D
(default: infinite, the reference). A choice of this command line: the loader's Integrator handling is unchanged (it refuses "ambientocclusion" as it refuses
"whitted"). One call, one device: --preview-every, --adaptive, --features, --samples, --devices and --camera-model do not combine with it.
--whitted [MAXDEPTH]: the same with the reference's Whitted integrator (rt_render_whitted; integrator/whitted.rs): every light sampled at every vertex, mirrors and glass
followed recursively up to MAXDEPTH (default 5, the reference's "maxdepth" default; the camera ray is depth 0). Also a choice of this command line - the loader keeps
refusing Integrator "whitted" - and also one call on one device: it combines with none of the options --ao excludes, nor with --ao.
--direct [MAXDEPTH] [--direct-strategy all|one]: the same with the reference's direct-lighting integrator (rt_render_direct; integrator/directlighting.rs): every light
("all", the default: from the sampler's stratified arrays) or one uniformly picked light ("one") sampled at every vertex with multiple importance sampling - soft shadows
from area and environment lights, no global illumination -, mirrors and glass followed up to MAXDEPTH (default 5). The loader keeps refusing Integrator
"directlighting"; one call on one device, with the exclusions of --whitted, and not with --whitted or --ao."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def camera_model_samples(s, model, seed=0, differentials=False):
    """The generator behind --camera-model: (w, h, spp, chunks) where `chunks` yields (s0, p_film [h, w, ns, 2] float64, rays [h, w, ns, 8] float32) for sample ranges
    [s0, s0 + ns) of at most RT_RAYS_MAX rays that together are [0, spp). The camera takes the file's camera-to-world and, orthographic, its "screenwindow" (pbrt's
    default from the aspect ratio without one); film positions are pixel + 0.5 + a jitter in [-0.5, 0.5) from numpy's default_rng(seed), drawn range after range.
    `differentials`: records of 20 floats with the camera model's differentials, scaled for `spp`."""
    import numpy as np
    from rustracer_amd import cameras, host
    p = s._render_params()
    w, h = int(p.xres), int(p.yres)
    spp = 1
    while spp < max(int(p.spp), 1):
        spp *= 2
    if w * h > host.RT_RAYS_MAX:
        raise SystemExit(f"--camera-model: a film of {w} x {h} pixels holds more than RT_RAYS_MAX rays per sample")
    c2w = np.float32(list(p.cam_to_world)).reshape(4, 4)
    win = tuple(float(v) for v in p.screen_window)
    if win == (0.0, 0.0, 0.0, 0.0):
        aspect = w / h
        win = (-aspect, aspect, -1.0, 1.0) if aspect > 1.0 else (-1.0, 1.0, -1.0 / aspect, 1.0 / aspect)

    def chunks():
        rng = np.random.default_rng(seed)
        step = max(1, min(spp, host.RT_RAYS_MAX // (w * h)))
        for s0 in range(0, spp, step):
            ns = min(step, spp - s0)
            p_film = cameras.pixel_centres(w, h, ns) + rng.uniform(-0.5, 0.5, (h, w, ns, 2))
            kw = dict(differentials=True, spp=spp) if differentials else {}
            rays = cameras.orthographic(c2w, win, w, h, p_film, **kw) if model == "orthographic" else cameras.environment(c2w, w, h, p_film, **kw)
            yield s0, p_film, rays

    return w, h, spp, chunks()


def render_camera_model(s, model, seed=0, differentials=False):
    """The scene through `HostScene.render_rays` with a camera of rustracer_amd/cameras.py in place of the file's: returns (rgb [yres, xres, 3] float32 - the box-filtered
    radiance, each pixel the mean of its own samples, scrubbed samples black as in the renderer -, stats summed over the calls). The camera takes the file's
    camera-to-world and, orthographic, its "screenwindow" (pbrt's default from the aspect ratio without one); film positions are pixel + 0.5 + a jitter in [-0.5, 0.5)
    from numpy's default_rng(seed); the samples go through in sample ranges of at most RT_RAYS_MAX rays. `differentials`: --ray-differentials."""
    import numpy as np
    w, h, spp, chunks = camera_model_samples(s, model, seed, differentials)
    total = np.zeros((h, w, 3), np.float64)
    stats = dict(ms_total=0.0, camera_rays=0, paths_scrubbed=0)
    for s0, _, rays in chunks:
        rad, st = s.render_rays(rays, sample0=s0, spp=spp)
        ok = rad[..., 3:4] == 0.0
        total += np.where(ok, rad[..., :3], 0.0).sum(axis=2, dtype=np.float64)
        for k in stats:
            stats[k] += st[k]
    return (total / spp * float(s._render_params().film_scale)).astype(np.float32), stats


def frame_rgb(frame):
    """The linear image of a frame from its own sums (RT_FRAME_SUMS): per pixel (sum of w * L) / (sum of w) in the radiance's RGB where the weight is not zero, max(0, .),
    times the film scale - Film::write_image's pixel without the detour through XYZ that RT_FRAME_RGB takes (two float32 matrices, inverse to each other within 1e-6): the
    box-filtered image is then the mean of a pixel's samples to float32 rounding, which is what `render_camera_model` returns."""
    import numpy as np
    a = frame.sums()
    w = a[..., 3:4]
    q = np.where(w != 0, np.maximum(a[..., :3] / np.where(w != 0, w, np.float32(1)), np.float32(0)), a[..., :3])
    return (q * np.float32(frame.scale)).astype(np.float32)


def render_camera_model_frame(s, model, seed=0, preview_every=0, adaptive=None, noise_floor=1e-3, min_samples=8, features=False, on_step=None, differentials=False):
    """--camera-model --ray-frame: the same rays and film positions as `render_camera_model` draws for `seed`, through a ray frame (`HostScene.progressive_rays`) - the
    film stage on the device, with the file's PixelFilter, max_sample_luminance and film scale instead of the numpy box filter. Steps of `preview_every` samples (0: a
    whole sample range each; 4 under `adaptive`); `on_step(frame)` is called after each. `adaptive` = T: the steps are `advance_adaptive(.., T, noise_floor,
    min_samples)` and end when no pixel is active. Returns dict(rgb [yres, xres, 3] float32 - `frame_rgb` -, png8 [yres, xres, 3] uint8 - RT_FRAME_RGB8 -, stats,
    samples_done, samples_taken, spp, counts - the per-pixel sample counts, adaptive only -, features - [yres, xres, 8] where asked for). `differentials`:
    --ray-differentials."""
    import numpy as np
    w, h, spp, chunks = camera_model_samples(s, model, seed, differentials)
    stats = dict(ms_total=0.0, camera_rays=0, paths_scrubbed=0)
    with s.progressive_rays(w, h, spp=spp, pixel_stats=adaptive is not None, features=features) as frame:
        stopped = False
        for s0, p_film, rays in chunks:
            ns = rays.shape[2]
            step = preview_every if preview_every > 0 else (4 if adaptive is not None else ns)
            for a in range(0, ns, step):
                r, pf = np.ascontiguousarray(rays[:, :, a:a + step]), np.ascontiguousarray(p_film[:, :, a:a + step], np.float32)
                st = frame.advance(r, pf) if adaptive is None else frame.advance_adaptive(r, pf, adaptive, noise_floor, min_samples)
                for k in stats:
                    stats[k] += st[k]
                if adaptive is not None and frame.active_pixels == 0:
                    stopped = True
                    break
                if on_step is not None:
                    on_step(frame)
            if stopped:
                break
        return dict(rgb=frame_rgb(frame), png8=frame.display(), stats=stats, samples_done=frame.samples_done, samples_taken=frame.samples_taken, spp=spp,
                    counts=frame.pixel_stats()[0] if adaptive is not None else None, features=frame.features() if features else None)


def render_device_camera_frame(s, model, preview_every=0, adaptive=None, noise_floor=1e-3, min_samples=8, features=False, on_step=None, differentials=False):
    """--camera-model --device-camera: the scene through a model frame (`HostScene.progressive_model`) whose camera is filled from the file's render parameters
    (`HostScene.camera_model_params`). Steps of `preview_every` samples (0: the whole frame; 4 under `adaptive`); `on_step(frame)` after each. Returns what
    `render_camera_model_frame` returns."""
    stats = dict(ms_total=0.0, camera_rays=0, paths_scrubbed=0)
    with s.progressive_model(model, s.camera_model_params(model), differentials=differentials, pixel_stats=adaptive is not None, features=features) as frame:
        spp = frame.spp
        step = preview_every if preview_every > 0 else (4 if adaptive is not None else spp)
        while frame.samples_done < spp:
            st = frame.advance(step) if adaptive is None else frame.advance_adaptive(step, adaptive, noise_floor, min_samples)
            for k in stats:
                stats[k] += st[k]
            if adaptive is not None and frame.active_pixels == 0:
                break
            if on_step is not None:
                on_step(frame)
        return dict(rgb=frame_rgb(frame), png8=frame.display(), stats=stats, samples_done=frame.samples_done, samples_taken=frame.samples_taken, spp=spp,
                    counts=frame.pixel_stats()[0] if adaptive is not None else None, features=frame.features() if features else None)


def main():
    from rustracer_amd import host
    from rustracer_amd.ingest import write_pfm, write_png
    ap = argparse.ArgumentParser()
    ap.add_argument("--camera-model", choices=["orthographic", "environment"], default=None,
                    help="render along the rays of this camera (rt_render_rays) instead of the file's perspective camera; box-filtered")
    ap.add_argument("--seed", type=int, default=0, help="with --camera-model: seed of the film-position jitter")
    ap.add_argument("--ray-frame", action="store_true",
                    help="with --camera-model: filter the samples on the device through a ray frame (rt_frame_advance_rays) with the file's PixelFilter, in steps")
    ap.add_argument("--ray-differentials", action="store_true",
                    help="with --camera-model: the rays carry the camera model's differentials (RT_FLAG_RAY_DIFFERENTIALS), so textures are filtered at the first hit")
    ap.add_argument("--device-camera", action="store_true",
                    help="with --camera-model: generate the camera's rays on the device from the file's sampler (rt_frame_begin_model) and render through a model frame")
    ap.add_argument("scene")
    ap.add_argument("out", nargs="?")
    ap.add_argument("--spp", type=int, default=0, help="override Sampler pixelsamples")
    ap.add_argument("--samples", metavar="OUT.npy", default=None, help="write the per-sample radiance and film positions of the pixel bounds instead of an image")
    ap.add_argument("--preview-every", type=int, default=0, metavar="N", help="rewrite the output image after every N samples per pixel")
    ap.add_argument("--adaptive", type=float, default=None, metavar="T", help="stop sampling a pixel once the relative standard error of its luminance is at most T")
    ap.add_argument("--min-samples", type=int, default=8, metavar="M", help="with --adaptive: samples every pixel takes before it may stop")
    ap.add_argument("--noise-floor", type=float, default=1e-3, metavar="F", help="with --adaptive: the error is relative to max(mean luminance, F)")
    ap.add_argument("--sample-map", metavar="OUT.npy", default=None, help="with --adaptive: write the per-pixel sample counts")
    ap.add_argument("--features", metavar="OUT.npy", default=None, help="write the per-pixel first-hit feature planes (albedo, normal, depth, coverage) beside the image")
    ap.add_argument("--devices", default=None, metavar="0,1,...", help="with --preview-every / --adaptive: render the frame on these GPUs of this process")
    ap.add_argument("--ao", type=int, default=0, metavar="N", help="render with the ambient-occlusion integrator: N occlusion rays per camera sample")
    ap.add_argument("--ao-distance", type=float, default=float("inf"), metavar="D", help="with --ao: the length of the occlusion rays (default: infinite)")
    ap.add_argument("--whitted", type=int, nargs="?", const=5, default=None, metavar="MAXDEPTH", help="render with the Whitted integrator, recursion limit MAXDEPTH (default 5)")
    ap.add_argument("--direct", type=int, nargs="?", const=5, default=None, metavar="MAXDEPTH", help="render with the direct-lighting integrator, recursion limit MAXDEPTH (default 5)")
    ap.add_argument("--direct-strategy", choices=("all", "one"), default=None, help="with --direct: sample every light at every vertex (all, the default) or one picked light (one)")
    a = ap.parse_args()
    if a.direct is not None and a.direct < 1:
        raise SystemExit("--direct MAXDEPTH must be >= 1 (the camera ray is depth 0)")
    if a.direct_strategy and a.direct is None:
        raise SystemExit("--direct-strategy needs --direct")
    if a.direct and (a.ao or a.whitted):
        raise SystemExit("--direct, --whitted and --ao each replace the file's Integrator: give one of them")
    if a.direct and (a.samples or a.preview_every > 0 or a.adaptive is not None or a.features or a.devices or a.camera_model):
        raise SystemExit("--direct renders the file's camera in one call: it does not combine with --samples, --preview-every, --adaptive, --features, --devices or --camera-model")
    if a.whitted is not None and a.whitted < 1:
        raise SystemExit("--whitted MAXDEPTH must be >= 1 (the camera ray is depth 0)")
    if a.whitted and a.ao:
        raise SystemExit("--whitted and --ao each replace the file's Integrator: give one of them")
    if a.whitted and (a.samples or a.preview_every > 0 or a.adaptive is not None or a.features or a.devices or a.camera_model):
        raise SystemExit("--whitted renders the file's camera in one call: it does not combine with --samples, --preview-every, --adaptive, --features, --devices or --camera-model")
    if a.ao and (a.samples or a.preview_every > 0 or a.adaptive is not None or a.features or a.devices or a.camera_model):
        raise SystemExit("--ao renders the file's camera in one call: it does not combine with --samples, --preview-every, --adaptive, --features, --devices or --camera-model")
    if a.ao_distance != float("inf") and not a.ao:
        raise SystemExit("--ao-distance goes with --ao")
    host.build()
    s = host.PbrtScene(a.scene)
    if a.spp:
        s.params.spp = a.spp
    if a.samples:
        import numpy as np
        rad, pf, stats = s.render_samples()
        np.save(a.samples, np.concatenate([rad, pf], axis=-1))
        x0, y0, x1, y1 = s.samples_window()
        print(f"{a.samples}: pixels [{x0}, {x1}) x [{y0}, {y1}), {rad.shape[2]} samples each, {int(rad[..., 3].sum())} scrubbed, {stats['ms_total']:.1f} ms, {s.n_warnings} parser warnings")
        return
    out = a.out or s.film_filename
    if not out.endswith((".pfm", ".png")):
        raise SystemExit("Unsupported file format")   # rc/imageio.rs:47-49 (EXR output is not written here)
    if a.ray_frame and not a.camera_model:
        raise SystemExit("--ray-frame goes with --camera-model")
    if a.ray_differentials and not a.camera_model:
        raise SystemExit("--ray-differentials goes with --camera-model")
    if a.device_camera and not a.camera_model:
        raise SystemExit("--device-camera goes with --camera-model")
    if a.camera_model and (a.ray_frame or a.device_camera):
        import numpy as np
        if a.devices:
            raise SystemExit("--ray-frame and --device-camera render on one device")

        def put(rgb, png8):
            if out.endswith(".pfm"):
                write_pfm(out, rgb)
            else:
                write_png(out, png8, 2, 8, filters=(1,))

        def preview(frame):
            put(frame_rgb(frame), frame.display())
            print(f"{out}: {frame.samples_done} / {frame.spp} samples per pixel" + (f", {frame.active_pixels} pixels active" if a.adaptive is not None else ""), flush=True)

        kw = dict(preview_every=a.preview_every, adaptive=a.adaptive, noise_floor=a.noise_floor, min_samples=a.min_samples, features=bool(a.features),
                  on_step=preview if a.preview_every > 0 else None, differentials=a.ray_differentials)
        r = render_device_camera_frame(s, a.camera_model, **kw) if a.device_camera else render_camera_model_frame(s, a.camera_model, a.seed, **kw)
        put(r["rgb"], r["png8"])
        if a.adaptive is not None:
            full = int(np.count_nonzero(r["counts"])) * r["spp"]
            print(f"{out}: {r['samples_taken']} samples taken / {full} of the full frame ({r['samples_taken'] / max(full, 1):.3f}), stopped after {r['samples_done']} of {r['spp']} indices")
            if a.sample_map:
                np.save(a.sample_map, r["counts"])
        if a.features:
            np.save(a.features, r["features"])
            print(f"{a.features}: {r['features'].shape[1]}x{r['features'].shape[0]} x (albedo rgb, normal xyz, depth, coverage), mean coverage {float(r['features'][..., 7].mean()):.3f}")
        stats = r["stats"]
        print(f"{out}: {r['rgb'].shape[1]}x{r['rgb'].shape[0]}, {a.camera_model} camera through a {'model' if a.device_camera else 'ray'} frame, {stats['camera_rays']} rays, {stats['paths_scrubbed']} scrubbed, {stats['ms_total']:.1f} ms, {s.n_warnings} parser warnings")
        return
    if a.camera_model:
        rgb, stats = render_camera_model(s, a.camera_model, a.seed, differentials=a.ray_differentials)
        if out.endswith(".pfm"):
            write_pfm(out, rgb)
        else:
            write_png(out, host.rgb_to_png8(rgb), 2, 8, filters=(1,))
        print(f"{out}: {rgb.shape[1]}x{rgb.shape[0]}, {a.camera_model} camera, {stats['camera_rays']} rays, {stats['paths_scrubbed']} scrubbed, {stats['ms_total']:.1f} ms, {s.n_warnings} parser warnings")
        return

    def write(film):
        rgb = host.film_to_rgb(film, s.params.film_scale)
        if out.endswith(".pfm"):
            write_pfm(out, rgb)
        else:
            write_png(out, host.rgb_to_png8(rgb), 2, 8, filters=(1,))

    devices = [int(v) for v in a.devices.split(",")] if a.devices else None
    if devices and a.adaptive is None and a.preview_every <= 0 and not a.features:
        raise SystemExit("--devices goes with --preview-every, --adaptive or --features")

    def begin(**kw):
        if a.features:
            kw["features"] = True
        return s.progressive_multi(devices, **kw) if devices else s.progressive(**kw)

    def step_ms(st):
        """ms_total of a step; a multi frame's step is (total, [per worker]): its slowest worker is printed beside the call's wall time."""
        if not devices:
            return st["ms_total"]
        total, per = st
        worst = max(p["ms_total"] for p in per)
        print(f"  step {total['ms_total']:.1f} ms on {len(per)} workers; slowest worker {worst:.1f} ms = {worst / max(total['ms_total'], 1e-9):.3f} of it", flush=True)
        return total["ms_total"]

    def save_features(frame):
        if a.features:
            import numpy as np
            f = frame.features()
            np.save(a.features, f)
            print(f"{a.features}: {f.shape[1]}x{f.shape[0]} x (albedo rgb, normal xyz, depth, coverage), mean coverage {float(f[..., 7].mean()):.3f}")

    if a.adaptive is not None:
        import numpy as np
        stats = {"ms_total": 0.0}
        step = a.preview_every if a.preview_every > 0 else 4
        with begin(pixel_stats=True) as frame:
            spp = frame.spp
            while frame.samples_done < spp:
                stats["ms_total"] += step_ms(frame.advance_adaptive(step, a.adaptive, a.noise_floor, a.min_samples))
                if frame.active_pixels == 0:
                    break
                if a.preview_every > 0:
                    write(frame.film())
                    print(f"{out}: {frame.samples_done} / {spp} sample indices offered, {frame.active_pixels} pixels active", flush=True)
            film = frame.film()
            write(film)
            counts = frame.pixel_stats()[0]
            full = int(np.count_nonzero(counts)) * spp
            print(f"{out}: {frame.samples_taken} samples taken / {full} of the full frame ({frame.samples_taken / max(full, 1):.3f}), stopped after {frame.samples_done} of {spp} indices")
            if a.sample_map:
                np.save(a.sample_map, counts)
            save_features(frame)
    elif a.preview_every > 0 or a.features:
        stats = {"ms_total": 0.0}
        with begin() as frame:
            spp = frame.spp
            while frame.samples_done < spp:
                stats["ms_total"] += step_ms(frame.advance(a.preview_every if a.preview_every > 0 else spp))
                film = frame.film()
                write(film)
                print(f"{out}: {frame.samples_done} / {spp} samples per pixel", flush=True)
            save_features(frame)
    elif a.direct:
        film, stats = s.render_direct(a.direct, a.direct_strategy or "all")
        write(film)
        print(f"{out}: direct lighting, strategy {a.direct_strategy or 'all'}, max depth {a.direct}, {stats['rays_closest']} li rays, {stats['rays_shadow']} visibility segments and "
              f"{stats['rays_mis']} BSDF-sampled rays from {stats['camera_rays']} camera samples")
    elif a.whitted:
        film, stats = s.render_whitted(a.whitted)
        write(film)
        print(f"{out}: Whitted, max depth {a.whitted}, {stats['rays_closest']} li rays and {stats['rays_shadow']} visibility segments from {stats['camera_rays']} camera samples")
    elif a.ao:
        film, stats = s.render_ao(a.ao, a.ao_distance)
        write(film)
        print(f"{out}: ambient occlusion, {a.ao} occlusion rays per sample, {stats['rays_shadow']} cast from {stats['camera_rays']} camera samples")
    else:
        film, stats = s.render()
        write(film)
    print(f"{out}: {film.shape[1]}x{film.shape[0]}, {s.params.spp} spp, {stats['ms_total']:.1f} ms, {s.n_warnings} parser warnings")


if __name__ == "__main__":
    main()
