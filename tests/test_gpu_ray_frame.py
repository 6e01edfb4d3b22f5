"""Ray frames on the GPU (HostScene.progressive_rays -> RayFrame; rt_frame_begin_rays / rt_frame_advance_rays*): a progressive frame whose steps take their rays and
film positions from the caller, held bit for bit to entry points that exist - the camera's rays and positions give the camera's film, statistics, features and shards -
and, under a wide filter, to FilmTile::add_sample's arithmetic over rt_render_rays' radiance.
A film of 24 x 20 pixels, 16 spp, steps [3, 5, 8]: 480 pixels are no multiple of the 64-, 32- or 16-pixel tiles k_raygen_rays_film forms for 3, 5 and 8 samples (the
partial-tile paths run), and 20 rows are five 4-row shard bands - an uneven split over 2 ranks. Scenes (a), (b), (d) of tests/test_gpu_render_rays.py at this size: (a)
Cornell - LDS-resident, split shade kernels -, (b) room - binned queue, generic front-end -, (d) instance - k_trace_big; box filter of radius 0.5. Rays: sample_features()'
o and d with t_max = inf; positions: render_samples(with_p_film=True). Every measured figure is printed before it is asserted."""
import numpy as np
import pytest

from util import bits

pytestmark = pytest.mark.gpu

W, H = 24, 20
SPP = 16
STEPS = [3, 5, 8]
COUNTS = ("camera_rays", "rays_closest", "rays_shadow", "rays_mis", "rays_mis_any", "rays_mis_not_cast", "rays_tail_not_cast", "rays_shadow_not_cast", "paths_scrubbed",
          "vertices_lambert_const", "vertices_lambert", "vertices_two_lobe", "vertices_generic")


def _box(d):
    d.film.filter_kind, d.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)   # box filter, radius 0.5
    return d


def _cornell():
    from rustracer_amd.scenes import cornell_box
    return _box(cornell_box(W, H, SPP))


def _room():
    """(b) of tests/test_gpu_render_rays.py: floor = matte over a uv texture, back wall = mirror, left wall = plastic with vertex normals, right wall = matte, a glass
    pane, a matte sphere, a ceiling over the back half only, one area light."""
    from rustracer_amd.scene_desc import SceneDesc
    s = SceneDesc()
    m_uv = s.matte(s.uv_tex(su=0.8, sv=0.7, du=0.1, dv=0.15))
    m_mirror, m_plastic, m_glass = s.mirror((0.9, 0.8, 0.7)), s.plastic((0.3, 0.4, 0.2), (0.4, 0.4, 0.4), 0.2), s.glass()
    m_wall, m_sphere = s.matte((0.7, 0.6, 0.5)), s.matte((0.2, 0.5, 0.8))
    s.add_mesh([(-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2)], [[0, 1, 2], [0, 2, 3]], m_uv, UV=[(0, 0), (1, 0), (1, 1), (0, 1)])
    s.add_quad((-2, 0, 2), (2, 0, 2), (2, 3, 2), (-2, 3, 2), m_mirror)
    tilt = np.float32([(1, 0.2, 0.1), (1, -0.1, 0.2), (1, 0.15, -0.2), (1, -0.2, -0.1)])
    s.add_mesh([(-2, 0, -2), (-2, 0, 2), (-2, 3, 2), (-2, 3, -2)], [[0, 1, 2], [0, 2, 3]], m_plastic, N=tilt / np.linalg.norm(tilt, axis=1, keepdims=True))
    s.add_quad((2, 0, 2), (2, 0, -2), (2, 3, -2), (2, 3, 2), m_wall)
    s.add_quad((-2, 3, 0), (2, 3, 0), (2, 3, 2), (-2, 3, 2), m_wall)
    s.add_quad((0.3, 0, 0.5), (1.3, 0, 0.5), (1.3, 1.5, 0.5), (0.3, 1.5, 0.5), m_glass)
    s.add_sphere((-0.8, 0.6, 0.3), 0.6, m_sphere)
    s.add_quad((-0.5, 2.99, 0.5), (0.5, 2.99, 0.5), (0.5, 2.99, 1.5), (-0.5, 2.99, 1.5), s.matte((0, 0, 0)), emission=(12, 12, 12))
    s.camera.pos, s.camera.look, s.camera.fov = (0.2, 1.5, -3.5), (0.0, 1.3, 0.0), 60.0
    s.film.xres, s.film.yres = W, H
    s.sampler.spp = SPP
    return _box(s)


def _instanced():
    """(d) of tests/test_gpu_render_rays.py: a floor, a light and one rotated and translated instance of an object of four flat triangles."""
    from rustracer_amd.scene_desc import SceneDesc
    s = SceneDesc()
    floor, red = s.matte((0.6, 0.5, 0.4)), s.matte((0.7, 0.2, 0.2))
    s.add_quad((-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3), floor)
    P = np.float32([(0, 1, 0), (-0.6, 0, -0.6), (0.6, 0, -0.6), (0.6, 0, 0.6), (-0.6, 0, 0.6)])
    o = s.add_object([dict(P=P, idx=np.int32([(0, 2, 1), (0, 3, 2), (0, 4, 3), (0, 1, 4)]), material=red)])
    a = np.float64((1.0, 2.0, 0.5)) / np.linalg.norm((1.0, 2.0, 0.5))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K, (0.3, 0.4, 0.2)
    s.add_instance(o, m.astype(np.float32))
    s.add_quad((-1, 4, -1), (1, 4, -1), (1, 4, 1), (-1, 4, 1), s.matte((0, 0, 0)), emission=(10, 10, 10))
    s.camera.pos, s.camera.look, s.camera.fov = (0, 2.5, -5), (0.2, 0.6, 0), 40.0
    s.film.xres, s.film.yres = W, H
    s.sampler.spp = SPP
    return _box(s)


def _rays_of(feat):
    rays = np.zeros(feat.shape[:3] + (8,), np.float32)
    rays[..., 0:3], rays[..., 3], rays[..., 4:7] = feat[..., 0:3], np.inf, feat[..., 3:6]
    return rays


def _cut(a, s0, n):
    return np.ascontiguousarray(a[:, :, s0:s0 + n])


def _step_rays(frame, rays, pf, steps, s0=0):
    """The steps of a ray frame from sample s0 on: the stats of each."""
    out = []
    for n in steps:
        out.append(frame.advance(_cut(rays, s0, n), None if pf is None else _cut(pf, s0, n)))
        s0 += n
    return out


def _xyz32(rgb):
    """frame_resolve_store's RGB -> XYZ in float32, term by term, left to right."""
    r, g, b = (np.float32(rgb[..., k]) for k in range(3))
    f = np.float32
    return np.stack([f(0.412453) * r + f(0.357580) * g + f(0.180423) * b, f(0.212671) * r + f(0.715160) * g + f(0.072169) * b,
                     f(0.019334) * r + f(0.119193) * g + f(0.950227) * b], axis=-1)


def _lum32(rgb):
    """The luminance of the header comment, float32, left to right."""
    f = np.float32
    return f(0.212671) * np.float32(rgb[..., 0]) + f(0.715160) * np.float32(rgb[..., 1]) + f(0.072169) * np.float32(rgb[..., 2])


@pytest.fixture(scope="module")
def scenes(gpu_host):
    """name -> dict(h, rays, pf, rad, film, ray_rad): each scene uploaded once, its camera's rays, film positions and per-sample radiance, rt_render's film and
    rt_render_rays' radiance along those rays. Rendered once, left unchanged."""
    out = {}
    for name, d in (("a", _cornell()), ("b", _room()), ("d", _instanced())):
        h = gpu_host.HostScene(d)
        assert h.samples_window() == (0, 0, W, H)
        assert h.scene_query(gpu_host.RT_QUERY_NEEDS_DIFFERENTIALS) == 0, name   # the camera's frame regenerates no differentials at bounce 0, as a ray frame never does
        feat = h.sample_features()
        rad, pf, _ = h.render_samples(with_p_film=True)
        film, film_stats = h.render()
        rays = _rays_of(feat)
        ray_rad, _ = h.render_rays(rays)
        lit = float((rad[..., :3].max(-1) > 0).mean())
        on_edge = int((pf == np.floor(pf)).sum())
        print(f"\nRAYFRAME scene ({name}): lit samples {lit:.3f}; film positions exactly on a pixel edge {on_edge}; lds resident {h.lds_resident()}")
        assert lit > 0.05   # the comparisons are not of black with black
        assert rays.shape == (H, W, SPP, 8) and pf.shape == (H, W, SPP, 2) and np.array_equal(np.floor(pf[..., 0]), np.broadcast_to(np.arange(W, dtype=np.float32)[None, :, None], (H, W, SPP)))
        assert np.array_equal(bits(ray_rad), bits(rad))   # (tests/test_gpu_render_rays.py's statement, at this size)
        for a in (rays, pf, rad, film, ray_rad):
            a.setflags(write=False)
        out[name] = dict(h=h, rays=rays, pf=pf, rad=rad, film=film, film_stats=film_stats, ray_rad=ray_rad)
    return out


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_the_cameras_rays_and_positions_give_the_cameras_film(scenes, name):
    sc = scenes[name]
    h = sc["h"]
    with h.progressive() as cam:
        cam_stats = [cam.advance(n) for n in STEPS]
        cam_film, cam_rgb, cam_png = cam.film(), cam.rgb(), cam.display()
    with h.progressive_rays(W, H) as fr:
        assert fr.spp == SPP and fr.samples_done == 0 and not fr.film().any()
        stats = _step_rays(fr, sc["rays"], sc["pf"], STEPS)
        assert fr.samples_done == SPP
        film, rgb, png = fr.film(), fr.rgb(), fr.display()
        raw = fr.sums()
        taken = fr.samples_taken
        done_again = fr.advance(_cut(sc["rays"], 0, 1), _cut(sc["pf"], 0, 1))   # a finished frame: RT_OK, zeroed stats
    d_render = int((bits(film) != bits(sc["film"])).sum())
    d_cam = int((bits(film) != bits(cam_film)).sum())
    d_rgb, d_png = int((bits(rgb) != bits(cam_rgb)).sum()), int((png != cam_png).sum())
    rays_per_step = [s["camera_rays"] for s in stats]
    sums = {k: (sum(s[k] for s in stats), sum(s[k] for s in cam_stats)) for k in COUNTS}
    print(f"\nRAYFRAME 1 ({name}) steps {STEPS}: film words differing from render() {d_render}, from the camera frame {d_cam}; rgb words {d_rgb}; display bytes {d_png}; "
          f"camera_rays per step {rays_per_step}; samples_taken {taken}; counts (ray frame, camera frame) {sums}")
    assert film.shape == (H, W, 4) and np.abs(film[..., :3]).max() > 0 and png.any()
    assert d_render == 0 and d_cam == 0 and d_rgb == 0 and d_png == 0
    assert rays_per_step == [W * H * n for n in STEPS] and sum(rays_per_step) == W * H * SPP == taken
    assert all(a == b for a, b in sums.values())
    assert done_again["camera_rays"] == 0 and done_again["rays_closest"] == 0
    # RT_FRAME_SUMS: the sums the other read-outs start from - film() is them through frame_resolve_store's float32 XYZ matrix, the weight as it is
    d_raw = int((bits(np.concatenate([_xyz32(raw[..., :3]), raw[..., 3:4]], axis=-1)) != bits(film)).sum())
    print(f"RAYFRAME 1 ({name}) sums(): words of film() differing from the sums through the XYZ matrix {d_raw}; weights {np.unique(raw[..., 3])}")
    assert raw.shape == (H, W, 4) and raw.dtype == np.float32 and d_raw == 0 and np.all(raw[..., 3] == SPP)
    if name == "a":
        assert h.lds_resident() and sums["vertices_lambert_const"][0] > 0
    if name == "b":
        assert sums["vertices_generic"][0] > 0


# ---------------------------------------------------------------------------------------------- 2
def test_steps_do_not_matter(scenes):
    sc = scenes["a"]
    h = sc["h"]
    films = {}
    for steps in ([16], [3, 5, 8], [1] * 16):
        with h.progressive_rays(W, H) as fr:
            _step_rays(fr, sc["rays"], sc["pf"], steps)
            films[tuple(steps)] = (fr.film(), fr.rgb(), fr.display())
    ref = films[(16,)]
    diffs = {k: [int((bits(a) != bits(b)).sum()) for a, b in zip(v, ref)] for k, v in films.items()}
    with h.progressive_rays(W, H) as fr:
        _step_rays(fr, sc["rays"], sc["pf"], [3, 5])
        part = fr.film()
    with h.progressive_rays(W, H) as fr:
        _step_rays(fr, sc["rays"], sc["pf"], [8])
        fresh = fr.film()
    d_part = int((bits(part) != bits(fresh)).sum())
    print(f"\nRAYFRAME 2 (a): words differing from one step of 16, (film, rgb, display): { {str(k if len(k) < 4 else '1 x 16'): v for k, v in diffs.items()} }; "
          f"after [3, 5] against a fresh frame's [8]: {d_part}")
    assert all(v == [0, 0, 0] for v in diffs.values()) and d_part == 0
    assert part[..., 3].max() == 8.0 and np.abs(part[..., :3]).max() > 0


# ---------------------------------------------------------------------------------------------- 3
def test_wide_filter_against_arithmetic(scenes, gpu_host):
    """Gaussian, radius 2, alpha 2, positions = pixel centres + a seeded jitter in [-0.5, 0.5): the expected film in float64 from rt_render_rays' radiance for the same
    rays with FilmTile::add_sample's footprint and table index (film.rs:298-361), the index arithmetic in float32 in film_add_sample's order - so the indices are exact.
    Every term is non-negative and a pixel receives at most 16 * 5 * 5 = 400 taps: 400 * 2^-23 relative plus 1e-7 absolute (test_wide_filter of
    tests/test_gpu_progressive.py)."""
    from rustracer_amd.scene_desc import FILTER_GAUSSIAN
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(W, H, SPP)
    d.film.filter_kind, d.film.filter_params = FILTER_GAUSSIAN, (2.0, 2.0, 2.0, 0.0)
    h = gpu_host.HostScene(d)
    st = h.setup()
    table = st["filter_table"].astype(np.float32)
    assert np.isinf(st["params"].max_sample_luminance) or st["params"].max_sample_luminance > 1e30   # no clamp in the expectation below
    rays = scenes["a"]["rays"]
    rng = np.random.default_rng(31)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    centre = np.stack([xs + np.float32(0.5), ys + np.float32(0.5)], axis=-1)[:, :, None, :]
    pf = (centre + rng.uniform(-0.5, 0.5, (H, W, SPP, 2))).astype(np.float32)
    rad, _ = h.render_rays(rays)
    with h.progressive_rays(W, H) as fr:
        _step_rays(fr, rays, pf, STEPS)
        got = fr.film().astype(np.float64)
    L = np.where(rad[..., 3:4] == 1.0, np.float32(0), rad[..., :3]).astype(np.float64)   # a scrubbed sample splats black, with its weight
    assert L.min() >= 0
    f32, r, inv_r = np.float32, np.float32(2.0), np.float32(1.0) / np.float32(2.0)
    dx, dy = pf[..., 0] - f32(0.5), pf[..., 1] - f32(0.5)
    x0 = np.maximum(np.ceil(dx - r), f32(0)).astype(np.int64); y0 = np.maximum(np.ceil(dy - r), f32(0)).astype(np.int64)
    x1 = np.minimum(np.floor(dx + r + f32(1.0)), f32(W)).astype(np.int64); y1 = np.minimum(np.floor(dy + r + f32(1.0)), f32(H)).astype(np.int64)
    assert (x1 - x0).max() <= 5 and (y1 - y0).max() <= 5 and (x1 - x0).min() >= 1
    want = np.zeros((H, W, 4), np.float64)
    for j in range(5):
        for i in range(5):
            yy, xx = y0 + j, x0 + i
            m = (yy < y1) & (xx < x1)
            fy = np.abs((yy.astype(np.float32) - dy) * inv_r * f32(16.0)); fx = np.abs((xx.astype(np.float32) - dx) * inv_r * f32(16.0))
            iy = np.minimum(np.floor(fy), f32(15.0)).astype(np.int64); ix = np.minimum(np.floor(fx), f32(15.0)).astype(np.int64)
            fw = table[np.clip(iy * 16 + ix, 0, 255)].astype(np.float64)
            for c in range(3):
                np.add.at(want[..., c], (yy[m], xx[m]), L[..., c][m] * fw[m])
            np.add.at(want[..., 3], (yy[m], xx[m]), fw[m])
    c = np.float64
    want_xyz = np.stack([c(np.float32(0.412453)) * want[..., 0] + c(np.float32(0.357580)) * want[..., 1] + c(np.float32(0.180423)) * want[..., 2],
                         c(np.float32(0.212671)) * want[..., 0] + c(np.float32(0.715160)) * want[..., 1] + c(np.float32(0.072169)) * want[..., 2],
                         c(np.float32(0.019334)) * want[..., 0] + c(np.float32(0.119193)) * want[..., 1] + c(np.float32(0.950227)) * want[..., 2], want[..., 3]], axis=-1)
    n = 16 * 25
    err = np.abs(got - want_xyz)
    worst = float(np.max(err / np.maximum(np.abs(want_xyz), 1e-30)))
    over = int((err > 1e-7 + n * 2.0 ** -23 * np.abs(want_xyz)).sum())
    print(f"\nRAYFRAME 3 gaussian r = 2, jittered positions: worst relative difference to add_sample's arithmetic {worst:.3e} (bound {n * 2.0 ** -23:.3e} + 1e-7), {over} values over; "
          f"weight sums in [{want[..., 3].min():.3f}, {want[..., 3].max():.3f}]")
    assert want[..., 3].min() > 0 and np.abs(want[..., :3]).max() > 0
    assert over == 0, worst


# ---------------------------------------------------------------------------------------------- 4
def test_no_positions_are_pixel_centres(scenes):
    sc = scenes["b"]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    centres = np.ascontiguousarray(np.broadcast_to(np.stack([xs + np.float32(0.5), ys + np.float32(0.5)], axis=-1)[:, :, None, :], (H, W, SPP, 2)))
    with sc["h"].progressive_rays(W, H) as fr:
        _step_rays(fr, sc["rays"], None, STEPS)
        none_film = fr.film()
    with sc["h"].progressive_rays(W, H) as fr:
        _step_rays(fr, sc["rays"], centres, STEPS)
        centre_film = fr.film()
    diff = int((bits(none_film) != bits(centre_film)).sum())
    print(f"\nRAYFRAME 4 (b): p_film=None against explicit pixel centres: {diff} words differ; weights {np.unique(none_film[..., 3])}")
    assert diff == 0 and np.all(none_film[..., 3] == SPP) and np.abs(none_film[..., :3]).max() > 0


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name", ["a", "b"])
def test_skipped_rays(scenes, name):
    """A seeded third of the rays carry t_max 0, -1 or NaN, and every ray of a seeded set of pixels does. Positions are the pixel centres, so a pixel's film value is its
    own sum alone: the float32 sequential sum of its traced samples' radiance (rt_render_rays; a scrubbed sample adds zero) and their count, through
    frame_resolve_store's float32 XYZ matrix."""
    sc = scenes[name]
    rng = np.random.default_rng(77)
    skip = rng.random((H, W, SPP)) < 1.0 / 3.0
    dead = rng.random((H, W)) < 0.1
    skip |= dead[:, :, None]
    rays = sc["rays"].copy()
    rays[..., 3][skip] = rng.choice(np.float32([0.0, -1.0, np.nan]), int(skip.sum()))
    assert all((rays[..., 3] == np.float32(v)).any() for v in (0.0, -1.0)) and np.isnan(rays[..., 3]).any() and dead.any() and not dead.all()
    with sc["h"].progressive_rays(W, H) as fr:
        stats = _step_rays(fr, rays, None, STEPS)
        film = fr.film()
    own = np.zeros((H, W, 3), np.float32)
    wsum = np.zeros((H, W), np.float32)
    for s in range(SPP):   # sample-index order, float32
        keep = ~skip[:, :, s]
        Ls = np.where(sc["ray_rad"][:, :, s, 3:4] == 1.0, np.float32(0), sc["ray_rad"][:, :, s, :3])
        own = np.where(keep[..., None], own + Ls, own)
        wsum = np.where(keep, wsum + np.float32(1), wsum)
    want = np.concatenate([_xyz32(own), wsum[..., None]], axis=-1).astype(np.float32)
    diff = int((bits(film) != bits(want)).sum())
    traced = int((~skip).sum())
    rays_counted = sum(s["camera_rays"] for s in stats)
    print(f"\nRAYFRAME 5 ({name}): {int(skip.sum())} of {skip.size} rays skipped, {int(dead.sum())} pixels wholly; film words differing from the sequential sums {diff}; "
          f"weight of wholly skipped pixels {np.unique(film[dead][:, 3])}; camera_rays {rays_counted} traced {traced}")
    assert np.all(film[dead] == 0)   # weight 0, and nothing else either
    assert diff == 0 and rays_counted == traced
    assert np.abs(film[..., :3]).max() > 0


# ---------------------------------------------------------------------------------------------- 6
def test_statistics_and_adaptive_steps(scenes, gpu_host):
    sc = scenes["a"]
    h, rays, pf = sc["h"], sc["rays"], sc["pf"]
    with h.progressive_rays(W, H, pixel_stats=True) as fr:
        _step_rays(fr, rays, pf, [4])
        n, sy, sy2 = (a.copy() for a in fr.pixel_stats())
        # the plane of a sequential float64 loop over rt_render_rays' radiance
        y = _lum32(np.where(sc["ray_rad"][..., 3:4] == 1.0, np.float32(0), sc["ray_rad"][..., :3])).astype(np.float64)
        want_sy, want_sy2 = np.zeros((H, W)), np.zeros((H, W))
        for s in range(4):
            want_sy = want_sy + y[:, :, s]
            want_sy2 = want_sy2 + y[:, :, s] * y[:, :, s]
        bits64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
        d_n, d_sy, d_sy2 = int((n != 4).sum()), int((bits64(sy) != bits64(want_sy)).sum()), int((bits64(sy2) != bits64(want_sy2)).sum())
        floor_y, min_samples = float(np.float32(1e-3)), 4
        mean = sy / n
        se = np.sqrt(np.maximum(sy2 - sy * mean, 0.0) / (n - 1.0) / n)
        rel = se / np.maximum(mean, floor_y)
        thr = float(np.float32(np.median(rel)))
        want_active = (n < max(min_samples, 2)) | (se > thr * np.maximum(mean, floor_y))
        share = float(want_active.mean())
        print(f"\nRAYFRAME 6 (a) after [4]: pixels with n != 4: {d_n}; sum_y words differing {d_sy}, sum_y2 words differing {d_sy2}; relative standard errors: "
              f"min {rel.min():.4f} median {np.median(rel):.4f} max {rel.max():.4f}; threshold {thr:.6f}; active share by the formula {share:.3f}")
        assert d_n == 0 and d_sy == 0 and d_sy2 == 0 and sy.max() > 0
        assert 0.1 <= share <= 0.9
        before = fr.film()
        st = fr.advance_adaptive(_cut(rays, 4, 4), _cut(pf, 4, 4), thr, floor_y, min_samples)
        n2 = fr.pixel_stats()[0]
        after = fr.film()
        grew = n2 > n
        d_set = int((grew != want_active).sum())
        inactive_moved = int((bits(after)[~want_active] != bits(before)[~want_active]).sum())
        print(f"RAYFRAME 6 (a) adaptive step of 4: pixels whose n grew {int(grew.sum())}, the formula selects {int(want_active.sum())}, sets differ in {d_set}; "
              f"words of inactive pixels that moved {inactive_moved}; active_pixels {fr.active_pixels}; camera_rays {st['camera_rays']}; samples_taken {fr.samples_taken}; "
              f"samples_done {fr.samples_done}")
        assert d_set == 0 and np.all(n2[grew] == 8) and np.all(n2[~grew] == 4)
        assert inactive_moved == 0 and (bits(after)[want_active] != bits(before)[want_active]).any()
        assert fr.active_pixels == int(want_active.sum()) and st["camera_rays"] == 4 * int(want_active.sum())
        assert fr.samples_taken == W * H * 4 + st["camera_rays"] and fr.samples_done == 8
    with h.progressive_rays(W, H) as plain:   # the adaptive call needs the statistics plane
        with pytest.raises(gpu_host.BackendError):
            plain.advance_adaptive(_cut(rays, 0, 4), _cut(pf, 0, 4), 0.1)


# ---------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("name", ["a", "b"])
def test_features(scenes, name):
    sc = scenes[name]
    with sc["h"].progressive(features=True) as cam:
        for n in STEPS:
            cam.advance(n)
        want, want_film = cam.features(), cam.film()
    with sc["h"].progressive_rays(W, H, features=True) as fr:
        _step_rays(fr, sc["rays"], sc["pf"], STEPS)
        got, film = fr.features(), fr.film()
    diff, d_film = int((bits(got) != bits(want)).sum()), int((bits(film) != bits(want_film)).sum())
    print(f"\nRAYFRAME 7 ({name}): feature words differing from the camera frame's {diff}; film words {d_film}; mean coverage {float(got[..., 7].mean()):.3f}")
    assert got.shape == (H, W, 8) and got[..., 7].mean() > 0.3 and np.abs(got[..., 0:3]).max() > 0
    assert diff == 0 and d_film == 0


# ---------------------------------------------------------------------------------------------- 8
def test_shards(scenes):
    sc = scenes["b"]
    with sc["h"].progressive_rays(W, H) as fr:
        whole_stats = _step_rays(fr, sc["rays"], sc["pf"], STEPS)
        whole = fr.film()
    assert np.array_equal(bits(whole), bits(sc["film"]))
    owner = (np.arange(H) // 4) % 2   # bands of 4 rows: rows 0-3, 8-11, 16-19 are rank 0's, 4-7 and 12-15 rank 1's
    rays_seen = []
    for rank in (0, 1):
        rays = sc["rays"].copy()
        rays[owner != rank] = np.float32(-3.0)   # the other rank's rows: never read - records that would all be skipped, and turn the step onto the queued route, if they were
        with sc["h"].progressive_rays(W, H, rank=rank, world_size=2) as fr:
            stats = _step_rays(fr, rays, sc["pf"], STEPS)
            part = fr.film()
        mine = owner == rank
        d_own = int((bits(part[mine]) != bits(whole[mine])).sum())
        others_zero = bool(np.all(part[~mine] == 0))
        rays_seen.append(sum(s["camera_rays"] for s in stats))
        print(f"\nRAYFRAME 8 (b) rank {rank} of 2: {int(mine.sum())} rows; words of its rows differing from the whole frame's {d_own}; other rows all zero: {others_zero}; "
              f"camera_rays {rays_seen[-1]}")
        assert d_own == 0 and others_zero and rays_seen[-1] == int(mine.sum()) * W * SPP
    assert sum(rays_seen) == sum(s["camera_rays"] for s in whole_stats) == W * H * SPP and rays_seen[0] != rays_seen[1]


# ---------------------------------------------------------------------------------------------- 9
def test_device_pointers_give_the_host_pointer_result(scenes):
    import torch
    for name in ("a", "b"):
        sc = scenes[name]
        d_rays, d_pf = torch.from_numpy(sc["rays"].copy()).cuda(), torch.from_numpy(sc["pf"].copy()).cuda()
        with sc["h"].progressive_rays(W, H) as fr:
            s0, rays_seen = 0, 0
            for n in STEPS:
                st = fr.advance(d_rays[:, :, s0:s0 + n].contiguous(), d_pf[:, :, s0:s0 + n].contiguous())
                rays_seen += st["camera_rays"]
                s0 += n
            torch.cuda.synchronize()
            film = fr.film()
        with sc["h"].progressive_rays(W, H) as fr:   # ... and without positions
            fr.advance(d_rays, None)
            film_centres = fr.film()
        with sc["h"].progressive_rays(W, H) as fr:
            fr.advance(sc["rays"], None)
            host_centres = fr.film()
        diff, d_c = int((bits(film) != bits(sc["film"])).sum()), int((bits(film_centres) != bits(host_centres)).sum())
        print(f"\nRAYFRAME 9 ({name}) device tensors: film words differing from the host-pointer film {diff}; without positions {d_c}; camera_rays {rays_seen}")
        assert diff == 0 and d_c == 0 and rays_seen == W * H * SPP
        assert np.array_equal(bits(d_rays.cpu().numpy()), bits(sc["rays"])) and np.array_equal(bits(d_pf.cpu().numpy()), bits(sc["pf"]))   # read, never written


# ---------------------------------------------------------------------------------------------- 10
def test_kinds_do_not_mix_and_nothing_else_moves(scenes, gpu_host):
    sc = scenes["a"]
    h = sc["h"]
    film0, _ = h.render()
    rad0, _ = h.render_rays(sc["rays"])
    with h.progressive_rays(W, H, pixel_stats=True) as fr, h.progressive(pixel_stats=True) as cam:
        _step_rays(fr, sc["rays"], sc["pf"], [3])
        msgs = {}
        for what, call in (("advance() on a ray frame", lambda: gpu_host.ProgressiveFrame.advance(fr, 3)),
                           ("advance_adaptive() on a ray frame", lambda: gpu_host.ProgressiveFrame.advance_adaptive(fr, 3, 0.1)),
                           ("advance_rays on a camera frame", lambda: gpu_host.RayFrame.advance(cam, _cut(sc["rays"], 0, 3), _cut(sc["pf"], 0, 3))),
                           ("advance_rays_adaptive on a camera frame", lambda: gpu_host.RayFrame.advance_adaptive(cam, _cut(sc["rays"], 0, 3), None, 0.1)),
                           ("n_samples past spp", lambda: fr.advance(_cut(sc["rays"], 2, 14), _cut(sc["pf"], 2, 14)))):
            with pytest.raises(gpu_host.BackendError) as e:
                call()
            msgs[what] = str(e.value)
        print("\nRAYFRAME 10 refusals:", msgs)
        assert all("(-1)" in m and "rt_frame_advance" in m for m in msgs.values())
        assert fr.samples_done == 3 and cam.samples_done == 0   # a refused step moves nothing
        _step_rays(fr, sc["rays"], sc["pf"], [13], s0=3)
        film = fr.film()
    film1, _ = h.render()
    rad1, _ = h.render_rays(sc["rays"])
    print(f"RAYFRAME 10 nothing moves: render() words differing {int((bits(film0) != bits(film1)).sum())}, render_rays() words differing {int((bits(rad0) != bits(rad1)).sum())}")
    assert film.tobytes() == sc["film"].tobytes()
    assert film0.tobytes() == film1.tobytes() == sc["film"].tobytes() and rad0.tobytes() == rad1.tobytes() == sc["ray_rad"].tobytes()


# ---------------------------------------------------------------------------------------------- 11
@pytest.fixture(scope="module")
def pbrt_frames(gpu_host):
    """scripts/render_pbrt.py --camera-model orthographic --ray-frame --preview-every 2 (render_camera_model_frame) on the scene text of
    test_render_pbrt_camera_models_render_a_scene_file with a box filter and with a Gaussian one, and render_camera_model() for the same seed. Rendered once."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("render_pbrt", os.path.join(root, "scripts", "render_pbrt.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    NX, NY, NS, SEED = 16, 12, 4, 7

    def text(pixel_filter):
        return f"""LookAt 0 2 0  0 0 0  0 0 1
Camera "perspective" "float fov" [45]
Sampler "02sequence" "integer pixelsamples" [{NS}]
{pixel_filter}
Film "image" "integer xresolution" [{NX}] "integer yresolution" [{NY}]
Integrator "path" "integer maxdepth" [1]
WorldBegin
LightSource "point" "rgb I" [3 2.5 2] "point from" [0.3 1.5 -0.2]
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 0 -3  3 0 -3  3 0 3  -3 0 3]
WorldEnd
"""
    s = gpu_host.PbrtScene(text=text('PixelFilter "box" "float xwidth" [0.5] "float ywidth" [0.5]'))
    want, st = rp.render_camera_model(s, "orthographic", SEED)
    seen = []
    r = rp.render_camera_model_frame(s, "orthographic", SEED, preview_every=2, on_step=lambda frame: seen.append(frame.samples_done))
    g = gpu_host.PbrtScene(text=text('PixelFilter "gaussian" "float xwidth" [2] "float ywidth" [2]'))
    wide = rp.render_camera_model_frame(g, "orthographic", SEED, preview_every=2)
    return dict(shape=(NY, NX, NS), want=want, want_stats=st, box=r, seen=seen, wide=wide)


def test_render_pbrt_ray_frame_honours_steps_and_the_files_filter(pbrt_frames):
    """The plumbing of --ray-frame: steps of --preview-every samples, every ray counted once, RT_FRAME_RGB and RT_FRAME_RGB8 read-outs, and an image that moves with
    the file's PixelFilter (Gaussian of radius 2 against the box)."""
    NY, NX, NS = pbrt_frames["shape"]
    r, got, wide = pbrt_frames["box"], pbrt_frames["box"]["rgb"], pbrt_frames["wide"]["rgb"]
    moved = float(np.abs(wide.astype(np.float64) - got).max() / np.abs(got).max())
    print(f"\nRAYFRAME 11 render_pbrt --ray-frame: orthographic {NX}x{NY}x{NS} in steps {pbrt_frames['seen']}; camera_rays {r['stats']['camera_rays']} / "
          f"{pbrt_frames['want_stats']['camera_rays']}; gaussian against box: {moved:.3e} of the brightest value")
    assert got.shape == (NY, NX, 3) and got.dtype == np.float32 and pbrt_frames["seen"] == [2, 4] and r["samples_done"] == r["spp"] == NS
    assert r["stats"]["camera_rays"] == pbrt_frames["want_stats"]["camera_rays"] == NX * NY * NS and r["png8"].shape == (NY, NX, 3) and r["png8"].any()
    assert moved > 1e-3      # the file's filter is honoured


def test_render_pbrt_ray_frame_image_is_the_box_filtered_image(pbrt_frames):
    """The image of --ray-frame under the box filter against render_camera_model()'s for the same seed: a mean of 4 samples against a filtered sum divided by its
    weight, 4 * 2^-23 = 4.77e-7 relative per value. The script forms that image from the frame's own sums (RT_FRAME_SUMS, frame_rgb): three float32 additions and one
    division, 2.4e-7 at most. Through RT_FRAME_RGB - Film::write_image's pixel, the RGB sums through the float32 RGB -> XYZ matrix and back through XYZ -> RGB - the same
    image measured 6.55e-7 on an MI355X: the two matrices' six-digit coefficients are inverses of each other to about 1e-6, and in float32 numpy the round trip alone
    moves colours of this light's hue by up to 8.8e-7."""
    got, want = pbrt_frames["box"]["rgb"], pbrt_frames["want"]
    err = float((np.abs(got.astype(np.float64) - want) / np.abs(want)).max())
    print(f"\nRAYFRAME 11 render_pbrt --ray-frame: worst relative difference of a value to render_camera_model() {err:.3e} (bound {4 * 2.0 ** -23:.3e})")
    assert want.min() > 0
    assert err <= 4 * 2.0 ** -23
