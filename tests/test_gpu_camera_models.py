"""Camera models generated on the device (rt_camera_model_rays / rt_frame_begin_model / rt_render_model; HostScene.camera_model_rays / progressive_model / render_model):
pbrt-v3's orthographic and environment cameras, held to the float64 model of tests/camera_model.py, to the perspective frame's camera sample, and - the frame - to the ray
frame of its own rays, byte for byte.
Shapes: a film of 16 x 12 (width != height shows an x / y or W / H swap), 4 spp, sampler dimensions 4, a camera-to-world that rotates about two axes and translates, the
screen window (-0.9, 1.1, -0.6, 0.7). The adaptive test alone opens its frames with 8 spp: an adaptive step decides from samples a plain step took before it.
The Gaussian pixel filter of the frame tests has radius 0.5 (alpha 2: weights from 0.39 at the pixel's centre to 0 at its edge, so every film position matters): each
tap then falls on the sample's own pixel, whose sum is one lane's loop in sample order, and "byte for byte" is a property of the code. Under a wider filter a sample
splats onto neighbouring pixels through float atomics whose order differs between any two launches - of the same frame as well (include/rtx_hip.h, rt_frame_advance_rays;
tests/test_gpu_progressive.py's wide-filter test) - so the radius-2 case holds the statistics and feature planes to bytes and the sums to that test's bound for the order
of the additions. Measured on an MI355X at radius 2, orthographic, steps [2, 2]: 22 to 25 of 3072 bytes of the sums differ from the ray frame's, 0 of the statistics and
feature planes - and the same ray frame run four times differs from its own first run in 11, 20 and 13 bytes.
Every measured figure is printed before it is asserted."""
import numpy as np
import pytest

import camera_model as cm
from util import bits

pytestmark = pytest.mark.gpu

NX, NY, NS = 16, 12, 4
WINDOW = (-0.9, 1.1, -0.6, 0.7)
POS, LOOK = (0.3, 1.7, -2.2), (0.1, 0.0, 0.2)
LENS, FOCAL = 0.05, 2.0
MODELS = ("orthographic", "environment")
KIND = dict(orthographic=cm.ORTHOGRAPHIC, environment=cm.ENVIRONMENT)
TOL = 4e-6   # ten float32 roundings of 6e-8 and the rounding of phi <= 2 pi, with a margin of 5 to 10


def _plain():
    """Nothing is traced on this scene (tests 1 to 3): a floor, a light, and a perspective camera at the origin looking down +z - camera-to-world is the identity - under a
    thin lens, whose camera_rays are the reference of the lens sample. Box filter of radius 0.5: the sample bounds are the film."""
    from rustracer_amd.scene_desc import SceneDesc
    s = SceneDesc()
    s.add_quad((-3, -1, -3), (3, -1, -3), (3, -1, 3), (-3, -1, 3), s.matte((0.5, 0.5, 0.5)))
    s.point_light((0.3, 1.5, -0.2), (3, 2.5, 2))
    s.camera.pos, s.camera.look, s.camera.up = (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)
    s.camera.lens_radius, s.camera.focal_distance = LENS, FOCAL
    s.film.xres, s.film.yres = NX, NY
    s.film.filter_kind, s.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)
    s.sampler.spp, s.sampler.dims = NS, 4
    return s


def _textured(pixel_filter="gauss"):
    """An image-mapped (trilinear) floor under a point light and a mirror pane: the floor's texture reads differentials, the mirror's first hit has another albedo and
    normal. A 64 x 64 random image repeated 8 times over a 6 x 6 floor: at half-pixel differentials of a 16 x 12 film the footprint spans several texels."""
    from rustracer_amd.scene_desc import SceneDesc
    rng = np.random.default_rng(23)
    s = SceneDesc()
    tri = s.image_tex(s.add_mip(rng.uniform(0.05, 0.95, (64, 64, 3)).astype(np.float32), trilinear=True), su=8.0, sv=8.0)
    s.add_mesh([(-3, 0, -3), (3, 0, -3), (3, 0, 3), (-3, 0, 3)], [[0, 1, 2], [0, 2, 3]], s.matte(tri), UV=[(0, 0), (1, 0), (1, 1), (0, 1)])
    s.add_quad((-0.2, 0.0, 0.9), (0.9, 0.0, 0.6), (0.9, 1.1, 0.6), (-0.2, 1.1, 0.9), s.mirror(0.9))
    s.point_light((0.3, 2.5, -0.4), (9, 8, 7))
    s.camera.pos, s.camera.look = POS, LOOK
    s.film.xres, s.film.yres = NX, NY
    s.film.filter_kind, s.film.filter_params = dict(gauss=(2, (0.5, 0.5, 2.0, 0.0)), wide=(2, (2.0, 2.0, 2.0, 0.0)), box=(0, (0.5, 0.5, 0.0, 0.0)))[pixel_filter]
    s.sampler.spp, s.sampler.dims = NS, 4
    s.integrator.max_depth = 3
    return s


def _cameras(host, lens=False):
    c2w = host.look_at(POS, LOOK, (0.0, 1.0, 0.0))[1]
    return dict(orthographic=host.camera_model("orthographic", c2w, NX, NY, screen_window=WINDOW, **(dict(lens_radius=LENS, focal_distance=FOCAL) if lens else {})),
                environment=host.camera_model("environment", c2w, NX, NY))


@pytest.fixture(scope="module")
def plain(gpu_host):
    h = gpu_host.HostScene(_plain())
    cams = _cameras(gpu_host)
    out = dict(h=h, cams=cams, persp=h.camera_rays(differentials=True))
    for m in MODELS:
        out[m] = h.camera_model_rays(m, cams[m], differentials=True)
    for pair in [out["persp"]] + [out[m] for m in MODELS]:
        for a in pair:
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def textured(gpu_host):
    """The scene of tests 4 to 7 uploaded once per pixel filter - Gaussian of radius 0.5, Gaussian of radius 2, box -, with each model's 20-float records and film
    positions of the four samples."""
    out = {}
    for name in ("gauss", "wide", "box"):
        h = gpu_host.HostScene(_textured(name))
        assert h.scene_query(gpu_host.RT_QUERY_NEEDS_DIFFERENTIALS) == 1
        cams = _cameras(gpu_host)
        out[name] = dict(h=h, cams=cams)
        for m in MODELS:
            rays, pf = h.camera_model_rays(m, cams[m], differentials=True)
            rays.setflags(write=False), pf.setflags(write=False)
            out[name][m] = (rays, pf)
    return out


def _cut(a, s0, n):
    return np.ascontiguousarray(a[:, :, s0:s0 + n])


def _err(got, want):
    """(worst |direction error|, worst origin error over (1 + max |component|)) of 20-float records against the float64 model's"""
    d_idx, o_idx = [4, 5, 6] + list(range(14, 20)), [0, 1, 2] + list(range(8, 14))
    e_d = float(np.abs(got[..., d_idx].astype(np.float64) - want[..., d_idx]).max())
    scale = 1.0 + np.abs(want[..., o_idx]).max()
    e_o = float(np.abs(got[..., o_idx].astype(np.float64) - want[..., o_idx]).max() / scale)
    return e_d, e_o


# ---------------------------------------------------------------------------------------------- 1
def test_film_positions_are_the_perspective_frames(plain):
    _, want = plain["persp"]
    for m in MODELS:
        rays, pf = plain[m]
        diff = int((bits(pf) != bits(want)).sum())
        print(f"\nCAMMODEL 1 ({m}): p_film words differing from camera_rays' {diff} of {pf.size}")
        assert pf.shape == (NY, NX, NS, 2) and pf.dtype == np.float32 and rays.shape == (NY, NX, NS, 20)
        assert diff == 0
    x, y = np.meshgrid(np.arange(NX), np.arange(NY))
    assert np.all(np.floor(want[..., 0]) == x[:, :, None]) and np.all(np.floor(want[..., 1]) == y[:, :, None])   # pixel + [0, 1): raster x to the right, y downwards


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("m", MODELS)
def test_rays_against_the_float64_model(plain, m):
    h, cam = plain["h"], plain["cams"][m]
    rays, pf = plain[m]
    want = cm.model_rays(KIND[m], cam, NX, NY, pf.astype(np.float64), NS)
    e_d, e_o = _err(rays, want)
    rays8, _ = h.camera_model_rays(m, cam)
    lo, lo_pf = h.camera_model_rays(m, cam, sample0=0, n_samples=1, differentials=True)
    hi, hi_pf = h.camera_model_rays(m, cam, sample0=1, differentials=True)
    d_8 = int((bits(rays8) != bits(np.ascontiguousarray(rays[..., :8]))).sum())
    d_cat = int((bits(np.concatenate([lo, hi], axis=2)) != bits(rays)).sum()) + int((bits(np.concatenate([lo_pf, hi_pf], axis=2)) != bits(pf)).sum())
    # what a wrong producer would give, against the same bound: W and H swapped, y mirrored, unscaled differentials
    swapped = _err(rays, cm.model_rays(KIND[m], cam, NY, NX, pf.astype(np.float64), NS))
    mirrored = _err(rays, cm.model_rays(KIND[m], cam, NX, NY, pf.astype(np.float64) * [1, -1] + [0, NY], NS))
    unscaled = _err(rays, cm.model_rays(KIND[m], cam, NX, NY, pf.astype(np.float64), 1))
    print(f"\nCAMMODEL 2 ({m}): direction error {e_d:.3e}, origin error / (1 + max |component|) {e_o:.3e} (bound {TOL:.1e}); 8-float form against the first 8 floats "
          f"{d_8}; [0, 1) + [1, 4) against the one call {d_cat}; a W / H swap would show {max(swapped):.3e}, a mirrored y {max(mirrored):.3e}, unscaled "
          f"differentials {max(unscaled):.3e}")
    assert np.all(np.isinf(rays[..., 3])) and np.all(rays[..., 3] > 0) and np.all(rays[..., 7] == 0)
    assert e_d <= TOL and e_o <= TOL
    assert d_8 == 0 and rays8.shape == (NY, NX, NS, 8) and d_cat == 0
    assert min(max(swapped), max(mirrored), max(unscaled)) > 100 * TOL   # the test has power


# ---------------------------------------------------------------------------------------------- 3
def test_orthographic_thin_lens(plain, gpu_host):
    h = plain["h"]
    cam = gpu_host.camera_model("orthographic", np.eye(4, dtype=np.float32), NX, NY, screen_window=WINDOW, lens_radius=LENS, focal_distance=FOCAL)
    rays, pf = h.camera_model_rays("orthographic", cam, differentials=True)
    persp, ppf = plain["persp"]
    o, d = rays[..., 0:3].astype(np.float64), rays[..., 4:7].astype(np.float64)
    r_max = float(np.hypot(o[..., 0], o[..., 1]).max())
    x0, x1, y0, y1 = (float(v) for v in np.float32(WINDOW))
    p = pf.astype(np.float64)
    focus = np.stack([x0 + p[..., 0] / NX * (x1 - x0), y1 - p[..., 1] / NY * (y1 - y0), np.full(p.shape[:-1], FOCAL)], axis=-1)
    t = (FOCAL - o[..., 2:3]) / d[..., 2:3]
    miss = float(np.abs(o + t * d - focus).max())
    # the same 2D#1 sample through concentric_sample_disk: the perspective camera's origins (identity camera-to-world; its origin nudge is of order gamma_3 * lens_radius)
    d_lens = float(np.abs(o - persp[..., 0:3].astype(np.float64)).max())
    want = cm.model_rays(cm.ORTHOGRAPHIC, cam, NX, NY, p, NS, lens_point=o[..., :2])
    e_d, e_o = _err(rays, want)
    spread = float(np.hypot(o[..., 0], o[..., 1]).std())
    print(f"\nCAMMODEL 3 orthographic lens {LENS} focus {FOCAL}: largest |origin.xy| {r_max:.6f}; rays miss their focus point by {miss:.3e} (bound {TOL * FOCAL:.1e}); origins "
          f"differ from the perspective camera's by {d_lens:.3e} (bound {TOL * LENS:.1e}); direction error {e_d:.3e}, origin error {e_o:.3e} against the float64 model; "
          f"std of |origin.xy| {spread:.4f}")
    assert pf.tobytes() == ppf.tobytes()
    assert np.all(rays[..., 2] == 0.0) and r_max <= LENS * (1 + 1e-6) and spread > 0.2 * LENS   # on the lens, and spread over it
    assert miss <= TOL * FOCAL
    assert d_lens <= TOL * LENS
    assert e_d <= TOL and e_o <= TOL
    assert np.array_equal(rays[..., 8:11], rays[..., 0:3]) and np.array_equal(rays[..., 11:14], rays[..., 0:3])   # rx_o = ry_o = the lens point


# ---------------------------------------------------------------------------------------------- 4
def _read(frame):
    return dict(sums=frame.sums(), stats=np.stack(frame.pixel_stats()), features=frame.features())


def _differing(a, b):
    return {k: int((np.ascontiguousarray(a[k]).view(np.uint8) != np.ascontiguousarray(b[k]).view(np.uint8)).sum()) for k in a}


def _model_and_ray_frames(sc, m, differentials, steps, **kw):
    h, cam = sc["h"], sc["cams"][m]
    rays, pf = sc[m]
    if not differentials:
        rays = np.ascontiguousarray(rays[..., :8])
    counts = []
    with h.progressive_model(m, cam, differentials=differentials, pixel_stats=True, features=True, **kw) as fr:
        st = [fr.advance(n) for n in steps]
        got = _read(fr)
        counts.append((sum(s["camera_rays"] for s in st), sum(s["paths_scrubbed"] for s in st), fr.samples_done, fr.samples_taken))
    with h.progressive_rays(NX, NY, pixel_stats=True, features=True, **kw) as fr:
        s0, st = 0, []
        for n in steps:
            st.append(fr.advance(_cut(rays, s0, n), _cut(pf, s0, n)))
            s0 += n
        want = _read(fr)
        counts.append((sum(s["camera_rays"] for s in st), sum(s["paths_scrubbed"] for s in st), fr.samples_done, fr.samples_taken))
    return got, want, counts


@pytest.mark.parametrize("m", MODELS)
def test_a_model_frame_is_the_ray_frame_of_its_own_rays(textured, m):
    sc = textured["gauss"]
    got, want, counts = _model_and_ray_frames(sc, m, True, [2, 2])
    diff = _differing(got, want)
    lit = float((got["sums"][..., :3].max(-1) > 0).mean())
    cover = got["features"][..., 7]
    print(f"\nCAMMODEL 4 ({m}) Gaussian filter, steps [2, 2], with differentials: bytes differing from the ray frame's {diff}; (camera_rays, paths_scrubbed, samples_done, "
          f"samples_taken) model {counts[0]} ray {counts[1]}; lit pixels {lit:.3f}; coverage min {cover.min():.2f} max {cover.max():.2f}")
    assert all(v == 0 for v in diff.values())
    assert counts[0] == counts[1] and counts[0][0] == NX * NY * NS and counts[0][2] == NS
    assert lit > 0.2 and cover.max() > 0.5 and np.abs(got["features"][..., 3:6]).max() > 0.5   # something is seen, and the planes hold it


@pytest.mark.parametrize("m", MODELS)
def test_a_model_frame_under_a_wide_filter(textured, m):
    """Gaussian, radius 2: the planes one lane owns are the ray frame's bytes; the sums are those of the same taps added in another order - all weights and radiances are
    non-negative, every partial sum is bounded by the result: n * 2^-23 relative with n = 4 * 5 * 5 taps at most per pixel, plus 1e-7 (tests/test_gpu_progressive.py)."""
    got, want, counts = _model_and_ray_frames(textured["wide"], m, True, [2, 2])
    diff = _differing(got, want)
    n = NS * 5 * 5
    a, b = got["sums"].astype(np.float64), want["sums"].astype(np.float64)
    worst = float((np.abs(a - b) / np.maximum(np.abs(b), 1e-30)).max())
    over = int((np.abs(a - b) > n * 2.0 ** -23 * np.abs(b) + 1e-7).sum())
    print(f"\nCAMMODEL 4 ({m}) Gaussian r = 2, steps [2, 2]: bytes differing from the ray frame's {diff}; worst relative difference of a sum {worst:.3e} (bound "
          f"{n * 2.0 ** -23:.3e} + 1e-7), {over} values over; counts {counts}")
    assert diff["stats"] == 0 and diff["features"] == 0 and counts[0] == counts[1]
    assert over == 0 and want["sums"][..., 3].min() > 0


def test_a_model_frame_without_differentials_on_a_scene_that_reads_them(textured):
    sc = textured["gauss"]
    got, want, counts = _model_and_ray_frames(sc, "orthographic", False, [2, 2])
    diff = _differing(got, want)
    with_diff, _, _ = _model_and_ray_frames(sc, "orthographic", True, [2, 2])
    moved = int((bits(with_diff["sums"]) != bits(got["sums"])).sum())
    print(f"\nCAMMODEL 4 (orthographic) without differentials: bytes differing from the ray frame of 8-float records {diff}; counts {counts}; sum words the differentials "
          f"move {moved} of {got['sums'].size}")
    assert all(v == 0 for v in diff.values()) and counts[0] == counts[1]
    assert moved > got["sums"].size // 10   # the option does something on this scene: zero-width lookups are other values


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("m", MODELS)
def test_adaptive_steps(textured, m):
    sc = textured["gauss"]
    h, cam = sc["h"], sc["cams"][m]
    rays, pf = h.camera_model_rays(m, cam, differentials=True, spp=8)
    floor_y, min_samples = 1e-3, 4
    with h.progressive_model(m, cam, spp=8, differentials=True, pixel_stats=True) as fr:
        fr.advance(4)
        mean, se = fr.noise()
        rel = se / np.maximum(mean, floor_y)
        thr = float(np.float32(np.median(rel[np.isfinite(rel) & (rel > 0)])))   # (half of the lit pixels: the environment camera's sky is black, its error 0)
        st = fr.advance_adaptive(4, thr, floor_y, min_samples)
        got = dict(sums=fr.sums(), n=fr.pixel_stats()[0], active=fr.active_pixels, taken=fr.samples_taken, done=fr.samples_done, rays=st["camera_rays"])
    with h.progressive_rays(NX, NY, spp=8, pixel_stats=True) as fr:
        fr.advance(_cut(rays, 0, 4), _cut(pf, 0, 4))
        st = fr.advance_adaptive(_cut(rays, 4, 4), _cut(pf, 4, 4), thr, floor_y, min_samples)
        want = dict(sums=fr.sums(), n=fr.pixel_stats()[0], active=fr.active_pixels, taken=fr.samples_taken, done=fr.samples_done, rays=st["camera_rays"])
    d_sums = int((bits(got["sums"]) != bits(want["sums"])).sum())
    print(f"\nCAMMODEL 5 ({m}) 8 spp, [4] then an adaptive 4 at threshold {thr:.5f}: active pixels model {got['active']} ray {want['active']} of {NX * NY}; samples taken "
          f"{got['taken']} / {want['taken']}; sum words differing {d_sums}")
    assert 0 < got["active"] < NX * NY
    assert got["active"] == want["active"] and got["taken"] == want["taken"] == NX * NY * 4 + 4 * got["active"] and got["done"] == want["done"] == 8
    assert got["rays"] == want["rays"] == 4 * got["active"] and np.array_equal(got["n"], want["n"])
    assert d_sums == 0


# ---------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("m", MODELS)
def test_shards_and_steps(textured, m):
    sc = textured["box"]
    h, cam = sc["h"], sc["cams"][m]
    films = {}
    for name, steps, kw in (("whole", [4], {}), ("stepped", [1, 3], {}), ("rank0", [4], dict(rank=0, world_size=2)), ("rank1", [1, 3], dict(rank=1, world_size=2))):
        with h.progressive_model(m, cam, differentials=True, **kw) as fr:
            rays = sum(fr.advance(n)["camera_rays"] for n in steps)
            films[name] = (fr.sums(), rays)
    whole = films["whole"][0]
    d_steps = int((bits(films["stepped"][0]) != bits(whole)).sum())
    owner = (np.arange(NY) // 4) % 2   # bands of 4 rows
    total = films["rank0"][0] + films["rank1"][0]
    d_sum = int((bits(total) != bits(whole)).sum())
    zero = bool(np.all(films["rank0"][0][owner == 1] == 0) and np.all(films["rank1"][0][owner == 0] == 0))
    print(f"\nCAMMODEL 6 ({m}) box filter: [1, 3] against [4]: words differing {d_steps}; rank 0 + rank 1 against the whole frame: {d_sum}; rows of the other rank zero: "
          f"{zero}; camera_rays {films['rank0'][1]} + {films['rank1'][1]} of {films['whole'][1]}")
    assert d_steps == 0 and d_sum == 0 and zero and whole[..., 3].min() > 0
    assert films["rank0"][1] == 8 * NX * NS and films["rank1"][1] == 4 * NX * NS and films["whole"][1] == NX * NY * NS
    # ... and the unsharded frame is the ray frame of the shard-independent rays
    got, want, _ = _model_and_ray_frames(sc, m, True, [4])
    assert got["sums"].tobytes() == want["sums"].tobytes() == whole.tobytes()


# ---------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("m", MODELS)
def test_one_call(textured, m):
    sc = textured["gauss"]
    h, cam = sc["h"], sc["cams"][m]
    film, st = h.render_model(m, cam, differentials=True)
    with h.progressive_model(m, cam, differentials=True) as fr:
        fr.advance(NS)
        want = fr.film()
    diff = int((bits(film) != bits(want)).sum())
    print(f"\nCAMMODEL 7 ({m}) render_model: film words differing from the finished model frame's {diff}; camera_rays {st['camera_rays']}")
    assert film.shape == (NY, NX, 4) and film.dtype == np.float32 and diff == 0 and st["camera_rays"] == NX * NY * NS and film[..., 3].min() > 0


# ---------------------------------------------------------------------------------------------- 8
def test_refusals(plain, gpu_host):
    h = plain["h"]
    good = gpu_host.camera_model("orthographic", np.eye(4, dtype=np.float32), NX, NY, screen_window=WINDOW, lens_radius=LENS, focal_distance=FOCAL)
    env = gpu_host.camera_model("environment", np.eye(4, dtype=np.float32), NX, NY)

    def edited(base, **kw):
        c = base.copy()
        for k, v in kw.items():
            c[int(k[1:])] = v
        return c

    cases = [("unknown model", 3, good, "model"), ("empty window", "orthographic", edited(good, _16=1.1), "screen_window"),
             ("window not finite", "orthographic", edited(good, _18=np.nan), "screen_window"), ("negative lens", "orthographic", edited(good, _20=-0.1), "lens_radius"),
             ("focal distance 0 under a lens", "orthographic", edited(good, _21=0.0), "focal_distance"), ("a lens on the environment camera", "environment", edited(env, _20=0.1), "lens_radius"),
             ("matrix not finite", "environment", edited(env, _7=np.inf), "camera_to_world"), ("reserved float", "orthographic", edited(good, _23=1.0), "reserved")]
    msgs = {}
    for name, kind, cam, word in cases:
        for what, call in (("camera_model_rays", lambda: h.camera_model_rays(kind, cam)), ("progressive_model", lambda: h.progressive_model(kind, cam)),
                           ("render_model", lambda: h.render_model(kind, cam))):
            with pytest.raises(gpu_host.BackendError) as e:
                call()
            msgs[(name, what)] = str(e.value)
            assert "(-1)" in str(e.value) and word in str(e.value), (name, what, str(e.value))
    print("\nCAMMODEL 8 refusals:", {k: v for k, v in msgs.items() if k[1] == "progressive_model"})
    rays, pf = plain["orthographic"]
    with h.progressive_model("orthographic", plain["cams"]["orthographic"], pixel_stats=True) as fr:
        for call in (lambda: gpu_host.RayFrame.advance(fr, _cut(rays, 0, 2), _cut(pf, 0, 2)),
                     lambda: gpu_host.RayFrame.advance_adaptive(fr, _cut(rays, 0, 2), _cut(pf, 0, 2), 0.1)):
            with pytest.raises(gpu_host.BackendError) as e:
                call()
            print("CAMMODEL 8 advance_rays on a model frame:", str(e.value))
            assert "(-1)" in str(e.value) and "rt_frame_begin_model" in str(e.value)
        assert fr.samples_done == 0 and fr.samples_taken == 0   # a refused step moves nothing
        assert fr.advance(NS)["camera_rays"] == NX * NY * NS


# ---------------------------------------------------------------------------------------------- 9
def test_render_pbrt_device_camera(gpu_host, tmp_path, monkeypatch, capsys):
    """scripts/render_pbrt.py --camera-model environment --device-camera --preview-every 2 on a small scene text, through main(): the previews arrive after 2 and 4
    samples, and the .pfm written last is progressive_model's image for the file's camera, sampler and filter."""
    import importlib.util
    import os
    import sys
    from rustracer_amd.ingest import read_pfm
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("render_pbrt", os.path.join(root, "scripts", "render_pbrt.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    text = f"""LookAt 0.3 1.7 -2.2  0.1 0 0.2  0 1 0
Camera "perspective" "float fov" [45]
Sampler "02sequence" "integer pixelsamples" [{NS}]
PixelFilter "gaussian" "float xwidth" [0.5] "float ywidth" [0.5]
Film "image" "integer xresolution" [{NX}] "integer yresolution" [{NY}]
Integrator "path" "integer maxdepth" [2]
WorldBegin
LightSource "point" "rgb I" [3 2.5 2] "point from" [0.3 1.5 -0.2]
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 0 -3  3 0 -3  3 0 3  -3 0 3]
WorldEnd
"""
    scene_file, out = tmp_path / "scene.pbrt", tmp_path / "out.pfm"
    scene_file.write_text(text)
    monkeypatch.setattr(sys, "argv", ["render_pbrt.py", str(scene_file), str(out), "--camera-model", "environment", "--device-camera", "--preview-every", "2"])
    rp.main()
    printed = capsys.readouterr().out
    previews = [ln for ln in printed.splitlines() if "samples per pixel" in ln]
    got = read_pfm(str(out))
    s = gpu_host.PbrtScene(text=text)
    with s.progressive_model("environment", s.camera_model_params("environment")) as fr:
        fr.advance(NS)
        want = rp.frame_rgb(fr)
    diff = int((bits(got) != bits(want)).sum())
    print(f"\nCAMMODEL 9 render_pbrt --device-camera: previews {previews}; image words differing from progressive_model's {diff}; brightest value {float(want.max()):.4f}")
    assert [f" {k} / {NS} samples per pixel" in ln for k, ln in zip((2, 4), previews)] == [True, True] and len(previews) == 2
    assert "environment camera through a model frame" in printed and f"{NX * NY * NS} rays" in printed
    assert got.shape == (NY, NX, 3) and diff == 0 and want.max() > 0
