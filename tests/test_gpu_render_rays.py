"""rt_render_rays on the GPU (HostScene.render_rays): PathIntegrator::li along caller-supplied rays, held to the frame of rt_render_samples bit for bit - the camera
rays rt_render_sample_features reports, fed back in, give the radiance rt_render_samples reports - and, for rays no perspective camera can make, to arithmetic.
32 x 32 x 16 scenes with a box filter of radius 0.5 (sample bounds = pixel bounds: the virtual film is the film): (a) the Cornell box - Lambert-only, LDS-resident,
k_shade_split with both fresh records -, (b) a room of matte-over-uv, mirror, plastic, glass and a sphere - the binned queue -, (d) one instance over a floor -
k_trace_big -, (b) again under a thin lens. None of them reads ray differentials (asserted: RT_QUERY_NEEDS_DIFFERENTIALS), so the camera's frame and the ray frame
shade alike. Every measured figure is printed before it is asserted."""
import numpy as np
import pytest

from util import bits

pytestmark = pytest.mark.gpu

W = H = 32
SPP = 16
COUNTS = ("camera_rays", "rays_closest", "rays_shadow", "rays_mis", "rays_mis_any", "rays_mis_not_cast", "rays_tail_not_cast", "rays_shadow_not_cast", "paths_scrubbed",
          "vertices_lambert_const", "vertices_lambert", "vertices_two_lobe", "vertices_generic")


def _box(d):
    d.film.filter_kind, d.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)   # box filter, radius 0.5
    return d


def _cornell():
    from rustracer_amd.scenes import cornell_box
    return _box(cornell_box(W, H, SPP))


def _room(lens_radius=0.0):
    """(b) of tests/test_gpu_features.py: floor = matte over a uv texture, back wall = mirror, left wall = plastic with vertex normals, right wall = matte, a glass pane,
    a matte sphere, a ceiling over the back half only, one area light."""
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
    if lens_radius > 0:
        s.camera.lens_radius, s.camera.focal_distance = lens_radius, 3.5
    s.film.xres, s.film.yres = W, H
    s.sampler.spp = SPP
    return _box(s)


def _instanced():
    """(d) of tests/test_gpu_features.py: a floor, a light and one rotated and translated instance of an object of four flat triangles."""
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


def _rays_of(feat, t_max=np.inf):
    rays = np.zeros(feat.shape[:3] + (8,), np.float32)
    rays[..., 0:3], rays[..., 3], rays[..., 4:7] = feat[..., 0:3], t_max, feat[..., 3:6]
    return rays


@pytest.fixture(scope="module")
def scenes(gpu_host):
    """name -> dict(h, feat, rays, rad, stats, ray_rad, ray_stats): each scene uploaded once, its camera's rays and per-sample radiance (the reference of every test
    here), and the ray frame over those rays. Rendered once, left unchanged."""
    out = {}
    for name, d in (("a", _cornell()), ("b", _room()), ("d", _instanced()), ("b_lens", _room(lens_radius=0.08))):
        h = gpu_host.HostScene(d)
        assert h.samples_window() == (0, 0, W, H)
        # no texture of these scenes reads differentials: the camera's frame regenerates none at bounce 0, as the ray frame never does
        assert h.scene_query(gpu_host.RT_QUERY_NEEDS_DIFFERENTIALS) == 0, name
        feat = h.sample_features()
        rad, _, stats = h.render_samples(with_p_film=False)
        rays = _rays_of(feat)
        ray_rad, ray_stats = h.render_rays(rays)
        for a in (feat, rad, rays, ray_rad):
            a.setflags(write=False)
        out[name] = dict(h=h, feat=feat, rays=rays, rad=rad, stats=stats, ray_rad=ray_rad, ray_stats=ray_stats)
    return out


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["a", "b", "d", "b_lens"])
def test_the_cameras_rays_give_the_cameras_radiance_bit_for_bit(scenes, gpu_host, name):
    sc = scenes[name]
    assert sc["ray_rad"].shape == (H, W, SPP, 4) and sc["rad"].shape == (H, W, SPP, 4)
    diff = int((bits(sc["ray_rad"]) != bits(sc["rad"])).sum())
    counts = {k: (sc["ray_stats"][k], sc["stats"][k]) for k in COUNTS}
    lit = float((sc["rad"][..., :3].max(-1) > 0).mean())
    print(f"\nRAYS ({name}) {W * H * SPP} rays: differing radiance words {diff}; lit samples {lit:.3f}; lds resident {sc['h'].lds_resident()}; counts (rays, samples) {counts}")
    assert lit > 0.05   # the comparison is not of black with black
    if name == "a":
        assert sc["h"].lds_resident() and sc["stats"]["vertices_lambert_const"] > 0
    if name in ("b", "b_lens"):
        assert sc["stats"]["vertices_generic"] > 0 and sc["stats"]["vertices_two_lobe"] + sc["stats"]["vertices_lambert"] > 0
    assert diff == 0
    assert all(a == b for a, b in counts.values()) and sc["ray_stats"]["camera_rays"] == W * H * SPP
    assert np.all(sc["ray_rad"][..., 3] == sc["rad"][..., 3]) and set(np.unique(sc["ray_rad"][..., 3])) <= {0.0, 1.0}
    if name == "b_lens":   # the lens moved the rays: this is not (b) again
        assert int((bits(sc["rays"]) != bits(scenes["b"]["rays"])).sum()) > W * H * SPP


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["a", "b"])
def test_skipped_rays_read_two_and_leave_the_others_alone(scenes, name):
    sc = scenes[name]
    rng = np.random.default_rng(2024)
    skip = rng.random((H, W, SPP)) < 0.5
    rays = sc["rays"].copy()
    rays[..., 3][skip] = rng.choice(np.float32([0.0, -1.0, np.nan]), int(skip.sum()))
    for v in (0.0, -1.0):
        assert (rays[..., 3] == np.float32(v)).any()
    assert np.isnan(rays[..., 3]).any()
    rad, st = sc["h"].render_rays(rays)
    kept_diff = int((bits(rad[~skip]) != bits(sc["ray_rad"][~skip])).sum())
    skipped_ok = bool(np.all(bits(rad[skip]) == bits(np.float32([0, 0, 0, 2.0]))))
    print(f"\nRAYS skip ({name}) kept {int((~skip).sum())} skipped {int(skip.sum())}: differing words among kept {kept_diff}; skipped read (0, 0, 0, 2): {skipped_ok}; camera_rays {st['camera_rays']}")
    assert kept_diff == 0 and skipped_ok
    assert st["camera_rays"] == int((~skip).sum())


# ---------------------------------------------------------------------------------------------- 3
def test_sample_ranges_concatenate_to_the_one_call(scenes):
    for name in ("a", "b"):
        sc = scenes[name]
        lo, _ = sc["h"].render_rays(sc["rays"][:, :, :8], sample0=0)
        hi, _ = sc["h"].render_rays(sc["rays"][:, :, 8:], sample0=8)
        diff = int((bits(np.concatenate([lo, hi], axis=2)) != bits(sc["ray_rad"])).sum())
        print(f"\nRAYS ranges ({name}) [0, 8) + [8, 16): differing words {diff}")
        assert diff == 0
    sc = scenes["a"]
    ones = np.concatenate([sc["h"].render_rays(sc["rays"][:, :, s:s + 1], sample0=s)[0] for s in range(SPP)], axis=2)
    diff = int((bits(ones) != bits(sc["ray_rad"])).sum())
    print(f"RAYS ranges (a) 16 calls of one sample: differing words {diff}")
    assert diff == 0
    # ranges that are no power of two, over a pixel window that is no multiple of a tile (k_raygen_rays: 64 pixels x 4 samples for 3, 16 x 16 for 13): rows 3 .. 31 of
    # (b) are pixels 96 .. 1023 of the film, so the window's own keys differ from the film's - it is compared with itself, cut two ways
    sc = scenes["b"]
    sub = np.ascontiguousarray(sc["rays"][3:, :29])
    whole, _ = sc["h"].render_rays(sub)
    parts = np.concatenate([sc["h"].render_rays(sub[:, :, :3], sample0=0)[0], sc["h"].render_rays(sub[:, :, 3:], sample0=3)[0]], axis=2)
    diff = int((bits(parts) != bits(whole)).sum())
    print(f"RAYS ranges (b) 29 x 29 pixels, [0, 3) + [3, 16): differing words {diff}; lit {float((whole[..., :3].max(-1) > 0).mean()):.3f}")
    assert diff == 0 and (whole[..., :3].max(-1) > 0).mean() > 0.05


# ---------------------------------------------------------------------------------------------- 4
def test_t_max_is_honoured(scenes):
    sc = scenes["a"]
    depth = sc["feat"][..., 9]
    hit = np.ascontiguousarray(sc["feat"][..., 6]).view(np.int32) >= 0
    assert hit.mean() > 0.5 and np.all(depth[hit] > 0) and float(np.abs(sc["ray_rad"][..., :3][hit]).max()) > 0
    # half the first-hit depth where the camera ray hits; a camera ray that leaves the box past its rim (depth 0) keeps t_max = inf - it misses anyway, and a t_max of
    # 0 would skip it instead of tracing it
    rad, st = sc["h"].render_rays(_rays_of(sc["feat"], t_max=np.where(hit, depth * np.float32(0.5), np.float32(np.inf))))
    print(f"\nRAYS t_max (a): max radiance {float(np.abs(rad[..., :3]).max())}, flags {np.unique(rad[..., 3])}, camera_rays {st['camera_rays']} rays_closest {st['rays_closest']} rays_shadow {st['rays_shadow']}")
    assert np.all(rad == 0)   # a miss on a scene without an infinite light: black, and a normal sample
    assert st["camera_rays"] == W * H * SPP and st["rays_closest"] == W * H * SPP and st["rays_shadow"] == 0 and st["rays_mis"] == 0


# ---------------------------------------------------------------------------------------------- 5
def test_orthographic_rays_over_a_textured_plane_against_arithmetic(gpu_host):
    """A matte plane y = 0 whose Kd is an image map of 16 x 16 seeded random texels, one point light above it, max_depth 1; 16 x 16 pixels x 4 samples of an orthographic
    camera looking straight down. Expected per ray, in float64: Kd(uv) / pi * Li * cos(theta), Kd(uv) from HostScene.texture_eval at the hit's uv with all-zero
    differentials and Li the reference's PointLight::sample_li, I / (4 pi r^2) (light/point.rs:43-54: its point light divides the intensity by 4 pi, and this backend
    computes what the reference computes; pbrt's own I / r^2 is 4 pi = 12.57 times that and is off by exactly that factor on every ray). Bound 1e-4 relative per ray: a dozen float32 operations, a few of them 1-ulp reciprocals and square roots - a few 1e-6; a lookup at another MIP level
    or with a camera's differentials moves a texel by O(1)."""
    from rustracer_amd import cameras
    from rustracer_amd.scene_desc import SceneDesc
    N, NS = 16, 4
    rng = np.random.default_rng(5)
    s = SceneDesc()
    tex = s.image_tex(s.add_mip(rng.uniform(0.2, 0.9, (16, 16, 3)).astype(np.float32)))
    s.add_mesh([(-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1)], [[0, 1, 2], [0, 2, 3]], s.matte(tex), UV=[(0, 0), (1, 0), (1, 1), (0, 1)])
    light, I = np.float64([0.3, 1.5, -0.2]), np.float64([3.0, 2.5, 2.0])
    s.point_light(tuple(light), tuple(I))
    s.film.xres, s.film.yres = N, N
    s.sampler.spp = NS
    s.integrator.max_depth = 1
    h = gpu_host.HostScene(_box(s))
    assert h.scene_query(gpu_host.RT_QUERY_NEEDS_DIFFERENTIALS) == 1   # an image map: a camera's frame would hand the lookup the camera ray's differentials
    _, c2w = gpu_host.look_at((0.0, 2.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    pf = cameras.pixel_centres(N, N, NS) + rng.uniform(-0.5, 0.5, (N, N, NS, 2))
    rays = cameras.orthographic(c2w, (-0.9, 0.9, -0.9, 0.9), N, N, pf)
    assert np.abs(rays[..., 4:7] - np.float32([0, -1, 0])).max() < 1e-6 and np.all(rays[..., 1] == 2.0)
    rad, st = h.render_rays(rays)
    p = rays[..., 0:3].reshape(-1, 3).astype(np.float64) * (1, 0, 1)   # straight down onto y = 0
    uv = np.stack([(p[:, 0] + 1) / 2, (p[:, 2] + 1) / 2], axis=1)
    kd = h.texture_eval(tex, uv.astype(np.float32)).astype(np.float64)
    r2 = ((light - p) ** 2).sum(1)
    want = kd / np.pi * (I / (4 * np.pi * r2[:, None])) * (light[1] / np.sqrt(r2))[:, None]
    got = rad[..., :3].reshape(-1, 3).astype(np.float64)
    err = float((np.abs(got - want) / want).max())
    print(f"\nRAYS ortho: {len(p)} rays, texels spread {float(kd.std()):.3f}, worst relative error {err:.3e} (bound 1e-4), camera_rays {st['camera_rays']} rays_shadow {st['rays_shadow']}")
    assert kd.std() > 0.1 and np.all(rad[..., 3] == 0) and st["camera_rays"] == N * N * NS
    assert err <= 1e-4


# ---------------------------------------------------------------------------------------------- 6
def test_device_pointers_give_the_host_pointer_result(scenes):
    import torch
    for name in ("a", "b"):
        sc = scenes[name]
        d_rays = torch.from_numpy(sc["rays"].copy()).cuda()
        d_out = torch.full((H, W, SPP, 4), -7.0, dtype=torch.float32, device="cuda")
        out, st = sc["h"].render_rays(d_rays, device_out=d_out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        diff = int((bits(got) != bits(sc["ray_rad"])).sum())
        print(f"\nRAYS device ({name}): differing words {diff}, camera_rays {st['camera_rays']}")
        assert out is d_out and diff == 0 and st["camera_rays"] == W * H * SPP
        assert np.array_equal(bits(d_rays.cpu().numpy()), bits(sc["rays"]))   # the rays are read, never written


# ---------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("name", ["a", "b"])
def test_nothing_else_moves(scenes, name):
    sc = scenes[name]
    h = sc["h"]
    film0, _ = h.render()
    rad, _ = h.render_rays(sc["rays"])
    film1, _ = h.render()
    again, _, _ = h.render_samples(with_p_film=False)
    print(f"\nRAYS nothing moves ({name}): film words differing {int((bits(film0) != bits(film1)).sum())}, render_samples words differing {int((bits(again) != bits(sc['rad'])).sum())}")
    assert film0.tobytes() == film1.tobytes() and np.abs(film0[..., :3]).max() > 0
    assert again.tobytes() == sc["rad"].tobytes() and rad.tobytes() == sc["ray_rad"].tobytes()


# ---------------------------------------------------------------------------------------------- 8
def test_render_pbrt_camera_models_render_a_scene_file(gpu_host):
    """scripts/render_pbrt.py --camera-model: a scene file through render_rays in place of its perspective camera. Orthographic, straight down onto a grey matte plane
    under a point light: every pixel is the mean over its samples of Kd / pi * I / (4 pi r^2) * cos(theta) (the reference's point light, as above) at the film positions the script's seeded generator draws - 1e-4
    relative, the bound of the test above (constant Kd: fewer operations). Environment: a lat-long image whose lower half sees the plane and whose upper half is black."""
    import importlib.util
    import os
    from rustracer_amd import cameras
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("render_pbrt", os.path.join(root, "scripts", "render_pbrt.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    NX, NY, NS, SEED = 16, 12, 4, 7
    text = f"""LookAt 0 2 0  0 0 0  0 0 1
Camera "perspective" "float fov" [45]
Sampler "02sequence" "integer pixelsamples" [{NS}]
Film "image" "integer xresolution" [{NX}] "integer yresolution" [{NY}]
Integrator "path" "integer maxdepth" [1]
WorldBegin
LightSource "point" "rgb I" [3 2.5 2] "point from" [0.3 1.5 -0.2]
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 0 -3  3 0 -3  3 0 3  -3 0 3]
WorldEnd
"""
    s = gpu_host.PbrtScene(text=text)
    rgb, st = rp.render_camera_model(s, "orthographic", SEED)
    assert rgb.shape == (NY, NX, 3) and rgb.dtype == np.float32 and st["camera_rays"] == NX * NY * NS and st["paths_scrubbed"] == 0
    pf = cameras.pixel_centres(NX, NY, NS) + np.random.default_rng(SEED).uniform(-0.5, 0.5, (NY, NX, NS, 2))
    c2w = np.float32(list(s.params.cam_to_world)).reshape(4, 4)
    rays = cameras.orthographic(c2w, (-NX / NY, NX / NY, -1.0, 1.0), NX, NY, pf)   # pbrt's default screen window of a wide film
    assert np.abs(rays[..., 4:7] - np.float32([0, -1, 0])).max() < 1e-6
    p = rays[..., 0:3].astype(np.float64) * (1, 0, 1)
    light, I = np.float64([0.3, 1.5, -0.2]), np.float64([3.0, 2.5, 2.0])
    r2 = ((light - p) ** 2).sum(-1)
    want = (0.5 / np.pi * I / (4 * np.pi * r2[..., None]) * (light[1] / np.sqrt(r2))[..., None]).mean(axis=2)
    err = float((np.abs(rgb - want) / want).max())
    env, st_env = rp.render_camera_model(s, "environment", SEED)
    # the lat-long camera at the same place: a ray sees the plane where it points down and lands inside the 6 x 6 quad, and nothing (black) elsewhere
    er = cameras.environment(c2w, NX, NY, pf)
    o, dr = er[..., 0:3].astype(np.float64), er[..., 4:7].astype(np.float64)
    down = dr[..., 1] < 0
    t = np.where(down, -o[..., 1] / np.where(down, dr[..., 1], -1.0), 0.0)
    pe = o + t[..., None] * dr
    on = down & (np.abs(pe[..., 0]) < 3) & (np.abs(pe[..., 2]) < 3)
    r2e = ((light - pe) ** 2).sum(-1)
    want_env = np.where(on[..., None], 0.5 / np.pi * I / (4 * np.pi * r2e[..., None]) * (light[1] / np.sqrt(r2e))[..., None], 0.0).mean(axis=2)
    err_env = float((np.abs(env - want_env) / np.maximum(want_env, 1e-4)).max())
    print(f"\nRAYS render_pbrt: orthographic {NX}x{NY}x{NS}, worst relative error of a pixel {err:.3e} (bound 1e-4); environment: {int(on.sum())} of {on.size} rays see the plane, "
          f"worst error of a pixel over max(value, 1e-4) {err_env:.3e} (bound 1e-4)")
    assert err <= 1e-4
    assert env.shape == (NY, NX, 3) and np.all(np.isfinite(env)) and st_env["camera_rays"] == NX * NY * NS
    assert 0.1 < on.mean() < 0.6 and err_env <= 1e-4
