"""Ray differentials with caller-supplied rays on the GPU (RT_FLAG_RAY_DIFFERENTIALS: records of 20 floats in HostScene.render_rays and RayFrame.advance*) and
HostScene.camera_rays (rt_camera_rays), held bit for bit to the camera's own frames on scenes whose textures READ differentials - where the 8-float records of
tests/test_gpu_render_rays.py and tests/test_gpu_ray_frame.py cannot reproduce them - and, for an orthographic camera, to arithmetic.
Shapes are those tests': 32 x 32 x 16 spp for calls, 24 x 20 x 16 with steps [3, 5, 8] for frames, box filter of radius 0.5. Scenes: (t) a plain-triangle room - matte
floor over an EWA image map, a closed-form checkerboard wall, an fbm wall, a plastic wall whose Kd is a trilinear image map, a bump-mapped plastic ceiling, a glass pane,
one area light: the Lambert, two-lobe and generic queue classes all occur -, (tg) = (t) plus a sphere and an object instance with textured materials (the GENERAL forms),
(t_lens) = (t) under a thin lens. The image maps are 64 x 64 random texels repeated 6 to 8 times over a wall: a camera ray's footprint at quarter-pixel differentials
(16 spp) then spans two texels or more at most first hits, so a zero-width lookup gives other values - test 2 asserts that it does. Every measured figure is printed
before it is asserted."""
import numpy as np
import pytest

from util import bits

pytestmark = pytest.mark.gpu

W = H = 32
FW, FH = 24, 20
SPP = 16
STEPS = [3, 5, 8]
COUNTS = ("camera_rays", "rays_closest", "rays_shadow", "rays_mis", "rays_mis_any", "rays_mis_not_cast", "rays_tail_not_cast", "rays_shadow_not_cast", "paths_scrubbed",
          "vertices_lambert_const", "vertices_lambert", "vertices_two_lobe", "vertices_generic")


def _box(d):
    d.film.filter_kind, d.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)   # box filter, radius 0.5
    return d


def _textured(w, h, general=False, lens_radius=0.0):
    from rustracer_amd.scene_desc import SceneDesc
    rng = np.random.default_rng(17)
    s = SceneDesc()
    uv4 = [(0, 0), (1, 0), (1, 1), (0, 1)]
    ewa = s.image_tex(s.add_mip(rng.uniform(0.05, 0.95, (64, 64, 3)).astype(np.float32)), su=8.0, sv=8.0)
    tri = s.image_tex(s.add_mip(rng.uniform(0.05, 0.95, (64, 64, 3)).astype(np.float32), trilinear=True), su=6.0, sv=6.0, du=0.3, dv=0.1)
    chk = s.checker_tex((0.85, 0.8, 0.7), (0.1, 0.15, 0.2), su=22.0, sv=18.0)
    fbm = s.fbm_tex(omega=0.6, octaves=8)
    m_floor, m_chk, m_fbm = s.matte(ewa), s.matte(chk), s.matte(s.scale_tex(s.const_tex((0.9, 0.8, 0.7)), fbm))
    m_plastic = s.plastic(tri, (0.3, 0.3, 0.3), 0.2)
    m_bump = s.set_bump(s.plastic((0.5, 0.45, 0.4), (0.3, 0.3, 0.3), 0.25), s.scale_tex(s.const_tex(0.05), chk))
    m_glass = s.glass()
    quad = [[0, 1, 2], [0, 2, 3]]
    s.add_mesh([(-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2)], quad, m_floor, UV=uv4)
    s.add_mesh([(-2, 0, 2), (2, 0, 2), (2, 3, 2), (-2, 3, 2)], quad, m_chk, UV=uv4)
    s.add_mesh([(2, 0, 2), (2, 0, -2), (2, 3, -2), (2, 3, 2)], quad, m_fbm, UV=uv4)
    s.add_mesh([(-2, 0, -2), (-2, 0, 2), (-2, 3, 2), (-2, 3, -2)], quad, m_plastic, UV=uv4)
    s.add_mesh([(-2, 3, -2), (2, 3, -2), (2, 3, 2), (-2, 3, 2)], quad, m_bump, UV=uv4)
    s.add_quad((0.3, 0, 0.5), (1.3, 0, 0.5), (1.3, 1.5, 0.5), (0.3, 1.5, 0.5), m_glass)
    if general:
        s.add_sphere((-0.9, 0.6, 0.4), 0.6, s.matte(s.image_tex(s.add_mip(rng.uniform(0.05, 0.95, (64, 64, 3)).astype(np.float32)), su=6.0, sv=4.0)))
        P = np.float32([(0, 1, 0), (-0.6, 0, -0.6), (0.6, 0, -0.6), (0.6, 0, 0.6), (-0.6, 0, 0.6)])
        o = s.add_object([dict(P=P, idx=np.int32([(0, 2, 1), (0, 3, 2), (0, 4, 3), (0, 1, 4)]), material=s.plastic(s.checker_tex((0.8, 0.2, 0.2), (0.1, 0.1, 0.3), su=9.0, sv=7.0), 0.2, 0.3))])
        m = np.eye(4, dtype=np.float32)
        m[:3, 3] = (0.6, 0.0, -0.6)
        s.add_instance(o, m)
    s.add_quad((-0.5, 2.99, -0.5), (0.5, 2.99, -0.5), (0.5, 2.99, 0.5), (-0.5, 2.99, 0.5), s.matte((0, 0, 0)), emission=(14, 14, 14))
    s.camera.pos, s.camera.look, s.camera.fov = (0.2, 1.5, -3.5), (0.0, 1.3, 0.0), 60.0
    if lens_radius > 0:
        s.camera.lens_radius, s.camera.focal_distance = lens_radius, 3.5
    s.film.xres, s.film.yres = w, h
    s.sampler.spp = SPP
    return _box(s)


def _reference(gpu_host, d, w, h):
    """One scene uploaded once: the camera's 20-float rays and film positions (camera_rays), its per-sample radiance and first-hit features. Left unchanged."""
    hs = gpu_host.HostScene(d)
    assert hs.samples_window() == (0, 0, w, h)
    assert hs.scene_query(gpu_host.RT_QUERY_NEEDS_DIFFERENTIALS) == 1   # the textures read differentials: the camera's frames regenerate them at bounce 0
    rays, cpf = hs.camera_rays(differentials=True)
    rad, pf, stats = hs.render_samples(with_p_film=True)
    out = dict(h=hs, rays=rays, cpf=cpf, rad=rad, pf=pf, stats=stats)
    for a in (rays, cpf, rad, pf):
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def scenes(gpu_host):
    out = {}
    for name, d in (("t", _textured(W, H)), ("tg", _textured(W, H, general=True)), ("t_lens", _textured(W, H, lens_radius=0.08))):
        out[name] = _reference(gpu_host, d, W, H)
        out[name]["ray_rad"], out[name]["ray_stats"] = out[name]["h"].render_rays(out[name]["rays"])
        out[name]["ray_rad"].setflags(write=False)
    return out


@pytest.fixture(scope="module")
def frame_scenes(gpu_host):
    return {name: _reference(gpu_host, d, FW, FH) for name, d in (("t", _textured(FW, FH)), ("tg", _textured(FW, FH, general=True)))}


def _cut(a, s0, n):
    return np.ascontiguousarray(a[:, :, s0:s0 + n])


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["t", "t_lens"])
def test_camera_rays_are_the_camera_frames_rays(scenes, name):
    import torch
    sc = scenes[name]
    h, rays, cpf = sc["h"], sc["rays"], sc["cpf"]
    feat = h.sample_features()
    assert rays.shape == (H, W, SPP, 20) and rays.dtype == np.float32 and cpf.shape == (H, W, SPP, 2)
    d_o, d_d = int((bits(rays[..., 0:3]) != bits(feat[..., 0:3])).sum()), int((bits(rays[..., 4:7]) != bits(feat[..., 3:6])).sum())
    d_pf = int((bits(cpf) != bits(sc["pf"])).sum())
    rays8, pf8 = h.camera_rays()
    d_8 = int((bits(rays8) != bits(np.ascontiguousarray(rays[..., :8]))).sum())
    lo, lo_pf = h.camera_rays(sample0=0, n_samples=3, differentials=True)
    hi, hi_pf = h.camera_rays(sample0=3, differentials=True)   # (n_samples None: the rest, 13)
    d_cat = int((bits(np.concatenate([lo, hi], axis=2)) != bits(rays)).sum()) + int((bits(np.concatenate([lo_pf, hi_pf], axis=2)) != bits(cpf)).sum())
    t_rays = torch.full((H, W, SPP, 20), -7.0, dtype=torch.float32, device="cuda")
    t_pf = torch.full((H, W, SPP, 2), -7.0, dtype=torch.float32, device="cuda")
    got_r, got_pf = h.camera_rays(differentials=True, device_out=(t_rays, t_pf))
    torch.cuda.synchronize()
    d_dev = int((bits(got_r.cpu().numpy()) != bits(rays)).sum()) + int((bits(got_pf.cpu().numpy()) != bits(cpf)).sum())
    no_pf = h.camera_rays(differentials=True, with_p_film=False)
    nonzero = float((np.abs(rays[..., 8:20]).max(-1) > 0).mean())
    off = float(np.abs(rays[..., 14:17] - rays[..., 4:7]).max())
    print(f"\nRAYDIFF 1 ({name}): o words differing from sample_features' {d_o}, d words {d_d}; p_film words differing from render_samples' {d_pf}; 8-float form against "
          f"the first 8 floats {d_8}; [0, 3) + [3, 16) against the one call {d_cat}; device outputs against host outputs {d_dev}; records with differentials {nonzero:.3f}; "
          f"largest |rx_d - d| {off:.3e}")
    assert d_o == 0 and d_d == 0 and np.all(np.isinf(rays[..., 3])) and np.all(rays[..., 3] > 0) and np.all(rays[..., 7] == 0)
    assert d_pf == 0 and d_8 == 0 and rays8.shape == (H, W, SPP, 8) and pf8.tobytes() == cpf.tobytes()
    assert lo.shape == (H, W, 3, 20) and hi.shape == (H, W, 13, 20) and d_cat == 0
    assert got_r is t_rays and got_pf is t_pf and d_dev == 0
    assert no_pf[1] is None and no_pf[0].tobytes() == rays.tobytes()
    assert nonzero == 1.0 and 0 < off < 0.05   # a quarter of a pixel of a 60 degree, 32-pixel film: 0.036 / 4


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["t", "tg", "t_lens"])
def test_the_cameras_rays_with_differentials_give_the_cameras_radiance_bit_for_bit(scenes, name):
    sc = scenes[name]
    h, rad, ray_rad = sc["h"], sc["rad"], sc["ray_rad"]
    diff = int((bits(ray_rad) != bits(rad)).sum())
    counts = {k: (sc["ray_stats"][k], sc["stats"][k]) for k in COUNTS}
    plain, plain_stats = h.render_rays(np.ascontiguousarray(sc["rays"][..., :8]))   # the same rays without the flag: zero-width lookups
    lit = rad[..., :3].max(-1) > 0
    moved = (bits(plain) != bits(rad)).any(-1)
    share_lit, share_moved = float(lit.mean()), float(moved[lit].mean())
    print(f"\nRAYDIFF 2 ({name}) {W * H * SPP} rays: radiance words differing from render_samples' {diff}; lit samples {share_lit:.3f}; lit samples the unflagged rays "
          f"move {share_moved:.3f}; counts (rays, samples) {counts}")
    assert sc["stats"]["vertices_lambert"] > 0 and sc["stats"]["vertices_two_lobe"] > 0 and sc["stats"]["vertices_generic"] > 0
    assert diff == 0
    assert all(a == b for a, b in counts.values()) and sc["ray_stats"]["camera_rays"] == W * H * SPP
    assert np.all(ray_rad[..., 3] == rad[..., 3]) and set(np.unique(ray_rad[..., 3])) <= {0.0, 1.0}
    assert share_lit > 0.05 and share_moved >= 0.25   # the test has power: without differentials the result is another one
    assert plain_stats["camera_rays"] == W * H * SPP


# ---------------------------------------------------------------------------------------------- 3
def test_ranges_windows_and_zeroed_fields(scenes, gpu_host):
    sc = scenes["tg"]
    h = sc["h"]
    # rows 3 .. 31, columns 0 .. 28: a window that is no multiple of a tile, whose own keys differ from the film's - compared with itself, cut two ways (ray_s0 != 0)
    sub = np.ascontiguousarray(sc["rays"][3:, :29])
    whole, _ = h.render_rays(sub)
    parts = np.concatenate([h.render_rays(_cut(sub, 0, 3), sample0=0)[0], h.render_rays(_cut(sub, 3, 13), sample0=3)[0]], axis=2)
    sub_plain, _ = h.render_rays(np.ascontiguousarray(sub[..., :8]))
    d_parts = int((bits(parts) != bits(whole)).sum())
    lit = whole[..., :3].max(-1) > 0
    moved = float((bits(sub_plain) != bits(whole)).any(-1)[lit].mean())
    print(f"\nRAYDIFF 3 (tg) 29 x 29 pixels, [0, 3) + [3, 16): differing words {d_parts}; lit {float(lit.mean()):.3f}; lit samples that move without the flag {moved:.3f}")
    assert d_parts == 0 and lit.mean() > 0.05 and moved >= 0.25
    # zeroed differential fields: compute_differential returns early (a division by zero), the vertex is that of a ray without differentials
    for name in ("t", "tg"):
        s2 = scenes[name]
        zeroed = s2["rays"].copy()
        zeroed[..., 8:] = 0
        z, z_stats = s2["h"].render_rays(zeroed)
        plain, plain_stats = s2["h"].render_rays(np.ascontiguousarray(s2["rays"][..., :8]))
        d_z = int((bits(z) != bits(plain)).sum())
        print(f"RAYDIFF 3 ({name}) zeroed differentials with the flag against the unflagged call: differing words {d_z}")
        assert d_z == 0 and all(z_stats[k] == plain_stats[k] for k in COUNTS)
    # a scene whose textures read no differentials: the fields are never read
    from test_gpu_render_rays import _cornell, _room
    rng = np.random.default_rng(8)
    for name, d in (("cornell", _cornell()), ("room", _room())):
        u = gpu_host.HostScene(d)
        assert u.scene_query(gpu_host.RT_QUERY_NEEDS_DIFFERENTIALS) == 0
        r20, _ = u.camera_rays(differentials=True)
        junk = r20.copy()
        junk[..., 8:] = rng.normal(size=junk[..., 8:].shape)   # whatever the fields hold
        a, a_stats = u.render_rays(np.ascontiguousarray(r20[..., :8]))
        b, b_stats = u.render_rays(r20)
        c, _ = u.render_rays(junk)
        ref, _, _ = u.render_samples(with_p_film=False)
        d_b, d_c, d_ref = int((bits(a) != bits(b)).sum()), int((bits(a) != bits(c)).sum()), int((bits(a) != bits(ref)).sum())
        print(f"RAYDIFF 3 untextured ({name}): flagged against unflagged {d_b}, flagged with arbitrary fields {d_c}, against render_samples {d_ref}")
        assert d_b == 0 and d_c == 0 and d_ref == 0 and all(a_stats[k] == b_stats[k] for k in COUNTS)


# ---------------------------------------------------------------------------------------------- 4
def _read(frame):
    return dict(film=frame.film(), stats=np.stack(frame.pixel_stats()), features=frame.features())


def _differing(a, b):
    return {k: int((np.ascontiguousarray(a[k]).view(np.uint8) != np.ascontiguousarray(b[k]).view(np.uint8)).sum()) for k in a}


@pytest.mark.parametrize("name", ["t", "tg"])
def test_a_ray_frame_of_the_cameras_rays_is_the_camera_frame(frame_scenes, name):
    sc = frame_scenes[name]
    h, rays, pf = sc["h"], sc["rays"], sc["cpf"]
    assert rays.shape == (FH, FW, SPP, 20)
    for rank, world in ((0, 1), (1, 2)):
        with h.progressive(rank=rank, world_size=world, pixel_stats=True, features=True) as cam:
            cam_stats = [cam.advance(n) for n in STEPS]
            want = _read(cam)
        with h.progressive_rays(FW, FH, rank=rank, world_size=world, pixel_stats=True, features=True) as fr:
            s0, stats = 0, []
            for n in STEPS:
                stats.append(fr.advance(_cut(rays, s0, n), _cut(pf, s0, n)))
                s0 += n
            got = _read(fr)
            taken = fr.samples_taken
        with h.progressive_rays(FW, FH, rank=rank, world_size=world, pixel_stats=True, features=True) as fr:   # the same steps without the flag
            s0 = 0
            for n in STEPS:
                fr.advance(_cut(np.ascontiguousarray(rays[..., :8]), s0, n), _cut(pf, s0, n))
                s0 += n
            plain = _read(fr)
        d, d_plain = _differing(got, want), _differing(plain, want)
        sums = {k: (sum(s[k] for s in stats), sum(s[k] for s in cam_stats)) for k in COUNTS}
        print(f"\nRAYDIFF 4 ({name}) rank {rank} of {world}, steps {STEPS}: bytes differing from the camera frame's (film, statistics, features) {d}; without the flag {d_plain}; "
              f"samples_taken {taken}; counts (ray frame, camera frame) {sums}")
        assert np.abs(want["film"][..., :3]).max() > 0 and want["features"][..., 7].mean() > 0.1
        assert d == dict(film=0, stats=0, features=0)
        assert all(a == b for a, b in sums.values()) and taken == sums["camera_rays"][0] > 0
        assert d_plain["film"] > 0   # the comparison has power: 8-float records give another film here
    assert np.array_equal(bits(h.render()[0]), bits(_whole_film(h, rays, pf)))


def _whole_film(h, rays, pf):
    with h.progressive_rays(FW, FH) as fr:
        fr.advance(rays, pf)
        return fr.film()


def test_an_adaptive_step_with_the_cameras_rays_is_the_camera_frames(frame_scenes):
    sc = frame_scenes["t"]
    h, rays, pf = sc["h"], sc["rays"], sc["cpf"]
    floor_y, min_samples = float(np.float32(1e-3)), 4
    with h.progressive(pixel_stats=True, features=True) as cam, h.progressive_rays(FW, FH, pixel_stats=True, features=True) as fr:
        cam.advance(4)
        fr.advance(_cut(rays, 0, 4), _cut(pf, 0, 4))
        n, sy, sy2 = (a.copy() for a in cam.pixel_stats())
        mean = sy / n
        se = np.sqrt(np.maximum(sy2 - sy * mean, 0.0) / (n - 1.0) / n)
        thr = float(np.float32(np.median(se / np.maximum(mean, floor_y))))   # about half the pixels stay active
        cam_st = cam.advance_adaptive(4, thr, floor_y, min_samples)
        st = fr.advance_adaptive(_cut(rays, 4, 4), _cut(pf, 4, 4), thr, floor_y, min_samples)
        d = _differing(_read(fr), _read(cam))
        share = fr.active_pixels / (FW * FH)
        print(f"\nRAYDIFF 4 (t) adaptive step of 4 after [4], threshold {thr:.6f}: active pixels {fr.active_pixels} / {cam.active_pixels} ({share:.3f}); camera_rays "
              f"{st['camera_rays']} / {cam_st['camera_rays']}; bytes differing (film, statistics, features) {d}")
        assert fr.active_pixels == cam.active_pixels and 0.1 <= share <= 0.9
        assert st["camera_rays"] == cam_st["camera_rays"] == 4 * fr.active_pixels and fr.samples_taken == cam.samples_taken
        assert d == dict(film=0, stats=0, features=0)


# ---------------------------------------------------------------------------------------------- 5
def test_orthographic_differentials_over_a_textured_plane_against_arithmetic(gpu_host):
    """test_orthographic_rays_over_a_textured_plane_against_arithmetic of tests/test_gpu_render_rays.py with a trilinear 64 x 64 map repeated 5 times and
    cameras.orthographic(.., differentials=True, spp=4): expected Kd = HostScene.texture_eval at the hit's uv with duv computed in float64 from the records' own
    rx_o - o and ry_o - o (parallel rays straight down onto y = 0: the hit moves as the origin does; u = (x + 1) / 2, v = (z + 1) / 2). Bound 1e-4 relative per ray, that
    test's: the float32 compute_differential puts a few 1e-6 of relative error on duv, and a trilinear lookup moves by about as much as duv does (measured on the CPU
    model: 1.3e-5 for 1e-5); an EWA lookup would not (1.7e-3). The filtered expectation must differ from the zero-width one by > 1 % on most rays."""
    from rustracer_amd import cameras
    from rustracer_amd.scene_desc import SceneDesc
    N, NS = 16, 4
    rng = np.random.default_rng(5)
    s = SceneDesc()
    tex = s.image_tex(s.add_mip(rng.uniform(0.2, 0.9, (64, 64, 3)).astype(np.float32), trilinear=True), su=5.0, sv=5.0)
    s.add_mesh([(-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1)], [[0, 1, 2], [0, 2, 3]], s.matte(tex), UV=[(0, 0), (1, 0), (1, 1), (0, 1)])
    light, I = np.float64([0.3, 1.5, -0.2]), np.float64([3.0, 2.5, 2.0])
    s.point_light(tuple(light), tuple(I))
    s.film.xres, s.film.yres = N, N
    s.sampler.spp = NS
    s.integrator.max_depth = 1
    h = gpu_host.HostScene(_box(s))
    assert h.scene_query(gpu_host.RT_QUERY_NEEDS_DIFFERENTIALS) == 1
    _, c2w = gpu_host.look_at((0.0, 2.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    pf = cameras.pixel_centres(N, N, NS) + rng.uniform(-0.5, 0.5, (N, N, NS, 2))
    rays = cameras.orthographic(c2w, (-0.9, 0.9, -0.9, 0.9), N, N, pf, differentials=True, spp=NS)
    assert rays.shape == (N, N, NS, 20) and np.abs(rays[..., 4:7] - np.float32([0, -1, 0])).max() < 1e-6 and np.all(rays[..., 1] == 2.0)
    rad, st = h.render_rays(rays)
    r64 = rays.reshape(-1, 20).astype(np.float64)
    p = r64[:, 0:3] * (1, 0, 1)   # straight down onto y = 0
    uv = np.stack([(p[:, 0] + 1) / 2, (p[:, 2] + 1) / 2], axis=1)
    dx, dy = r64[:, 8:11] - r64[:, 0:3], r64[:, 11:14] - r64[:, 0:3]
    duv = np.stack([dx[:, 0] / 2, dx[:, 2] / 2, dy[:, 0] / 2, dy[:, 2] / 2], axis=1)   # dudx dvdx dudy dvdy
    kd = h.texture_eval(tex, uv.astype(np.float32), duv=duv.astype(np.float32)).astype(np.float64)
    kd0 = h.texture_eval(tex, uv.astype(np.float32)).astype(np.float64)
    r2 = ((light - p) ** 2).sum(1)
    shade = (I / (4 * np.pi * r2[:, None])) * (light[1] / np.sqrt(r2))[:, None] / np.pi
    got = rad[..., :3].reshape(-1, 3).astype(np.float64)
    err = float((np.abs(got - kd * shade) / (kd * shade)).max())
    err0 = float((np.abs(got - kd0 * shade) / (kd0 * shade)).max())
    far = float(((np.abs(kd - kd0) / kd0).max(1) > 0.01).mean())
    step = float(np.abs(duv).max())
    print(f"\nRAYDIFF 5 ortho: {len(p)} rays, largest |duv| {step:.4f} (a texel of the repeated map: {1 / (5 * 64):.4f}); worst relative error against the filtered lookup "
          f"{err:.3e} (bound 1e-4), against the zero-width lookup {err0:.3e}; rays whose filtered Kd is > 1 % off the zero-width one {far:.3f}; camera_rays {st['camera_rays']}")
    assert np.all(rad[..., 3] == 0) and st["camera_rays"] == N * N * NS
    assert far > 0.5
    assert err <= 1e-4


# ---------------------------------------------------------------------------------------------- 6
def test_nothing_else_moves(scenes):
    sc = scenes["t"]
    h = sc["h"]
    rays8 = np.ascontiguousarray(sc["rays"][..., :8])
    pf = sc["cpf"]

    def unflagged():
        film, _ = h.render()
        rad, _, _ = h.render_samples(with_p_film=False)
        ray_rad, _ = h.render_rays(rays8)
        with h.progressive_rays(W, H) as fr:
            fr.advance(_cut(rays8, 0, 5), _cut(pf, 0, 5))
            frame = fr.film()
        return dict(film=film, rad=rad, ray_rad=ray_rad, frame=frame)

    before = unflagged()
    flagged, _ = h.render_rays(sc["rays"])
    with h.progressive_rays(W, H) as fr:
        fr.advance(_cut(sc["rays"], 0, 5), _cut(pf, 0, 5))
        flagged_frame = fr.film()
    after = unflagged()
    d = _differing(after, before)
    print(f"\nRAYDIFF 6 (t): bytes of render(), render_samples(), an unflagged render_rays and an unflagged ray frame that differ after flagged calls {d}; words of the "
          f"flagged frame differing from the unflagged one {int((bits(flagged_frame) != bits(before['frame'])).sum())}")
    assert d == dict(film=0, rad=0, ray_rad=0, frame=0)
    assert before["rad"].tobytes() == sc["rad"].tobytes() and flagged.tobytes() == sc["ray_rad"].tobytes() and np.abs(before["film"][..., :3]).max() > 0
    assert (bits(flagged_frame) != bits(before["frame"])).any()


def test_render_pbrt_ray_differentials(gpu_host):
    """scripts/render_pbrt.py --camera-model environment --ray-frame --ray-differentials on a small scene file with a closed-form checkerboard: a finite image, another
    one than the run without the option gives; and so without --ray-frame."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("render_pbrt", os.path.join(root, "scripts", "render_pbrt.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    NX, NY, NS, SEED = 16, 12, 4, 7
    text = f"""LookAt 0 1 0  1 0.5 0  0 1 0
Camera "perspective" "float fov" [45]
Sampler "02sequence" "integer pixelsamples" [{NS}]
PixelFilter "box" "float xwidth" [0.5] "float ywidth" [0.5]
Film "image" "integer xresolution" [{NX}] "integer yresolution" [{NY}]
Integrator "path" "integer maxdepth" [1]
WorldBegin
LightSource "point" "rgb I" [30 25 20] "point from" [0.3 2.5 -0.2]
Texture "chk" "spectrum" "checkerboard" "float uscale" [40] "float vscale" [40] "rgb tex1" [0.9 0.9 0.9] "rgb tex2" [0.05 0.05 0.05]
Material "matte" "texture Kd" "chk"
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-6 0 -6  6 0 -6  6 0 6  -6 0 6] "float uv" [0 0 1 0 1 1 0 1]
WorldEnd
"""
    s = gpu_host.PbrtScene(text=text)
    assert s.scene_query(gpu_host.RT_QUERY_NEEDS_DIFFERENTIALS) == 1
    plain = rp.render_camera_model_frame(s, "environment", SEED)
    diff = rp.render_camera_model_frame(s, "environment", SEED, differentials=True)
    again = rp.render_camera_model_frame(s, "environment", SEED)
    call_plain, _ = rp.render_camera_model(s, "environment", SEED)
    call_diff, st = rp.render_camera_model(s, "environment", SEED, differentials=True)
    moved = float(np.abs(diff["rgb"].astype(np.float64) - plain["rgb"]).max() / np.abs(plain["rgb"]).max())
    moved_call = float(np.abs(call_diff.astype(np.float64) - call_plain).max() / np.abs(call_plain).max())
    agree = float(np.abs(diff["rgb"].astype(np.float64) - call_diff).max() / np.abs(call_diff).max())
    print(f"\nRAYDIFF 6 render_pbrt --camera-model environment --ray-differentials, {NX}x{NY}x{NS}: --ray-frame image moves by {moved:.3e} of its brightest value, "
          f"the plain call's by {moved_call:.3e}; the two routes differ by {agree:.3e}; camera_rays {diff['stats']['camera_rays']}")
    assert diff["rgb"].shape == (NY, NX, 3) and np.all(np.isfinite(diff["rgb"])) and diff["rgb"].max() > 0 and diff["stats"]["camera_rays"] == NX * NY * NS
    assert moved > 1e-3 and moved_call > 1e-3
    assert again["rgb"].tobytes() == plain["rgb"].tobytes()   # the default output of the script does not change
    assert np.all(np.isfinite(call_diff)) and st["camera_rays"] == NX * NY * NS and agree <= 4 * 2.0 ** -23   # (a mean of 4 against sums over weights: tests/test_gpu_ray_frame.py)
