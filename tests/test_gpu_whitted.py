"""rt_render_rays_whitted / rt_render_whitted on the GPU (HostScene.render_rays_whitted, HostScene.render_whitted) held to the float64 model of tests/whitted_model.py:
EVERY sample of every batch - 40 x 24 pixels x 4 samples = 3840 rays, 15 workgroups of the vertex kernel, the last one partial - is compared, its radiance and the exact
shape of its recursion (info: li invocations and get_2d() draws). That is legitimate because the batches keep their distance from every decision float32 could take
differently (tests/whitted_cases.py; tests/test_whitted_cpu.py asserts the margins of the model alone). Every measured figure is printed before it is asserted.

Tolerances on L, per sample and channel, |L - model| <= RTOL * max(model over the batch) + RTOL * |model|:
  flat scenes (floor, mirrors, mix): RTOL = 2e-4. A float32 hit point is within gamma(7) |p| ~ 4e-7 x 10 scene units of the exact one, ~1e-5 of the distances (>= 0.5) that
    enter 1 / r^2 and the cosines; a flat mirror passes that on unamplified, 16 of them add up to <= 2e-4; the throughput is a product of at most 16 factors of a few
    2^-24 each (v_rcp_f32 included: 1 ulp), which is below that.
  curved glass (glass, area): RTOL = 3e-3. A sphere of radius 0.5 turns a position error e into a direction error ~ e / r at each of up to four interfaces and the
    floor is ~1 - 2 units further: (1 + 2 / 0.5)^2 ~ 25 per pair of interfaces, ~10^2 over a tree of depth 5, on 1e-5: 1e-3; the Fresnel term near the 1e-3-margin of the
    critical angle varies like 1 / sqrt(1 - sin^2), a factor <= 30 on the same error. 3e-3 covers both.
The area light's figures at dimensions = 8 differ from dimensions = 2 (other draws), both against the model."""
import numpy as np
import pytest

import whitted_cases as wc
from util import bits

pytestmark = pytest.mark.gpu

RTOL = dict(many=2e-4, floor=2e-4, mirrors=2e-4, mix=2e-4, glass=3e-3, glass_triangles=2e-4, glass_inside=2e-4, area=3e-3)
N = wc.H * wc.W * wc.NS


@pytest.fixture(scope="module")
def scenes(gpu_host):
    """One uploaded HostScene per (case, dimensions), made on first use."""
    made = {}

    def get(orc, name, dims):
        if (name, dims) not in made:
            b, _ = wc.settled(orc, name)
            h = gpu_host.HostScene(b.desc(dims))
            h.upload(0)
            made[(name, dims)] = h
        return made[(name, dims)]
    return get


def _compare(tag, name, L, info, st, res, rays, n_lights):
    """Print, then assert: status, info and radiance of every sample against the model's Result."""
    L, info = L.reshape(N, 4), info.reshape(N, 2).astype(np.int64)
    active = rays.reshape(N, 8)[:, 3] > 0
    want = res.L
    scale = np.abs(want).max()
    err = np.abs(L[:, :3].astype(np.float64) - want)
    bound = RTOL[name] * scale + RTOL[name] * np.abs(want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    node_diff, draw_diff = int((info[:, 0] != res.nodes).sum()), int((info[:, 1] != res.draws).sum())
    print(f"\n{tag}: nodes {res.nodes[active].min()} .. {res.nodes.max()} (differ: {node_diff}), draws up to {res.draws.max()} (differ: {draw_diff}), max |L| {scale:.4g}, "
          f"lit samples {(want.sum(1) > 0).mean():.2f}, worst error / bound {worst:.3f} (max abs error {err.max():.3e}), status {np.unique(L[:, 3])}; "
          f"rays {st['camera_rays']} / {st['rays_closest']} / {st['rays_shadow']}, launches {st['launches_trace_path']} / {st['launches_shade']} / {st['launches_trace_shadow']}")
    assert np.array_equal(L[:, 3], np.where(active, 0.0, 2.0).astype(np.float32))
    assert node_diff == 0 and draw_diff == 0
    assert not info[~active].any() and not L[~active, :3].any()
    assert worst <= 1.0
    assert st["camera_rays"] == int(active.sum()) and st["rays_closest"] == int(res.nodes.sum()) and st["paths_scrubbed"] == 0
    steps = int(res.nodes.max())   # a step per node of the deepest tree: one closest-hit launch, max(n_lights, 1) vertex rounds, n_lights any-hit launches
    assert (st["launches_trace_path"], st["launches_shade"], st["launches_trace_shadow"]) == (steps, steps * max(n_lights, 1), steps * n_lights)


RUN_IDS = [(name, md, dims) for name in wc.CASES for md, dims in wc.RUNS[name]]


@pytest.mark.parametrize("name,max_depth,dims", RUN_IDS, ids=[f"{n}-d{m}-dims{d}" for n, m, d in RUN_IDS])
def test_every_sample_against_the_model(scenes, orc, name, max_depth, dims):
    """The cases of tests/whitted_cases.py: 1 a matte floor under a point light with misses and skipped rays; 2 two facing mirrors before a lit wall at max_depth 1, 2, 5
    and 16 (the deepest stack); 3 a glass slab and a glass sphere (the GENERAL kernel), the slab alone (the plain kernel), rays inside the slab beyond the critical angle;
    4 the glass scene under a two-triangle area light with every draw from the stream (dimensions = 2) and the first six from the tables (dimensions = 8);
    5 a mix of two mirrors (u[0] chooses the lobe) under a point light and a constant infinite light; 6 (first) 48 listed lights - 48 rounds per step, 100 draws per
    sample, most of them from the stream and carried from round to round in the state record."""
    res, (b, rays) = wc.reference(orc, name, max_depth, dims)
    h = scenes(orc, name, dims)
    L, info, st = h.render_rays_whitted(rays, max_depth=max_depth, with_info=True)
    n_lights = len(b.model.lights)
    _compare(f"Whitted {name} max_depth {max_depth} dimensions {dims}", name, L, info, st, res, rays, n_lights)
    active = rays.reshape(N, 8)[:, 3] > 0
    if name == "floor":  # (1, n_lights) at depth 1, (1, n_lights + 2) at depth 5; a miss: L = 0, (1, 0)
        hit = active & (np.arange(N) < 16 * wc.W * wc.NS)
        miss = active & ~hit
        inf = info.reshape(N, 2)
        assert (inf[hit] == (1, n_lights if max_depth == 1 else n_lights + 2)).all() and (inf[miss] == (1, 0)).all() and not L.reshape(N, 4)[miss, :3].any()
        assert int((~active).sum()) == wc.H * wc.NS + 1
    if name == "mirrors":
        assert res.nodes.max() == max_depth and (max_depth < 16 or res.nodes.min() < 16)  # some rays reach the wall before the depth limit, some do not
    if name == "glass_inside":  # total internal reflection at every vertex: a chain, no transmission child
        assert (info.reshape(N, 2)[:, 0] == max_depth).all() and (info.reshape(N, 2)[:, 1] == max_depth * n_lights + 2 * (max_depth - 1)).all()
    general = h.scene_query(8)
    print(f"kernel launched: {general} (1 plain, 2 GENERAL)")
    assert general == (2 if name in ("glass", "glass_inside", "area") else 1)


def test_sample_ranges_add_up_bit_for_bit_and_device_buffers(scenes, orc):
    """Calls over [0, 1) + [1, 4) give the call over [0, 4) bit for bit - radiance and info - and so does the call on device pointers."""
    import torch
    res, (b, rays) = wc.reference(orc, "area", 5, 2)
    h = scenes(orc, "area", 2)
    L, info, _ = h.render_rays_whitted(rays, max_depth=5, with_info=True)
    La, ia, _ = h.render_rays_whitted(rays[:, :, :1], max_depth=5, sample0=0, with_info=True)
    Lb, ib, _ = h.render_rays_whitted(rays[:, :, 1:], max_depth=5, sample0=1, with_info=True)
    d1 = int((bits(np.concatenate([La, Lb], axis=2)) != bits(L)).sum()) + int((np.concatenate([ia, ib], axis=2) != info).sum())
    dev_rays = torch.from_numpy(rays).cuda()
    out, inf = torch.zeros((wc.H, wc.W, wc.NS, 4), dtype=torch.float32, device="cuda"), torch.zeros((wc.H, wc.W, wc.NS, 2), dtype=torch.int32, device="cuda")
    h.render_rays_whitted(dev_rays, max_depth=5, with_info=True, device_out=out, device_info_out=inf)
    torch.cuda.synchronize()
    d2 = int((bits(out.cpu().numpy()) != bits(L)).sum()) + int((inf.cpu().numpy().astype(np.uint32) != info).sum())
    again, _, _ = h.render_rays_whitted(rays, max_depth=5)
    d3 = int((bits(again) != bits(L)).sum())
    print(f"\nWhitted ranges: [0, 1) + [1, 4) differs from [0, 4) in {d1} words, the device-pointer call in {d2}, a second call in {d3}")
    assert d1 == 0 and d2 == 0 and d3 == 0


def _splat_rgb(rgb, pf, table, rx, ry, cropped):
    """FilmTile::add_sample for every sample, per channel, then the film's RGB -> XYZ (test_gpu_ao._splat splats one grey value: its Y row is the weighted sum itself,
    times the sum of the Y coefficients)."""
    from test_gpu_ao import _splat
    c = lambda *v: sum(np.float64(np.float32(x)) for x in v)
    ysum = c(0.212671, 0.715160, 0.072169)
    parts = [_splat(rgb[..., k], pf, table, rx, ry, cropped) for k in range(3)]
    R, G, B = (p[..., 1] / ysum for p in parts)
    m = [[np.float64(np.float32(x)) for x in row] for row in ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))]
    return np.stack([m[0][0] * R + m[0][1] * G + m[0][2] * B, m[1][0] * R + m[1][1] * G + m[1][2] * B, m[2][0] * R + m[2][1] * G + m[2][2] * B, parts[0][..., 3]], axis=-1)


def _frame_scene(gpu_host, orc, gaussian):
    from rustracer_amd.scene_desc import FILTER_GAUSSIAN
    b, _ = wc.settled(orc, "glass")
    d = b.desc(4)
    d.film.filter_kind, d.film.filter_params = (FILTER_GAUSSIAN, (1.5, 1.5, 2.0, 0.0)) if gaussian else (0, (0.5, 0.5, 0.0, 0.0))
    h = gpu_host.HostScene(d)
    h.upload(0)
    return h


def test_frame_is_the_splat_of_the_ray_entrys_samples(gpu_host, orc):
    """rt_render_whitted, 32 x 32 x 4 spp under a Gaussian of radius 1.5, against rt_render_rays_whitted over rt_camera_rays' records splatted by the reference's
    FilmTile::add_sample in float64 (1e-6: the film kernel's float32 sums of up to 36 samples per pixel)."""
    h = _frame_scene(gpu_host, orc, True)
    film, st = h.render_whitted(5)
    setup = h.setup()
    cam_rays, pf = h.camera_rays()
    L, _, st_r = h.render_rays_whitted(cam_rays, max_depth=5)
    want = _splat_rgb(L[..., :3], pf, setup["filter_table"].astype(np.float32), 1.5, 1.5, [int(v) for v in setup["cropped"]])
    err = float(np.linalg.norm(film.astype(np.float64) - want) / np.linalg.norm(want))
    print(f"\nWhitted frame vs splat of rt_render_rays_whitted over rt_camera_rays' records: relative L2 {err:.3e}; film mean Y {film[..., 1].mean():.4f}, "
          f"rays {st['camera_rays']} / {st['rays_closest']} / {st['rays_shadow']} vs {st_r['camera_rays']} / {st_r['rays_closest']} / {st_r['rays_shadow']}")
    assert film.shape == (32, 32, 4) and err <= 1e-6 and film[..., 1].mean() > 1e-3
    assert (st["camera_rays"], st["rays_closest"], st["rays_shadow"]) == (st_r["camera_rays"], st_r["rays_closest"], st_r["rays_shadow"])


def test_two_shards_merge_to_the_unsharded_film_and_the_path_frame_is_untouched(gpu_host, orc):
    """Under the box filter films compare bit for bit: rank 0 + rank 1 of two is the unsharded frame; rt_render before and after a Whitted frame is the same film."""
    from rustracer_amd.distributed import touched_rows
    h = _frame_scene(gpu_host, orc, False)
    before, _ = h.render()
    whole, _ = h.render_whitted(5)
    parts = [h.render_whitted(5, rank=r, world_size=2)[0] for r in range(2)]
    after, _ = h.render()
    st = h.setup()
    rows = touched_rows([int(v) for v in st["cropped"]], [int(v) for v in st["sample_bounds"]], 1, 2, 0.5)
    merged = parts[0].copy()
    merged[rows] += parts[1][rows]
    differ, path_differ = int((bits(merged) != bits(whole)).sum()), int((bits(before) != bits(after)).sum())
    print(f"\nWhitted shards: merged film differs from the unsharded one in {differ} words; rt_render before / after differs in {path_differ}; rank films non-zero: {[bool(p.any()) for p in parts]}")
    assert differ == 0 and path_differ == 0 and all(p.any() for p in parts) and not np.array_equal(whole[..., :3], before[..., :3])


def _textured_scene(gpu_host):
    """A checkerboard floor (closed-form antialiasing: it reads the ray differentials) under a glass slab whose Kr is a checkerboard too - a depth-0 vertex that is pushed,
    popped and rebuilt -, a matte wall and one point light."""
    from rustracer_amd.scene_desc import FILTER_GAUSSIAN, SceneDesc
    s = SceneDesc()
    s.film.xres, s.film.yres = 32, 32
    s.film.filter_kind, s.film.filter_params = FILTER_GAUSSIAN, (1.5, 1.5, 2.0, 0.0)
    s.sampler.spp, s.sampler.dims = 4, 4
    s.camera.pos, s.camera.look, s.camera.fov = (0.0, 2.2, -5.0), (0.0, 0.3, 0.0), 45.0
    # (axes oblique to every face of the scene: on a face perpendicular to v1 the footprint's ds is exactly 0 and the closed form's (b1 - b0) / (2 ds) is 0 / 0 where t
    # crosses a cell - the reference's own NaN (checkerboard.rs:129-131), scrubbed by the renderer; not what this test is about)
    planar = dict(mapping="planar", v1=(1.0, 0.3, 0.2), v2=(0.1, 0.25, 1.0))
    floor = s.matte(s.checker_tex(s.const_tex((0.9, 0.8, 0.2)), s.const_tex((0.1, 0.2, 0.7)), **planar, udelta=0.13, vdelta=0.27))
    kr = s.checker_tex(s.const_tex(1.0), s.const_tex(0.2), **planar, udelta=0.4, vdelta=0.1)
    s.add_quad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6), floor)
    s.add_quad((-6, 0, 6), (6, 0, 6), (6, 12, 6), (-6, 12, 6), s.matte((0.7, 0.5, 0.3)))
    glass, (lo, hi) = s.glass(kr, 1.0, 1.5), ((-1.5, 0.5, -1.0), (1.5, 0.8, 1.0))
    c = [(lo[0], lo[1], lo[2]), (hi[0], lo[1], lo[2]), (hi[0], hi[1], lo[2]), (lo[0], hi[1], lo[2]), (lo[0], lo[1], hi[2]), (hi[0], lo[1], hi[2]), (hi[0], hi[1], hi[2]), (lo[0], hi[1], hi[2])]
    for q in ((0, 3, 2, 1), (4, 5, 6, 7), (0, 4, 7, 3), (1, 2, 6, 5), (3, 7, 6, 2), (0, 1, 5, 4)):
        s.add_quad(*[c[i] for i in q], glass)
    s.point_light((0.5, 5.0, -2.0), (300.0, 300.0, 300.0))
    h = gpu_host.HostScene(s)
    h.upload(0)
    return h


def test_first_vertex_differentials_of_a_textured_scene(gpu_host):
    """A scene whose textures read ray differentials (RT_QUERY_NEEDS_DIFFERENTIALS). The two sources of the first vertex's differentials against each other: the frame
    rebuilds the camera ray's from the film position, rt_render_rays_whitted over rt_camera_rays' 20-float records loads them - the Gaussian-filtered frame is the splat of
    those samples (1e-6, as the untextured frame test). The same rays as 8-float records have no differentials - zero-width lookups - and give another image. And at
    max_depth 1 under the one point light, Whitted::li is f Li |cos| / 1 at the first vertex - what PathIntegrator::li with max_depth 1 returns for a delta light picked
    with probability 1: rt_render_rays on the same 20-float records, the path integrator's first-vertex lookup (k_shade_rays), within 1e-5 of the largest L (a dozen
    float32 operations in another order)."""
    h = _textured_scene(gpu_host)
    assert h.scene_query(6) == 1
    film, st = h.render_whitted(5)
    setup = h.setup()
    cam20, pf = h.camera_rays(differentials=True)
    L20, info20, st_r = h.render_rays_whitted(cam20, max_depth=5, with_info=True)
    want = _splat_rgb(L20[..., :3], pf, setup["filter_table"].astype(np.float32), 1.5, 1.5, [int(v) for v in setup["cropped"]])
    err = float(np.linalg.norm(film.astype(np.float64) - want) / np.linalg.norm(want))
    L8, info8, _ = h.render_rays_whitted(np.ascontiguousarray(cam20[..., :8]), max_depth=5, with_info=True)
    scale = float(L20[..., :3].max())
    moved = float(np.abs(L8[..., :3] - L20[..., :3]).max())
    w1, _, _ = h.render_rays_whitted(cam20, max_depth=1)
    p1, _ = h.render_rays(cam20, max_depth=1)
    d1 = float(np.abs(w1[..., :3].astype(np.float64) - p1[..., :3]).max())
    print(f"\nWhitted textured: frame vs splat of the 20-float records: relative L2 {err:.3e}; 8-float records move L by up to {moved:.4f} of max {scale:.4f}; "
          f"max_depth 1 against rt_render_rays: max abs difference {d1:.3e} of max {float(p1[..., :3].max()):.4f}; nodes up to {info20[..., 0].max()}, rays {st['rays_closest']} / {st_r['rays_closest']}")
    assert np.isfinite(L20).all() and not L20[..., 3].any() and st["paths_scrubbed"] == 0
    assert err <= 1e-6 and film[..., 1].mean() > 1e-3
    assert (st["camera_rays"], st["rays_closest"], st["rays_shadow"]) == (st_r["camera_rays"], st_r["rays_closest"], st_r["rays_shadow"])
    assert np.array_equal(info8, info20) and moved > 1e-2 * scale   # the same trees, other texture values
    assert p1[..., :3].max() > 0.05 and d1 <= 1e-5 * float(p1[..., :3].max()) and info20[..., 0].max() >= 7


def test_a_small_stack_budget_halves_the_pass_and_changes_no_bit(gpu_host, orc, monkeypatch):
    """64 x 64 x 16 spp at max_depth 5 is one pass of 65 536 paths with 16 MiB of pending stack; with a budget of 5 MiB (RTX_WHITTED_STACK_BUDGET) the pass is halved twice
    - 2^14 paths, 4 MiB - and the box-filtered film is the same, bit for bit."""
    b, _ = wc.settled(orc, "glass")
    d = b.desc(4)
    d.film.xres, d.film.yres, d.sampler.spp = 64, 64, 16
    h = gpu_host.HostScene(d)
    h.upload(0)
    whole, st = h.render_whitted(5)
    monkeypatch.setenv("RTX_WHITTED_STACK_BUDGET", str(5 << 20))
    cut, st_c = h.render_whitted(5)
    differ = int((bits(cut) != bits(whole)).sum())
    print(f"\nWhitted stack budget: passes {st['n_passes']} -> {st_c['n_passes']}, films differ in {differ} words, rays {st['rays_closest']} / {st_c['rays_closest']}")
    assert st["n_passes"] == 1 and st_c["n_passes"] == 4 and differ == 0 and st["rays_closest"] == st_c["rays_closest"] and whole[..., 1].mean() > 1e-3


def test_counters_and_timers(scenes, orc):
    res, (b, rays) = wc.reference(orc, "glass", 5, 4)
    h = scenes(orc, "glass", 4)
    _, _, st = h.render_rays_whitted(rays, max_depth=5)
    _, _, sc = h.render_rays_whitted(rays, max_depth=5, count_traversal=True)
    _, _, tk = h.render_rays_whitted(rays, max_depth=5, time_kernels=True)
    print(f"\nWhitted counters: rays {sc['rays_closest']} / {sc['rays_shadow']}, nodes {sc['nodes_closest']} / {sc['nodes_shadow']}, tris {sc['tris_closest']} / {sc['tris_shadow']}; "
          f"ms closest {tk['ms_trace_closest']:.3f} any {tk['ms_trace_any']:.3f} vertex {tk['ms_shade']:.3f}; launches {st['launches_trace_path']} / {st['launches_shade']} / {st['launches_trace_shadow']}")
    assert (sc["rays_closest"], sc["rays_shadow"]) == (st["rays_closest"], st["rays_shadow"]) and st["rays_mis"] == 0
    assert min(sc["nodes_closest"], sc["nodes_shadow"], sc["tris_closest"]) > 0
    assert min(tk["ms_trace_closest"], tk["ms_trace_any"], tk["ms_shade"]) > 0
