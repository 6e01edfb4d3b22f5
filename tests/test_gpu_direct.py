"""rt_render_rays_direct / rt_render_direct on the GPU (HostScene.render_rays_direct, HostScene.render_direct) held to the float64 model of tests/direct_model.py: EVERY
sample of every batch - 40 x 24 pixels x 4 samples = 3840 rays, 15 workgroups of the vertex kernel, the last one partial - under both light strategies: its status, its four
info words (li invocations, get_2d() draws, get_1d() draws, vertices that reached uniform_sample_all_light) exactly, and its radiance. Legitimate because the batches keep
their distance from every decision float32 could take differently (tests/direct_cases.py; tests/test_direct_cpu.py asserts the margins of the model alone). Every measured
figure is printed before it is asserted.

Tolerances on L, per sample and channel, |L - model| <= RTOL * max(model over the batch) + RTOL * |model|: tests/test_gpu_whitted.py's, unchanged - 2e-4 on the flat scenes
(floor, area, mix, many, and the slab alone), 3e-3 through the curved glass of `glass`; their derivations hold for the tree, which is Whitted's. What estimate_direct adds:
  the MIS weight. A light-half term is f li |cos| w / p with w = p^2 / (p^2 + q^2), p the light's pdf and q the BSDF's: d ln(w / p) / d ln p = (q^2 - p^2) / (p^2 + q^2),
    within [-1, 1], and d ln(w / p) / d ln q = -2 q^2 / (p^2 + q^2), within [-2, 0]. The BSDF-half term f |cos| le w' / q with w' = q^2 / (p^2 + q^2) has the same two
    bounds with p and q exchanged. So the weight passes p's relative error on at most once - as the unweighted 1 / p of Whitted's term does - and q's at most twice;
    q = |cos| / pi at the surface, whose absolute error is the direction's (~1e-5) while the term itself carries the factor |cos|: 2e-5 of the term at normal incidence,
    no more in absolute terms at grazing incidence. Nothing is widened for it.
  the emitter's cosine. p = r^2 / (|cos_l| area): the relative error of 1 / |cos_l| is the direction's error over |cos_l|. The cases keep |cos_l| >= 0.1 at every live
    light sample, pdf_li hit and probe hit (`grazing`, direct_cases.GRAZING): 1e-5 / 0.1 = 1e-4, half of the flat scenes' 2e-4 and inside it together with the 1e-5 of
    the distances. Whitted's light term divides by the same pdf; its cases did not bound the cosine, these do.
No tolerance is wider than Whitted's."""
import numpy as np
import pytest

import direct_cases as dc
from util import bits

pytestmark = pytest.mark.gpu

RTOL = dict(many=2e-4, floor=2e-4, area=2e-4, mix=2e-4, glass=3e-3, glass_triangles=2e-4)
N = dc.H * dc.W * dc.NS


@pytest.fixture(scope="module")
def scenes(gpu_host):
    """One uploaded HostScene per (case, dimensions), made on first use."""
    made = {}

    def get(orc, name, dims):
        if (name, dims) not in made:
            b, _ = dc.settled(orc, name)
            h = gpu_host.HostScene(b.desc(dims))
            h.upload(0)
            made[(name, dims)] = h
        return made[(name, dims)]
    return get


def _launches(b, res, sname):
    """(closest-hit launches of the walk, vertex launches, any-hit launches, probe launches) of a run: a step per node of the deepest tree; per step, under "all" a
    round per light (one at the least), an any-hit launch per light and a probe launch per non-delta light; under "one" one round, one any-hit launch if the scene lists
    a light, one probe launch if it lists a non-delta one."""
    steps = int(res.nodes.max())
    lights = b.model.lights
    area = sum(1 for l in lights if l[0] not in ("point", "distant"))
    if sname == "all":
        return steps, steps * max(len(lights), 1), steps * len(lights), steps * area
    return steps, steps, steps * min(len(lights), 1), steps * min(area, 1)


def _compare(tag, name, sname, L, info, st, res, rays, b):
    L, info = L.reshape(N, 4), info.reshape(N, 4).astype(np.int64)
    active = rays.reshape(N, 8)[:, 3] > 0
    want, winfo = res.L, res.info()
    scale = np.abs(want).max()
    err = np.abs(L[:, :3].astype(np.float64) - want)
    bound = RTOL[name] * scale + RTOL[name] * np.abs(want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    diffs = [int((info[:, k] != winfo[:, k]).sum()) for k in range(4)]
    print(f"\n{tag}: nodes up to {res.nodes.max()}, get_2d up to {res.draws.max()}, get_1d up to {res.draws1.max()}, array vertices up to {res.verts.max()} (info words differ: {diffs}), "
          f"max |L| {scale:.4g}, lit samples {(want.sum(1) > 0).mean():.2f}, worst error / bound {worst:.3f} (max abs error {err.max():.3e}), status {np.unique(L[:, 3])}; "
          f"rays {st['camera_rays']} / {st['rays_closest']} / {st['rays_shadow']} / {st['rays_mis']} (model {int(res.nodes.sum())} / {res.n_shadow} / {res.n_probe}), "
          f"launches {st['launches_trace_path']} / {st['launches_shade']} / {st['launches_trace_shadow']} / {st['launches_trace_mis']}")
    assert np.array_equal(L[:, 3], np.where(active, 0.0, 2.0).astype(np.float32))
    assert diffs == [0, 0, 0, 0]
    assert not info[~active].any() and not L[~active, :3].any()
    assert worst <= 1.0
    assert st["camera_rays"] == int(active.sum()) and st["rays_closest"] == int(res.nodes.sum()) and st["paths_scrubbed"] == 0
    assert st["rays_shadow"] == res.n_shadow and st["rays_mis"] == res.n_probe
    assert (st["launches_trace_path"], st["launches_shade"], st["launches_trace_shadow"], st["launches_trace_mis"]) == _launches(b, res, sname)


RUN_IDS = [(name, md, dims, sname) for name in dc.CASES for md, dims in dc.RUNS[name] for sname, _ in dc.STRATEGIES]


@pytest.mark.parametrize("name,max_depth,dims,sname", RUN_IDS, ids=[f"{n}-d{m}-dims{d}-{s}" for n, m, d, s in RUN_IDS])
def test_every_sample_against_the_model(scenes, orc, name, max_depth, dims, sname):
    """The cases of tests/direct_cases.py under "all" and "one": a matte floor under a point light with misses and skipped rays (a delta light: no probe, its arrays
    consumed); floor, wall and blocker under a two-triangle emitter with every draw from the stream (dimensions 2) and the first from the tables (8); Whitted's glass scene
    under the area light (GENERAL kernel; trees that exhaust the arrays beside single vertices that do not) and the slab alone (plain kernel); a mix of matte and mirror
    under a point and an infinite light (probes that leave the scene); 48 lights, 288 arrays."""
    res, (b, rays) = dc.reference(orc, name, max_depth, dims, sname)
    h = scenes(orc, name, dims)
    L, info, st = h.render_rays_direct(rays, max_depth=max_depth, strategy=sname, with_info=True)
    _compare(f"direct {name} max_depth {max_depth} dimensions {dims} strategy {sname}", name, sname, L, info, st, res, rays, b)
    general = h.scene_query(9)
    print(f"kernel launched: {general} (1 plain, 2 GENERAL)")
    assert general == (2 if name == "glass" else 1)


def _plastic_scene(gpu_host):
    """Quads of plastic, disney and substrate - no specular lobe anywhere, none of them in the model - over a matte floor, one point light."""
    from rustracer_amd.scene_desc import SceneDesc
    s = SceneDesc()
    s.film.xres, s.film.yres = 32, 32
    s.film.filter_kind, s.film.filter_params = 0, (0.5, 0.5, 0.0, 0.0)
    s.sampler.spp, s.sampler.dims = 4, 4
    s.camera.pos, s.camera.look, s.camera.fov = (0.0, 2.5, -5.0), (0.0, 0.2, 0.0), 45.0
    s.add_quad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6), s.matte((0.6, 0.6, 0.6)))
    mats = [s.plastic((0.3, 0.5, 0.2), (0.4, 0.4, 0.4), 0.15), s.disney(color=(0.7, 0.3, 0.2), roughness=0.4, metallic=0.3), s.substrate((0.4, 0.3, 0.5), (0.3, 0.3, 0.3), 0.2, 0.1)]
    for k, m in enumerate(mats):
        x = -2.4 + 1.8 * k
        s.add_quad((x, 0.4, -1.0), (x, 0.6, 1.0), (x + 1.4, 0.6, 1.0), (x + 1.4, 0.4, -1.0), m)
    s.point_light((0.5, 4.0, -2.0), (120.0, 110.0, 100.0))
    h = gpu_host.HostScene(s)
    h.upload(0)
    return h


def test_one_light_at_depth_one_is_the_path_integrator_at_depth_one(gpu_host):
    """Materials the model does not have (plastic, disney, substrate: no specular lobe), one point light, max_depth 1, strategy "one": Le + uniform_sample_one_light is
    what PathIntegrator::li returns at max_depth 1 with one light, from the same draws (get_1d for the pick, then u_light, u_scattering). rt_render_rays_direct against
    rt_render_rays on the same records: within 1e-5 of the largest L, test_gpu_whitted.py's bound for the same comparison."""
    h = _plastic_scene(gpu_host)
    cam, _ = h.camera_rays()
    d1, info, st = h.render_rays_direct(cam, max_depth=1, strategy="one", with_info=True)
    p1, _ = h.render_rays(cam, max_depth=1)
    top = float(p1[..., :3].max())
    diff = float(np.abs(d1[..., :3].astype(np.float64) - p1[..., :3]).max())
    print(f"\ndirect 'one' at max_depth 1 against rt_render_rays: max abs difference {diff:.3e} of max {top:.4f}; get_1d draws {np.unique(info[..., 2])}, get_2d draws {np.unique(info[..., 1])}, "
          f"rays {st['rays_closest']} / {st['rays_shadow']} / {st['rays_mis']}")
    assert top > 0.05 and diff <= 1e-5 * top and not d1[..., 3].any() and st["rays_mis"] == 0


def test_sample_ranges_add_up_bit_for_bit_and_device_buffers(scenes, orc):
    """Calls over [0, 1) + [1, 4) give the call over [0, 4) bit for bit - radiance and info - and so do the call on device pointers and a second call."""
    import torch
    _, (b, rays) = dc.reference(orc, "glass", 5, 4, "all")
    h = scenes(orc, "glass", 4)
    kw = dict(max_depth=5, strategy="all", with_info=True)
    L, info, _ = h.render_rays_direct(rays, **kw)
    La, ia, _ = h.render_rays_direct(rays[:, :, :1], sample0=0, **kw)
    Lb, ib, _ = h.render_rays_direct(rays[:, :, 1:], sample0=1, **kw)
    d1 = int((bits(np.concatenate([La, Lb], axis=2)) != bits(L)).sum()) + int((np.concatenate([ia, ib], axis=2) != info).sum())
    dev_rays = torch.from_numpy(rays).cuda()
    out, inf = torch.zeros((dc.H, dc.W, dc.NS, 4), dtype=torch.float32, device="cuda"), torch.zeros((dc.H, dc.W, dc.NS, 4), dtype=torch.int32, device="cuda")
    h.render_rays_direct(dev_rays, device_out=out, device_info_out=inf, **kw)
    torch.cuda.synchronize()
    d2 = int((bits(out.cpu().numpy()) != bits(L)).sum()) + int((inf.cpu().numpy().astype(np.uint32) != info).sum())
    again, _, _ = h.render_rays_direct(rays, max_depth=5, strategy="all")
    d3 = int((bits(again) != bits(L)).sum())
    print(f"\ndirect ranges: [0, 1) + [1, 4) differs from [0, 4) in {d1} words, the device-pointer call in {d2}, a second call in {d3}")
    assert d1 == 0 and d2 == 0 and d3 == 0


def _frame_scene(gpu_host, orc, gaussian, res=32, spp=4):
    from rustracer_amd.scene_desc import FILTER_GAUSSIAN
    b, _ = dc.settled(orc, "glass")
    d = b.desc(4)
    d.film.xres, d.film.yres, d.sampler.spp = res, res, spp
    d.film.filter_kind, d.film.filter_params = (FILTER_GAUSSIAN, (1.5, 1.5, 2.0, 0.0)) if gaussian else (0, (0.5, 0.5, 0.0, 0.0))
    h = gpu_host.HostScene(d)
    h.upload(0)
    return h


@pytest.mark.parametrize("sname", ["all", "one"])
def test_frame_is_the_splat_of_the_ray_entrys_samples(gpu_host, orc, sname):
    """rt_render_direct, 32 x 32 x 4 spp under a Gaussian of radius 1.5, against rt_render_rays_direct over rt_camera_rays' records splatted by the reference's
    FilmTile::add_sample in float64 (1e-6: the film kernel's float32 sums of up to 36 samples per pixel), and equal ray counts."""
    from test_gpu_whitted import _splat_rgb
    h = _frame_scene(gpu_host, orc, True)
    film, st = h.render_direct(5, sname)
    setup = h.setup()
    cam_rays, pf = h.camera_rays()
    L, _, st_r = h.render_rays_direct(cam_rays, max_depth=5, strategy=sname)
    want = _splat_rgb(L[..., :3], pf, setup["filter_table"].astype(np.float32), 1.5, 1.5, [int(v) for v in setup["cropped"]])
    err = float(np.linalg.norm(film.astype(np.float64) - want) / np.linalg.norm(want))
    keys = ("camera_rays", "rays_closest", "rays_shadow", "rays_mis")
    print(f"\ndirect '{sname}' frame vs splat of rt_render_rays_direct over rt_camera_rays' records: relative L2 {err:.3e}; film mean Y {film[..., 1].mean():.4f}, "
          f"rays {[st[k] for k in keys]} vs {[st_r[k] for k in keys]}")
    assert film.shape == (32, 32, 4) and err <= 1e-6 and film[..., 1].mean() > 1e-3
    assert [st[k] for k in keys] == [st_r[k] for k in keys] and st["rays_mis"] > 0


def test_two_shards_merge_and_the_other_integrators_are_untouched(gpu_host, orc):
    """Under the box filter films compare bit for bit: rank 0 + rank 1 of two is the unsharded frame; rt_render and rt_render_whitted before and after a direct-lighting
    frame are the same bytes."""
    from rustracer_amd.distributed import touched_rows
    h = _frame_scene(gpu_host, orc, False)
    before, wbefore = h.render()[0], h.render_whitted(5)[0]
    whole, _ = h.render_direct(5)
    parts = [h.render_direct(5, rank=r, world_size=2)[0] for r in range(2)]
    one, _ = h.render_direct(5, "one")
    after, wafter = h.render()[0], h.render_whitted(5)[0]
    st = h.setup()
    rows = touched_rows([int(v) for v in st["cropped"]], [int(v) for v in st["sample_bounds"]], 1, 2, 0.5)
    merged = parts[0].copy()
    merged[rows] += parts[1][rows]
    differ, path_differ, whitted_differ = int((bits(merged) != bits(whole)).sum()), int((bits(before) != bits(after)).sum()), int((bits(wbefore) != bits(wafter)).sum())
    print(f"\ndirect shards: merged film differs from the unsharded one in {differ} words; rt_render before / after differs in {path_differ}, rt_render_whitted in {whitted_differ}; "
          f"rank films non-zero: {[bool(p.any()) for p in parts]}; mean Y all {whole[..., 1].mean():.4f}, one {one[..., 1].mean():.4f}, whitted {wbefore[..., 1].mean():.4f}")
    assert differ == 0 and path_differ == 0 and whitted_differ == 0 and all(p.any() for p in parts)
    assert not np.array_equal(whole[..., :3], wbefore[..., :3]) and not np.array_equal(whole[..., :3], one[..., :3])


def test_a_small_table_budget_cuts_the_frame_in_batches_and_changes_no_bit(gpu_host, orc, monkeypatch):
    """64 x 64 x 16 spp at max_depth 5 with two lights: 20 arrays, 800 B of array tables per pixel, 3.1 MiB for the frame's 4096 pixels - one batch. With a budget of
    800 KiB (RTX_DIRECT_TABLE_BUDGET) the batch is halved twice, to 1024 pixels: four batches, and the box-filtered film is the same, bit for bit."""
    h = _frame_scene(gpu_host, orc, False, res=64, spp=16)
    whole, st = h.render_direct(5)
    monkeypatch.setenv("RTX_DIRECT_TABLE_BUDGET", str(800 << 10))
    cut, st_c = h.render_direct(5)
    differ = int((bits(cut) != bits(whole)).sum())
    keys = ("rays_closest", "rays_shadow", "rays_mis")
    print(f"\ndirect table budget: passes {st['n_passes']} -> {st_c['n_passes']}, films differ in {differ} words, rays {[st[k] for k in keys]} / {[st_c[k] for k in keys]}")
    assert st["n_passes"] == 1 and st_c["n_passes"] >= 4 and differ == 0 and [st[k] for k in keys] == [st_c[k] for k in keys] and whole[..., 1].mean() > 1e-3


def test_counters_and_timers(scenes, orc):
    _, (b, rays) = dc.reference(orc, "glass", 5, 4, "all")
    h = scenes(orc, "glass", 4)
    _, _, st = h.render_rays_direct(rays, max_depth=5)
    _, _, sc = h.render_rays_direct(rays, max_depth=5, count_traversal=True)
    _, _, tk = h.render_rays_direct(rays, max_depth=5, time_kernels=True)
    print(f"\ndirect counters: rays {sc['rays_closest']} / {sc['rays_shadow']} / {sc['rays_mis']}, nodes {sc['nodes_closest']} / {sc['nodes_shadow']} / {sc['nodes_mis']}, "
          f"tris {sc['tris_closest']} / {sc['tris_shadow']}; ms closest {tk['ms_trace_closest']:.3f} any {tk['ms_trace_any']:.3f} mis {tk['ms_trace_mis']:.3f} vertex + arrays {tk['ms_shade']:.3f} "
          f"probe {tk['ms_resolve']:.3f}")
    assert (sc["rays_closest"], sc["rays_shadow"], sc["rays_mis"]) == (st["rays_closest"], st["rays_shadow"], st["rays_mis"]) and st["rays_mis"] > 0
    assert min(sc["nodes_closest"], sc["nodes_shadow"], sc["nodes_mis"], sc["tris_closest"]) > 0
    assert min(tk["ms_trace_closest"], tk["ms_trace_any"], tk["ms_trace_mis"], tk["ms_shade"], tk["ms_resolve"]) > 0
