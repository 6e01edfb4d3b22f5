"""Direct lighting of every kind of light on the HIP path, held to the float64 radiometric model of tests/radiometry_model.py - not to the oracle.

HostScene.render_rays with every sample of a "pixel" on the same ray makes that pixel one receiver point x; on a Lambertian receiver with max_depth = 1 every
sample's expectation is rho / pi * E(x), whichever light was picked, whichever half of the MIS estimator found it and whichever shade front end ran. The cases,
their points and rays are tests/radiometry_cases.py's (tests/test_radiometry_model_cpu.py holds the oracle to the same model on them and checks their layout);
the statistic and its noise caps are radiometry_model.statistic's: per point |m - M| <= 5 se + 1e-4 M, pooled |sum m - sum M| <= 5 sqrt(sum se^2) + 1e-4 sum M,
and the samples must be quiet enough to judge (pooled se <= 0.002 sum M, se_p <= 0.03 M_p). Points whose irradiance is 0 - behind a one-sided emitter, in an
occluder's umbra, facing away from a point or distant light - must be 0.0 in every sample. Every case prints its record before it asserts."""
import numpy as np
import pytest

import radiometry_cases as rc
import radiometry_model as rm

pytestmark = pytest.mark.gpu

RT_QUERY_SHADOW_EMPTY = 4     # include/rtx_hip.h
N = rc.N_SAMPLES


def render(gpu_host, c):
    h = gpu_host.HostScene(c.desc)
    h.upload(0)
    rad, st = h.render_rays(c.rays(N), spp=N, max_depth=1)
    assert rad.shape == (1, c.x.shape[0], N, 4) and st["camera_rays"] == c.x.shape[0] * N
    return h, rad[0], st


def judge(c, rad, who):
    m = rc.model_radiance(c)
    assert np.all(rad[..., 3] == 0.0), "a sample carries the scrub flag (or was not traced)"
    assert np.all(np.isfinite(rad))
    st = rm.statistic(rad[..., 1], m[:, 1], c.extra)
    print("\n" + rm.line("device", who, st))
    dark = (m.max(axis=1) == 0) & (True if c.extra is None else c.extra == 0)
    assert np.all(rad[dark][..., :3] == 0.0), f"{who}: {int((rad[dark][..., :3] != 0).sum())} non-zero values at points no light reaches"
    rm.require(st, who)
    return st


def routed(st, name, front_end):
    """The case's vertices all went through the front end's kernel: its counter of rt_stats, and no other."""
    counts = {k: int(st[k]) for k in rc.VERTEX_COUNTERS}
    print(f"vertices {counts}")
    want = rc.counter(name, front_end)
    assert counts[want] > 0 and all(v == 0 for k, v in counts.items() if k != want), (name, front_end, counts)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_direct_lighting_against_the_model(gpu_host, name):
    c = rc.case(name)
    h, rad, st = render(gpu_host, c)
    print(f"\n{name}: lds resident {h.lds_resident()}, shadow rays {st['rays_shadow']} ({st['rays_shadow_not_cast']} not cast), MIS rays {st['rays_mis']}")
    routed(st, name, "const")
    if name == "two_triangles_occluder":   # the shadow sets answer part of the segments, the any-hit walk the rest
        empty = h.scene_query(RT_QUERY_SHADOW_EMPTY)
        print(f"EMPTY shadow-set pairs {empty}")
        assert h.lds_resident() and empty > 0 and 0 < st["rays_shadow_not_cast"] < st["rays_shadow"]
    judge(c, rad, name)


@pytest.mark.parametrize("front_end", rc.FRONT_ENDS)
@pytest.mark.parametrize("name", list(rc.FRONT_END_CASES))
def test_every_shade_front_end(gpu_host, name, front_end):
    """The same light code is instantiated in each shade kernel: a triangle emitter, a sphere (cone sampling) and the mapped environment under each of five
    receiver materials whose BSDF is rho / pi."""
    c = rc.FRONT_END_CASES[name](front_end)
    h, rad, st = render(gpu_host, c)
    routed(st, name, front_end)
    judge(c, rad, f"{name}/{front_end}")
    # the material is what the case says: f = rho / pi, from the kernel form the front end stands for (two-lobe: 5, its wide form: 6; Lambert: 3; generic: 0)
    f = h.bsdf_eval(c.mat, [(0.3, 0.2, 0.9327)], [(-0.5, 0.1, 0.8602)], [(0.3, 0.7)])["f"][0]
    form = (h.scene_query(gpu_host.RT_QUERY_BSDF_LAUNCHED) - 1) // 2
    print(f"bsdf_eval f {f}, kernel form {form}")
    assert np.allclose(f, c.rho / np.pi, rtol=1e-5)
    assert form == dict(const=3, image=3, plastic=5, uber=6, mix=0)[front_end]


@pytest.mark.parametrize("receiver", ["disk", "instance"])
def test_other_receivers(gpu_host, receiver):
    """The triangle-emitter case with the floor as a disk quadric, and inside a rotated object instance: neither scene is LDS-resident, other trace kernels answer."""
    c = rc.quad_case(receiver=receiver)
    h, rad, st = render(gpu_host, c)
    assert not h.lds_resident()
    routed(st, c.name, "const")
    judge(c, rad, c.name)


@pytest.mark.parametrize("name", ["quad", "quad_two_sided", "quad_reversed", "quad_normals", "quad_overhead", "sphere_outside", "sphere_inside", "disk_tilted", "disk_overhead", "cylinder"])
def test_emitters_seen_directly(gpu_host, name):
    """max_depth = 0: a ray that meets an emitter on its emitting side returns exactly Le, on the other side exactly 0 (Le if two-sided)."""
    c = rc.case(name)
    assert len(c.probes) >= 4
    rays = np.zeros((1, len(c.probes), 1, 8), np.float32)
    for k, (o, d, _) in enumerate(c.probes):
        rays[0, k, 0, 0:3], rays[0, k, 0, 3], rays[0, k, 0, 4:7] = o, np.inf, d
    h = gpu_host.HostScene(c.desc)
    h.upload(0)
    rad, _ = h.render_rays(rays, max_depth=0)
    want = np.float32([le for _, _, le in c.probes])
    print(f"\n{name}: {len(c.probes)} rays, {int((want.max(axis=1) > 0).sum())} expect Le; got {rad[0, :, 0, :3].tolist()}")
    assert (want.max(axis=1) > 0).any() and np.array_equal(rad[0, :, 0, :3], want) and np.all(rad[..., 3] == 0.0)


def test_escaping_rays_see_the_map(gpu_host):
    """max_depth = 0 under the mapped environment: a ray that escapes returns the level-0 bilinear value of the map, to 1e-5.
    Directions: two per cell between texel centres, over the whole map but for the cells that touch the sun's edge: there the interpolant climbs a thousandfold
    within a texel and float32's 2^-23 of phi * 16 is more than 1e-5 of the value at the foot of the ramp. The cell inside the sun is among the directions."""
    c = rc.case("env_map")
    env = c.lights[0]
    st_uv = [((cx + 0.5 + fu) / 16.0, (cy + 0.5 + fv) / 8.0) for cy in range(0, 7) for cx in range(16) for fu, fv in ((0.3, 0.6), (0.8, 0.15))
             if not (4 <= cx <= 6 and 1 <= cy <= 3) or (cx, cy) == (5, 2)]
    u, v = np.array(st_uv).T
    th, ph = np.pi * v, 2.0 * np.pi * u
    w = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=-1) @ env.rot.T
    want = env.radiance(w)
    rays = np.zeros((1, w.shape[0], 1, 8), np.float32)
    rays[0, :, 0, 0:3], rays[0, :, 0, 3], rays[0, :, 0, 4:7] = np.where(w[:, 1:2] > 0, (0.0, 3.0, 0.0), (0.0, -3.0, 0.0)), np.inf, w   # away from the pyramid
    h = gpu_host.HostScene(c.desc)
    h.upload(0)
    rad, _ = h.render_rays(rays, max_depth=0)
    got = rad[0, :, 0, :3].astype(np.float64)
    worst = float(np.abs(got / want - 1.0).max())
    print(f"\nENV {w.shape[0]} escaping rays, values {want.min():.3f} .. {want.max():.1f}: largest relative difference from the bilinear value {worst:.2e}")
    assert want.max() > 500.0 and np.all(rad[..., 3] == 0.0)
    assert worst <= 1e-5
