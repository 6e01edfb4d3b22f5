"""Shadow sets on the device: the film and the ray counts of a frame are the same with RTX_SHADOW_SETS=0 and 1, the segments the
sets answer are counted in rays_shadow_not_cast, and both the oracle's intersect_p and the reference walk (rt_trace_any) find every segment of an EMPTY pair
unoccluded - segments built with the product's rt_offset_ray_origin, on S1 and on random rooms and soups (tests/test_shadow_sets_cpu.py's generators)."""
import os

import numpy as np
import pytest

from rustracer_amd import host
from rustracer_amd.scenes import cornell_box

from oracle import orc
from test_shadow_sets_cpu import F, SHIFTS, classify, random_room, random_soup_lit, segments, voxel_of

pytestmark = pytest.mark.gpu


def render(desc, sets, count=False):
    old = os.environ.get("RTX_SHADOW_SETS")
    os.environ["RTX_SHADOW_SETS"] = "1" if sets else "0"
    try:
        h = host.HostScene(desc)
        h.upload(0)
        a, st_a = h.render(count_traversal=count)
        b, st_b = h.render(count_traversal=count)
        return h, a, b, st_a, st_b
    finally:
        if old is None:
            del os.environ["RTX_SHADOW_SETS"]
        else:
            os.environ["RTX_SHADOW_SETS"] = old


@pytest.mark.parametrize("res, spp", [(400, 64), (256, 16)])
def test_film_and_rays_equal_with_and_without_sets(res, spp):
    d = cornell_box(res, res, spp)
    h1, a1, b1, st1, _ = render(d, True)
    h0, a0, b0, st0, _ = render(d, False)
    assert np.array_equal(a1, b1) and np.array_equal(a0, b0), "a frame is not reproducible with itself"
    assert np.array_equal(a1, a0), f"{int(np.sum(a1 != a0))} film values differ"
    assert h1.scene_query(4) > 0 and h0.scene_query(4) == 0
    for k in ("camera_rays", "rays_closest", "rays_shadow", "rays_mis"):
        assert st1[k] == st0[k], (k, st1[k], st0[k])
    assert st0["rays_shadow_not_cast"] == 0
    assert 0.2 * st1["rays_shadow"] < st1["rays_shadow_not_cast"] < st1["rays_shadow"], (st1["rays_shadow_not_cast"], st1["rays_shadow"])


def test_counting_frames_walk_every_segment():
    d = cornell_box(64, 64, 16)
    _, _, _, st1, _ = render(d, True, count=True)
    _, _, _, st0, _ = render(d, False, count=True)
    assert st1["rays_shadow_not_cast"] == 0
    for k in ("rays_shadow", "nodes_shadow", "tris_shadow", "nodes_closest", "tris_closest"):
        assert st1[k] == st0[k], (k, st1[k], st0[k])


def test_reference_walk_agrees_on_empty_segments():
    d = cornell_box(64, 64, 16)
    h = host.HostScene(d)
    h.upload(0)
    ss = h.shadow_sets()
    b = h.bvh()["bounds"][0]
    rays, li, p = segments(d, 100_000, seed=7)
    vx, vy, vz = voxel_of(p, b[:3].astype(F), b[3:].astype(F), ss["nvox"])
    empty = ss["kind"][vz, vy, vx, li] == 1
    assert empty.mean() > 0.2
    r = h.trace(rays, any_hit=True)
    occ = np.asarray(r["occluded"]).astype(bool)
    assert not np.any(occ & empty)


@pytest.mark.parametrize("make, seed", [(random_room, 0), (random_room, 1), (random_room, 3), (random_room, 7), (random_soup_lit, 0), (random_soup_lit, 2)])
def test_random_scenes_with_device_offsets(make, seed):
    d = make((100 if make is random_room else 200) + seed, SHIFTS[seed % 4])
    rays, li, p = segments(d, 100_000, seed=seed, offset=host.offset_ray_origin)
    kind, _ = classify(d, rays, li, p)
    empty = kind == 1
    assert not np.any(orc.OracleScene(d).trace(rays, any_hit=True)["occluded"] & empty)
    h = host.HostScene(d)
    h.upload(0)
    assert not np.any(np.asarray(h.trace(rays, any_hit=True)["occluded"]).astype(bool) & empty)


@pytest.mark.parametrize("seed", [0, 7])
def test_random_room_film_equal_with_and_without_sets(seed):
    d = random_room(100 + seed, SHIFTS[seed % 4])
    d.film.xres, d.film.yres, d.sampler.spp = 64, 64, 16
    h1, a1, b1, st1, _ = render(d, True)
    h0, a0, b0, st0, _ = render(d, False)
    assert np.array_equal(a1, b1) and np.array_equal(a0, b0), "a frame is not reproducible with itself"
    assert np.array_equal(a1, a0), f"{int(np.sum(a1 != a0))} film values differ"
    assert h1.scene_query(4) > 0 and st1["rays_shadow_not_cast"] > 0
    for k in ("camera_rays", "rays_closest", "rays_shadow", "rays_mis"):
        assert st1[k] == st0[k], (k, st1[k], st0[k])


def test_multi_render_reports_uncast_segments():
    d = cornell_box(128, 128, 16)
    h = host.HostScene(d)
    h.upload(0)
    _, st = h.render()
    _, total, per = h.render_multi([0], chunks_per_device=2)
    assert total["rays_shadow_not_cast"] == per[0]["rays_shadow_not_cast"] == st["rays_shadow_not_cast"] > 0
    assert total["rays_shadow"] == st["rays_shadow"]
