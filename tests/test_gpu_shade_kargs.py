"""Frames of a Lambert-only scene with its records in LDS (the Cornell box) through the shade kernels that re-read their arguments from the kernarg segment at every
vertex (k_shade_split<1>, k_shade_split<2>, k_shade<1, .., 1>: RT_SHADE_KARGS) against the same frame through the control kernels that keep the
arguments live (RTX_SHADE_KARGS=0, read per render call: k_shade_split_live, k_shade_const_live): the film bit for bit and every integer field of the stats. The
shapes of tests/test_gpu_shade_split.py: a pass that is no multiple of 64 or 256 entries, depth limits 0 and 1, both counting frames, a cropped pass (bounce 0
through k_shade<1, .., 1>, the later bounces through k_shade_split<2>) and a progressive frame in two steps."""
import ctypes
import os

import numpy as np
import pytest

from rustracer_amd.scenes import cornell_box

pytestmark = pytest.mark.gpu
KNOB = "RTX_SHADE_KARGS"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _off_then_on(fn):
    """fn() with the knob at 0 (the control kernels), then with the knob unset."""
    saved = os.environ.pop(KNOB, None)
    try:
        os.environ[KNOB] = "0"
        off = fn()
        del os.environ[KNOB]
        on = fn()
    finally:
        os.environ.pop(KNOB, None)
        if saved is not None:
            os.environ[KNOB] = saved
    return off, on


def _int_fields(host):
    return [n for n, t in host.Stats._fields_ if t is ctypes.c_uint64]


def _assert_same(host, off, on):
    (film0, st0), (film1, st1) = off, on
    assert np.array_equal(bits(film0), bits(film1))
    for k in _int_fields(host):
        assert st0[k] == st1[k], (k, st0[k], st1[k])
    assert st0["shade_section_cycles"] == st1["shade_section_cycles"]
    return st1


@pytest.mark.parametrize("res,spp", [((33, 17), 5), ((96, 80), 16)])
def test_frame_is_the_same_through_either_form(gpu_host, res, spp):
    h = gpu_host.HostScene(cornell_box(res[0], res[1], spp))
    st = _assert_same(gpu_host, *_off_then_on(h.render))
    assert st["camera_rays"] % (res[0] * res[1]) == 0 and st["camera_rays"] >= res[0] * res[1] * spp  # (the sampler rounds spp up to a power of two)
    assert st["vertices_lambert_const"] > st["camera_rays"]
    assert st["launches_shade"] > 0 and st["rays_tail_not_cast"] > 0


def test_frame_is_the_same_without_the_split_kernels(gpu_host, monkeypatch):
    """RTX_SHADE_SPLIT=0: every bounce through k_shade<1, .., 1> / k_shade_const_live<1>"""
    monkeypatch.setenv("RTX_SHADE_SPLIT", "0")
    h = gpu_host.HostScene(cornell_box(33, 17, 5))
    st = _assert_same(gpu_host, *_off_then_on(h.render))
    assert st["vertices_lambert_const"] > st["camera_rays"]


@pytest.mark.parametrize("as_rendered", [False, True])
def test_counting_frame_is_the_same_through_either_form(gpu_host, as_rendered):
    h = gpu_host.HostScene(cornell_box(96, 80, 16))
    st = _assert_same(gpu_host, *_off_then_on(lambda: h.render(count_traversal=True, count_as_rendered=as_rendered)))
    assert st["nodes_closest"] > 0 and st["tris_closest"] > 0
    assert (st["rays_tail_not_cast"] > 0) == as_rendered


@pytest.mark.parametrize("max_depth", [0, 1])
def test_depth_limits_end_the_camera_vertices(gpu_host, max_depth):
    h = gpu_host.HostScene(cornell_box(33, 17, 5, max_depth=max_depth))
    st = _assert_same(gpu_host, *_off_then_on(h.render))
    n = st["camera_rays"]
    assert n % (33 * 17) == 0 and n >= 33 * 17 * 5 and n % 256 != 0  # (spp rounded up to a power of two; the pass is no multiple of a workgroup)
    if max_depth == 0:  # no vertex continues: nothing is cast or left uncast past the camera rays
        assert st["rays_closest"] == n and st["rays_tail_not_cast"] == 0 and st["rays_shadow"] == 0
    else:  # every camera vertex that samples a direction ends at the limit: its ray is the tail that is not cast
        assert st["rays_tail_not_cast"] > 0 and st["rays_closest"] == n + st["rays_tail_not_cast"]


def test_cropped_pass(gpu_host):
    d = cornell_box(33, 17, 5)
    d.integrator.pixel_bounds = (5, 29, 3, 15)  # samples outside the bounds: bounce 0 has a queue (k_shade<1, .., 1>), the later bounces run k_shade_split<2>
    h = gpu_host.HostScene(d)
    st = _assert_same(gpu_host, *_off_then_on(h.render))
    assert 0 < st["camera_rays"] < 33 * 17 * 5 and st["camera_rays"] % (24 * 12) == 0 and st["vertices_lambert_const"] > st["camera_rays"]


def test_progressive_frame_in_two_steps(gpu_host):
    h = gpu_host.HostScene(cornell_box(33, 17, 5))

    def run():
        with h.progressive() as fr:
            s1 = fr.advance(3)
            s2 = fr.advance(fr.spp - 3)
            return fr.film(), {k: s1[k] + s2[k] for k in _int_fields(gpu_host)} | {"shade_section_cycles": s2["shade_section_cycles"]}

    off, on = _off_then_on(run)
    _assert_same(gpu_host, off, on)
    whole, _ = h.render()
    assert np.array_equal(bits(on[0]), bits(whole))
