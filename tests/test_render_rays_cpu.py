"""rt_render_rays (path-traced radiance along caller-supplied rays) without a GPU: the prototype is declared with the arity and types the issue names, exported from
both libraries, spelled out for the Rust binding and wrapped by HostScene.render_rays; RT_RAYS_MAX agrees between header and Python; every refusal answers
RT_ERR_INVALID with a message before any device work (the scene pointer is a dummy that is never dereferenced); the numpy cameras of rustracer_amd/cameras.py make
the rays pbrt-v3 defines."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_abi_cpu import parse_c_prototypes, parse_rust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1
RT_FLAG_REF_STREAM = 16


class SamplerDesc(C.Structure):
    _fields_ = [("spp", C.c_int32), ("dimensions", C.c_int32)]


class PathDesc(C.Structure):
    _fields_ = [("max_depth", C.c_int32), ("rr_threshold", C.c_float), ("light_strategy", C.c_int32), ("pixel_bounds", C.c_int32 * 4)]


def test_prototype_is_declared_exported_documented_and_wrapped(host):
    hip = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_hip.h"))
    hosth = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_host.h"))
    assert hip["rt_render_rays"] == ("i32", ["*rt_scene", "*f32", "i32", "i32", "i32", "i32", "*rt_sampler_desc", "*rt_path_desc", "u32", "*c_void", "*f32", "*rt_stats"])
    assert hosth["rtxh_render_rays"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "*f32", "i32", "i32", "i32", "i32", "*c_void", "*f32", "*rt_stats"])
    assert hasattr(host.hip_lib(), "rt_render_rays") and hasattr(host.lib(), "rtxh_render_rays")
    _, fns = parse_rust(os.path.join(ROOT, "INTEGRATION.md"))   # (tests/test_abi_cpu.py then holds the argument types to the header's)
    assert "rt_render_rays" in fns and len(fns["rt_render_rays"][1]) == 12
    assert callable(host.HostScene.render_rays)
    params = list(inspect.signature(host.HostScene.render_rays).parameters)
    assert params == ["self", "rays", "sample0", "spp", "max_depth", "device_out", "stream", "count_traversal", "time_kernels"], params
    src = open(os.path.join(ROOT, "include", "rtx_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(RT_RAYS_MAX)\s+(\d+)", src)}
    assert defs == {"RT_RAYS_MAX": host.RT_RAYS_MAX} and host.RT_RAYS_MAX == 1 << 27
    assert sizeof_matches(host)


def sizeof_matches(host):
    L = host.hip_lib()
    return L.rt_sizeof(b"rt_sampler_desc") == C.sizeof(SamplerDesc) and L.rt_sizeof(b"rt_path_desc") == C.sizeof(PathDesc)


def test_every_refusal_answers_invalid_with_a_message_and_no_device(host):
    L = host.hip_lib()
    L.rt_render_rays.restype = C.c_int
    L.rt_render_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    buf = C.create_string_buffer(4096)
    scene = C.cast(buf, C.c_void_p)   # never dereferenced: every check comes before the scene is looked at
    f = np.zeros(64, np.float32)
    p = f.ctypes.data_as(C.c_void_p)

    def call(scene=scene, rays=p, w=2, h=2, s0=0, ns=2, spp=4, dims=4, has_smp=True, has_path=True, flags=0, rad=p):
        smp, path = SamplerDesc(spp, dims), PathDesc(5, 1.0, 0, (C.c_int32 * 4)(0, 0, 0, 0))
        L.rt_render_rays.restype = C.c_int
        rc = L.rt_render_rays(scene, rays, w, h, s0, ns, C.byref(smp) if has_smp else None, C.byref(path) if has_path else None, flags, None, rad, None)
        return rc, host.hip_lib().rt_last_error().decode()

    cases = dict(
        null_scene=dict(scene=None), null_rays=dict(rays=None), null_sampler=dict(has_smp=False), null_path=dict(has_path=False), null_radiance=dict(rad=None),
        zero_width=dict(w=0), negative_width=dict(w=-3), zero_height=dict(h=0), negative_height=dict(h=-1), zero_samples=dict(ns=0), negative_samples=dict(ns=-2),
        negative_sample0=dict(s0=-1), range_past_spp=dict(s0=3, ns=2, spp=4), range_past_rounded_spp=dict(s0=0, ns=9, spp=5),
        too_many_rays=dict(w=4096, h=4096, ns=16, spp=16), too_many_rays_wraps_32_bits=dict(w=65536, h=65536, ns=1, spp=1),
        too_many_rays_wraps_64_bits=dict(w=2 ** 31 - 1, h=2 ** 31 - 1, ns=8, spp=8), spp_too_large=dict(spp=16385, ns=1),
        dimensions_too_small=dict(dims=1), dimensions_too_large=dict(dims=9), ref_stream=dict(flags=RT_FLAG_REF_STREAM))
    for name, kw in cases.items():
        rc, msg = call(**kw)
        print(f"{name}: {rc} {msg!r}")
        assert rc == RT_ERR_INVALID and msg and "rt_render_rays" in msg, (name, rc, msg)
    # (range_past_rounded_spp: spp 5 is rounded up to 8, which holds [0, 8) and not a ninth sample.) The host layer refuses the same sizes before it uploads the scene
    H = host.lib()
    H.rtxh_render_rays.restype = C.c_int
    H.rtxh_render_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    from rustracer_amd.scenes import cornell_box
    h = host.HostScene(cornell_box(16, 16, 4))
    prm = h.setup()["params"]
    st = host.Stats()
    for kw in (dict(s=None), dict(rays=None), dict(rad=None), dict(w=0), dict(ns=0), dict(s0=-1), dict(s0=2, ns=3), dict(w=4096, h=4096 * 8 + 1, ns=4)):
        a = dict(s=h.h, rays=p, rad=p, w=2, h=2, s0=0, ns=2)
        a.update(kw)
        rc = H.rtxh_render_rays(a["s"], C.byref(prm), a["rays"], a["w"], a["h"], a["s0"], a["ns"], None, a["rad"], C.byref(st))
        assert rc == RT_ERR_INVALID and H.rtxh_last_error(), (kw, rc)   # (before the scene is uploaded: this machine has no device)
    with pytest.raises(host.BackendError):
        h.render_rays(np.zeros((2, 2, 2, 7), np.float32))


def test_orthographic_rays_are_parallel_and_start_on_the_screen_window(host):
    from rustracer_amd import cameras
    W, H, NS = 7, 5, 3
    rng = np.random.default_rng(11)
    pf = cameras.pixel_centres(W, H, NS) + rng.uniform(-0.5, 0.5, (H, W, NS, 2))
    win = (-1.5, 2.5, -0.75, 1.25)
    # camera space = world space
    r = cameras.orthographic(np.eye(4), win, W, H, pf)
    assert r.shape == (H, W, NS, 8) and r.dtype == np.float32
    assert np.all(r[..., 4:7] == np.float32([0, 0, 1])) and np.all(np.isinf(r[..., 3])) and np.all(r[..., 7] == 0)
    assert np.allclose(r[..., 0], win[0] + pf[..., 0] / W * (win[1] - win[0]), atol=1e-6) and np.all(r[..., 2] == 0)
    assert np.allclose(r[..., 1], win[3] - pf[..., 1] / H * (win[3] - win[2]), atol=1e-6)   # raster y = 0 is the window's top
    assert r[..., 0].min() >= win[0] and r[..., 0].max() <= win[1] and r[..., 1].min() >= win[2] and r[..., 1].max() <= win[3]
    corners = cameras.orthographic(np.eye(4), win, W, H, np.broadcast_to(np.float64([[0, 0], [W, H]]).reshape(1, 1, 2, 2), (H, W, 2, 2)))
    assert np.allclose(corners[0, 0, 0, :3], (win[0], win[3], 0)) and np.allclose(corners[0, 0, 1, :3], (win[1], win[2], 0))
    # a rigid camera_to_world: still parallel, unit length, along the camera's +z; origins on the transformed window's plane
    _, c2w = host.look_at((1.0, 4.0, -2.0), (0.5, 0.0, 0.3), (0.0, 0.0, 1.0))
    r = cameras.orthographic(c2w, win, W, H, pf)
    d = r[..., 4:7].reshape(-1, 3).astype(np.float64)
    axis = c2w[:3, 2].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6 and np.abs(d - axis / np.linalg.norm(axis)).max() < 1e-6 and np.abs(d - d[0]).max() == 0
    o = r[..., 0:3].reshape(-1, 3).astype(np.float64) - c2w[:3, 3]
    assert np.abs(o @ axis).max() < 1e-5
    loc = o @ c2w[:3, :2].astype(np.float64)   # back to the window's coordinates
    assert loc[:, 0].min() >= win[0] - 1e-5 and loc[:, 0].max() <= win[1] + 1e-5 and loc[:, 1].min() >= win[2] - 1e-5 and loc[:, 1].max() <= win[3] + 1e-5


def test_environment_rays_have_unit_length_and_cover_the_sphere(host):
    from rustracer_amd import cameras
    W, H = 16, 8
    pf = cameras.pixel_centres(W, H, 1)
    r = cameras.environment(np.eye(4), W, H, pf)
    assert r.shape == (H, W, 1, 8) and r.dtype == np.float32 and np.all(r[..., 0:3] == 0) and np.all(np.isinf(r[..., 3]))
    d = r[..., 4:7].reshape(-1, 3).astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6
    theta, phi = np.pi * pf[..., 1].ravel() / H, 2 * np.pi * pf[..., 0].ravel() / W   # pbrt-v3: EnvironmentCamera::GenerateRay
    want = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=1)
    assert np.abs(d - want).max() < 1e-6
    # the sphere is covered: every octant is hit, the top row looks up (+y), the bottom row down, and the solid-angle-weighted mean direction vanishes
    assert {tuple(s) for s in np.sign(d).astype(int)} >= {(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)}
    assert d.reshape(H, W, 3)[0, :, 1].min() > 0.9 and d.reshape(H, W, 3)[-1, :, 1].max() < -0.9
    assert np.abs((d * np.sin(theta)[:, None]).sum(0)).max() < 1e-9 * len(d) + 1e-6
    # film edges: y = 0 is the pole +y, y = H the pole -y; x = 0 and x = W are the same meridian
    edge = cameras.environment(np.eye(4), W, H, np.broadcast_to(np.float64([[3.0, 0.0], [3.0, H], [0.0, 2.0], [W, 2.0]]).reshape(1, 1, 4, 2), (H, W, 4, 2)))[0, 0]
    assert np.allclose(edge[0, 4:7], (0, 1, 0), atol=1e-6) and np.allclose(edge[1, 4:7], (0, -1, 0), atol=1e-6) and np.allclose(edge[2, 4:7], edge[3, 4:7], atol=1e-6)
    _, c2w = host.look_at((0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (0.0, 1.0, 0.0))
    moved = cameras.environment(c2w, W, H, pf)
    assert np.allclose(moved[..., 0:3], (0.0, 1.0, 0.0)) and np.abs(np.linalg.norm(moved[..., 4:7].astype(np.float64), axis=-1) - 1).max() < 1e-6
    assert np.allclose(moved[..., 4:7].reshape(-1, 3), want @ c2w[:3, :3].astype(np.float64).T, atol=1e-6)


def test_ray_generation_is_a_kernel_of_its_own(host):
    """k_raygen_rays and k_rays_scan are in the library beside k_raygen / k_raygen_masked / k_sample_store, and the streaming kernel stays light: no scratch, no spill,
    at most 64 VGPRs (eight waves per SIMD). That no shade kernel moved is tests/test_shade_split_budget_cpu.py's to say, unchanged."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_budget", os.path.join(ROOT, "scripts", "kernel_budget.py"))
    kb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kb)
    res = kb.kernel_resources(host.HIP_LIB)
    for k in ("rtx::k_raygen", "rtx::k_raygen_masked", "rtx::k_raygen_rays", "rtx::k_rays_scan", "rtx::k_sample_store"):
        assert k in res, (k, sorted(n for n in res if "raygen" in n))
    r = res["rtx::k_raygen_rays"]
    print("k_raygen_rays", r)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["vgpr"] <= 64   # eight waves per SIMD: a streaming kernel
