"""Ray differentials with caller-supplied rays (RT_FLAG_RAY_DIFFERENTIALS) and rt_camera_rays, without a GPU: the additions are declared, exported, spelled out for the
Rust binding and wrapped; every refusal of rt_camera_rays answers RT_ERR_INVALID with a message before any device work (the scene pointer is a dummy that is never
dereferenced) and a valid call answers RT_ERR_NO_DEVICE; the flag is a legal bit of a ray-frame step and an unknown bit is not; the numpy cameras make the differentials
pbrt-v3 defines, held to a float64 model written here; and each k_shade_rays<M, G> fits the budget of its sibling k_shade<M, G>."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from test_abi_cpu import parse_c_prototypes, parse_rust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID, RT_ERR_NO_DEVICE = -1, -2
RT_FLAG_FILM_ON_DEVICE, RT_FLAG_REF_STREAM, RT_FLAG_RAY_DIFFERENTIALS = 2, 16, 128


class Camera(C.Structure):
    _fields_ = [("raster_to_camera", C.c_float * 16), ("camera_to_world", C.c_float * 16), ("dx_camera", C.c_float * 3), ("dy_camera", C.c_float * 3),
                ("lens_radius", C.c_float), ("focal_distance", C.c_float)]


class FilmDesc(C.Structure):
    _fields_ = [("cropped_pixel_bounds", C.c_int32 * 4), ("sample_bounds", C.c_int32 * 4), ("filter_radius", C.c_float * 2), ("filter_table", C.c_float * 256),
                ("max_sample_luminance", C.c_float)]


class SamplerDesc(C.Structure):
    _fields_ = [("spp", C.c_int32), ("dimensions", C.c_int32)]


# ---------------------------------------------------------------------------------------------- headers and exports
def test_the_additions_are_declared_exported_documented_and_wrapped(host):
    hip = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_hip.h"))
    hosth = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_host.h"))
    assert hip["rt_camera_rays"] == ("i32", ["*rt_scene", "*rt_camera", "*rt_film_desc", "*rt_sampler_desc", "i32", "i32", "u32", "*c_void", "*f32", "*f32"])
    assert hosth["rtxh_camera_rays"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "i32", "i32", "u32", "*c_void", "*f32", "*f32"])
    assert hasattr(host.hip_lib(), "rt_camera_rays") and hasattr(host.lib(), "rtxh_camera_rays")
    src = open(os.path.join(ROOT, "include", "rtx_hip.h")).read()
    assert re.search(r"#define\s+RT_FLAG_RAY_DIFFERENTIALS\s+128u\b", src) and re.search(r"#define\s+RT_RAY_DIFF_FLOATS\s+20\b", src)
    host_src = open(os.path.join(ROOT, "include", "rtx_host.h")).read()
    assert "RT_FLAG_RAY_DIFFERENTIALS" in host_src and "RT_RAY_DIFF_FLOATS" in host_src   # the host layer's entry points name them (it includes rtx_hip.h)
    assert host.RT_FLAG_RAY_DIFFERENTIALS == 128 and host.RT_RAY_DIFF_FLOATS == 20
    # the signatures of the entry points that take the flag stay what tests/test_render_rays_cpu.py and tests/test_ray_frame_cpu.py pin
    assert len(hip["rt_render_rays"][1]) == 12 and len(hip["rt_frame_advance_rays"][1]) == 7 and len(hip["rt_frame_advance_rays_adaptive"][1]) == 10
    _, fns = parse_rust(os.path.join(ROOT, "INTEGRATION.md"))   # (tests/test_abi_cpu.py then holds the argument types to the header's)
    assert "rt_camera_rays" in fns and len(fns["rt_camera_rays"][1]) == 10
    assert "RT_FLAG_RAY_DIFFERENTIALS (128)" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    params = inspect.signature(host.HostScene.camera_rays).parameters
    assert list(params) == ["self", "sample0", "n_samples", "differentials", "with_p_film", "device_out", "stream"]
    assert (params["sample0"].default, params["n_samples"].default, params["differentials"].default, params["with_p_film"].default, params["device_out"].default) == \
        (0, None, False, True, None)
    assert host.hip_lib().rt_sizeof(b"rt_camera") == C.sizeof(Camera) and host.hip_lib().rt_sizeof(b"rt_film_desc") == C.sizeof(FilmDesc)


def test_ray_arrays_are_8_or_20_floats_wide(host):
    from rustracer_amd.scenes import cornell_box
    h = host.HostScene(cornell_box(16, 16, 4))
    for width in (7, 9, 12, 19, 21):
        with pytest.raises(ValueError):
            h.render_rays(np.zeros((2, 2, 2, width), np.float32))
        fr = host.RayFrame.__new__(host.RayFrame)
        fr.h, fr.width, fr.height = C.c_void_p(1), 5, 3   # (_step_args looks at the shapes only; the handle is never used)
        with pytest.raises(ValueError):
            fr._step_args(np.zeros((3, 5, 2, width), np.float32), None)
        fr.h = None
    fr = host.RayFrame.__new__(host.RayFrame)
    fr.h, fr.width, fr.height = C.c_void_p(1), 5, 3
    assert fr._step_args(np.zeros((3, 5, 2, 8), np.float32), None)[3] == 0
    assert fr._step_args(np.zeros((3, 5, 2, 20), np.float32), np.zeros((3, 5, 2, 2), np.float32))[3] == RT_FLAG_RAY_DIFFERENTIALS
    fr.h = None


# ---------------------------------------------------------------------------------------------- refusals without a device
def test_every_refusal_of_rt_camera_rays_answers_invalid_with_a_message_and_a_valid_call_no_device(host):
    L = host.hip_lib()
    L.rt_camera_rays.restype = C.c_int
    L.rt_camera_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    buf = C.create_string_buffer(4096)
    scene = C.cast(buf, C.c_void_p)   # never dereferenced: every check comes before the scene is looked at
    f = np.zeros(4 * 4 * 4 * 20, np.float32)
    p = f.ctypes.data_as(C.c_void_p)

    def call(scene=scene, has_cam=True, has_film=True, has_smp=True, rays=p, sb=(0, 0, 4, 4), crop=(0, 0, 4, 4), s0=0, ns=2, spp=4, dims=4, flags=0):
        cam, film, smp = Camera(), FilmDesc(), SamplerDesc(spp, dims)
        film.sample_bounds[:], film.cropped_pixel_bounds[:] = sb, crop
        film.filter_radius[0] = film.filter_radius[1] = 0.5
        rc = L.rt_camera_rays(scene, C.byref(cam) if has_cam else None, C.byref(film) if has_film else None, C.byref(smp) if has_smp else None, s0, ns, flags, None, rays, None)
        return rc, L.rt_last_error().decode()

    cases = dict(
        null_scene=dict(scene=None), null_camera=dict(has_cam=False), null_film=dict(has_film=False), null_sampler=dict(has_smp=False), null_rays=dict(rays=None),
        empty_film=dict(sb=(0, 0, 0, 4)), empty_film_rows=dict(sb=(2, 3, 6, 3)), empty_cropped_film=dict(crop=(0, 0, 4, 0)),
        zero_samples=dict(ns=0), negative_samples=dict(ns=-2), negative_sample0=dict(s0=-1), range_past_spp=dict(s0=3, ns=2, spp=4),
        range_past_rounded_spp=dict(s0=0, ns=9, spp=5), too_many_rays=dict(sb=(0, 0, 4096, 4096), ns=16, spp=16),
        too_many_rays_wraps_32_bits=dict(sb=(0, 0, 65536, 65536), ns=1, spp=1), too_many_rays_wraps_64_bits=dict(sb=(-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), ns=8, spp=8),
        spp_too_large=dict(spp=16385, ns=1), dimensions_too_small=dict(dims=1), dimensions_too_large=dict(dims=9),
        flag_ref_stream=dict(flags=RT_FLAG_REF_STREAM), flag_count_traversal=dict(flags=1), flag_unknown=dict(flags=256))
    for name, kw in cases.items():
        rc, msg = call(**kw)
        print(f"{name}: {rc} {msg!r}")
        assert rc == RT_ERR_INVALID and msg and "rt_camera_rays" in msg, (name, rc, msg)
    for flags in (0, RT_FLAG_RAY_DIFFERENTIALS, RT_FLAG_FILM_ON_DEVICE | RT_FLAG_RAY_DIFFERENTIALS):
        rc, msg = call(flags=flags)   # a valid call: this machine has no device, and the library has no CPU fallback
        print(f"valid, flags {flags}: {rc} {msg!r}")
        assert not host.device_available() and rc == RT_ERR_NO_DEVICE and "rt_camera_rays" in msg, (rc, msg)
    # the host layer refuses the same sizes before it uploads the scene
    H = host.lib()
    H.rtxh_camera_rays.restype = C.c_int
    H.rtxh_camera_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    from rustracer_amd.scenes import cornell_box
    h = host.HostScene(cornell_box(16, 16, 4))
    prm = h.setup()["params"]
    for kw in (dict(s=None), dict(rays=None), dict(ns=0), dict(s0=-1), dict(s0=2, ns=3), dict(flags=256), dict(flags=RT_FLAG_REF_STREAM)):
        a = dict(s=h.h, rays=p, s0=0, ns=2, flags=0)
        a.update(kw)
        rc = H.rtxh_camera_rays(a["s"], C.byref(prm), a["s0"], a["ns"], a["flags"], None, a["rays"], None)
        assert rc == RT_ERR_INVALID and H.rtxh_last_error(), (kw, rc)


def test_the_flag_is_a_legal_bit_of_a_step_and_an_unknown_bit_is_not(host):
    L = host.hip_lib()
    L.rt_frame_advance_rays.restype = C.c_int
    L.rt_frame_advance_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.rt_frame_advance_rays_adaptive.restype = C.c_int
    L.rt_frame_advance_rays_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    f = np.zeros(64, np.float32)
    p = f.ctypes.data_as(C.c_void_p)
    buf = C.create_string_buffer(65536)
    frame = C.cast(buf, C.c_void_p)   # a zeroed dummy: not a ray frame (ray_frame = false), so a step that passes the flag check is refused for its kind
    for who, step in (("rt_frame_advance_rays", lambda fr, flags: L.rt_frame_advance_rays(fr, p, None, 1, flags, None, None)),
                      ("rt_frame_advance_rays_adaptive", lambda fr, flags: L.rt_frame_advance_rays_adaptive(fr, p, None, 1, 0.1, 0.0, 4, flags, None, None))):
        rc = step(None, RT_FLAG_RAY_DIFFERENTIALS)
        msg = L.rt_last_error().decode()
        print(f"{who}, NULL frame, flag 128: {rc} {msg!r}")
        assert rc == RT_ERR_INVALID and who in msg and "null frame" in msg
        rc = step(frame, 256)
        msg = L.rt_last_error().decode()
        print(f"{who}, flag 256: {rc} {msg!r}")
        assert rc == RT_ERR_INVALID and who in msg and "flags of a step" in msg
        rc = step(frame, 256 | RT_FLAG_RAY_DIFFERENTIALS)
        assert rc == RT_ERR_INVALID and "flags of a step" in L.rt_last_error().decode()
        for flags in (RT_FLAG_RAY_DIFFERENTIALS, RT_FLAG_RAY_DIFFERENTIALS | RT_FLAG_FILM_ON_DEVICE):   # legal bits: the refusal is the next check's
            rc = step(frame, flags)
            msg = L.rt_last_error().decode()
            print(f"{who}, flags {flags}: {rc} {msg!r}")
            assert rc == RT_ERR_INVALID and who in msg and "flags of a step" not in msg and "begun with a camera" in msg


# ---------------------------------------------------------------------------------------------- cameras.py against a float64 model
def _model_world(c2w, o_cam, d_cam):
    m = np.asarray(c2w, np.float64).reshape(4, 4)
    o = np.einsum("ij,...j->...i", m[:3, :3], o_cam) + m[:3, 3]
    d = np.einsum("ij,...j->...i", m[:3, :3], d_cam)
    return o, d / np.sqrt((d * d).sum(-1, keepdims=True))


def _pull(main, shifted, spp):
    return main + (shifted - main) / np.sqrt(np.float64(spp))


@pytest.mark.parametrize("spp", [1, 4, 16])
def test_orthographic_differentials_are_the_windows_pixel_steps(host, spp):
    from rustracer_amd import cameras
    W, H, NS = 7, 5, 3
    rng = np.random.default_rng(3)
    pf = cameras.pixel_centres(W, H, NS) + rng.uniform(-0.5, 0.5, (H, W, NS, 2))
    win = (-1.5, 2.5, -0.75, 1.25)
    _, c2w = host.look_at((1.0, 4.0, -2.0), (0.5, 0.0, 0.3), (0.0, 0.0, 1.0))
    plain = cameras.orthographic(c2w, win, W, H, pf)
    r = cameras.orthographic(c2w, win, W, H, pf, differentials=True, spp=spp)
    assert r.shape == (H, W, NS, 20) and r.dtype == np.float32 and plain.shape == (H, W, NS, 8)
    assert r[..., :8].tobytes() == plain.tobytes()   # the ray itself does not move
    m = c2w.astype(np.float64)
    x_axis, y_axis = m[:3, 0], m[:3, 1]
    step_x, step_y = (win[1] - win[0]) / W, (win[3] - win[2]) / H
    s = 1.0 / np.sqrt(spp)
    # the model: o on the window, rx_o one pixel to the right (+x of the camera), ry_o one pixel down (-y of the camera), pulled in by 1 / sqrt(spp); directions = d
    o_cam = np.stack([win[0] + pf[..., 0] / W * (win[1] - win[0]), win[3] - pf[..., 1] / H * (win[3] - win[2]), np.zeros(pf.shape[:3])], axis=-1)
    d_cam = np.broadcast_to(np.float64([0, 0, 1]), o_cam.shape)
    o, d = _model_world(c2w, o_cam, d_cam)
    want = np.concatenate([o + x_axis * step_x * s, o - y_axis * step_y * s, d, d], axis=-1)
    err = float(np.abs(r[..., 8:20].astype(np.float64) - want).max())
    # the statement of the issue, on the records themselves: rx_o - o and ry_o - o are the pixel steps (float32 rounding of coordinates of magnitude <= 5: 5 * 2^-23 each)
    dx = r[..., 8:11].astype(np.float64) - r[..., 0:3].astype(np.float64)
    dy = r[..., 11:14].astype(np.float64) - r[..., 0:3].astype(np.float64)
    e_dx, e_dy = float(np.abs(dx - x_axis * step_x * s).max()), float(np.abs(dy + y_axis * step_y * s).max())
    print(f"\northographic spp {spp}: differential fields against the model {err:.3e}; rx_o - o against the x step {e_dx:.3e}, ry_o - o against the -y step {e_dy:.3e}")
    assert err <= 5 * 2.0 ** -23 and e_dx <= 10 * 2.0 ** -23 and e_dy <= 10 * 2.0 ** -23
    assert np.array_equal(r[..., 14:17], r[..., 4:7]) and np.array_equal(r[..., 17:20], r[..., 4:7])   # rx_d = ry_d = d, exactly


@pytest.mark.parametrize("spp", [1, 4, 16])
def test_environment_differentials_are_the_generators_rays_one_pixel_on(host, spp):
    from rustracer_amd import cameras
    W, H, NS = 16, 8, 2
    rng = np.random.default_rng(4)
    pf = cameras.pixel_centres(W, H, NS) + rng.uniform(-0.5, 0.5, (H, W, NS, 2))
    _, c2w = host.look_at((0.0, 1.0, 0.0), (1.0, 1.2, 0.3), (0.0, 1.0, 0.0))
    plain = cameras.environment(c2w, W, H, pf)
    r = cameras.environment(c2w, W, H, pf, differentials=True, spp=spp)
    assert r.shape == (H, W, NS, 20) and r.dtype == np.float32 and r[..., :8].tobytes() == plain.tobytes()

    def gen(q):   # pbrt-v3: EnvironmentCamera::GenerateRay, in float64
        theta, phi = np.pi * q[..., 1] / H, 2 * np.pi * q[..., 0] / W
        d_cam = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
        return _model_world(c2w, np.zeros_like(d_cam), d_cam)

    (o, d), (ox, dx), (oy, dy) = gen(pf), gen(pf + (1.0, 0.0)), gen(pf + (0.0, 1.0))
    want = np.concatenate([_pull(o, ox, spp), _pull(o, oy, spp), _pull(d, dx, spp), _pull(d, dy, spp)], axis=-1)
    err = float(np.abs(r[..., 8:20].astype(np.float64) - want).max())
    moved = float(np.abs(r[..., 14:17] - r[..., 4:7]).max())
    # ... and against the module's own 8-float generator at the shifted positions (spp 1: no pull)
    own = np.concatenate([cameras.environment(c2w, W, H, pf + (1.0, 0.0))[..., 4:7], cameras.environment(c2w, W, H, pf + (0.0, 1.0))[..., 4:7]], axis=-1)
    print(f"\nenvironment spp {spp}: differential fields against the model {err:.3e} (coordinates <= 1: 2^-24 each); rx_d moves off d by up to {moved:.3e}")
    assert err <= 2.0 ** -23 and moved > 0.1 / np.sqrt(spp)
    assert np.all(r[..., 8:14] == np.float32([0.0, 1.0, 0.0] * 2))   # every ray from the camera's origin, the shifted ones too
    if spp == 1:
        assert np.abs(r[..., 14:20].astype(np.float64) - own).max() <= 2.0 ** -23


def test_without_differentials_the_output_is_todays(host):
    """The 8-float records, byte for byte, against the arithmetic the module has always used (float64, rounded once)."""
    from rustracer_amd import cameras
    W, H, NS = 6, 4, 2
    pf = cameras.pixel_centres(W, H, NS) + np.random.default_rng(9).uniform(-0.5, 0.5, (H, W, NS, 2))
    _, c2w = host.look_at((1.0, 4.0, -2.0), (0.5, 0.0, 0.3), (0.0, 0.0, 1.0))
    m = np.asarray(c2w, np.float64).reshape(4, 4)

    def rays(o_cam, d_cam):
        o = o_cam @ m[:3, :3].T + m[:3, 3]
        d = d_cam @ m[:3, :3].T
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        out = np.zeros(o.shape[:-1] + (8,), np.float32)
        out[..., 0:3], out[..., 3], out[..., 4:7] = o, np.inf, d
        return out

    win = (-1.5, 2.5, -0.75, 1.25)
    o = np.zeros((H, W, NS, 3))
    o[..., 0] = win[0] + pf[..., 0] / W * (win[1] - win[0])
    o[..., 1] = win[3] - pf[..., 1] / H * (win[3] - win[2])
    d = np.zeros_like(o)
    d[..., 2] = 1.0
    assert cameras.orthographic(c2w, win, W, H, pf).tobytes() == rays(o, d).tobytes()
    assert cameras.orthographic(c2w, win, W, H, pf, differentials=False, spp=16).tobytes() == rays(o, d).tobytes()
    theta, phi = np.pi * pf[..., 1] / H, 2.0 * np.pi * pf[..., 0] / W
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
    assert cameras.environment(c2w, W, H, pf).tobytes() == rays(np.zeros_like(d), d).tobytes()


# ---------------------------------------------------------------------------------------------- budgets
@pytest.fixture(scope="module")
def resources(host):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_budget
    finally:
        sys.path.pop(0)
    return kernel_budget.kernel_resources(host.HIP_LIB)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("mode", [0, 3, 5, 6])
def test_a_shade_kernel_for_rays_fits_its_siblings_budget(resources, mode, general):
    """k_shade_rays<M, G> drops the camera arithmetic and the lens-table lookup of k_shade<M, G> and adds one set of differentials (12 floats) and its address: no more
    VGPRs, no more LDS, at most 16 more spilled dwords than the sibling. As built (vgpr / spilled dwords, sibling in brackets): <0, false> 255 / 0 (256 / 18),
    <0, true> 256 / 0 (256 / 19), <3, false> 168 / 16 (168 / 25), <3, true> 239 / 0 (252 / 0), <5, false> 168 / 38 (168 / 52), <5, true> 256 / 4 (256 / 29),
    <6, false> 168 / 45 (168 / 65), <6, true> 256 / 24 (256 / 34); 272 B of LDS each (MEASUREMENTS.md)."""
    g = "true" if general else "false"
    r, sib = resources[f"rtx::k_shade_rays<{mode}, {g}>"], resources[f"rtx::k_shade<{mode}, {g}, false, false, false, 0>"]
    print(f"\nk_shade_rays<{mode}, {g}> {r}\n  sibling k_shade<{mode}, {g}> {sib}")
    assert r["vgpr"] <= sib["vgpr"], (r, sib)
    assert r["lds"] <= sib["lds"], (r, sib)
    assert r["vgpr_spills"] <= sib["vgpr_spills"] + 16, (r, sib)


def test_the_new_kernels_are_in_the_library_and_the_ray_producers_stay_light(resources):
    for k in ("rtx::k_camera_rays", "rtx::k_raygen_rays", "rtx::k_raygen_rays_film", "rtx::k_raygen_rays_film_masked", "rtx::k_rays_scan", "rtx::k_rays_scan_owned"):
        r = resources[k]
        print(k, r)
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["vgpr"] <= 64, (k, r)   # streaming kernels: eight waves per SIMD
