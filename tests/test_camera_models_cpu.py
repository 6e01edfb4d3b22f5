"""Camera models on the device (rt_camera_model_rays / rt_frame_begin_model / rt_render_model) without a GPU: the prototypes are declared in both headers with the argument
lists the entry points have, exported, spelled out for the Rust binding and wrapped in Python; `host.camera_model` packs the 24 floats and finds pbrt's default screen
window; the float64 model of both cameras (tests/camera_model.py), which the GPU tests hold the kernels to, reproduces rustracer_amd/cameras.py bit for bit where that has
a say (no lens) and has the thin lens' geometry; every refusal answers RT_ERR_INVALID with a message that names the field before any device work (the scene pointer is a
dummy that is never dereferenced); the two kernels are in the code object, streaming kernels without scratch."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import camera_model as cm
from test_abi_cpu import parse_c_prototypes, parse_rust
from test_ray_frame_cpu import FilmDesc, PathDesc, SamplerDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1
NX, NY, NS = 16, 12, 4
WINDOW = (-0.9, 1.1, -0.6, 0.7)

RAYS = ("i32", ["*rt_scene", "i32", "*f32", "*rt_film_desc", "*rt_sampler_desc", "i32", "i32", "u32", "*c_void", "*f32", "*f32"])
BEGIN = ("i32", ["*rt_scene", "i32", "*f32", "*rt_film_desc", "*rt_sampler_desc", "*rt_path_desc", "*rt_shard", "u32", "u64", "**rt_frame"])
RENDER = ("i32", ["*rt_scene", "i32", "*f32", "*rt_film_desc", "*rt_sampler_desc", "*rt_path_desc", "*rt_shard", "u32", "*c_void", "*f32", "*rt_stats"])


def camera_to_world():
    """Rotations about two axes and a translation, in float32."""
    a, b = 0.4, -0.3
    ry = np.float64([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.float64([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx
    m[:3, 3] = (0.3, 1.7, -2.2)
    return m.astype(np.float32)


def test_prototypes_are_declared_exported_documented_and_wrapped(host):
    hip = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_hip.h"))
    hosth = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_host.h"))
    assert hip["rt_camera_model_rays"] == RAYS
    assert hip["rt_frame_begin_model"] == BEGIN
    assert hip["rt_render_model"] == RENDER
    assert hosth["rtxh_camera_model"] == ("i32", ["*rtxh_render_params", "i32", "*f32"])
    assert hosth["rtxh_camera_model_rays"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "i32", "*f32", "i32", "i32", "u32", "*c_void", "*f32", "*f32"])
    assert hosth["rtxh_frame_begin_model"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "i32", "*f32", "u64", "**rtxh_frame"])
    assert hosth["rtxh_render_model"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "i32", "*f32", "*c_void", "*f32", "*rt_stats"])
    for name in ("rt_camera_model_rays", "rt_frame_begin_model", "rt_render_model"):
        assert hasattr(host.hip_lib(), name) and hasattr(host.lib(), name.replace("rt_", "rtxh_", 1)), name
    _, fns = parse_rust(os.path.join(ROOT, "INTEGRATION.md"))   # (tests/test_abi_cpu.py then holds the argument types to the header's)
    assert [len(fns[n][1]) for n in ("rt_camera_model_rays", "rt_frame_begin_model", "rt_render_model")] == [11, 10, 11]
    src = open(os.path.join(ROOT, "include", "rtx_hip.h")).read()
    for define, value in (("RT_CAMERA_ORTHOGRAPHIC", 1), ("RT_CAMERA_ENVIRONMENT", 2), ("RT_CAMERA_MODEL_FLOATS", 24)):
        assert f"#define {define} {value}\n" in src and getattr(host, define) == value
    # the Python layer
    assert list(inspect.signature(host.camera_model).parameters) == ["kind", "camera_to_world", "width", "height", "screen_window", "lens_radius", "focal_distance"]
    d = {k: v.default for k, v in inspect.signature(host.camera_model).parameters.items()}
    assert d["screen_window"] is None and d["lens_radius"] == 0 and d["focal_distance"] == 1e6
    assert list(inspect.signature(host.HostScene.camera_model_rays).parameters)[:7] == ["self", "kind", "camera", "sample0", "n_samples", "differentials", "with_p_film"]
    assert list(inspect.signature(host.HostScene.progressive_model).parameters)[:3] == ["self", "kind", "camera"]
    assert list(inspect.signature(host.HostScene.render_model).parameters)[:3] == ["self", "kind", "camera"]
    assert issubclass(host.ModelFrame, host.ProgressiveFrame) and not issubclass(host.ModelFrame, host.RayFrame)
    for inherited in ("advance", "advance_adaptive", "film", "rgb", "sums", "display", "pixel_stats", "features", "noise", "close", "samples_done", "samples_taken",
                      "active_pixels", "state_bytes"):
        assert getattr(host.ModelFrame, inherited) is getattr(host.ProgressiveFrame, inherited), inherited


def test_camera_model_packs_the_floats_and_finds_the_default_window(host):
    m = camera_to_world()
    c = host.camera_model("orthographic", m, NX, NY, screen_window=WINDOW, lens_radius=0.05, focal_distance=2.0)
    assert c.dtype == np.float32 and c.shape == (24,)
    assert c[:16].tobytes() == m.reshape(16).tobytes()
    assert c[16:20].tobytes() == np.float32(WINDOW).tobytes() and c[20] == np.float32(0.05) and c[21] == 2.0 and c[22] == 0 and c[23] == 0
    e = host.camera_model("environment", m, NX, NY)
    assert e[20] == 0 and e[21] == np.float32(1e6) and e[22] == 0 and e[23] == 0
    # pbrt's default: the shorter axis spans [-1, 1]
    wide = host.camera_model("orthographic", m, 16, 12)[16:20]
    tall = host.camera_model("orthographic", m, 12, 16)[16:20]
    square = host.camera_model("orthographic", m, 8, 8)[16:20]
    a = np.float32(16) / np.float32(12)
    assert wide.tolist() == [-a, a, -1.0, 1.0]
    b = np.float32(12) / np.float32(16)
    assert tall.tolist() == [-1.0, 1.0, np.float32(-1.0) / b, np.float32(1.0) / b]
    assert square.tolist() == [-1.0, 1.0, -1.0, 1.0]
    with pytest.raises(host.BackendError):
        host.camera_model("fisheye", m, NX, NY)
    # the helper that fills the floats from render parameters (a loaded pbrt scene's) agrees
    L = host.lib()
    from rustracer_amd.scenes import cornell_box
    h = host.HostScene(cornell_box(NX, NY, NS))
    p = h.setup()["params"]
    got = h.camera_model_params("orthographic")
    assert got[:16].tobytes() == np.float32(list(p.cam_to_world)).tobytes() and got[16:20].tolist() == wide.tolist() and got[22:].tolist() == [0, 0]
    assert got[20] == np.float32(p.lens_radius) and got[21] == np.float32(p.focal_distance)
    q = type(p).from_buffer_copy(p)
    q.xres, q.yres, q.lens_radius, q.focal_distance = 12, 16, 0.25, 3.0
    q.screen_window[:] = [0.0] * 4
    out = np.zeros(24, np.float32)
    assert L.rtxh_camera_model(C.byref(q), 1, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert out[16:20].tolist() == tall.tolist() and out[20] == 0.25 and out[21] == 3.0
    assert L.rtxh_camera_model(C.byref(q), 2, out.ctypes.data_as(C.POINTER(C.c_float))) == 0 and out[20] == 0 and out[21] == 0   # the environment camera has no lens
    q.screen_window[:] = list(WINDOW)
    assert L.rtxh_camera_model(C.byref(q), 1, out.ctypes.data_as(C.POINTER(C.c_float))) == 0 and out[16:20].tobytes() == np.float32(WINDOW).tobytes()
    assert L.rtxh_camera_model(C.byref(q), 3, out.ctypes.data_as(C.POINTER(C.c_float))) == RT_ERR_INVALID and b"model" in L.rtxh_last_error()


def _film_positions():
    rng = np.random.default_rng(5)
    x, y = np.meshgrid(np.arange(NX, dtype=np.float64), np.arange(NY, dtype=np.float64))
    return (np.stack([x, y], axis=-1)[:, :, None, :] + rng.uniform(0.0, 1.0, (NY, NX, NS, 2))).astype(np.float32).astype(np.float64)


def test_the_float64_model_without_a_lens_is_cameras_py_to_the_last_float32_bit(host):
    from rustracer_amd import cameras
    m, p = camera_to_world(), _film_positions()
    win = [float(v) for v in np.float32(WINDOW)]
    cam_o = host.camera_model("orthographic", m, NX, NY, screen_window=WINDOW)
    cam_e = host.camera_model("environment", m, NX, NY)
    for spp in (4, 16):
        got_o = cm.model_rays(cm.ORTHOGRAPHIC, cam_o, NX, NY, p, spp).astype(np.float32)
        got_e = cm.model_rays(cm.ENVIRONMENT, cam_e, NX, NY, p, spp).astype(np.float32)
        want_o = cameras.orthographic(m, win, NX, NY, p, differentials=True, spp=spp)
        want_e = cameras.environment(m, NX, NY, p, differentials=True, spp=spp)
        assert got_o.shape == want_o.shape == (NY, NX, NS, 20)
        assert got_o.tobytes() == want_o.tobytes()
        assert got_e.tobytes() == want_e.tobytes()
        assert got_o[..., :8].tobytes() == cameras.orthographic(m, win, NX, NY, p).tobytes()
    # W / H, the window's orientation and the scaling are visible in these shapes: a swapped or mirrored model is another array
    assert np.abs(want_o[..., 8:11] - want_o[..., 0:3]).max() > 1e-2 and np.abs(want_e[..., 14:17] - want_e[..., 4:7]).max() > 1e-2


def test_the_float64_thin_lens_has_its_geometry():
    rng = np.random.default_rng(9)
    p = _film_positions()
    u = rng.uniform(0.0, 1.0, (NY, NX, NS, 2))
    cam = np.zeros(24)
    cam[:16] = np.eye(4).reshape(16)
    cam[16:20], cam[20], cam[21] = WINDOW, 0.05, 2.0
    disk = cm.concentric_sample_disk(u)
    assert np.all(np.hypot(disk[..., 0], disk[..., 1]) <= 1.0) and np.allclose(cm.concentric_sample_disk(np.float64([[0.5, 0.5]])), 0.0)
    # area-preserving: a quarter of the samples within half the radius
    assert abs(float((np.hypot(disk[..., 0], disk[..., 1]) <= 0.5).mean()) - 0.25) < 0.06
    r = cm.model_rays(cm.ORTHOGRAPHIC, cam, NX, NY, p, 1, p_lens=u)
    o, d = r[..., 0:3], r[..., 4:7]
    assert np.all(o[..., 2] == 0.0) and np.allclose(o[..., :2], 0.05 * disk, atol=1e-15)
    x0, x1, y0, y1 = WINDOW
    focus = np.stack([x0 + p[..., 0] / NX * (x1 - x0), y1 - p[..., 1] / NY * (y1 - y0), np.full(p.shape[:-1], 2.0)], axis=-1)
    t = (2.0 - o[..., 2:3]) / d[..., 2:3]
    assert np.abs(o + t * d - focus).max() < 1e-14 and np.allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-15)
    # the differential rays leave the same lens point and meet the plane z = ft at the neighbouring pixel's point (spp = 1: unscaled)
    ft = 2.0 / d[..., 2:3]
    for k, step in ((0, np.float64([(x1 - x0) / NX, 0.0, 0.0])), (1, np.float64([0.0, -(y1 - y0) / NY, 0.0]))):
        ro, rd = r[..., 8 + 3 * k:11 + 3 * k], r[..., 14 + 3 * k:17 + 3 * k]
        assert np.array_equal(ro, o)
        target = focus * np.float64([1, 1, 0]) + step + np.concatenate([np.zeros_like(ft), np.zeros_like(ft), ft], axis=-1)
        tt = ft / rd[..., 2:3]
        assert np.abs(ro + tt * rd - target).max() < 1e-14
    # a lens point given directly is the same ray
    again = cm.model_rays(cm.ORTHOGRAPHIC, cam, NX, NY, p, 1, lens_point=0.05 * disk)
    assert np.array_equal(again, r)


def test_every_refusal_answers_invalid_with_a_message_that_names_the_field_and_no_device(host):
    L = host.hip_lib()
    L.rt_last_error.restype = C.c_char_p
    L.rt_camera_model_rays.restype = L.rt_frame_begin_model.restype = L.rt_render_model.restype = C.c_int
    L.rt_camera_model_rays.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_frame_begin_model.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    L.rt_render_model.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    buf = C.create_string_buffer(4096)
    scene = C.cast(buf, C.c_void_p)   # never dereferenced: every check comes before the scene is looked at
    sink = np.zeros(NX * NY * NS * 20, np.float32)

    def call(model=1, edit=None, x0y0=(0, 0), dims=4):
        cam = host.camera_model("orthographic", camera_to_world(), NX, NY, screen_window=WINDOW, lens_radius=0.05, focal_distance=2.0)
        if model == 2:
            cam[20] = 0.0
        if edit:
            for k, v in edit.items():
                cam[k] = v
        film = FilmDesc()
        film.cropped_pixel_bounds[:] = [x0y0[0], x0y0[1], NX, NY]
        film.filter_radius[0] = film.filter_radius[1] = 0.5
        film.max_sample_luminance = np.inf
        smp, path = SamplerDesc(NS, dims), PathDesc(5, 1.0, 0, (C.c_int32 * 4)(0, 0, 0, 0))
        pc = cam.ctypes.data_as(C.c_void_p)
        out = C.c_void_p(0x1234)
        res = []
        rc = L.rt_camera_model_rays(scene, model, pc, C.byref(film), C.byref(smp), 0, NS, 128, None, sink.ctypes.data_as(C.c_void_p), None)
        res.append(("rt_camera_model_rays", rc, L.rt_last_error().decode()))
        rc = L.rt_frame_begin_model(scene, model, pc, C.byref(film), C.byref(smp), C.byref(path), None, 0, 0, C.byref(out))
        res.append(("rt_frame_begin_model", rc, L.rt_last_error().decode()))
        assert not out.value   # *out is NULL after a refusal
        rc = L.rt_render_model(scene, model, pc, C.byref(film), C.byref(smp), C.byref(path), None, 0, None, sink.ctypes.data_as(C.c_void_p), None)
        res.append(("rt_render_model", rc, L.rt_last_error().decode()))
        return res

    cases = dict(
        unknown_model=(dict(model=3), "model"), model_zero=(dict(model=0), "model"),
        empty_window_x=(dict(edit={16: 1.0, 17: 1.0}), "screen_window"), inverted_window_y=(dict(edit={18: 0.7, 19: -0.6}), "screen_window"),
        window_nan=(dict(edit={17: np.nan}), "screen_window"), window_inf=(dict(edit={19: np.inf}), "screen_window"),
        negative_lens=(dict(edit={20: -0.01}), "lens_radius"), lens_nan=(dict(edit={20: np.nan}), "lens_radius"),
        zero_focal_distance=(dict(edit={21: 0.0}), "focal_distance"), negative_focal_distance=(dict(edit={21: -2.0}), "focal_distance"),
        focal_distance_nan=(dict(edit={21: np.nan}), "focal_distance"),
        lens_on_the_environment_camera=(dict(model=2, edit={20: 0.05}), "lens_radius"),
        matrix_nan=(dict(edit={5: np.nan}), "camera_to_world"), matrix_inf=(dict(model=2, edit={3: -np.inf}), "camera_to_world"),
        reserved_22=(dict(edit={22: 1.0}), "reserved"), reserved_23=(dict(model=2, edit={23: -1e-30}), "reserved"),
        cropped_film=(dict(x0y0=(2, 0)), "cropped_pixel_bounds"), empty_film=(dict(x0y0=(NX, 0)), "cropped_pixel_bounds"))
    for name, (kw, word) in cases.items():
        for fn, rc, msg in call(**kw):
            print(f"{name}: {fn} {rc} {msg!r}")
            assert rc == RT_ERR_INVALID and msg.startswith("rt_") and word in msg, (name, fn, rc, msg)
            assert fn in msg or (fn == "rt_render_model" and "rt_frame_begin_model" in msg), (name, fn, msg)
    # the environment camera reads no window and no focal distance: garbage there is no refusal of the model (the call goes on to ask for a device, or to the sampler)
    for fn, rc, msg in call(model=2, edit={16: np.nan, 17: np.nan, 21: -1.0}, dims=1):
        assert rc == RT_ERR_INVALID and "dimensions" in msg, (fn, rc, msg)
    # flags of rt_camera_model_rays other than RT_FLAG_FILM_ON_DEVICE | RT_FLAG_RAY_DIFFERENTIALS, and null pointers
    cam = host.camera_model("environment", camera_to_world(), NX, NY)
    film = FilmDesc()
    film.cropped_pixel_bounds[:] = [0, 0, NX, NY]
    smp = SamplerDesc(NS, 4)
    for flags, camera, where in ((4, cam.ctypes.data_as(C.c_void_p), "flags"), (0, None, "null")):
        rc = L.rt_camera_model_rays(scene, 2, camera, C.byref(film), C.byref(smp), 0, NS, flags, None, sink.ctypes.data_as(C.c_void_p), None)
        assert rc == RT_ERR_INVALID and where in L.rt_last_error().decode()
    rc = L.rt_camera_model_rays(scene, 2, cam.ctypes.data_as(C.c_void_p), C.byref(film), C.byref(smp), 2, NS, 0, None, sink.ctypes.data_as(C.c_void_p), None)
    assert rc == RT_ERR_INVALID and "sample0" in L.rt_last_error().decode()


def test_the_producers_are_kernels_of_their_own_translation_unit_and_stream(host):
    """k_camera_model_rays and its masked form are in the library beside k_camera_rays: no scratch, no spill, no LDS, at most 96 VGPRs (five waves per SIMD: the
    argument reduction of sinf / cosf is what they hold beyond k_camera_rays' 59)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_budget", os.path.join(ROOT, "scripts", "kernel_budget.py"))
    kb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kb)
    res = kb.kernel_resources(host.HIP_LIB)
    assert "rtx::k_camera_rays" in res
    for k in ("rtx::k_camera_model_rays", "rtx::k_camera_model_rays_masked"):
        r = res[k]
        print(k, r)
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["lds"] == 0 and r["vgpr"] <= 96 and r["agpr"] == 0, (k, r)
