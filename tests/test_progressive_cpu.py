"""Progressive frames (rt_frame_* / rtxh_frame_* / HostScene.progressive) without a GPU: the entry points are declared, exported, spelled out for the Rust binding
and wrapped by the Python host layer; every refusal of rt_frame_begin precedes any device work, so a machine without a GPU gives the same code and message; the two
new film kernels keep the register budget of the film kernel they restate."""
import ctypes as C
import importlib.util
import os

from test_abi_cpu import parse_c_prototypes, parse_rust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1
RT_FLAG_REF_STREAM = 16


class Camera(C.Structure):
    _fields_ = [("raster_to_camera", C.c_float * 16), ("camera_to_world", C.c_float * 16), ("dx_camera", C.c_float * 3), ("dy_camera", C.c_float * 3),
                ("lens_radius", C.c_float), ("focal_distance", C.c_float)]


class FilmDesc(C.Structure):
    _fields_ = [("cropped_pixel_bounds", C.c_int32 * 4), ("sample_bounds", C.c_int32 * 4), ("filter_radius", C.c_float * 2), ("filter_table", C.c_float * 256),
                ("max_sample_luminance", C.c_float)]


class SamplerDesc(C.Structure):
    _fields_ = [("spp", C.c_int32), ("dimensions", C.c_int32)]


class PathDesc(C.Structure):
    _fields_ = [("max_depth", C.c_int32), ("rr_threshold", C.c_float), ("light_strategy", C.c_int32), ("pixel_bounds", C.c_int32 * 4)]


class Shard(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world_size", C.c_int32)]


def test_entry_points_are_declared_exported_documented_and_wrapped(host):
    hip = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_hip.h"))
    hosth = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_host.h"))
    assert hip["rt_frame_begin"] == ("i32", ["*rt_scene", "*rt_camera", "*rt_film_desc", "*rt_sampler_desc", "*rt_path_desc", "*rt_shard", "u32", "u64", "**rt_frame"])
    assert hip["rt_frame_advance"] == ("i32", ["*rt_frame", "i32", "*c_void", "*rt_stats"])
    assert hip["rt_frame_read"] == ("i32", ["*rt_frame", "i32", "f32", "u32", "*c_void", "*c_void"])
    assert hip["rt_frame_query"] == ("i32", ["*rt_frame", "i32", "*u64"])
    assert hip["rt_frame_end"] == ("c_void", ["*rt_frame"])
    assert hosth["rtxh_frame_begin"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "u64", "**rtxh_frame"])
    assert hosth["rtxh_frame_advance"] == ("i32", ["*rtxh_frame", "i32", "*c_void", "*rt_stats"])
    assert hosth["rtxh_frame_read"] == ("i32", ["*rtxh_frame", "i32", "f32", "u32", "*c_void", "*c_void"])
    assert hosth["rtxh_frame_query"] == ("i32", ["*rtxh_frame", "i32", "*u64"])
    assert hosth["rtxh_frame_end"] == ("c_void", ["*rtxh_frame"])
    _, fns = parse_rust(os.path.join(ROOT, "INTEGRATION.md"))   # (tests/test_abi_cpu.py then holds their argument types to the header's)
    for name in ("begin", "advance", "read", "query", "end"):
        assert hasattr(host.hip_lib(), "rt_frame_" + name), name
        assert hasattr(host.lib(), "rtxh_frame_" + name), name
        assert "rt_frame_" + name in fns, name
    assert "render_mi355x_progressive" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert callable(host.HostScene.progressive) and callable(host.PbrtScene.progressive)
    for m in ("advance", "film", "rgb", "display", "close", "__enter__", "__exit__"):
        assert callable(getattr(host.ProgressiveFrame, m)), m
    for m in ("samples_done", "spp", "tables_resident"):
        assert isinstance(getattr(host.ProgressiveFrame, m), property), m
    assert (host.RT_FRAME_XYZW, host.RT_FRAME_RGB, host.RT_FRAME_RGB8) == (0, 1, 2)
    assert (host.RT_FRAME_SAMPLES_DONE, host.RT_FRAME_SPP, host.RT_FRAME_TABLES_RESIDENT, host.RT_FRAME_STATE_BYTES) == (0, 1, 2, 3)
    for doc in ("README.md", "DESIGN.md"):
        assert "rt_frame_begin" in open(os.path.join(ROOT, doc)).read(), doc


def _descriptions():
    cam, film, smp, path = Camera(), FilmDesc(), SamplerDesc(16, 4), PathDesc()
    film.cropped_pixel_bounds[:] = [0, 0, 32, 32]
    film.sample_bounds[:] = [0, 0, 32, 32]
    film.filter_radius[:] = [0.5, 0.5]
    path.max_depth, path.pixel_bounds[:] = 5, [0, 0, 32, 32]
    return cam, film, smp, path


def test_rt_frame_begin_refuses_before_any_device_work(host):
    """Each refusal has its own message and needs no device: the scene handle is a dummy that is never looked at."""
    L = host.hip_lib()
    L.rt_frame_begin.restype = C.c_int
    L.rt_frame_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)

    def begin(flags=0, spp=16, dims=4, shard=None, film_edit=None, null_out=False):
        cam, film, smp, path = _descriptions()
        smp.spp, smp.dimensions = spp, dims
        if film_edit:
            film_edit(film)
        out = C.c_void_p(0x1234)
        rc = L.rt_frame_begin(scene, C.byref(cam), C.byref(film), C.byref(smp), C.byref(path), None if shard is None else C.byref(shard), flags, 0,
                              None if null_out else C.byref(out))
        assert null_out or out.value is None, "a refused call leaves no handle"
        return rc, L.rt_last_error().decode()

    def empty_crop(f):
        f.cropped_pixel_bounds[:] = [8, 8, 8, 20]

    def empty_samples(f):
        f.sample_bounds[:] = [0, 0, 32, 0]

    cases = {"ref stream": (dict(flags=RT_FLAG_REF_STREAM), "reference-stream"),
             "spp": (dict(spp=16385), "spp > 16384"),
             "spp huge": (dict(spp=2**31 - 1), "spp > 16384"),
             "dims low": (dict(dims=1), "dimensions"),
             "dims high": (dict(dims=9), "dimensions"),
             "shard rank": (dict(shard=Shard(2, 2)), "bad shard"),
             "shard negative": (dict(shard=Shard(-1, 2)), "bad shard"),
             "shard world": (dict(shard=Shard(0, 0)), "bad shard"),
             "empty crop": (dict(film_edit=empty_crop), "empty film"),
             "empty sample bounds": (dict(film_edit=empty_samples), "empty film"),
             "null out": (dict(null_out=True), "NULL out")}
    seen = {}
    for name, (kw, word) in cases.items():
        rc, msg = begin(**kw)
        assert rc == RT_ERR_INVALID and msg.startswith("rt_frame_begin") and word in msg, (name, rc, msg)
        seen[word] = msg
    assert len(set(seen.values())) == len(seen), seen   # one message per kind of refusal


def test_frame_calls_on_null_handles(host):
    L, H = host.hip_lib(), host.lib()
    L.rt_frame_end.restype = None
    L.rt_frame_end.argtypes = [C.c_void_p]
    L.rt_frame_end(None)   # returns
    H.rtxh_frame_end.restype = None
    H.rtxh_frame_end.argtypes = [C.c_void_p]
    H.rtxh_frame_end(None)
    v = C.c_uint64()
    buf = C.create_string_buffer(64)
    assert L.rt_frame_advance(None, C.c_int32(4), None, None) == RT_ERR_INVALID and L.rt_last_error()
    assert L.rt_frame_read(None, C.c_int32(0), C.c_float(1.0), C.c_uint32(0), None, buf) == RT_ERR_INVALID
    assert L.rt_frame_query(None, C.c_int32(0), C.byref(v)) == RT_ERR_INVALID
    assert H.rtxh_frame_advance(None, C.c_int32(4), None, None) == RT_ERR_INVALID and H.rtxh_last_error()
    assert H.rtxh_frame_begin(None, None, C.c_uint64(0), None) == RT_ERR_INVALID


def test_frame_kernels_keep_the_film_kernels_budget(host):
    """k_film_accumulate_frame shares its body with k_film_accumulate and stays inside the same 96 VGPRs without scratch; the resolve kernel is a per-pixel
    stream (16-byte loads, no scratch)."""
    spec = importlib.util.spec_from_file_location("kernel_budget", os.path.join(ROOT, "scripts", "kernel_budget.py"))
    kb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kb)
    res = kb.kernel_resources(host.HIP_LIB)
    for name, vg in (("rtx::k_film_accumulate", 96), ("rtx::k_film_accumulate_frame", 96), ("rtx::k_frame_resolve", 64)):
        r = res[name]
        print(f"\n{name}: {r}")
        assert r["vgpr"] <= vg and r["agpr"] == 0 and r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
