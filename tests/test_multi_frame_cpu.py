"""Progressive frames across the workers of an rt_multi (rt_multi_frame_* / rtxh_multi_frame_* / HostScene.progressive_multi) without a GPU: the twelve entry points
are declared with the agreed prototypes, exported, spelled out for the Rust binding and wrapped by the Python host layer; NULL handles are refused by both layers
with a message before any device is touched; the kernels of the merged read-out are plain streams - no scratch, no LDS - and the resolve kernel they share their
arithmetic with keeps its figures."""
import ctypes as C
import importlib.util
import os
import re

from test_abi_cpu import parse_c_prototypes, parse_rust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1
NAMES = ("begin", "advance", "advance_adaptive", "read", "query", "end")


def test_entry_points_are_declared_exported_documented_and_wrapped(host):
    hip = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_hip.h"))
    hosth = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_host.h"))
    assert hip["rt_multi_frame_begin"] == ("i32", ["*rt_multi", "*rt_camera", "*rt_film_desc", "*rt_sampler_desc", "*rt_path_desc", "u32", "u64", "**rt_multi_frame"])
    assert hip["rt_multi_frame_advance"] == ("i32", ["*rt_multi_frame", "i32", "*rt_stats", "*rt_stats"])
    assert hip["rt_multi_frame_advance_adaptive"] == ("i32", ["*rt_multi_frame", "i32", "f32", "f32", "i32", "*rt_stats", "*rt_stats"])
    assert hip["rt_multi_frame_read"] == ("i32", ["*rt_multi_frame", "i32", "f32", "u32", "*c_void"])
    assert hip["rt_multi_frame_query"] == ("i32", ["*rt_multi_frame", "i32", "*u64"])
    assert hip["rt_multi_frame_end"] == ("c_void", ["*rt_multi_frame"])
    assert hosth["rtxh_multi_frame_begin"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "*i32", "i32", "u64", "**rtxh_multi_frame"])
    assert hosth["rtxh_multi_frame_advance"] == ("i32", ["*rtxh_multi_frame", "i32", "*rt_stats", "*rt_stats"])
    assert hosth["rtxh_multi_frame_advance_adaptive"] == ("i32", ["*rtxh_multi_frame", "i32", "f32", "f32", "i32", "*rt_stats", "*rt_stats"])
    assert hosth["rtxh_multi_frame_read"] == ("i32", ["*rtxh_multi_frame", "i32", "f32", "u32", "*c_void"])
    assert hosth["rtxh_multi_frame_query"] == ("i32", ["*rtxh_multi_frame", "i32", "*u64"])
    assert hosth["rtxh_multi_frame_end"] == ("c_void", ["*rtxh_multi_frame"])
    _, fns = parse_rust(os.path.join(ROOT, "INTEGRATION.md"))   # (tests/test_abi_cpu.py then holds their argument types to the header's)
    for name in NAMES:
        assert hasattr(host.hip_lib(), "rt_multi_frame_" + name), name
        assert hasattr(host.lib(), "rtxh_multi_frame_" + name), name
        assert "rt_multi_frame_" + name in fns, name
    assert fns["rt_multi_frame_begin"] == ("i32", ["*RtMulti", "*RtCamera", "*RtFilmDesc", "*RtSamplerDesc", "*RtPathDesc", "u32", "u64", "**rt_multi_frame"])
    assert fns["rt_multi_frame_advance_adaptive"] == ("i32", ["*rt_multi_frame", "i32", "f32", "f32", "i32", "*RtStats", "*RtStats"])
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"rt_multi_frame_advance_adaptive\(frame,", text) and re.search(r"rt_multi_frame_read\(frame,", text), "INTEGRATION.md shows a usage loop"
    for cls in (host.HostScene, host.PbrtScene):
        assert callable(cls.progressive_multi)
        for arg in ("devices", "table_budget", "count_traversal", "time_kernels", "pixel_stats"):
            assert arg in cls.progressive_multi.__code__.co_varnames, (cls, arg)
    for m in ("advance", "advance_adaptive", "film", "rgb", "display", "pixel_stats", "noise", "close", "__enter__", "__exit__"):
        assert callable(getattr(host.MultiProgressiveFrame, m)), m
    for m in ("samples_done", "spp", "tables_resident", "state_bytes", "samples_taken", "active_pixels"):
        assert isinstance(getattr(host.MultiProgressiveFrame, m), property), m
    header = open(os.path.join(ROOT, "include", "rtx_hip.h")).read()
    assert "A MULTI FRAME MUST BE ENDED BEFORE rt_multi_destroy" in header and "A FRAME MUST BE ENDED BEFORE ITS SCENE IS DESTROYED" in header
    for doc in ("README.md", "DESIGN.md"):
        assert "rt_multi_frame_begin" in open(os.path.join(ROOT, doc)).read(), doc


def test_null_handles_are_refused_with_a_message_and_end_returns(host):
    """No device is touched: the machine that runs this has none, and every call answers RT_ERR_INVALID with a message that names the call."""
    L, H = host.hip_lib(), host.lib()
    v = C.c_uint64()
    buf = C.create_string_buffer(64)
    out = C.c_void_p(0x1234)
    for lib_, prefix, last in ((L, "rt_multi_frame_", L.rt_last_error), (H, "rtxh_multi_frame_", H.rtxh_last_error)):
        end = getattr(lib_, prefix + "end")
        end.restype = None
        end.argtypes = [C.c_void_p]
        end(None)   # returns
        adv = getattr(lib_, prefix + "advance")
        adv.restype = C.c_int
        adv.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        ada = getattr(lib_, prefix + "advance_adaptive")
        ada.restype = C.c_int
        ada.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]
        rd = getattr(lib_, prefix + "read")
        rd.restype = C.c_int
        rd.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_uint32, C.c_void_p]
        qu = getattr(lib_, prefix + "query")
        qu.restype = C.c_int
        qu.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        for name, call in (("advance", lambda: adv(None, 4, None, None)), ("advance_adaptive", lambda: ada(None, 4, 0.05, 1e-3, 4, None, None)),
                           ("read", lambda: rd(None, 0, 1.0, 0, buf)), ("query", lambda: qu(None, 0, C.byref(v)))):
            rc = call()
            msg = last().decode()
            print(f"\n{prefix}{name}(NULL): {rc}, {msg!r}")
            assert rc == RT_ERR_INVALID and (prefix + name) in msg and "null" in msg, (name, rc, msg)
    # begin: a NULL multi leaves no handle, a NULL out is refused
    L.rt_multi_frame_begin.restype = C.c_int
    L.rt_multi_frame_begin.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_uint64, C.c_void_p]
    rc = L.rt_multi_frame_begin(None, buf, buf, buf, buf, 0, 0, C.byref(out))
    msg = L.rt_last_error().decode()
    print(f"\nrt_multi_frame_begin(NULL multi): {rc}, {msg!r}")
    assert rc == RT_ERR_INVALID and out.value is None and msg.startswith("rt_multi_frame_begin") and "multi" in msg
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    rc = L.rt_multi_frame_begin(dummy, buf, buf, buf, buf, 0, 0, None)
    msg = L.rt_last_error().decode()
    assert rc == RT_ERR_INVALID and msg.startswith("rt_multi_frame_begin") and "NULL out" in msg, (rc, msg)
    H.rtxh_multi_frame_begin.restype = C.c_int
    H.rtxh_multi_frame_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p]
    out = C.c_void_p(0x1234)
    rc = H.rtxh_multi_frame_begin(None, None, None, 0, 0, C.byref(out))
    assert rc == RT_ERR_INVALID and out.value is None and H.rtxh_last_error().decode().startswith("rtxh_multi_frame_begin")
    assert H.rtxh_multi_frame_begin(dummy, buf, buf, 1, 0, None) == RT_ERR_INVALID and "NULL out" in H.rtxh_last_error().decode()


def test_the_merge_kernels_are_plain_streams_and_the_resolve_kernel_keeps_its_figures(host):
    """k_multi_frame_pack and k_multi_frame_resolve (and the statistics gather beside them): no scratch, no LDS, no spills, no accumulation registers, inside the 64
    VGPRs their siblings are held to. k_frame_resolve now calls the shared read-out function: its figures are the ones it had with the arithmetic written out -
    26 VGPRs, no scratch, no LDS."""
    spec = importlib.util.spec_from_file_location("kernel_budget", os.path.join(ROOT, "scripts", "kernel_budget.py"))
    kb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kb)
    res = kb.kernel_resources(host.HIP_LIB)
    for name, vg in (("rtx::k_multi_frame_pack", 64), ("rtx::k_multi_frame_resolve", 64), ("rtx::k_multi_frame_stats_read", 64), ("rtx::k_frame_resolve", 26)):
        r = res[name]
        print(f"\n{name}: {r}")
        assert r["vgpr"] <= vg and r["agpr"] == 0 and r["scratch"] == 0 and r["lds"] == 0 and r["vgpr_spills"] == 0, (name, r)
