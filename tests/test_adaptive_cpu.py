"""Frame statistics and adaptive steps (RT_FLAG_FRAME_STATS, rt_frame_read(RT_FRAME_STATS), rt_frame_advance_adaptive / rtxh_frame_advance_adaptive,
ProgressiveFrame.advance_adaptive) without a GPU: the entry point is declared with the agreed prototype, exported, spelled out for the Rust binding, documented and
wrapped; a NULL handle is refused by both layers with a message; the new kernels take no scratch, spill nothing, use no accumulation registers, and the stats film
kernel stays inside the 96 VGPRs its sibling is held to."""
import ctypes as C
import importlib.util
import os
import re

from test_abi_cpu import parse_c_prototypes, parse_rust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1


def test_the_adaptive_entry_point_is_declared_exported_documented_and_wrapped(host):
    hip = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_hip.h"))
    hosth = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_host.h"))
    assert hip["rt_frame_advance_adaptive"] == ("i32", ["*rt_frame", "i32", "f32", "f32", "i32", "*c_void", "*rt_stats"])
    assert hosth["rtxh_frame_advance_adaptive"] == ("i32", ["*rtxh_frame", "i32", "f32", "f32", "i32", "*c_void", "*rt_stats"])
    assert hasattr(host.hip_lib(), "rt_frame_advance_adaptive") and hasattr(host.lib(), "rtxh_frame_advance_adaptive")
    _, fns = parse_rust(os.path.join(ROOT, "INTEGRATION.md"))   # (tests/test_abi_cpu.py then holds its argument types to the header's)
    assert fns["rt_frame_advance_adaptive"] == ("i32", ["*rt_frame", "i32", "f32", "f32", "i32", "*c_void", "*RtStats"])
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"rt_frame_advance_adaptive\(frame,", text), "INTEGRATION.md shows a usage loop"
    for m in ("advance_adaptive", "pixel_stats", "noise"):
        assert callable(getattr(host.ProgressiveFrame, m)), m
    for m in ("samples_taken", "active_pixels"):
        assert isinstance(getattr(host.ProgressiveFrame, m), property), m
    for cls in (host.HostScene, host.PbrtScene):
        assert "pixel_stats" in cls.progressive.__code__.co_varnames, cls
    for doc in ("README.md", "DESIGN.md"):
        assert "rt_frame_advance_adaptive" in open(os.path.join(ROOT, doc)).read(), doc


def test_constants(host):
    assert host.RT_FLAG_FRAME_STATS == 32 and host.RT_FRAME_STATS == 3
    assert (host.RT_FRAME_SAMPLES_TAKEN, host.RT_FRAME_ACTIVE_PIXELS) == (4, 5)
    src = open(os.path.join(ROOT, "include", "rtx_hip.h")).read()
    assert re.search(r"#define\s+RT_FLAG_FRAME_STATS\s+32u", src)
    for name, value in (("RT_FRAME_STATS", 3), ("RT_FRAME_SAMPLES_TAKEN", 4), ("RT_FRAME_ACTIVE_PIXELS", 5)):
        assert re.search(name + r"\s*=\s*%d\b" % value, src), name
    # the earlier values stay where they were
    assert (host.RT_FRAME_XYZW, host.RT_FRAME_RGB, host.RT_FRAME_RGB8) == (0, 1, 2)
    assert (host.RT_FRAME_SAMPLES_DONE, host.RT_FRAME_SPP, host.RT_FRAME_TABLES_RESIDENT, host.RT_FRAME_STATE_BYTES) == (0, 1, 2, 3)


def test_null_handles_are_refused_with_a_message(host):
    L, H = host.hip_lib(), host.lib()
    for lib_, fn, last in ((L, "rt_frame_advance_adaptive", L.rt_last_error), (H, "rtxh_frame_advance_adaptive", H.rtxh_last_error)):
        f = getattr(lib_, fn)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]
        rc = f(None, 4, 0.05, 1e-3, 4, None, None)
        msg = last().decode()
        print(f"\n{fn}(NULL): {rc}, {msg!r}")
        assert rc == RT_ERR_INVALID and fn in msg and "null frame" in msg, (fn, rc, msg)


def test_the_new_kernels_take_no_scratch_and_the_stats_film_kernel_keeps_the_budget(host):
    spec = importlib.util.spec_from_file_location("kernel_budget", os.path.join(ROOT, "scripts", "kernel_budget.py"))
    kb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kb)
    res = kb.kernel_resources(host.HIP_LIB)
    for name, vg in (("rtx::k_film_accumulate_frame_stats", 96), ("rtx::k_raygen_masked", 128), ("rtx::k_frame_active", 64), ("rtx::k_frame_stats_read", 64)):
        r = res[name]
        print(f"\n{name}: {r}")
        assert r["vgpr"] <= vg and r["agpr"] == 0 and r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
    # the moments live in registers while a lane walks its samples: no LDS either (the compiler promotes a private array, such as a record's padding, to LDS)
    assert res["rtx::k_film_accumulate_frame_stats"]["lds"] == 0
