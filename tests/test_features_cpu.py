"""First-hit feature planes (rt_render_sample_features / rtxh_render_sample_features, RT_FLAG_FRAME_FEATURES, rt_frame_read(RT_FRAME_FEATURES), HostScene.sample_features,
ProgressiveFrame.features) without a GPU: the entry point is declared with the agreed prototype in both headers, exported by both libraries, spelled out for the Rust
binding, documented and wrapped; the constants hold their values and the earlier ones keep theirs; a NULL scene and a NULL frame are refused by both layers with a message
that names the function; the new kernels take no scratch, spill nothing and use no LDS."""
import ctypes as C
import importlib.util
import os
import re

from test_abi_cpu import parse_c_prototypes, parse_rust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1


def test_the_entry_point_is_declared_exported_documented_and_wrapped(host):
    hip = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_hip.h"))
    hosth = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_host.h"))
    assert hip["rt_render_sample_features"] == ("i32", ["*rt_scene", "*rt_camera", "*rt_film_desc", "*rt_sampler_desc", "*rt_path_desc", "u32", "*c_void", "*f32"])
    assert hosth["rtxh_render_sample_features"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "*c_void", "*f32"])
    assert hasattr(host.hip_lib(), "rt_render_sample_features") and hasattr(host.lib(), "rtxh_render_sample_features")
    _, fns = parse_rust(os.path.join(ROOT, "INTEGRATION.md"))   # (tests/test_abi_cpu.py then holds its argument types to the header's)
    assert fns["rt_render_sample_features"] == ("i32", ["*RtScene", "*RtCamera", "*RtFilmDesc", "*RtSamplerDesc", "*RtPathDesc", "u32", "*c_void", "*f32"])
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"rt_frame_read\(frame, 4,", text), "INTEGRATION.md shows how the planes are read"
    assert "RT_FLAG_FRAME_FEATURES" in text
    assert callable(host.HostScene.sample_features) and callable(host.ProgressiveFrame.features) and callable(host.MultiProgressiveFrame.features)
    for cls in (host.HostScene, host.PbrtScene):
        assert "features" in cls.progressive.__code__.co_varnames and "features" in cls.progressive_multi.__code__.co_varnames, cls
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        t = open(os.path.join(ROOT, doc)).read()
        assert "rt_render_sample_features" in t and "RT_FLAG_FRAME_FEATURES" in t, doc
    assert "k_feature_hits" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "--features" in open(os.path.join(ROOT, "scripts", "render_pbrt.py")).read()


def test_constants(host):
    assert host.RT_FLAG_FRAME_FEATURES == 64 and host.RT_FRAME_FEATURES == 4 and host.RT_FEATURE_FLOATS == 16 and host.RT_FEATURE_SAMPLES_MAX == 2 ** 25
    src = open(os.path.join(ROOT, "include", "rtx_hip.h")).read()
    assert re.search(r"#define\s+RT_FLAG_FRAME_FEATURES\s+64u", src)
    assert re.search(r"#define\s+RT_FEATURE_FLOATS\s+16\b", src)
    assert int(re.search(r"#define\s+RT_FEATURE_SAMPLES_MAX\s+(\d+)", src).group(1)) == 2 ** 25
    assert re.search(r"RT_FRAME_FEATURES\s*=\s*4\b", src)
    # the earlier values stay where they were
    assert re.search(r"#define\s+RT_FLAG_FRAME_STATS\s+32u", src) and re.search(r"#define\s+RT_FLAG_REF_STREAM\s+16u", src)
    assert int(re.search(r"#define\s+RT_SAMPLES_MAX\s+(\d+)", src).group(1)) == 2 ** 27
    for name, value in (("RT_FRAME_XYZW", 0), ("RT_FRAME_RGB", 1), ("RT_FRAME_RGB8", 2), ("RT_FRAME_STATS", 3), ("RT_FRAME_SAMPLES_TAKEN", 4), ("RT_FRAME_ACTIVE_PIXELS", 5)):
        assert re.search(name + r"\s*=\s*%d\b" % value, src), name
    assert (host.RT_FLAG_FRAME_STATS, host.RT_FRAME_XYZW, host.RT_FRAME_RGB, host.RT_FRAME_RGB8, host.RT_FRAME_STATS) == (32, 0, 1, 2, 3)
    assert (host.RT_FRAME_SAMPLES_DONE, host.RT_FRAME_SPP, host.RT_FRAME_TABLES_RESIDENT, host.RT_FRAME_STATE_BYTES, host.RT_FRAME_SAMPLES_TAKEN, host.RT_FRAME_ACTIVE_PIXELS) == (0, 1, 2, 3, 4, 5)
    assert host.RT_SAMPLES_MAX == 2 ** 27


def test_null_handles_are_refused_with_a_message(host):
    L, H = host.hip_lib(), host.lib()
    out = (C.c_float * 16)()
    L.rt_render_sample_features.restype = C.c_int
    L.rt_render_sample_features.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p]
    rc = L.rt_render_sample_features(None, None, None, None, None, 0, None, out)
    msg = L.rt_last_error().decode()
    print(f"\nrt_render_sample_features(NULL scene): {rc}, {msg!r}")
    assert rc == RT_ERR_INVALID and "rt_render_sample_features" in msg and "null" in msg
    H.rtxh_render_sample_features.restype = C.c_int
    H.rtxh_render_sample_features.argtypes = [C.c_void_p] * 4
    rc = H.rtxh_render_sample_features(None, None, None, out)
    msg = H.rtxh_last_error().decode()
    print(f"rtxh_render_sample_features(NULL scene): {rc}, {msg!r}")
    assert rc == RT_ERR_INVALID and "rtxh_render_sample_features" in msg and "null" in msg
    # the planes of a NULL frame
    for lib_, fn, last, args in ((L, "rt_frame_read", L.rt_last_error, (None, 4, 1.0, 0, None, out)), (H, "rtxh_frame_read", H.rtxh_last_error, (None, 4, 1.0, 0, None, out)),
                                 (L, "rt_multi_frame_read", L.rt_last_error, (None, 4, 1.0, 0, out)), (H, "rtxh_multi_frame_read", H.rtxh_last_error, (None, 4, 1.0, 0, out))):
        f = getattr(lib_, fn)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_uint32] + [C.c_void_p] * (len(args) - 4)
        rc = f(*args)
        msg = last().decode()
        print(f"{fn}(NULL frame, RT_FRAME_FEATURES): {rc}, {msg!r}")
        assert rc == RT_ERR_INVALID and fn in msg and "null" in msg, (fn, rc, msg)


def test_the_new_kernels_take_no_scratch_no_lds_and_spill_nothing(host):
    spec = importlib.util.spec_from_file_location("kernel_budget", os.path.join(ROOT, "scripts", "kernel_budget.py"))
    kb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kb)
    res = kb.kernel_resources(host.HIP_LIB)
    # the plain form of the hit kernel is a triangle fill and four stores; the general form holds the quadric and the instance fill inline (three waves per SIMD at 168)
    want = {"rtx::k_feature_hits<false, false>": 64, "rtx::k_feature_hits<true, false>": 64, "rtx::k_feature_hits<false, true>": 168, "rtx::k_feature_hits<true, true>": 168,
            "rtx::k_feature_albedo<false>": 32, "rtx::k_feature_albedo<true>": 32, "rtx::k_feature_accumulate": 64, "rtx::k_frame_features_read<false>": 32,
            "rtx::k_frame_features_read<true>": 32}
    for name, vg in want.items():
        r = res[name]
        print(f"\n{name}: {r}")
        assert r["vgpr"] <= vg and r["agpr"] == 0 and r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["lds"] == 0, (name, r)
