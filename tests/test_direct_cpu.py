"""The direct-lighting integrator without a GPU: the margins of every batch tests/test_gpu_direct.py compares (asserted on the float64 model alone), the model's replay
of the sampler's tables against the oracle's, the model's estimator against a closed-form irradiance, rt_direct_plan on numbers, the C boundary - rt_direct_desc in the
header, the ctypes mirror, the Rust declarations of INTEGRATION.md, the exported symbols - and every refusal with its message. No test here touches a device.
rt_direct_desc is declared as `struct rt_direct_desc {..}; typedef struct rt_direct_desc rt_direct_desc;` and its Rust mirror stands in a block of its own, as
rt_whitted_desc's does."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import direct_cases as dc
import direct_model as dm
import whitted_model as wm
from test_abi_cpu import parse_c_prototypes, _strip_comments
from test_ao_cpu import SamplerDesc, _header_struct, _rust_fn_types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID, RT_ERR_UNSUPPORTED = -1, -5
RT_FLAG_REF_STREAM = 16
RUN_IDS = [(name, md, dims, sname) for name in dc.CASES for md, dims in dc.RUNS[name] for sname, _ in dc.STRATEGIES]


# ---------------------------------------------------------------- the batches
@pytest.mark.parametrize("name", list(dc.CASES))
def test_every_ray_of_every_batch_keeps_its_distance_from_a_decision(orc, name):
    """After settling - from the salts of tests/golden/direct_salts.npz, so nothing moves - NO sample of any run of the case violates a margin: every sample is compared
    on the GPU, none is left out. The glass runs under "all" hold samples that exhaust their arrays (more than max_depth vertices reach uniform_sample_all_light) beside
    samples that do not."""
    dc.settled(orc, name)
    moved = dc._cache[("salt", name)]
    with np.load(dc.SALTS) as z:
        assert np.array_equal(z[name].astype(int), moved), "the committed salts are where the settling ends"
    for md, dims in dc.RUNS[name]:
        for sname, _ in dc.STRATEGIES:
            res, (b, rays) = dc.reference(orc, name, md, dims, sname)
            bad = dc.violations(res)
            print(f"{name} max_depth {md} dimensions {dims} {sname}: violations {int(bad.sum())}; margins edge {res.edge.min():.2e} shadow {res.shadow.min():.2e} sin2 {res.sin2.min():.2e} "
                  f"grazing {res.grazing.min():.3f} pick {res.pick.min():.2e}; nodes up to {res.nodes.max()}, array vertices {res.verts.min()} .. {res.verts.max()}, "
                  f"segments {res.n_shadow}, probes {res.n_probe}, salts up to {moved.max()}")
            assert not bad.any()
            assert res.n_shadow > 0 and np.isfinite(res.L).all() and res.L.max() > 0
            if name in ("glass", "glass_triangles") and sname == "all":
                hit = res.verts > 0
                assert (res.verts > md).any() and (hit & (res.verts <= md)).any(), "some samples exhaust their arrays and some do not"
                assert (res.draws[res.verts > md] > 2 * (res.nodes[res.verts > md] - 1)).any()   # exhausted: the lights' draws come from get_2d()
            if name in ("area", "glass", "glass_triangles", "mix", "many"):
                assert res.n_probe > 0
            if name == "floor":
                assert res.n_probe == 0
            if sname == "one":
                assert not res.verts.any() and res.draws1.max() >= 1
            else:
                assert not res.draws1.any()
    assert moved.max() <= dc.N_SALTS - 1


def test_many_is_288_arrays(orc):
    b, _ = dc.settled(orc, "many")
    assert dc.n_arrays(b, 3, dm.ALL) == 288 and dc.n_arrays(b, 3, dm.ONE) == 0


# ---------------------------------------------------------------- the sampler's tables
@pytest.mark.parametrize("spp,dims", [(4, 2), (4, 4), (4, 8), (16, 4), (5, 3)])
def test_the_replay_of_the_first_tables_is_the_oracles_bit_for_bit(orc, spp, dims):
    """The model's own sobol_2d / van_der_corput / shuffle over the pixel's raw draws (orc.rng_stream(pixel_index, n)) gives the oracle's 2 * dims tables, bit for bit,
    for 24 pixels - only then is its continuation, the array tables, trusted. The arrays are (0,2) tables too: every one holds each sample index' stratum once."""
    spp_r = 1
    while spp_r < spp:
        spp_r *= 2
    pixels = np.concatenate([np.arange(20), [959, 4095, 123456, 2 ** 31 + 7]])
    t1, t2, arr, retries = dm.replay_tables(orc, pixels, spp_r, dims, 6)
    for k, p in enumerate(pixels):
        o1, o2, _ = orc.sampler_tables(spp, dims, 1, int(p))
        assert np.array_equal(o1.view(np.uint32), t1[k].view(np.uint32)) and np.array_equal(o2.view(np.uint32), t2[k].view(np.uint32)), (spp, dims, int(p))
    strata = np.floor(arr[..., 0].astype(np.float64) * spp_r).astype(int)
    assert (np.sort(strata, axis=-1) == np.arange(spp_r)).all()      # the first coordinate is a van der Corput point set: one point per stratum of width 1 / spp
    assert len({a.tobytes() for a in arr[0]}) == 6                     # six different tables
    print(f"spp {spp} dims {dims}: 24 pixels equal the oracle's tables; retries met: {retries}")


def test_the_replay_takes_the_bounded_draws_retry(orc):
    """A pixel whose start_pixel stream holds a retried bounded draw (the oracle's scan names them) is replayed like any other."""
    with np.load(os.path.join(ROOT, "tests", "golden", "sampler_retry_pixels.npz")) as z:   # ~1e-5 of all pixels at 1024 spp (tests/golden/make_golden.py)
        hits = z["spp1024"][:2]
    assert len(hits) == 2 and all(len(orc.sampler_retry_scan(1024, 4, int(p), 1)) == 1 for p in hits)
    t1, t2, _, retries = dm.replay_tables(orc, hits, 1024, 4, 1)
    for k, p in enumerate(hits):
        o1, o2, _ = orc.sampler_tables(1024, 4, 1, int(p))
        assert np.array_equal(o1.view(np.uint32), t1[k].view(np.uint32)) and np.array_equal(o2.view(np.uint32), t2[k].view(np.uint32))
    print(f"pixels {list(hits)}: retries {retries}")
    assert retries >= len(hits)


def test_draws_leave_the_tables_into_one_stream_in_call_order():
    """get_1d() and get_2d() past the tables take from ONE stream in call order; a get_2d() returns (second draw, first draw)."""
    T1, T2 = np.arange(3, dtype=np.float32).reshape(1, 3) + 10, np.arange(6, dtype=np.float32).reshape(1, 3, 2) + 20
    R = np.arange(16, dtype=np.float32).reshape(1, 16)
    d = dm.Draws(T1, T2, np.zeros((1, 0, 2), np.float32), R, 3)
    ids = np.array([0])
    assert d.get_2d(ids).tolist() == [[24.0, 25.0]]          # 2-D table 2
    assert d.get_1d(ids).tolist() == [11.0] and d.get_1d(ids).tolist() == [12.0]   # 1-D tables 1, 2
    assert d.get_2d(ids).tolist() == [[1.0, 0.0]]            # the stream: (second, first)
    assert d.get_1d(ids).tolist() == [2.0]
    assert d.get_2d(ids).tolist() == [[4.0, 3.0]]
    assert (d.k2[0], d.k1[0], d.pos[0]) == (3, 3, 5)


# ---------------------------------------------------------------- the estimator against a closed form
def _corner_factor(a, b, h):
    """The form factor from a point to a rectangle a x b parallel to its plane at height h, one corner on the point's normal."""
    sa, sb = math.sqrt(a * a + h * h), math.sqrt(b * b + h * h)
    return (a / sa * math.atan(b / sa) + b / sb * math.atan(a / sb)) / (2.0 * math.pi)


def test_the_estimators_mean_is_the_closed_form_irradiance(monkeypatch):
    """A point of a matte floor (Kd 0.6) under a 3 x 3 emitter (two triangle lights, L = 5) one unit above it: the outgoing radiance is Kd L F with F the emitter's form
    factor, the sum of four corner rectangles. The mean of the "all" estimator over 160 000 samples with uniform random arrays agrees within 4 standard errors, which is
    under 1 % of the value; so do the light half alone and the BSDF half alone with the weights forced to 1."""
    sc = wm.Scene()
    sc.add_quad((-40, 0, -40), (-40, 0, 40), (40, 0, 40), (40, 0, -40), ("matte", 0.6))
    sc.add_quad((-1.5, 1.0, -1.0), (1.5, 1.0, -1.0), (1.5, 1.0, 2.0), (-1.5, 1.0, 2.0), ("matte", 0.0), emission=(5.0, 5.0, 5.0))   # normal -y
    px, pz = 0.3, 0.2
    F_exact = sum(_corner_factor(a, b, 1.0) for a in (1.5 + px, 1.5 - px) for b in (pz + 1.0, 2.0 - pz))
    exact = 0.6 * 5.0 * F_exact
    n = 160000
    o = np.tile(np.float64((px + 0.2, 0.5, pz - 0.3)), (n, 1))
    d = np.tile(np.float64((-0.2, -0.5, 0.3)), (n, 1))
    rng = np.random.default_rng(5)
    for tag, light, bsdf, mis in (("both halves, MIS", True, True, True), ("light half alone", True, False, False), ("BSDF half alone", False, True, False)):
        monkeypatch.setattr(dm, "LIGHT_HALF", light)
        monkeypatch.setattr(dm, "BSDF_HALF", bsdf)
        monkeypatch.setattr(dm, "MIS", mis)
        arr = rng.random((n, 4, 2)).astype(np.float32)
        dr = dm.Draws(np.zeros((n, 2), np.float32), np.zeros((n, 2, 2), np.float32), arr, np.zeros((n, 8), np.float32), 2)
        res = dm.render(sc, o, d, 1, dm.ALL, dr)
        mean, se = res.L[:, 0].mean(), res.L[:, 0].std() / math.sqrt(n)
        print(f"{tag}: mean {mean:.5f} +- {se:.5f}, closed form {exact:.5f} (F = {F_exact:.4f}); deviation {abs(mean - exact) / se:.2f} standard errors, 4 SE = {4 * se / exact:.3%}")
        assert (res.verts == 1).all() and (res.nodes == 1).all()
        assert 4 * se < 0.01 * exact and abs(mean - exact) <= 4 * se


# ---------------------------------------------------------------- the plan
def test_direct_plan_on_numbers(host):
    L = host.hip_lib()
    L.rt_direct_plan.restype = C.c_int
    L.rt_direct_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64] + [C.POINTER(C.c_uint64)] * 3
    bpp, chunk, stack = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def plan(md, nl, st, spp, pixels, budget, cap=1 << 14):
        rc = L.rt_direct_plan(md, nl, st, spp, pixels, cap, budget, C.byref(bpp), C.byref(chunk), C.byref(stack))
        return rc, bpp.value, chunk.value, stack.value
    GiB = 1 << 30
    for md, nl, spp in ((5, 2, 16), (3, 48, 4), (16, 32, 1024), (1, 1, 1)):
        A = 2 * md * nl
        rc, b, c, s = plan(md, nl, 0, spp, 1 << 19, GiB)
        assert rc == 0 and b == A * (spp * 2 + 8) and s == 64 * (md - 1) * (1 << 14), (md, nl, spp, rc, b, s)
        assert c * b <= GiB or c == 64
        assert c == 1 << 19 or 2 * c * b > GiB      # halved no further than needed
    assert plan(5, 2, 0, 5, 4096, GiB)[1] == 20 * (8 * 2 + 8)                     # spp rounded up to a power of two
    assert plan(5, 2, 1, 16, 4096, 1)[1:3] == (0, 4096)                          # "one": no arrays, nothing to cut
    assert plan(5, 2, 0, 16, 4096, 800 << 10)[2] == 1024                          # 800 B per pixel under 800 KiB
    assert plan(5, 2, 0, 16, 4096, 1)[2] == 64 and plan(5, 2, 0, 16, 40, 1)[2] == 40   # never below one workgroup's pixels
    rc = L.rt_direct_plan(3, 171, 0, 4, 4096, 1 << 14, GiB, None, None, None)
    assert rc == RT_ERR_UNSUPPORTED and "one" in L.rt_last_error().decode()
    assert L.rt_direct_plan(3, 170, 0, 4, 4096, 1 << 14, GiB, None, None, None) == 0   # 1020 arrays
    assert L.rt_direct_plan(3, 100000, 1, 4, 4096, 1 << 14, GiB, None, None, None) == 0
    for bad in ((0, 1, 0, 4), (5, 1, 2, 4), (5, -1, 0, 4), (5, 1, 0, 0)):
        assert L.rt_direct_plan(*bad, 4096, 1 << 14, GiB, None, None, None) == RT_ERR_INVALID, bad
    assert L.rt_direct_plan(17, 1, 0, 4, 4096, 1 << 14, GiB, None, None, None) == RT_ERR_UNSUPPORTED


# ---------------------------------------------------------------- the boundary
def test_rt_direct_desc_in_header_ctypes_rust_and_library_agree(host):
    src = _strip_comments(open(os.path.join(ROOT, "include", "rtx_hip.h")).read())
    fields = _header_struct(src, "rt_direct_desc")
    assert fields == [("int32_t", "max_depth"), ("int32_t", "strategy"), ("int32_t", "reserved[2]")], fields
    assert re.search(r"typedef struct rt_direct_desc rt_direct_desc;", src)
    assert [n for n, _ in host.DirectDesc._fields_] == ["max_depth", "strategy", "reserved"] and host.DirectDesc._fields_[2][1] is (C.c_int32 * 2) and host.DirectDesc._fields_[0][1] is C.c_int32
    assert C.sizeof(host.DirectDesc) == 16 and host.hip_lib().rt_sizeof(b"rt_direct_desc") == 16
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rust = _strip_comments("\n".join(re.findall(r"```rust\n(.*?)```", md, flags=re.S)))
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct RtDirectDesc\s*\{(.*?)\}", rust, flags=re.S)
    assert m, "INTEGRATION.md spells RtDirectDesc out"
    rs = [tuple(x.strip() for x in f.split(":")) for f in re.split(r",(?![^\[]*\])", m.group(1)) if f.strip()]
    assert rs == [("max_depth", "i32"), ("strategy", "i32"), ("reserved", "[i32; 2]")], rs
    defs = dict(re.findall(r"#define\s+(RT_DIRECT_\w+)\s+(\d+)", src))
    assert (int(defs["RT_DIRECT_ALL"]), int(defs["RT_DIRECT_ONE"])) == (host.RT_DIRECT_ALL, host.RT_DIRECT_ONE) == (0, 1)
    assert int(defs["RT_DIRECT_MAX_ARRAYS"]) == host.RT_DIRECT_MAX_ARRAYS == 1024 and int(defs["RT_DIRECT_INFO_WORDS"]) == host.RT_DIRECT_INFO_WORDS == 4
    assert re.search(r"RT_QUERY_DIRECT_LAUNCHED\s*=\s*9", src) and host.RT_QUERY_DIRECT_LAUNCHED == 9


def test_prototypes_are_declared_exported_documented_and_wrapped(host):
    hip = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_hip.h"))
    hosth = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_host.h"))
    assert hip["rt_render_rays_direct"] == ("i32", ["*rt_scene", "*f32", "i32", "i32", "i32", "i32", "*rt_sampler_desc", "*rt_direct_desc", "u32", "*c_void", "*f32", "*u32", "*rt_stats"])
    assert hip["rt_render_direct"] == ("i32", ["*rt_scene", "*rt_camera", "*rt_film_desc", "*rt_sampler_desc", "*rt_direct_desc", "*rt_shard", "u32", "*c_void", "*f32", "*rt_stats"])
    assert hip["rt_direct_plan"] == ("i32", ["i32", "i32", "i32", "i32", "u64", "u64", "u64", "*u64", "*u64", "*u64"])
    assert hosth["rtxh_render_rays_direct"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "*f32", "i32", "i32", "i32", "i32", "i32", "i32", "*c_void", "*f32", "*u32", "*rt_stats"])
    assert hosth["rtxh_render_direct"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "i32", "i32", "*c_void", "*f32", "*rt_stats"])
    for lib, names in ((host.hip_lib(), ("rt_render_rays_direct", "rt_render_direct", "rt_direct_plan")), (host.lib(), ("rtxh_render_rays_direct", "rtxh_render_direct"))):
        for n in names:
            assert hasattr(lib, n), n
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _rust_fn_types(md, "rt_render_rays_direct") == ["*mut RtScene", "*const f32", "i32", "i32", "i32", "i32", "*const RtSamplerDesc", "*const RtDirectDesc", "u32",
                                                          "*mut c_void", "*mut f32", "*mut u32", "*mut RtStats"]
    assert _rust_fn_types(md, "rt_render_direct") == ["*mut RtScene", "*const RtCamera", "*const RtFilmDesc", "*const RtSamplerDesc", "*const RtDirectDesc", "*const RtShard",
                                                     "u32", "*mut c_void", "*mut f32", "*mut RtStats"]
    sig = inspect.signature(host.HostScene.render_rays_direct).parameters
    assert list(sig)[:7] == ["self", "rays", "max_depth", "strategy", "sample0", "spp", "with_info"], list(sig)
    assert sig["max_depth"].default == 5 and sig["strategy"].default == "all" and sig["with_info"].default is False
    sig = inspect.signature(host.HostScene.render_direct).parameters
    assert list(sig)[:5] == ["self", "max_depth", "strategy", "rank", "world_size"] and sig["max_depth"].default == 5 and sig["strategy"].default == "all"


def test_every_refusal_answers_with_its_code_and_a_message_and_no_device(host):
    L = host.hip_lib()
    L.rt_render_rays_direct.restype = C.c_int
    L.rt_render_rays_direct.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_render_direct.restype = C.c_int
    L.rt_render_direct.argtypes = [C.c_void_p] * 6 + [C.c_uint32] + [C.c_void_p] * 3
    buf = C.create_string_buffer(4096)
    scene = C.cast(buf, C.c_void_p)   # never dereferenced: every check of these cases comes before the scene is looked at
    f = np.zeros(256, np.float32)
    p = f.ctypes.data_as(C.c_void_p)

    def desc(depth, strategy, reserved):
        d = host.DirectDesc(depth, strategy)
        d.reserved[0], d.reserved[1] = reserved
        return d

    def call(scene=scene, rays=p, w=2, h=2, s0=0, ns=2, spp=4, dims=4, has_smp=True, has_d=True, depth=5, strategy=0, reserved=(0, 0), flags=0, out=p):
        smp, dd = SamplerDesc(spp, dims), desc(depth, strategy, reserved)
        rc = L.rt_render_rays_direct(scene, rays, w, h, s0, ns, C.byref(smp) if has_smp else None, C.byref(dd) if has_d else None, flags, None, out, None, None)
        return rc, L.rt_last_error().decode()

    cases = dict(
        # what Whitted refuses
        null_scene=dict(scene=None), null_rays=dict(rays=None), null_sampler=dict(has_smp=False), null_out=dict(out=None),
        zero_width=dict(w=0), negative_height=dict(h=-1), zero_samples=dict(ns=0), negative_sample0=dict(s0=-1), range_past_spp=dict(s0=3, ns=2, spp=4),
        too_many_rays=dict(w=4096, h=4096, ns=16, spp=16), spp_too_large=dict(spp=16385, ns=1), dimensions_too_small=dict(dims=1), dimensions_too_large=dict(dims=9),
        ref_stream=dict(flags=RT_FLAG_REF_STREAM),
        # the integrator's own
        null_desc=dict(has_d=False), zero_depth=dict(depth=0), negative_depth=dict(depth=-2), strategy_two=dict(strategy=2), strategy_negative=dict(strategy=-1),
        reserved_first=dict(reserved=(1, 0)), reserved_second=dict(reserved=(0, -1)))
    for name, kw in cases.items():
        rc, msg = call(**kw)
        print(f"{name}: {rc} {msg!r}")
        assert rc == RT_ERR_INVALID and msg and "rt_render_rays_direct" in msg, (name, rc, msg)
    assert "strategy" in call(strategy=2)[1] and "reserved" in call(reserved=(1, 0))[1] and "max_depth" in call(depth=0)[1] and "reference-stream" in call(flags=RT_FLAG_REF_STREAM)[1]
    rc, msg = call(depth=17)
    print(f"depth 17: {rc} {msg!r}")
    assert rc == RT_ERR_UNSUPPORTED and "rt_render_rays_direct" in msg and "16" in msg

    def frame(scene=scene, cam=p, film=p, has_smp=True, spp=4, dims=4, has_d=True, depth=5, strategy=0, reserved=(0, 0), flags=0, out=p):
        smp, dd = SamplerDesc(spp, dims), desc(depth, strategy, reserved)
        rc = L.rt_render_direct(scene, cam, film, C.byref(smp) if has_smp else None, C.byref(dd) if has_d else None, None, flags, None, out, None)
        return rc, L.rt_last_error().decode()

    for name, kw in dict(null_scene=dict(scene=None), null_camera=dict(cam=None), null_film=dict(film=None), null_sampler=dict(has_smp=False), null_desc=dict(has_d=False),
                         null_film_out=dict(out=None), spp_too_large=dict(spp=16385), dimensions_too_small=dict(dims=1), zero_depth=dict(depth=0), strategy_two=dict(strategy=2),
                         reserved_set=dict(reserved=(0, 7)), ref_stream=dict(flags=RT_FLAG_REF_STREAM)).items():
        rc, msg = frame(**kw)
        print(f"rt_render_direct {name}: {rc} {msg!r}")
        assert rc == RT_ERR_INVALID and msg and "rt_render_direct" in msg, (name, rc, msg)
    rc, msg = frame(depth=17)
    assert rc == RT_ERR_UNSUPPORTED and "rt_render_direct" in msg

    # the host layer refuses the same before it uploads the scene (no device here: an upload would answer RT_ERR_NO_DEVICE), and so do the Python arguments
    from rustracer_amd.scenes import cornell_box
    hs = host.HostScene(cornell_box(8, 8, 4))
    rays = np.zeros((2, 2, 2, 8), np.float32)
    for kw in (dict(max_depth=0), dict(max_depth=17), dict(strategy=2), dict(sample0=3), dict(spp=5, sample0=7)):
        with pytest.raises(host.BackendError) as e:
            hs.render_rays_direct(rays, **kw)
        print(kw, e.value)
        assert "rtxh_render_rays_direct" in str(e.value) and "no HIP device" not in str(e.value)
    for kw in (dict(max_depth=0), dict(max_depth=2000), dict(strategy=5)):
        with pytest.raises(host.BackendError) as e:
            hs.render_direct(**kw)
        assert "rtxh_render_direct" in str(e.value) and "no HIP device" not in str(e.value)
    with pytest.raises(host.BackendError) as e:
        hs.render_direct(strategy="some")
    assert "'all' or 'one'" in str(e.value)
    with pytest.raises(host.BackendError):
        hs.render_rays_direct(np.zeros((2, 2, 2, 7), np.float32))
    with pytest.raises(host.BackendError):
        hs.render_rays_direct(rays, device_out=np.zeros((2, 2, 2, 4), np.float32))


def test_1282_lights_under_all_are_refused_and_the_message_names_one(host):
    """1282 listed lights need 2 * 1 * 1282 = 2564 sample arrays per pixel even at max_depth 1: RT_ERR_UNSUPPORTED before the scene is uploaded, and the message names
    strategy "one" - under which the same call goes on to the upload (here: no device)."""
    from rustracer_amd.scene_desc import SceneDesc
    s = SceneDesc()
    s.film.xres, s.film.yres = 8, 8
    s.sampler.spp, s.sampler.dims = 4, 4
    s.add_quad((-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1), s.matte(0.5))
    for k in range(1282):
        s.point_light((0.01 * k - 6.0, 3.0, 0.0), (1.0, 1.0, 1.0))
    hs = host.HostScene(s)
    rays = np.zeros((2, 2, 2, 8), np.float32)
    for call in (lambda: hs.render_rays_direct(rays, max_depth=1, strategy="all"), lambda: hs.render_direct(1, "all")):
        with pytest.raises(host.BackendError) as e:
            call()
        print(e.value)
        assert '"one"' in str(e.value) and "2564" in str(e.value) and "RT_DIRECT_MAX_ARRAYS" in str(e.value) and "no HIP device" not in str(e.value)
        assert e.value.code == RT_ERR_UNSUPPORTED if hasattr(e.value, "code") else True
    if not host.device_available():
        with pytest.raises(host.BackendError) as e:
            hs.render_rays_direct(rays, max_depth=1, strategy="one")
        assert "RT_DIRECT_MAX_ARRAYS" not in str(e.value)


@pytest.mark.parametrize("args,needle", [(["--direct=0"], "--direct MAXDEPTH must be >= 1"), (["--direct", "--whitted"], "give one of them"), (["--direct", "--ao", "4"], "give one of them"),
                                         (["--direct", "3", "--samples", "s.npy"], "does not combine"), (["--direct", "--devices", "0,1"], "does not combine"),
                                         (["--direct-strategy", "one"], "--direct-strategy needs --direct")])
def test_render_pbrt_refuses_what_does_not_combine_with_direct(args, needle):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_pbrt.py"), "nothing.pbrt", "out.pfm"] + args, capture_output=True, text=True)
    print(args, r.returncode, r.stderr.strip().splitlines()[-1:])
    assert r.returncode != 0 and needle in r.stderr


# ---------------------------------------------------------------- the kernels' allocation
@pytest.fixture(scope="module")
def resources(host):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_budget
    finally:
        sys.path.pop(0)
    return kernel_budget.kernel_resources(host.HIP_LIB)


@pytest.mark.parametrize("general", [False, True])
def test_vertex_kernel_keeps_two_waves_per_simd(resources, general):
    """k_direct_vertex is held to the bound of k_whitted_vertex and the generic shade kernel: at most 256 VGPRs and no accumulation registers (two waves per SIMD)."""
    g = "true" if general else "false"
    w = resources[f"rtx::k_direct_vertex<{g}>"]
    print(f"k_direct_vertex<{g}>", w, f"\nk_direct_probe<{g}>", resources[f"rtx::k_direct_probe<{g}>"], "\nk_sampler_array_tables", resources["rtx::k_sampler_array_tables"])
    assert w["vgpr"] <= 256 and w["agpr"] == 0 and w["lds"] <= 512
    assert resources[f"rtx::k_direct_probe<{g}>"]["vgpr_spills"] == 0
    assert resources["rtx::k_sampler_array_tables"]["scratch"] == 0 and resources["rtx::k_direct_info"]["scratch"] == 0
