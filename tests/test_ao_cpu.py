"""The ambient-occlusion and normal integrators (rt_render_rays_ao, rt_render_ao) without a GPU: the numpy model's own properties, the C boundary - rt_ao_desc in the
header, the ctypes mirror, the Rust declarations of INTEGRATION.md, the exported symbols, every refusal answered with RT_ERR_INVALID and a message before any device
work (the scene pointer is a dummy that is never dereferenced) - and the register budget of the new kernels, read from the built code object.

rt_ao_desc is declared as `struct rt_ao_desc {..}; typedef struct rt_ao_desc rt_ao_desc;` and its Rust mirror in a block of its own: tests/test_abi_cpu.py holds the
set of `typedef struct .. {` records of the header and of the first Rust block to a fixed list, so the new record is parsed here."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

import ao_model
from test_abi_cpu import parse_c_prototypes, _strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1
RT_FLAG_REF_STREAM = 16
EPS = 2.0 ** -24


class SamplerDesc(C.Structure):
    _fields_ = [("spp", C.c_int32), ("dimensions", C.c_int32)]


# ---------------------------------------------------------------- the model
def test_model_directions_are_unit_and_on_the_normals_side():
    rng = np.random.default_rng(7)
    u = rng.random((4096, 2)).astype(np.float32)
    u[:4] = [(0, 0), (0.5, 0.25), (1 - 2.0 ** -24, 1 - 2.0 ** -24), (0.5, 0.5)]
    n = np.float64((0.3, -0.8, 0.52))
    n /= np.linalg.norm(n)
    w, dn = ao_model.ao_directions(u, n)
    length = np.linalg.norm(w.astype(np.float64), axis=1)
    print("max | |w| - 1 | =", np.abs(length - 1).max() / EPS, "x 2^-24")
    assert np.abs(length - 1).max() <= 4 * EPS   # z exact, r and the products rounded once each
    assert w.dtype == np.float32
    assert (w.astype(np.float64) @ n >= 0).all() and (dn < 0).sum() > 1000 and (dn > 0).sum() > 1000
    raw = ao_model.uniform_sample_sphere(u)
    assert np.array_equal(w[dn < 0], -raw[dn < 0]) and np.array_equal(w[dn >= 0], raw[dn >= 0])
    assert np.array_equal(raw[:, 2], np.float32(1) - np.float32(2) * u[:, 0])


def test_model_samples_come_from_the_tables_and_then_the_stream_second_draw_first(orc):
    spp, dims, pixel, s = 4, 4, 37, 3
    u = ao_model.sample_u(orc, spp, dims, pixel, s, 8)
    _, t2, _ = orc.sampler_tables(spp, dims, 1, pixel)
    _, f = orc.rng_stream(pixel * spp + s + (1 << 32), 12)
    assert np.array_equal(u[0], t2[2, s]) and np.array_equal(u[1], t2[3, s])           # k = 0, 1: 2D#2, 2D#3
    for j in range(6):                                                                  # k >= 2: (second, first) of the keyed stream
        assert u[2 + j, 0] == f[2 * j + 1] and u[2 + j, 1] == f[2 * j], j
    assert len({float(x) for x in f}) == 12
    u2 = ao_model.sample_u(orc, spp, 2, pixel, s, 3)                                   # dimensions = 2: no table is left after get_camera_sample
    assert np.array_equal(u2[:, 0], f[1:6:2]) and np.array_equal(u2[:, 1], f[0:6:2])


def test_model_value_is_one_divide():
    occ = np.array([[True, False, False], [False, False, False], [True, True, True]])
    assert np.array_equal(ao_model.ao_value(occ), np.float32([2, 3, 0]) / np.float32(3))


def test_model_rebuilds_the_interaction_from_the_oracles_hit_records(orc):
    """Geometry.from_hit_records names the primitive by the record's own (t, b0, b1): on the three record scenes of tests/test_gpu_ao.py its point and normal are the
    brute-force float64 closest hit's - every ray, the mesh with vertex normals, the sphere and the instanced object included."""
    import test_gpu_ao as g
    for name, (make, eye, (lo, hi)) in g.RECORD_SCENES.items():
        desc = make()
        geo = ao_model.Geometry(desc)
        rays = g._toward(eye, g._targets(lo, hi, 11))
        o, d = rays[..., 0:3].reshape(-1, 3).astype(np.float64), rays[..., 4:7].reshape(-1, 3).astype(np.float64)
        rec = orc.OracleScene(desc).trace(rays.reshape(-1, 8))
        hit = rec["prim"] >= 0
        t, p, n = geo.closest(o, d)
        q, nq, perr, res, _ = geo.from_hit_records(o, d, np.where(hit, rec["t"], 0.0), rec["b0"], rec["b1"])
        dn = (n * nq).sum(1)[hit]
        print(name, int(hit.sum()), "hits; |p - p'| <=", np.linalg.norm(p - q, axis=1)[hit].max(), "residual <=", res[hit].max(), "n . n' >=", dn.min(), "p_error <=", perr[hit].max())
        assert np.array_equal(hit, np.isfinite(t)) and hit.sum() >= 64
        assert np.linalg.norm(p - q, axis=1)[hit].max() < 1e-4 and res[hit].max() < 1e-4 and dn.min() > 1 - 1e-6
        assert 0 < perr[hit].max() < 1e-5
    down = ao_model.Geometry(g._mesh())
    assert sum(1 for pr in down.prims if pr[5] is not None) == 66 and all(pr[5][:, 1].max() < 0 for pr in down.prims if pr[5] is not None)


# ---------------------------------------------------------------- the boundary
def _header_struct(src, name):
    m = re.search(r"(?<!typedef )struct %s\s*\{(.*?)\}\s*;" % name, src, flags=re.S)
    return [tuple(d.split()) for d in m.group(1).split(";") if d.strip()]


def test_rt_ao_desc_in_header_ctypes_rust_and_library_agree(host):
    src = _strip_comments(open(os.path.join(ROOT, "include", "rtx_hip.h")).read())
    fields = _header_struct(src, "rt_ao_desc")
    assert fields == [("int32_t", "n_samples"), ("float", "max_distance")], fields
    assert re.search(r"typedef struct rt_ao_desc rt_ao_desc;", src)
    ct = {"int32_t": C.c_int32, "float": C.c_float}
    assert host.AoDesc._fields_ == [(n, ct[t]) for t, n in fields]
    assert C.sizeof(host.AoDesc) == 8 and host.hip_lib().rt_sizeof(b"rt_ao_desc") == 8
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rust = _strip_comments("\n".join(re.findall(r"```rust\n(.*?)```", md, flags=re.S)))
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct RtAoDesc\s*\{(.*?)\}", rust, flags=re.S)
    assert m, "INTEGRATION.md spells RtAoDesc out"
    rs = [tuple(x.strip() for x in f.split(":")) for f in m.group(1).split(",") if f.strip()]
    assert rs == [("n_samples", "i32"), ("max_distance", "f32")], rs
    defs = dict(re.findall(r"#define\s+(RT_AO_\w+)\s+(\d+)", src))
    assert int(defs["RT_AO_FLOATS"]) == host.RT_AO_FLOATS == 4 and int(defs["RT_AO_SAMPLES_MAX"]) == host.RT_AO_SAMPLES_MAX == 1024


def _rust_fn_types(md, name):
    rust = _strip_comments("\n".join(re.findall(r"```rust\n(.*?)```", md, flags=re.S)))
    m = re.search(r"fn %s\s*\((.*?)\)\s*->\s*i32;" % name, rust, flags=re.S)
    return [" ".join(a.split(":", 1)[1].split()) for a in m.group(1).split(",") if a.strip()]


def test_prototypes_are_declared_exported_documented_and_wrapped(host):
    hip = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_hip.h"))
    hosth = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_host.h"))
    assert hip["rt_render_rays_ao"] == ("i32", ["*rt_scene", "*f32", "i32", "i32", "i32", "i32", "*rt_sampler_desc", "*rt_ao_desc", "u32", "*c_void", "*f32", "*f32", "*rt_stats"])
    assert hip["rt_render_ao"] == ("i32", ["*rt_scene", "*rt_camera", "*rt_film_desc", "*rt_sampler_desc", "*rt_ao_desc", "*rt_shard", "u32", "*c_void", "*f32", "*rt_stats"])
    assert hosth["rtxh_render_rays_ao"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "*f32", "i32", "i32", "i32", "i32", "i32", "f32", "*c_void", "*f32", "*f32", "*rt_stats"])
    assert hosth["rtxh_render_ao"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "i32", "f32", "*c_void", "*f32", "*rt_stats"])
    for lib, names in ((host.hip_lib(), ("rt_render_rays_ao", "rt_render_ao")), (host.lib(), ("rtxh_render_rays_ao", "rtxh_render_ao"))):
        for n in names:
            assert hasattr(lib, n), n
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _rust_fn_types(md, "rt_render_rays_ao") == ["*mut RtScene", "*const f32", "i32", "i32", "i32", "i32", "*const RtSamplerDesc", "*const RtAoDesc", "u32", "*mut c_void",
                                                      "*mut f32", "*mut f32", "*mut RtStats"]
    assert _rust_fn_types(md, "rt_render_ao") == ["*mut RtScene", "*const RtCamera", "*const RtFilmDesc", "*const RtSamplerDesc", "*const RtAoDesc", "*const RtShard", "u32",
                                                 "*mut c_void", "*mut f32", "*mut RtStats"]
    p = list(inspect.signature(host.HostScene.render_rays_ao).parameters)
    assert p[:9] == ["self", "rays", "n_samples", "max_distance", "sample0", "spp", "with_rays", "device_out", "stream"], p
    p = list(inspect.signature(host.HostScene.render_ao).parameters)
    assert p[:5] == ["self", "n_samples", "max_distance", "rank", "world_size"], p
    assert inspect.signature(host.HostScene.render_ao).parameters["max_distance"].default == float("inf")


def test_every_refusal_answers_invalid_with_a_message_and_no_device(host):
    L = host.hip_lib()
    L.rt_render_rays_ao.restype = C.c_int
    L.rt_render_rays_ao.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
    L.rt_render_ao.restype = C.c_int
    L.rt_render_ao.argtypes = [C.c_void_p] * 6 + [C.c_uint32] + [C.c_void_p] * 3
    buf = C.create_string_buffer(4096)
    scene = C.cast(buf, C.c_void_p)   # never dereferenced: every check comes before the scene is looked at
    f = np.zeros(256, np.float32)
    p = f.ctypes.data_as(C.c_void_p)
    inf, nan = float("inf"), float("nan")

    def call(scene=scene, rays=p, w=2, h=2, s0=0, ns=2, spp=4, dims=4, has_smp=True, has_ao=True, n_ao=3, dist=inf, flags=0, out=p, ao_rays=None):
        smp, ao = SamplerDesc(spp, dims), host.AoDesc(n_ao, dist)
        rc = L.rt_render_rays_ao(scene, rays, w, h, s0, ns, C.byref(smp) if has_smp else None, C.byref(ao) if has_ao else None, flags, None, out, ao_rays, None)
        return rc, L.rt_last_error().decode()

    cases = dict(
        # rt_render_rays' list
        null_scene=dict(scene=None), null_rays=dict(rays=None), null_sampler=dict(has_smp=False), null_out=dict(out=None),
        zero_width=dict(w=0), negative_width=dict(w=-3), zero_height=dict(h=0), negative_height=dict(h=-1), zero_samples=dict(ns=0), negative_samples=dict(ns=-2),
        negative_sample0=dict(s0=-1), range_past_spp=dict(s0=3, ns=2, spp=4), range_past_rounded_spp=dict(s0=0, ns=9, spp=5),
        too_many_rays=dict(w=4096, h=4096, ns=16, spp=16), too_many_rays_wraps_32_bits=dict(w=65536, h=65536, ns=1, spp=1),
        too_many_rays_wraps_64_bits=dict(w=2 ** 31 - 1, h=2 ** 31 - 1, ns=8, spp=8), spp_too_large=dict(spp=16385, ns=1),
        dimensions_too_small=dict(dims=1), dimensions_too_large=dict(dims=9), ref_stream=dict(flags=RT_FLAG_REF_STREAM),
        # the integrator's own
        null_ao=dict(has_ao=False), no_occlusion_samples=dict(n_ao=0), negative_occlusion_samples=dict(n_ao=-4), too_many_occlusion_samples=dict(n_ao=1025),
        zero_distance=dict(dist=0.0), negative_distance=dict(dist=-1.0), nan_distance=dict(dist=nan),
        too_many_ray_records=dict(w=1024, h=1024, ns=16, spp=16, n_ao=16, ao_rays=p))
    for name, kw in cases.items():
        rc, msg = call(**kw)
        print(f"{name}: {rc} {msg!r}")
        assert rc == RT_ERR_INVALID and msg and "rt_render_rays_ao" in msg, (name, rc, msg)

    def frame(scene=scene, cam=p, film=p, has_smp=True, spp=4, dims=4, has_ao=True, n_ao=3, dist=inf, flags=0, out=p):
        smp, ao = SamplerDesc(spp, dims), host.AoDesc(n_ao, dist)
        rc = L.rt_render_ao(scene, cam, film, C.byref(smp) if has_smp else None, C.byref(ao) if has_ao else None, None, flags, None, out, None)
        return rc, L.rt_last_error().decode()

    for name, kw in dict(null_scene=dict(scene=None), null_camera=dict(cam=None), null_film=dict(film=None), null_sampler=dict(has_smp=False), null_ao=dict(has_ao=False),
                         null_film_out=dict(out=None), spp_too_large=dict(spp=16385), dimensions_too_small=dict(dims=1), dimensions_too_large=dict(dims=9),
                         no_occlusion_samples=dict(n_ao=0), too_many_occlusion_samples=dict(n_ao=1025), zero_distance=dict(dist=0.0), nan_distance=dict(dist=nan),
                         ref_stream=dict(flags=RT_FLAG_REF_STREAM)).items():
        rc, msg = frame(**kw)
        print(f"rt_render_ao {name}: {rc} {msg!r}")
        assert rc == RT_ERR_INVALID and msg and "rt_render_ao" in msg, (name, rc, msg)

    # the host layer refuses the same before it uploads the scene (no device here: an upload would answer RT_ERR_NO_DEVICE)
    from rustracer_amd.scenes import cornell_box
    hs = host.HostScene(cornell_box(8, 8, 4))
    rays = np.zeros((2, 2, 2, 8), np.float32)
    for kw in (dict(n_samples=0), dict(n_samples=1025), dict(n_samples=3, max_distance=0.0), dict(n_samples=3, max_distance=nan), dict(n_samples=3, sample0=3),
               dict(n_samples=3, spp=5, sample0=7)):
        with pytest.raises(host.BackendError) as e:
            hs.render_rays_ao(rays, **kw)
        print(kw, e.value)
        assert "rtxh_render_rays_ao" in str(e.value) and "no HIP device" not in str(e.value)
    for kw in (dict(n_samples=0), dict(n_samples=2000), dict(n_samples=2, max_distance=-1.0)):
        with pytest.raises(host.BackendError) as e:
            hs.render_ao(**kw)
        assert "rtxh_render_ao" in str(e.value) and "no HIP device" not in str(e.value)
    with pytest.raises(host.BackendError):
        hs.render_rays_ao(np.zeros((2, 2, 2, 7), np.float32), 3)


# ---------------------------------------------------------------- the kernels' allocation
@pytest.fixture(scope="module")
def resources(host):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_budget
    finally:
        sys.path.pop(0)
    return kernel_budget.kernel_resources(host.HIP_LIB)


# As built: k_ao_rays<false> 81 VGPRs, 106 SGPRs, 68 B of LDS (block_push's counters); k_ao_rays<true> (quadrics, instances) 158 VGPRs, 106 SGPRs, 68 B;
# k_ao_fold 23 VGPRs, 73 SGPRs, no LDS; k_ao_finish 25 VGPRs, 56 SGPRs, no LDS. Nothing in scratch, no vector register spilled.
@pytest.mark.parametrize("name", ["rtx::k_ao_rays<false>", "rtx::k_ao_rays<true>", "rtx::k_ao_fold", "rtx::k_ao_finish"])
def test_ao_kernels_use_no_scratch_and_spill_no_vector_register(resources, name):
    r = resources[name]
    print(name, r)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0, r
    assert r["lds"] <= 128, r
