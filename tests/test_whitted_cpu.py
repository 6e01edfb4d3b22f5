"""The Whitted integrator (rt_render_rays_whitted, rt_render_whitted) without a GPU: the margins that make the GPU tests' every-sample comparison legitimate, the float64
model's own properties, the C boundary - rt_whitted_desc in the header, the ctypes mirror, the Rust declarations of INTEGRATION.md, the exported symbols, every refusal
answered with its code and a message before any device work (the scene pointer is a dummy that is never dereferenced) -, render_pbrt.py's --whitted conflicts, and the
register and scratch numbers of the new kernels, read from the built code object.

rt_whitted_desc is declared as `struct rt_whitted_desc {..}; typedef struct rt_whitted_desc rt_whitted_desc;` and its Rust mirror in a block of its own, as rt_ao_desc
is: tests/test_abi_cpu.py holds the set of `typedef struct .. {` records to a fixed list."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import whitted_cases as wc
import whitted_model as wm
from test_abi_cpu import parse_c_prototypes, _strip_comments
from test_ao_cpu import SamplerDesc, _header_struct, _rust_fn_types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID, RT_ERR_UNSUPPORTED = -1, -5
RT_FLAG_REF_STREAM = 16


# ---------------------------------------------------------------- the margins of the GPU tests' batches
@pytest.mark.parametrize("name", list(wc.CASES))
def test_every_ray_of_every_batch_keeps_its_distance_from_a_decision(orc, name):
    """Every li ray and visibility segment of every run of the case stays >= 1e-3 scene units from an edge, a silhouette or a shadow boundary, and every refraction
    >= 1e-3 in sin^2 from the critical angle: float32 and float64 walk the same tree, so tests/test_gpu_whitted.py may compare every sample. The salts of
    tests/golden/whitted_salts.npz are where whitted_cases.settled ended; with them nothing has to move."""
    for md, dims in wc.RUNS[name]:
        res, (b, rays) = wc.reference(orc, name, md, dims)
        active = rays.reshape(-1, 8)[:, 3] > 0
        print(f"{name} max_depth {md} dimensions {dims}: edge {res.edge[active].min():.3e}, shadow {res.shadow[active].min():.3e}, sin^2 {res.sin2[active].min():.3e}; "
              f"nodes {res.nodes[active].min()} .. {res.nodes.max()}, draws up to {res.draws.max()}")
        assert res.edge[active].min() >= 1e-3 and res.shadow[active].min() >= 1e-3 and res.sin2[active].min() >= 1e-3
        assert not res.nodes[~active].any() and res.draws.max() < wc.N_DRAWS
    with np.load(wc.SALTS) as z:
        assert np.array_equal(z[name], wc._cache[("salt", name)]), "the committed salts are where the settling ends"
    assert rays.shape == (24, 40, 4, 8)


# ---------------------------------------------------------------- the model
def _u(n, k=64, seed=3):
    return np.random.default_rng(seed).random((n, k, 2)).astype(np.float32)


def _floor_scene():
    sc = wm.Scene()
    sc.add_quad((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4), ("matte", 0.5))
    sc.lights.append(("point", (0.0, 2.0, 0.0), (8.0, 8.0, 8.0)))
    return sc


def test_model_max_depth_one_is_direct_light_only():
    sc = _floor_scene()
    o = np.float64([(1.0, 1.0, 0.0), (0.0, 3.0, -1.0), (0.0, 1.0, 0.0)])
    d = np.float64([(0.0, -1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 1.0, 0.0)])
    r1, r5 = wm.render(sc, o, d, 1, _u(3)), wm.render(sc, o, d, 5, _u(3))
    p = np.float64([(1.0, 0.0, 0.0), (0.0, 0.0, -1.0)])
    v = np.float64((0.0, 2.0, 0.0)) - p
    r2 = (v * v).sum(1)
    want = 0.5 / np.pi * 8.0 / (4.0 * np.pi * r2) * (2.0 / np.sqrt(r2))   # rho / pi * I / (4 pi r^2) * cos
    print("direct light:", r1.L[:2, 0], "closed form:", want)
    assert np.allclose(r1.L[:2], want[:, None], rtol=1e-12) and np.array_equal(r1.L, r5.L)
    assert r1.nodes.tolist() == [1, 1, 1] and r1.draws.tolist() == [1, 1, 0] and r5.draws.tolist() == [3, 3, 0]   # a miss draws nothing; the two recursion draws are consumed on matte
    assert not r1.L[2].any()


def test_model_two_facing_mirrors_give_max_depth_nodes():
    sc = wm.Scene()
    sc.add_quad((-0.5, -50, -50), (-0.5, -50, 50), (-0.5, 50, 50), (-0.5, 50, -50), ("mirror", 0.9))
    sc.add_quad((0.5, -50, -50), (0.5, 50, -50), (0.5, 50, 50), (0.5, -50, 50), ("mirror", 0.9))
    sc.lights.append(("point", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    o, d = np.zeros((2, 3)), wm._norm(np.float64([(1.0, 0.1, 0.2), (-1.0, 0.0, 0.3)]))
    for md in (1, 2, 5, 16):
        r = wm.render(sc, o, d, md, _u(2))
        print(f"mirrors, max_depth {md}: nodes {r.nodes}, draws {r.draws}")
        assert (r.nodes == md).all() and (r.draws == md * 1 + 2 * (md - 1)).all() and not r.L.any()


def test_model_glass_slab_node_count_by_hand_at_depth_three():
    """A slab over nothing, a ray from above, max_depth 3. Depth 0, the top face: reflection -> a miss (1 node), transmission -> depth 1, the bottom face from inside:
    reflection -> depth 2, the top face from inside (no recursion at depth 2), transmission -> depth 2, a miss. 1 + 1 + 1 + 1 + 1 = 5 li invocations; draws: the three
    hits each take one light draw, the hits at depth 0 and 1 two more."""
    b = wc.Both()
    b.box((-1, 0, -1), (1, 0.2, 1), wc.GLASS)
    b.point((0.0, 5.0, 0.0), (1.0, 1.0, 1.0))
    r = wm.render(b.model, np.float64([(0.1, 2.0, 0.05)]), wm._norm(np.float64([(0.1, -1.0, 0.2)])), 3, _u(1))
    print("slab at depth 3: nodes", r.nodes, "draws", r.draws, "sin^2 gap", r.sin2)
    assert r.nodes.tolist() == [5] and r.draws.tolist() == [3 + 2 * 2]
    deeper = wm.render(b.model, np.float64([(0.1, 2.0, 0.05)]), wm._norm(np.float64([(0.1, -1.0, 0.2)])), 4, _u(1))
    assert deeper.nodes[0] == 7   # the inside hit at depth 2 now recurses: its reflection meets the bottom face again, its transmission leaves upwards


def test_model_reflection_and_transmission_weights_conserve_energy():
    """Per vertex, with the interface's physical reflectance (fr_dielectric under the cosine's sign): R + T = 1 wherever light is transmitted and R = 1 under total
    internal reflection, once the eta^2 factor of SpecularTransmission under RADIANCE - radiance, not energy, is what widens on the way out of glass - is taken out: at most
    1, and exactly 1. That holds the refraction, the eta^2 factor and fr_dielectric together. The reference reaches fr_dielectric through FresnelDielectric::evaluate,
    which passes |cos| (fresnel.rs:125): its reflection and transmission lobes evaluate the interface at two different angles as (1, eta), so ITS weights - the model's
    and the device's - do not add up to 1 (printed); what is asserted of them is that either alone stays within its physical range.
    For a mix of two mirrors the expectation over the lobe choice is the mix of the reflectances."""
    lb = wm.lobes(wc.GLASS)
    rng = np.random.default_rng(5)
    n = np.float64((0.0, 0.0, 1.0)) * np.ones((512, 3))
    wo = wm._norm(rng.normal(size=(512, 3)))
    u = rng.random((512, 2)).astype(np.float32)
    ent = wo[:, 2] > 0
    unscale = np.where(ent, 1.5 ** 2, 1.5 ** -2)   # (eta_t / eta_i)^2
    wr, _, vr, _ = wm.sample_specular(lb, "spec_r", wo, n, u, signed_fresnel=True)
    wt, wi, vt, gap = wm.sample_specular(lb, "spec_t", wo, n, u, signed_fresnel=True)
    energy = wr[:, 0] + np.where(vt, wt[:, 0] * unscale, 0.0)
    print(f"glass, physical reflectance: R + T / (eta_i / eta_t)^2 in [{energy.min():.12f}, {energy.max():.12f}], total internal reflection at {int((~vt).sum())} of 512 directions")
    assert vr.all() and energy.max() <= 1.0 + 1e-9 and np.allclose(energy, 1.0, atol=1e-9) and 50 < (~vt).sum() < 300   # (1e-9: cos_t = sqrt(1 - sin^2) loses half its digits next to the critical angle)
    assert not vt[~ent & (1.5 ** 2 * (1 - wo[:, 2] ** 2) >= 1)].any() and np.allclose(np.linalg.norm(wi[vt], axis=1), 1.0)
    qr, _, _, _ = wm.sample_specular(lb, "spec_r", wo, n, u)
    qt, qi, qv, _ = wm.sample_specular(lb, "spec_t", wo, n, u)
    q = qr[:, 0] + np.where(qv, qt[:, 0] * unscale, 0.0)
    print(f"glass, the reference's |cos|: R + T / (eta_i / eta_t)^2 in [{q.min():.4f}, {q.max():.4f}]")
    assert np.array_equal(qv, vt) and np.allclose(qi[qv], wi[vt]) and (qr[:, 0] <= 1.0).all() and (qt[qv, 0] * unscale[qv] <= 1.0).all() and (qr >= 0).all() and (qt >= 0).all()
    mix = wm.lobes(("mix", ("mirror", 0.9), ("mirror", 0.2), 0.3))
    w, _, v, _ = wm.sample_specular(mix, "spec_r", wo, n, u)
    first = np.floor(u[:, 0].astype(np.float64) * 2) == 0
    assert v.all() and np.allclose(w[first, 0], 0.3 * 0.9 * 2) and np.allclose(w[~first, 0], 0.7 * 0.2 * 2) and abs(w[:, 0].mean() - (0.3 * 0.9 + 0.7 * 0.2)) < 0.05


def test_model_lights():
    """sample_li of the four kinds: the point light's I / (4 pi r^2), the distant light's constant L, the triangle's pdf r^2 / (|cos| area) whose estimator integrates to
    the emitter's solid-angle-weighted radiance, and the constant environment's pdf integrating to one over the sphere."""
    p = np.zeros((4096, 3))
    u = np.random.default_rng(9).random((4096, 2)).astype(np.float32)
    sc = wm.Scene()
    tri = np.float64([(-0.5, 2.0, -0.5), (0.5, 2.0, -0.5), (0.5, 2.0, 0.5)])   # (p0 - p2) x (p1 - p2) points down
    sc.add_tri(*tri, ("matte", 0.0), emission=(3.0, 3.0, 3.0))
    li, wi, pdf, dist, surf = wm.sample_light(sc, ("tri", 0), p, u)
    est = (li[:, 0] * wi[:, 1] / pdf).mean()   # the irradiance on a floor point facing up: int L cos cos' / r^2 dA
    g = (np.arange(400) + 0.5) / 400
    b0, b1 = np.meshgrid(g, g, indexing="ij")
    inside = b0 + b1 <= 1
    q = b0[inside, None] * tri[0] + b1[inside, None] * tri[1] + (1 - b0 - b1)[inside, None] * tri[2]
    r2 = (q * q).sum(1)
    quad = (3.0 * (q[:, 1] / np.sqrt(r2)) ** 2 / r2).mean() * 0.5
    print(f"triangle light: estimator {est:.5f}, quadrature {quad:.5f}")
    assert (li[:, 0] == 3.0).all() and surf == sc.tris[0][4] and abs(est / quad - 1) < 0.03, (est, quad)
    li, wi, pdf, _, _ = wm.sample_light(sc, ("point", (0.0, 2.0, 0.0), (8.0, 4.0, 2.0)), p[:1], u[:1])
    assert np.allclose(li[0], np.float64((8.0, 4.0, 2.0)) / (16.0 * np.pi)) and np.allclose(wi[0], (0, 1, 0)) and pdf[0] == 1.0
    li, wi, pdf, _, _ = wm.sample_light(sc, ("distant", (0.0, 3.0, 4.0), (1.0, 2.0, 3.0)), p[:1], u[:1])
    assert np.allclose(li[0], (1, 2, 3)) and np.allclose(wi[0], (0, 0.6, 0.8)) and pdf[0] == 1.0
    wi, pdf = wm.infinite_sample(8, u)
    print(f"environment: mean 1 / pdf = {(1.0 / pdf).mean():.4f} (4 pi = {4 * np.pi:.4f})")
    assert np.allclose(np.linalg.norm(wi, axis=1), 1.0) and abs((1.0 / pdf).mean() / (4 * np.pi) - 1) < 0.03


# ---------------------------------------------------------------- the boundary
def test_rt_whitted_desc_in_header_ctypes_rust_and_library_agree(host):
    src = _strip_comments(open(os.path.join(ROOT, "include", "rtx_hip.h")).read())
    fields = _header_struct(src, "rt_whitted_desc")
    assert fields == [("int32_t", "max_depth"), ("int32_t", "reserved")], fields
    assert re.search(r"typedef struct rt_whitted_desc rt_whitted_desc;", src)
    assert host.WhittedDesc._fields_ == [(n, C.c_int32) for _, n in fields]
    assert C.sizeof(host.WhittedDesc) == 8 and host.hip_lib().rt_sizeof(b"rt_whitted_desc") == 8
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rust = _strip_comments("\n".join(re.findall(r"```rust\n(.*?)```", md, flags=re.S)))
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct RtWhittedDesc\s*\{(.*?)\}", rust, flags=re.S)
    assert m, "INTEGRATION.md spells RtWhittedDesc out"
    rs = [tuple(x.strip() for x in f.split(":")) for f in m.group(1).split(",") if f.strip()]
    assert rs == [("max_depth", "i32"), ("reserved", "i32")], rs
    defs = dict(re.findall(r"#define\s+(RT_WHITTED_\w+)\s+(\d+)", src))
    assert int(defs["RT_WHITTED_MAX_DEPTH"]) == host.RT_WHITTED_MAX_DEPTH == 16 and int(defs["RT_WHITTED_INFO_WORDS"]) == host.RT_WHITTED_INFO_WORDS == 2


def test_prototypes_are_declared_exported_documented_and_wrapped(host):
    hip = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_hip.h"))
    hosth = parse_c_prototypes(os.path.join(ROOT, "include", "rtx_host.h"))
    assert hip["rt_render_rays_whitted"] == ("i32", ["*rt_scene", "*f32", "i32", "i32", "i32", "i32", "*rt_sampler_desc", "*rt_whitted_desc", "u32", "*c_void", "*f32", "*u32", "*rt_stats"])
    assert hip["rt_render_whitted"] == ("i32", ["*rt_scene", "*rt_camera", "*rt_film_desc", "*rt_sampler_desc", "*rt_whitted_desc", "*rt_shard", "u32", "*c_void", "*f32", "*rt_stats"])
    assert hosth["rtxh_render_rays_whitted"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "*f32", "i32", "i32", "i32", "i32", "i32", "*c_void", "*f32", "*u32", "*rt_stats"])
    assert hosth["rtxh_render_whitted"] == ("i32", ["*rtxh_scene", "*rtxh_render_params", "i32", "*c_void", "*f32", "*rt_stats"])
    for lib, names in ((host.hip_lib(), ("rt_render_rays_whitted", "rt_render_whitted")), (host.lib(), ("rtxh_render_rays_whitted", "rtxh_render_whitted"))):
        for n in names:
            assert hasattr(lib, n), n
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _rust_fn_types(md, "rt_render_rays_whitted") == ["*mut RtScene", "*const f32", "i32", "i32", "i32", "i32", "*const RtSamplerDesc", "*const RtWhittedDesc", "u32",
                                                           "*mut c_void", "*mut f32", "*mut u32", "*mut RtStats"]
    assert _rust_fn_types(md, "rt_render_whitted") == ["*mut RtScene", "*const RtCamera", "*const RtFilmDesc", "*const RtSamplerDesc", "*const RtWhittedDesc", "*const RtShard",
                                                      "u32", "*mut c_void", "*mut f32", "*mut RtStats"]
    sig = inspect.signature(host.HostScene.render_rays_whitted).parameters
    assert list(sig)[:10] == ["self", "rays", "max_depth", "sample0", "spp", "with_info", "device_out", "stream", "count_traversal", "time_kernels"], list(sig)
    assert sig["max_depth"].default == 5 and sig["with_info"].default is False
    sig = inspect.signature(host.HostScene.render_whitted).parameters
    assert list(sig)[:4] == ["self", "max_depth", "rank", "world_size"] and sig["max_depth"].default == 5


def test_every_refusal_answers_with_its_code_and_a_message_and_no_device(host):
    L = host.hip_lib()
    L.rt_render_rays_whitted.restype = C.c_int
    L.rt_render_rays_whitted.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_render_whitted.restype = C.c_int
    L.rt_render_whitted.argtypes = [C.c_void_p] * 6 + [C.c_uint32] + [C.c_void_p] * 3
    buf = C.create_string_buffer(4096)
    scene = C.cast(buf, C.c_void_p)   # never dereferenced: every check comes before the scene is looked at
    f = np.zeros(256, np.float32)
    p = f.ctypes.data_as(C.c_void_p)

    def call(scene=scene, rays=p, w=2, h=2, s0=0, ns=2, spp=4, dims=4, has_smp=True, has_w=True, depth=5, reserved=0, flags=0, out=p):
        smp, wd = SamplerDesc(spp, dims), host.WhittedDesc(depth, reserved)
        rc = L.rt_render_rays_whitted(scene, rays, w, h, s0, ns, C.byref(smp) if has_smp else None, C.byref(wd) if has_w else None, flags, None, out, None, None)
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
        null_desc=dict(has_w=False), zero_depth=dict(depth=0), negative_depth=dict(depth=-2), reserved_set=dict(reserved=1))
    for name, kw in cases.items():
        rc, msg = call(**kw)
        print(f"{name}: {rc} {msg!r}")
        assert rc == RT_ERR_INVALID and msg and "rt_render_rays_whitted" in msg, (name, rc, msg)
    rc, msg = call(depth=17)
    print(f"depth 17: {rc} {msg!r}")
    assert rc == RT_ERR_UNSUPPORTED and "rt_render_rays_whitted" in msg and "16" in msg

    def frame(scene=scene, cam=p, film=p, has_smp=True, spp=4, dims=4, has_w=True, depth=5, reserved=0, flags=0, out=p):
        smp, wd = SamplerDesc(spp, dims), host.WhittedDesc(depth, reserved)
        rc = L.rt_render_whitted(scene, cam, film, C.byref(smp) if has_smp else None, C.byref(wd) if has_w else None, None, flags, None, out, None)
        return rc, L.rt_last_error().decode()

    for name, kw in dict(null_scene=dict(scene=None), null_camera=dict(cam=None), null_film=dict(film=None), null_sampler=dict(has_smp=False), null_desc=dict(has_w=False),
                         null_film_out=dict(out=None), spp_too_large=dict(spp=16385), dimensions_too_small=dict(dims=1), dimensions_too_large=dict(dims=9),
                         zero_depth=dict(depth=0), reserved_set=dict(reserved=-1), ref_stream=dict(flags=RT_FLAG_REF_STREAM)).items():
        rc, msg = frame(**kw)
        print(f"rt_render_whitted {name}: {rc} {msg!r}")
        assert rc == RT_ERR_INVALID and msg and "rt_render_whitted" in msg, (name, rc, msg)
    rc, msg = frame(depth=40)
    assert rc == RT_ERR_UNSUPPORTED and "rt_render_whitted" in msg

    # the host layer refuses the same before it uploads the scene (no device here: an upload would answer RT_ERR_NO_DEVICE), and so do the Python arguments
    from rustracer_amd.scenes import cornell_box
    hs = host.HostScene(cornell_box(8, 8, 4))
    rays = np.zeros((2, 2, 2, 8), np.float32)
    for kw in (dict(max_depth=0), dict(max_depth=-1), dict(max_depth=17), dict(sample0=3), dict(spp=5, sample0=7)):
        with pytest.raises(host.BackendError) as e:
            hs.render_rays_whitted(rays, **kw)
        print(kw, e.value)
        assert "rtxh_render_rays_whitted" in str(e.value) and "no HIP device" not in str(e.value)
    for kw in (dict(max_depth=0), dict(max_depth=2000)):
        with pytest.raises(host.BackendError) as e:
            hs.render_whitted(**kw)
        assert "rtxh_render_whitted" in str(e.value) and "no HIP device" not in str(e.value)
    with pytest.raises(host.BackendError):
        hs.render_rays_whitted(np.zeros((2, 2, 2, 7), np.float32))
    with pytest.raises(host.BackendError):
        hs.render_rays_whitted(rays, device_out=np.zeros((2, 2, 2, 4), np.float32))


def test_stack_plan_halves_a_pass_over_the_budget_and_never_below_the_smallest(host):
    """rt_whitted_stack_plan: what reserve_workspace asks per candidate pass. 64 B per level and path, max_depth - 1 levels; halved while over the budget, down to 2^14 paths."""
    L = host.hip_lib()
    L.rt_whitted_stack_plan.restype = C.c_int
    L.rt_whitted_stack_plan.argtypes = [C.c_int32, C.c_uint64, C.c_int32, C.c_uint64, C.POINTER(C.c_uint64)]
    b = C.c_uint64(0)
    GiB = 1 << 30
    assert L.rt_whitted_stack_plan(5, 1 << 29, 29, GiB, C.byref(b)) == 1 and b.value == 64 * 4 * (1 << 29)      # the frame's usual pass at depth 5: 128 GiB
    assert L.rt_whitted_stack_plan(5, 1 << 22, 22, GiB, C.byref(b)) == 0 and b.value == GiB                      # exactly the budget fits
    assert L.rt_whitted_stack_plan(5, (1 << 22) + 1, 23, GiB, None) == 1
    assert L.rt_whitted_stack_plan(1, 1 << 29, 29, GiB, C.byref(b)) == 0 and b.value == 0                        # max_depth 1 never recurses: no stack
    assert L.rt_whitted_stack_plan(16, 1 << 14, 14, 1 << 20, C.byref(b)) == 0 and b.value == 64 * 15 << 14       # the smallest pass is never halved
    log2 = 29
    while L.rt_whitted_stack_plan(16, 1 << log2, log2, GiB, None):
        log2 -= 1
    assert log2 == 20 and 64 * 15 << 20 <= GiB < 64 * 15 << 21   # the loop of reserve_workspace ends at the largest pass that fits


def test_render_pbrt_refuses_a_depth_below_one():
    for v in ("0", "-1"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_pbrt.py"), "nothing.pbrt", "out.pfm", "--whitted=" + v], capture_output=True, text=True)
        print(v, r.returncode, r.stderr.strip().splitlines()[-1:])
        assert r.returncode != 0 and "--whitted MAXDEPTH must be >= 1" in r.stderr


@pytest.mark.parametrize("args", [["--whitted", "--ao", "4"], ["--whitted", "3", "--samples", "s.npy"], ["--whitted", "--preview-every", "2"], ["--whitted", "--adaptive", "0.1"],
                                  ["--whitted", "--features", "f.npy"], ["--whitted", "--devices", "0,1"], ["--whitted", "5", "--camera-model", "orthographic"]])
def test_render_pbrt_refuses_what_does_not_combine_with_whitted(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_pbrt.py"), "nothing.pbrt", "out.pfm"] + args, capture_output=True, text=True)
    print(args, r.returncode, r.stderr.strip().splitlines()[-1:])
    assert r.returncode != 0 and "--whitted" in r.stderr and ("does not combine" in r.stderr or "give one of them" in r.stderr)


# ---------------------------------------------------------------- the kernels' allocation
@pytest.fixture(scope="module")
def resources(host):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_budget
    finally:
        sys.path.pop(0)
    return kernel_budget.kernel_resources(host.HIP_LIB)


# As built: k_whitted_vertex<false> 256 VGPRs, 60 spilled dwords, 1840 B of scratch, 260 spilled scalars, 136 B of LDS (block_push's counters);
# k_whitted_vertex<true> 251 / 34 / 1792 / 270 / 136; beside them k_shade<0, false> and <0, true> of the same build: 251 VGPRs, nothing spilled, 1680 B, 157 / 184 scalars.
# The vertex kernel is held to the generic shade kernel's two-waves-per-SIMD bound (<= 256 VGPRs, no accumulation register), and its scratch to the shade kernel's plus
# 256 B: both keep a SurfaceInteraction and an eight-lobe Bsdf in scratch for the out-of-line material and lobe functions, and the walk keeps more alive across those
# calls than a path vertex does - the vertex's incoming ray and hit record for the pending entry, the throughput, the two counters, the pending mask - which at 256
# registers costs up to 60 spilled dwords (240 B). Unbounded the kernel takes 302 / 312 registers and runs one wave per SIMD (MEASUREMENTS.md).
@pytest.mark.parametrize("general", [False, True])
def test_vertex_kernel_stays_beside_the_generic_shade_kernel(resources, general):
    g = "true" if general else "false"
    w, k = resources[f"rtx::k_whitted_vertex<{g}>"], resources[f"rtx::k_shade<0, {g}, false, false, false, 0>"]
    print(f"k_whitted_vertex<{g}>", w, f"\nk_shade<0, {g}>", k)
    assert w["vgpr"] <= 256 and w["agpr"] == 0 and k["vgpr"] <= 256
    assert w["scratch"] <= k["scratch"] + 256 and w["vgpr_spills"] <= 64
    assert w["lds"] <= 256


def test_info_kernel_uses_no_scratch(resources):
    r = resources["rtx::k_whitted_info"]
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["lds"] == 0
