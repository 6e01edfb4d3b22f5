"""Textures on the GPU lookup by lookup (rt_texture_eval, the evaluator the shade kernels call) and in films: every existing kind and graphs of any depth
against the oracle's probe, planar checkerboards against the oracle's uv checkerboard at the planar map, fbm under a transform against the oracle's identity
fbm at the transformed point, and the file / multi-GPU / shard paths."""
import copy

import numpy as np
import pytest

from util import rel_l2

pytestmark = pytest.mark.gpu
N = 1200


def _records(seed, n=N):
    rng = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32)
    uv = rng.normal(0.0, 3.0, (n, 2))
    uv[::7] *= 1e3          # large coordinates
    uv[::5] = -np.abs(uv[::5])
    duv = rng.normal(0.0, 1.0, (n, 4)) * 10.0 ** rng.uniform(-4, 0.5, (n, 1))
    p = rng.normal(0.0, 4.0, (n, 3))
    p[::13] *= 300.0
    dpdx = rng.normal(0.0, 1.0, (n, 3)) * 10.0 ** rng.uniform(-4, 0, (n, 1))
    dpdy = rng.normal(0.0, 1.0, (n, 3)) * 10.0 ** rng.uniform(-4, 0, (n, 1))
    zero = np.arange(n) % 3 == 0  # a third of the records without differentials (what every vertex past the camera ray has)
    duv[zero] = 0.0; dpdx[zero] = 0.0; dpdy[zero] = 0.0
    return dict(uv=f(uv), p=f(p), duv=f(duv), dpdx=f(dpdx), dpdy=f(dpdy)), zero


def _probe(o, tex, r):
    return np.stack([o.tex_probe(tex, r["uv"][i], r["p"][i], r["duv"][i], r["dpdx"][i], r["dpdy"][i]) for i in range(r["uv"].shape[0])])


def _gate(name, cat, got, want, zero):
    same = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
    print(f"{name:28s} {cat:6s} bit-unequal {100.0 * (1.0 - same.mean()):6.2f} % of {len(same)}")
    assert np.isfinite(got).all() == np.isfinite(want).all()
    if cat == "exact":
        assert same.all(), (name, np.argwhere(~same)[:5].ravel())
    elif cat == "fbm":  # ocml's log2f against glibc's: the octave count may differ in its last bit where there are differentials
        assert same[zero].all(), name
        assert np.abs(got - want).max() <= 1e-5, (name, float(np.abs(got - want).max()))
    else:  # image maps
        err = np.abs(got.astype(np.float64) - want) - 1e-5 * np.abs(want.astype(np.float64)) - 1e-7
        assert err.max() <= 0.0, (name, float(err.max()))


def _base():
    from rustracer_amd.scenes import cornell_box
    return cornell_box(16, 16, 1)


def _images(d):
    from rustracer_amd.scene_desc import WRAP_BLACK, WRAP_CLAMP, WRAP_REPEAT
    from rustracer_amd.scenes.procedural import checker_fbm_image
    a = d.add_mip(checker_fbm_image(32, 5, (0.9, 0.3, 0.2), (0.2, 0.3, 0.9), 4), trilinear=False, max_aniso=8.0, wrap=WRAP_REPEAT)
    b = d.add_mip(checker_fbm_image(16, 6), trilinear=True, wrap=WRAP_CLAMP)
    c = d.add_mip(checker_fbm_image(16, 7), trilinear=False, max_aniso=2.0, wrap=WRAP_BLACK)
    return d.image_tex(a, 3, 2, 0.1, 0.2), d.image_tex(b, 2, 2), d.image_tex(c, 1.5, 1.5, -0.2, 0.0)


def test_every_existing_kind_matches_the_oracle_probe(gpu_host, orc):
    d = _base()
    ew, tri, blk = _images(d)
    c1, c2, amt = d.const_tex((0.9, 0.2, 0.4)), d.const_tex((0.1, 0.7, 0.3)), d.const_tex(0.3)
    uv = d.uv_tex(2.0, 3.0, 0.1, -0.2)
    fbm = d.fbm_tex(0.6, 6)
    cases = {
        "const": (c1, "exact"), "uv": (uv, "exact"),
        "checker_closedform": (d.checker_tex(c1, c2, 4, 3, 0.1, 0.3), "exact"), "checker_none": (d.checker_tex(c1, c2, 5, 5, aa="none"), "exact"),
        "scale": (d.scale_tex(uv, c1), "exact"), "mix": (d.mix_tex(c1, uv, amt), "exact"),
        "two_level": (d.scale_tex(d.checker_tex(uv, c2, 3, 3), d.mix_tex(uv, c1, amt)), "exact"),
        "fbm": (fbm, "fbm"), "fbm_graph": (d.mix_tex(d.checker_tex(fbm, c1, 2, 2), c2, fbm), "fbm"),
        "image_ewa_repeat": (ew, "image"), "image_trilinear_clamp": (tri, "image"), "image_ewa_black": (blk, "image"),
        "image_graph": (d.mix_tex(d.scale_tex(ew, c1), tri, amt), "image"),
    }
    h = gpu_host.HostScene(d)
    o = orc.OracleScene(d)
    for k, (name, (tex, cat)) in enumerate(cases.items()):
        r, zero = _records(k)
        _gate(name, cat, h.texture_eval(tex, **r), _probe(o, tex, r), zero)


def _random_graph(d, rng, depth, leaves, pool):
    """a combinator `depth` deep (its first operand one level less), other operands random and sometimes a sub-graph made before (shared)"""
    if depth == 0:
        return int(rng.choice(leaves))

    def op():
        if pool and rng.random() < 0.3:
            return int(rng.choice(pool))
        return _random_graph(d, rng, int(rng.integers(0, depth)), leaves, pool)
    k = rng.integers(3)
    first = _random_graph(d, rng, depth - 1, leaves, pool)
    if k == 0:
        t = d.scale_tex(first, op())
    elif k == 1:
        t = d.mix_tex(first, op(), op()) if rng.random() < 0.5 else d.mix_tex(op(), first, first)  # amounts that are combinators
    else:
        su, sv = rng.uniform(0.5, 6, 2)
        t = d.checker_tex(first, op(), float(su), float(sv), float(rng.uniform(-1, 1)), 0.0, aa="none" if rng.random() < 0.3 else "closedform")
    pool.append(t)
    return t


def _deep_graphs(d, seed, n=12, with_fbm_and_images=False):
    rng = np.random.default_rng(seed)
    leaves = [d.const_tex((0.9, 0.2, 0.4)), d.const_tex((0.2, 0.6, 0.9)), d.const_tex(0.35), d.uv_tex(2.0, 3.0, 0.1, -0.2), d.uv_tex(0.5, 0.5)]
    if with_fbm_and_images:
        ew, tri, _ = _images(d)
        leaves += [d.fbm_tex(0.5, 5), ew, tri]
    pool = []
    return [_random_graph(d, rng, 3 + i % 4, leaves, pool) for i in range(n)]


@pytest.mark.parametrize("mixed", [False, True])
def test_deep_graphs_match_the_oracle_probe(gpu_host, orc, mixed):
    d = _base()
    roots = _deep_graphs(d, 7 + mixed, with_fbm_and_images=mixed)
    h, o = gpu_host.HostScene(d), orc.OracleScene(d)
    for k, t in enumerate(roots):
        r, zero = _records(100 + k, 1000)
        got, want = h.texture_eval(t, **r), _probe(o, t, r)
        if mixed:  # an fbm or image leaf anywhere below: the looser of their gates
            err = np.abs(got.astype(np.float64) - want) - 1e-5 * np.abs(want.astype(np.float64)) - 1e-5
            same = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
            print(f"deep graph {k} bit-unequal {100.0 * (1.0 - same.mean()):.2f} %")
            assert err.max() <= 0.0, (k, float(err.max()))
        else:
            _gate(f"deep graph {k}", "exact", got, want, zero)


def _room_with_deep_graphs(spp=8):
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(32, 32, spp)
    g = _deep_graphs(d, 11, n=8)
    floor = d.matte(g[3])
    back = d.plastic(g[4], (0.3, 0.3, 0.3), d.scale_tex(g[5], d.const_tex(0.3)))
    left = d.set_bump(d.matte((0.6, 0.5, 0.4)), d.scale_tex(g[6], d.const_tex(0.01)))
    d._mat[0][:] = floor
    d._mat[2][:] = back
    d._mat[4][:] = left
    P = np.float32([[100, 20, 500], [450, 20, 500], [450, 400, 500], [100, 400, 500]])
    mask = d.scale_tex(d.checker_tex(0.0, 1.0, 4, 4, aa="none"), d.mix_tex(d.const_tex(1.0), d.uv_tex(), d.const_tex(0.5)))  # (masks: two-level graphs)
    d.add_mesh(P, np.int32([[0, 1, 2], [0, 2, 3]]), d.matte((0.2, 0.8, 0.3)), UV=np.float32([[0, 0], [3, 0], [3, 3], [0, 3]]), alpha=mask, two_sided=False)
    return d, g[7]


def test_room_with_deep_graphs_matches_oracle_films(gpu_host, orc):
    d, _ = _room_with_deep_graphs()
    fo, _ = orc.OracleScene(d).render(mode=1)
    fh, _ = gpu_host.HostScene(d).render()
    assert np.array_equal(fo[..., 3], fh[..., 3])
    err = rel_l2(gpu_host.film_to_rgb(fh), orc.film_to_rgb(fo))
    print(f"deep-graph room: rel L2 {err:.2e}")
    assert err < 1e-3, err


def _masked_room(mask):
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(32, 32, 8)
    P = np.float32([[100, 20, 500], [450, 20, 500], [450, 400, 500], [100, 400, 500]])
    d.add_mesh(P, np.int32([[0, 1, 2], [0, 2, 3]]), d.matte((0.2, 0.8, 0.3)), UV=np.float32([[0, 0], [3, 0], [3, 3], [0, 3]]), alpha=mask(d), two_sided=False)
    return d


def _deep_mask(d):
    """a depth-5 graph with a combinator as mix amount and a shared sub-graph (needs 2 value slots)"""
    c = d.checker_tex(0.0, 1.0, 4, 4, aa="none")
    s = d.scale_tex(c, d.uv_tex(2, 2))
    m = d.mix_tex(s, d.const_tex(1.0), d.checker_tex(s, d.const_tex(0.2), 3, 3, aa="none"))
    return d.scale_tex(d.mix_tex(m, s, d.const_tex(0.5)), d.checker_tex(m, d.const_tex(1.0), 2, 2, aa="none"))


def test_a_deep_graph_as_alpha_mask_matches_oracle_films(gpu_host, orc):
    d = _masked_room(_deep_mask)
    fo, _ = orc.OracleScene(d).render(mode=1)
    fh, _ = gpu_host.HostScene(d).render()
    assert np.array_equal(fo[..., 3], fh[..., 3])
    err = rel_l2(gpu_host.film_to_rgb(fh), orc.film_to_rgb(fo))
    print(f"deep alpha mask: rel L2 {err:.2e}")
    assert err < 1e-3, err


def test_mapped_masks_render_and_a_mask_beyond_its_slots_is_refused_by_name(gpu_host):
    planar = lambda d: d.checker_tex(0.0, 1.0, mapping="planar", v1=(0.02, 0, 0), v2=(0, 0.02, 0), aa="none")
    # (a mask cuts where its value is exactly 0: fbm alone almost never is, so it rides on the checkerboard's zeros)
    fbm = lambda d: d.scale_tex(planar(d), d.fbm_tex(0.5, 4, tex2world=np.diag([0.02, 0.02, 0.02, 1.0])))
    plain, _ = gpu_host.HostScene(_masked_room(lambda d: d.const_tex(1.0))).render()
    for mask in (planar, fbm):
        film, _ = gpu_host.HostScene(_masked_room(mask)).render()
        assert np.isfinite(film).all() and not np.array_equal(film, plain)

    def wide(d):  # a complete binary tree of scales four deep: 5 values at once
        level = [d.const_tex(1.0)] * 32
        while len(level) > 1:
            level = [d.scale_tex(a, b) for a, b in zip(level[::2], level[1::2])]
        return level[0]
    with pytest.raises(gpu_host.BackendError, match="RT_TEX_MASK_SLOTS"):
        gpu_host.HostScene(_masked_room(wide)).render()


def _dot(a, b):  # Vector3f::dot in f32, x y z order
    return a[:, 0] * b[0] + a[:, 1] * b[1] + a[:, 2] * b[2]


@pytest.mark.parametrize("aa", ["closedform", "none"])
def test_planar_checkerboard_is_the_uv_checkerboard_at_the_planar_map(gpu_host, orc, aa):
    d = _base()
    c1, c2 = d.const_tex((0.9, 0.2, 0.4)), d.const_tex((0.1, 0.7, 0.3))
    ref = d.checker_tex(c1, c2, 1.0, 1.0, 0.0, 0.0, aa=aa)
    o = orc.OracleScene(d)  # (kinds the oracle knows only)
    g = copy.deepcopy(d)
    v1, v2, ud, vd = np.float32([0.5, -0.25, 1.5]), np.float32([0.125, 2.0, -0.75]), np.float32(0.3), np.float32(-1.7)
    pl = g.checker_tex(c1, c2, mapping="planar", v1=v1, v2=v2, udelta=ud, vdelta=vd, aa=aa)
    h = gpu_host.HostScene(g)
    r, zero = _records(21)
    s, t = ud + _dot(r["p"], v1), vd + _dot(r["p"], v2)
    q = dict(uv=np.stack([s, t], 1), p=r["p"], duv=np.stack([_dot(r["dpdx"], v1), _dot(r["dpdx"], v2), _dot(r["dpdy"], v1), _dot(r["dpdy"], v2)], 1),
             dpdx=r["dpdx"], dpdy=r["dpdy"])
    _gate(f"planar checker {aa}", "exact", h.texture_eval(pl, **r), _probe(o, ref, q), zero)


def _rot(deg, axis):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + s * K + (1 - c) * K @ K
    return m


MATRICES = {
    "translate": [[1, 0, 0, 1.5], [0, 1, 0, -2.25], [0, 0, 1, 0.5], [0, 0, 0, 1]],
    "scale": np.diag([2.0, 0.5, -3.0, 1.0]),
    "rotate": _rot(33.0, (1.0, 2.0, -0.5)),
    "affine": [[1.2, 0.3, -0.4, 2.0], [0.1, 0.9, 0.25, -1.0], [-0.6, 0.2, 1.4, 0.75], [0, 0, 0, 1]],
    "projective": [[1.0, 0.2, 0.0, 0.5], [0.0, 1.1, 0.3, 0.0], [0.1, 0.0, 0.9, -0.25], [0.02, -0.01, 0.03, 1.5]],
}


@pytest.mark.parametrize("name", list(MATRICES))
def test_mapped_fbm_is_the_identity_fbm_at_the_transformed_point(gpu_host, orc, name):
    m = np.float32(MATRICES[name])
    d = _base()
    ref = d.fbm_tex(0.55, 7)
    o = orc.OracleScene(d)
    g = copy.deepcopy(d)
    t = g.fbm_tex(0.55, 7, tex2world=m)
    h = gpu_host.HostScene(g)
    r, zero = _records(31)
    p, a, b = r["p"], r["dpdx"], r["dpdy"]
    row = lambda v, k, w: v[:, 0] * m[k, 0] + v[:, 1] * m[k, 1] + v[:, 2] * m[k, 2] + (m[k, 3] if w else np.float32(0))  # Transform * Point3f / * Vector3f
    pp = np.stack([row(p, k, True) for k in range(3)], 1)
    w = row(p, 3, True)
    pp = np.where((w != 1)[:, None], pp / w[:, None], pp).astype(np.float32)
    q = dict(uv=r["uv"], p=pp, duv=r["duv"], dpdx=np.stack([row(a, k, False) for k in range(3)], 1), dpdy=np.stack([row(b, k, False) for k in range(3)], 1))
    assert (w != 0).all()
    _gate(f"mapped fbm {name}", "fbm", h.texture_eval(t, **r), _probe(o, ref, q), zero)


def _plane(planar):
    """a floor quad inside the Cornell box, checkered by a planar map, or by a uv checkerboard whose vertex uvs are that map at the vertices (exact there)"""
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(40, 40, 8)
    d.integrator.max_depth = 1  # camera vertices only: their ray differentials make the closed-form filter continuous across check edges, where a point
    # sample of either twin may land on the other side of an edge by one rounding
    P = np.float32([[64, 1, 64], [448, 1, 64], [448, 1, 512], [64, 1, 512]])
    v1, v2, ud, vd = (0.03125, 0.0, 0.0), (0.0, 0.0, 0.015625), 0.5, -0.25
    c1, c2 = (0.8, 0.7, 0.2), (0.1, 0.2, 0.6)
    if planar:
        m = d.matte(d.checker_tex(c1, c2, mapping="planar", v1=v1, v2=v2, udelta=ud, vdelta=vd))
        d.add_mesh(P, np.int32([[0, 1, 2], [0, 2, 3]]), m)
    else:
        UV = np.float32([[ud + x * v1[0], vd + z * v2[2]] for x, _, z in P])
        m = d.matte(d.checker_tex(c1, c2))
        d.add_mesh(P, np.int32([[0, 1, 2], [0, 2, 3]]), m, UV=UV)
    return d


def test_planar_checkered_plane_equals_its_uv_twin(gpu_host):
    fa, _ = gpu_host.HostScene(_plane(True)).render()
    fb, _ = gpu_host.HostScene(_plane(False)).render()
    assert np.array_equal(fa[..., 3], fb[..., 3])
    err = rel_l2(gpu_host.film_to_rgb(fa), gpu_host.film_to_rgb(fb))
    print(f"planar vs uv twin: rel L2 {err:.2e}")
    assert err < 1e-3, err


def _file_scene():
    from rustracer_amd.scenes import cornell_box
    d = cornell_box(32, 32, 4)
    xf = np.float32([[2, 0, 0, 1], [0, 0.5, 0, 2], [0, 0, 4, 3], [0, 0, 0, 1]])  # Translate 1 2 3, Scale 2 0.5 4
    fs = d.fbm_tex(0.5, 6, tex2world=xf)
    pc = d.checker_tex((0.8, 0.7, 0.2), fs, mapping="planar", v1=(0.03125, 0, 0), v2=(0, 0, 0.0625), udelta=0.25, vdelta=0.5)
    fb = d.scale_tex(d.fbm_tex(0.4, 5, tex2world=xf), d.const_tex(3.0))
    d._mat[0][:] = d.set_bump(d.matte(pc), fb)
    d._mat[2][:] = d.matte(d.scale_tex(fs, d.const_tex((0.9, 0.6, 0.4))))
    return d


def _as_attribute_blocks(text):
    """the exporter's `TransformBegin / Transform [m] / Texture / TransformEnd` of a mapped fbm, written as `AttributeBegin / Translate 1 2 3 / Scale 2 0.5 4 /
    Texture / Identity`, each block closed before WorldEnd (so that the texture names stay declared)"""
    out, opened, lines, i = [], 0, text.split("\n"), 0
    while i < len(lines):
        if lines[i] == "TransformBegin" and lines[i + 3] == "TransformEnd":
            assert lines[i + 1].strip().startswith("Transform [")
            out += ["AttributeBegin", "  Translate 1 2 3", "  Scale 2 0.5 4", lines[i + 2], "  Identity"]
            opened += 1
            i += 4
            continue
        if lines[i].startswith("WorldEnd"):
            out += ["AttributeEnd"] * opened
        out.append(lines[i])
        i += 1
    assert opened >= 2
    return "\n".join(out)


def test_file_multi_and_shards_are_bit_equal_to_the_scene_in_memory(gpu_host, tmp_path):
    from rustracer_amd.pbrt_export import write_pbrt
    d = _file_scene()
    h = gpu_host.HostScene(d)
    film, _ = h.render()
    assert np.isfinite(film).all() and film[..., :3].max() > 0
    pb = str(tmp_path / "m.pbrt")
    write_pbrt(d, pb)
    text = _as_attribute_blocks(open(pb).read())
    open(pb, "w").write(text)
    assert "AttributeBegin\n  Translate 1 2 3\n  Scale 2 0.5 4" in text and '"string mapping" "planar"' in text and '"float" "fbm"' in text
    fp, _ = gpu_host.PbrtScene(pb).render()
    assert np.array_equal(fp, film)
    multi, _, _ = h.render_multi([0])
    assert np.array_equal(multi, film)
    shards = [h.render(rank=r, world_size=2)[0] for r in range(2)]
    assert np.array_equal(shards[0] + shards[1], film)
