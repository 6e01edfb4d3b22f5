"""Planar checkerboards, fbm under a transform and texture graphs of any depth, without a GPU: what the .pbrt loader builds, the exporter round trip
and the checks rt_scene_create makes on a texture table before it touches a device."""
import ctypes as C

import numpy as np
import pytest

from rustracer_amd import host
from rustracer_amd import scene_desc as sd
from rustracer_amd.pbrt_export import write_pbrt
from rustracer_amd.scenes import cornell_box

from util import RtImage, RtMaterial, RtSceneDesc, RtTexture

RT_ERR_INVALID = -1

_SCENE = """LookAt 0 0 5  0 0 0  0 1 0
Camera "perspective" "float fov" [30]
Film "image" "integer xresolution" [16] "integer yresolution" [16]
Sampler "02sequence" "integer pixelsamples" [4]
WorldBegin
LightSource "point" "point from" [0 0 3] "rgb I" [5 5 5]
{textures}
Material "matte" "texture Kd" "{kd}"
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0  1 -1 0  1 1 0  -1 1 0]
WorldEnd
"""


def _load(tmp_path, textures, kd="k"):
    p = tmp_path / "s.pbrt"
    p.write_text(_SCENE.format(textures=textures, kd=kd))
    return host.PbrtScene(str(p))


def _by_kind(s, kind):
    t = s.table("textures")
    return [i for i in range(len(t)) if t[i]["kind"] == kind]


def test_loader_builds_a_planar_checkerboard_with_the_file_words(tmp_path):
    s = _load(tmp_path, 'Texture "k" "spectrum" "checkerboard" "string mapping" "planar" "vector v1" [0.5 -0.25 2] "vector3 v2" [0 0.125 -3] '
                        '"float udelta" [0.75] "float vdelta" [-1.5] "float uscale" [7] "float vscale" [9] "string aamode" "none"')
    ids = _by_kind(s, sd.TEX_CHECKER_PLANAR)
    assert len(ids) == 1
    w = s.texture_words(ids[0])
    assert np.array_equal(w.view(np.uint32), np.float32([0.5, -0.25, 2, 0, 0.125, -3, 0.75, -1.5]).view(np.uint32))  # uscale / vscale play no part
    assert s.table("textures")[ids[0]]["amount"] == 0


def test_loader_planar_defaults(tmp_path):
    s = _load(tmp_path, 'Texture "k" "spectrum" "checkerboard" "string mapping" "planar"')
    (i,) = _by_kind(s, sd.TEX_CHECKER_PLANAR)
    assert np.array_equal(s.texture_words(i), np.float32([1, 0, 0, 0, 1, 0, 0, 0]))
    assert s.table("textures")[i]["amount"] == 1  # closedform


def _ctm_words(s, kind=sd.TEX_FBM_MAPPED):
    ids = _by_kind(s, kind)
    assert len(ids) == 1
    return s.texture_words(ids[0]).reshape(4, 4)


@pytest.mark.parametrize("xf, m", [
    ("Translate 1 -2 0.5", [[1, 0, 0, 1], [0, 1, 0, -2], [0, 0, 1, 0.5], [0, 0, 0, 1]]),
    ("Scale 2 0.5 -4", [[2, 0, 0, 0], [0, 0.5, 0, 0], [0, 0, -4, 0], [0, 0, 0, 1]]),
    ("Translate 1 2 3\nScale 2 2 2", [[2, 0, 0, 1], [0, 2, 0, 2], [0, 0, 2, 3], [0, 0, 0, 1]]),
    ("Transform [1 0 0 0.25  0 2 0 0  0 0 1 0  3 4 5 1]", [[1, 0, 0, 3], [0, 2, 0, 4], [0, 0, 1, 5], [0.25, 0, 0, 1]]),  # column-major in the file
])
def test_loader_maps_fbm_under_a_transform_with_the_ctm(tmp_path, xf, m):
    s = _load(tmp_path, f'AttributeBegin\n{xf}\nTexture "k" "spectrum" "fbm" "float omega" [0.25] "integer octaves" [5]\nAttributeEnd')
    w = _ctm_words(s)
    assert np.array_equal(w.view(np.uint32), np.float32(m).view(np.uint32))  # the CTM itself (the reference's world_to_texture), not its inverse
    t = s.table("textures")[_by_kind(s, sd.TEX_FBM_MAPPED)[0]]
    assert t["value"][0] == np.float32(0.25) and t["amount"] == 5


def test_loader_keeps_identity_fbm_as_before(tmp_path):
    s = _load(tmp_path, 'AttributeBegin\nTranslate 0 0 0\nTexture "k" "spectrum" "fbm"\nAttributeEnd')
    assert len(_by_kind(s, sd.TEX_FBM)) == 1 and not _by_kind(s, sd.TEX_FBM_MAPPED)


def test_loader_float_fbm_under_scale_as_bump(tmp_path):
    s = _load(tmp_path, 'Texture "k" "spectrum" "constant" "rgb value" [0.5 0.5 0.5]\nTransformBegin\nScale 2 3 4\n'
                        'Texture "b" "float" "fbm" "float omega" [0.5]\nTransformEnd\nMaterial "matte" "texture bumpmap" "b"')
    assert np.array_equal(_ctm_words(s), np.float32(np.diag([2, 3, 4, 1])))


@pytest.mark.parametrize("textures, needle", [
    ('Texture "k" "spectrum" "checkerboard" "string mapping" "spherical"', "unimplemented"),
    ('Texture "k" "spectrum" "checkerboard" "string mapping" "cylindrical"', "unimplemented"),
    ('Texture "k" "spectrum" "checkerboard" "integer dimension" [3]', "dimension 2"),
    ('Texture "k" "spectrum" "imagemap" "string filename" "x.png" "string mapping" "planar"', "imagemap"),
    ('Texture "k" "spectrum" "uv" "string mapping" "planar"', "uv texture"),
])
def test_loader_keeps_the_remaining_refusals(tmp_path, textures, needle):
    with pytest.raises(host.BackendError, match=needle):
        _load(tmp_path, textures)


@pytest.mark.parametrize("cls, kind", [("checkerboard", sd.TEX_CHECKER), ("uv", sd.TEX_UV)])
def test_loader_falls_back_to_uv_for_an_unknown_mapping(tmp_path, cls, kind):
    s = _load(tmp_path, f'Texture "k" "spectrum" "{cls}" "string mapping" "warped" "float uscale" [4] "float udelta" [0.5]')
    ids = _by_kind(s, kind)
    assert len(ids) == 1
    assert np.array_equal(s.table("textures")[ids[0]]["mapping"], np.float32([1, 1, 0, 0]))  # UVMapping2D(1, 1, 0, 0), as the reference
    assert s.n_warnings >= 1 and "warped" in s.first_warning, (s.n_warnings, s.first_warning)


def _mapped_scene():
    d = cornell_box(16, 16, 1)
    f = d.fbm_tex(0.4, 6, tex2world=[[2, 0, 0, 1], [0, 0.5, 0, -2], [0, 0, 1, 0.25], [0, 0, 0, 1]])
    c = d.checker_tex((0.9, 0.1, 0.1), f, mapping="planar", v1=(0.5, 0, 0.25), v2=(0, 2, 0), udelta=0.5, vdelta=-0.25)
    deep = d.mix_tex(d.scale_tex(c, d.checker_tex(d.uv_tex(2, 2), c, 3, 3)), d.const_tex(0.2), d.scale_tex(f, d.const_tex(0.5)))
    m = d.set_bump(d.matte(deep), d.scale_tex(d.fbm_tex(0.5, 4, tex2world=np.diag([1, 2, 3, 1])), d.const_tex(0.02)))
    d._mat[0][:] = m
    return d


def test_export_round_trips_mapped_textures(tmp_path):
    d = _mapped_scene()
    a = host.HostScene(d)
    path = str(tmp_path / "m.pbrt")
    write_pbrt(d, path)
    b = host.PbrtScene(path)
    ta, tb = a.table("textures"), b.table("textures")
    # (the exporter writes a texture once per type it is used as: the fbm under the planar checkerboard is a spectrum there and a float in the mix amount)
    ka = {(int(t["kind"]), float(t["value"][0]), int(t["amount"]), a.texture_words(i).tobytes()) for i, t in enumerate(ta) if t["kind"] in (sd.TEX_CHECKER_PLANAR, sd.TEX_FBM_MAPPED)}
    kb = {(int(t["kind"]), float(t["value"][0]), int(t["amount"]), b.texture_words(i).tobytes()) for i, t in enumerate(tb) if t["kind"] in (sd.TEX_CHECKER_PLANAR, sd.TEX_FBM_MAPPED)}
    assert ka == kb and len(ka) == 3
    text = open(path).read()
    assert '"string mapping" "planar"' in text and "TransformBegin" in text


# ---------------------------------------------------------------- rt_scene_create's checks (made before any device is touched)
def _create(texs, block_words=16, mat_kind=sd.MAT_MATTE, mat_slot=-1, pyramid_first=False):
    """rt_scene_create over `texs` (kind, tex1, tex2, amount, image) tuples, image 0 = a word block of `block_words` words, image 1 = a 1x1 pyramid
    (swapped with pyramid_first), one material; the rest of the description is empty."""
    keep = []
    words = np.arange((block_words + 2) // 3 * 3, dtype=np.float32)
    px = np.zeros(3, np.float32); keep += [words, px]
    imgs = (RtImage * 2)()
    b, p = (1, 0) if pyramid_first else (0, 1)
    imgs[b].n_levels = 0; imgs[b].texels = words.ctypes.data; imgs[b].n_texels = words.size // 3
    if not any(k in (CP, FM) for k, *_ in texs) and mat_kind != sd.MAT_FOURIER:  # a block no mapped texture names would be a Fourier table: a pyramid instead
        imgs[b].n_levels = 1; imgs[b].width[0] = imgs[b].height[0] = 1; imgs[b].texels = px.ctypes.data; imgs[b].n_texels = 1
    imgs[p].n_levels = 1; imgs[p].width[0] = imgs[p].height[0] = 1; imgs[p].texels = px.ctypes.data; imgs[p].n_texels = 1
    tx = (RtTexture * len(texs))()
    for i, (k, t1, t2, am, im) in enumerate(texs):
        tx[i].kind, tx[i].tex1, tx[i].tex2, tx[i].amount, tx[i].image = k, t1, t2, am, im
        tx[i].mapping[0] = tx[i].mapping[1] = 1.0
    mats = (RtMaterial * 1)()
    mats[0].kind = mat_kind; mats[0].bump = -1
    for k in range(16):
        mats[0].slot[k] = -1
    mats[0].slot[0] = 0 if texs else -1
    mats[0].slot[14] = mat_slot
    d = RtSceneDesc()
    d.n_images, d.images = 2, C.cast(imgs, C.c_void_p)
    d.n_materials, d.materials = 1, C.cast(mats, C.c_void_p)
    d.n_textures, d.textures = len(texs), C.cast(tx, C.c_void_p)
    out = C.c_void_p()
    L = host.hip_lib()
    rc = L.rt_scene_create(C.byref(d), -1, C.byref(out))
    msg = L.rt_last_error().decode()
    if rc == 0:
        L.rt_scene_destroy(out)
    return rc, msg


K, SC, MX, CH, CP, FM = sd.TEX_CONST, sd.TEX_SCALE, sd.TEX_MIX, sd.TEX_CHECKER, sd.TEX_CHECKER_PLANAR, sd.TEX_FBM_MAPPED


def _passes(rc, msg):
    return rc != RT_ERR_INVALID or msg == "empty scene"  # RT_ERR_NO_DEVICE here, "empty scene" on a GPU box: the texture checks passed


def _root_first(t, root):
    """the same graph with texture `root` moved to id 0 (the material's Kd)"""
    perm = [root] + [i for i in range(len(t)) if i != root]
    where = {old: new for new, old in enumerate(perm)}
    m = lambda i: where[i] if i >= 0 else -1
    return [(t[o][0], m(t[o][1]), m(t[o][2]), m(t[o][3]) if t[o][0] == MX else t[o][3], t[o][4]) for o in perm]


def test_scene_create_accepts_deep_graphs_and_mapped_kinds():
    t = [(K, -1, -1, -1, -1)]
    for i in range(12):  # 12 deep, every other level a mix whose amount is the combinator below
        t.append((MX, len(t) - 1, 0, len(t) - 1, -1) if i % 2 else (SC, len(t) - 1, 0, -1, -1))
    assert _passes(*_create(_root_first(t, len(t) - 1)))
    assert _passes(*_create([(CP, 1, 2, 1, 0), (K, -1, -1, -1, -1), (FM, -1, -1, 3, 0)]))


def test_scene_create_refuses_a_cycle():
    rc, msg = _create([(SC, 1, 2, -1, -1), (MX, 2, 2, 0, -1), (K, -1, -1, -1, -1)])
    assert rc == RT_ERR_INVALID and "cycle" in msg, msg
    rc, msg = _create([(CH, 0, 1, 1, -1), (K, -1, -1, -1, -1)])  # a checkerboard that is its own operand
    assert rc == RT_ERR_INVALID and "cycle" in msg, msg


@pytest.mark.parametrize("texs, needle", [
    ([(SC, 1, 5, -1, -1), (K, -1, -1, -1, -1)], "operand out of range"),
    ([(MX, 1, 1, 9, -1), (K, -1, -1, -1, -1)], "mix amount out of range"),
    ([(CP, 1, -1, 1, 0), (K, -1, -1, -1, -1)], "operand out of range"),
    ([(FM, -1, -1, 4, 7)], "out of range"),
    ([(FM, -1, -1, 4, 1)], "MIP pyramid"),
    ([(CP, 1, 1, 1, 1), (K, -1, -1, -1, -1)], "MIP pyramid"),
    ([(12, -1, -1, -1, -1)], "unknown texture kind"),
])
def test_scene_create_refuses_bad_operands_and_blocks(texs, needle):
    rc, msg = _create(texs)
    assert rc == RT_ERR_INVALID and needle in msg, msg


def test_scene_create_refuses_short_blocks():
    rc, msg = _create([(FM, -1, -1, 4, 0)], block_words=15)
    assert rc == RT_ERR_INVALID and "shorter than 16 words" in msg, msg
    rc, msg = _create([(CP, 1, 1, 1, 0), (K, -1, -1, -1, -1)], block_words=6)  # (blocks are whole texels: 6 words)
    assert rc == RT_ERR_INVALID and "shorter than 8 words" in msg, msg
    assert _passes(*_create([(CP, 1, 1, 1, 0), (K, -1, -1, -1, -1)], block_words=8))


def test_scene_create_refuses_crossed_references_to_a_block():
    rc, msg = _create([(FM, -1, -1, 4, 0)], mat_kind=sd.MAT_FOURIER, mat_slot=0)
    assert rc == RT_ERR_INVALID and "word block" in msg and "Fourier" in msg, msg
    rc, msg = _create([(FM, -1, -1, 4, 0), (sd.TEX_IMAGE, -1, -1, -1, 0)])
    assert rc == RT_ERR_INVALID and "image texture" in msg, msg


def _shared(n):
    """X_k = scale(c, c) for k < n, read by two chains A_k = scale(A_{k-1}, X_k) and B_k = scale(B_{k-1}, X_k), root = scale(A, B): evaluating A first
    leaves every X_k alive until B reads it"""
    t = [(K, -1, -1, -1, -1)]
    xs = []
    for _ in range(n):
        t.append((SC, 0, 0, -1, -1)); xs.append(len(t) - 1)
    a = b = 0
    for x in xs:
        t.append((SC, a, x, -1, -1)); a = len(t) - 1
    for x in xs:
        t.append((SC, b, x, -1, -1)); b = len(t) - 1
    t.append((SC, a, b, -1, -1))
    return _root_first(t, len(t) - 1)


def _complete_tree(depth):
    """a complete binary tree of scale combinators `depth` levels deep over constants: 2^depth - 1 combinators, Sethi-Ullman number `depth`"""
    t = [(K, -1, -1, -1, -1)]
    level = [0] * (1 << depth)
    while len(level) > 1:
        nxt = []
        for a, b in zip(level[::2], level[1::2]):
            t.append((SC, a, b, -1, -1)); nxt.append(len(t) - 1)
        level = nxt
    return _root_first(t, len(t) - 1)


def test_scene_create_bounds_the_value_slots_by_name():
    t = _complete_tree(8)  # 255 combinators that need 8 values at once: RT_TEX_SLOTS
    assert sum(1 for x in t if x[0] == SC) == 255
    assert _passes(*_create(t))
    assert _passes(*_create(_shared(7)))  # 7 shared values and the running chain
    rc, msg = _create(_complete_tree(9))
    assert rc == RT_ERR_INVALID and "value slots" in msg and "RT_TEX_SLOTS" in msg and "texture 0" in msg, msg
    rc, msg = _create(_shared(8))
    assert rc == RT_ERR_INVALID and "value slots" in msg, msg
