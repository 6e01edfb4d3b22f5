"""rt_scene_create's checks of a scene description (rtx_scene_plan.h), without a GPU: every refusal is made before the device is asked for, so a faulty description
gets the same code and message on any machine, and a valid one gets RT_ERR_NO_DEVICE here (RT_OK where there is a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rustracer_amd import host, scenes
from rustracer_amd import scene_desc as sd

from util import RtBvhNode, RtImage, RtInstance, RtLight, RtMaterial, RtSceneDesc, RtSphere, RtTexture, RtTriMeta

RT_OK, RT_ERR_INVALID, RT_ERR_NO_DEVICE, RT_ERR_UNSUPPORTED = 0, -1, -2, -5
HAS_N, HAS_UV, HAS_S, HAS_ALPHA, SPHERE, INSTANCE = 2, 4, 8, 16, 64, 128
KD, SIGMA, M1, M2 = 0, 4, 14, 15
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]


def test_mirrors_have_the_header_sizes():
    for cls, name in ((RtBvhNode, b"rt_bvh_node"), (RtTriMeta, b"rt_tri_meta"), (RtSphere, b"rt_sphere"), (RtInstance, b"rt_instance"), (RtLight, b"rt_light")):
        assert host.hip_lib().rt_sizeof(name) == C.sizeof(cls), name


def _bits(i):
    return float(np.uint32(i).view(np.float32))


class Desc:
    """A scene description as Python lists, one dict per record; create() flattens it into the C structs and calls rt_scene_create. The default is the
    smallest valid scene: one leaf node over one triangle, one matte material over two constant textures."""

    def __init__(self):
        self.nodes = [dict(bmin=(0, 0, 0), bmax=(1, 1, 1), offset=0, n_prims=1)]
        self.tri_p = [[0, 0, 0, 1, 0, 0, 0, 1, 0]]
        self.meta = [dict(material=0, light=-1, flags=0)]
        self.tri_n = self.tri_uv = self.tri_s = self.alpha = None
        self.textures = [dict(kind=sd.TEX_CONST, value=(0.5, 0.5, 0.5)), dict(kind=sd.TEX_CONST)]
        self.materials = [dict(kind=sd.MAT_MATTE, slots={KD: 0, SIGMA: 1})]
        self.spheres, self.instances, self.images, self.lights = [], [], [], []
        self.n_unlisted = self.n_top_nodes = self.n_top_prims = 0
        self.null = set()  # tables handed over as NULL although their count says otherwise
        self.keep = []

    def add_prim(self, p, **meta):
        self.tri_p.append(list(p)); self.meta.append(dict(dict(material=0, light=-1, flags=0), **meta))
        self.nodes[0]["n_prims"] = len(self.tri_p)  # (one leaf over every top-level primitive)
        return len(self.tri_p) - 1

    def add_texture(self, kind, tex1=-1, tex2=-1, amount=-1, image=-1):
        self.textures.append(dict(kind=kind, tex1=tex1, tex2=tex2, amount=amount, image=image))
        return len(self.textures) - 1

    def add_words(self, words, n_texels=None):
        """an image with n_levels == 0 over `words` (a word block, or a Fourier BSDF table); n_texels: what the record claims, if not what is there"""
        w = np.ascontiguousarray(words, np.uint32) if words is not None else None
        self.images.append(dict(n_levels=0, texels=w, n_texels=(w.size // 3 if n_texels is None else n_texels)))
        return len(self.images) - 1

    def add_pyramid(self, **kw):
        self.images.append(dict(dict(n_levels=1, width=1, height=1, offset=0, texels=np.zeros(3, np.float32), n_texels=1), **kw))
        return len(self.images) - 1

    def add_infinite(self, image):
        one, cdf = np.ones(1, np.float32), np.float32([0, 1])
        self.lights.append(dict(kind=3, image=image, dist_nu=1, dist_nv=1, dist_func=one, dist_cdf=cdf, dist_func_int=one, marg_func=one, marg_cdf=cdf, marg_func_int=1.0))

    def _array(self, cls, records, fill):
        arr = (cls * max(len(records), 1))()
        for a, r in zip(arr, records):
            fill(a, r)
        self.keep.append(arr)
        return C.cast(arr, C.c_void_p)

    def _floats(self, a, width):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.float32 if width else np.int32); self.keep.append(a)
        return a.ctypes.data

    def create(self):
        def node(a, r):
            a.bmin[:], a.bmax[:], a.offset, a.n_prims = r["bmin"], r["bmax"], r["offset"], r["n_prims"]

        def meta(a, r):
            a.material, a.light, a.flags = r["material"], r["light"], r["flags"]

        def sphere(a, r):
            a.o2w[:], a.w2o[:], a.radius, a.z_min, a.z_max, a.theta_min, a.theta_max, a.phi_max = IDENTITY, IDENTITY, 1, -1, 1, np.pi, 0, 2 * np.pi

        def instance(a, r):
            a.o2w[:], a.w2o[:], a.node_base, a.n_nodes, a.prim_base, a.n_prims = IDENTITY, IDENTITY, r["node_base"], r["n_nodes"], r["prim_base"], r["n_prims"]

        def texture(a, r):
            a.kind, a.tex1, a.tex2, a.amount, a.image = r["kind"], r.get("tex1", -1), r.get("tex2", -1), r.get("amount", -1), r.get("image", -1)
            a.value[:], a.mapping[:] = r.get("value", (0, 0, 0)), (1, 1, 0, 0)

        def image(a, r):
            a.n_levels, a.n_texels = r["n_levels"], r["n_texels"]
            a.width[0], a.height[0], a.offset[0] = r.get("width", 0), r.get("height", 0), r.get("offset", 0)
            if r["texels"] is not None:
                self.keep.append(r["texels"]); a.texels = r["texels"].ctypes.data

        def material(a, r):
            a.kind, a.bump = r["kind"], r.get("bump", -1)
            a.slot[:] = [r["slots"].get(k, -1) for k in range(16)]

        def light(a, r):
            a.kind, a.prim, a.image, a.dist_nu, a.dist_nv, a.marg_func_int = r["kind"], r.get("prim", -1), r.get("image", -1), r.get("dist_nu", 0), r.get("dist_nv", 0), r.get("marg_func_int", 0)
            a.rgb[:], a.area, a.world_radius = (1, 1, 1), 0.5, 2
            for f in ("dist_func", "dist_cdf", "dist_func_int", "marg_func", "marg_cdf"):
                if r.get(f) is not None:
                    self.keep.append(r[f]); setattr(a, f, r[f].ctypes.data)

        d = RtSceneDesc()
        d.n_nodes, d.nodes = len(self.nodes), self._array(RtBvhNode, self.nodes, node)
        d.n_tris, d.tri_p, d.tri_meta = len(self.tri_p), self._floats(self.tri_p, 9), self._array(RtTriMeta, self.meta, meta)
        d.tri_n, d.tri_uv, d.tri_s, d.tri_alpha = self._floats(self.tri_n, 9), self._floats(self.tri_uv, 6), self._floats(self.tri_s, 9), self._floats(self.alpha, 0)
        d.n_spheres, d.spheres = len(self.spheres), self._array(RtSphere, self.spheres, sphere)
        d.n_instances, d.instances = len(self.instances), self._array(RtInstance, self.instances, instance)
        d.n_textures, d.textures = len(self.textures), self._array(RtTexture, self.textures, texture)
        d.n_images, d.images = len(self.images), self._array(RtImage, self.images, image)
        d.n_materials, d.materials = len(self.materials), self._array(RtMaterial, self.materials, material)
        d.n_lights, d.lights = len(self.lights) - self.n_unlisted, self._array(RtLight, self.lights, light)
        d.n_unlisted_lights, d.n_top_nodes, d.n_top_prims = self.n_unlisted, self.n_top_nodes, self.n_top_prims
        for name in self.null:
            setattr(d, name, None)
        out = C.c_void_p()
        L = host.hip_lib()
        rc = L.rt_scene_create(C.byref(d), -1, C.byref(out))
        msg = L.rt_last_error().decode()
        if rc == RT_OK:
            L.rt_scene_destroy(out)
        return rc, msg


# ---- the variants of the minimal scene
def minimal():
    return Desc()


def with_sphere():
    d = Desc()
    d.spheres.append({})
    d.add_prim([-1, -1, -1, 1, 1, 1, _bits(0), 0, 0], flags=SPHERE)
    return d


def with_instance():
    """the top level: one instance primitive; the object: one triangle under a one-node tree of its own"""
    d = Desc()
    d.tri_p[0][6] = _bits(0); d.meta[0]["flags"] = INSTANCE
    d.tri_p.append([0, 0, 0, 1, 0, 0, 0, 1, 0]); d.meta.append(dict(material=0, light=-1, flags=0))
    d.nodes.append(dict(bmin=(0, 0, 0), bmax=(1, 1, 1), offset=0, n_prims=1))
    d.instances.append(dict(node_base=1, n_nodes=1, prim_base=1, n_prims=1))
    d.n_top_nodes = d.n_top_prims = 1
    return d


def with_mask():
    d = Desc()
    d.meta[0]["flags"] = HAS_ALPHA; d.alpha = [[1, -1]]
    return d


def with_infinite():
    d = Desc()
    d.add_infinite(d.add_pyramid())
    return d


def with_mix():
    d = Desc()
    d.materials.append(dict(kind=sd.MAT_MIX, slots={M1: 0, M2: 0}))
    d.meta[0]["material"] = 1
    return d


def with_area_light():
    d = Desc()
    d.lights.append(dict(kind=0, prim=0)); d.meta[0]["light"] = 0
    return d


VARIANTS = [minimal, with_sphere, with_instance, with_mask, with_infinite, with_mix, with_area_light]


def _valid(rc):
    return rc == (RT_OK if host.device_available() else RT_ERR_NO_DEVICE)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda f: f.__name__)
def test_valid_descriptions_reach_the_device(variant):
    rc, msg = variant().create()
    assert _valid(rc), (rc, msg)


@pytest.mark.parametrize("name, make", [
    ("cornell", lambda: scenes.cornell_box(16, 16, 1)), ("soup", lambda: scenes.random_soup(300, seed=3)), ("blob", lambda: scenes.blob_scene(32, 16, 16, 16, 1)),
    ("mis", lambda: scenes.mis_plates(16, 16, 1, sphere_level=1)), ("mis-spheres", lambda: scenes.mis_plates(16, 16, 1, analytic_spheres=True)),
    ("room", lambda: scenes.room_env(16, 16, 1, detail=2.0, tex_size=16, env_size=16)), ("forest", lambda: scenes.forest(3, 1, 1, res=(16, 16))),
    ("forest-flat", lambda: scenes.forest(3, 1, 1, two_level=False, res=(16, 16)))])
def test_scene_generators_reach_the_device(name, make):
    h = host.HostScene(make())
    if host.device_available():
        h.upload(0)
    else:
        with pytest.raises(host.BackendError, match=r"\(-2\)"):
            h.upload(0)


# ---- refusals: (message, code, variant, mutation). Every message rt_plan_scene can give is here, in the order of the checks.
def fourier_words(n_mu=2, m_max=1, n_ch=1, n_coeffs=0, eta=1.0, mu=(-1.0, 1.0), cell=(0, 0)):
    """the words of a Fourier BSDF table (rtx_hip.h, rt_image): header, mu, cdf, (offset, length) per cell - and no coefficients"""
    w = np.concatenate([np.uint32([n_mu, m_max, n_ch, n_coeffs]), np.float32([eta]).view(np.uint32), np.float32(mu).view(np.uint32), np.zeros(n_mu * n_mu, np.uint32),
                        np.tile(np.uint32(cell), n_mu * n_mu)])
    return np.concatenate([w, np.zeros((-w.size) % 3, np.uint32)])


def complete_tree(d, depth):
    """a complete binary tree of scale combinators over constant 0, `depth` levels: it needs `depth` values at once (its Sethi-Ullman number)"""
    level = [0] * (1 << depth)
    while len(level) > 1:
        level = [d.add_texture(sd.TEX_SCALE, a, b) for a, b in zip(level[::2], level[1::2])]
    return level[0]


def scale_chain(d, n):
    """t_k = scale(t_{k-1}, constant), n deep. From k = 3 on a root is past the two-level evaluator and gets a program over its whole sub-graph: 8 words of
    block, the count and 5 words per combinator, in whole 12-word records. Returns the root whose program takes the scene past 2^24 words."""
    total, over, t = 0, None, 0
    for k in range(1, n + 1):
        t = d.add_texture(sd.TEX_SCALE, t, 0)
        if k >= 3 and over is None:
            total += (9 + 5 * k + 11) // 12 * 12
            over = t if total > 1 << 24 else None
    assert over is not None
    return over


def _set(path, value):
    """mutation: d.<table>[i][field] = value, or d.<attr> = value"""
    def f(d):
        if len(path) == 1:
            setattr(d, path[0], value)
        else:
            getattr(d, path[0])[path[1]][path[2]] = value
    return f


def _do(*steps):
    def f(d):
        for s in steps:
            s(d)
    return f


MAPPED = lambda d: d.add_texture(sd.TEX_FBM_MAPPED, amount=4, image=d.add_words(np.zeros(18, np.uint32)))  # noqa: E731  (texture 2 over the word block image 0)
TABLE = lambda d: d.add_words(fourier_words())  # noqa: E731
HUGE = (1 << 27) + 100  # coefficients a table claims (none is read before the sizes are refused)
I, U = RT_ERR_INVALID, RT_ERR_UNSUPPORTED

REFUSALS = [
    # texture_programs
    ("texture table missing", I, minimal, lambda d: d.null.add("textures")),
    ("texture 0: unknown texture kind", I, minimal, _set(("textures", 0, "kind"), 12)),
    ("texture 2: texture operand out of range", I, minimal, lambda d: d.add_texture(sd.TEX_SCALE, 0, 7)),
    ("texture 2: mix amount out of range", I, minimal, lambda d: d.add_texture(sd.TEX_MIX, 0, 1, 9)),
    ("texture 2: word block image index out of range", I, minimal, lambda d: d.add_texture(sd.TEX_FBM_MAPPED, amount=4, image=5)),
    ("texture 2: a mapped texture names a MIP pyramid, not a word block (n_levels == 0)", I, minimal, lambda d: d.add_texture(sd.TEX_FBM_MAPPED, amount=4, image=d.add_pyramid())),
    ("texture 2: word block shorter than 16 words", I, minimal, lambda d: d.add_texture(sd.TEX_FBM_MAPPED, amount=4, image=d.add_words(np.zeros(15, np.uint32)))),
    ("texture 2: the texture graph has a cycle", I, minimal, lambda d: d.add_texture(sd.TEX_SCALE, 2, 0)),
    ("texture 512: its graph needs at least 9 value slots, more than the 8 (RT_TEX_SLOTS) of the device evaluator", I, minimal, lambda d: complete_tree(d, 9)),
    (None, I, minimal, lambda d: "texture %d: the scene's texture programs would exceed 16777216 words (graphs nested that deep are not supported)" % scale_chain(d, 2600)),
    # fourier_table_error / fourier_desc_error
    ("image 0: Fourier BSDF table without words", I, minimal, lambda d: d.add_words(None, n_texels=7)),
    ("image 0: Fourier BSDF table larger than 2^28 words", I, minimal, lambda d: d.add_words(fourier_words(), n_texels=(1 << 28) + 1)),
    ("image 0: Fourier BSDF table shorter than its header", I, minimal, lambda d: d.add_words(fourier_words(), n_texels=1)),
    ("image 0: Fourier BSDF table: nMu must lie in [2, 8192]", I, minimal, lambda d: d.add_words(fourier_words(n_mu=1, mu=(0.0,)))),
    ("image 0: Fourier BSDF table: nChannels must be 1 or 3", I, minimal, lambda d: d.add_words(fourier_words(n_ch=2))),
    ("image 0: Fourier BSDF table: nCoeffs larger than 2^28", I, minimal, lambda d: d.add_words(fourier_words(n_coeffs=(1 << 28) + 1))),
    ("image 0: Fourier BSDF table: eta is not finite", I, minimal, lambda d: d.add_words(fourier_words(eta=np.inf))),
    ("image 0: Fourier BSDF table: sizes do not add up (19 words for 8 texels)", I, minimal, lambda d: d.add_words(np.concatenate([fourier_words(), np.zeros(3, np.uint32)]))),
    ("image 0: Fourier BSDF table: mu is not strictly ascending", I, minimal, lambda d: d.add_words(fourier_words(mu=(0.5, 0.5)))),
    ("image 0: Fourier BSDF table: a cell's length exceeds mMax", I, minimal, lambda d: d.add_words(fourier_words(cell=(0, 2)))),
    ("image 0: Fourier BSDF table: a cell's coefficients run past nCoeffs", I, minimal, lambda d: d.add_words(fourier_words(cell=(0, 1)))),
    ("Fourier BSDF tables larger than 2^28 words in all", I, minimal, lambda d: [d.add_words(fourier_words(n_coeffs=HUGE), n_texels=(19 + HUGE + 2) // 3) for _ in range(2)]),
    ("material 0: a Fourier material names the word block of a mapped texture, not a Fourier BSDF table", I, minimal,
     _do(MAPPED, _set(("materials", 0, "kind"), sd.MAT_FOURIER), _set(("materials", 0, "slots"), {M1: 0}))),
    ("material 0: a Fourier material must name a Fourier BSDF table (n_levels == 0) in slot M1, not a MIP pyramid", I, minimal,
     _do(Desc.add_pyramid, _set(("materials", 0, "kind"), sd.MAT_FOURIER), _set(("materials", 0, "slots"), {M1: 0}))),
    ("texture 2: an image texture names a Fourier BSDF table, not a MIP pyramid", I, minimal, lambda d: d.add_texture(sd.TEX_IMAGE, image=TABLE(d))),
    ("texture 3: an image texture names the word block of a mapped texture, not a MIP pyramid", I, minimal, _do(MAPPED, lambda d: d.add_texture(sd.TEX_IMAGE, image=0))),
    ("light 0: an infinite light names a Fourier BSDF table, not a MIP pyramid", I, with_infinite, lambda d: _set(("lights", 0, "image"), TABLE(d))(d)),
    ("light 0: an infinite light names the word block of a mapped texture, not a MIP pyramid", I, with_infinite,
     lambda d: _set(("lights", 0, "image"), d.add_words(np.zeros(18, np.uint32)))(d) or d.add_texture(sd.TEX_FBM_MAPPED, amount=4, image=1)),
    # the description itself
    ("empty scene", I, minimal, _do(_set(("tri_p",), []), _set(("meta",), []))),
    ("tri flags need tri_n", I, minimal, _set(("meta", 0, "flags"), HAS_N)),
    ("tri flags need tri_uv", I, minimal, _set(("meta", 0, "flags"), HAS_UV)),
    ("tri flags need tri_s", I, minimal, _set(("meta", 0, "flags"), HAS_S)),
    ("instance index out of range", I, with_instance, lambda d: d.tri_p[0].__setitem__(6, _bits(5))),
    ("an instance primitive carries triangle attributes or a light", I, with_instance, _set(("meta", 0, "flags"), INSTANCE | 1)),
    ("material index out of range", I, minimal, _set(("meta", 0, "material"), 3)),
    ("light index out of range", I, minimal, _set(("meta", 0, "light"), 0)),
    ("tri flags need tri_alpha", I, with_mask, _set(("alpha",), None)),
    ("alpha texture out of range", I, with_mask, _set(("alpha",), [[9, -1]])),
    ("alpha texture 32: its graph needs 5 value slots, more than the 4 (RT_TEX_MASK_SLOTS) a mask has", U, with_mask, lambda d: _set(("alpha",), [[complete_tree(d, 5), -1]])(d)),
    ("sphere index out of range", I, with_sphere, lambda d: d.tri_p[1].__setitem__(6, _bits(4))),
    ("a sphere primitive carries triangle attributes", I, with_sphere, _do(_set(("meta", 1, "flags"), SPHERE | HAS_N), _set(("tri_n",), np.zeros((2, 9))))),
    ("bad instance tables", I, with_instance, _set(("n_top_nodes",), 0)),
    ("instance ranges out of bounds", I, with_instance, _set(("instances", 0, "n_prims"), 0)),
    ("an instanced object holds triangles and quadrics only, and no light of the scene's list", U, with_instance,
     _do(lambda d: d.lights.append(dict(kind=0, prim=1)), _set(("meta", 1, "light"), 0))),
    ("bad mip level count", I, minimal, lambda d: d.add_pyramid(n_levels=17)),
    ("MIP level sizes must be powers of two (rc/mipmap.rs:75-139)", I, minimal, lambda d: d.add_pyramid(width=3, texels=np.zeros(9, np.float32), n_texels=3)),
    ("MIP level outside the texel array", I, minimal, lambda d: d.add_pyramid(offset=5)),
    ("image index out of range", I, minimal, lambda d: d.add_texture(sd.TEX_IMAGE, image=7)),
    ("bump texture out of range", I, minimal, _set(("materials", 0, "bump"), 9)),
    ("mix operand out of range", I, with_mix, _set(("materials", 1, "slots"), {M1: 7, M2: 0})),
    ("mix nesting deeper than 2", I, with_mix, lambda d: d.materials.extend([dict(kind=sd.MAT_MIX, slots={M1: 1, M2: 1}), dict(kind=sd.MAT_MIX, slots={M1: 2, M2: 2})])),
    ("infinite light tables missing or larger than 65534 entries per row", I, with_infinite, _set(("lights", 0, "dist_cdf"), None)),
    ("area light prim out of range", I, with_area_light, _set(("lights", 0, "prim"), 9)),
    ("an unlisted emitter must be a diffuse area light", I, minimal, _do(lambda d: d.lights.append(dict(kind=1)), _set(("n_unlisted",), 1))),
    ("more than 4 infinite lights", I, with_infinite, lambda d: [d.add_infinite(0) for _ in range(4)]),
    ("infinite light image out of range", I, with_infinite, _set(("lights", 0, "image"), 3)),
    ("malformed BVH", I, minimal, _set(("nodes", 0, "n_prims"), 2)),
    ("BVH deeper than the 64-entry traversal stack", I, minimal, lambda d: deep_tree(d, 64)),
    ("malformed or too deep object BVH", I, with_instance, _set(("nodes", 1, "n_prims"), 2)),
]
# id accumulates over the instances' n_prims, each of which rt_plan_scene walks first: 2^31 primitive visits before the refusal
NOT_CONSTRUCTIBLE = ["more than 2^31 instanced primitives"]


def deep_tree(d, depth):
    """a chain: every interior node's first child is the next interior node, its second a leaf of one triangle - `depth` levels below the root"""
    d.nodes, d.tri_p, d.meta = [], [], []
    box = dict(bmin=(0, 0, 0), bmax=(1, 1, 1))

    def leaf():
        d.nodes.append(dict(box, offset=len(d.tri_p), n_prims=1))
        d.tri_p.append([0, 0, 0, 1, 0, 0, 0, 1, 0]); d.meta.append(dict(material=0, light=-1, flags=0))

    interior = []
    for _ in range(depth):
        interior.append(len(d.nodes)); d.nodes.append(dict(box, offset=0, n_prims=0))
    leaf()
    for i in reversed(interior):
        d.nodes[i]["offset"] = len(d.nodes); leaf()


@pytest.mark.parametrize("message, code, variant, mutate", REFUSALS, ids=[(m or "texture programs exceed 2^24 words")[:60] for m, *_ in REFUSALS])
def test_refusals(message, code, variant, mutate):
    d = variant()
    computed = mutate(d)
    rc, msg = d.create()
    assert (rc, msg) == (code, message if message is not None else computed)


def test_a_deep_tree_within_the_stack_is_valid():
    d = Desc(); deep_tree(d, 63)
    rc, msg = d.create()
    assert _valid(rc), (rc, msg)


def test_every_refusal_of_the_plan_is_in_the_table():
    """every string literal of rtx_scene_plan.h outside comments, includes, static_assert and getenv is (part of) a message that the table above expects"""
    src = open(os.path.join(os.path.dirname(host.__file__), "csrc", "rtx_scene_plan.h")).read()
    expected = [m for m, *_ in REFUSALS if m] + NOT_CONSTRUCTIBLE + ["texture 0: the scene's texture programs would exceed 16777216 words (graphs nested that deep are not supported)"]
    literals = set()
    for line in src.splitlines():
        line = re.sub(r'(static_assert\(.*|getenv\("[A-Z_]+"\)|^\s*#include.*)', "", line)
        code = re.match(r'((?:[^"/]|"(?:[^"\\]|\\.)*"|/(?!/))*)', line).group(1)  # up to a // comment outside a string
        literals.update(s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', code) if s.strip())
    assert len(literals) > 50
    missing = sorted(s for s in literals if not any(s in m for m in expected))
    assert not missing, missing
