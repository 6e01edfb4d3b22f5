"""ctypes binding of the product libraries (csrc/_build/librtx_host.so -> librtx_hip.so).

`HostScene` plays the role of rustracer's `RealApi` + `world_end` (rc/api.rs:913-1010): it feeds the
unflattened scene description to the C++ host layer (SAH BVH build, flattening, camera/film set-up)
and renders through the HIP backend. Nothing here computes radiance and nothing falls back to a CPU
path: without a GPU `render`/`trace` raise `BackendError`.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
# RTX_LIB_DIR (measurement knob): load librtx_hip.so / librtx_host.so from this directory instead of csrc/_build - another build of the libraries, such as the parent
# commit's in an A/B run (scripts/feature_cost.py) - as they are: build() then compiles nothing.
_BUILD = os.environ.get("RTX_LIB_DIR") or os.path.join(_CSRC, "_build")
HOST_LIB = os.path.join(_BUILD, "librtx_host.so")
HIP_LIB = os.path.join(_BUILD, "librtx_hip.so")

RT_FLAG_COUNT_TRAVERSAL = 1
RT_FLAG_FILM_ON_DEVICE = 2
RT_FLAG_TIME_KERNELS = 4
RT_FLAG_COUNT_AS_RENDERED = 8
RT_FLAG_REF_STREAM = 16
RT_FLAG_FRAME_STATS = 32   # rt_frame_begin: per-pixel luminance moments, adaptive steps
RT_FLAG_FRAME_FEATURES = 64  # rt_frame_begin: per-pixel sums of the samples' first-hit features (albedo, normal, depth, coverage)
RT_FLAG_RAY_DIFFERENTIALS = 128  # rt_render_rays / rt_frame_advance_rays* / rt_camera_rays: ray records of RT_RAY_DIFF_FLOATS floats (the ray, then rx_o, ry_o, rx_d, ry_d)
RT_RAY_DIFF_FLOATS = 20
RT_CAMERA_ORTHOGRAPHIC, RT_CAMERA_ENVIRONMENT = 1, 2  # rt_camera_model_rays / rt_frame_begin_model / rt_render_model: the camera models generated on the device
RT_CAMERA_MODEL_FLOATS = 24
CAMERA_MODELS = dict(orthographic=RT_CAMERA_ORTHOGRAPHIC, environment=RT_CAMERA_ENVIRONMENT)
RT_FEATURE_FLOATS = 16
RT_FEATURE_SAMPLES_MAX = 1 << 25
RT_BSDF_FRONT_AUTO, RT_BSDF_FRONT_GENERIC, RT_BSDF_FRONT_LAMBERT, RT_BSDF_FRONT_TWO_LOBE, RT_BSDF_FRONT_TWO_LOBE_WIDE = range(5)
RT_BSDF_SURFACE_FLOATS = 40
RT_BSDF_OUT_FLOATS = 13
RT_LIGHT_PICK = -1            # rt_light_eval: the light is picked per query as uniform_sample_one_light does
RT_LIGHT_REF_FLOATS = 9
RT_LIGHT_OUT_FLOATS = 20
RT_LIGHT_EVAL_VISIBILITY, RT_LIGHT_EVAL_GENERAL = 1, 2
RT_LIGHT_EVAL_MAX = 1 << 24   # queries per call
LIGHT_STRATEGIES = dict(spatial=0, uniform=1)
RT_SAMPLES_MAX = 1 << 27
RT_RAYS_MAX = 1 << 27       # rt_render_rays: rays per call (4 GiB of rays, 2 GiB of radiance); a larger job is cut by sample range
RT_AO_FLOATS = 4            # rt_render_rays_ao: floats per ray of its output (ao, |d . n|, t, status)
RT_AO_SAMPLES_MAX = 1024    # ... and the most occlusion rays per hit
RT_WHITTED_MAX_DEPTH = 16   # rt_render_whitted / rt_render_rays_whitted: the deepest recursion (Whitted::new(n))
RT_WHITTED_INFO_WORDS = 2   # rt_render_rays_whitted: uint32 per ray of its info output (li invocations, get_2d() draws)
RT_DIRECT_ALL, RT_DIRECT_ONE = 0, 1  # rt_direct_desc.strategy: uniform_sample_all_light / uniform_sample_one_light
RT_DIRECT_STRATEGIES = {"all": RT_DIRECT_ALL, "one": RT_DIRECT_ONE}
RT_DIRECT_MAX_ARRAYS = 1024 # ... 2 * max_depth * n_lights under "all": above it the call is refused
RT_DIRECT_INFO_WORDS = 4    # rt_render_rays_direct: uint32 per ray of its info output (li invocations, get_2d() draws, get_1d() draws, array vertices)
RT_QUERY_DIRECT_LAUNCHED = 9   # rt_scene_query: the same of k_direct_vertex and the last direct-lighting call
RT_QUERY_WHITTED_LAUNCHED = 8  # rt_scene_query: 1 + GENERAL of the k_whitted_vertex instantiation the scene's last Whitted call launched (0: none yet)
RT_QUERY_LDS_SPEC = 7  # rt_scene_query: the form of the closest-hit link walk of an LDS-resident scene of plain triangles (RTX_LDS_SPEC: 0, 1)
RT_QUERY_NEEDS_DIFFERENTIALS = 6  # rt_scene_query: 1 if some texture or bump map of the scene reads ray differentials
RT_QUERY_BSDF_LAUNCHED = 5# rt_scene_query: 1 + 2 * mode + const_tex of the k_bsdf_eval instantiation the scene's last bsdf_eval launched (0 generic, 3 / 5 / 6)
RT_FRAME_XYZW, RT_FRAME_RGB, RT_FRAME_RGB8, RT_FRAME_STATS, RT_FRAME_FEATURES, RT_FRAME_SUMS = range(6)                    # rt_frame_read: what
RT_FRAME_SAMPLES_DONE, RT_FRAME_SPP, RT_FRAME_TABLES_RESIDENT, RT_FRAME_STATE_BYTES, RT_FRAME_SAMPLES_TAKEN, RT_FRAME_ACTIVE_PIXELS = range(6)   # rt_frame_query: what
BSDF_FRONT_ENDS = dict(auto=RT_BSDF_FRONT_AUTO, generic=RT_BSDF_FRONT_GENERIC, lambert=RT_BSDF_FRONT_LAMBERT, two_lobe=RT_BSDF_FRONT_TWO_LOBE,
                       two_lobe_wide=RT_BSDF_FRONT_TWO_LOBE_WIDE)


class BackendError(RuntimeError):
    pass


class RayRecordError(BackendError, ValueError):
    """A ray array whose last axis is neither 8 nor RT_RAY_DIFF_FLOATS floats: a ValueError, and a BackendError as every other refusal of `render_rays` is."""


STAMP = os.path.join(_BUILD, "source.sha")


def source_sha() -> str:
    """sha256 over everything the two libraries are built from (csrc/*.{h,hip,cpp,inl}, the Makefile, include/*.h)."""
    import hashlib
    h = hashlib.sha256()
    files = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith((".h", ".hip", ".cpp", ".inl")) or f == "Makefile"]
    files += [os.path.join(_HERE, "..", "include", f) for f in ("rtx_hip.h", "rtx_host.h")]
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()


def build(force: bool = False) -> None:
    """Compile both libraries for gfx950 (hipcc cross-compiles without a GPU). Whether the built libraries are current is decided by CONTENT: the sha256 of the
    sources is stamped beside them (csrc/_build/source.sha) - the libraries are untracked and travel to the GPU box by snapshot, where file times mean nothing."""
    if os.environ.get("RTX_LIB_DIR"):
        return
    sha = source_sha()
    stamped = open(STAMP).read().strip() if os.path.exists(STAMP) else None
    if force or stamped != sha or not (os.path.exists(HOST_LIB) and os.path.exists(HIP_LIB)):
        subprocess.check_call(["make", "-C", _CSRC, "-s"] + (["-B"] if force or (stamped is not None and stamped != sha) else []))
        with open(STAMP, "w") as f:
            f.write(sha + "\n")


class RenderParams(C.Structure):
    _fields_ = [
        ("xres", C.c_int32), ("yres", C.c_int32), ("crop", C.c_float * 4),
        ("filter_kind", C.c_int32), ("filter_params", C.c_float * 4),
        ("film_scale", C.c_float), ("max_sample_luminance", C.c_float),
        ("cam_to_world", C.c_float * 16), ("cam_to_world_inv", C.c_float * 16),
        ("fov", C.c_float), ("lens_radius", C.c_float), ("focal_distance", C.c_float),
        ("spp", C.c_int32), ("sampler_dims", C.c_int32),
        ("max_depth", C.c_int32), ("rr_threshold", C.c_float), ("light_strategy", C.c_int32),
        ("pixel_bounds", C.c_int32 * 4), ("rank", C.c_int32), ("world_size", C.c_int32), ("flags", C.c_uint32),
        ("screen_window", C.c_float * 4), ("has_pixel_bounds", C.c_int32),
    ]


class AoDesc(C.Structure):
    """rt_ao_desc (rtx_hip.h): the ambient-occlusion integrators' parameters."""
    _fields_ = [("n_samples", C.c_int32), ("max_distance", C.c_float)]


class WhittedDesc(C.Structure):
    """rt_whitted_desc (rtx_hip.h): the Whitted integrator's parameters."""
    _fields_ = [("max_depth", C.c_int32), ("reserved", C.c_int32)]


class DirectDesc(C.Structure):
    """rt_direct_desc (rtx_hip.h): the direct-lighting integrator's parameters."""
    _fields_ = [("max_depth", C.c_int32), ("strategy", C.c_int32), ("reserved", C.c_int32 * 2)]


class Stats(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in (
        "camera_rays", "rays_closest", "rays_shadow", "rays_mis", "nodes_closest", "nodes_shadow", "nodes_mis",
        "tris_closest", "tris_shadow", "tris_mis", "paths_scrubbed")] +
        [(n, C.c_double) for n in ("ms_total", "ms_sampler", "ms_raygen", "ms_trace_closest", "ms_trace_any", "ms_trace_mis",
                                   "ms_shade", "ms_resolve", "ms_film", "ms_lightdist")] +
        [(n, C.c_uint64) for n in ("launches_trace_closest", "n_passes", "vertices_lambert_const", "vertices_lambert", "vertices_two_lobe", "vertices_generic")] +
        [(n, C.c_double) for n in ("ms_shade_lambert_const", "ms_shade_lambert", "ms_shade_two_lobe", "ms_shade_generic", "ms_shade_bin", "ms_shade_miss")] +
        [("shade_section_cycles", C.c_uint64 * 32)] +
        [(n, C.c_uint64) for n in ("rays_mis_any", "nodes_mis_any", "tris_mis_any")] + [("ms_trace_mis_any", C.c_double), ("ms_gather", C.c_double), ("rays_mis_not_cast", C.c_uint64), ("rays_tail_not_cast", C.c_uint64)] +
        [(n, C.c_uint64) for n in ("launches_trace_path", "launches_trace_shadow", "launches_trace_mis", "launches_trace_mis_any", "launches_shade", "rays_shadow_not_cast")])

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n == "shade_section_cycles" else getattr(self, n)) for n, _ in self._fields_}


_lib = None
_hip = None


def lib():
    global _lib, _hip
    if _lib is None:
        if not os.path.exists(HOST_LIB):
            raise BackendError(f"{HOST_LIB} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _hip = C.CDLL(HIP_LIB, mode=C.RTLD_GLOBAL)
        _lib = C.CDLL(HOST_LIB)
        L = _lib
        L.rtxh_scene_new.restype = C.c_void_p
        L.rtxh_scene_free.argtypes = [C.c_void_p]
        L.rtxh_last_error.restype = C.c_char_p
        _hip.rt_last_error.restype = C.c_char_p
        _hip.rt_version.restype = C.c_char_p
        # the mirrors below are positional: a stale library (or a stale mirror) must not be used at all
        for name, mirror in (("rt_stats", Stats), ("rtxh_render_params", RenderParams), ("rtxh_pbrt_result", PbrtResult)):
            n = L.rtxh_sizeof(name.encode())
            if n != C.sizeof(mirror):
                _lib = _hip = None
                raise BackendError(f"{HOST_LIB}: sizeof({name}) = {n}, the ctypes mirror {mirror.__name__} has {C.sizeof(mirror)} bytes - rebuild (make -C rustracer_amd/csrc)")
    return _lib


def hip_lib():
    lib()
    return _hip


def device_available() -> bool:
    return bool(hip_lib().rt_device_available())


def _p(a, t=C.c_float):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _check(rc, what):
    if rc < 0:
        msg = lib().rtxh_last_error()
        raise BackendError(f"{what} failed ({rc}): {msg.decode(errors='replace') if msg else '?'}")
    return rc


def look_at(pos, look, up):
    m = np.zeros((4, 4), np.float32)
    mi = np.zeros((4, 4), np.float32)
    lib().rtxh_look_at(_p(np.float32(pos)), _p(np.float32(look)), _p(np.float32(up)), _p(m), _p(mi))
    return m, mi


def default_screen_window(width, height):
    """pbrt's default screen window of a film of `width` x `height` pixels: the shorter axis spans [-1, 1] (float32 arithmetic, as rtxh_camera_model's)."""
    a = np.float32(width) / np.float32(height)
    if a > 1.0:
        return (float(-a), float(a), -1.0, 1.0)
    return (-1.0, 1.0, float(np.float32(-1.0) / a), float(np.float32(1.0) / a))


def camera_model(kind, camera_to_world, width, height, screen_window=None, lens_radius=0, focal_distance=1e6):
    """The RT_CAMERA_MODEL_FLOATS float32 of a camera model (rt_camera_model_rays, rt_frame_begin_model): camera_to_world (4 x 4, row-major, points as columns:
    `look_at(pos, look, up)[1]`), the screen window (x0, x1, y0, y1) - None: pbrt's default from the aspect ratio width / height -, lens_radius, focal_distance and two
    reserved zeros. `kind`: "orthographic" / "environment" (or the RT_CAMERA_* value). The environment camera reads neither window nor lens: its lens must be 0."""
    if CAMERA_MODELS.get(kind, kind) not in CAMERA_MODELS.values():
        raise BackendError(f"camera_model: unknown kind {kind!r} (orthographic, environment)")
    out = np.zeros(RT_CAMERA_MODEL_FLOATS, np.float32)
    out[:16] = np.asarray(camera_to_world, np.float32).reshape(16)
    out[16:20] = default_screen_window(width, height) if screen_window is None else [float(v) for v in screen_window]
    out[20] = lens_radius
    out[21] = focal_distance
    return out


def _model_args(kind, camera):
    model = CAMERA_MODELS.get(kind, kind)
    cam = np.ascontiguousarray(camera, np.float32).reshape(-1)
    if cam.size != RT_CAMERA_MODEL_FLOATS:
        raise BackendError(f"a camera model is {RT_CAMERA_MODEL_FLOATS} floats (host.camera_model), not {cam.size}")
    return int(model) if isinstance(model, (int, np.integer)) else -1, cam


def screen_window_of(camera):
    """PerspectiveCamera::create (camera.rs:86-107): explicit "screenwindow", else from "frameaspectratio", else (0, 0, 0, 0) = the default."""
    if getattr(camera, "screen_window", None) is not None:
        return tuple(camera.screen_window)
    fr = getattr(camera, "frame_aspect", None)
    if fr is None:
        return (0.0, 0.0, 0.0, 0.0)
    fr = np.float32(fr)
    return (-fr, fr, -1.0, 1.0) if fr > 1.0 else (-1.0, 1.0, np.float32(-1.0) / fr, np.float32(1.0) / fr)


def render_params(desc, rank=0, world_size=1, flags=0) -> RenderParams:
    p = RenderParams()
    f, c, s, it = desc.film, desc.camera, desc.sampler, desc.integrator
    p.xres, p.yres = f.xres, f.yres
    p.crop[:] = [float(x) for x in f.crop]
    p.filter_kind = f.filter_kind
    p.filter_params[:] = [float(x) for x in f.filter_params]
    p.film_scale = f.scale
    p.max_sample_luminance = f.max_sample_luminance
    w2c, c2w = look_at(c.pos, c.look, c.up)  # CTM = identity * LookAt (api.rs:637); camera_to_world = CTM.inverse() (:726)
    w2c, c2w = w2c + np.float32(0.0), c2w + np.float32(0.0)  # the product with the identity CTM turns a -0 entry into +0
    p.cam_to_world[:] = c2w.reshape(-1).tolist()
    p.cam_to_world_inv[:] = w2c.reshape(-1).tolist()
    p.fov, p.lens_radius, p.focal_distance = c.fov, c.lens_radius, c.focal_distance
    p.screen_window[:] = [float(x) for x in screen_window_of(c)]
    p.spp, p.sampler_dims = s.spp, s.dims
    p.max_depth, p.rr_threshold = it.max_depth, it.rr_threshold
    p.light_strategy = 1 if it.light_strategy == "uniform" else 0
    pb = it.pixel_bounds
    p.pixel_bounds[:] = list(pb) if pb is not None else [0, 0, 0, 0]
    p.has_pixel_bounds = 1 if pb is not None else 0
    p.rank, p.world_size, p.flags = rank, world_size, flags
    return p


class HostScene:
    def __init__(self, desc, device_bvh=False, device_ingest=False):
        """device_bvh=True: the tree comes from the GPU's linear builder (rt_bvh_build) instead of the host SAH build.
        device_ingest=True: MIP pyramids and environment-map sampling tables are built on the GPU (bit-identical tables)."""
        L = lib()
        L.rtxh_set_device_ingest(1 if device_ingest else 0)
        try:
            self._build(desc, device_bvh)
        finally:
            L.rtxh_set_device_ingest(0)

    def _build(self, desc, device_bvh):
        L = lib()
        self.desc = desc
        self.h = C.c_void_p(L.rtxh_scene_new())
        P, idx, N, UV, S, mat, light, flags = desc.arrays()
        self._keep = (P, idx, N, UV, S, mat, light, flags)
        if idx.shape[0]:  # (a scene may hold spheres / object instances only)
            _check(L.rtxh_scene_set_mesh(self.h, _p(P), P.shape[0], _p(idx, C.c_int32), idx.shape[0], _p(N), _p(UV), _p(S),
                                         _p(mat, C.c_int32), _p(light, C.c_int32), _p(flags, C.c_uint8)), "set_mesh")
        alpha = desc.alpha_ids() if hasattr(desc, "alpha_ids") else None
        if alpha is not None:
            self._keep += (alpha,)
            _check(L.rtxh_scene_set_alpha(self.h, _p(alpha, C.c_int32)), "set_alpha")
        for m in desc.mipmaps:
            if getattr(m, "path", None) is not None:  # scene_desc.FourierTable: the C++ reader loads the .bsdf file
                _check(L.rtxh_scene_add_fourier_table(self.h, os.fsencode(m.path)), "add_fourier_table")
                continue
            h, w = m.data.shape[:2]
            _check(L.rtxh_scene_add_mipmap(self.h, w, h, _p(m.data), int(m.trilinear), C.c_float(m.max_aniso), m.wrap), "add_mipmap")
        for t in desc.textures:
            if getattr(t, "words", None) is not None:  # TEX_CHECKER_PLANAR / TEX_FBM_MAPPED: the word block becomes an image the texture names
                w = np.ascontiguousarray(t.words, np.float32)
                _check(L.rtxh_scene_add_texture_mapped(self.h, t.kind, _p(np.float32(t.value)), t.tex1, t.tex2, t.amount, _p(w), w.size), "add_texture_mapped")
                continue
            _check(L.rtxh_scene_add_texture(self.h, t.kind, _p(np.float32(t.value)), t.tex1, t.tex2, t.amount, t.mip, _p(np.float32(t.mapping))), "add_texture")
        for m in desc.materials:
            _check(L.rtxh_scene_add_material(self.h, m.kind, _p(m.slots(), C.c_int32), int(m.remap_roughness), int(m.bump)), "add_material")
        for sp in getattr(desc, "spheres", []):
            _check(L.rtxh_scene_add_quadric(self.h, int(getattr(sp, "kind", 0)), _p(sp.o2w), _p(sp.w2o), C.c_float(sp.radius), C.c_float(sp.z_min), C.c_float(sp.z_max),
                                            C.c_float(sp.phi_max), int(sp.reverse_orientation), sp.material, sp.light), "add_quadric")
        for rgb, two_sided in getattr(desc, "emitters", []):
            _check(L.rtxh_scene_add_emitter(self.h, _p(np.float32(rgb)), int(two_sided)), "add_emitter")
        for k, o in enumerate(getattr(desc, "objects", [])):
            self._keep += (o,)
            _check(L.rtxh_scene_add_object(self.h, _p(o.P), o.P.shape[0], _p(o.idx, C.c_int32), o.idx.shape[0], _p(o.N), _p(o.UV), _p(o.S),
                                           _p(o.mat, C.c_int32), _p(o.flags, C.c_uint8)), "add_object")
            if getattr(o, "emit", None) is not None:
                _check(L.rtxh_scene_object_emitters(self.h, k, _p(o.emit, C.c_int32)), "object_emitters")
            for q in getattr(o, "quadrics", None) or []:  # quadrics of the object definition, in object space; light -2 - k: unlisted emitter k
                _check(L.rtxh_object_add_quadric(self.h, k, int(q.kind), _p(q.o2w), _p(q.w2o), C.c_float(q.radius), C.c_float(q.z_min), C.c_float(q.z_max), C.c_float(q.phi_max),
                                                 int(q.reverse_orientation), q.material, (-2 - q.light) if q.light <= -2 else -1), "object_add_quadric")
            if getattr(o, "alpha", None) is not None:
                _check(L.rtxh_object_set_alpha(self.h, k, _p(o.alpha, C.c_int32)), "object_set_alpha")
        for i in getattr(desc, "instances", []):
            _check(L.rtxh_scene_add_instance(self.h, i.obj, _p(i.o2w), _p(i.w2o)), "add_instance")
        for l in desc.lights:
            l2w = None if l.l2w is None else np.ascontiguousarray(l.l2w, np.float32)
            w2l = None if l.w2l is None else np.ascontiguousarray(l.w2l, np.float32)
            tri = l.tri if getattr(l, "sphere", -1) < 0 else -2 - l.sphere  # -2 - k: the area light sits on sphere k
            _check(L.rtxh_scene_add_light(self.h, l.kind, tri, _p(np.float32(l.rgb)), int(l.two_sided), _p(np.float32(l.vec)), l.mip, _p(l2w), _p(w2l)), "add_light")
        self.bvh_build_ms = None
        if device_bvh:
            ms = C.c_float()
            _check(L.rtxh_scene_commit_device_bvh(self.h, desc.max_prims_per_node, C.byref(ms)), "commit_device_bvh")
            self.bvh_build_ms = ms.value
        else:
            _check(L.rtxh_scene_commit(self.h, desc.max_prims_per_node), "commit")

    def __del__(self):
        try:
            lib().rtxh_scene_free(self.h)
        except Exception:
            pass

    # ---- CPU-side products -----------------------------------------------------------------
    def bvh(self):
        L = lib()
        nn, npr = C.c_int32(), C.c_int32()
        L.rtxh_scene_bvh_sizes(self.h, C.byref(nn), C.byref(npr))
        bounds = np.zeros((nn.value, 6), np.float32)
        offset = np.zeros(nn.value, np.uint32)
        nprims = np.zeros(nn.value, np.uint16)
        axis = np.zeros(nn.value, np.uint8)
        ordered = np.zeros(npr.value, np.int32)
        L.rtxh_scene_bvh_get(self.h, _p(bounds), _p(offset, C.c_uint32), _p(nprims, C.c_uint16), _p(axis, C.c_uint8), _p(ordered, C.c_int32))
        return dict(bounds=bounds, offset=offset, n_prims=nprims, axis=axis, ordered=ordered)

    def bvh_sizes(self):
        nn, npr = C.c_int32(), C.c_int32()
        lib().rtxh_scene_bvh_sizes(self.h, C.byref(nn), C.byref(npr))
        return nn.value, npr.value

    def link_tables(self, mid=False):
        """The link tables rt_scene_create gives the stackless LDS walks of this scene (rt_link_tables: host only, no device), as
        dict(kept=[9 rows x n_nodes], full=..., start_kept=[9], start_full=[9], rays=[9], tests_all=[9], tests_kept=[9])."""
        nn = self.bvh_sizes()[0]
        words = 9 * nn + 9
        kept, full, stats = np.zeros(words, np.uint32), np.zeros(words, np.uint32), np.zeros(27, np.float64)
        _check(lib().rtxh_scene_link_tables(self.h, C.c_int32(1 if mid else 0), _p(kept, C.c_uint32), _p(full, C.c_uint32), C.c_uint64(words), _p(stats, C.c_double)), "rtxh_scene_link_tables")

        def split(t):
            rows = np.concatenate([t[:8 * nn].reshape(8, nn), t[8 * nn + 8:9 * nn + 8].reshape(1, nn)])
            return rows, np.concatenate([t[8 * nn:8 * nn + 8], t[9 * nn + 8:9 * nn + 9]])
        (rk, sk), (rf, sf) = split(kept), split(full)
        return dict(kept=rk, full=rf, start_kept=sk, start_full=sf, rays=stats[:9], tests_all=stats[9:18], tests_kept=stats[18:27])

    def shadow_sets(self):
        """The shadow sets rt_scene_create gives an LDS-resident plain-triangle scene of two triangle lights (rt_shadow_sets: host only, no device), as
        dict(nvox=(nx, ny, nz), kind=[nz, ny, nx, 2] (1 = EMPTY: no shadow segment from the voxel to the light can be occluded, 0 = walk), pairs=, empty=)."""
        nv, st = np.zeros(3, np.int32), np.zeros(2, np.uint64)
        _check(lib().rtxh_scene_shadow_sets(self.h, None, C.c_uint64(0), _p(nv, C.c_int32), _p(st, C.c_uint64)), "rtxh_scene_shadow_sets")
        words = np.zeros(2 * int(np.prod(nv)), np.uint32)
        _check(lib().rtxh_scene_shadow_sets(self.h, _p(words, C.c_uint32), C.c_uint64(words.size), _p(nv, C.c_int32), _p(st, C.c_uint64)), "rtxh_scene_shadow_sets")
        return dict(nvox=tuple(int(x) for x in nv), kind=(words & 3).reshape(int(nv[2]), int(nv[1]), int(nv[0]), 2), pairs=int(st[0]), empty=int(st[1]))

    def scene_query(self, what):
        """rt_scene_query of the uploaded scene (RT_QUERY_* of rtx_hip.h)."""
        return _check(lib().rtxh_scene_query(self.h, C.c_int32(what)), "scene_query")

    def lds_resident(self):
        """Does the traversal kernel keep this scene's nodes and primitives in LDS? Asked of the uploaded scene (rt_scene_query: what rt_scene_create decided,
        not re-derived here)."""
        return bool(_check(lib().rtxh_scene_query(self.h, 0), "scene_query"))

    def _render_params(self, **kw):
        return render_params(self.desc, **kw)

    def n_lights(self):
        return len(self.desc.lights)

    def table(self, name):
        return scene_table(self.h, name)

    def setup(self, **kw):
        p = self._render_params(**kw)
        r2c = np.zeros((4, 4), np.float32)
        dxdy = np.zeros(6, np.float32)
        table = np.zeros(256, np.float32)
        sb = np.zeros(4, np.int32)
        cr = np.zeros(4, np.int32)
        _check(lib().rtxh_camera_film_setup(C.byref(p), _p(r2c), _p(dxdy), _p(table), _p(sb, C.c_int32), _p(cr, C.c_int32)), "camera_film_setup")
        return dict(raster_to_camera=r2c, dx_camera=dxdy[:3].copy(), dy_camera=dxdy[3:].copy(), filter_table=table, sample_bounds=sb, cropped=cr, params=p)

    def mip_levels(self, mip):
        L = lib()
        w, h = C.c_int32(), C.c_int32()
        n = _check(L.rtxh_mip_level(self.h, mip, 0, C.byref(w), C.byref(h), None), "mip_level")
        out = []
        for lvl in range(n):
            L.rtxh_mip_level(self.h, mip, lvl, C.byref(w), C.byref(h), None)
            a = np.zeros((h.value, w.value, 3), np.float32)
            L.rtxh_mip_level(self.h, mip, lvl, C.byref(w), C.byref(h), _p(a))
            out.append(a)
        return out

    # ---- GPU ---------------------------------------------------------------------------------
    def upload(self, device=-1):
        _check(lib().rtxh_scene_upload(self.h, device), "upload")

    def render(self, rank=0, world_size=1, count_traversal=False, time_kernels=False, device_out=None, stream=0, count_as_rendered=False, ref_stream=False):
        """renderer::render on the GPU. Returns (film_xyzw (H,W,4) over the cropped bounds, stats dict).
        `device_out`: optional torch CUDA tensor (H,W,4) float32 that receives the film in HBM. `ref_stream`: the reference's own sampler stream - one RNG stream per
        16 x 16 tile, one lane per tile (RT_FLAG_REF_STREAM; slow by construction) - instead of the pixel-keyed one."""
        flags = ((RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0) |
                 (RT_FLAG_COUNT_AS_RENDERED if count_as_rendered else 0) | (RT_FLAG_REF_STREAM if ref_stream else 0))
        st = self.setup(rank=rank, world_size=world_size)
        cr = st["cropped"]
        w, h = int(cr[2] - cr[0]), int(cr[3] - cr[1])
        p = st["params"]
        stats = Stats()
        if device_out is not None:
            assert tuple(device_out.shape) == (h, w, 4) and device_out.is_contiguous()
            p.flags = flags | RT_FLAG_FILM_ON_DEVICE
            _check(lib().rtxh_render(self.h, C.byref(p), C.c_void_p(stream), C.c_void_p(device_out.data_ptr()), C.byref(stats)), "render")
            return device_out, stats.as_dict()
        p.flags = flags
        film = np.zeros((h, w, 4), np.float32)
        _check(lib().rtxh_render(self.h, C.byref(p), C.c_void_p(stream), _p(film), C.byref(stats)), "render")
        return film, stats.as_dict()

    def progressive(self, rank=0, world_size=1, table_budget=None, count_traversal=False, time_kernels=False, pixel_stats=False, features=False):
        """The frame of `render` in steps (rt_frame_*): a ProgressiveFrame whose film can be read after any number of samples per pixel. `table_budget`: bytes the
        frame may spend on sampler tables that stay resident between steps (None: the backend's default; too small: every step rebuilds them - same film).
        `pixel_stats`: the frame keeps per-pixel luminance moments (RT_FLAG_FRAME_STATS) - `pixel_stats()`, `noise()` and `advance_adaptive()` need it.
        `features`: the frame keeps per-pixel sums of its samples' first-hit features (RT_FLAG_FRAME_FEATURES) - `features()` needs it."""
        return ProgressiveFrame(self, rank=rank, world_size=world_size, table_budget=table_budget, count_traversal=count_traversal, time_kernels=time_kernels,
                                pixel_stats=pixel_stats, features=features)

    def progressive_rays(self, width, height, spp=None, max_depth=None, rank=0, world_size=1, table_budget=None, pixel_stats=False, features=False, count_traversal=False,
                         time_kernels=False):
        """A progressive frame over a `width` x `height` film whose steps take their rays and film positions from the caller (rt_frame_begin_rays): a RayFrame. The film
        is `render_rays`' virtual film - pixel (x, y) draws the sampler values of pixel_index y * width + x - with the scene's pixel filter, max_sample_luminance and film
        scale; no camera is set up. `spp` (default: the scene's sampler's) is the frame's sample count, `max_depth` defaults to the scene's integrator's. rank /
        world_size, table_budget, pixel_stats and features as in `progressive`."""
        return RayFrame(self, width, height, spp=spp, max_depth=max_depth, rank=rank, world_size=world_size, table_budget=table_budget, pixel_stats=pixel_stats,
                        features=features, count_traversal=count_traversal, time_kernels=time_kernels)

    def progressive_multi(self, devices, table_budget=None, count_traversal=False, time_kernels=False, pixel_stats=False, features=False):
        """The frame of `progressive` across several GPUs of this process (rt_multi_frame_*): a MultiProgressiveFrame with the methods and properties of
        ProgressiveFrame whose read-outs are the merged frame, formed on devices[0]. One worker per entry of `devices` (an entry may repeat), worker k owns the
        interleaved bands k of len(devices); `table_budget` is per worker. `advance*` return (total stats, [per-device stats])."""
        return MultiProgressiveFrame(self, devices, table_budget=table_budget, count_traversal=count_traversal, time_kernels=time_kernels, pixel_stats=pixel_stats,
                                     features=features)

    def render_multi(self, devices, chunks_per_device=1, count_traversal=False, time_kernels=False, count_as_rendered=False, device_out=None):
        """The frame on several GPUs of this process (rt_multi_render): one host thread per entry of `devices`, chunks of tile rows pulled from a
        shared queue, rows gathered on devices[0]. Returns (film, total stats, [per-device stats]).
        `device_out`: optional torch CUDA tensor (H,W,4) float32 on devices[0] that receives the merged film in HBM."""
        flags = ((RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0) |
                 (RT_FLAG_COUNT_AS_RENDERED if count_as_rendered else 0))
        st = self.setup()
        cr = st["cropped"]
        w, h = int(cr[2] - cr[0]), int(cr[3] - cr[1])
        p = st["params"]
        dev = np.ascontiguousarray(devices, np.int32)
        total, per = Stats(), (Stats * len(dev))()
        if device_out is not None:
            assert tuple(device_out.shape) == (h, w, 4) and device_out.is_contiguous()
            p.flags = flags | RT_FLAG_FILM_ON_DEVICE
            _check(lib().rtxh_render_multi(self.h, C.byref(p), _p(dev, C.c_int32), len(dev), int(chunks_per_device), C.c_void_p(device_out.data_ptr()), C.byref(total), per), "render_multi")
            return device_out, total.as_dict(), [s.as_dict() for s in per]
        p.flags = flags
        film = np.zeros((h, w, 4), np.float32)
        _check(lib().rtxh_render_multi(self.h, C.byref(p), _p(dev, C.c_int32), len(dev), int(chunks_per_device), _p(film), C.byref(total), per), "render_multi")
        return film, total.as_dict(), [s.as_dict() for s in per]

    def fourier_eval(self, material, wo, wi, u):
        """FourierBSDF f / pdf / sample_f of Material "fourier" `material` through the shade kernel's device lobe functions (rt_fourier_eval; shading frame,
        radiance mode). wo, wi: (n, 3), u: (n, 2). Returns dict(f=(n, 3), pdf=(n,), sf=(n, 3), swi=(n, 3), spdf=(n,)). Uploads the scene first if need be."""
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(u, np.float32).reshape(-1, 2)
        n = wo.shape[0]
        assert wi.shape[0] == n and u.shape[0] == n
        dev = C.c_void_p()
        _check(lib().rtxh_scene_device(self.h, C.byref(dev)), "scene_device")
        out = np.zeros((n, 11), np.float32)
        rc = hip_lib().rt_fourier_eval(dev, C.c_int32(material), C.c_uint64(n), _p(wo), _p(wi), _p(u), _p(out))
        if rc != 0:
            raise BackendError(f"rt_fourier_eval failed ({rc}): {hip_lib().rt_last_error().decode(errors='replace')}")
        return dict(f=out[:, 0:3], pdf=out[:, 3], sf=out[:, 4:7], swi=out[:, 7:10], spdf=out[:, 10])

    def texture_eval(self, tex, uv, p=None, duv=None, dpdx=None, dpdy=None):
        """Texture::evaluate of texture `tex` through the device evaluator of the shade kernels (rt_texture_eval), vectorised over records with the argument
        names of OracleScene.tex_probe: uv (n, 2), p (n, 3), duv (n, 4) = dudx dvdx dudy dvdy, dpdx / dpdy (n, 3); omitted ones are zero. Returns (n, 3) float32.
        Uploads the scene first if need be."""
        uv = np.asarray(uv, np.float32).reshape(-1, 2)
        n = uv.shape[0]
        col = lambda v, w: np.zeros((n, w), np.float32) if v is None else np.broadcast_to(np.asarray(v, np.float32).reshape(-1, w), (n, w))
        rec = np.ascontiguousarray(np.concatenate([uv, col(duv, 4), col(p, 3), col(dpdx, 3), col(dpdy, 3)], axis=1), np.float32)
        dev = C.c_void_p()
        _check(lib().rtxh_scene_device(self.h, C.byref(dev)), "scene_device")
        out = np.zeros((n, 3), np.float32)
        if n == 0:
            return out
        rc = hip_lib().rt_texture_eval(dev, C.c_int32(tex), C.c_uint64(n), _p(rec), _p(out))
        if rc != 0:
            raise BackendError(f"rt_texture_eval failed ({rc}): {hip_lib().rt_last_error().decode(errors='replace')}")
        return out

    def bsdf_eval(self, material, wo, wi, u, surface=None, front_end="auto"):
        """The Bsdf material `material` builds at a surface point, evaluated per query by a front-end of the shade kernels (rt_bsdf_eval): wo, wi (n, 3) in WORLD space,
        u (n, 2); surface None = the canonical hit (n = +z, dpdu = +x, dpdv = +y, uv = (0.5, 0.5)) or (n, 40) records (`surface_records`); front_end one of
        "auto", "generic", "lambert", "two_lobe", "two_lobe_wide". Returns dict(f=(n, 3), pdf=(n,), sf=(n, 3), swi=(n, 3), spdf=(n,), stype=(n,) int, n_lobes=(n,) int,
        raw=(n, 13) float32). Uploads the scene first if need be."""
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(u, np.float32).reshape(-1, 2)
        n = wo.shape[0]
        assert wi.shape[0] == n and u.shape[0] == n
        if surface is not None:
            surface = np.ascontiguousarray(surface, np.float32).reshape(-1, RT_BSDF_SURFACE_FLOATS)
            assert surface.shape[0] == n
        dev = C.c_void_p()
        _check(lib().rtxh_scene_device(self.h, C.byref(dev)), "scene_device")
        out = np.zeros((n, RT_BSDF_OUT_FLOATS), np.float32)
        rc = hip_lib().rt_bsdf_eval(dev, C.c_int32(material), C.c_int32(BSDF_FRONT_ENDS[front_end] if isinstance(front_end, str) else int(front_end)), C.c_uint64(n),
                                    _p(surface), _p(wo), _p(wi), _p(u), _p(out))
        if rc != 0:
            raise BackendError(f"rt_bsdf_eval failed ({rc}): {hip_lib().rt_last_error().decode(errors='replace')}")
        return dict(f=out[:, 0:3], pdf=out[:, 3], sf=out[:, 4:7], swi=out[:, 7:10], spdf=out[:, 10], stype=out[:, 11].astype(np.int32), n_lobes=out[:, 12].astype(np.int32), raw=out)

    def light_eval(self, p, n, u, light=None, strategy="spatial", wi=None, visibility=False, p_error=None, general=False):
        """The light half of the shade stage per query (rt_light_eval), run by the shade kernels' own light functions: p (q, 3) reference points, n (q, 3) their
        normals or None (zero: points in free space), u (q, 3) = u_pick, u_light.x, u_light.y, p_error (q, 3) or None (zero). light: an index of the scene's light
        list for every query, or None = picked per query as uniform_sample_one_light does, from the "spatial" or "uniform" distribution (a point whose voxel has no
        table row: light -1, pick pdf 0, zeros elsewhere). wi (q, 3) world space or None: the direction Light::pdf_li and Light::le are asked about.
        visibility: trace the segments of the records with pdf > 0 and a non-black Li by the any-hit launch. general: the GENERAL light functions.
        Returns dict(light=(q,) int, pick_pdf=(q,), li=(q, 3), wi=(q, 3), pdf=(q,), p1=(q, 3), n1=(q, 3), visible=(q,) 1 / 0 / -1 not traced, pdf_li=(q,), le=(q, 3),
        raw=(q, 20) float32). Uploads the scene first if need be."""
        p = np.asarray(p, np.float32).reshape(-1, 3)
        q = p.shape[0]
        col = lambda v: np.zeros((q, 3), np.float32) if v is None else np.broadcast_to(np.asarray(v, np.float32).reshape(-1, 3), (q, 3))
        ref = np.ascontiguousarray(np.concatenate([p, col(n), col(p_error)], axis=1), np.float32)
        u = np.ascontiguousarray(u, np.float32).reshape(-1, 3)
        assert u.shape[0] == q
        if wi is not None:
            wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
            assert wi.shape[0] == q
        dev = C.c_void_p()
        _check(lib().rtxh_scene_device(self.h, C.byref(dev)), "scene_device")
        out = np.zeros((q, RT_LIGHT_OUT_FLOATS), np.float32)
        flags = (RT_LIGHT_EVAL_VISIBILITY if visibility else 0) | (RT_LIGHT_EVAL_GENERAL if general else 0)
        rc = hip_lib().rt_light_eval(dev, C.c_int32(RT_LIGHT_PICK if light is None else int(light)), C.c_int32(LIGHT_STRATEGIES[strategy] if isinstance(strategy, str) else int(strategy)),
                                     C.c_uint64(q), _p(ref), _p(u), _p(wi), C.c_uint32(flags), _p(out))
        if rc != 0:
            raise BackendError(f"rt_light_eval failed ({rc}): {hip_lib().rt_last_error().decode(errors='replace')}")
        return dict(light=out[:, 0].astype(np.int32), pick_pdf=out[:, 1], li=out[:, 2:5], wi=out[:, 5:8], pdf=out[:, 8], p1=out[:, 9:12], n1=out[:, 12:15],
                    visible=out[:, 15].astype(np.int32), pdf_li=out[:, 16], le=out[:, 17:20], raw=out)

    def direct_irradiance(self, points, normals, blocks=64, grid=8, seed=0):
        """Direct irradiance E rgb at arbitrary points with unit normals - no surface, no BSDF, no path (a light probe, a lightmap bake): for every light of the scene
        the estimator Li max(0, n . wi) V / pdf of `light_eval` with visibility. A delta light (point, distant) takes one query per point; any other takes `blocks`
        independent jittered `grid` x `grid` sets of u_light per point, and the standard error comes from the `blocks` block means (float64 on the host).
        Returns (E (P, 3), its standard error (P, 3)) as float64."""
        x = np.asarray(points, np.float64).reshape(-1, 3)
        nrm = np.asarray(normals, np.float64).reshape(-1, 3)
        assert nrm.shape == x.shape and blocks >= 2 and grid >= 1
        P, cells = x.shape[0], grid * grid
        kinds = self.table("lights")["kind"]
        rng = np.random.default_rng(seed)
        e, var = np.zeros((P, 3)), np.zeros((P, 3))
        gx, gy = np.meshgrid(np.arange(grid), np.arange(grid), indexing="ij")

        def estimate(r, n_rep):
            w = np.maximum((np.float64(r["wi"]) * n_rep).sum(-1), 0.0) * (r["visible"] == 1)
            pdf = np.float64(r["pdf"])
            return np.where((pdf > 0)[:, None], np.float64(r["li"]) * (w / np.where(pdf > 0, pdf, 1.0))[:, None], 0.0)
        for k, kind in enumerate(kinds):
            if int(kind) in (1, 2):      # RT_LIGHT_POINT, RT_LIGHT_DISTANT: sample_li does not read u
                e += estimate(self.light_eval(x, nrm, np.zeros((P, 3), np.float32), light=k, visibility=True), nrm)
                continue
            per_call = max(1, (1 << 20) // (blocks * cells))     # points per call: about 2^20 queries
            for p0 in range(0, P, per_call):
                p1 = min(P, p0 + per_call)
                m = p1 - p0
                u = np.zeros((m, blocks, cells, 3), np.float32)
                jit = rng.random((m, blocks, cells, 2))
                u[..., 1] = np.minimum((gx.reshape(-1) + jit[..., 0]) / grid, np.float32(1.0) - np.float32(2.0 ** -24))
                u[..., 2] = np.minimum((gy.reshape(-1) + jit[..., 1]) / grid, np.float32(1.0) - np.float32(2.0 ** -24))
                rep = lambda a: np.repeat(a[p0:p1], blocks * cells, axis=0)
                r = self.light_eval(rep(x), rep(nrm), u.reshape(-1, 3), light=k, visibility=True)
                bm = estimate(r, rep(nrm)).reshape(m, blocks, cells, 3).mean(axis=2)      # block means
                e[p0:p1] += bm.mean(axis=1)
                var[p0:p1] += bm.var(axis=1, ddof=1) / blocks
        return e, np.sqrt(var)

    def samples_window(self):
        """(x0, y0, x1, y1) of the pixels render_samples returns: the integrator's "pixelbounds" inside the film's sample bounds (PathIntegrator::create, path.rs:53-69)."""
        st = self.setup()
        sb, p = [int(v) for v in st["sample_bounds"]], st["params"]
        if p.has_pixel_bounds:  # x0 x1 y0 y1, as the scene file lists them
            pb = list(p.pixel_bounds)
            sb = [max(sb[0], pb[0]), max(sb[1], pb[2]), min(sb[2], pb[1]), min(sb[3], pb[3])]
        return tuple(sb)

    def render_samples(self, count_traversal=False, time_kernels=False, with_p_film=True, stream=0):
        """The frame of `render`, sample by sample (rt_render_samples): returns (radiance (h, w, spp, 4), p_film (h, w, spp, 2) or None, stats dict) over
        `samples_window()`; radiance[..., :3] is L as PathIntegrator::li returned it, radiance[..., 3] is 1 where the renderer scrubs the sample."""
        x0, y0, x1, y1 = self.samples_window()
        w, h = x1 - x0, y1 - y0
        p = self.setup()["params"]
        spp = 1
        while spp < max(int(p.spp), 1):
            spp *= 2
        if w <= 0 or h <= 0 or w * h * spp > RT_SAMPLES_MAX:
            raise BackendError(f"render_samples: a window of {max(w, 0)} x {max(h, 0)} pixels x {spp} samples is empty or holds more than RT_SAMPLES_MAX samples")
        p.flags = (RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0)
        rad = np.zeros((h, w, spp, 4), np.float32)
        pf = np.zeros((h, w, spp, 2), np.float32) if with_p_film else None
        stats = Stats()
        _check(lib().rtxh_render_samples(self.h, C.byref(p), C.c_void_p(stream), _p(rad), _p(pf), C.byref(stats)), "render_samples")
        return rad, pf, stats.as_dict()

    def sample_features(self, device_out=None, stream=0):
        """The first-hit features of every sample of `samples_window()` (rt_render_sample_features): (h, w, spp, 16) float32 - camera ray o.xyz, d.xyz, then the
        closest hit's prim (int bits - `out[..., 6].view(np.int32)` -, -1 = miss), b0, b1, then depth = |p - o|, the shading normal (world space, unit, facing the ray origin, no bump
        map) and the albedo = the camera vertex's throughput factor f |wi.n| / pdf (zero at max_depth 0). A miss: prim -1, everything after the ray zero.
        `device_out`: a contiguous torch CUDA float32 tensor of that shape that receives the records in HBM."""
        x0, y0, x1, y1 = self.samples_window()
        w, h = x1 - x0, y1 - y0
        p = self.setup()["params"]
        spp = 1
        while spp < max(int(p.spp), 1):
            spp *= 2
        if w <= 0 or h <= 0 or w * h * spp > RT_FEATURE_SAMPLES_MAX:
            raise BackendError(f"sample_features: a window of {max(w, 0)} x {max(h, 0)} pixels x {spp} samples is empty or holds more than RT_FEATURE_SAMPLES_MAX samples")
        L = lib()
        L.rtxh_render_sample_features.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if device_out is not None:
            assert tuple(device_out.shape) == (h, w, spp, RT_FEATURE_FLOATS) and device_out.is_contiguous() and device_out.element_size() == 4
            p.flags = RT_FLAG_FILM_ON_DEVICE
            _check(L.rtxh_render_sample_features(self.h, C.byref(p), C.c_void_p(stream), C.c_void_p(device_out.data_ptr())), "sample_features")
            return device_out
        p.flags = 0
        out = np.zeros((h, w, spp, RT_FEATURE_FLOATS), np.float32)
        _check(L.rtxh_render_sample_features(self.h, C.byref(p), C.c_void_p(stream), out.ctypes.data_as(C.c_void_p)), "sample_features")
        return out

    def camera_rays(self, sample0=0, n_samples=None, differentials=False, with_p_film=True, device_out=None, stream=0):
        """The perspective camera's rays as a camera frame generates them (rt_camera_rays): (rays (H, W, ns, 8) float32 - o.xyz, t_max = inf, d.xyz, 0 -, p_film
        (H, W, ns, 2) or None) for samples [sample0, sample0 + ns) of every pixel of the film's sample bounds; `n_samples` defaults to the rest of the (rounded) spp.
        `differentials=True`: records of 20 floats, the ray and then rx_o, ry_o, rx_d, ry_d as the camera frame's bounce 0 uses them (scaled by 1 / sqrt(spp)) - the
        input of `render_rays` / `RayFrame.advance` that reproduces the camera frame on a textured scene. `device_out`: a contiguous torch CUDA float32 tensor of the
        rays' shape, or a pair (rays, p_film) of them; they receive the records in HBM and are returned."""
        st = self.setup()
        p = st["params"]
        sb = [int(v) for v in st["sample_bounds"]]
        w, h = sb[2] - sb[0], sb[3] - sb[1]
        spp = 1
        while spp < max(int(p.spp), 1):
            spp *= 2
        ns = spp - int(sample0) if n_samples is None else int(n_samples)
        rec = RT_RAY_DIFF_FLOATS if differentials else 8
        if w <= 0 or h <= 0 or ns <= 0 or w * h * ns > RT_RAYS_MAX:
            raise BackendError(f"camera_rays: {max(w, 0)} x {max(h, 0)} pixels x {ns} samples are none, or more than RT_RAYS_MAX rays - cut the job by sample range")
        flags = RT_FLAG_RAY_DIFFERENTIALS if differentials else 0
        L = lib()
        L.rtxh_camera_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        if device_out is not None:
            d_rays, d_pf = device_out if isinstance(device_out, (tuple, list)) else (device_out, None)
            for t, shape in ((d_rays, (h, w, ns, rec)),) + (() if d_pf is None else ((d_pf, (h, w, ns, 2)),)):
                if tuple(t.shape) != shape or not t.is_contiguous() or t.element_size() != 4:
                    raise BackendError(f"camera_rays: device_out must be contiguous float32 of shape {shape}")
            _check(L.rtxh_camera_rays(self.h, C.byref(p), int(sample0), ns, flags | RT_FLAG_FILM_ON_DEVICE, C.c_void_p(stream), C.c_void_p(d_rays.data_ptr()),
                                      None if d_pf is None else C.c_void_p(d_pf.data_ptr())), "camera_rays")
            return d_rays, d_pf
        rays = np.zeros((h, w, ns, rec), np.float32)
        pf = np.zeros((h, w, ns, 2), np.float32) if with_p_film else None
        _check(L.rtxh_camera_rays(self.h, C.byref(p), int(sample0), ns, flags, C.c_void_p(stream), rays.ctypes.data_as(C.c_void_p),
                                  None if pf is None else pf.ctypes.data_as(C.c_void_p)), "camera_rays")
        return rays, pf

    def camera_model_params(self, kind):
        """`host.camera_model` filled from this scene's render parameters (rtxh_camera_model), such as a loaded pbrt scene's: camera-to-world, "screenwindow" or
        pbrt's default from the film's aspect ratio, and - orthographic - "lensradius" / "focaldistance"."""
        out = np.zeros(RT_CAMERA_MODEL_FLOATS, np.float32)
        p = self._render_params()
        _check(lib().rtxh_camera_model(C.byref(p), C.c_int32(int(CAMERA_MODELS.get(kind, kind))), _p(out)), "camera_model")
        return out

    def _model_params(self, spp, max_depth, **kw):
        p = self._render_params(**kw)
        if spp is not None:
            p.spp = int(spp)
        if max_depth is not None:
            p.max_depth = int(max_depth)
        return p

    def camera_model_rays(self, kind, camera, sample0=0, n_samples=None, differentials=False, with_p_film=True, device_out=None, stream=0, spp=None):
        """`camera_rays` for a camera model (rt_camera_model_rays): (rays (H, W, ns, 8 | 20) float32, p_film (H, W, ns, 2) or None) of the orthographic or environment
        camera `camera` (`host.camera_model`) over the scene's film resolution, generated on the device from the pixel-keyed sampler: p_film is `camera_rays`' of a
        film with these bounds, and the records are what a model frame (`progressive_model`) traces. `spp` (default: the scene's sampler's) sizes the tables and
        scales the differentials; the other arguments as in `camera_rays`."""
        model, cam = _model_args(kind, camera)
        p = self._model_params(spp, None)
        w, h = int(p.xres), int(p.yres)
        r = 1
        while r < max(int(p.spp), 1):
            r *= 2
        ns = r - int(sample0) if n_samples is None else int(n_samples)
        rec = RT_RAY_DIFF_FLOATS if differentials else 8
        if w <= 0 or h <= 0 or ns <= 0 or w * h * ns > RT_RAYS_MAX:
            raise BackendError(f"camera_model_rays: {max(w, 0)} x {max(h, 0)} pixels x {ns} samples are none, or more than RT_RAYS_MAX rays - cut the job by sample range")
        flags = RT_FLAG_RAY_DIFFERENTIALS if differentials else 0
        L = lib()
        L.rtxh_camera_model_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        pc = cam.ctypes.data_as(C.c_void_p)
        if device_out is not None:
            d_rays, d_pf = device_out if isinstance(device_out, (tuple, list)) else (device_out, None)
            for t, shape in ((d_rays, (h, w, ns, rec)),) + (() if d_pf is None else ((d_pf, (h, w, ns, 2)),)):
                if tuple(t.shape) != shape or not t.is_contiguous() or t.element_size() != 4:
                    raise BackendError(f"camera_model_rays: device_out must be contiguous float32 of shape {shape}")
            _check(L.rtxh_camera_model_rays(self.h, C.byref(p), model, pc, int(sample0), ns, flags | RT_FLAG_FILM_ON_DEVICE, C.c_void_p(stream), C.c_void_p(d_rays.data_ptr()),
                                            None if d_pf is None else C.c_void_p(d_pf.data_ptr())), "camera_model_rays")
            return d_rays, d_pf
        rays = np.zeros((h, w, ns, rec), np.float32)
        pf = np.zeros((h, w, ns, 2), np.float32) if with_p_film else None
        _check(L.rtxh_camera_model_rays(self.h, C.byref(p), model, pc, int(sample0), ns, flags, C.c_void_p(stream), rays.ctypes.data_as(C.c_void_p),
                                        None if pf is None else pf.ctypes.data_as(C.c_void_p)), "camera_model_rays")
        return rays, pf

    def progressive_model(self, kind, camera, spp=None, max_depth=None, differentials=False, rank=0, world_size=1, table_budget=None, pixel_stats=False, features=False,
                          count_traversal=False, time_kernels=False):
        """A progressive frame of the orthographic or environment camera `camera` (`host.camera_model`) whose steps generate their rays on the device
        (rt_frame_begin_model): a ProgressiveFrame - `advance`, `advance_adaptive` and every read-out - over the scene's film resolution with its pixel filter, clamp and
        film scale. No ray, film position or sample crosses the host bus. `differentials=True`: bounce 0 is shaded with the model's ray differentials on a scene that
        reads them. The frame is the ray frame (`progressive_rays`) of `camera_model_rays`' records and positions, byte for byte."""
        return ModelFrame(self, kind, camera, spp=spp, max_depth=max_depth, differentials=differentials, rank=rank, world_size=world_size, table_budget=table_budget,
                          pixel_stats=pixel_stats, features=features, count_traversal=count_traversal, time_kernels=time_kernels)

    def render_model(self, kind, camera, spp=None, max_depth=None, differentials=False, rank=0, world_size=1, device_out=None, stream=0, time_kernels=False):
        """The finished frame of `progressive_model` in one call (rt_render_model): (film_xyzw (H, W, 4) float32, stats dict). `device_out`: a contiguous torch CUDA
        float32 tensor (H, W, 4) that receives the film in HBM and is returned."""
        model, cam = _model_args(kind, camera)
        p = self._model_params(spp, max_depth, rank=rank, world_size=world_size)
        p.flags = (RT_FLAG_RAY_DIFFERENTIALS if differentials else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0)
        w, h = int(p.xres), int(p.yres)
        L = lib()
        L.rtxh_render_model.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        stats = Stats()
        if device_out is not None:
            if tuple(device_out.shape) != (h, w, 4) or not device_out.is_contiguous() or device_out.element_size() != 4:
                raise BackendError(f"render_model: device_out must be contiguous float32 of shape {(h, w, 4)}")
            p.flags |= RT_FLAG_FILM_ON_DEVICE
            _check(L.rtxh_render_model(self.h, C.byref(p), model, cam.ctypes.data_as(C.c_void_p), C.c_void_p(stream), C.c_void_p(device_out.data_ptr()), C.byref(stats)), "render_model")
            return device_out, stats.as_dict()
        film = np.zeros((h, w, 4), np.float32)
        _check(L.rtxh_render_model(self.h, C.byref(p), model, cam.ctypes.data_as(C.c_void_p), C.c_void_p(stream), film.ctypes.data_as(C.c_void_p), C.byref(stats)), "render_model")
        return film, stats.as_dict()

    def render_rays(self, rays, sample0=0, spp=None, max_depth=None, device_out=None, stream=0, count_traversal=False, time_kernels=False):
        """Path-traced radiance along caller-supplied rays (rt_render_rays): `rays` (H, W, ns, 8) float32 - o.xyz, t_max, d.xyz, unused; d is used as given -, returns
        (radiance (H, W, ns, 4), stats dict): L rgb as PathIntegrator::li returns it and a fourth float 0.0 / 1.0 (the renderer would scrub the sample) / 2.0 (t_max not
        > 0: the ray was not traced). Ray (x, y, sl) is sample sample0 + sl of pixel y * W + x of a virtual W x H film: `spp` (default: the scene's sampler's) sizes
        the sampler tables and [sample0, sample0 + ns) must lie inside it - a job of more than RT_RAYS_MAX rays is cut by sample range. `max_depth` defaults to the
        scene's integrator's; rr_threshold, light strategy and sampler dimensions are the scene's. `rays` may be a contiguous torch CUDA float32 tensor: `device_out`
        must then be one of shape (H, W, ns, 4) (RT_FLAG_FILM_ON_DEVICE: both stay in HBM) and is returned.
        A last axis of 20 floats sets RT_FLAG_RAY_DIFFERENTIALS: the record goes on with the ray's differentials rx_o, ry_o, rx_d, ry_d (world space, used as given), which
        enter compute_differential at the first vertex - what `camera_rays(differentials=True)` and `cameras.orthographic / environment(differentials=True)` return.
        All-zero differentials, or a scene whose textures read none, give the 8-float result bit for bit. Any other width is a ValueError."""
        p = self._render_params()
        if spp is not None:
            p.spp = int(spp)
        if max_depth is not None:
            p.max_depth = int(max_depth)
        p.flags = (RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0)
        on_device = hasattr(rays, "data_ptr")
        if not on_device:
            rays = np.ascontiguousarray(rays, np.float32)
        if len(rays.shape) == 4 and rays.shape[3] not in (8, RT_RAY_DIFF_FLOATS):
            raise RayRecordError(f"render_rays: a ray record is 8 floats, or {RT_RAY_DIFF_FLOATS} with differentials, not {int(rays.shape[3])}")
        if len(rays.shape) != 4:
            raise BackendError(f"render_rays: rays must have shape (H, W, ns, 8 | {RT_RAY_DIFF_FLOATS}), not {tuple(rays.shape)}")
        if rays.shape[3] == RT_RAY_DIFF_FLOATS:
            p.flags |= RT_FLAG_RAY_DIFFERENTIALS
        h, w, ns = (int(v) for v in rays.shape[:3])
        if h * w * ns > RT_RAYS_MAX:
            raise BackendError(f"render_rays: {h} x {w} x {ns} rays are more than RT_RAYS_MAX - cut the job by sample range")
        L = lib()
        L.rtxh_render_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        stats = Stats()
        if on_device:
            if device_out is None or tuple(device_out.shape) != (h, w, ns, 4) or not (rays.is_contiguous() and device_out.is_contiguous()) or rays.element_size() != 4 or device_out.element_size() != 4:
                raise BackendError("render_rays: device rays need a contiguous float32 device_out of shape (H, W, ns, 4)")
            p.flags |= RT_FLAG_FILM_ON_DEVICE
            _check(L.rtxh_render_rays(self.h, C.byref(p), C.c_void_p(rays.data_ptr()), w, h, int(sample0), ns, C.c_void_p(stream), C.c_void_p(device_out.data_ptr()), C.byref(stats)), "render_rays")
            return device_out, stats.as_dict()
        if device_out is not None:
            raise BackendError("render_rays: device_out needs device rays (RT_FLAG_FILM_ON_DEVICE names both pointers)")
        rad = np.zeros((h, w, ns, 4), np.float32)
        _check(L.rtxh_render_rays(self.h, C.byref(p), rays.ctypes.data_as(C.c_void_p), w, h, int(sample0), ns, C.c_void_p(stream), rad.ctypes.data_as(C.c_void_p), C.byref(stats)), "render_rays")
        return rad, stats.as_dict()

    def render_rays_ao(self, rays, n_samples, max_distance=float("inf"), sample0=0, spp=None, with_rays=False, device_out=None, stream=0, count_traversal=False,
                       time_kernels=False, device_rays_out=None):
        """The ambient-occlusion and normal integrators along caller-supplied rays (rt_render_rays_ao: AmbientOcclusion::li, Normal::li). `rays` as in `render_rays` -
        (H, W, ns, 8) float32, or 20 floats whose differentials are not read; ray (x, y, sl) is sample sample0 + sl of pixel y * W + x of a virtual W x H film. Each hit
        casts `n_samples` occlusion rays of t_max `max_distance` (inf: the reference) over the hemisphere of its geometric normal. Returns (out (H, W, ns, 4), stats):
        ao = n_clear / n_samples, |dot(d, n)| with d as given, t of the hit, status 0 hit / 1 miss / 2 not traced (t_max not > 0). `with_rays`: returns
        (out, ao_rays (H, W, ns, n_samples, 8), stats) - every occlusion ray as cast, o.xyz, t_max, d.xyz, 1.0 occluded / 0.0 clear; zeros for a miss or a skipped ray.
        `rays` may be a contiguous torch CUDA float32 tensor: `device_out` must then be one of shape (H, W, ns, 4), and with `with_rays` `device_rays_out` one of shape
        (H, W, ns, n_samples, 8) (RT_FLAG_FILM_ON_DEVICE: all stay in HBM); they are returned."""
        p = self._render_params()
        if spp is not None:
            p.spp = int(spp)
        p.flags = (RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0)
        on_device = hasattr(rays, "data_ptr")
        if not on_device:
            rays = np.ascontiguousarray(rays, np.float32)
        if len(rays.shape) != 4 or rays.shape[3] not in (8, RT_RAY_DIFF_FLOATS):
            raise BackendError(f"render_rays_ao: rays must have shape (H, W, ns, 8 | {RT_RAY_DIFF_FLOATS}), not {tuple(rays.shape)}")
        if rays.shape[3] == RT_RAY_DIFF_FLOATS:
            p.flags |= RT_FLAG_RAY_DIFFERENTIALS
        h, w, ns = (int(v) for v in rays.shape[:3])
        n_ao = int(n_samples)
        if h * w * ns > RT_RAYS_MAX or (with_rays and n_ao > 0 and h * w * ns * n_ao > RT_RAYS_MAX):
            raise BackendError(f"render_rays_ao: {h} x {w} x {ns} rays (x {n_ao} occlusion rays handed out) are more than RT_RAYS_MAX - cut the job by sample range")
        L = lib()
        L.rtxh_render_rays_ao.restype = C.c_int
        L.rtxh_render_rays_ao.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
        stats = Stats()
        if on_device:
            ok = device_out is not None and tuple(device_out.shape) == (h, w, ns, RT_AO_FLOATS) and rays.is_contiguous() and device_out.is_contiguous() and rays.element_size() == 4 and device_out.element_size() == 4
            if with_rays:
                ok = ok and device_rays_out is not None and tuple(device_rays_out.shape) == (h, w, ns, n_ao, 8) and device_rays_out.is_contiguous() and device_rays_out.element_size() == 4
            if not ok:
                raise BackendError("render_rays_ao: device rays need a contiguous float32 device_out of shape (H, W, ns, 4), and with_rays a device_rays_out of shape (H, W, ns, n_samples, 8)")
            p.flags |= RT_FLAG_FILM_ON_DEVICE
            _check(L.rtxh_render_rays_ao(self.h, C.byref(p), C.c_void_p(rays.data_ptr()), w, h, int(sample0), ns, n_ao, float(max_distance), C.c_void_p(stream),
                                         C.c_void_p(device_out.data_ptr()), C.c_void_p(device_rays_out.data_ptr()) if with_rays else None, C.byref(stats)), "render_rays_ao")
            return (device_out, device_rays_out, stats.as_dict()) if with_rays else (device_out, stats.as_dict())
        if device_out is not None or device_rays_out is not None:
            raise BackendError("render_rays_ao: device outputs need device rays (RT_FLAG_FILM_ON_DEVICE names every pointer)")
        out = np.zeros((h, w, ns, RT_AO_FLOATS), np.float32)
        ao_rays = np.zeros((h, w, ns, max(n_ao, 0), 8), np.float32) if with_rays else None
        _check(L.rtxh_render_rays_ao(self.h, C.byref(p), rays.ctypes.data_as(C.c_void_p), w, h, int(sample0), ns, n_ao, float(max_distance), C.c_void_p(stream),
                                     out.ctypes.data_as(C.c_void_p), ao_rays.ctypes.data_as(C.c_void_p) if with_rays else None, C.byref(stats)), "render_rays_ao")
        return (out, ao_rays, stats.as_dict()) if with_rays else (out, stats.as_dict())

    def render_ao(self, n_samples, max_distance=float("inf"), rank=0, world_size=1, count_traversal=False, time_kernels=False, device_out=None, stream=0):
        """The frame of `render` with the ambient-occlusion integrator (rt_render_ao): the same camera rays, film positions, pixel filter and shard bands, every sample's
        L = grey(n_clear / n_samples) over `n_samples` occlusion rays of t_max `max_distance`. Returns (film_xyzw (H, W, 4) over the cropped bounds, stats dict).
        `device_out`: optional torch CUDA tensor (H, W, 4) float32 that receives the film in HBM."""
        flags = (RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0)
        st = self.setup(rank=rank, world_size=world_size)
        cr = st["cropped"]
        w, h = int(cr[2] - cr[0]), int(cr[3] - cr[1])
        p = st["params"]
        L = lib()
        L.rtxh_render_ao.restype = C.c_int
        L.rtxh_render_ao.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        stats = Stats()
        if device_out is not None:
            assert tuple(device_out.shape) == (h, w, 4) and device_out.is_contiguous()
            p.flags = flags | RT_FLAG_FILM_ON_DEVICE
            _check(L.rtxh_render_ao(self.h, C.byref(p), int(n_samples), float(max_distance), C.c_void_p(stream), C.c_void_p(device_out.data_ptr()), C.byref(stats)), "render_ao")
            return device_out, stats.as_dict()
        p.flags = flags
        film = np.zeros((h, w, 4), np.float32)
        _check(L.rtxh_render_ao(self.h, C.byref(p), int(n_samples), float(max_distance), C.c_void_p(stream), _p(film), C.byref(stats)), "render_ao")
        return film, stats.as_dict()

    def render_rays_whitted(self, rays, max_depth=5, sample0=0, spp=None, with_info=False, device_out=None, stream=0, count_traversal=False, time_kernels=False,
                            device_info_out=None):
        """The Whitted integrator along caller-supplied rays (rt_render_rays_whitted: Whitted::li). `rays` as in `render_rays` - (H, W, ns, 8) float32, or 20 floats
        whose differentials enter the first vertex; ray (x, y, sl) is sample sample0 + sl of pixel y * W + x of a virtual W x H film. `max_depth` is Whitted::new(n):
        the camera ray is depth 0, 1 never recurses. Returns (L (H, W, ns, 4), info or None, stats): L rgb as li returns it and the status 0 / 1 scrubbed / 2 not traced
        (t_max not > 0); `with_info`: info (H, W, ns, 2) uint32 - the li invocations of the sample (tree nodes, misses included) and the get_2d() draws it consumed after
        the camera sample. `rays` may be a contiguous torch CUDA float32 tensor: `device_out` must then be one of shape (H, W, ns, 4), and with `with_info`
        `device_info_out` an int32 one of shape (H, W, ns, 2) (RT_FLAG_FILM_ON_DEVICE: all stay in HBM); they are returned."""
        p = self._render_params()
        if spp is not None:
            p.spp = int(spp)
        p.flags = (RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0)
        on_device = hasattr(rays, "data_ptr")
        if not on_device:
            rays = np.ascontiguousarray(rays, np.float32)
        if len(rays.shape) != 4 or rays.shape[3] not in (8, RT_RAY_DIFF_FLOATS):
            raise BackendError(f"render_rays_whitted: rays must have shape (H, W, ns, 8 | {RT_RAY_DIFF_FLOATS}), not {tuple(rays.shape)}")
        if rays.shape[3] == RT_RAY_DIFF_FLOATS:
            p.flags |= RT_FLAG_RAY_DIFFERENTIALS
        h, w, ns = (int(v) for v in rays.shape[:3])
        if h * w * ns > RT_RAYS_MAX:
            raise BackendError(f"render_rays_whitted: {h} x {w} x {ns} rays are more than RT_RAYS_MAX - cut the job by sample range")
        L = lib()
        L.rtxh_render_rays_whitted.restype = C.c_int
        L.rtxh_render_rays_whitted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        stats = Stats()
        if on_device:
            ok = device_out is not None and tuple(device_out.shape) == (h, w, ns, 4) and rays.is_contiguous() and device_out.is_contiguous() and rays.element_size() == 4 and device_out.element_size() == 4
            if with_info:
                ok = ok and device_info_out is not None and tuple(device_info_out.shape) == (h, w, ns, RT_WHITTED_INFO_WORDS) and device_info_out.is_contiguous() and device_info_out.element_size() == 4
            if not ok:
                raise BackendError("render_rays_whitted: device rays need a contiguous float32 device_out of shape (H, W, ns, 4), and with_info a 4-byte integer device_info_out of shape (H, W, ns, 2)")
            p.flags |= RT_FLAG_FILM_ON_DEVICE
            _check(L.rtxh_render_rays_whitted(self.h, C.byref(p), C.c_void_p(rays.data_ptr()), w, h, int(sample0), ns, int(max_depth), C.c_void_p(stream),
                                              C.c_void_p(device_out.data_ptr()), C.c_void_p(device_info_out.data_ptr()) if with_info else None, C.byref(stats)), "render_rays_whitted")
            return device_out, (device_info_out if with_info else None), stats.as_dict()
        if device_out is not None or device_info_out is not None:
            raise BackendError("render_rays_whitted: device outputs need device rays (RT_FLAG_FILM_ON_DEVICE names every pointer)")
        rad = np.zeros((h, w, ns, 4), np.float32)
        info = np.zeros((h, w, ns, RT_WHITTED_INFO_WORDS), np.uint32) if with_info else None
        _check(L.rtxh_render_rays_whitted(self.h, C.byref(p), rays.ctypes.data_as(C.c_void_p), w, h, int(sample0), ns, int(max_depth), C.c_void_p(stream),
                                          rad.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p) if with_info else None, C.byref(stats)), "render_rays_whitted")
        return rad, info, stats.as_dict()

    def render_whitted(self, max_depth=5, rank=0, world_size=1, count_traversal=False, time_kernels=False, device_out=None, stream=0):
        """The frame of `render` with the Whitted integrator (rt_render_whitted): the same camera rays, film positions, pixel filter and shard bands, every sample's
        L = Whitted::li(ray, 0) with recursion limit `max_depth`. Returns (film_xyzw (H, W, 4) over the cropped bounds, stats dict).
        `device_out`: optional torch CUDA tensor (H, W, 4) float32 that receives the film in HBM."""
        flags = (RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0)
        st = self.setup(rank=rank, world_size=world_size)
        cr = st["cropped"]
        w, h = int(cr[2] - cr[0]), int(cr[3] - cr[1])
        p = st["params"]
        L = lib()
        L.rtxh_render_whitted.restype = C.c_int
        L.rtxh_render_whitted.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        stats = Stats()
        if device_out is not None:
            assert tuple(device_out.shape) == (h, w, 4) and device_out.is_contiguous()
            p.flags = flags | RT_FLAG_FILM_ON_DEVICE
            _check(L.rtxh_render_whitted(self.h, C.byref(p), int(max_depth), C.c_void_p(stream), C.c_void_p(device_out.data_ptr()), C.byref(stats)), "render_whitted")
            return device_out, stats.as_dict()
        p.flags = flags
        film = np.zeros((h, w, 4), np.float32)
        _check(L.rtxh_render_whitted(self.h, C.byref(p), int(max_depth), C.c_void_p(stream), _p(film), C.byref(stats)), "render_whitted")
        return film, stats.as_dict()

    def _direct_strategy(self, who, strategy):
        if strategy in RT_DIRECT_STRATEGIES:
            return RT_DIRECT_STRATEGIES[strategy]
        if isinstance(strategy, int) and not isinstance(strategy, bool):
            return strategy  # (the library answers for a number outside {0, 1})
        raise BackendError(f"{who}: strategy must be 'all' or 'one', not {strategy!r}")

    def render_rays_direct(self, rays, max_depth=5, strategy="all", sample0=0, spp=None, with_info=False, device_out=None, stream=0, count_traversal=False,
                           time_kernels=False, device_info_out=None):
        """The direct-lighting integrator along caller-supplied rays (rt_render_rays_direct: DirectLightingIntegrator::li). `rays`, `max_depth`, `sample0`, `spp` and the
        device-pointer form as in `render_rays_whitted`; `strategy` "all" (every light at every vertex, from the sampler's arrays) or "one" (one light picked uniformly).
        Returns (L (H, W, ns, 4), info or None, stats): `with_info`: info (H, W, ns, 4) uint32 - li invocations, get_2d() draws and get_1d() draws after the camera
        sample, and the vertices that reached uniform_sample_all_light (above max_depth the sample exhausted its arrays; 0 under "one")."""
        p = self._render_params()
        if spp is not None:
            p.spp = int(spp)
        p.flags = (RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0)
        st = self._direct_strategy("render_rays_direct", strategy)
        on_device = hasattr(rays, "data_ptr")
        if not on_device:
            rays = np.ascontiguousarray(rays, np.float32)
        if len(rays.shape) != 4 or rays.shape[3] not in (8, RT_RAY_DIFF_FLOATS):
            raise BackendError(f"render_rays_direct: rays must have shape (H, W, ns, 8 | {RT_RAY_DIFF_FLOATS}), not {tuple(rays.shape)}")
        if rays.shape[3] == RT_RAY_DIFF_FLOATS:
            p.flags |= RT_FLAG_RAY_DIFFERENTIALS
        h, w, ns = (int(v) for v in rays.shape[:3])
        if h * w * ns > RT_RAYS_MAX:
            raise BackendError(f"render_rays_direct: {h} x {w} x {ns} rays are more than RT_RAYS_MAX - cut the job by sample range")
        L = lib()
        L.rtxh_render_rays_direct.restype = C.c_int
        L.rtxh_render_rays_direct.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        stats = Stats()
        if on_device:
            ok = device_out is not None and tuple(device_out.shape) == (h, w, ns, 4) and rays.is_contiguous() and device_out.is_contiguous() and rays.element_size() == 4 and device_out.element_size() == 4
            if with_info:
                ok = ok and device_info_out is not None and tuple(device_info_out.shape) == (h, w, ns, RT_DIRECT_INFO_WORDS) and device_info_out.is_contiguous() and device_info_out.element_size() == 4
            if not ok:
                raise BackendError("render_rays_direct: device rays need a contiguous float32 device_out of shape (H, W, ns, 4), and with_info a 4-byte integer device_info_out of shape (H, W, ns, 4)")
            p.flags |= RT_FLAG_FILM_ON_DEVICE
            _check(L.rtxh_render_rays_direct(self.h, C.byref(p), C.c_void_p(rays.data_ptr()), w, h, int(sample0), ns, int(max_depth), st, C.c_void_p(stream),
                                             C.c_void_p(device_out.data_ptr()), C.c_void_p(device_info_out.data_ptr()) if with_info else None, C.byref(stats)), "render_rays_direct")
            return device_out, (device_info_out if with_info else None), stats.as_dict()
        if device_out is not None or device_info_out is not None:
            raise BackendError("render_rays_direct: device outputs need device rays (RT_FLAG_FILM_ON_DEVICE names every pointer)")
        rad = np.zeros((h, w, ns, 4), np.float32)
        info = np.zeros((h, w, ns, RT_DIRECT_INFO_WORDS), np.uint32) if with_info else None
        _check(L.rtxh_render_rays_direct(self.h, C.byref(p), rays.ctypes.data_as(C.c_void_p), w, h, int(sample0), ns, int(max_depth), st, C.c_void_p(stream),
                                         rad.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p) if with_info else None, C.byref(stats)), "render_rays_direct")
        return rad, info, stats.as_dict()

    def render_direct(self, max_depth=5, strategy="all", rank=0, world_size=1, count_traversal=False, time_kernels=False, device_out=None, stream=0):
        """The frame of `render` with the direct-lighting integrator (rt_render_direct): the same camera rays, film positions, pixel filter and shard bands, every sample's
        L = DirectLightingIntegrator::li(ray, 0) with recursion limit `max_depth` and light strategy "all" or "one". Returns (film_xyzw (H, W, 4) over the cropped
        bounds, stats dict). `device_out`: optional torch CUDA tensor (H, W, 4) float32 that receives the film in HBM."""
        flags = (RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0)
        strat = self._direct_strategy("render_direct", strategy)
        st = self.setup(rank=rank, world_size=world_size)
        cr = st["cropped"]
        w, h = int(cr[2] - cr[0]), int(cr[3] - cr[1])
        p = st["params"]
        L = lib()
        L.rtxh_render_direct.restype = C.c_int
        L.rtxh_render_direct.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        stats = Stats()
        if device_out is not None:
            assert tuple(device_out.shape) == (h, w, 4) and device_out.is_contiguous()
            p.flags = flags | RT_FLAG_FILM_ON_DEVICE
            _check(L.rtxh_render_direct(self.h, C.byref(p), int(max_depth), strat, C.c_void_p(stream), C.c_void_p(device_out.data_ptr()), C.byref(stats)), "render_direct")
            return device_out, stats.as_dict()
        p.flags = flags
        film = np.zeros((h, w, 4), np.float32)
        _check(L.rtxh_render_direct(self.h, C.byref(p), int(max_depth), strat, C.c_void_p(stream), _p(film), C.byref(stats)), "render_direct")
        return film, stats.as_dict()

    def texture_words(self, tex):
        """The word block of texture `tex` as the host holds it (float32), or an empty array for a texture that names none."""
        L = lib()
        n = _check(L.rtxh_texture_words(self.h, int(tex), None, 0), "texture_words")
        out = np.zeros(n, np.float32)
        if n:
            L.rtxh_texture_words(self.h, int(tex), _p(out), n)
        return out

    def trace(self, rays, any_hit=False, count=True):
        """count=True: the visit-counting kernels (one node per step, the reference's sequence); count=False: the
        kernels rt_render launches (same hit records, no counters)."""
        rays = np.ascontiguousarray(rays, np.float32)
        n = rays.shape[0]
        cnt = np.zeros(2, np.uint64)
        pc = _p(cnt, C.c_uint64) if count else None
        if any_hit:
            occ = np.zeros(n, np.uint32)
            _check(lib().rtxh_trace(self.h, _p(rays), C.c_uint64(n), 1, occ.ctypes.data_as(C.POINTER(C.c_float)), pc), "trace_any")
            return dict(occluded=occ > 0, nodes=int(cnt[0]), tris=int(cnt[1]))
        out = np.zeros((n, 4), np.float32)
        _check(lib().rtxh_trace(self.h, _p(rays), C.c_uint64(n), 0, _p(out), pc), "trace_closest")
        return dict(t=out[:, 0].copy(), prim=out[:, 1].copy().view(np.int32), b0=out[:, 2].copy(), b1=out[:, 3].copy(), nodes=int(cnt[0]), tris=int(cnt[1]))

    def trace_device(self, d_rays_ptr, n, d_hits_ptr, reps=10, stream=0):
        ms = C.c_float()
        _check(lib().rtxh_trace_device(self.h, C.c_void_p(d_rays_ptr), C.c_uint64(n), C.c_void_p(d_hits_ptr), reps, C.c_void_p(stream), C.byref(ms)), "trace_device")
        return ms.value

    def light_distribution(self):
        nv = np.zeros(3, np.int32)
        _check(lib().rtxh_light_distribution(self.h, _p(nv, C.c_int32), None, None, None), "light_distribution")
        total = int(nv[0]) * int(nv[1]) * int(nv[2])
        if total == 0:
            return dict(n_voxels=nv)
        nl = self.n_lights()
        func = np.zeros((total, nl), np.float32)
        cdf = np.zeros((total, nl + 1), np.float32)
        fint = np.zeros(total, np.float32)
        _check(lib().rtxh_light_distribution(self.h, _p(nv, C.c_int32), _p(func), _p(cdf), _p(fint)), "light_distribution")
        return dict(n_voxels=nv, func=func, cdf=cdf, func_int=fint)


class ProgressiveFrame:
    """A frame rendered in steps (HostScene.progressive). `advance(n)` renders the next n samples of every pixel; `film()`, `rgb()` and `display()` read the film as
    it stands. A context manager; it keeps its scene alive and must be closed (or left) before the scene goes."""

    def __init__(self, scene, rank=0, world_size=1, table_budget=None, count_traversal=False, time_kernels=False, pixel_stats=False, features=False):
        L = lib()
        L.rtxh_frame_end.argtypes = [C.c_void_p]
        self.scene = scene   # (the frame's device state belongs to the scene's device: the scene must outlive it)
        self.h = None
        st = scene.setup(rank=rank, world_size=world_size)
        cr = st["cropped"]
        self.width, self.height = int(cr[2] - cr[0]), int(cr[3] - cr[1])
        p = st["params"]
        p.flags = ((RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0) | (RT_FLAG_FRAME_STATS if pixel_stats else 0) |
                   (RT_FLAG_FRAME_FEATURES if features else 0))
        self.scale = float(p.film_scale)
        h = C.c_void_p()
        _check(L.rtxh_frame_begin(scene.h, C.byref(p), C.c_uint64(0 if table_budget is None else max(int(table_budget), 1)), C.byref(h)), "frame_begin")
        self.h = h

    def close(self):
        if self.h is not None:
            lib().rtxh_frame_end(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _query(self, what):
        if self.h is None:
            raise BackendError("the progressive frame is closed")
        v = C.c_uint64()
        _check(lib().rtxh_frame_query(self.h, C.c_int32(what), C.byref(v)), "frame_query")
        return int(v.value)

    samples_done = property(lambda self: self._query(RT_FRAME_SAMPLES_DONE))
    spp = property(lambda self: self._query(RT_FRAME_SPP))
    tables_resident = property(lambda self: bool(self._query(RT_FRAME_TABLES_RESIDENT)))
    state_bytes = property(lambda self: self._query(RT_FRAME_STATE_BYTES))
    samples_taken = property(lambda self: self._query(RT_FRAME_SAMPLES_TAKEN))    # camera samples traced so far, over all steps
    active_pixels = property(lambda self: self._query(RT_FRAME_ACTIVE_PIXELS))    # pixels the last adaptive step sampled (0 before one has run)

    def advance(self, n, stream=0):
        """Renders samples [samples_done, min(samples_done + n, spp)) of every pixel; returns the step's stats dict (all zero once the frame is finished)."""
        if self.h is None:
            raise BackendError("the progressive frame is closed")
        stats = Stats()
        _check(lib().rtxh_frame_advance(self.h, C.c_int32(int(n)), C.c_void_p(stream), C.byref(stats)), "frame_advance")
        return stats.as_dict()

    def advance_adaptive(self, n, threshold, floor_y=0.0, min_samples=4, stream=0):
        """Offers samples [samples_done, min(samples_done + n, spp)) to the pixels that are still noisy (rt_frame_advance_adaptive; the frame needs pixel_stats=True):
        a pixel takes them if it holds fewer than max(min_samples, 2) samples or the standard error of its mean luminance exceeds threshold * max(mean, floor_y).
        Returns the step's stats dict (camera_rays = samples taken; all zero when no pixel is active). The frame is then no longer `render`'s frame."""
        if self.h is None:
            raise BackendError("the progressive frame is closed")
        stats = Stats()
        _check(lib().rtxh_frame_advance_adaptive(self.h, C.c_int32(int(n)), C.c_float(threshold), C.c_float(floor_y), C.c_int32(int(min_samples)), C.c_void_p(stream),
                                                 C.byref(stats)), "frame_advance_adaptive")
        return stats.as_dict()

    def pixel_stats(self, device_out=None, stream=0):
        """(n, sum_y, sum_y2): three (H, W) float64 arrays over the cropped pixel bounds - the number of samples each pixel took and the sums of their luminance and
        its square (RT_FRAME_STATS). With `device_out`, a torch CUDA tensor (H, W, 3) float64, the three are views of it."""
        a = self._read(RT_FRAME_STATS, 1.0, 3, np.float64, device_out, stream)
        return a[..., 0], a[..., 1], a[..., 2]

    def features(self, device_out=None, stream=0):
        """(H, W, 8) float32 over the cropped pixel bounds (RT_FRAME_FEATURES; the frame needs features=True): the means over each pixel's own samples of the first-hit
        albedo rgb and shading normal xyz (not renormalised; misses add zero), the mean depth over the samples that hit, and coverage = hits / samples. Unfiltered;
        zeros where a pixel has taken no sample. With `device_out`, a torch CUDA tensor (H, W, 8) float32, that tensor."""
        return self._read(RT_FRAME_FEATURES, 1.0, 8, np.float32, device_out, stream)

    def noise(self):
        """(mean, se): each pixel's mean luminance and the standard error of that mean, from `pixel_stats()` with the arithmetic of the adaptive criterion
        (var = max(0, sum_y2 - sum_y * mean) / (n - 1), se = sqrt(var / n)); mean is 0 where n = 0, se is inf where n < 2."""
        n, sy, sy2 = self.pixel_stats()
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(n > 0, sy / n, 0.0)
            se = np.where(n > 1, np.sqrt(np.maximum(0.0, sy2 - sy * mean) / (n - 1) / n), np.inf)
        return mean, se

    def _read(self, what, scale, channels, dtype, device_out, stream):
        if self.h is None:
            raise BackendError("the progressive frame is closed")
        shape = (self.height, self.width, channels)
        if device_out is not None:
            assert tuple(device_out.shape) == shape and device_out.is_contiguous() and device_out.element_size() == np.dtype(dtype).itemsize
            _check(lib().rtxh_frame_read(self.h, C.c_int32(what), C.c_float(scale), C.c_uint32(RT_FLAG_FILM_ON_DEVICE), C.c_void_p(stream), C.c_void_p(device_out.data_ptr())), "frame_read")
            return device_out
        out = np.zeros(shape, dtype)
        _check(lib().rtxh_frame_read(self.h, C.c_int32(what), C.c_float(scale), C.c_uint32(0), C.c_void_p(stream), out.ctypes.data_as(C.c_void_p)), "frame_read")
        return out

    def film(self, device_out=None, stream=0):
        """(H, W, 4) float32 (X, Y, Z, filter weight sum) of the samples so far: what `render` returns once the frame is finished."""
        return self._read(RT_FRAME_XYZW, 1.0, 4, np.float32, device_out, stream)

    def rgb(self, scale=None, device_out=None, stream=0):
        """(H, W, 3) float32: Film::write_image's pixels (film_to_rgb of `film()`); `scale` defaults to the film's own."""
        return self._read(RT_FRAME_RGB, self.scale if scale is None else float(scale), 3, np.float32, device_out, stream)

    def sums(self, device_out=None, stream=0):
        """(H, W, 4) float32: the frame's sums as it holds them (RT_FRAME_SUMS) - (sum of w * L) rgb and the filter weight sum, before any colour arithmetic; `film()` is
        these through the float32 RGB -> XYZ matrix. A frame on one device only."""
        return self._read(RT_FRAME_SUMS, 1.0, 4, np.float32, device_out, stream)

    def display(self, scale=None, device_out=None, stream=0):
        """(H, W, 3) uint8: the pixels of `rgb()` through the PNG writer's sRGB quantisation (rgb_to_png8)."""
        return self._read(RT_FRAME_RGB8, self.scale if scale is None else float(scale), 3, np.uint8, device_out, stream)


class RayFrame(ProgressiveFrame):
    """A progressive frame whose steps take their rays and film positions from the caller (HostScene.progressive_rays; rt_frame_begin_rays / rt_frame_advance_rays*):
    the film stage - pixel filter, clamp, read-outs, statistics, features, shards - for rays of any camera. `advance(rays, p_film=None)` renders the next n samples of
    every pixel from `rays` (H, W, n, 8) float32 - or (H, W, n, 20): the ray and its differentials, as in `HostScene.render_rays` (RT_FLAG_RAY_DIFFERENTIALS, per step) -
    and splats each at `p_film` (H, W, n, 2) (None: the pixel centre); a ray whose t_max is not > 0 is skipped. Both may be
    numpy arrays or contiguous torch device tensors (then both of them). Every read-out method and property is ProgressiveFrame's."""

    def __init__(self, scene, width, height, spp=None, max_depth=None, rank=0, world_size=1, table_budget=None, pixel_stats=False, features=False, count_traversal=False,
                 time_kernels=False):
        L = lib()
        L.rtxh_frame_end.argtypes = [C.c_void_p]
        L.rtxh_frame_begin_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]
        L.rtxh_frame_advance_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rtxh_frame_advance_rays_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
        self.scene = scene   # (the frame's device state belongs to the scene's device: the scene must outlive it)
        self.h = None
        self.width, self.height = int(width), int(height)
        p = scene._render_params(rank=rank, world_size=world_size)
        if spp is not None:
            p.spp = int(spp)
        if max_depth is not None:
            p.max_depth = int(max_depth)
        p.flags = ((RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0) | (RT_FLAG_FRAME_STATS if pixel_stats else 0) |
                   (RT_FLAG_FRAME_FEATURES if features else 0))
        self.scale = float(p.film_scale)
        h = C.c_void_p()
        _check(L.rtxh_frame_begin_rays(scene.h, C.byref(p), self.width, self.height, C.c_uint64(0 if table_budget is None else max(int(table_budget), 1)), C.byref(h)),
               "frame_begin_rays")
        self.h = h

    def _step_args(self, rays, p_film):
        """(rays pointer, p_film pointer or None, n, flags, the arrays to keep alive over the call)"""
        if self.h is None:
            raise BackendError("the progressive frame is closed")
        on_device = hasattr(rays, "data_ptr")
        if p_film is not None and hasattr(p_film, "data_ptr") != on_device:
            raise BackendError("ray frame: rays and p_film must both be numpy arrays or both be device tensors (RT_FLAG_FILM_ON_DEVICE names both pointers)")
        if not on_device:
            rays = np.ascontiguousarray(rays, np.float32)
            if p_film is not None:
                p_film = np.ascontiguousarray(p_film, np.float32)
        if len(rays.shape) == 4 and rays.shape[3] not in (8, RT_RAY_DIFF_FLOATS):
            raise RayRecordError(f"ray frame: a ray record is 8 floats, or {RT_RAY_DIFF_FLOATS} with differentials, not {int(rays.shape[3])}")
        if len(rays.shape) != 4 or tuple(rays.shape[:2]) != (self.height, self.width):
            raise BackendError(f"ray frame: rays must have shape ({self.height}, {self.width}, n, 8 | {RT_RAY_DIFF_FLOATS}), not {tuple(rays.shape)}")
        n = int(rays.shape[2])
        diff = RT_FLAG_RAY_DIFFERENTIALS if rays.shape[3] == RT_RAY_DIFF_FLOATS else 0
        if p_film is not None and tuple(p_film.shape) != (self.height, self.width, n, 2):
            raise BackendError(f"ray frame: p_film must have shape ({self.height}, {self.width}, {n}, 2), not {tuple(p_film.shape)}")
        if on_device:
            for t in (rays,) + (() if p_film is None else (p_film,)):
                if not t.is_contiguous() or t.element_size() != 4:
                    raise BackendError("ray frame: device rays and p_film must be contiguous float32 tensors")
            return C.c_void_p(rays.data_ptr()), (None if p_film is None else C.c_void_p(p_film.data_ptr())), n, RT_FLAG_FILM_ON_DEVICE | diff, (rays, p_film)
        return rays.ctypes.data_as(C.c_void_p), (None if p_film is None else p_film.ctypes.data_as(C.c_void_p)), n, diff, (rays, p_film)

    def advance(self, rays, p_film=None, stream=0):
        """Renders samples [samples_done, samples_done + n) of every pixel from `rays` (H, W, n, 8); returns the step's stats dict. n past the frame's spp is refused."""
        pr, pp, n, flags, keep = RayFrame._step_args(self, rays, p_film)
        stats = Stats()
        _check(lib().rtxh_frame_advance_rays(self.h, pr, pp, C.c_int32(n), C.c_uint32(flags), C.c_void_p(stream), C.byref(stats)), "frame_advance_rays")
        del keep
        return stats.as_dict()

    def advance_adaptive(self, rays, p_film, threshold, floor_y=0.0, min_samples=4, stream=0):
        """ProgressiveFrame.advance_adaptive with the caller's rays (the frame needs pixel_stats=True): the rays of a pixel that is not active are passed over like
        skipped rays. Returns the step's stats dict (camera_rays = samples taken)."""
        pr, pp, n, flags, keep = RayFrame._step_args(self, rays, p_film)
        stats = Stats()
        _check(lib().rtxh_frame_advance_rays_adaptive(self.h, pr, pp, C.c_int32(n), C.c_float(threshold), C.c_float(floor_y), C.c_int32(int(min_samples)), C.c_uint32(flags),
                                                      C.c_void_p(stream), C.byref(stats)), "frame_advance_rays_adaptive")
        del keep
        return stats.as_dict()


class ModelFrame(ProgressiveFrame):
    """A progressive frame of a camera model (HostScene.progressive_model; rt_frame_begin_model): ProgressiveFrame's `advance`, `advance_adaptive`, read-outs and
    properties, with the orthographic or environment camera's rays generated on the device from the pixel-keyed sampler at every step."""

    def __init__(self, scene, kind, camera, spp=None, max_depth=None, differentials=False, rank=0, world_size=1, table_budget=None, pixel_stats=False, features=False,
                 count_traversal=False, time_kernels=False):
        L = lib()
        L.rtxh_frame_end.argtypes = [C.c_void_p]
        L.rtxh_frame_begin_model.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p]
        self.scene = scene   # (the frame's device state belongs to the scene's device: the scene must outlive it)
        self.h = None
        model, cam = _model_args(kind, camera)
        p = scene._model_params(spp, max_depth, rank=rank, world_size=world_size)
        self.width, self.height = int(p.xres), int(p.yres)
        p.flags = ((RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0) | (RT_FLAG_FRAME_STATS if pixel_stats else 0) |
                   (RT_FLAG_FRAME_FEATURES if features else 0) | (RT_FLAG_RAY_DIFFERENTIALS if differentials else 0))
        self.scale = float(p.film_scale)
        h = C.c_void_p()
        _check(L.rtxh_frame_begin_model(scene.h, C.byref(p), model, cam.ctypes.data_as(C.c_void_p), C.c_uint64(0 if table_budget is None else max(int(table_budget), 1)),
                                        C.byref(h)), "frame_begin_model")
        self.h = h


class MultiProgressiveFrame(ProgressiveFrame):
    """A frame rendered in steps by several GPUs of this process (HostScene.progressive_multi): ProgressiveFrame's methods and properties over the merged frame.
    `advance` / `advance_adaptive` return (total stats, [per-device stats]); `device_out` tensors live on devices[0]. Calls on one scene's multi frames and
    `render_multi` come from one thread at a time."""

    def __init__(self, scene, devices, table_budget=None, count_traversal=False, time_kernels=False, pixel_stats=False, features=False):
        L = lib()
        L.rtxh_multi_frame_end.argtypes = [C.c_void_p]
        L.rtxh_multi_frame_end.restype = None
        self.scene = scene   # (the replicas the frame lives on belong to the scene: the scene must outlive it)
        self.h = None
        self.devices = [int(d) for d in devices]
        st = scene.setup()
        cr = st["cropped"]
        self.width, self.height = int(cr[2] - cr[0]), int(cr[3] - cr[1])
        p = st["params"]
        p.flags = ((RT_FLAG_COUNT_TRAVERSAL if count_traversal else 0) | (RT_FLAG_TIME_KERNELS if time_kernels else 0) | (RT_FLAG_FRAME_STATS if pixel_stats else 0) |
                   (RT_FLAG_FRAME_FEATURES if features else 0))
        self.scale = float(p.film_scale)
        dev = np.ascontiguousarray(self.devices, np.int32)
        h = C.c_void_p()
        _check(L.rtxh_multi_frame_begin(scene.h, C.byref(p), _p(dev, C.c_int32), len(dev), C.c_uint64(0 if table_budget is None else max(int(table_budget), 1)), C.byref(h)),
               "multi_frame_begin")
        self.h = h

    def close(self):
        if self.h is not None:
            lib().rtxh_multi_frame_end(self.h)
            self.h = None

    def _query(self, what):
        if self.h is None:
            raise BackendError("the progressive frame is closed")
        v = C.c_uint64()
        _check(lib().rtxh_multi_frame_query(self.h, C.c_int32(what), C.byref(v)), "multi_frame_query")
        return int(v.value)

    def advance(self, n):
        """Renders samples [samples_done, min(samples_done + n, spp)) of every pixel, each worker its own; returns (total, [per-device]) stats dicts of the step."""
        if self.h is None:
            raise BackendError("the progressive frame is closed")
        total, per = Stats(), (Stats * len(self.devices))()
        _check(lib().rtxh_multi_frame_advance(self.h, C.c_int32(int(n)), C.byref(total), per), "multi_frame_advance")
        return total.as_dict(), [s.as_dict() for s in per]

    def advance_adaptive(self, n, threshold, floor_y=0.0, min_samples=4):
        """ProgressiveFrame.advance_adaptive on every worker at once (each pixel is decided from its owner's plane); returns (total, [per-device]) stats dicts."""
        if self.h is None:
            raise BackendError("the progressive frame is closed")
        total, per = Stats(), (Stats * len(self.devices))()
        _check(lib().rtxh_multi_frame_advance_adaptive(self.h, C.c_int32(int(n)), C.c_float(threshold), C.c_float(floor_y), C.c_int32(int(min_samples)), C.byref(total), per),
               "multi_frame_advance_adaptive")
        return total.as_dict(), [s.as_dict() for s in per]

    def _read(self, what, scale, channels, dtype, device_out, stream):
        if self.h is None:
            raise BackendError("the progressive frame is closed")
        shape = (self.height, self.width, channels)
        if device_out is not None:
            assert tuple(device_out.shape) == shape and device_out.is_contiguous() and device_out.element_size() == np.dtype(dtype).itemsize
            _check(lib().rtxh_multi_frame_read(self.h, C.c_int32(what), C.c_float(scale), C.c_uint32(RT_FLAG_FILM_ON_DEVICE), C.c_void_p(device_out.data_ptr())), "multi_frame_read")
            return device_out
        out = np.zeros(shape, dtype)
        _check(lib().rtxh_multi_frame_read(self.h, C.c_int32(what), C.c_float(scale), C.c_uint32(0), out.ctypes.data_as(C.c_void_p)), "multi_frame_read")
        return out


def copper():
    """(eta rgb, k rgb): the defaults of Material "metal" (Metal::create, rc/material/metal.rs:25-29)."""
    e, k = (C.c_float * 3)(), (C.c_float * 3)()
    lib().rtxh_copper(e, k)
    return np.float32(list(e)), np.float32(list(k))


def spectrum_from_sampled(wavelengths_nm, values):
    """Spectrum::from_sampled (rc/spectrum.rs:108-126) -> RGB."""
    lam, v = np.ascontiguousarray(wavelengths_nm, np.float32), np.ascontiguousarray(values, np.float32)
    out = (C.c_float * 3)()
    _check(lib().rtxh_spectrum_from_sampled(_p(lam), _p(v), len(lam), out), "spectrum_from_sampled")
    return np.float32(list(out))


def spectrum_blackbody(temperature, scale=1.0):
    """A "blackbody" parameter's value (rc/paramset.rs:291-310) -> RGB."""
    out = (C.c_float * 3)()
    _check(lib().rtxh_spectrum_blackbody(C.c_float(temperature), C.c_float(scale), out), "spectrum_blackbody")
    return np.float32(list(out))


class PbrtResult(C.Structure):
    _fields_ = [("scene", C.c_void_p), ("params", RenderParams), ("max_prims_per_node", C.c_int32), ("n_warnings", C.c_int32),
                ("film_filename", C.c_char * 512)]


_TEXTURE_DT = np.dtype([("kind", "<i4"), ("value", "<f4", 3), ("tex1", "<i4"), ("tex2", "<i4"), ("amount", "<i4"), ("image", "<i4"), ("mapping", "<f4", 4)])
_MATERIAL_DT = np.dtype([("kind", "<i4"), ("slot", "<i4", 16), ("remap_roughness", "<i4"), ("bump", "<i4")])
_LIGHT_DT = np.dtype([("kind", "<i4"), ("tri", "<i4"), ("rgb", "<f4", 3), ("two_sided", "<i4"), ("vec", "<f4", 3), ("mip", "<i4"), ("l2w", "<f4", 12), ("w2l", "<f4", 12)])
_TABLES = {"textures": (0, _TEXTURE_DT), "materials": (1, _MATERIAL_DT), "lights": (2, _LIGHT_DT), "P": (3, np.dtype(("<f4", 3))), "N": (4, np.dtype(("<f4", 3))),
           "UV": (5, np.dtype(("<f4", 2))), "S": (6, np.dtype(("<f4", 3))), "indices": (7, np.dtype(("<i4", 3))), "tri_material": (8, np.dtype("<i4")),
           "tri_light": (9, np.dtype("<i4")), "tri_flags": (10, np.dtype("u1")), "env_func": (11, np.dtype("<f4")), "env_cdf": (12, np.dtype("<f4")),
           "env_row_int": (13, np.dtype("<f4")), "env_marg_cdf": (14, np.dtype("<f4")),
           "instances": (15, np.dtype([("object", "<i4"), ("o2w", "<f4", (4, 4)), ("w2o", "<f4", (4, 4))])),
           "emitters": (16, np.dtype([("rgb", "<f4", (3,)), ("two_sided", "<i4")])),
           "quadrics": (17, np.dtype([("o2w", "<f4", (4, 4)), ("w2o", "<f4", (4, 4)), ("radius", "<f4"), ("z_min", "<f4"), ("z_max", "<f4"), ("theta_min", "<f4"), ("theta_max", "<f4"),
                                      ("phi_max", "<f4"), ("reverse_orientation", "<i4"), ("swaps_handedness", "<i4"), ("kind", "<i4"), ("height", "<f4"), ("inner_radius", "<f4"),
                                      ("material", "<i4"), ("light", "<i4")]))}
_OBJECT_TABLES = {"P": (0, np.dtype(("<f4", 3))), "N": (1, np.dtype(("<f4", 3))), "UV": (2, np.dtype(("<f4", 2))), "S": (3, np.dtype(("<f4", 3))),
                  "indices": (4, np.dtype(("<i4", 3))), "tri_material": (5, np.dtype("<i4")), "tri_flags": (6, np.dtype("u1")), "tri_emitter": (7, np.dtype("<i4"))}


def scene_table(handle, name):
    """Copy of one unflattened table of an rtxh_scene (rtxh_scene_inspect)."""
    if isinstance(name, tuple) and name[1] in ("quadrics", "tri_alpha"):  # what else the object definition holds: RTXH_TABLE_OBJECT_EXTRA_BASE + 2 * object + {0, 1}
        which, dt = 100000 + 2 * int(name[0]) + (0 if name[1] == "quadrics" else 1), (_TABLES["quadrics"][1] if name[1] == "quadrics" else np.dtype(("<i4", 2)))
    elif isinstance(name, tuple):  # (object index, table): the object-space soup of one ObjectBegin block
        j, dt = _OBJECT_TABLES[name[1]]
        which = 1000 + 8 * int(name[0]) + j
    else:
        which, dt = _TABLES[name]
    n = C.c_uint64()
    _check(lib().rtxh_scene_inspect(handle, which, None, C.c_uint64(0), C.byref(n)), "scene_inspect")
    out = np.zeros(n.value, dt)
    if n.value:
        _check(lib().rtxh_scene_inspect(handle, which, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), C.byref(n)), "scene_inspect")
    return out


class PbrtScene(HostScene):
    """A scene read from a pbrt-v3 file by the C++ host (rtxh_pbrt_load): what `rustracer scene.pbrt` builds up to
    `renderer::render` (rc/pbrt/mod.rs:16-27, rc/api.rs:977-1010). Same methods as HostScene."""

    def __init__(self, path=None, text=None, base_dir="", device_ingest=False, flatten_instances=False):
        """flatten_instances=True: every ObjectInstance is written out as world-space triangles (single-level traversal kernels) instead of the
        reference's one tree per object (rc/primitive.rs:79-118), which is the default."""
        L = lib()
        res = PbrtResult()
        L.rtxh_set_device_ingest(1 if device_ingest else 0)  # MIP pyramids / environment tables on the GPU (bit-identical)
        L.rtxh_set_flatten_instances(1 if flatten_instances else 0)
        try:
            if path is not None:
                _check(L.rtxh_pbrt_load(os.fsencode(path), C.byref(res)), "pbrt_load")
            else:
                _check(L.rtxh_pbrt_parse(text.encode(), os.fsencode(base_dir), C.byref(res)), "pbrt_parse")
        finally:
            L.rtxh_set_device_ingest(0)
            L.rtxh_set_flatten_instances(0)
        self.h = C.c_void_p(res.scene)
        self.desc = None
        self.params = RenderParams.from_buffer_copy(res.params)
        self.max_prims_per_node = res.max_prims_per_node
        self.n_warnings = res.n_warnings
        self.first_warning = (L.rtxh_last_error() or b"").decode(errors="replace") if res.n_warnings else ""  # (the loader leaves the first warning's text there)
        self.film_filename = res.film_filename.decode(errors='replace')

    def _render_params(self, rank=0, world_size=1, flags=0):
        p = RenderParams.from_buffer_copy(self.params)
        p.rank, p.world_size, p.flags = rank, world_size, flags
        return p

    def n_lights(self):
        return len(scene_table(self.h, "lights"))


def pbrt_tokens(text: str):
    """The host lexer's token list: [("K", word) | ("N", float) | ("S", string) | ("[", None) | ("]", None)]."""
    buf = C.create_string_buffer(16 * len(text) + 64)
    n = _check(lib().rtxh_pbrt_tokens(text.encode(), buf, C.c_uint64(len(buf))), "pbrt_tokens")
    out = []
    for line in buf.value.decode().split("\n")[:n]:
        if line in ("[", "]"):
            out.append((line, None))
        elif line[0] == "N":
            out.append(("N", float(line[2:])))
        else:
            out.append((line[0], line[2:]))
    return out


def sampler_tables(spp, dims, pixel0, n_pixels, plain=False):
    """K0 on the GPU: (scrambles (n,3*dims) u32, perms (n, 2*dims, spp) u16). plain=True: the single-kernel
    in-order statement of the algorithm (cross-check of the segmented sampler rt_render uses)."""
    spp2 = 1
    while spp2 < spp:
        spp2 *= 2
    sc = np.zeros((n_pixels, 3 * dims), np.uint32)
    pm = np.zeros((n_pixels, 2 * dims, spp2), np.uint16)
    fn = hip_lib().rt_sampler_tables_plain if plain else hip_lib().rt_sampler_tables
    rc = fn(spp, dims, C.c_uint64(pixel0), C.c_uint64(n_pixels), _p(sc, C.c_uint32), _p(pm, C.c_uint16))
    if rc < 0:
        raise BackendError(f"rt_sampler_tables failed ({rc}): {hip_lib().rt_last_error().decode(errors='replace')}")
    return sc, pm


def sampler_replay(partners, kernel=1):
    """The shuffle replay alone on caller-supplied swap partners: `partners` (n_chains, spp) u16 with i <= partners[c, i] < spp, spp a power of two. kernel 0: the
    chain kernel (one lane per chain), 1: the parallel replay (one wave per chain, 64 <= spp <= 1024). Returns the permutations, (n_chains, spp) u16."""
    o = np.ascontiguousarray(partners, np.uint16)
    if o.ndim != 2:
        raise ValueError("sampler_replay: partners must be (n_chains, spp)")
    pm = np.zeros_like(o)
    rc = hip_lib().rt_sampler_replay(C.c_int32(o.shape[1]), C.c_int32(o.shape[0]), _p(o, C.c_uint16), _p(pm, C.c_uint16), C.c_int32(kernel))
    if rc < 0:
        raise BackendError(f"rt_sampler_replay failed ({rc}): {hip_lib().rt_last_error().decode(errors='replace')}")
    return pm


def frame_plan(owned_pixels, spp, dims, pass_log2=29, batch_log2=19, lead_on=None, fixed_cut=None, n_cu=256):
    """rt_frame_plan (host only, no device): the cut of `owned_pixels` pixels x `spp` samples into batches and passes, as
    dict(batch_pixels, lead_pixels, pass_samples, cap, shard_cap, n_slots, multi_batch, batches=[(first pixel, pixels, samples per pass)]).
    lead_on None: the default (on at 1024 spp); fixed_cut: (batch_pixels, lead_pixels) of a frame with resident sampler tables. Raises BackendError
    with the entry point's code in `.code`."""
    fixed = fixed_cut or (0, 0)
    args = [C.c_uint64(owned_pixels), C.c_int32(spp), C.c_int32(dims), C.c_int32(pass_log2), C.c_int32(batch_log2), C.c_int32((spp == 1024) if lead_on is None else bool(lead_on)),
            C.c_uint64(fixed[0]), C.c_uint64(fixed[1]), C.c_int32(n_cu)]
    plan, n = np.zeros(7, np.uint64), C.c_uint64(0)
    rc = hip_lib().rt_frame_plan(*args, _p(plan, C.c_uint64), None, C.c_uint64(0), C.byref(n))
    batches = np.zeros((n.value, 3), np.uint64)
    if rc == 0:
        rc = hip_lib().rt_frame_plan(*args, _p(plan, C.c_uint64), _p(batches, C.c_uint64), C.c_uint64(n.value), C.byref(n))
    if rc < 0:
        err = BackendError(f"rt_frame_plan failed ({rc}): {hip_lib().rt_last_error().decode(errors='replace')}")
        err.code = rc
        raise err
    out = {k: int(v) for k, v in zip(("batch_pixels", "lead_pixels", "pass_samples", "cap", "shard_cap", "n_slots"), plan)}
    out["multi_batch"] = bool(plan[6])
    out["batches"] = [tuple(int(x) for x in b) for b in batches]
    return out


def offset_ray_origin(p, p_error, n, w):
    """offset_ray_origin (rc/geometry/mod.rs:203-220) on the device for (k, 3) float32 arrays: the parity hook of the ulp stepping every spawned ray goes through."""
    a = [np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (p, p_error, n, w)]
    out = np.zeros_like(a[0])
    rc = hip_lib().rt_offset_ray_origin(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), C.c_uint64(a[0].shape[0]), _p(out))
    if rc < 0:
        raise BackendError(f"rt_offset_ray_origin failed ({rc}): {hip_lib().rt_last_error().decode(errors='replace')}")
    return out


def surface_records(n, p=None, n_geom=None, n_shading=None, dpdu=None, dpdv=None, sh_dpdu=None, sh_dpdv=None, uv=None, duv=None, dpdx=None, dpdy=None, flip=None):
    """(n, 40) float32 surface records for HostScene.bsdf_eval in the order rtx_hip.h documents (p, n, shading n, dpdu, dpdv, shading dpdu, shading dpdv, dndu, dndv,
    uv, dudx dvdx dudy dvdy, dpdx, dpdy, flip). Omitted fields take the canonical hit's values; shading fields default to the geometric ones."""
    col = lambda v, w, d: np.broadcast_to(np.asarray(d if v is None else v, np.float32).reshape(-1, w), (n, w))
    ng = col(n_geom, 3, (0, 0, 1))
    du, dv = col(dpdu, 3, (1, 0, 0)), col(dpdv, 3, (0, 1, 0))
    rec = np.concatenate([col(p, 3, (0, 0, 0)), ng, ng if n_shading is None else col(n_shading, 3, None), du, dv, du if sh_dpdu is None else col(sh_dpdu, 3, None),
                          dv if sh_dpdv is None else col(sh_dpdv, 3, None), np.zeros((n, 6), np.float32), col(uv, 2, (0.5, 0.5)), col(duv, 4, (0, 0, 0, 0)),
                          col(dpdx, 3, (0, 0, 0)), col(dpdy, 3, (0, 0, 0)), col(flip, 1, (0,))], axis=1)
    return np.ascontiguousarray(rec, np.float32)


def film_to_rgb(film_xyzw: np.ndarray, scale: float = 1.0) -> np.ndarray:
    """Film::write_image's pixel maths (rc/film.rs:196-234) in float32 numpy: XYZ -> RGB, / weight, clamp, * scale."""
    f = np.asarray(film_xyzw, np.float32)
    X, Y, Z, Wt = f[..., 0], f[..., 1], f[..., 2], f[..., 3]
    c = np.float32
    r = c(3.240479) * X - c(1.537150) * Y - c(0.498535) * Z
    g = c(-0.969256) * X + c(1.875991) * Y + c(0.041556) * Z
    b = c(0.055648) * X - c(0.204043) * Y + c(1.057311) * Z
    rgb = np.stack([r, g, b], -1)
    nz = Wt != 0
    inv = np.where(nz, c(1.0) / np.where(nz, Wt, c(1.0)), c(1.0)).astype(np.float32)
    rgb = np.where(nz[..., None], np.maximum(c(0.0), rgb * inv[..., None]), rgb)
    return (rgb * c(scale)).astype(np.float32)


def rgb_to_png8(rgb: np.ndarray) -> np.ndarray:
    """write_image_png's quantisation (rc/imageio.rs:52-63): clamp(255 * gamma_correct(v) + 0.5, 0, 255) as u8, sRGB curve of
    rc/spectrum.rs:387-393."""
    v = np.asarray(rgb, np.float32)
    c = np.float32
    with np.errstate(invalid="ignore"):
        g = np.where(v <= c(0.0031308), c(12.92) * v, c(1.055) * np.power(np.maximum(v, c(0.0)), c(1.0) / c(2.4), dtype=np.float32) - c(0.055)).astype(np.float32)
    q = np.clip(c(255.0) * g + c(0.5), c(0.0), c(255.0))
    return np.nan_to_num(q, nan=0.0).astype(np.uint8)   # Rust's `as u8` maps NaN to 0
