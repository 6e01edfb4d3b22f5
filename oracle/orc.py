"""ORACLE — TEST INFRASTRUCTURE ONLY. ctypes binding of oracle/_build/liborc.so.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module; the
product path (rustracer_amd/) never does.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_build", "liborc.so")
_lib = None


def build(force: bool = False) -> str:
    if force or not os.path.exists(_LIB_PATH) or any(
            os.path.getmtime(os.path.join(_HERE, f)) > os.path.getmtime(_LIB_PATH)
            for f in os.listdir(_HERE) if f.endswith((".h", ".cpp"))):
        subprocess.check_call(["make", "-C", _HERE, "-s"])
    return _LIB_PATH


class RenderParams(C.Structure):
    _fields_ = [
        ("xres", C.c_int32), ("yres", C.c_int32), ("crop", C.c_float * 4),
        ("filter_kind", C.c_int32), ("filter_params", C.c_float * 4),
        ("film_scale", C.c_float), ("max_sample_luminance", C.c_float),
        ("cam_to_world", C.c_float * 16), ("cam_to_world_inv", C.c_float * 16),
        ("fov", C.c_float), ("lens_radius", C.c_float), ("focal_distance", C.c_float),
        ("spp", C.c_int32), ("sampler_dims", C.c_int32), ("sampler_mode", C.c_int32),
        ("max_depth", C.c_int32), ("rr_threshold", C.c_float), ("light_strategy", C.c_int32),
        ("pixel_bounds", C.c_int32 * 4), ("n_threads", C.c_int32), ("tile_size", C.c_int32),
        ("screen_window", C.c_float * 4), ("has_pixel_bounds", C.c_int32), ("mis_mode", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "camera_rays", "rays_closest", "rays_shadow", "rays_mis", "nodes_closest", "nodes_shadow", "nodes_mis",
        "tris_closest", "tris_shadow", "tris_mis", "pdf_wi_tests", "zero_radiance", "nee_total", "path_len_sum", "scrubbed")] + [
        ("seconds", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_LIB_PATH)
        L = _lib
        L.orc_scene_new.restype = C.c_void_p
        L.orc_scene_object_handle.restype = C.c_void_p
        L.orc_scene_object_handle.argtypes = [C.c_void_p, C.c_int]
        L.orc_scene_free.argtypes = [C.c_void_p]
        for name in ("orc_scene_set_mesh", "orc_scene_add_mipmap", "orc_scene_add_texture", "orc_scene_add_material",
                     "orc_scene_add_light", "orc_scene_add_object", "orc_scene_object_emitter", "orc_scene_object_quadric_emitter", "orc_scene_add_instance", "orc_scene_commit", "orc_scene_bvh_sizes", "orc_scene_bvh_get", "orc_trace",
                     "orc_render", "orc_light_distrib", "orc_li_keyed", "orc_li_keyed_range", "orc_camera_film_setup"):
            getattr(L, name).restype = C.c_int
        L.orc_radical_inverse.restype = C.c_float
        L.orc_radical_inverse.argtypes = [C.c_int, C.c_uint64]
        L.orc_next_float_up.restype = C.c_float
        L.orc_next_float_up.argtypes = [C.c_float]
        L.orc_next_float_down.restype = C.c_float
        L.orc_next_float_down.argtypes = [C.c_float]
        L.orc_gamma.restype = C.c_float
        L.orc_rng_bounded.restype = C.c_uint32
        L.orc_rng_bounded.argtypes = [C.c_int64, C.c_uint32, C.c_int]
    return _lib


def _p(a, t=C.c_float):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def screen_window_of(camera, film):
    """PerspectiveCamera::create (camera.rs:86-107): explicit "screenwindow", else from "frameaspectratio", else (0, 0, 0, 0) = the default."""
    if getattr(camera, "screen_window", None) is not None:
        return tuple(camera.screen_window)
    fr = getattr(camera, "frame_aspect", None)
    if fr is None:
        return (0.0, 0.0, 0.0, 0.0)
    fr = np.float32(fr)
    return (-fr, fr, -1.0, 1.0) if fr > 1.0 else (-1.0, 1.0, np.float32(-1.0) / fr, np.float32(1.0) / fr)


def look_at(pos, look, up):
    m = np.zeros((4, 4), np.float32)
    mi = np.zeros((4, 4), np.float32)
    lib().orc_look_at(_p(np.float32(pos)), _p(np.float32(look)), _p(np.float32(up)), _p(m), _p(mi))
    return m, mi


def render_params(desc, mode: int, n_threads: int = 0) -> RenderParams:
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
    p.screen_window[:] = [float(x) for x in screen_window_of(c, f)]
    p.spp, p.sampler_dims, p.sampler_mode = s.spp, s.dims, mode
    p.max_depth, p.rr_threshold = it.max_depth, it.rr_threshold
    p.light_strategy = 1 if it.light_strategy == "uniform" else 0
    pb = it.pixel_bounds
    p.pixel_bounds[:] = list(pb) if pb is not None else [0, 0, 0, 0]
    p.has_pixel_bounds = 1 if pb is not None else 0
    p.n_threads = n_threads
    p.tile_size = 16
    return p


class OracleScene:
    """Oracle-side scene: builds its own SAH BVH from the unflattened description."""

    def __init__(self, desc):
        L = lib()
        self.desc = desc
        self.h = C.c_void_p(L.orc_scene_new())
        P, idx, N, UV, S, mat, light, flags = desc.arrays()
        self._keep = (P, idx, N, UV, S, mat, light, flags)
        rc = 0 if idx.shape[0] == 0 else L.orc_scene_set_mesh(self.h, _p(P), P.shape[0], _p(idx, C.c_int32), idx.shape[0], _p(N), _p(UV), _p(S),
                                                             _p(mat, C.c_int32), _p(light, C.c_int32), _p(flags, C.c_uint8))
        assert rc == 0
        alpha = desc.alpha_ids() if hasattr(desc, "alpha_ids") else None
        if alpha is not None:
            self._keep += (alpha,)
            assert L.orc_scene_set_alpha(self.h, _p(alpha, C.c_int32)) == 0
        for m in desc.mipmaps:
            h, w = m.data.shape[:2]
            assert L.orc_scene_add_mipmap(self.h, w, h, _p(m.data), int(m.trilinear), C.c_float(m.max_aniso), m.wrap) >= 0
        for t in desc.textures:
            v = np.float32(t.value)
            mp = np.float32(t.mapping)
            L.orc_scene_add_texture(self.h, t.kind, _p(v), t.tex1, t.tex2, t.amount, t.mip, _p(mp))
        for m in desc.materials:
            sl = m.slots()
            L.orc_scene_add_material(self.h, m.kind, _p(sl, C.c_int32), int(m.remap_roughness), int(m.bump))
        for sp in getattr(desc, "spheres", []):
            L.orc_scene_add_sphere(self.h, _p(sp.o2w), _p(sp.w2o), C.c_float(sp.radius), C.c_float(sp.z_min), C.c_float(sp.z_max), C.c_float(sp.phi_max),
                                   int(sp.reverse_orientation), sp.material, sp.light, int(getattr(sp, "kind", 0)))
        for k, o in enumerate(getattr(desc, "objects", [])):
            self._keep += (o,)
            assert L.orc_scene_add_object(self.h, _p(o.P), o.P.shape[0], _p(o.idx, C.c_int32), o.idx.shape[0], _p(o.N), _p(o.UV), _p(o.S),
                                          _p(o.mat, C.c_int32), _p(o.flags, C.c_uint8)) >= 0
            if getattr(o, "emit", None) is not None:  # emitting meshes inside the object: area lights that are in no light list (api.rs:954-964)
                for t in range(o.emit.shape[0]):
                    if o.emit[t] >= 0:
                        rgb, two_sided = desc.emitters[int(o.emit[t])]
                        assert L.orc_scene_object_emitter(self.h, k, t, _p(np.float32(rgb)), int(two_sided)) >= 0
            oh = None
            for q in getattr(o, "quadrics", None) or []:  # quadrics of the object definition (object space), emitters among them in no light list
                oh = oh or C.c_void_p(L.orc_scene_object_handle(self.h, k))
                light = -1
                if q.light <= -2:
                    rgb, two_sided = desc.emitters[-2 - q.light]
                    light = L.orc_scene_object_quadric_emitter(self.h, k, _p(np.float32(rgb)), int(two_sided))
                    assert light >= 0
                assert L.orc_scene_add_sphere(oh, _p(q.o2w), _p(q.w2o), C.c_float(q.radius), C.c_float(q.z_min), C.c_float(q.z_max), C.c_float(q.phi_max),
                                              int(q.reverse_orientation), q.material, light, int(q.kind)) >= 0
            if getattr(o, "alpha", None) is not None:
                oh = oh or C.c_void_p(L.orc_scene_object_handle(self.h, k))
                assert L.orc_scene_set_alpha(oh, _p(o.alpha, C.c_int32)) == 0
        for i in getattr(desc, "instances", []):
            assert L.orc_scene_add_instance(self.h, i.obj, _p(i.o2w), _p(i.w2o)) >= 0
        for l in desc.lights:
            rgb = np.float32(l.rgb)
            vec = np.float32(l.vec)
            l2w = None if l.l2w is None else np.ascontiguousarray(l.l2w, np.float32)
            w2l = None if l.w2l is None else np.ascontiguousarray(l.w2l, np.float32)
            tri = l.tri if getattr(l, "sphere", -1) < 0 else -2 - l.sphere  # -2 - k: the area light sits on sphere k
            assert L.orc_scene_add_light(self.h, l.kind, tri, _p(rgb), int(l.two_sided), _p(vec), l.mip, _p(l2w), _p(w2l)) >= 0
        L.orc_scene_commit(self.h, desc.max_prims_per_node)

    def __del__(self):
        try:
            lib().orc_scene_free(self.h)
        except Exception:
            pass

    def bvh(self):
        L = lib()
        nn, npr = C.c_int(), C.c_int()
        L.orc_scene_bvh_sizes(self.h, C.byref(nn), C.byref(npr))
        bounds = np.zeros((nn.value, 6), np.float32)
        offset = np.zeros(nn.value, np.uint32)
        nprims = np.zeros(nn.value, np.uint16)
        axis = np.zeros(nn.value, np.uint8)
        ordered = np.zeros(npr.value, np.int32)
        L.orc_scene_bvh_get(self.h, _p(bounds), _p(offset, C.c_uint32), _p(nprims, C.c_uint16), _p(axis, C.c_uint8), _p(ordered, C.c_int32))
        return dict(bounds=bounds, offset=offset, n_prims=nprims, axis=axis, ordered=ordered)

    def tex_probe(self, tex, uv=(0.0, 0.0), p=(0.0, 0.0, 0.0), duv=(0.0, 0.0, 0.0, 0.0), dpdx=(0.0, 0.0, 0.0), dpdy=(0.0, 0.0, 0.0)):
        out = np.zeros(3, np.float32)
        f = lambda v: _p(np.asarray(v, np.float32))
        lib().orc_tex_probe(self.h, int(tex), f(uv), f(p), f(duv), f(dpdx), f(dpdy), _p(out))
        return out

    def bsdf_probe_surface(self, material, surface, wo, wi, u):
        """orc_bsdf_probe_surface query by query: surface (n, 40) records in rt_bsdf_eval's order or None (the canonical hit), wo, wi (n, 3) world space, u (n, 2).
        Returns (n, 13) float32 in rt_bsdf_eval's output order: f rgb, pdf, sampled f rgb, wi xyz, pdf, type flags, lobe count."""
        wo, wi, u = (np.ascontiguousarray(a, np.float32) for a in (wo, wi, u))
        n = wo.shape[0]
        if surface is not None:
            surface = np.ascontiguousarray(surface, np.float32).reshape(n, 40)
        out = np.zeros((n, 13), np.float32)
        f, smp, pdf = np.zeros(3, np.float32), np.zeros(8, np.float32), C.c_float()
        probe = lib().orc_bsdf_probe_surface
        for i in range(n):
            nl = probe(self.h, int(material), None if surface is None else _p(surface[i]), _p(wo[i]), _p(wi[i]), _p(u[i]), _p(f), C.byref(pdf), _p(smp))
            out[i, 0:3], out[i, 3], out[i, 4:12], out[i, 12] = f, pdf.value, smp, nl
        return out

    def mip_levels(self, mip):
        L = lib()
        w, h = C.c_int32(), C.c_int32()
        n = L.orc_mip_level(self.h, mip, 0, C.byref(w), C.byref(h), None)
        assert n > 0
        out = []
        for lvl in range(n):
            L.orc_mip_level(self.h, mip, lvl, C.byref(w), C.byref(h), None)
            a = np.zeros((h.value, w.value, 3), np.float32)
            L.orc_mip_level(self.h, mip, lvl, C.byref(w), C.byref(h), _p(a))
            out.append(a)
        return out

    def trace(self, rays: np.ndarray, any_hit: bool = False):
        """rays (n,8) f32: o.xyz, tmax, d.xyz, pad -> dict(t, prim, b0, b1 | occluded), counters"""
        rays = np.ascontiguousarray(rays, np.float32)
        n = rays.shape[0]
        out = np.zeros((n, 4), np.float32)
        cnt = np.zeros(2, np.uint64)
        lib().orc_trace(self.h, _p(rays), C.c_int64(n), int(any_hit), _p(out), _p(cnt, C.c_uint64))
        if any_hit:
            return dict(occluded=out[:, 0] > 0.5, nodes=int(cnt[0]), tris=int(cnt[1]))
        return dict(t=out[:, 0].copy(), prim=out[:, 1].copy().view(np.int32), b0=out[:, 2].copy(), b1=out[:, 3].copy(),
                    nodes=int(cnt[0]), tris=int(cnt[1]))

    def setup(self, mode=1):
        p = render_params(self.desc, mode)
        r2c = np.zeros((4, 4), np.float32)
        dxdy = np.zeros(6, np.float32)
        table = np.zeros(256, np.float32)
        sb = np.zeros(4, np.int32)
        cr = np.zeros(4, np.int32)
        lib().orc_camera_film_setup(C.byref(p), _p(r2c), _p(dxdy), _p(table), _p(sb, C.c_int32), _p(cr, C.c_int32))
        return dict(raster_to_camera=r2c, dx_camera=dxdy[:3].copy(), dy_camera=dxdy[3:].copy(), filter_table=table,
                    sample_bounds=sb, cropped=cr, params=p)

    def render(self, mode: int = 1, n_threads: int = 0, mis_mode: int = 0):
        """Returns (film_xyzw (H,W,4) over the cropped pixel bounds, stats dict). mis_mode != 0: test hook (light sampling alone / BSDF sampling
        alone in estimate_direct), see PathIntegrator::mis_mode in orc_render.h."""
        st = self.setup(mode)
        p = st["params"]
        p.n_threads = n_threads
        p.mis_mode = mis_mode
        cr = st["cropped"]
        w, h = int(cr[2] - cr[0]), int(cr[3] - cr[1])
        film = np.zeros((h, w, 4), np.float32)
        stats = Stats()
        rc = lib().orc_render(self.h, C.byref(p), _p(film), C.byref(stats))
        assert rc == 0
        return film, stats.as_dict()

    def li_keyed(self, px, py, sample, n=None, mis_mode=0):
        """PathIntegrator::li of sample `sample` of pixel (px, py) in KEYED mode, (3,); with `n`: of the samples [sample, sample + n), (n, 3). mis_mode: the test
        hook of `render` (1: light sampling alone, 2: BSDF sampling alone in estimate_direct)."""
        p = render_params(self.desc, 1)
        p.mis_mode = int(mis_mode)
        if n is None:
            out = np.zeros(3, np.float32)
            lib().orc_li_keyed(self.h, C.byref(p), px, py, sample, _p(out))
            return out
        out = np.zeros((int(n), 3), np.float32)
        lib().orc_li_keyed_range(self.h, C.byref(p), int(px), int(py), int(sample), int(n), _p(out))
        return out

    def light_distrib(self, max_voxels=None):
        L = lib()
        nv = np.zeros(3, np.int32)
        strategy = 1 if self.desc.integrator.light_strategy == "uniform" else 0
        L.orc_light_distrib(self.h, strategy, _p(nv, C.c_int32), None, None, None, C.c_int64(0))
        total = int(nv[0]) * int(nv[1]) * int(nv[2])
        if total == 0:
            return dict(n_voxels=nv)
        lim = total if max_voxels is None else min(total, max_voxels)
        nl = len(self.desc.lights)
        func = np.zeros((lim, nl), np.float32)
        cdf = np.zeros((lim, nl + 1), np.float32)
        fint = np.zeros(lim, np.float32)
        L.orc_light_distrib(self.h, strategy, _p(nv, C.c_int32), _p(func), _p(cdf), _p(fint), C.c_int64(lim))
        return dict(n_voxels=nv, func=func, cdf=cdf, func_int=fint)


def film_to_rgb(film_xyzw: np.ndarray, scale: float = 1.0) -> np.ndarray:
    f = np.ascontiguousarray(film_xyzw, np.float32)
    out = np.zeros(f.shape[:-1] + (3,), np.float32)
    lib().orc_film_to_rgb(_p(f), C.c_int64(f.size // 4), C.c_float(scale), _p(out))
    return out


def sampler_tables(spp, dims, mode, seed):
    spp2 = 1
    while spp2 < spp:
        spp2 *= 2
    o1 = np.zeros((dims, spp2), np.float32)
    o2 = np.zeros((dims, spp2, 2), np.float32)
    st = np.zeros(2, np.uint64)
    lib().orc_sampler_tables(spp, dims, mode, C.c_uint64(seed), _p(o1), _p(o2), _p(st, C.c_uint64))
    return o1, o2, st


def sampler_retry_scan(spp, dims, pixel0, n, cap=64):
    """Keyed pixel indices in [pixel0, pixel0+n) whose start_pixel stream contains a bounded-draw retry."""
    out = np.zeros(cap, np.uint64)
    k = lib().orc_sampler_retry_scan(spp, dims, C.c_uint64(pixel0), C.c_uint64(n), _p(out, C.c_uint64), cap)
    return out[:k].copy()


def translate_apply(delta, v, is_vector=False):
    out = np.zeros(3, np.float32)
    lib().orc_translate_apply(_p(np.asarray(delta, np.float32)), _p(np.asarray(v, np.float32)), int(is_vector), _p(out))
    return out


def noise(x, y, z):
    L = lib()
    L.orc_noise.restype = C.c_float
    return float(L.orc_noise(C.c_float(x), C.c_float(y), C.c_float(z)))


def round_up_pow2(v):
    return int(lib().orc_round_up_pow2(int(v)))


def rng_stream(seq, n):
    u = np.zeros(n, np.uint32)
    f = np.zeros(n, np.float32)
    lib().orc_rng_stream(C.c_int64(seq), n, _p(u, C.c_uint32), _p(f))
    return u, f
