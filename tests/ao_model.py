"""A numpy model of the ambient-occlusion and normal integrators, written from the reference's integrator/ao.rs, integrator/normal.rs, sampling/mod.rs:14-20
(uniform_sample_sphere) and interaction.rs:56-60 (spawn_ray) - not from the device code.

  li(scene, ray, sampler):  hit = scene.intersect(ray); n = hit.n  (the GEOMETRIC normal)
      for k in 0 .. n_samples:  s = sampler.get_2d(); w = uniform_sample_sphere(s); if dot(w, n) < 0: w = -w
                                if not scene.intersect_p(hit.spawn_ray(w)): n_clear += 1
      return grey(float32(n_clear) / float32(n_samples))                         Normal::li: grey(|dot(ray.d, hit.n)|)

The sampler values come from the oracle's restatement of ZeroTwoSequence (oracle.orc.sampler_tables, keyed by pixel index) and of the PCG32 stream (orc.rng_stream);
uniform_sample_sphere is evaluated in float32, operation by operation; the geometry of a hit - p and n - in float64, by a brute-force closest hit over the scene's
world-space triangles and spheres, so that no numbering of primitives is shared with the code under test."""
import numpy as np

F = np.float32


def sample_u(orc, spp, dims, pixel_index, s, n):
    """The first n get_2d() values after get_camera_sample (cur_2d = 2) of sample s of the pixel keyed pixel_index: (n, 2) float32. While 2 + k < dims the table value
    2D#(2 + k) at index s; after that two draws of the stream pixel_index * spp + s + 2^32, returned as (second draw, first draw) (zerotwosequence.rs:168-180)."""
    spp_r = 1
    while spp_r < spp:
        spp_r *= 2
    _, t2, _ = orc.sampler_tables(spp_r, dims, 1, pixel_index)
    n_rng = max(0, n - max(0, dims - 2))
    _, f = orc.rng_stream(pixel_index * spp_r + s + (1 << 32), max(2 * n_rng, 1))
    u = np.zeros((n, 2), F)
    for k in range(n):
        if 2 + k < dims:
            u[k] = t2[2 + k, s]
        else:
            j = k - max(0, dims - 2)
            u[k] = (f[2 * j + 1], f[2 * j])
    return u


def uniform_sample_sphere(u):
    """sampling/mod.rs:14-20 in float32: (n, 2) -> (n, 3)."""
    u = np.asarray(u, F).reshape(-1, 2)
    z = F(1.0) - F(2.0) * u[:, 0]
    r = np.sqrt(np.maximum(F(1.0) - z * z, F(0.0))).astype(F)
    phi = (F(2.0) * F(np.pi)) * u[:, 1]
    return np.stack([r * np.cos(phi).astype(F), r * np.sin(phi).astype(F), z], axis=1).astype(F)


def ao_directions(u, n):
    """w of ao.rs:43-47 for the samples u (k, 2) at a hit of geometric normal n (3,) float64: (w (k, 3) float32, dot(w, n) (k,) float64 before the flip)."""
    w = uniform_sample_sphere(u)
    dn = w.astype(np.float64) @ np.asarray(n, np.float64)
    w = np.where(dn[:, None] < 0.0, -w, w)
    return w, dn


def ao_value(occluded):
    """float32(n_clear) / float32(n_samples) over the last axis of a boolean array (ao.rs:54)."""
    occluded = np.asarray(occluded, bool)
    return (F(1.0) * (~occluded).sum(axis=-1).astype(F)) / F(occluded.shape[-1])


EPS = 2.0 ** -24


def gamma(n):
    """rc/lib.rs:90-92"""
    return n * EPS / (1 - n * EPS)


def _xf_error(m, p_obj, perr_obj):
    """Transform::transform_point_with_error's bound (transform.rs:190-219) for the 4 x 4 matrix m, in float64: (n, 3) -> (n, 3)."""
    a = np.abs(m[:3, :3])
    return (gamma(3) + 1.0) * (perr_obj @ a.T) + gamma(3) * (np.abs(p_obj) @ a.T + np.abs(m[:3, 3]))


class Geometry:
    """World-space triangles and full spheres of a SceneDesc, in float64: top-level meshes (with their reverse-orientation flag and per-vertex normals), spheres under a
    translation, and the triangles of instanced objects under their instance's object-to-world matrix (kept with their object-space vertices: the reference bounds
    p_error there)."""

    def __init__(self, desc):
        P, idx, N, _, _, _, _, flags = desc.arrays()
        self.prims = []  # (world triangle (3, 3), object-space triangle, matrix or None, flipped, passed over by scene.intersect, vertex normals (3, 3) or None)
        alpha = desc.alpha_ids()
        for k in range(idx.shape[0]):
            tri = P[idx[k]].astype(np.float64)
            vn = N[idx[k]].astype(np.float64) if (N is not None and flags[k] & 2) else None
            self.prims.append((tri, tri, None, bool(flags[k] & 1), bool(alpha is not None and alpha[k, 0] >= 0), vn))  # (the tests' only alpha texture is the constant 0)
        for inst in getattr(desc, "instances", []):
            o = desc.objects[inst.obj]
            m = inst.o2w.astype(np.float64)
            Po = np.asarray(o.P, np.float64)
            Pw = Po @ m[:3, :3].T + m[:3, 3]
            for k in range(o.idx.shape[0]):
                assert not (np.asarray(o.flags)[k] & 2), "the model's instanced objects carry no vertex normals"
                self.prims.append((Pw[o.idx[k]], Po[o.idx[k]], m, bool(np.asarray(o.flags)[k] & 1), False, None))
        self.spheres = [(sp.o2w.astype(np.float64), float(sp.radius), bool(sp.reverse_orientation)) for sp in getattr(desc, "spheres", [])]
        for m, _, _ in self.spheres:
            assert np.array_equal(m[:3, :3], np.eye(3)), "the model's spheres sit under a translation"

    @staticmethod
    def _tri_normal(tri, fl, vn, b):
        """hit.n of Triangle::intersect (mesh.rs:385, 417-425) for barycentrics b (n, 3): normalize(cross(p0 - p2, p1 - p2)); on a mesh with vertex normals turned to the
        side of the interpolated one (face_forward), else negated under reverse orientation."""
        n = np.cross(tri[0] - tri[2], tri[1] - tri[2])
        n = np.broadcast_to(n / np.linalg.norm(n), b.shape).copy()
        if vn is not None:
            ns = b @ vn
            n[(n * ns).sum(1) < 0] *= -1.0
        elif fl:
            n = -n
        return n

    def closest(self, o, d):
        """Brute-force closest hit of rays o, d (n, 3) in float64: (t (n,), p (n, 3), n (n, 3)); t = inf on a miss. Used to check `from_hit_records` without a device."""
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        nr = o.shape[0]
        best_t = np.full(nr, np.inf)
        best_n = np.zeros((nr, 3))
        for tri, _, _, fl, sk, vn in self.prims:
            if sk:
                continue
            p0, p1, p2 = tri
            e1, e2 = p1 - p0, p2 - p0
            pv = np.cross(d, e2)
            det = pv @ e1
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / det
                tv = o - p0
                b1 = (tv * pv).sum(1) * inv
                qv = np.cross(tv, e1)
                b2 = (d * qv).sum(1) * inv
                t = (qv @ e2) * inv
            ok = (np.abs(det) > 0) & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1) & (t > 0) & (t < best_t)
            if not ok.any():
                continue
            b = np.where(ok[:, None], np.stack([1.0 - b1 - b2, b1, b2], axis=1), 1.0 / 3.0)
            best_t = np.where(ok, t, best_t)
            best_n = np.where(ok[:, None], self._tri_normal(tri, fl, vn, b), best_n)
        for m, r, rev in self.spheres:
            oc = o - m[:3, 3]
            a = (d * d).sum(1)
            b = 2.0 * (d * oc).sum(1)
            disc = b * b - 4 * a * ((oc * oc).sum(1) - r * r)
            sq = np.sqrt(np.maximum(disc, 0.0))
            t0, t1 = (-b - sq) / (2 * a), (-b + sq) / (2 * a)
            t = np.where(t0 > 0, t0, t1)
            ok = (disc >= 0) & (t > 0) & (t < best_t)
            n = (oc + t[:, None] * d) / r * (-1.0 if rev else 1.0)
            best_t = np.where(ok, t, best_t)
            best_n = np.where(ok[:, None], n, best_n)
        p = o + np.where(np.isfinite(best_t), best_t, 0.0)[:, None] * d
        return best_t, p, best_n

    def from_hit_records(self, o, d, t, b0, b1):
        """The interaction of hits named by closest-hit records (t, b0, b1) of rays o, d (n, 3), in float64: (p (n, 3), n (n, 3), p_error (n, 3), residual (n,), sin_theta (n,)).
        The record does not say which primitive it met in a numbering this model knows, so every primitive is asked for its point from the record - a triangle's
        b0 p0 + b1 p1 + (1 - b0 - b1) p2 (mesh.rs:336), a sphere's o + t d scaled onto the sphere (sphere.rs:172-177) - and the one nearest o + t d is taken; `residual`
        is that distance; sin_theta is 1 on a triangle and the sine of the hit's polar angle on a sphere (hypot(x, y) / r in object space: what Sphere::intersect divides by
        on the way to dpdu, dpdv and the normal). p_error is the reference's bound evaluated in float64: gamma(7) * sum |b_i p_i| (mesh.rs:328-332), gamma(5) * |p| for a sphere
        (sphere.rs:188), each through transform_point_with_error where the primitive lives in an object space.
        A sphere's ray point is evaluated as Sphere::intersect evaluates it - the origin taken to object space by Ray::transform, nudge included, and o + t d formed in FLOAT32
        (sphere.rs:94, 172) - and only
        then scaled onto the sphere in float64: the reference's p_error bounds that scaling (gamma(5) |p|), not the rounding of the ray point along the surface, which
        belongs to the hit and is the same for every caller of the interaction."""
        o32, d32, t32 = np.asarray(o, F), np.asarray(d, F), np.asarray(t, F)
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        b0, b1 = np.asarray(b0, np.float64), np.asarray(b1, np.float64)
        q = o + np.asarray(t, np.float64)[:, None] * d
        b = np.stack([b0, b1, 1.0 - b0 - b1], axis=1)
        nr = o.shape[0]
        best = np.full(nr, np.inf)
        out_p, out_n, out_e, out_s = np.zeros((nr, 3)), np.zeros((nr, 3)), np.zeros((nr, 3)), np.ones(nr)
        for tri, tri_obj, m, fl, sk, vn in self.prims:
            if sk:
                continue
            p = b @ tri
            res = np.linalg.norm(p - q, axis=1)
            better = res < best
            if not better.any():
                continue
            err = gamma(7) * np.abs(b[:, :, None] * tri_obj[None]).sum(1)
            if m is not None:
                err = _xf_error(m, b @ tri_obj, err)
            n = self._tri_normal(tri, fl, vn, b)
            best = np.where(better, res, best)
            out_p, out_n, out_e = np.where(better[:, None], p, out_p), np.where(better[:, None], n, out_n), np.where(better[:, None], err, out_e)
            out_s = np.where(better, 1.0, out_s)
        for m, r, rev in self.spheres:
            c = m[:3, 3]
            # Ray::transform(world_to_object) (ray.rs:46-71; the translation by -c), float32, one rounding per operation: the origin, its error bound gamma(3) * (|x| + |c|),
            # the step dt = dot(|d|, o_error) / |d|^2 along d that takes the origin off its error box; t of the record counts from THAT origin
            c32 = c.astype(F)
            g3 = F(3 * EPS) / (F(1) - F(3 * EPS))
            o_obj = o32 - c32
            o_err = g3 * (np.abs(o32) + np.abs(c32))
            ad = np.abs(d32)
            l2 = d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1] + d32[:, 2] * d32[:, 2]
            dt = (ad[:, 0] * o_err[:, 0] + ad[:, 1] * o_err[:, 1] + ad[:, 2] * o_err[:, 2]) / l2
            o_obj = o_obj + d32 * dt[:, None]
            q_obj = (o_obj + t32[:, None] * d32).astype(np.float64)
            dist = np.linalg.norm(q_obj, axis=1)
            p_obj = q_obj * (r / np.maximum(dist, 1e-300))[:, None]
            res = np.abs(dist - r)
            better = res < best
            n = p_obj / r * (-1.0 if rev else 1.0)
            err = _xf_error(m, p_obj, gamma(5) * np.abs(p_obj))
            best = np.where(better, res, best)
            out_p, out_n, out_e = np.where(better[:, None], c + p_obj, out_p), np.where(better[:, None], n, out_n), np.where(better[:, None], err, out_e)
            out_s = np.where(better, np.hypot(p_obj[:, 0], p_obj[:, 1]) / r, out_s)
        return out_p, out_n, out_e, best, out_s
