"""A float64 model of the irradiance every kind of light of this renderer delivers at a point, written from the definitions of radiometry - not from
oracle/ and not from rustracer_amd/csrc/ - and the statistic that holds a renderer's per-sample radiance to it.

A Lambertian receiver of albedo rho at x with unit normal n, seen along any ray, with max_depth = 1, returns samples whose expectation is rho / pi * E(x):
whichever light was picked, whichever half of the MIS estimator found it, whichever kernel shaded it. E(x) is

  area emitter    E = int_A Le [emits toward x] max(0, n.w) max(0, n_y.(-w)) / r^2 V(x, y) dA     (two_sided: |n_y.(-w)|)
  point light     E = I / (4 pi r^2) max(0, n.w) V          the 1 / (4 pi) is the reference's: rustracer-core/src/light/point.rs:50 divides the intensity by
                                                            4 pi r^2 (pbrt's own PointLight::Sample_Li returns I / r^2)
  distant light   E = L max(0, n.w) V
  infinite light  E = int L(w2l w) max(0, n.w) V dw         L: the level-0 bilinear lookup at (phi / 2 pi, theta / pi) of the map (light/infinite.rs:211-219 looks
                                                            it up with width 0: MIPMap::lookup goes to triangle(0, st)); the texels are mipmap_model.MipModel's
  several lights  the sum.

V(x, y) is a float64 Moeller-Trumbore test of the open segment against a list of occluder triangles.

Conventions that are the reference's, not radiometry's, and are inputs of the integrals:
  * a triangle's normal is (p0 - p2) x (p1 - p2), negated under reverse_orientation (shapes/mesh.rs:385, 419-421, 624); with vertex normals it is turned
    to the side of the interpolated normal instead and reverse_orientation is not read (mesh.rs:418, 623);
  * a sphere's and a cylinder's normal points away from the object-space z axis / centre, a disk's along +z; reverse_orientation negates it
    (sphere.rs:299-302, cylinder.rs:263-266, disk.rs:142-145).

Configurations the reference does not render as the integral, for which this model RAISES (NotPhysical) instead of returning a number:
  * a sphere under a scale: Sphere::sample_si's cone branch uses the object-space radius at the world-space centre (shapes/sphere.rs:246, 274);
  * a ring or a partial disk: Disk::sample ignores inner_radius and phi_max (disk.rs:138-140) while Disk::area counts them (disk.rs:156-158);
  * a partial sphere: Sphere::sample / sample_si ignore z_min, z_max and phi_max (sphere.rs:227-234, 267-299);
  * a non-rigid transform of a disk or a cylinder: 1 / area() is taken in object space (disk.rs:151, 156; cylinder.rs:255-257, 277);
  * a one-sided disk: Disk::sample gives the point the normal +z of object space (disk.rs:142), Disk::intersect gives it dpdu x dpdv with dpdv = (x, y, 0) *
    (radius - inner_radius) / r (disk.rs:95-96, interaction.rs:118; pbrt has inner_radius - radius), which is -z. A light-sampled point so emits to the +z side
    and a point the BSDF-sampled ray or a camera ray finds to the -z side: in front of the disk the MIS estimate lacks its BSDF-sampled half (1 - 2 % at 2.5 radii),
    behind it that half alone arrives. A `two_sided` disk is the integral.
  * a receiver inside a one-sided sphere that emits inward by reverse_orientation: Sphere::sample leaves the normal pointing outward (sphere.rs:230-233, no
    reverse_orientation there, unlike :300), so the light-sampled half of the estimator is black while the BSDF-sampled half, weighted as if it were not, sees Le.
    (`two_sided` emits inward physically.)

Quadrature. Every integral runs over the shape's own parameters - (b1, b2) of a triangle, the polar angles of a sphere about the axis through the receiver,
(z, phi) of a cylinder, (rho, phi) of a disk, (theta, phi) of the environment, its first cells cut at the texel centres where the bilinear interpolant has
its kinks - by 3 x 3 Gauss-Legendre cells that are split in four where it matters: each cell is evaluated itself and as its four children, and the cells
whose two values differ most are split until the summed difference is below `tol` of the integral (or 400 000 cells are spent: an occluder's edge). Every
integral is evaluated so at two resolutions whose cells share no line (`two_resolutions`); `irradiance` returns the finer value and the difference between
the two. Callers require that to be <= 1e-4 of the value. The lines on which an integrand is known to have a kink or a jump - the receiver's horizon, the
outline of an occluder - are followed down a fixed number of splits whatever the cells' two values say (`_mixed`): a line that cuts only a corner off a cell
passes by all of its nodes. The terminator of a one-sided sphere or cylinder lies on an edge of the first cells.

numpy only; the one project import is tests/mipmap_model.py.
"""
import numpy as np

from mipmap_model import WRAP_REPEAT, MipModel


class NotPhysical(ValueError):
    """The reference's sampling of this configuration is not the radiometric integral (see the module docstring)."""


# ------------------------------------------------------------------------------------------------ adaptive quadrature
_GX = np.array([-np.sqrt(0.6), 0.0, np.sqrt(0.6)])
_GW = np.array([5.0, 8.0, 5.0]) / 9.0
_W2 = _GW[:, None] * _GW[None, :]


def _gl_cells(f, u0, u1, v0, v1):
    """3 x 3 Gauss-Legendre over each cell [u0, u1] x [v0, v1]; f(u, v) -> (..., C). Returns (cells, C)."""
    hu, hv = 0.5 * (u1 - u0), 0.5 * (v1 - v0)
    u = (0.5 * (u0 + u1))[:, None, None] + hu[:, None, None] * _GX[None, :, None]
    v = (0.5 * (v0 + v1))[:, None, None] + hv[:, None, None] * _GX[None, None, :]
    u, v = np.broadcast_arrays(u, v)
    val = f(u, v)
    return (val * (_W2[None] * (hu * hv)[:, None, None])[..., None]).sum(axis=(1, 2))


def _split(u0, u1, v0, v1):
    """The four children of every cell, child-major: child k of cell i is entry k * n + i."""
    um, vm = 0.5 * (u0 + u1), 0.5 * (v0 + v1)
    return (np.concatenate([u0, um, u0, um]), np.concatenate([um, u1, um, u1]), np.concatenate([v0, v0, vm, vm]), np.concatenate([vm, vm, v1, v1]))


def _mixed(f, u0, u1, v0, v1):
    """Does a line on which the integrand has a kink or a jump cross the cell? f.edge(u, v) -> (..., K) quantities that change sign on such lines (the
    receiver's horizon, an occluder's outline), looked at in the cell's four corners and its centre: a line that cuts no more than a corner off a cell, and
    passes by all of its nodes, still parts that corner from the rest."""
    u = np.stack([u0, u1, u0, u1, 0.5 * (u0 + u1)], axis=-1)
    v = np.stack([v0, v0, v1, v1, 0.5 * (v0 + v1)], axis=-1)
    pos = f.edge(u, v) > 0.0
    return (pos.any(axis=1) & ~pos.all(axis=1)).any(axis=-1)


def integrate2d(f, u_edges, v_edges, tol=2e-6, max_cells=400_000, edge_depth=4):
    """int f du dv over the grid of first cells, adaptively (module docstring). Returns (value (C,), summed |fine - coarse| (scalar, largest channel)).
    Where f has an `edge` (see _mixed), the cells a kink or a jump crosses are split `edge_depth` times whatever their two values say."""
    ue, ve = np.asarray(u_edges, np.float64), np.asarray(v_edges, np.float64)
    a, b = np.meshgrid(np.arange(ue.size - 1), np.arange(ve.size - 1), indexing="ij")
    a, b = a.ravel(), b.ravel()
    cell = [ue[a], ue[a + 1], ve[b], ve[b + 1]]
    q_self = _gl_cells(f, *cell)
    n = q_self.shape[0]
    q_child = _gl_cells(f, *_split(*cell)).reshape(4, n, -1).transpose(1, 0, 2)   # (n, 4, C)
    has_edge = hasattr(f, "edge")
    todo = _mixed(f, *cell) if has_edge and edge_depth > 0 else np.zeros(n, bool)  # cells that are split regardless
    depth = np.zeros(n, np.int64)
    evaluated = 5 * n
    while True:
        fine = q_child.sum(axis=1)
        err = np.abs(fine - q_self).max(axis=-1)
        total, total_err = fine.sum(axis=0), float(err.sum())
        if (total_err <= tol * float(np.abs(total).max()) and not todo.any()) or evaluated > max_cells:
            return total, total_err
        r = todo | ((err > 0.5 * total_err / err.size) & (total_err > tol * float(np.abs(total).max())))
        m = int(r.sum())
        kid = _split(*(c[r] for c in cell))                                         # 4 m cells, child-major
        kid_self = q_child[r].transpose(1, 0, 2).reshape(4 * m, -1)
        kid_child = _gl_cells(f, *_split(*kid)).reshape(4, 4 * m, -1).transpose(1, 0, 2)
        kid_depth = np.tile(depth[r] + 1, 4)
        kid_todo = (_mixed(f, *kid) & (kid_depth < edge_depth)) if has_edge else np.zeros(4 * m, bool)
        evaluated += 16 * m
        cell = [np.concatenate([c[~r], k]) for c, k in zip(cell, kid)]
        q_self = np.concatenate([q_self[~r], kid_self])
        q_child = np.concatenate([q_child[~r], kid_child])
        depth, todo = np.concatenate([depth[~r], kid_depth]), np.concatenate([todo[~r], kid_todo])


def _at_least(e, k):
    e = np.asarray(e, np.float64)
    while e.size - 1 < k:
        e = np.sort(np.concatenate([e, 0.5 * (e[1:] + e[:-1])]))
    return e


def _cut_at_a_third(e):
    e = np.asarray(e, np.float64)
    return np.sort(np.concatenate([e, e[:-1] + (e[1:] - e[:-1]) / 3.0]))


def two_resolutions(f, u_edges, v_edges, tol, cells=16, edge_depth=4):
    """The integral at two resolutions: from at least `cells` x `cells` first cells as listed, and from four times as many, every first cell cut at a third of its
    width and height - so that the two trees of cells share no line but the first cells' own, and what all the nodes of a cell of one miss (the corner a kink
    cuts off it where `_mixed` was not told of the kink) the other sees. Returns (the finer run's value (C,), the largest channel's |finer - coarser|)."""
    ue, ve = _at_least(u_edges, cells), _at_least(v_edges, cells)
    a, _ = integrate2d(f, ue, ve, tol, edge_depth=edge_depth)
    b, _ = integrate2d(f, _cut_at_a_third(ue), _cut_at_a_third(ve), tol, edge_depth=edge_depth)
    return b, float(np.abs(a - b).max())


# ------------------------------------------------------------------------------------------------ visibility
def _blocked(o, d, t_max, occluders):
    """Does the open segment o + t d, 0 < t < t_max (arrays (..., 3), t_max (...) or inf), meet one of the triangles (T, 3, 3)? Moeller-Trumbore in float64."""
    hit = np.zeros(d.shape[:-1], bool)
    if occluders is None or len(occluders) == 0:
        return hit
    for tri in np.asarray(occluders, np.float64).reshape(-1, 3, 3):
        e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
        p = np.cross(d, e2)
        det = (p * e1).sum(-1)
        ok = np.abs(det) > 1e-300
        inv = 1.0 / np.where(ok, det, 1.0)
        s = o - tri[0]
        u = (s * p).sum(-1) * inv
        q = np.cross(s, e1)
        v = (d * q).sum(-1) * inv
        t = (q * e2).sum(-1) * inv
        hit |= ok & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t > 1e-9) & (t < t_max * (1.0 - 1e-9))
    return hit


# ------------------------------------------------------------------------------------------------ lights
def _rgb(v):
    v = np.asarray(v, np.float64)
    return np.full(3, float(v)) if v.ndim == 0 else v.reshape(3)


def _rigid(o2w, what):
    m = np.asarray(o2w, np.float64).reshape(4, 4)
    r = m[:3, :3]
    if not (np.allclose(r.T @ r, np.eye(3), atol=1e-5) and np.linalg.det(r) > 0 and np.allclose(m[3], (0, 0, 0, 1))):
        raise NotPhysical(f"{what} under a transform that is no rotation and translation: the sampling takes the radius (shapes/sphere.rs:246, 274) or the "
                          f"area (disk.rs:151, cylinder.rs:277) in object space")
    return r, m[:3, 3]


class _Area:
    """An area emitter over a parameter rectangle: point(u, v) -> (y, n_y, dA / du dv)."""
    two_sided = False

    def param(self, x):
        """(point(u, v) -> (y, n_y, dA / du dv), (u_edges, v_edges)): the parametrisation, which may place its axis and its first cells by the receiver."""
        return self.point, self.edges

    def integrand(self, x, n, occluders, point):
        def f(u, v):
            y, ny, jac = point(u, v)
            w = y - x
            r2 = (w * w).sum(-1)
            r = np.sqrt(r2)
            w = w / r[..., None]
            cos_x = np.maximum((w * n).sum(-1), 0.0)
            cos_y = -(ny * w).sum(-1)
            cos_y = np.abs(cos_y) if self.two_sided else np.maximum(cos_y, 0.0)
            g = cos_x * cos_y / r2 * jac
            if occluders is not None and len(occluders):
                g = np.where(_blocked(np.broadcast_to(x, w.shape), w, r, occluders), 0.0, g)
            return g[..., None] * self.le

        def edge(u, v):
            w = point(u, v)[0] - x
            out = [(w * n).sum(-1)]                                  # the receiver's horizon
            if occluders is not None and len(occluders):
                r = np.sqrt((w * w).sum(-1))
                out.append(0.5 - _blocked(np.broadcast_to(x, w.shape), w / r[..., None], r, occluders))
            return np.stack(out, axis=-1)
        f.edge = edge
        return f

    def irradiance(self, x, n, occluders, tol, cells=16):
        point, edges = self.param(x)
        return two_resolutions(self.integrand(x, n, occluders, point), *edges, tol=tol, cells=cells, edge_depth=7 if occluders is not None and len(occluders) else 4)


class Triangle(_Area):
    def __init__(self, p, le, two_sided=False, reverse_orientation=False, normals=None):
        self.p = np.asarray(p, np.float64).reshape(3, 3)
        self.le, self.two_sided = _rgb(le), bool(two_sided)
        ng = np.cross(self.p[0] - self.p[2], self.p[1] - self.p[2])
        self.area2 = np.linalg.norm(ng)
        self.ng = ng / self.area2
        self.normals = None if normals is None else np.asarray(normals, np.float64).reshape(3, 3)
        if self.normals is None and reverse_orientation:
            self.ng = -self.ng
        self.edges = (np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9))

    def point(self, u, v):
        b1, b2 = u, v * (1.0 - u)            # the unit square onto the triangle; dA = |e1 x e2| (1 - u) du dv
        b0 = 1.0 - b1 - b2
        y = b0[..., None] * self.p[0] + b1[..., None] * self.p[1] + b2[..., None] * self.p[2]
        ny = np.broadcast_to(self.ng, y.shape)
        if self.normals is not None:
            ns = b0[..., None] * self.normals[0] + b1[..., None] * self.normals[1] + b2[..., None] * self.normals[2]
            ny = np.where(((ny * ns).sum(-1) < 0.0)[..., None], -ny, ny)
        return y, ny, self.area2 * (1.0 - u)


def quad(p0, p1, p2, p3, le, **kw):
    """The two triangles (0 1 2), (0 2 3) of a quadrilateral; `normals`: four vertex normals."""
    nrm = kw.pop("normals", None)
    pick = lambda a, i: None if a is None else [a[k] for k in i]
    p = [p0, p1, p2, p3]
    return [Triangle(pick(p, i), le, normals=pick(nrm, i), **kw) for i in ((0, 1, 2), (0, 2, 3))]


class _Quadric(_Area):
    def __init__(self, o2w, radius, le, two_sided, reverse_orientation, what):
        self.rot, self.shift = _rigid(o2w, what)
        self.radius, self.le, self.two_sided = float(radius), _rgb(le), bool(two_sided)
        self.sign = -1.0 if reverse_orientation else 1.0

    def world(self, p_obj, n_obj):
        return p_obj @ self.rot.T + self.shift, self.sign * (n_obj @ self.rot.T)


class Sphere(_Quadric):
    def __init__(self, o2w, radius, le, two_sided=False, reverse_orientation=False, z_min=None, z_max=None, phi_max=360.0):
        super().__init__(o2w, radius, le, two_sided, reverse_orientation, "a sphere emitter")
        z0, z1 = (-radius if z_min is None else z_min), (radius if z_max is None else z_max)
        if min(z0, z1) > -radius or max(z0, z1) < radius or phi_max < 360.0:
            raise NotPhysical("a partial sphere emitter: Sphere::sample and sample_si ignore the clipping (shapes/sphere.rs:227-234, 267-299)")

    def param(self, x):
        """A full sphere has no axis of its own: (alpha, phi) are taken about the axis through the receiver, dA = r^2 sin(alpha) dalpha dphi. The terminator of a
        one-sided sphere seen from outside is then the parameter line alpha = acos(r / D), and first cells end on it."""
        a = np.asarray(x, np.float64) - self.shift
        dist = np.linalg.norm(a)
        a = a / dist if dist > 1e-12 * self.radius else np.array([0.0, 0.0, 1.0])
        t1 = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.6 else [0.0, 1.0, 0.0])
        t1 /= np.linalg.norm(t1)
        t2 = np.cross(a, t1)

        def point(alpha, phi):
            sa = np.sin(alpha)
            d = (sa * np.cos(phi))[..., None] * t1 + (sa * np.sin(phi))[..., None] * t2 + np.cos(alpha)[..., None] * a
            # from outside only the cap alpha < acos(r / D) is in view: the sphere hides the rest of itself, whichever way that emits
            return self.shift + self.radius * d, self.sign * d, self.radius ** 2 * sa * (1.0 if dist <= self.radius else alpha < cut)
        if dist > self.radius:
            cut = np.arccos(self.radius / dist)
            alpha = np.concatenate([np.linspace(0.0, cut, 9), np.linspace(cut, np.pi, 5)[1:]])
        else:
            alpha = np.linspace(0.0, np.pi, 13)
        return point, (alpha, np.linspace(0.0, 2.0 * np.pi, 17))

    def irradiance(self, x, n, occluders, tol, cells=16):
        if self.sign < 0 and not self.two_sided and np.linalg.norm(np.asarray(x, np.float64) - self.shift) <= self.radius:
            raise NotPhysical("a receiver inside a one-sided sphere emitting inward by reverse_orientation (shapes/sphere.rs:230-233)")
        return super().irradiance(x, n, occluders, tol, cells)


class Disk(_Quadric):
    def __init__(self, o2w, radius, le, two_sided=False, reverse_orientation=False, height=0.0, inner_radius=0.0, phi_max=360.0):
        super().__init__(o2w, radius, le, two_sided, reverse_orientation, "a disk emitter")
        if inner_radius != 0.0 or phi_max < 360.0:
            raise NotPhysical("a ring or a partial disk emitter: Disk::sample ignores inner_radius and phi_max (shapes/disk.rs:138-140)")
        if not two_sided:
            raise NotPhysical("a one-sided disk emitter: a sampled point's normal is +z (shapes/disk.rs:142), an intersected point's -z (disk.rs:95-96 with "
                              "interaction.rs:118), so the two halves of the estimator light opposite sides")
        self.height = float(height)
        self.edges = (np.linspace(0.0, self.radius, 9), np.linspace(0.0, 2.0 * np.pi, 33))

    def point(self, rho, phi):
        p = np.stack([rho * np.cos(phi), rho * np.sin(phi), np.full(rho.shape, self.height)], axis=-1)
        y, ny = self.world(p, np.broadcast_to(np.array([0.0, 0.0, 1.0]), p.shape))
        return y, ny, rho                                    # dA = rho drho dphi


class Cylinder(_Quadric):
    def __init__(self, o2w, radius, le, z_min=-1.0, z_max=1.0, phi_max=360.0, two_sided=False, reverse_orientation=False):
        super().__init__(o2w, radius, le, two_sided, reverse_orientation, "a cylinder emitter")
        if two_sided or reverse_orientation:     # physical, but the inside of a cylinder is seen past its own wall, which this model does not intersect
            raise NotImplementedError("a cylinder that emits from its inside: the model leaves out the cylinder's shadow on itself")
        self.z = (min(z_min, z_max), max(z_min, z_max))
        self.phi_max = np.radians(min(max(phi_max, 0.0), 360.0))

    def param(self, x):
        """(z, phi), dA = r dz dphi. Seen from outside, the surface turns away from the receiver along two lines of constant phi: first cells end there."""
        xo = (np.asarray(x, np.float64) - self.shift) @ self.rot          # the receiver in object space
        rho = np.hypot(xo[0], xo[1])
        phi = [0.0, self.phi_max]
        if rho > self.radius:
            half, mid = np.arccos(self.radius / rho), np.arctan2(xo[1], xo[0])
            phi += [c for c in np.mod([mid - half, mid + half], 2.0 * np.pi) if 0.0 < c < self.phi_max]
        phi = np.unique(phi)
        phi = np.concatenate([np.linspace(a, b, max(2, int(np.ceil((b - a) / (np.pi / 8))) + 1))[:-1] for a, b in zip(phi[:-1], phi[1:])] + [[self.phi_max]])
        return self.point, (np.linspace(self.z[0], self.z[1], 9), phi)

    def point(self, z, phi):
        c, s = np.cos(phi), np.sin(phi)
        y, ny = self.world(np.stack([self.radius * c, self.radius * s, z], axis=-1), np.stack([c, s, np.zeros(z.shape)], axis=-1))
        return y, ny, np.full(z.shape, self.radius)


class Point:
    def __init__(self, pos, intensity):
        self.pos, self.i = np.asarray(pos, np.float64).reshape(3), _rgb(intensity)

    def irradiance(self, x, n, occluders, tol, cells=16):
        w = self.pos - x
        r = np.linalg.norm(w)
        w = w / r
        if _blocked(x, w, r, occluders):
            return np.zeros(3), 0.0
        return self.i / (4.0 * np.pi * r * r) * max(0.0, float(w @ n)), 0.0     # light/point.rs:50


class Distant:
    def __init__(self, to_light, radiance):
        w = np.asarray(to_light, np.float64).reshape(3)
        self.w, self.l = w / np.linalg.norm(w), _rgb(radiance)

    def irradiance(self, x, n, occluders, tol, cells=16):
        if _blocked(x, self.w, np.inf, occluders):
            return np.zeros(3), 0.0
        return self.l * max(0.0, float(self.w @ n)), 0.0


class Infinite:
    """An environment map (h, w, 3), both sizes a power of two so that level 0 of the pyramid is the data, under a rotation l2w."""

    def __init__(self, image, l2w=None):
        img = np.asarray(image, np.float32)
        h, w = img.shape[:2]
        if (w & (w - 1)) or (h & (h - 1)):
            raise ValueError("the model integrates level 0 as given: use a power-of-two map")
        self.mip = MipModel(img, wrap=WRAP_REPEAT)     # InfiniteAreaLight::new builds its MIPMap with WrapMode::Repeat (light/infinite.rs:71-77)
        self.w, self.h = w, h
        self.rot, _ = _rigid(np.eye(4) if l2w is None else l2w, "an infinite light")
        # bilinear interpolation is a polynomial between texel centres: first cells end there (and at the map's edges)
        cut = lambda k, span: np.unique(np.concatenate([[0.0], (np.arange(k) + 0.5) / k, [1.0]])) * span
        refine = lambda e: np.unique(np.concatenate([e, 0.5 * (e[1:] + e[:-1])]))
        self.edges = (refine(cut(h, np.pi)), refine(cut(w, 2.0 * np.pi)))

    def radiance_st(self, st_s, st_t):
        """The level-0 bilinear lookup of MIPMap::triangle (mipmap.rs:285-308) at (s, t) in [0, 1]^2, over mipmap_model's texels."""
        s, t = st_s * self.w - 0.5, st_t * self.h - 0.5
        s0, t0 = np.floor(s), np.floor(t)
        ds, dt = (s - s0)[..., None], (t - t0)[..., None]
        s0, t0 = s0.astype(np.int64), t0.astype(np.int64)
        tx = lambda a, b: self.mip.texel(0, s0 + a, t0 + b)
        return (1 - ds) * (1 - dt) * tx(0, 0) + (1 - ds) * dt * tx(0, 1) + ds * (1 - dt) * tx(1, 0) + ds * dt * tx(1, 1)

    def radiance(self, w_world):
        """L arriving from direction w (unit, world space): light/infinite.rs:211-219."""
        wl = np.asarray(w_world, np.float64) @ self.rot          # w2l = l2w^T
        phi = np.arctan2(wl[..., 1], wl[..., 0])
        phi = np.where(phi < 0.0, phi + 2.0 * np.pi, phi)
        return self.radiance_st(phi / (2.0 * np.pi), np.arccos(np.clip(wl[..., 2], -1.0, 1.0)) / np.pi)

    def irradiance(self, x, n, occluders, tol, cells=16):
        def f(theta, phi):
            st = np.sin(theta)
            w = np.stack([st * np.cos(phi), st * np.sin(phi), np.cos(theta)], axis=-1) @ self.rot.T
            g = np.maximum((w * n).sum(-1), 0.0) * st
            if occluders is not None and len(occluders):
                g = np.where(_blocked(np.broadcast_to(x, w.shape), w, np.inf, occluders), 0.0, g)
            return g[..., None] * self.radiance_st(phi / (2.0 * np.pi), theta / np.pi)

        def edge(theta, phi):
            st = np.sin(theta)
            w = np.stack([st * np.cos(phi), st * np.sin(phi), np.cos(theta)], axis=-1) @ self.rot.T
            out = [(w * n).sum(-1)]
            if occluders is not None and len(occluders):
                out.append(0.5 - _blocked(np.broadcast_to(x, w.shape), w, np.inf, occluders))
            return np.stack(out, axis=-1)
        f.edge = edge
        return two_resolutions(f, *self.edges, tol=tol, cells=cells)


def irradiance(lights, x, n, occluders=None, tol=2e-6, cells=16):
    """E(x) (3,) of the lights (one, or a list; `quad` returns a list) on a receiver at x with unit normal n, and the difference between the two
    resolutions, summed over the lights (a scalar: the largest channel's). `occluders`: (T, 3, 3) triangles; `tol`, `cells`: of the quadrature (the defaults
    serve the 1e-4 the tests' cases ask for)."""
    x, n = np.asarray(x, np.float64).reshape(3), np.asarray(n, np.float64).reshape(3)
    n = n / np.linalg.norm(n)
    flat = []
    for l in (lights if isinstance(lights, (list, tuple)) else [lights]):
        flat.extend(l if isinstance(l, (list, tuple)) else [l])
    e, d = np.zeros(3), 0.0
    for l in flat:
        ei, di = l.irradiance(x, n, occluders, tol, cells)
        e, d = e + ei, d + di
    return e, d


# ------------------------------------------------------------------------------------------------ the statistic
K_SIGMA = 5.0        # a case makes 1e2 - 1e3 comparisons; a Gaussian tail beyond 5 standard errors is 6e-7. The (0, 2)-sequence stratifies, so se overstates
REL_FLOOR = 1e-4     # the project's allowance for radiance-only v_rcp arithmetic (tests/test_gpu_scenes.py, ..._stays_ten_times_inside_the_image_gate)
CAP_POOLED = 0.002   # sqrt(sum se^2) <= CAP_POOLED * sum M: a pooled bias of about 1 % cannot hide in the noise
CAP_POINT = 0.03     # se_p <= CAP_POINT * M_p


def statistic(samples, model, extra=None):
    """samples (P, N): one channel of the per-sample radiance of P receiver points; model (P,): rho / pi * E; extra (P,): a further absolute allowance per
    point (the oracle's pixel footprint; float32 geometry of a point in an emitter's plane). Returns a dict of the figures and of the verdicts:
      point_ok   |m_p - M_p| <= 5 se_p + 1e-4 M_p + extra_p, every point with M_p > 0; M_p = 0: every sample is 0, or, with an extra, |m_p| <= extra_p
      pooled_ok  |sum m - sum M| <= 5 sqrt(sum se^2) + 1e-4 sum M + sum extra, over the points with M_p > 0
      caps_ok    sqrt(sum se^2) <= 0.002 sum M and se_p <= 0.03 M_p, on these very samples."""
    s = np.asarray(samples, np.float64)
    big_m = np.asarray(model, np.float64)
    p, n = s.shape
    assert big_m.shape == (p,)
    extra = np.zeros(p) if extra is None else np.asarray(extra, np.float64)
    m, se = s.mean(axis=1), s.std(axis=1, ddof=1) / np.sqrt(n)
    dev = np.abs(m - big_m)
    allow = K_SIGMA * se + REL_FLOOR * big_m + extra
    lit = big_m > 0
    # a black point: 5 se of its samples would let a single stray one pass (its mean is about its se). Every sample is 0 - or, where the point has an allowance
    # (float32 geometry in an emitter's plane), the mean stays inside that allowance alone
    allow = np.where(lit, allow, extra)
    point_ok = (dev <= allow) & (lit | (extra > 0) | np.all(s == 0.0, axis=1))
    sm, sbm, pse = float(m[lit].sum()), float(big_m[lit].sum()), float(np.sqrt((se[lit] ** 2).sum()))
    z = np.where(lit & (se > 0), (m - big_m) / np.where(se > 0, se, 1.0), 0.0)
    worst = int(np.argmax(np.abs(z)))
    out = dict(n=n, points=p, lit=int(lit.sum()), m=m, se=se, model=big_m, dev=dev, allow=allow,
               point_ok=point_ok, pooled_dev=abs(sm - sbm), pooled_allow=K_SIGMA * pse + REL_FLOOR * sbm + float(extra[lit].sum()),
               pooled_rel=(sm / sbm - 1.0) if sbm > 0 else 0.0, pooled_se_rel=(pse / sbm) if sbm > 0 else 0.0,
               worst_z=float(z[worst]), worst_point=worst,
               point_cap=float((se[lit] / big_m[lit]).max()) if lit.any() else 0.0)
    out["pooled_ok"] = out["pooled_dev"] <= out["pooled_allow"]
    out["caps_ok"] = out["pooled_se_rel"] <= CAP_POOLED and out["point_cap"] <= CAP_POINT
    return out


def line(who, case, st):
    """The record of a case, as MEASUREMENTS.md lists it."""
    return (f"RADIOMETRY {who} {case}: N {st['n']}, points {st['points']} ({st['lit']} lit), pooled sum m / sum M - 1 = {st['pooled_rel']:+.2e}, "
            f"pooled se / sum M = {st['pooled_se_rel']:.2e}, worst (m - M) / se = {st['worst_z']:+.2f} (point {st['worst_point']}), "
            f"largest se_p / M_p = {st['point_cap']:.2e}")


def require(st, what=""):
    """Assert the three verdicts of `statistic`, naming the points that miss."""
    bad = np.flatnonzero(~st["point_ok"])
    assert st["caps_ok"], f"{what}: the samples are too noisy to judge: pooled se / sum M = {st['pooled_se_rel']:.3e} (cap {CAP_POOLED}), largest se_p / M_p = {st['point_cap']:.3e} (cap {CAP_POINT})"
    assert bad.size == 0, f"{what}: points {bad.tolist()} miss: m {st['m'][bad]}, M {st['model'][bad]}, se {st['se'][bad]}, allowed {st['allow'][bad]}"
    assert st["pooled_ok"], f"{what}: pooled |sum m - sum M| = {st['pooled_dev']:.4e} > {st['pooled_allow']:.4e} (sum m / sum M - 1 = {st['pooled_rel']:+.3e})"
