"""Ray generators for cameras the backend has no struct for, as inputs of `HostScene.render_rays` (rt_render_rays). Plain numpy, written from the definitions of
pbrt-v3 (cameras/orthographic.cpp, cameras/environment.cpp); the reference renderer has neither camera.

Both take `camera_to_world` (4 x 4, row-major, points as columns: `host.look_at(pos, look, up)[1]`), the film's resolution and `p_film` (H, W, ns, 2): the film
position of every sample in raster coordinates - x in [0, width) to the right, y in [0, height) downwards -, and return (H, W, ns, 8) float32 rays:
o.xyz, t_max = inf, d.xyz (unit length), 0. The arithmetic is float64, rounded once at the end.

`differentials=True` makes records of 20 floats for RT_FLAG_RAY_DIFFERENTIALS: the eight above, then rx_o, ry_o, rx_d, ry_d - the rays through the film positions one
raster pixel to the right and one down (pbrt-v3's GenerateRayDifferential of each camera), pulled toward the main ray by 1 / sqrt(spp) as the renderer's
ScaleDifferentials does: rx_o = o + (rx_o - o) / sqrt(spp), and likewise for the other three. `spp` is the sample count the caller renders with.
"""
from __future__ import annotations

import numpy as np


def _world(camera_to_world, o_cam, d_cam):
    m = np.asarray(camera_to_world, np.float64).reshape(4, 4)
    o = o_cam @ m[:3, :3].T + m[:3, 3]
    d = d_cam @ m[:3, :3].T
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return o, d


def _rays(camera_to_world, o_cam, d_cam, shifted=None, spp=1):
    """shifted: ((o_cam, d_cam) at p_film + (1, 0), the same at p_film + (0, 1)) - the record then carries the scaled differentials."""
    o, d = _world(camera_to_world, o_cam, d_cam)
    out = np.zeros(o.shape[:-1] + (8 if shifted is None else 20,), np.float32)
    if shifted is not None:
        s = 1.0 / np.sqrt(float(spp))
        (rx_o, rx_d), (ry_o, ry_d) = (_world(camera_to_world, oc, dc) for oc, dc in shifted)
        out[..., 8:11] = o + (rx_o - o) * s
        out[..., 11:14] = o + (ry_o - o) * s
        out[..., 14:17] = d + (rx_d - d) * s
        out[..., 17:20] = d + (ry_d - d) * s
    out[..., 0:3] = o
    out[..., 3] = np.inf
    out[..., 4:7] = d
    return out


def _film_positions(width, height, p_film):
    p = np.asarray(p_film, np.float64)
    if p.ndim != 4 or p.shape[0] != height or p.shape[1] != width or p.shape[3] != 2:
        raise ValueError(f"p_film must have shape ({height}, {width}, ns, 2), not {p.shape}")
    return p


def pixel_centres(width, height, n_samples=1):
    """p_film of the pixel centres: (H, W, ns, 2), every sample of pixel (x, y) at (x + 0.5, y + 0.5)."""
    x, y = np.meshgrid(np.arange(width, dtype=np.float64) + 0.5, np.arange(height, dtype=np.float64) + 0.5)
    return np.broadcast_to(np.stack([x, y], axis=-1)[:, :, None, :], (height, width, n_samples, 2)).copy()


def orthographic(camera_to_world, screen_window, width, height, p_film, differentials=False, spp=1):
    """OrthographicCamera::GenerateRay: the film position is mapped onto `screen_window` = (x_min, x_max, y_min, y_max) of the plane z = 0 of camera space - raster
    y = 0 is the window's y_max - and the ray leaves that point along +z. Parallel directions, origins on the window.
    differentials (OrthographicCamera::GenerateRayDifferential): rx_o = o + dxCamera, ry_o = o + dyCamera - the window's pixel steps along the camera's x and -y axes -,
    rx_d = ry_d = d, then scaled by 1 / sqrt(spp)."""
    p = _film_positions(width, height, p_film)
    x0, x1, y0, y1 = (float(v) for v in screen_window)

    def gen(q):
        o = np.zeros(q.shape[:3] + (3,), np.float64)
        o[..., 0] = x0 + q[..., 0] / width * (x1 - x0)
        o[..., 1] = y1 - q[..., 1] / height * (y1 - y0)
        d = np.zeros_like(o)
        d[..., 2] = 1.0
        return o, d

    o, d = gen(p)
    if not differentials:
        return _rays(camera_to_world, o, d)
    dx, dy = np.float64([(x1 - x0) / width, 0.0, 0.0]), np.float64([0.0, -(y1 - y0) / height, 0.0])
    return _rays(camera_to_world, o, d, ((o + dx, d), (o + dy, d)), spp)


def environment(camera_to_world, width, height, p_film, differentials=False, spp=1):
    """EnvironmentCamera::GenerateRay (lat-long): theta = pi * y / height, phi = 2 pi * x / width, direction (sin theta cos phi, cos theta, sin theta sin phi) in
    camera space, every ray from the camera's origin.
    differentials (the base Camera::GenerateRayDifferential): this generator's own ray at p_film + (1, 0) and at p_film + (0, 1), then scaled by 1 / sqrt(spp)."""
    p = _film_positions(width, height, p_film)

    def gen(q):
        theta = np.pi * q[..., 1] / height
        phi = 2.0 * np.pi * q[..., 0] / width
        d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
        return np.zeros_like(d), d

    o, d = gen(p)
    if not differentials:
        return _rays(camera_to_world, o, d)
    return _rays(camera_to_world, o, d, (gen(p + np.float64([1.0, 0.0])), gen(p + np.float64([0.0, 1.0]))), spp)
