"""Ray generators for cameras the backend has no struct for, as inputs of `HostScene.render_rays` (rt_render_rays). Plain numpy, written from the definitions of
pbrt-v3 (cameras/orthographic.cpp, cameras/environment.cpp); the reference renderer has neither camera.

Both take `camera_to_world` (4 x 4, row-major, points as columns: `host.look_at(pos, look, up)[1]`), the film's resolution and `p_film` (H, W, ns, 2): the film
position of every sample in raster coordinates - x in [0, width) to the right, y in [0, height) downwards -, and return (H, W, ns, 8) float32 rays:
o.xyz, t_max = inf, d.xyz (unit length), 0. The arithmetic is float64, rounded once at the end.
"""
from __future__ import annotations

import numpy as np


def _rays(camera_to_world, o_cam, d_cam):
    m = np.asarray(camera_to_world, np.float64).reshape(4, 4)
    o = o_cam @ m[:3, :3].T + m[:3, 3]
    d = d_cam @ m[:3, :3].T
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    out = np.zeros(o.shape[:-1] + (8,), np.float32)
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


def orthographic(camera_to_world, screen_window, width, height, p_film):
    """OrthographicCamera::GenerateRay: the film position is mapped onto `screen_window` = (x_min, x_max, y_min, y_max) of the plane z = 0 of camera space - raster
    y = 0 is the window's y_max - and the ray leaves that point along +z. Parallel directions, origins on the window."""
    p = _film_positions(width, height, p_film)
    x0, x1, y0, y1 = (float(v) for v in screen_window)
    o = np.zeros(p.shape[:3] + (3,), np.float64)
    o[..., 0] = x0 + p[..., 0] / width * (x1 - x0)
    o[..., 1] = y1 - p[..., 1] / height * (y1 - y0)
    d = np.zeros_like(o)
    d[..., 2] = 1.0
    return _rays(camera_to_world, o, d)


def environment(camera_to_world, width, height, p_film):
    """EnvironmentCamera::GenerateRay (lat-long): theta = pi * y / height, phi = 2 pi * x / width, direction (sin theta cos phi, cos theta, sin theta sin phi) in
    camera space, every ray from the camera's origin."""
    p = _film_positions(width, height, p_film)
    theta = np.pi * p[..., 1] / height
    phi = 2.0 * np.pi * p[..., 0] / width
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
    return _rays(camera_to_world, np.zeros_like(d), d)
