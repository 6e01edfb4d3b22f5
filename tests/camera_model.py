"""A float64 model of the two camera models the backend generates on the device (rt_camera_model_rays): pbrt-v3's OrthographicCamera - thin lens included - and
EnvironmentCamera, written from the definitions in include/rtx_hip.h, not from the device code.

`model_rays(kind, camera, width, height, p_film, spp)` takes the 24 floats of `host.camera_model` and film positions (..., 2) in raster coordinates and returns float64
records (..., 20): o.xyz, t_max = inf, d.xyz, 0, then rx_o, ry_o, rx_d, ry_d in world space, the differentials pulled toward the main ray by 1 / sqrt(spp). Nothing is
rounded to float32: the caller compares, or rounds once. The lens sample is given as `p_lens` (..., 2) in [0, 1)^2 - mapped to the disk here - or as `lens_point`
(..., 2), the point on the lens itself (a test that has no access to the sampler's 2D#1 reads it off the ray's origin)."""
import numpy as np

ORTHOGRAPHIC, ENVIRONMENT = 1, 2


def concentric_sample_disk(u):
    """pbrt-v3's ConcentricSampleDisk: [0, 1)^2 -> the unit disk."""
    u = np.asarray(u, np.float64)
    ox, oy = 2.0 * u[..., 0] - 1.0, 2.0 * u[..., 1] - 1.0
    wide = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(wide, ox, oy)
        theta = np.where(wide, (np.pi / 4.0) * (oy / ox), np.pi / 2.0 - (np.pi / 4.0) * (ox / oy))
    zero = (ox == 0.0) & (oy == 0.0)
    r, theta = np.where(zero, 0.0, r), np.where(zero, 0.0, theta)
    return np.stack([r * np.cos(theta), r * np.sin(theta)], axis=-1)


def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _vec(x, y, z):
    x, y, z = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(z, np.float64))
    return np.stack([x, y, z], axis=-1)


def camera_space(kind, camera, width, height, p_film, p_lens=None, lens_point=None):
    """(o, d, rx_o, ry_o, rx_d, ry_d) in camera space, before the world transform and the scaling."""
    cam = np.asarray(camera, np.float64).reshape(-1)
    p = np.asarray(p_film, np.float64)
    if kind == ENVIRONMENT:
        def gen(q):
            theta = np.pi * q[..., 1] / height
            phi = 2.0 * np.pi * q[..., 0] / width
            return np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
        d = gen(p)
        o = np.zeros_like(d)
        return o, d, o, o, gen(p + np.float64([1.0, 0.0])), gen(p + np.float64([0.0, 1.0]))
    assert kind == ORTHOGRAPHIC
    x0, x1, y0, y1 = cam[16:20]
    lens_radius, focal_distance = cam[20], cam[21]
    p_cam = _vec(x0 + p[..., 0] / width * (x1 - x0), y1 - p[..., 1] / height * (y1 - y0), 0.0)
    dx, dy = np.float64([(x1 - x0) / width, 0.0, 0.0]), np.float64([0.0, -(y1 - y0) / height, 0.0])
    d = np.zeros_like(p_cam)
    d[..., 2] = 1.0
    if not lens_radius > 0.0:
        return p_cam, d, p_cam + dx, p_cam + dy, d, d
    pl = np.asarray(lens_point, np.float64) if lens_point is not None else lens_radius * concentric_sample_disk(p_lens)
    ft = focal_distance / d[..., 2:3]
    p_focus = p_cam + ft * d
    o = _vec(pl[..., 0], pl[..., 1], 0.0)
    d = _normalize(p_focus - o)
    ft = focal_distance / d[..., 2:3]      # of the main ray after the lens step
    plane = np.concatenate([np.zeros_like(ft), np.zeros_like(ft), ft], axis=-1)
    return o, d, o, o, _normalize(p_cam + dx + plane - o), _normalize(p_cam + dy + plane - o)


def model_rays(kind, camera, width, height, p_film, spp, p_lens=None, lens_point=None):
    cam = np.asarray(camera, np.float64).reshape(-1)
    m = cam[:16].reshape(4, 4)

    def world(o_cam, d_cam):   # o_w = M o, d_w = normalize(M3x3 d): no origin nudge
        o = o_cam @ m[:3, :3].T + m[:3, 3]
        d = d_cam @ m[:3, :3].T
        return o, d / np.linalg.norm(d, axis=-1, keepdims=True)

    o_c, d_c, rxo_c, ryo_c, rxd_c, ryd_c = camera_space(kind, cam, width, height, p_film, p_lens, lens_point)
    o, d = world(o_c, d_c)
    rx_o, rx_d = world(rxo_c, rxd_c)
    ry_o, ry_d = world(ryo_c, ryd_c)
    s = 1.0 / np.sqrt(float(spp))
    out = np.zeros(o.shape[:-1] + (20,), np.float64)
    out[..., 0:3], out[..., 3], out[..., 4:7] = o, np.inf, d
    out[..., 8:11] = o + (rx_o - o) * s
    out[..., 11:14] = o + (ry_o - o) * s
    out[..., 14:17] = d + (rx_d - d) * s
    out[..., 17:20] = d + (ry_d - d) * s
    return out
