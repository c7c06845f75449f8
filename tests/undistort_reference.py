"""NumPy float64 restatement of the undistortion rule (the comment at the top of
pegasus_amd/csrc/undistort.hip.h): the camera models, the Newton inverse, the bilinear remap and the box mean, with the same
expression trees as the kernels.  It shares no code with the package and nothing here runs on a device.  ``Backend`` is what
pegasus_amd.undistort takes in place of the device, so the host tests run the camera rule and the whole project job on it.
"""
import numpy as np

# (number of focal lengths, number of distortion coefficients) per model name
SHAPES = {"SIMPLE_PINHOLE": (1, 0), "PINHOLE": (2, 0), "SIMPLE_RADIAL": (1, 1), "RADIAL": (1, 2), "OPENCV": (2, 4),
          "OPENCV_FISHEYE": (2, 4), "FULL_OPENCV": (2, 8)}
TIE_EPS = 1e-6                       # a pre-rounding value this close to k + 0.5 is a near tie


def split(model, params):
    """fx, fy, cx, cy, k [8] of a model's parameters in COLMAP's order"""
    p = [float(v) for v in params]
    n_f, n_k = SHAPES[model]
    assert len(p) == n_f + 2 + n_k, (model, len(p))
    fx, fy = (p[0], p[0]) if n_f == 1 else (p[0], p[1])
    cx, cy = p[n_f], p[n_f + 1]
    k = np.zeros(8)
    k[:n_k] = p[n_f + 2:]
    return fx, fy, cx, cy, k


def displacement(model, k, u, v):
    """(du, dv) of normalised points, elementwise"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if model in ("SIMPLE_PINHOLE", "PINHOLE"):
        return np.zeros_like(u), np.zeros_like(v)
    with np.errstate(all="ignore"):
        if model == "OPENCV_FISHEYE":
            r = np.sqrt(u * u + v * v)
            t = np.arctan(r)
            t2 = t * t
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            td = t * ((((1.0 + k[0] * t2) + k[1] * t4) + k[2] * t6) + k[3] * t8)
            small = r < 1e-12
            s = td / np.where(small, 1.0, r) - 1.0
            return np.where(small, 0.0, u * s), np.where(small, 0.0, v * s)
        u2, v2 = u * u, v * v
        r2 = u2 + v2
        if model == "SIMPLE_RADIAL":
            rad = k[0] * r2
            return u * rad, v * rad
        r4 = r2 * r2
        if model == "RADIAL":
            rad = k[0] * r2 + k[1] * r4
            return u * rad, v * rad
        uv = u * v
        p1, p2 = k[2], k[3]
        if model == "OPENCV":
            rad = k[0] * r2 + k[1] * r4
            return ((u * rad + ((2.0 * p1) * uv)) + p2 * (r2 + 2.0 * u2),
                    (v * rad + ((2.0 * p2) * uv)) + p1 * (r2 + 2.0 * v2))
        assert model == "FULL_OPENCV"
        r6 = r4 * r2
        rad = (((1.0 + k[0] * r2) + k[1] * r4) + k[4] * r6) / (((1.0 + k[5] * r2) + k[6] * r4) + k[7] * r6)
        return (((u * rad + ((2.0 * p1) * uv)) + p2 * (r2 + 2.0 * u2)) - u,
                ((v * rad + ((2.0 * p2) * uv)) + p1 * (r2 + 2.0 * v2)) - v)


def jacobian(model, k, u, v):
    """J = I + d(du, dv)/d(u, v): j00, j01, j10, j11"""
    one, zero = np.ones_like(u), np.zeros_like(u)
    if model in ("SIMPLE_PINHOLE", "PINHOLE"):
        return one, zero, zero, one
    with np.errstate(all="ignore"):
        u2, v2 = u * u, v * v
        r2 = u2 + v2
        uv = u * v
        p1 = p2 = 0.0
        if model == "SIMPLE_RADIAL":
            rad, drad = k[0] * r2, k[0] * one
        elif model in ("RADIAL", "OPENCV"):
            rad = k[0] * r2 + k[1] * (r2 * r2)
            drad = k[0] + (2.0 * k[1]) * r2
            if model == "OPENCV":
                p1, p2 = k[2], k[3]
        elif model == "FULL_OPENCV":
            r4 = r2 * r2
            r6 = r4 * r2
            num = ((1.0 + k[0] * r2) + k[1] * r4) + k[4] * r6
            den = ((1.0 + k[5] * r2) + k[6] * r4) + k[7] * r6
            dnum = (k[0] + (2.0 * k[1]) * r2) + (3.0 * k[4]) * r4
            dden = (k[5] + (2.0 * k[6]) * r2) + (3.0 * k[7]) * r4
            rad = num / den - 1.0
            drad = (dnum * den - num * dden) / (den * den)
            p1, p2 = k[2], k[3]
        else:
            r = np.sqrt(r2)
            t = np.arctan(r)
            t2 = t * t
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            td = t * ((((1.0 + k[0] * t2) + k[1] * t4) + k[2] * t6) + k[3] * t8)
            dtd = (((1.0 + (3.0 * k[0]) * t2) + (5.0 * k[1]) * t4) + (7.0 * k[2]) * t6) + (9.0 * k[3]) * t8
            small = r < 1e-12
            rs = np.where(small, 1.0, r)
            rad = np.where(small, 0.0, td / rs - 1.0)
            drad = np.where(small, 0.0, ((dtd / (1.0 + r2)) * rs - td) / (np.where(small, 1.0, r2) * (2.0 * rs)))
        cross = ((2.0 * uv) * drad + (2.0 * p1) * u) + (2.0 * p2) * v
        j00 = 1.0 + (((rad + (2.0 * u2) * drad) + (2.0 * p1) * v) + (6.0 * p2) * u)
        j11 = 1.0 + (((rad + (2.0 * v2) * drad) + (2.0 * p2) * u) + (6.0 * p1) * v)
    return j00, cross, cross, j11


def distort(model, params, uv):
    """normalised points [n,2] -> image points [n,2]"""
    fx, fy, cx, cy, k = split(model, params)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    du, dv = displacement(model, k, uv[:, 0], uv[:, 1])
    return np.stack([fx * (uv[:, 0] + du) + cx, fy * (uv[:, 1] + dv) + cy], axis=1)


def residual(model, params, uv, xy):
    """|distort(uv) - x_d|_inf per point, in normalised units, and the bound 1e-12 max(1, |x_d|_inf) it is held against"""
    fx, fy, cx, cy, k = split(model, params)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    xd, yd = (xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy
    du, dv = displacement(model, k, uv[:, 0], uv[:, 1])
    res = np.maximum(np.abs((uv[:, 0] + du) - xd), np.abs((uv[:, 1] + dv) - yd))
    return res, 1e-12 * np.maximum(1.0, np.maximum(np.abs(xd), np.abs(yd)))


def undistort_points(model, params, xy):
    """image points [n,2] -> (normalised points [n,2], ok uint8 [n]); a point that is not ok is NaN"""
    fx, fy, cx, cy, k = split(model, params)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    xd, yd = (xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy
    x, y = xd.copy(), yd.copy()
    live = np.ones(len(x), bool)                 # still iterating
    converged = np.zeros(len(x), bool)
    with np.errstate(all="ignore"):
        for _ in range(100):
            if not live.any():
                break
            du, dv = displacement(model, k, x, y)
            j00, j01, j10, j11 = jacobian(model, k, x, y)
            det = j00 * j11 - j01 * j10
            sheet = (det > 0.0) & (j00 + j11 > 0.0)
            live &= sheet                        # an iterate off the sheet that holds the origin ends the point as failed
            rx, ry = (x + du) - xd, (y + dv) - yd
            sx, sy = (j11 * rx - j01 * ry) / det, (j00 * ry - j10 * rx) / det
            x = np.where(live, x - sx, x)
            y = np.where(live, y - sy, y)
            done = live & (sx * sx + sy * sy < 1e-20)
            converged |= done
            live &= ~done
        du, dv = displacement(model, k, x, y)
        res = np.maximum(np.abs((x + du) - xd), np.abs((y + dv) - yd))
        ok = converged & (res <= 1e-12 * np.maximum(1.0, np.maximum(np.abs(xd), np.abs(yd))))
    uv = np.stack([np.where(ok, x, np.nan), np.where(ok, y, np.nan)], axis=1)
    return uv, ok.astype(np.uint8)


def remap(src, model, params, pinhole, out_w, out_h, with_ties=False):
    """The remap of one image: src uint8 [h,w] or [h,w,c] -> uint8 [out_h,out_w(,c)].  ``with_ties``: also a bool [out_h,out_w]
    mask of the pixels one of whose channels lies within TIE_EPS of a rounding tie before it is rounded."""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    squeeze = src.ndim == 2
    s = (src[:, :, None] if squeeze else src).astype(np.float64)
    h, w, c = s.shape
    fx, fy, cx, cy, k = split(model, params)
    pfx, pfy, pcx, pcy = (float(v) for v in pinhole)
    u = ((np.arange(out_w, dtype=np.float64) + 0.5) - pcx) / pfx
    v = ((np.arange(out_h, dtype=np.float64) + 0.5) - pcy) / pfy
    u, v = np.broadcast_to(u[None, :], (out_h, out_w)), np.broadcast_to(v[:, None], (out_h, out_w))
    du, dv = displacement(model, k, u, v)
    with np.errstate(all="ignore"):
        sx, sy = (fx * (u + du) + cx) - 0.5, (fy * (v + dv) + cy) - 0.5
        inside = (sx >= 0.0) & (sx <= w - 1.0) & (sy >= 0.0) & (sy <= h - 1.0)
    sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    fx0, fy0 = np.floor(sx), np.floor(sy)
    ax, ay = (sx - fx0)[..., None], (sy - fy0)[..., None]
    ix0, iy0 = fx0.astype(np.int64), fy0.astype(np.int64)
    ix1, iy1 = np.minimum(ix0 + 1, w - 1), np.minimum(iy0 + 1, h - 1)
    p00, p01, p10, p11 = s[iy0, ix0], s[iy0, ix1], s[iy1, ix0], s[iy1, ix1]
    val = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11)
    out = np.minimum(255.0, np.floor(val + 0.5))
    out = np.where(inside[..., None], out, 0.0).astype(np.uint8)
    out = out[:, :, 0] if squeeze else out
    if not with_ties:
        return out
    frac = val - np.floor(val)
    ties = (np.abs(frac - 0.5) <= TIE_EPS).any(axis=2) & inside
    return out, ties


def box_downscale(src, f):
    """(sum of f x f bytes + f f / 2) // (f f) per channel; columns and rows beyond a multiple of f are dropped"""
    src = np.asarray(src)
    squeeze = src.ndim == 2
    s = (src[:, :, None] if squeeze else src).astype(np.int64)
    oh, ow = s.shape[0] // f, s.shape[1] // f
    t = s[:oh * f, :ow * f].reshape(oh, f, ow, f, -1).sum(axis=(1, 3))
    out = ((t + (f * f) // 2) // (f * f)).astype(np.uint8)
    return out[:, :, 0] if squeeze else out


class Backend:
    """The device's place in pegasus_amd.undistort (the ``backend`` argument): images are numpy arrays."""
    device_png = False

    def undistort_points(self, camera, xy):
        return undistort_points(camera.model, camera.params, xy)

    def upload(self, image):
        return np.asarray(image)

    def download(self, image):
        return np.asarray(image)

    def undistort_images(self, images, cameras, out_cameras):
        return [remap(im, c.model, c.params, o.params, o.width, o.height) for im, c, o in zip(images, cameras, out_cameras)]

    def box_downscale(self, images, factor):
        return [box_downscale(im, factor) for im in images]


# ---- the fixtures the host and the GPU tests share --------------------------------------------------------------------------
COEFFS = {"SIMPLE_PINHOLE": [], "PINHOLE": [], "SIMPLE_RADIAL": [-0.12], "RADIAL": [-0.15, 0.04],
          "OPENCV": [-0.2, 0.06, 0.004, -0.003], "FULL_OPENCV": [0.1, -0.05, 0.003, 0.002, 0.01, 0.02, -0.01, 0.005],
          "OPENCV_FISHEYE": [0.05, -0.02, 0.01, -0.004]}
DISTORTED = ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV", "OPENCV_FISHEYE")
POLYNOMIAL = ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")
REMAP_WIDTHS, REMAP_HEIGHTS, REMAP_CHANNELS = (1, 3, 4, 5, 255, 256, 257), (1, 7), (1, 3, 4)
SEED = 20260


def camera_params(model, fx, fy, cx, cy, coeffs=None):
    """A model's parameters in COLMAP's order (one-focal models take fx)"""
    focal = [fx] if SHAPES[model][0] == 1 else [fx, fy]
    return np.array(focal + [cx, cy] + list(COEFFS[model] if coeffs is None else coeffs), dtype=np.float64)


def remap_cases(model):
    """The remap fixtures of one model: every output width x height x channel count of the lists above, a seeded random
    source a little larger or smaller than the output so that some pixels fall outside, and row paddings for both images.
    Each case: dict(model, params, src, pinhole, out_w, out_h, pad_src, pad_dst)."""
    rng = np.random.default_rng(SEED + sorted(SHAPES).index(model))
    cases = []
    for i, (W, H, c) in enumerate((W, H, c) for W in REMAP_WIDTHS for H in REMAP_HEIGHTS for c in REMAP_CHANNELS):
        w, h = max(2, W + (3, -1, 0)[i % 3]), max(2, H + (2, 1)[i % 2])
        f = 0.9 * max(w, h) + 0.37
        params = camera_params(model, f, 1.04 * f, 0.5 * w + 0.3, 0.5 * h - 0.2)
        src = rng.integers(0, 256, size=(h, w) if c == 1 and i % 2 else (h, w, c), dtype=np.uint8)
        cases.append(dict(model=model, params=params, src=src, pinhole=np.array([f, f, 0.5 * W, 0.5 * H]), out_w=W, out_h=H,
                          pad_src=(0, 1, 5)[i % 3], pad_dst=(0, 3, 4, 7)[i % 4]))
    return cases
