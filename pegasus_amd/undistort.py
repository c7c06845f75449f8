"""Undistortion of a COLMAP project on the device (csrc/undistort.hip.h): what ``colmap
image_undistorter`` does between a raw COLMAP run and the trainer, with this package alone.

    python -m pegasus_amd.undistort -s <src>            # <src>/input + <src>/distorted/sparse/0 -> <src>/images + <src>/sparse/0

The cameras of the project (SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV, OPENCV_FISHEYE; the pinhole models pass through) become
PINHOLE cameras whose principal point is the image centre by default (``principal_point="center"``: what
pegasus_amd.cameras.Camera assumes), the images and masks are resampled to them, the 2D observations are moved and the 3D points
are copied.  The arithmetic is float64 on the device and is pinned against a NumPy restatement; parity with COLMAP's own files
is not pinned (COLMAP does not run here).  There is no CPU path: the ``backend`` argument of ``undistort_camera`` and
``undistort_project`` exists for the tests, which put their reference in the device's place.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import shutil
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from . import colmap_io
from .colmap_io import ColmapCamera, UnsupportedCameraModel

MODEL_IDS = {name: mid for mid, (name, _) in colmap_io.CAMERA_MODELS.items()}
MODELS = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV")
PYRAMID = (2, 4, 8)
MAX_WORKERS = 16


def _check_model(camera: ColmapCamera) -> ColmapCamera:
    if camera.model not in MODELS:
        raise UnsupportedCameraModel(f"COLMAP camera {camera.id}: model {camera.model} cannot be undistorted here "
                                     f"(only {' / '.join(MODELS)})")
    n = colmap_io.CAMERA_MODELS[MODEL_IDS[camera.model]][1]
    if len(camera.params) != n:
        raise ValueError(f"COLMAP camera {camera.id}: model {camera.model} has {n} parameters, not {len(camera.params)}")
    return camera


def _params(camera: ColmapCamera):
    p = (C.c_double * 12)()
    for i, v in enumerate(_check_model(camera).params):
        p[i] = float(v)
    return MODEL_IDS[camera.model], p


# ---- the device calls -----------------------------------------------------------------------------------------------------
def _points(x):
    import torch
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64))
    if t.device.type != "cuda":
        t = t.cuda()
    t = t.to(torch.float64).reshape(-1, 2).contiguous()
    return t


def distort(camera: ColmapCamera, uv):
    """Normalised points [n,2] -> image points [n,2] of ``camera`` (float64 device tensor; pgr_distort_points)."""
    import torch

    from . import _lib
    uv = _points(uv)
    xy = torch.empty_like(uv)
    model, p = _params(camera)
    _lib.call("pgr_distort_points", uv.device, model, p, uv.shape[0], _lib.ptr(uv), _lib.ptr(xy))
    return xy


def undistort_points(camera: ColmapCamera, xy):
    """Image points [n,2] of ``camera`` -> (normalised points [n,2] float64, ok [n] uint8), device tensors
    (pgr_undistort_points).  A point the Newton inverse does not reach is NaN with ok 0."""
    import torch

    from . import _lib
    xy = _points(xy)
    uv = torch.empty_like(xy)
    ok = torch.empty(xy.shape[0], dtype=torch.uint8, device=xy.device)
    model, p = _params(camera)
    _lib.call("pgr_undistort_points", xy.device, model, p, xy.shape[0], _lib.ptr(xy), _lib.ptr(uv), _lib.ptr(ok))
    return uv, ok


def _image_geometry(t):
    """(height, width, channels, row stride in bytes) of a uint8 image tensor read where it lies"""
    import torch
    if t.device.type != "cuda" or t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise ValueError("undistort takes uint8 [H,W] or [H,W,C] tensors on the HIP device (there is no CPU path), "
                         f"not {t.dtype} {tuple(t.shape)} on {t.device}")
    h, w = int(t.shape[0]), int(t.shape[1])
    c = 1 if t.dim() == 2 else int(t.shape[2])
    if c not in (1, 3, 4) or h < 1 or w < 1:
        raise ValueError(f"an image has 1, 3 or 4 channels and at least one pixel, not {tuple(t.shape)}")
    if (t.dim() == 3 and c > 1 and t.stride(2) != 1) or (w > 1 and t.stride(1) != c):
        raise ValueError("the channels of a pixel and the pixels of a row must be adjacent bytes (only the row stride is free)")
    stride = int(t.stride(0)) if h > 1 else w * c
    if stride < w * c:
        raise ValueError("the rows of an image must not overlap")
    return h, w, c, stride


def _job(src, dst):
    from . import _lib
    sh, sw, sc, ss = _image_geometry(src)
    dh, dw, dc, ds = _image_geometry(dst)
    if sc != dc:
        raise ValueError(f"source has {sc} channels, destination {dc}")
    return _lib.PgrUndistortJob(src=src.data_ptr(), src_width=sw, src_height=sh, channels=sc, src_stride=ss, dst=dst.data_ptr(),
                                dst_width=dw, dst_height=dh, dst_stride=ds)


def _new_like(src, height, width):
    import torch
    return torch.empty((height, width) + tuple(src.shape[2:]), dtype=torch.uint8, device=src.device)


def undistort_images(images, cameras, out_cameras, out=None):
    """``images``: uint8 device tensors [H,W] or [H,W,C] (C = 1, 3, 4), each of its camera's size; views are read where they
    lie when only the row stride differs from a packed image.  ``cameras`` / ``out_cameras``: one ColmapCamera per image (or
    one for all); the output cameras are PINHOLE (undistort_camera).  Returns one new tensor per image of its output camera's
    size (or fills ``out``, tensors or row-strided views of that size).  One call of pgr_undistort_images."""
    from . import _lib
    images = list(images)
    n = len(images)
    cameras = [cameras] * n if isinstance(cameras, ColmapCamera) else list(cameras)
    out_cameras = [out_cameras] * n if isinstance(out_cameras, ColmapCamera) else list(out_cameras)
    if len(cameras) != n or len(out_cameras) != n:
        raise ValueError(f"{len(cameras)} cameras and {len(out_cameras)} output cameras for {n} images")
    if n == 0:
        return []
    device = images[0].device
    outs = [_new_like(im, o.height, o.width) for im, o in zip(images, out_cameras)] if out is None else list(out)
    jobs = (_lib.PgrUndistortJob * n)()
    for k, (im, cam, ocam, dst) in enumerate(zip(images, cameras, out_cameras, outs)):
        if im.device != device or dst.device != device:
            raise ValueError("the images of one batch lie on one device")
        if ocam.model != "PINHOLE":
            raise ValueError(f"the output camera of image {k} is {ocam.model}, not PINHOLE")
        j = _job(im, dst)
        if (j.src_width, j.src_height) != (cam.width, cam.height) or (j.dst_width, j.dst_height) != (ocam.width, ocam.height):
            raise ValueError(f"image {k}: {j.src_width} x {j.src_height} -> {j.dst_width} x {j.dst_height} but its cameras "
                             f"say {cam.width} x {cam.height} -> {ocam.width} x {ocam.height}")
        j.model, j.params = _params(cam)
        j.pinhole = (C.c_double * 4)(*[float(v) for v in ocam.params])
        jobs[k] = j
    _lib.call("pgr_undistort_images", device, jobs, n)
    return outs


def box_downscale(images, factor: int):
    """f x f integer box means, (sum + f f / 2) // (f f) per channel, f = 2, 4 or 8: one new [H // f, W // f(, C)] tensor per
    image (pgr_image_box_downscale)."""
    from . import _lib
    images = list(images)
    if factor not in PYRAMID:
        raise ValueError(f"factor is one of {PYRAMID}, not {factor}")
    if not images:
        return []
    device = images[0].device
    outs = []
    for im in images:
        if im.shape[0] < factor or im.shape[1] < factor:
            raise ValueError(f"an image of {im.shape[1]} x {im.shape[0]} pixels has no {factor} x {factor} box")
        outs.append(_new_like(im, int(im.shape[0]) // factor, int(im.shape[1]) // factor))
    jobs = (_lib.PgrUndistortJob * len(images))(*[_job(im, o) for im, o in zip(images, outs)])
    _lib.call("pgr_image_box_downscale", device, jobs, len(images), int(factor))
    return outs


class _Device:
    """The device behind undistort_camera / undistort_project; the tests' reference has the same methods."""
    device_png = True

    def undistort_points(self, camera, xy):
        uv, ok = undistort_points(camera, xy)
        return uv.cpu().numpy(), ok.cpu().numpy()

    def upload(self, image):
        import torch
        return torch.from_numpy(np.array(image, dtype=np.uint8)).cuda()      # (a copy: PIL's arrays are read-only)

    def download(self, image):
        return image.cpu().numpy()

    undistort_images = staticmethod(undistort_images)
    box_downscale = staticmethod(box_downscale)


# ---- the undistorted camera -----------------------------------------------------------------------------------------------
def _border(w, h):
    """The border samples and the sides each belongs to: image points [n,2], and index arrays left, right, top, bottom"""
    ys, xs = np.arange(h, dtype=np.float64) + 0.5, np.arange(w, dtype=np.float64) + 0.5
    pts = np.concatenate([np.stack([np.zeros(h), ys], 1), np.stack([np.full(h, float(w)), ys], 1),
                          np.stack([xs, np.zeros(w)], 1), np.stack([xs, np.full(w, float(h))], 1),
                          np.array([[0.0, 0.0], [w, 0.0], [0.0, h], [w, h]], dtype=np.float64)])
    c = 2 * h + 2 * w                                    # the corners: (0,0) (w,0) (0,h) (w,h)
    left = np.r_[np.arange(0, h), c, c + 2]
    right = np.r_[np.arange(h, 2 * h), c + 1, c + 3]
    top = np.r_[np.arange(2 * h, 2 * h + w), c, c + 1]
    bottom = np.r_[np.arange(2 * h + w, c), c + 2, c + 3]
    return pts, left, right, top, bottom


def _axis_scale(c, size, lo, hi, blank_pixels, min_scale, max_scale):
    """scale of one axis from the undistorted extremes of its two borders: lo = (min, max) of the near one, hi of the far"""
    with np.errstate(all="ignore"):
        s_min = min(np.float64(c) / (c - lo[0]), np.float64(size - c) / (hi[1] - c))
        s_max = max(np.float64(c) / (c - lo[1]), np.float64(size - c) / (hi[0] - c))
        scale = np.float64(1.0) / (s_min * blank_pixels + s_max * (1.0 - blank_pixels))
    if not np.isfinite(scale):
        scale = max_scale if scale > 0 else min_scale
    return float(min(max(scale, min_scale), max_scale))


def undistort_camera(camera: ColmapCamera, blank_pixels=0.0, min_scale=0.2, max_scale=2.0, max_image_size=-1,
                     principal_point="center", multiple_of=1, *, backend=None) -> ColmapCamera:
    """The PINHOLE camera that ``camera``'s images are undistorted to: the source's focal lengths, a
    size that shows all of the source and nothing else (``blank_pixels=0``), all of the source and blank corners (1) or between,
    and the principal point at the centre (``"center"``) or where the source has it (``"keep"``).  ``multiple_of``: the size is
    cut to a multiple (right and bottom in ``keep`` mode).  Raises ValueError naming the camera when its distortion cannot be
    inverted all along the image border."""
    if principal_point not in ("center", "keep"):
        raise ValueError(f"principal_point is 'center' or 'keep', not {principal_point!r}")
    if not 0.0 <= blank_pixels <= 1.0 or not 0.0 < min_scale <= max_scale or multiple_of < 1:
        raise ValueError("blank_pixels lies in 0..1, 0 < min_scale <= max_scale, multiple_of >= 1")
    _check_model(camera)
    backend = backend or _Device()
    w, h = int(camera.width), int(camera.height)
    fx, fy = camera.distorted_focal
    cxs, cys = camera.principal_point
    cx, cy = (cxs, cys) if principal_point == "keep" else (w / 2.0, h / 2.0)
    pts, left, right, top, bottom = _border(w, h)
    uv, ok = backend.undistort_points(camera, pts)
    uv, ok = np.asarray(uv, dtype=np.float64), np.asarray(ok)
    if not ok.all():
        bad = pts[np.flatnonzero(ok == 0)[0]]
        raise ValueError(f"COLMAP camera {camera.id} ({camera.model}): the distortion is not invertible over the image: the "
                         f"border point ({bad[0]:g}, {bad[1]:g}) has no undistorted position")
    # the working pinhole's projection fx u + cx, written so that a point the distortion leaves alone keeps its coordinates
    # exactly: X + fx (u - x_d) + (cx - cx_source), x_d = (X - cx_source) / fx
    px = pts[:, 0] + fx * (uv[:, 0] - (pts[:, 0] - cxs) / fx) + (cx - cxs)
    py = pts[:, 1] + fy * (uv[:, 1] - (pts[:, 1] - cys) / fy) + (cy - cys)
    scale_x = _axis_scale(cx, w, (px[left].min(), px[left].max()), (px[right].min(), px[right].max()), blank_pixels, min_scale,
                          max_scale)
    scale_y = _axis_scale(cy, h, (py[top].min(), py[top].max()), (py[bottom].min(), py[bottom].max()), blank_pixels, min_scale,
                          max_scale)
    W, H = max(1, math.floor(scale_x * w)), max(1, math.floor(scale_y * h))
    fxo, fyo = fx, fy
    if max_image_size > 0 and max(W, H) > max_image_size:
        s = max_image_size / max(W, H)
        W2, H2 = max(1, math.floor(W * s)), max(1, math.floor(H * s))
        fxo, fyo = fx * (W2 / W), fy * (H2 / H)
        W, H = W2, H2
    # cx W / w: the source's own value where the size did not change (cx w / w need not round back to cx)
    cxo, cyo = cx if W == w else cx * W / w, cy if H == h else cy * H / h
    if multiple_of > 1:
        if W < multiple_of or H < multiple_of:
            raise ValueError(f"COLMAP camera {camera.id}: an undistorted size of {W} x {H} has no multiple of {multiple_of}")
        W, H = W - W % multiple_of, H - H % multiple_of
    if principal_point == "center":
        cxo, cyo = W / 2.0, H / 2.0                      # (w / 2) W / w, without its rounding
    return ColmapCamera(camera.id, "PINHOLE", W, H, np.array([fxo, fyo, cxo, cyo], dtype=np.float64))


def undistort_observations(camera: ColmapCamera, out_camera: ColmapCamera, xys, point3D_ids, *, backend=None):
    """The 2D observations of ``camera``'s images in ``out_camera``: (xys [n,2], point3D_ids [n]).  A point the inverse does not
    reach keeps its place with NaN coordinates and id -1."""
    backend = backend or _Device()
    xys = np.asarray(xys, dtype=np.float64).reshape(-1, 2)
    ids = np.asarray(point3D_ids, dtype=np.int64).reshape(-1).copy()
    if len(xys) == 0:
        return xys.copy(), ids
    uv, ok = backend.undistort_points(camera, xys)
    uv, ok = np.asarray(uv, dtype=np.float64), np.asarray(ok).astype(bool)
    fx, fy, cx, cy = (float(v) for v in out_camera.params)
    out = np.stack([fx * uv[:, 0] + cx, fy * uv[:, 1] + cy], axis=1)
    out[~ok] = np.nan
    ids[~ok] = -1
    return out, ids


# ---- the whole job --------------------------------------------------------------------------------------------------------
def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGBA" if im.mode in ("LA", "PA") or "transparency" in im.info else "RGB")
        return np.asarray(im, dtype=np.uint8)


def _encode(path, array):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    if path.suffix.lower() in (".jpg", ".jpeg"):
        Image.fromarray(array).save(path, quality=95)
    else:
        Image.fromarray(array).save(path)


def _write_batch(pool, backend, png, jpeg, paths, images):
    """The files of a batch of images that lie with the backend: PNG and JPEG on the device where asked and possible, else on the
    host"""
    # pegasus_amd.png and pegasus_amd.jpeg write gray and RGB; the rest (RGBA, other formats) goes to the host
    encoders = {".png": "png" if png == "gpu" and backend.device_png else None}
    encoders[".jpg"] = encoders[".jpeg"] = "jpeg" if jpeg == "gpu" and backend.device_png else None
    on_device = [(e := encoders.get(p.suffix.lower())) and (im.dim() == 2 or im.shape[2] == 3) and e for p, im in zip(paths, images)]
    for name in ("png", "jpeg"):
        pick = [k for k, d in enumerate(on_device) if d == name]
        if not pick:
            continue
        if name == "png":
            from . import png as device_png
            files = device_png.encode_batch_bytes([images[k] for k in pick])
        else:
            from . import jpeg as device_jpeg                    # quality 95 at 4:2:0: what _encode asks of PIL
            files = device_jpeg.encode_batch_bytes([images[k] for k in pick], quality=95, subsampling="4:2:0")
        for k, data in zip(pick, files):
            paths[k].parent.mkdir(parents=True, exist_ok=True)
            paths[k].write_bytes(data)
    rest = [k for k, d in enumerate(on_device) if not d]
    arrays = [backend.download(images[k]) for k in rest]
    list(pool.map(_encode, [paths[k] for k in rest], arrays))


def undistort_project(image_path, input_path, output_path, *, blank_pixels=0.0, min_scale=0.2, max_scale=2.0, max_image_size=-1,
                      principal_point="center", masks=None, resize=False, png="host", jpeg="host", batch=8, backend=None) -> dict:
    """Undistorts the COLMAP project ``input_path`` (a sparse model, .bin or .txt) with images under ``image_path`` into
    ``output_path``: ``images/<same name>`` (PNG through the host or, ``png="gpu"``, pegasus_amd.png; JPEG through PIL at quality
    95 or, ``jpeg="gpu"``, gray and RGB ones through pegasus_amd.jpeg at quality 95, 4:2:0 -- PIL's default), ``sparse/0`` in the input's format (PINHOLE cameras, moved 2D observations, points3D copied verbatim),
    ``masks/<mask file>`` of each image with ``masks=<dir>``, the pyramid ``images_2``, ``images_4``, ``images_8`` with
    ``resize`` (box means; the undistorted size is then a multiple of 8, so the fields of view hold at every level) and
    ``undistort.json`` (the options and both cameras per camera id).  Returns the seconds spent decoding, on the device and
    encoding, and the output cameras."""
    if png not in ("host", "gpu"):
        raise ValueError(f"png is 'host' or 'gpu', not {png!r}")
    if jpeg not in ("host", "gpu"):
        raise ValueError(f"jpeg is 'host' or 'gpu', not {jpeg!r}")
    backend = backend or _Device()
    image_path, input_path, output_path = Path(image_path), Path(input_path), Path(output_path)
    binary = (input_path / "cameras.bin").exists() and (input_path / "images.bin").exists()
    ext = ".bin" if binary else ".txt"
    if not binary and not ((input_path / "cameras.txt").exists() and (input_path / "images.txt").exists()):
        raise FileNotFoundError(f"no COLMAP model (cameras / images .bin or .txt) under {input_path}")
    if not (input_path / f"points3D{ext}").exists():
        raise FileNotFoundError(f"no points3D{ext} under {input_path}")
    read_cameras = colmap_io.read_cameras_binary if binary else colmap_io.read_cameras_text
    read_images = colmap_io.read_images_binary if binary else colmap_io.read_images_text
    cameras = read_cameras(input_path / f"cameras{ext}", distorted=True)
    images = read_images(input_path / f"images{ext}", points2D=True)
    options = dict(blank_pixels=blank_pixels, min_scale=min_scale, max_scale=max_scale, max_image_size=max_image_size,
                   principal_point=principal_point, multiple_of=8 if resize else 1)
    t0 = time.perf_counter()
    out_cameras = {cid: undistort_camera(cam, backend=backend, **options) for cid, cam in cameras.items()}
    # the observations: one call per camera
    for cid, cam in cameras.items():
        mine = [im for im in images.values() if im.camera_id == cid and im.xys is not None and len(im.xys)]
        if not mine:
            continue
        xys, ids = undistort_observations(cam, out_cameras[cid], np.concatenate([im.xys for im in mine]),
                                          np.concatenate([im.point3D_ids for im in mine]), backend=backend)
        first = 0
        for im in mine:
            n = len(im.xys)
            im.xys, im.point3D_ids = xys[first:first + n], ids[first:first + n]
            first += n
    seconds = dict(decode=0.0, device=time.perf_counter() - t0, encode=0.0)
    sparse = output_path / "sparse" / "0"
    colmap_io.write_colmap_model(sparse, out_cameras, images, np.zeros((0, 3)), np.zeros((0, 3), np.uint8), binary=binary)
    shutil.copyfile(input_path / f"points3D{ext}", sparse / f"points3D{ext}")

    # the images (and masks), a batch at a time: decode on a thread pool, remap in one call, encode
    work = []                                                    # (source file, camera id, destination relative to output_path)
    for im in sorted(images.values(), key=lambda i: i.name):
        work.append((image_path / im.name, im.camera_id, Path("images") / im.name))
        if masks:
            m = Path(colmap_io.mask_path(str(masks), im.name))
            work.append((m, im.camera_id, Path("masks") / m.name))
    with ThreadPoolExecutor(max_workers=min(MAX_WORKERS, os.cpu_count() or 1)) as pool:
        for first in range(0, len(work), max(1, int(batch))):
            chunk = work[first:first + max(1, int(batch))]
            t0 = time.perf_counter()
            arrays = list(pool.map(_decode, [c[0] for c in chunk]))
            t1 = time.perf_counter()
            for (src, cid, _), a in zip(chunk, arrays):
                if (a.shape[1], a.shape[0]) != (cameras[cid].width, cameras[cid].height):
                    raise ValueError(f"{src}: {a.shape[1]} x {a.shape[0]} pixels, but camera {cid} has "
                                     f"{cameras[cid].width} x {cameras[cid].height}")
            dev = [backend.upload(a) for a in arrays]
            outs = backend.undistort_images(dev, [cameras[c[1]] for c in chunk], [out_cameras[c[1]] for c in chunk])
            levels = {1: outs}
            if resize:
                for f in PYRAMID:
                    levels[f] = backend.box_downscale(outs, f)
            if backend.device_png:
                import torch
                torch.cuda.synchronize()
            t2 = time.perf_counter()
            for f, level in levels.items():
                paths = [output_path / (c[2] if f == 1 else Path(f"{c[2].parts[0]}_{f}", *c[2].parts[1:])) for c in chunk]
                _write_batch(pool, backend, png, jpeg, paths, level)
            t3 = time.perf_counter()
            seconds["decode"] += t1 - t0
            seconds["device"] += t2 - t1
            seconds["encode"] += t3 - t2

    def as_json(c):
        return dict(model=c.model, width=int(c.width), height=int(c.height), params=[float(v) for v in c.params])
    output_path.mkdir(parents=True, exist_ok=True)
    (output_path / "undistort.json").write_text(json.dumps(dict(
        options=dict(options, masks=str(masks) if masks else None, resize=bool(resize), png=png, jpeg=jpeg),
        cameras={str(cid): dict(source=as_json(cameras[cid]), undistorted=as_json(out_cameras[cid])) for cid in cameras}),
        indent=1) + "\n")
    return dict(seconds=seconds, cameras=out_cameras, n_images=len(images))


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m pegasus_amd.undistort", description=__doc__.split("\n\n")[0])
    ap.add_argument("-s", "--source_path", help="<src>/input and <src>/distorted/sparse/0 -> <src>/images and <src>/sparse/0")
    ap.add_argument("--image_path")
    ap.add_argument("--input_path")
    ap.add_argument("--output_path")
    ap.add_argument("--principal_point", choices=("center", "keep"), default="center")
    ap.add_argument("--blank_pixels", type=float, default=0.0)
    ap.add_argument("--min_scale", type=float, default=0.2)
    ap.add_argument("--max_scale", type=float, default=2.0)
    ap.add_argument("--max_image_size", type=int, default=-1)
    ap.add_argument("--resize", action="store_true", help="also write images_2, images_4, images_8")
    ap.add_argument("--masks", default=None, help="a directory with one mask per image, undistorted into <out>/masks")
    ap.add_argument("--png", choices=("host", "gpu"), default="host")
    ap.add_argument("--jpeg", choices=("host", "gpu"), default="host",
                    help="where gray and RGB JPEG files are encoded: PIL on the host, or pegasus_amd.jpeg on the GPU")
    args = ap.parse_args(argv)
    if args.source_path:
        src = Path(args.source_path)
        image_path, input_path, output_path = src / "input", src / "distorted" / "sparse" / "0", src
    elif args.image_path and args.input_path and args.output_path:
        image_path, input_path, output_path = args.image_path, args.input_path, args.output_path
    else:
        ap.error("give -s <src>, or --image_path, --input_path and --output_path")
    t0 = time.perf_counter()
    res = undistort_project(image_path, input_path, output_path, blank_pixels=args.blank_pixels, min_scale=args.min_scale,
                            max_scale=args.max_scale, max_image_size=args.max_image_size, principal_point=args.principal_point,
                            masks=args.masks, resize=args.resize, png=args.png, jpeg=args.jpeg)
    s = res["seconds"]
    print(f"undistorted {res['n_images']} images in {time.perf_counter() - t0:.2f} s (decode {s['decode']:.2f} s, device "
          f"{s['device']:.2f} s, encode {s['encode']:.2f} s) -> {output_path}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
