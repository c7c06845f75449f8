"""COLMAP sparse models (``<source>/sparse/0/{cameras,images,points3D}.{bin,txt}``) read into what the trainer needs:
cameras with their ground-truth images, the initial point cloud and the camera extent -- the upstream 3DGS scene reader's
conventions, written for this package (no plyfile / cv2: PLY through ply_io, images through PIL).

Conventions (the ones pegasus_amd.cameras.Camera uses):
  R = qvec2rotmat(qvec)^T   (camera-to-world rotation),   T = tvec   (world-to-camera translation)
  FoVx = focal2fov(fx, width), FoVy = focal2fov(fy, height)
Only PINHOLE and SIMPLE_PINHOLE cameras are supported: the rasterizer has no distortion model.  pegasus_amd.undistort turns
a project with distorted cameras into one of these; for it the readers take ``distorted=True`` (no model check) and carry the
2D observations and the tracks, which they skip otherwise."""
from __future__ import annotations

import os
import struct
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from .graphics import focal2fov, getWorld2View2
from .ply_io import read_ply_vertices, write_ply_vertices

# model id -> (name, number of parameters) of every COLMAP camera model (COLMAP src/colmap/sensor/models.h)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5),
                 4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5),
                 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
SUPPORTED_MODELS = ("PINHOLE", "SIMPLE_PINHOLE")
ONE_FOCAL_MODELS = ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")
TWO_FOCAL_MODELS = ("PINHOLE", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "FOV", "THIN_PRISM_FISHEYE")
LLFF_HOLD = 8                                   # eval: every 8th image (sorted by name) is a test camera


class UnsupportedCameraModel(ValueError):
    pass


@dataclass
class ColmapCamera:
    id: int
    model: str
    width: int
    height: int
    params: np.ndarray

    @property
    def focal(self):
        """(fx, fy)"""
        if self.model == "SIMPLE_PINHOLE":
            return float(self.params[0]), float(self.params[0])
        if self.model == "PINHOLE":
            return float(self.params[0]), float(self.params[1])
        raise UnsupportedCameraModel(f"COLMAP camera {self.id}: model {self.model} is not supported (only "
                                     f"{' / '.join(SUPPORTED_MODELS)}: undistort the images first)")

    @property
    def distorted_focal(self):
        """(fx, fy) of any model whose parameters start with one focal length (f, cx, cy, ...) or two (fx, fy, cx, cy, ...)"""
        if self.model in ONE_FOCAL_MODELS:
            return float(self.params[0]), float(self.params[0])
        if self.model in TWO_FOCAL_MODELS:
            return float(self.params[0]), float(self.params[1])
        raise UnsupportedCameraModel(f"COLMAP camera {self.id}: model {self.model} has no focal lengths this package knows")

    @property
    def principal_point(self):
        """(cx, cy) of the models ``distorted_focal`` knows"""
        first = 1 if self.model in ONE_FOCAL_MODELS else 2
        self.distorted_focal
        return float(self.params[first]), float(self.params[first + 1])


@dataclass
class ColmapImage:
    id: int
    qvec: np.ndarray                            # w, x, y, z (world-to-camera)
    tvec: np.ndarray
    camera_id: int
    name: str
    xys: np.ndarray = None                      # [n,2] float64 2D observations (readers: points2D=True)
    point3D_ids: np.ndarray = None              # [n] int64, -1 for an observation without a 3D point


def qvec2rotmat(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def rotmat2qvec(R):
    """Unit quaternion (w, x, y, z), w >= 0, of a rotation matrix (the inverse of qvec2rotmat)."""
    m = np.asarray(R, dtype=np.float64)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q = [0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = 2.0 * np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2])
        q = [(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
    elif m[1, 1] > m[2, 2]:
        s = 2.0 * np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2])
        q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1])
        q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s]
    q = np.asarray(q) / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def _check_model(cam: ColmapCamera) -> ColmapCamera:
    if cam.model not in SUPPORTED_MODELS:
        raise UnsupportedCameraModel(f"COLMAP camera {cam.id}: model {cam.model} is not supported (only "
                                     f"{' / '.join(SUPPORTED_MODELS)}: undistort the images first)")
    return cam


def _lines(path):
    for line in Path(path).read_text().splitlines():
        line = line.strip()
        if line and not line.startswith("#"):
            yield line


# ---- text -----------------------------------------------------------------------------------------------------------------
def read_cameras_text(path, distorted=False) -> dict:
    """``distorted``: any camera model is read (pegasus_amd.undistort); otherwise a distorted one raises."""
    cams = {}
    for line in _lines(path):
        tok = line.split()
        cam = ColmapCamera(int(tok[0]), tok[1], int(tok[2]), int(tok[3]), np.array([float(v) for v in tok[4:]]))
        cams[cam.id] = cam if distorted else _check_model(cam)
    return cams


def read_images_text(path, points2D=False) -> dict:
    """``points2D``: every image carries its observations (xys, point3D_ids)."""
    imgs = {}
    raw = [ln.strip() for ln in Path(path).read_text().splitlines() if not ln.strip().startswith("#")]
    # two lines per image: the pose line and the (possibly empty) 2D point line
    i = 0
    while i < len(raw):
        if not raw[i]:
            i += 1
            continue
        tok = raw[i].split()
        img = ColmapImage(int(tok[0]), np.array([float(v) for v in tok[1:5]]), np.array([float(v) for v in tok[5:8]]),
                          int(tok[8]), " ".join(tok[9:]))
        if points2D:
            obs = raw[i + 1].split() if i + 1 < len(raw) else []
            img.xys = np.array([float(v) for k, v in enumerate(obs) if k % 3 != 2], dtype=np.float64).reshape(-1, 2)
            img.point3D_ids = np.array([int(v) for v in obs[2::3]], dtype=np.int64)
        imgs[img.id] = img
        i += 2
    return imgs


def read_points3D_text(path, tracks=False):
    """(xyz [N,3] float64, rgb [N,3] uint8); with ``tracks`` also errors [N] float64, the tracks (a list of int32 [L,2]
    arrays of (image id, index of the 2D point)) and the point ids [N] int64."""
    xyz, rgb, err, trk, ids = [], [], [], [], []
    for line in _lines(path):
        tok = line.split()
        xyz.append([float(v) for v in tok[1:4]])
        rgb.append([int(v) for v in tok[4:7]])
        if tracks:
            ids.append(int(tok[0]))
            err.append(float(tok[7]))
            trk.append(np.array([int(v) for v in tok[8:]], dtype=np.int32).reshape(-1, 2))
    out = np.array(xyz, dtype=np.float64).reshape(-1, 3), np.array(rgb, dtype=np.uint8).reshape(-1, 3)
    return out + (np.array(err, dtype=np.float64), trk, np.array(ids, dtype=np.int64)) if tracks else out


# ---- binary (little endian) -----------------------------------------------------------------------------------------------
class _Reader:
    def __init__(self, path):
        self.data, self.off = Path(path).read_bytes(), 0

    def read(self, fmt):
        vals = struct.unpack_from("<" + fmt, self.data, self.off)
        self.off += struct.calcsize("<" + fmt)
        return vals

    def cstring(self):
        end = self.data.index(b"\x00", self.off)
        s = self.data[self.off:end].decode("utf-8")
        self.off = end + 1
        return s


def read_cameras_binary(path, distorted=False) -> dict:
    r, cams = _Reader(path), {}
    (n,) = r.read("Q")
    for _ in range(n):
        cam_id, model_id, w, h = r.read("iiQQ")
        if model_id not in CAMERA_MODELS:
            raise UnsupportedCameraModel(f"COLMAP camera {cam_id}: unknown model id {model_id}")
        name, n_params = CAMERA_MODELS[model_id]
        params = np.array(r.read("d" * n_params))
        cam = ColmapCamera(cam_id, name, int(w), int(h), params)
        cams[cam_id] = cam if distorted else _check_model(cam)
    return cams


def read_images_binary(path, points2D=False) -> dict:
    r, imgs = _Reader(path), {}
    (n,) = r.read("Q")
    for _ in range(n):
        vals = r.read("idddddddi")
        name = r.cstring()
        (n2d,) = r.read("Q")
        img = ColmapImage(vals[0], np.array(vals[1:5]), np.array(vals[5:8]), vals[8], name)
        if points2D:                             # (x, y, point3D_id) per 2D point, 24 bytes
            obs = np.frombuffer(r.data, dtype=np.dtype([("xy", "<f8", 2), ("id", "<i8")]), count=n2d, offset=r.off)
            img.xys, img.point3D_ids = obs["xy"].astype(np.float64), obs["id"].astype(np.int64)
        r.off += n2d * 24
        imgs[vals[0]] = img
    return imgs


def read_points3D_binary(path, tracks=False):
    """As read_points3D_text."""
    r = _Reader(path)
    (n,) = r.read("Q")
    xyz, rgb = np.empty((n, 3)), np.empty((n, 3), dtype=np.uint8)
    err, trk, ids = np.empty(n), [], np.empty(n, dtype=np.int64)
    for i in range(n):
        vals = r.read("QdddBBBd")
        xyz[i], rgb[i] = vals[1:4], vals[4:7]
        ids[i], err[i] = vals[0], vals[7]
        (track,) = r.read("Q")
        if tracks:
            trk.append(np.frombuffer(r.data, dtype="<i4", count=2 * track, offset=r.off).astype(np.int32).reshape(-1, 2))
        r.off += track * 8
    return (xyz, rgb, err, trk, ids) if tracks else (xyz, rgb)


# ---- writers (test fixtures, synthetic datasets) --------------------------------------------------------------------------
_MODEL_IDS = {name: mid for mid, (name, _) in CAMERA_MODELS.items()}


def write_colmap_model(sparse_dir, cameras, images, xyz, rgb, binary=True, errors=None, tracks=None, point_ids=None) -> None:
    """Writes cameras / images / points3D (.bin or .txt).  cameras: {id: ColmapCamera}; images: {id: ColmapImage};
    xyz [N,3], rgb [N,3] uint8.  An image that carries observations (xys, point3D_ids) has them written, one without has
    none; ``errors`` [N], ``tracks`` (a list of [L,2] (image id, 2D point index) arrays) and ``point_ids`` [N] are what
    read_points3D_*(tracks=True) returns and default to error 0, empty tracks and the ids 1..N."""
    d = Path(sparse_dir)
    d.mkdir(parents=True, exist_ok=True)
    n = len(xyz)
    errors = [0.0] * n if errors is None else [float(e) for e in errors]
    tracks = [np.zeros((0, 2), np.int32)] * n if tracks is None else [np.asarray(t, dtype=np.int32).reshape(-1, 2) for t in tracks]
    point_ids = list(range(1, n + 1)) if point_ids is None else [int(i) for i in point_ids]

    def observations(im):
        if im.xys is None:
            return np.zeros((0, 2)), np.zeros(0, np.int64)
        return np.asarray(im.xys, dtype=np.float64).reshape(-1, 2), np.asarray(im.point3D_ids, dtype=np.int64).reshape(-1)
    if binary:
        b = struct.pack("<Q", len(cameras))
        for c in cameras.values():
            b += struct.pack("<iiQQ", c.id, _MODEL_IDS[c.model], c.width, c.height)
            b += struct.pack("<" + "d" * len(c.params), *map(float, c.params))
        (d / "cameras.bin").write_bytes(b)
        b = struct.pack("<Q", len(images))
        for im in images.values():
            b += struct.pack("<idddddddi", im.id, *map(float, im.qvec), *map(float, im.tvec), im.camera_id)
            xys, ids = observations(im)
            obs = np.zeros(len(ids), dtype=np.dtype([("xy", "<f8", 2), ("id", "<i8")]))
            obs["xy"], obs["id"] = xys, ids
            b += im.name.encode("utf-8") + b"\x00" + struct.pack("<Q", len(ids)) + obs.tobytes()
        (d / "images.bin").write_bytes(b)
        b = struct.pack("<Q", len(xyz))
        for i, (p, c) in enumerate(zip(np.asarray(xyz, dtype=np.float64), np.asarray(rgb, dtype=np.uint8))):
            b += struct.pack("<QdddBBBdQ", point_ids[i], *map(float, p), *map(int, c), errors[i], len(tracks[i]))
            b += tracks[i].astype("<i4").tobytes()
        (d / "points3D.bin").write_bytes(b)
    else:
        (d / "cameras.txt").write_text("# Camera list\n" + "".join(
            f"{c.id} {c.model} {c.width} {c.height} {' '.join(repr(float(v)) for v in c.params)}\n"
            for c in cameras.values()))
        (d / "images.txt").write_text("# Image list\n" + "".join(
            f"{im.id} {' '.join(repr(float(v)) for v in im.qvec)} {' '.join(repr(float(v)) for v in im.tvec)} "
            f"{im.camera_id} {im.name}\n" + " ".join(f"{float(x)!r} {float(y)!r} {int(k)}" for (x, y), k in zip(*observations(im)))
            + "\n" for im in images.values()))
        (d / "points3D.txt").write_text("# 3D point list\n" + "".join(
            f"{point_ids[i]} {' '.join(repr(float(v)) for v in p)} {' '.join(str(int(v)) for v in c)} {errors[i]!r}"
            f"{''.join(f' {int(a)} {int(b)}' for a, b in tracks[i])}\n"
            for i, (p, c) in enumerate(zip(np.asarray(xyz, dtype=np.float64), np.asarray(rgb, dtype=np.uint8)))))


# ---- the scene ------------------------------------------------------------------------------------------------------------
def _sparse_dir(source_path) -> Path:
    d = Path(source_path) / "sparse" / "0"
    return d if d.is_dir() else Path(source_path) / "sparse"


def read_model(source_path, distorted=False, points2D=False):
    """(cameras, images) of ``source_path``'s sparse model, binary preferred.  ``distorted`` / ``points2D``: as the readers."""
    d = _sparse_dir(source_path)
    if (d / "images.bin").exists() and (d / "cameras.bin").exists():
        return read_cameras_binary(d / "cameras.bin", distorted), read_images_binary(d / "images.bin", points2D)
    if (d / "images.txt").exists() and (d / "cameras.txt").exists():
        return read_cameras_text(d / "cameras.txt", distorted), read_images_text(d / "images.txt", points2D)
    raise FileNotFoundError(f"no COLMAP model (cameras / images .bin or .txt) under {d}")


class PointCloud:
    def __init__(self, points, colors):
        self.points, self.colors = np.asarray(points, dtype=np.float32), np.asarray(colors, dtype=np.float32)


def fetch_point_cloud(source_path) -> PointCloud:
    """The initial point cloud, cached as ``sparse/0/points3D.ply`` (x, y, z, normals, red / green / blue in 0..255)."""
    d = _sparse_dir(source_path)
    ply = d / "points3D.ply"
    if not ply.exists():
        if (d / "points3D.bin").exists():
            xyz, rgb = read_points3D_binary(d / "points3D.bin")
        elif (d / "points3D.txt").exists():
            xyz, rgb = read_points3D_text(d / "points3D.txt")
        else:
            raise FileNotFoundError(f"no points3D.bin / .txt / .ply under {d}")
        store_ply(ply, xyz, rgb)
    return read_point_cloud_ply(ply)


def store_ply(path, xyz, rgb) -> None:
    xyz = np.asarray(xyz, dtype=np.float64)
    rgb = np.asarray(rgb)
    write_ply_vertices(path, {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "nx": np.zeros(len(xyz)),
                              "ny": np.zeros(len(xyz)), "nz": np.zeros(len(xyz)), "red": rgb[:, 0],
                              "green": rgb[:, 1], "blue": rgb[:, 2]})


def read_point_cloud_ply(path) -> PointCloud:
    v = read_ply_vertices(path)
    pts = np.stack([v["x"], v["y"], v["z"]], axis=1)
    cols = np.stack([v["red"], v["green"], v["blue"]], axis=1).astype(np.float32) / 255.0
    return PointCloud(pts, cols)


@dataclass
class CameraInfo:
    uid: int
    R: np.ndarray
    T: np.ndarray
    FoVx: float
    FoVy: float
    image_path: str
    image_name: str
    width: int
    height: int


def camera_infos(source_path, images_dir="images") -> list:
    """One CameraInfo per registered image, sorted by image name."""
    cams, imgs = read_model(source_path)
    out = []
    for im in imgs.values():
        cam = cams[im.camera_id]
        fx, fy = cam.focal
        out.append(CameraInfo(uid=im.id, R=np.transpose(qvec2rotmat(im.qvec)), T=np.asarray(im.tvec, dtype=np.float64),
                              FoVx=focal2fov(fx, cam.width), FoVy=focal2fov(fy, cam.height),
                              image_path=os.path.join(source_path, images_dir, im.name),
                              image_name=os.path.splitext(os.path.basename(im.name))[0], width=cam.width,
                              height=cam.height))
    return sorted(out, key=lambda c: c.image_name)


def split_train_test(infos, eval_split: bool):
    if not eval_split:
        return list(infos), []
    return ([c for i, c in enumerate(infos) if i % LLFF_HOLD != 0], [c for i, c in enumerate(infos) if i % LLFF_HOLD == 0])


def camera_extent(infos) -> float:
    """1.1 x the largest distance of a camera centre from the mean centre (upstream getNerfppNorm's radius)."""
    centres = np.stack([np.linalg.inv(getWorld2View2(c.R, c.T))[:3, 3] for c in infos])
    return float(1.1 * np.linalg.norm(centres - centres.mean(0), axis=1).max())


def _target_size(w, h, resolution, scale=1.0):
    if resolution in (1, 2, 4, 8):
        return round(w / (scale * resolution)), round(h / (scale * resolution))
    if resolution == -1:
        f = w / 1600 if w > 1600 else 1.0               # large images come down to 1600 pixels across
    else:
        f = w / resolution
    f *= scale
    return int(w / f), int(h / f)


MASK_EXTENSIONS = (".png", ".jpg", ".jpeg", ".PNG", ".JPG", ".JPEG")


def mask_path(masks_dir, image_name: str) -> str:
    """The mask file of an image in a mask directory: the file with the image's stem and a png or jpg extension (the
    layout of PEGASUS's object reconstruction: one mask per image, named like it).  Raises FileNotFoundError naming the
    image when there is none."""
    stem = os.path.splitext(os.path.basename(image_name))[0]
    for ext in MASK_EXTENSIONS:
        p = os.path.join(masks_dir, stem + ext)
        if os.path.isfile(p):
            return p
    raise FileNotFoundError(f"no mask for image {image_name!r} in {masks_dir} (looked for {stem}.png / {stem}.jpg)")


def load_mask(path, size) -> np.ndarray:
    """A mask file as float32 [H,W] in 0..1: greyscale / 255, resized (bilinear) to ``size`` = (W, H)."""
    from PIL import Image
    with Image.open(path) as m:
        m = m.convert("L")
        if m.size != tuple(size):
            m = m.resize(tuple(size), Image.BILINEAR)
        return np.clip(np.asarray(m, dtype=np.float32) / 255.0, 0.0, 1.0)


def load_camera(info: CameraInfo, resolution=-1, white_background=False, data_device="cuda", masks=""):
    """Camera with its ground-truth image ([3,H,W] in 0..1, resized per ``resolution``; an alpha channel composites the
    image over the training background: white with ``white_background``, else black).

    ``masks``: a per-image object mask for alpha supervision, kept as ``camera.gt_mask`` [1,H,W].  A directory (the mask
    of each image is the file with its stem, png or jpg, read as greyscale / 255, resized bilinearly to the image's training
    size), or ``"alpha"`` (the image's own alpha channel).  With masks the RGB is NOT composited: the trainer composites the
    target over each step's background.  An image without a mask raises an error that names it.  ``""``: no masks."""
    import torch
    from PIL import Image

    from .cameras import Camera
    with Image.open(info.image_path) as im:
        im = im.convert("RGBA") if im.mode in ("RGBA", "LA", "P") else im.convert("RGB")
        size = _target_size(im.width, im.height, resolution)
        if size != (im.width, im.height):
            im = im.resize(size, Image.BICUBIC)
        a = np.asarray(im, dtype=np.float32) / 255.0
    rgb = a[..., :3]
    mask = None
    if masks == "alpha":
        if a.shape[-1] != 4:
            raise ValueError(f"masks='alpha' but image {info.image_name!r} ({info.image_path}) has no alpha channel")
        mask = np.clip(a[..., 3], 0.0, 1.0)
    elif masks:
        mask = load_mask(mask_path(masks, info.image_name), size)
    elif a.shape[-1] == 4:
        bg = 1.0 if white_background else 0.0
        rgb = rgb * a[..., 3:4] + bg * (1.0 - a[..., 3:4])
    image = torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1)))
    gt_mask = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask))[None]
    return Camera(colmap_id=info.uid, R=info.R, T=info.T, FoVx=info.FoVx, FoVy=info.FoVy, image=image, gt_alpha_mask=None,
                  image_name=info.image_name, uid=info.uid, data_device=data_device, gt_mask=gt_mask)
