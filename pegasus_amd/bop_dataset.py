"""A BOP dataset and a BOP models directory on disk: the one place that knows their layout.  Host only.

Layout and naming follow the reference's writer (src/visualization/object_visualization.py:373-391, 458-480;
pegasus.py:347-358, 491) and the toolkit's docs/bop_datasets_format.md:

    <dataset>/<split>/<scene:06d>/rgb/<frame:06d>.png                8-bit RGB,  (img * 255).astype(uint8)
    <dataset>/<split>/<scene:06d>/depth/<frame:06d>.png              16-bit grey, (depth * 1000).astype(uint16): millimetres
    <dataset>/<split>/<scene:06d>/mask_visib/<frame:06d>_<k:06d>.png 8-bit 0/255, visible mask of scene_gt's k-th entry;
                                                                     mask/ likewise: its silhouette
    <dataset>/<split>/<scene:06d>/sem_mask/<frame:06d>.png           8-bit RGB, uint8 of the semantic image
    <dataset>/<split>/<scene:06d>/scene_gt.json, scene_camera.json   {frame: ...}, the records of pegasus_amd.bop_pose
    <dataset>/<split>/<scene:06d>/scene_gt_info.json                 {frame: [per entry: pixel counts, visib_fract, boxes]}, optional
    <dataset>/<split>/<scene:06d>/scene_gt_coco[_modal].json         COCO annotations (pegasus_amd.coco.coco_file_name)
    <models>/obj_<id:06d>.ply, <models>/models_info.json             meshes in millimetres; {id: diameter, box, symmetries}

The record files are compact ``json.dumps`` without a trailing newline, their frames ordered by number.  The reference
encodes PNGs with imageio; PNG is deflate + CRC, so zlib is all it takes.
"""
from __future__ import annotations

import json
import re
import struct
import zlib
from functools import cached_property
from pathlib import Path

import numpy as np

SCENE_GT, SCENE_CAMERA, SCENE_GT_INFO, MODELS_INFO = "scene_gt.json", "scene_camera.json", "scene_gt_info.json", "models_info.json"
IMAGE_KINDS = ("rgb", "depth", "mask_visib", "mask", "sem_mask")
JPEG_EXTENSIONS = (".jpg", ".jpeg")


# ---- names and discovery ----------------------------------------------------------------------------------------------
def image_name(i, k=None, ext: str = "png") -> str:
    """The PNG of frame ``i``; with ``k`` the mask of its k-th entry.  ``ext``: "jpg" for the colour image of a JPEG scene."""
    return f"{int(i):06d}.{ext}" if k is None else f"{int(i):06d}_{int(k):06d}.{ext}"


def scene_name(scene_id) -> str:
    return f"{int(scene_id):06d}"


def model_stem(obj_id) -> str:
    return f"obj_{int(obj_id):06d}"


def scene_dir(dataset_dir, split: str, scene_id) -> Path:
    return Path(dataset_dir) / split / scene_name(scene_id)


def scene_dirs(dataset_dir, split: str = "train", having: str = SCENE_GT) -> list:
    """The directories under <dataset>/<split> that hold the file ``having``, sorted; whatever their names."""
    return sorted(p for p in (Path(dataset_dir) / split).iterdir() if (p / having).exists())


def by_frame(records: dict) -> dict:
    """``records`` with its keys in the order of their numbers ("9" before "10"): how the record files are written."""
    return {k: records[k] for k in sorted(records, key=int)}


# ---- one scene --------------------------------------------------------------------------------------------------------
class BopScene:
    """The files of one scene directory; the record files are read once, when first asked for."""

    def __init__(self, path):
        self.path = Path(path)

    def read_json(self, name: str):
        return json.loads((self.path / name).read_text())

    def write_json(self, name: str, doc) -> None:
        (self.path / name).write_text(json.dumps(doc))

    @cached_property
    def gt(self) -> dict:
        return self.read_json(SCENE_GT)

    @cached_property
    def camera(self) -> dict:
        return self.read_json(SCENE_CAMERA)

    @cached_property
    def gt_info(self):
        """None when the scene has no scene_gt_info.json."""
        return self.read_json(SCENE_GT_INFO) if (self.path / SCENE_GT_INFO).exists() else None

    @property
    def image_ids(self) -> list:
        """scene_gt's keys (strings) in the order of their numbers."""
        return sorted(self.gt, key=int)

    def make_dirs(self, kinds=IMAGE_KINDS) -> None:
        for kind in kinds:
            (self.path / kind).mkdir(parents=True, exist_ok=True)

    def image_path(self, kind: str, i, k=None) -> Path:
        """rgb/, depth/ or sem_mask/ of frame ``i``; with ``k``, mask/ or mask_visib/ of its k-th entry.  The colour image of
        a scene that stores rgb/ as JPEG (BOP's train_pbr splits): the .png when it exists, else an existing .jpg / .jpeg,
        else the .png path."""
        png = self.path / kind / image_name(i, k)
        if kind == "rgb" and k is None and not png.exists():
            for ext in JPEG_EXTENSIONS:
                if (jpg := png.with_suffix(ext)).exists():
                    return jpg
        return png

    def read_png(self, kind: str, i, k=None) -> np.ndarray:
        return decode_png(self.image_path(kind, i, k).read_bytes())

    def read_image(self, kind: str, i, k=None) -> np.ndarray:
        """``read_png`` that also opens the JPEG of a scene whose rgb/ is stored as JPEG."""
        return read_image(self.image_path(kind, i, k))

    def image_size(self, i):
        """(W, H) of frame ``i`` from the header of its rgb PNG or JPEG, else of its first visible mask, else (0, 0)."""
        return _first_size([self.image_path("rgb", i)] + sorted((self.path / "mask_visib").glob(f"{int(i):06d}_*.png"))) or (0, 0)

    def first_image_size(self):
        """(W, H) of the scene's first rgb (else depth) PNG or JPEG; None when it has neither."""
        return _first_size(p for kind in ("rgb", "depth") for p in sorted((self.path / kind).glob("*"))
                           if p.suffix in (".png",) + JPEG_EXTENSIONS)


def _first_size(files):
    """The size of the first of ``files`` that exists and is a PNG or a JPEG, else None."""
    return next((s for p in files if p.exists() and
                 (s := jpeg_size(p) if p.suffix in JPEG_EXTENSIONS else png_size(p)) is not None), None)


# ---- record fields ----------------------------------------------------------------------------------------------------
def cam_K(camera_entry: dict) -> np.ndarray:
    return np.asarray(camera_entry["cam_K"], np.float64).reshape(3, 3)


def pose_of(gt_entry: dict):
    """(R [3,3], t [3]) model to camera, float64; t in the unit scene_gt was written with."""
    return np.asarray(gt_entry["cam_R_m2c"], np.float64).reshape(3, 3), np.asarray(gt_entry["cam_t_m2c"], np.float64).reshape(3)


def unit_of(translation_scale) -> float:
    """Millimetres in scene_gt's unit: ``translation_scale`` is what its translations were written with (1: metres)."""
    return float(translation_scale) / 1000.0


def depth_unit(camera_entry: dict, unit: float) -> float:
    """What a depth image's samples are multiplied by to be in scene_gt's unit."""
    return float(camera_entry.get("depth_scale", 1.0)) * unit


# ---- models directory -------------------------------------------------------------------------------------------------
def model_files(models_dir) -> dict:
    """{obj_id: path} of every obj_NNNNNN.ply under ``models_dir``."""
    files = {int(m.group(1)): p for p in sorted(Path(models_dir).glob("obj_*.ply")) if (m := re.fullmatch(r"obj_(\d+)", p.stem))}
    if not files:
        raise FileNotFoundError(f"no obj_NNNNNN.ply under {models_dir}")
    return files


def read_models_info(models_dir) -> dict:
    """models_info.json as loaded (string keys); {} without the file."""
    path = Path(models_dir) / MODELS_INFO
    return json.loads(path.read_text()) if path.exists() else {}


# ---- PNG --------------------------------------------------------------------------------------------------------------
def encode_png(a: np.ndarray, level: int = 1) -> bytes:
    """uint8 [H,W] / [H,W,3] or uint16 [H,W] -> PNG bytes (colour type 0 or 2, no interlace, filter 0)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8 and a.ndim == 2:
        depth, ctype, rows = 8, 0, a
    elif a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3:
        depth, ctype, rows = 8, 2, a.reshape(a.shape[0], -1)
    elif a.dtype == np.uint16 and a.ndim == 2:
        depth, ctype, rows = 16, 0, a.astype(">u2").view(np.uint8).reshape(a.shape[0], -1)     # big-endian samples
    else:
        raise ValueError("encode_png takes uint8 [H,W], uint8 [H,W,3] or uint16 [H,W]")
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()                  # filter type 0 per row

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw, level)) + chunk(b"IEND", b""))


def decode_png(data: bytes) -> np.ndarray:
    """Inverse of encode_png for the files it writes (filter 0 only)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype = hdr[:4]
    ch = 3 if ctype == 2 else 1
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * ch * depth // 8)
    assert not raw[:, 0].any()
    body = raw[:, 1:]
    if depth == 16:
        return body.reshape(h, w, 2).copy().view(">u2").reshape(h, w).astype(np.uint16)
    return body.reshape(h, w, 3).copy() if ch == 3 else body.copy()


def png_size(path):
    """(W, H) from the IHDR of a PNG file; None when its first chunk is not one."""
    head = Path(path).read_bytes()[:24]
    return struct.unpack(">II", head[16:24]) if head[12:16] == b"IHDR" else None


# ---- JPEG -------------------------------------------------------------------------------------------------------------
def jpeg_size(path):
    """(W, H) from the SOF0 / SOF2 segment of a JPEG file, without decoding; None when the file has none."""
    data = Path(path).read_bytes()
    if data[:2] != b"\xff\xd8":
        return None
    pos = 2
    while pos + 4 <= len(data) and data[pos] == 0xFF:
        marker = data[pos + 1]
        if marker == 0xFF:                                   # a fill byte
            pos += 1
            continue
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        if marker in (0xC0, 0xC2) and pos + 9 <= len(data):
            h, w = struct.unpack(">HH", data[pos + 5:pos + 9])
            return w, h
        if marker == 0xDA:                                   # the scan: no frame header in front of it
            return None
        pos += 2 + n
    return None


def read_image(path) -> np.ndarray:
    """uint8 [H,W] / [H,W,3] or uint16 [H,W] of a PNG (``decode_png``) or a JPEG (PIL, imported when first needed)."""
    path = Path(path)
    if path.suffix.lower() not in JPEG_EXTENSIONS:
        return decode_png(path.read_bytes())
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError(f"{path} is a JPEG: reading it needs PIL (pip install pillow); this package only encodes JPEG") from e
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB"):
            im = im.convert("RGB")
        return np.asarray(im).copy()
