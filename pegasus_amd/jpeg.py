"""JPEG files of device images, encoded on the device (pgr_jpeg_encode / pgr_jpeg_emit).

Baseline JPEG for images that lie in HBM: colour transform, DCT, quantisation, per-file Huffman tables and the entropy-coded
scan run as HIP kernels, a batch of images per call; what crosses PCIe is the files.  Every JPEG reader opens them (JFIF,
one interleaved scan, restart intervals; the rule is at the top of csrc/jpeg.hip.h).  There is no host path here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

RESTART_MCUS = _lib.PGR_JPEG_RESTART_MCUS
SUBSAMPLINGS = {"4:4:4": _lib.PGR_JPEG_444, "444": _lib.PGR_JPEG_444, "4:2:0": _lib.PGR_JPEG_420, "420": _lib.PGR_JPEG_420}


def subsampling_code(subsampling) -> int:
    """'4:4:4' / '4:2:0' (or '444' / '420', or the ABI's own 0 / 1) as PGR_JPEG_444 / PGR_JPEG_420."""
    if isinstance(subsampling, (int, np.integer)) and not isinstance(subsampling, bool) and int(subsampling) in (0, 1):
        return int(subsampling)
    try:
        return SUBSAMPLINGS[str(subsampling)]
    except KeyError:
        raise ValueError(f"subsampling is '4:4:4' or '4:2:0', not {subsampling!r}") from None


def _job(image: torch.Tensor, quality: int, subsampling: int) -> _lib.PgrJpegJob:
    if image.device.type != "cuda":
        raise RuntimeError("jpeg.encode_batch needs HIP device tensors; there is no CPU path")
    if image.dim() == 3 and image.shape[2] == 4:
        raise ValueError("jpeg.encode_batch does not take RGBA images: JPEG has no alpha channel (drop it, or write a PNG)")
    if image.dtype in (torch.int16, torch.uint16):
        raise ValueError("jpeg.encode_batch does not take 16-bit images: baseline JPEG is 8-bit (png.encode_batch writes 16-bit gray)")
    if image.dtype == torch.uint8 and image.dim() == 2:
        kind, bpp, subsampling = _lib.PGR_JPEG_GRAY8, 1, _lib.PGR_JPEG_444
    elif image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3:
        kind, bpp = _lib.PGR_JPEG_RGB8, 3
        if image.stride(2) != 1:
            raise ValueError("an RGB image's three channels must be adjacent bytes (stride 1 in the last dimension)")
    else:
        raise ValueError(f"jpeg.encode_batch takes uint8 [H,W] or uint8 [H,W,3] tensors, not {image.dtype} {tuple(image.shape)}")
    H, W = int(image.shape[0]), int(image.shape[1])
    if H < 1 or W < 1:
        raise ValueError(f"an image of {W} x {H} pixels has no JPEG")
    # a dimension of one pixel may carry any stride: give it the packed one
    pixel_stride = int(image.stride(1)) if W > 1 else bpp
    row_stride = int(image.stride(0)) if H > 1 else (W - 1) * pixel_stride + bpp
    return _lib.PgrJpegJob(pixels=image.data_ptr(), width=W, height=H, kind=kind, row_stride=row_stride,
                           pixel_stride=pixel_stride, quality=quality, subsampling=subsampling)


def max_bytes(width: int, height: int, kind: int, subsampling="4:4:4") -> int:
    """What no file of that shape exceeds (pgr_jpeg_max_bytes; host only); 0 outside the domain."""
    return int(_lib.lib().pgr_jpeg_max_bytes(int(width), int(height), int(kind), subsampling_code(subsampling)))


def quant_tables(quality: int):
    """The luminance and chrominance tables of ``quality`` (1..100) in natural order, uint8 [64] each: the IJG rule."""
    lum, chroma = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    u8 = C.POINTER(C.c_uint8)
    _lib.check(_lib.lib().pgr_jpeg_quant_tables(int(quality), lum.ctypes.data_as(u8), chroma.ctypes.data_as(u8)), "pgr_jpeg_quant_tables")
    return lum, chroma


def encode_batch(images, quality=95, subsampling="4:2:0"):
    """``images``: device tensors, each uint8 [H,W] (gray) or uint8 [H,W,3] (RGB).  Views are read where they lie when only the
    row and pixel strides differ from a packed image (a slice of a frame record, a plane of a stack, a crop).  ``quality``
    (1..100) and ``subsampling`` ('4:4:4' or '4:2:0'; gray images have none) are one value for all images or one per image.
    Returns (files, offsets): a numpy uint8 buffer and int64 [n + 1]; file k is ``files[offsets[k]:offsets[k + 1]]``."""
    images = list(images)
    n = len(images)
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.int64)
    qualities = [int(quality)] * n if np.isscalar(quality) else [int(q) for q in quality]
    subs = [subsampling] * n if isinstance(subsampling, (str, int, np.integer)) else list(subsampling)
    if len(qualities) != n or len(subs) != n:
        raise ValueError(f"{len(qualities)} qualities and {len(subs)} subsamplings for {n} images")
    if any(not 1 <= q <= 100 for q in qualities):
        raise ValueError("quality is 1..100")
    device = images[0].device
    if any(im.device != device for im in images):
        raise ValueError("the images of one batch lie on one device")
    jobs = (_lib.PgrJpegJob * n)(*[_job(im, q, subsampling_code(s)) for im, q, s in zip(images, qualities, subs)])
    ws = _lib.workspace("pgr_jpeg", device, n, jobs)
    sizes = torch.empty(n, dtype=torch.int64, device=device)
    _lib.call("pgr_jpeg_encode", device, jobs, n, _lib.ptr(sizes), _lib.ptr(ws), ws.numel())
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
    torch.cumsum(sizes, 0, out=offsets[1:])
    offsets_host = offsets.cpu().numpy()                     # the one small copy (it also orders the host behind the encode pass)
    total = int(offsets_host[-1])
    files = torch.empty(total, dtype=torch.uint8, device=device)
    _lib.call("pgr_jpeg_emit", device, jobs, n, _lib.ptr(offsets), total, _lib.ptr(files), total, _lib.ptr(ws), ws.numel())
    return files.cpu().numpy(), offsets_host


def encode_batch_bytes(images, quality=95, subsampling="4:2:0"):
    """``encode_batch`` as a list of ``bytes``, one per image."""
    files, offsets = encode_batch(images, quality, subsampling)
    return [files[offsets[k]:offsets[k + 1]].tobytes() for k in range(len(offsets) - 1)]
