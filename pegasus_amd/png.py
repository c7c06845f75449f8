"""PNG files of device images, encoded on the device (pgr_png_encode / pgr_png_emit).

``bop_dataset.encode_png`` for images that lie in HBM: deflate, CRC-32, Adler-32 and the chunk framing run as HIP kernels, a
batch of images per call; what crosses PCIe is the files.  The files are read by ``bop_dataset.decode_png`` and every PNG
reader (signature, IHDR, one IDAT, IEND; filter type 0; the rule is at the top of csrc/png.hip.h).  There is no host path
here: ``bop_dataset.encode_png`` is the host encoder.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

SEGMENT_BYTES = _lib.PGR_PNG_SEGMENT_BYTES


def _job(image: torch.Tensor, scale: int) -> _lib.PgrPngJob:
    if image.device.type != "cuda":
        raise RuntimeError("png.encode_batch needs HIP device tensors; there is no CPU path (bop_dataset.encode_png is the host encoder)")
    item = image.element_size()
    if image.dtype == torch.uint8 and image.dim() == 2:
        kind = _lib.PGR_PNG_GRAY8
    elif image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3:
        kind = _lib.PGR_PNG_RGB8
        if image.stride(2) != 1:
            raise ValueError("an RGB image's three channels must be adjacent bytes (stride 1 in the last dimension)")
    elif image.dtype in (torch.int16, torch.uint16) and image.dim() == 2:
        kind = _lib.PGR_PNG_GRAY16
    else:
        raise ValueError("png.encode_batch takes uint8 [H,W], uint8 [H,W,3] or int16 / uint16 [H,W] tensors, "
                         f"not {image.dtype} {tuple(image.shape)}")
    if scale not in (1, 255) or (scale == 255 and kind != _lib.PGR_PNG_GRAY8):
        raise ValueError("scale is 1, or 255 for a uint8 [H,W] mask of 0 / 1")
    H, W = int(image.shape[0]), int(image.shape[1])
    if H < 1 or W < 1:
        raise ValueError(f"an image of {W} x {H} pixels has no PNG")
    # a dimension of one pixel may carry any stride: give it the packed one
    bpp = (1, 3, 2)[kind]
    pixel_stride = int(image.stride(1)) * item if W > 1 else bpp
    row_stride = int(image.stride(0)) * item if H > 1 else (W - 1) * pixel_stride + bpp
    return _lib.PgrPngJob(pixels=image.data_ptr(), width=W, height=H, kind=kind, row_stride=row_stride,
                          pixel_stride=pixel_stride, scale=scale)


def max_bytes(width: int, height: int, kind: int) -> int:
    """What no file of that shape exceeds: 63 + raw bytes + 5 per segment (pgr_png_max_bytes; host only)."""
    return int(_lib.lib().pgr_png_max_bytes(int(width), int(height), int(kind)))


def encode_batch(images, level: int = 1, scale=None):
    """``images``: device tensors, each uint8 [H,W] (gray), uint8 [H,W,3] (RGB) or int16 / uint16 [H,W] (16-bit gray; int16 is
    the bit pattern of uint16, as masks.pack_frames stores depth).  Views are read where they lie when only the row and pixel
    strides differ from a packed image (a slice of a frame record, a plane of a stack, a crop).  ``scale``: None, 1 or 255 for
    all images, or one value per image -- 255 writes a 0 / 1 mask as 0 / 255.  ``level``: 0 codes literals only, 1 matches.
    Returns (files, offsets): a numpy uint8 buffer and int64 [n + 1]; file k is ``files[offsets[k]:offsets[k + 1]]``.
    Two launches' worth of work and two copies to the host: the offsets, then the bytes of the files."""
    images = list(images)
    n = len(images)
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.int64)
    scales = [1] * n if scale is None else [int(scale)] * n if np.isscalar(scale) else [int(s) for s in scale]
    if len(scales) != n:
        raise ValueError(f"{len(scales)} scales for {n} images")
    device = images[0].device
    if any(im.device != device for im in images):
        raise ValueError("the images of one batch lie on one device")
    jobs = (_lib.PgrPngJob * n)(*[_job(im, s) for im, s in zip(images, scales)])
    ws = _lib.workspace("pgr_png", device, n, jobs)
    sizes = torch.empty(n, dtype=torch.int64, device=device)
    _lib.call("pgr_png_encode", device, jobs, n, int(level), _lib.ptr(sizes), _lib.ptr(ws), ws.numel())
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
    torch.cumsum(sizes, 0, out=offsets[1:])
    offsets_host = offsets.cpu().numpy()                     # the one small copy (it also orders the host behind the encode pass)
    total = int(offsets_host[-1])
    files = torch.empty(total, dtype=torch.uint8, device=device)
    _lib.call("pgr_png_emit", device, jobs, n, _lib.ptr(offsets), total, _lib.ptr(files), total, _lib.ptr(ws), ws.numel())
    return files.cpu().numpy(), offsets_host


def encode_batch_bytes(images, level: int = 1, scale=None):
    """``encode_batch`` as a list of ``bytes``, one per image."""
    files, offsets = encode_batch(images, level, scale)
    return [files[offsets[k]:offsets[k + 1]].tobytes() for k in range(len(offsets) - 1)]


def code_lengths(freq, limit: int):
    """The encoder's length-limited code builder on host arrays (pgr_png_code_lengths): uint8 [n] code lengths."""
    freq = np.ascontiguousarray(freq, dtype=np.uint32)
    lengths = np.zeros(freq.shape[0], np.uint8)
    _lib.check(_lib.lib().pgr_png_code_lengths(freq.ctypes.data_as(C.POINTER(C.c_uint32)), int(freq.shape[0]), int(limit),
                                               lengths.ctypes.data_as(C.POINTER(C.c_uint8))), "pgr_png_code_lengths")
    return lengths
