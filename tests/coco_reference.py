"""The COCO mask rules restated in plain NumPy, independent of the kernels and of pegasus_amd.coco: run-length encoding in
column-major order starting with a run of zeros, its inverse, the smallest box, and overlap counts.  ``rle_encode`` and
``mask_stats`` have the signatures of pegasus_amd.coco's, on host arrays: this module is the device-free backend of the host
tests and the reference of the GPU tests.  tests/test_coco_host.py holds it against the BOP toolkit's recorded outputs."""
import numpy as np

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def rle_counts(mask) -> np.ndarray:
    """The counts of one mask [H,W]: int64 [n_counts]."""
    flat = (np.asarray(mask) != 0).ravel(order="F")
    change = np.flatnonzero(np.diff(np.concatenate(([False], flat)).astype(np.int8)) != 0)      # a virtual unset pixel in front
    return np.diff(np.concatenate(([0], change, [flat.size]))).astype(np.int64)


def decode(counts, size) -> np.ndarray:
    """uint8 [H,W] of 0 / 1 from alternating runs that start with zeros; the counts must sum to H*W."""
    H, W = int(size[0]), int(size[1])
    counts = np.asarray(counts, np.int64)
    assert counts.min(initial=0) >= 0 and int(counts.sum()) == H * W
    values = (np.arange(len(counts)) % 2).astype(np.uint8)
    return np.repeat(values, counts).reshape(W, H).T.copy()


def stats_row(mask) -> np.ndarray:
    """n_counts, area, x_min, y_min, x_max, y_max; INT32_MAX / INT32_MIN extents when the mask is empty."""
    m = np.asarray(mask) != 0
    ys, xs = np.nonzero(m)
    if len(xs) == 0:
        ext = [INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN]
    else:
        ext = [xs.min(), ys.min(), xs.max(), ys.max()]
    return np.asarray([len(rle_counts(m)), int(m.sum())] + [int(e) for e in ext], np.int64)


def bbox(mask) -> list:
    """[x, y, w, h] of the smallest box holding every set pixel of a non-empty mask."""
    s = stats_row(mask)
    return [int(s[2]), int(s[3]), int(s[4] - s[2] + 1), int(s[5] - s[3] + 1)]


def rle_encode(masks):
    """(counts int32 [total], offsets int64 [n+1], stats int32 [n,6]) of a stack [n,H,W]."""
    masks = np.asarray(masks)
    per = [rle_counts(m) for m in masks]
    offsets = np.zeros(len(per) + 1, np.int64)
    np.cumsum([len(c) for c in per], out=offsets[1:])
    return np.concatenate(per).astype(np.int32), offsets, mask_stats(masks)


def mask_stats(masks):
    return np.stack([stats_row(m) for m in np.asarray(masks)]).astype(np.int32)


def overlap(a, b):
    """(inter int64 [n_a,n_b], area_a [n_a], area_b [n_b]) of two stacks [n,H,W]."""
    A = (np.asarray(a) != 0).reshape(len(a), -1).astype(np.int64)
    B = (np.asarray(b) != 0).reshape(len(b), -1).astype(np.int64)
    return A @ B.T, A.sum(1), B.sum(1)


def ious(a, b):
    inter, aa, ab = overlap(a, b)
    union = aa[:, None] + ab[None, :] - inter
    return np.where(union > 0, inter / np.maximum(union, 1), 0.0)
