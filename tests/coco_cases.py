"""Deterministic mask stacks for the COCO tests (tests/test_coco_host.py, tests/test_coco_gpu.py and
tests/golden/make_golden_coco.py): every case is a uint8 [n,H,W] stack with n = 1, 3 or 4, named, with the reason it exists.
The sizes at which the kernels change path are read from pegasus_amd/_lib.py, which mirrors include/pegasus_raster.h."""
import numpy as np

from pegasus_amd import _lib

WORD_ROWS = _lib.PGR_RLE_WORD_ROWS                  # rows per bit-plane word
TILE_COLS = _lib.PGR_RLE_TILE_COLS                  # columns per wave of the plane kernel / per workgroup of the column kernels
BLOCK_ROWS = _lib.PGR_RLE_BLOCK_ROWS                # rows per workgroup of the plane kernel
DECODE_CHUNK = _lib.PGR_RLE_DECODE_CHUNK            # runs a decode workgroup scans at a time
DECODE_MIN_SLICE = _lib.PGR_RLE_DECODE_MIN_SLICE    # pixels per decode workgroup
OVERLAP_CHUNK = _lib.PGR_MASK_OVERLAP_CHUNK         # pixels per overlap workgroup
DECODE_MAX_SLICES = _lib.PGR_RLE_DECODE_MAX_SLICES  # slices per mask above which they grow
MAX_SIDE = 8192
GOLDEN_MAX_PIXELS = 400_000                         # cases up to this size are recorded from the toolkit (one Python step per pixel)
SCENE_W, SCENE_H = 40, 24


def blobs(rng, H, W, n=6):
    """A few filled ellipses: compact regions with curved borders, like object masks."""
    y, x = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(n):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        rx, ry = rng.uniform(0.05, 0.3) * W + 1, rng.uniform(0.05, 0.3) * H + 1
        m |= ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1.0
    return m.astype(np.uint8)


def random_stack(seed, n, H, W, p=0.5):
    rng = np.random.default_rng(seed)
    return (rng.random((n, H, W)) < p).astype(np.uint8)


def checker(H, W, phase):
    y, x = np.mgrid[0:H, 0:W]
    return (((x * H + y) + phase) % 2).astype(np.uint8)     # alternates along the column-major order: H*W runs of 1


def alternating_strip(n_counts):
    """A 1-wide column whose RLE has exactly ``n_counts`` counts: pixel 0 unset, then alternating, then a long tail."""
    H, T = n_counts + 40, n_counts - 1
    p = np.arange(H)
    m = np.where(p <= T, p % 2, T % 2).astype(np.uint8)     # transitions at 1 .. T, then the tail keeps pixel T's value
    return m.reshape(1, H, 1)


def shape_of(pixels):
    """(W, H) with W * H == pixels, as square as the factors allow, or None when a side would pass MAX_SIDE."""
    W = next(w for w in range(int(pixels ** 0.5), 0, -1) if pixels % w == 0)
    return (W, pixels // W) if pixels // W <= MAX_SIDE else None


def shapes_around(pixels):
    """Image shapes of one pixel less than, exactly, and the fewest pixels more than ``pixels`` that sides up to MAX_SIDE
    can form."""
    above = next(s for s in map(shape_of, range(pixels + 1, pixels + 65)) if s is not None)
    return [shape_of(pixels - 1), shape_of(pixels), above]


def toolkit_unions(ious_toolkit):
    """The unions behind what pycoco_utils.compute_ious returned: it divides any-overlap (0 or 1) by the union, so where
    two masks overlap the union is the reciprocal, an integer up to rounding."""
    ious = np.asarray(ious_toolkit, np.float64)
    return np.where(ious > 0, np.rint(1.0 / np.where(ious > 0, ious, 1.0)), 0).astype(np.int64)


def cases():
    """[(name, stack uint8 [n,H,W], why)] -- deterministic."""
    out = []

    def add(name, stack, why):
        stack = np.ascontiguousarray(stack, np.uint8)
        assert stack.ndim == 3 and stack.shape[0] in (1, 3, 4), name
        out.append((name, stack, why))
    add("1x1 unset", np.zeros((1, 1, 1)), "the smallest mask: counts [1]")
    add("1x1 set", np.ones((1, 1, 1)), "pixel 0 set and last: counts [0, 1]")
    for W in (7, 300):
        add(f"row strip W={W}", random_stack(W, 3, 1, W), "H = 1: every transition is across columns")
    for H in (7, 300):
        add(f"column strip H={H}", random_stack(100 + H, 3, H, 1), "W = 1: no transition is across columns")
    for W, H in ((5, 7), (7, 5), (17, 33), (33, 17)):
        add(f"odd {W}x{H}", random_stack(W * H, 3, H, W),
            "W and H*W are no multiples of 4: masks 1 and 2 and most rows start on odd byte offsets")
    for W, H in ((63, 65), (64, 64), (65, 63)):
        add(f"wave {W}x{H}", random_stack(W + 1000 * H, 1, H, W, 0.3), "63 / 64 / 65 columns and rows: the wave boundaries")
    for W in (TILE_COLS - 1, TILE_COLS, TILE_COLS + 1, 2 * TILE_COLS + 1):
        add(f"tile cols W={W}", random_stack(W, 1, 9, W, 0.4), "one below, at, above the column tile (and two tiles plus one)")
    for H in (WORD_ROWS - 1, WORD_ROWS, WORD_ROWS + 1, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1):
        add(f"tile rows H={H}", random_stack(7000 + H, 1, H, 9, 0.4), "one below, at, above a plane word and a workgroup's rows")
    edge = np.zeros((3, 33, 17), np.uint8)
    edge[0, 0, 0] = 1
    edge[1, -1, -1] = 1
    edge[2, -1, 0] = edge[2, 0, 1] = 1
    add("pixel 0 / last pixel / column seam", edge, "only pixel 0; only the last pixel; two pixels either side of a column end")
    add("all zero 17x33", np.zeros((3, 33, 17)), "no transition: counts [H*W]")
    add("all set 17x33", np.full((3, 33, 17), 255), "counts [0, H*W]")
    full_cols = np.zeros((1, 33, 17), np.uint8)
    full_cols[0, :, 3:7] = 1
    add("full columns", full_cols, "a block of full columns is ONE run across three column boundaries")
    seam = np.zeros((3, 33, 17), np.uint8)
    seam[0, 20:, 4] = 1; seam[0, :6, 5] = 1                 # through the bottom of column 4 into the top of column 5: one run
    seam[1, 20:, 4] = 1; seam[1, 1:6, 5] = 1                # ends exactly at the last row; the next starts one row below the top
    seam[2, 20:-1, 4] = 1; seam[2, :6, 5] = 1               # ends one above the last row; the next starts at the first row
    add("runs at a column end", seam, "a run that ends at a column's last row next to one that starts at the next column's first")
    add("checkerboard 17x33", np.stack([checker(33, 17, 0), checker(33, 17, 1), checker(33, 17, 0)]),
        "561 and 562 counts of 1 (and a leading 0): the most runs a mask can have, three decode chunks")
    mixed = np.zeros((1, 12, 9), np.uint8)
    mixed[0, 2:11, 3] = [1, 2, 255, 1, 128, 2, 255, 1, 2]
    mixed[0, :4, 4] = [255, 1, 2, 1]
    add("bytes 1, 2, 255 in one run", mixed, "any non-zero byte is set: mixed bytes do not split a run")
    add("300x300 all zero", np.zeros((1, 300, 300)), "one count of 90 000: more than 16 bits")
    rng = np.random.default_rng(77)
    stack = np.zeros((4, SCENE_H, SCENE_W), np.uint8)
    stack[1] = 1
    stack[3, 5, 7] = stack[3, 20, 33] = stack[3, 21, 33] = 1
    add("empty, dense, empty, sparse", stack, "a stack in one call: an empty mask's slot is exactly one count; pins the offsets")
    sparse = np.zeros((3, SCENE_H, SCENE_W), np.uint8)
    sparse[1, 5, 7] = sparse[1, 20, 33] = 1
    sparse[2] = blobs(rng, SCENE_H, SCENE_W, 3)
    add("empty, sparse, blobs", sparse, "few counts next to many in one call")
    for n in (DECODE_CHUNK - 1, DECODE_CHUNK, DECODE_CHUNK + 1):
        add(f"{n} counts", alternating_strip(n), "one below, at, above the runs a decode workgroup scans at a time")
    for unit in sorted({DECODE_MIN_SLICE, OVERLAP_CHUNK}):
        for W, H in shapes_around(unit):
            add(f"slice {W}x{H}", blobs(np.random.default_rng(W), H, W)[None], "one below, at, above a decode slice / an overlap chunk")
    for W, H in shapes_around(DECODE_MAX_SLICES * DECODE_MIN_SLICE):
        add(f"slices {W}x{H}", blobs(np.random.default_rng(H + W), H, W, 5)[None],
            "below, at, above the most decode slices a mask is cut into: they grow beyond")
    pair = np.stack([blobs(np.random.default_rng(s), 480, 640, 8) for s in (1, 2, 3)])
    pair[1] *= 255
    add("640x480 blobs", pair, "the real-size case")
    return out


def scene():
    """Two images of SCENE_W x SCENE_H for the scene_gt_coco golden: per image the instances' (obj_id, visible mask, full
    mask, visib_fract).  Covers a skipped instance in the middle (empty visible mask), one skipped in amodal mode only
    (empty full mask), ignore = True (visib_fract < 0.1) and the boundary visib_fract = 0.1 (not ignored)."""
    rng = np.random.default_rng(5)
    H, W = SCENE_H, SCENE_W
    full = [blobs(rng, H, W, 2) for _ in range(6)]
    cut = np.zeros((H, W), np.uint8)
    cut[:, : W // 2] = 1
    tiny = np.zeros((H, W), np.uint8)
    tiny[3, 4] = 1
    images = {
        0: [(5, full[0] * cut, full[0], 0.55), (2, np.zeros((H, W), np.uint8), full[1], 0.0), (9, tiny * 255, full[2] | tiny, 0.02)],
        3: [(2, full[3], full[3], 1.0), (5, full[4] * cut, np.zeros((H, W), np.uint8), 0.4), (7, full[5] * (1 - cut), full[5], 0.1)],
    }
    for inst in images.values():
        assert all(v.any() or f < 0.1 for _, v, _, f in inst)
    return images


DATES = ("date_created", "date_captured", "year")          # left out of every comparison with the toolkit's dicts


def undated(o):
    if isinstance(o, dict):
        return {k: undated(v) for k, v in o.items() if k not in DATES}
    if isinstance(o, list):
        return [undated(v) for v in o]
    return o


def golden_cases(golden):
    """[(name, stack, per-mask counts, boxes, decoded)] of the cases the toolkit was run on."""
    stacks = {name: stack for name, stack, _ in cases()}
    out = []
    for i, name in enumerate(golden["names"].tolist()):
        stack = stacks[name]
        ends = np.cumsum(golden[f"case{i}_lengths"])
        counts = np.split(golden[f"case{i}_counts"], ends[:-1])
        decoded = np.unpackbits(golden[f"case{i}_decoded"], axis=-1)[..., : stack.shape[2]]
        out.append((name, stack, counts, golden[f"case{i}_bbox"], decoded))
    return out
