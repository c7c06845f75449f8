"""Seeded cases for the COCO score tests (tests/test_coco_eval_host.py, tests/test_coco_eval_gpu.py): masks as run lists,
group tables for the IoU kernels, and whole ground-truth / detection sets.  Images are 17x33 and 64x48."""
import functools

import numpy as np

SMALL, LARGE = (17, 33), (64, 48)                       # (H, W)
CHUNK, LDS_RUNS = 256, 4096                             # include/pegasus_raster.h PGR_COCO_CHUNK, PGR_COCO_LDS_RUNS


# ---- masks ------------------------------------------------------------------------------------------------------------
def rle_of(mask):
    """The run lengths of a mask [H,W] in column-major pixel order, starting with a run of zeros."""
    flat = np.asarray(mask, bool).T.reshape(-1)
    edges = np.flatnonzero(np.diff(np.r_[False, flat])) if flat.size else np.zeros(0, np.int64)
    return np.diff(np.r_[0, edges, flat.size]).tolist() if len(edges) else [int(flat.size)]


def ellipse(size, cy, cx, ry, rx):
    y, x = np.mgrid[:size[0], :size[1]]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def stripes(size, period, phase=0, vertical=False):
    y, x = np.mgrid[:size[0], :size[1]]
    return (((x if vertical else y) + phase) // period) % 2 == 0


def checkerboard(size, phase=0):
    y, x = np.mgrid[:size[0], :size[1]]
    return (x + y + phase) % 2 == 0


def rect(size, y0, x0, h, w):
    m = np.zeros(size, bool)
    m[max(y0, 0):max(y0 + h, 0), max(x0, 0):max(x0 + w, 0)] = True
    return m


def runs_exactly(n, n_pixels, rng, first_zero=False):
    """A run list with exactly ``n`` counts that sum to ``n_pixels``: every count >= 1 (the first one 0 with ``first_zero``)."""
    if n == 1:
        return [n_pixels]
    c = np.ones(n, np.int64)
    if first_zero:
        c[0] = 0
    spare = n_pixels - int(c.sum())
    assert spare >= 0, (n, n_pixels)
    cuts = np.sort(rng.integers(0, spare + 1, n - 1))
    c += np.diff(np.r_[0, cuts, spare])
    if first_zero:
        c[1] += c[0]
        c[0] = 0
    assert int(c.sum()) == n_pixels and len(c) == n
    return c.tolist()


def with_zero_runs(counts, where):
    """``counts`` with a pair of zero-length runs inserted in front of index ``where`` (the mask does not change)."""
    return list(counts[:where]) + [0, 0] + list(counts[where:])


def family(size, rng):
    """name -> run list: every kind of mask the IoU kernel meets at one image size."""
    H, W = size
    n = H * W
    out = {
        "empty": [n], "full": [0, n],
        "ellipse": rle_of(ellipse(size, H / 2, W / 2, H / 3, W / 3)),
        "ellipse off": rle_of(ellipse(size, H / 2 + 2, W / 2 - 3, H / 4, W / 2.5)),
        "stripes": rle_of(stripes(size, 3)), "stripes v": rle_of(stripes(size, 2, 1, True)),
        "checkerboard": rle_of(checkerboard(size)), "checkerboard odd": rle_of(checkerboard(size, 1)),
        "pixel 0": [0, 1, n - 1], "last pixel": [n - 1, 1],
    }
    base = out["ellipse"]
    out["zeros in front"] = with_zero_runs(base, 0)
    out["zeros inside"] = with_zero_runs(with_zero_runs(base, 3), 3)
    out["zeros at the end"] = list(base) + [0, 0]
    out["one zero at the end"] = list(out["stripes"]) + [0]
    out["only zeros then full"] = [0, 0, 0, n]
    for runs in (2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1):
        if runs <= n:
            out[f"{runs} runs"] = runs_exactly(runs, n, rng, first_zero=bool(runs % 2 == 0 and runs > 2))
    if n >= 4 * CHUNK + 1:
        out[f"{4 * CHUNK + 1} runs"] = runs_exactly(4 * CHUNK + 1, n, rng)
        out["1500 runs"] = runs_exactly(1500, n, rng, first_zero=True)
    for name, c in out.items():
        assert sum(c) == n and min(c) >= 0, name
    return out


@functools.lru_cache(maxsize=None)
def iou_cases():
    """name -> dict(size, dt, gt: run lists, crowd, groups: rows (dt_begin, dt_count, gt_begin, gt_count)).  Every family
    against every other, the run-count edges, zero-length runs, crowd columns, empty groups, and groups whose GT runs are at,
    below and beyond what is staged in LDS."""
    rng = np.random.default_rng(20240611)
    out = {}
    for size in (SMALL, LARGE):
        fam = list(family(size, rng).values())
        n = len(fam)
        crowd = [(k % 3 == 1) for k in range(n)]
        out[f"all against all {size[0]}x{size[1]}"] = dict(size=size, dt=fam, gt=fam, crowd=crowd, groups=[(0, n, 0, n)])
        # the same masks cut into several groups, with empty ones between and rows / columns that belong to no group
        out[f"split {size[0]}x{size[1]}"] = dict(size=size, dt=fam, gt=fam, crowd=crowd,
                                                 groups=[(0, 1, 0, 1), (1, 0, 1, 3), (1, 3, 4, 0), (5, 0, 4, 0), (5, n - 6, 5, n - 6)])
    n_pix = LARGE[0] * LARGE[1]
    many = [runs_exactly(1025, n_pix, rng) for _ in range(5)]               # 5125 runs: beyond LDS_RUNS
    few = [runs_exactly(1024, n_pix, rng, True) for _ in range(4)]           # 4096 runs: exactly LDS_RUNS
    over = few[:3] + [runs_exactly(1025, n_pix, rng)]                        # 4097 runs: one beyond
    probes = [rle_of(ellipse(LARGE, 30, 20, 18, 12)), runs_exactly(1500, n_pix, rng), [n_pix], [0, n_pix]]
    assert sum(map(len, many)) > LDS_RUNS and sum(map(len, few)) == LDS_RUNS and sum(map(len, over)) == LDS_RUNS + 1
    out["GT runs beyond LDS"] = dict(size=LARGE, dt=probes, gt=many, crowd=[0, 1, 0, 0, 1], groups=[(0, 4, 0, 5)])
    out["GT runs fill LDS"] = dict(size=LARGE, dt=probes, gt=few, crowd=[0, 0, 1, 0], groups=[(0, 4, 0, 4)])
    out["GT runs one beyond LDS"] = dict(size=LARGE, dt=probes, gt=over, crowd=[1, 0, 0, 0], groups=[(0, 4, 0, 4)])
    out["staged and unstaged groups"] = dict(size=LARGE, dt=probes + probes, gt=few[:2] + many, crowd=[0] * 7,
                                             groups=[(0, 4, 0, 2), (4, 4, 2, 5)])
    out["no groups"] = dict(size=SMALL, dt=[[561]], gt=[[0, 561]], crowd=[0], groups=[])
    return out


def box_cases():
    """name -> dict(dt, gt: float64 [n,4], crowd, groups).  Boxes whose products and sums are not exact in float64 (an FMA
    changes the last bit of the union), touching and disjoint boxes, zero-area boxes, identical boxes."""
    rng = np.random.default_rng(77)
    n_d, n_g = 70, 67
    dt = np.c_[rng.uniform(0, 40, (n_d, 2)), rng.uniform(0.5, 30, (n_d, 2))]
    gt = np.c_[rng.uniform(0, 40, (n_g, 2)), rng.uniform(0.5, 30, (n_g, 2))]
    dt[:5] = gt[:5]                                                         # identical: IoU 1
    dt[5] = [0, 0, 10, 10]; gt[5] = [10, 0, 10, 10]                         # touching: iw = 0
    dt[6] = [0, 0, 0, 5]; gt[6] = [0, 0, 0, 5]                              # zero-area pair: 0, not 0/0
    dt[7] = [1 / 3, 1 / 7, 10 / 3, 20 / 7]; gt[7] = [2 / 3, 2 / 7, 10 / 3, 20 / 7]
    dt[8] = [100, 100, 96, 96]; gt[8] = [100, 100, 96, 96]
    crowd = (np.arange(n_g) % 4 == 2).astype(np.uint8)
    return {"one group": dict(dt=dt, gt=gt, crowd=crowd, groups=[(0, n_d, 0, n_g)]),
            "several groups": dict(dt=dt, gt=gt, crowd=crowd, groups=[(0, 9, 0, 9), (9, 0, 9, 4), (9, 30, 13, 0), (39, 31, 13, 54)])}


# ---- whole evaluations ----------------------------------------------------------------------------------------------------
def _bbox(mask):
    ys, xs = np.nonzero(mask)
    if not len(ys):
        return [0.0, 0.0, 0.0, 0.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]


def _random_mask(size, rng):
    H, W = size
    kind = rng.integers(0, 6)
    if kind == 0:
        return ellipse(size, rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2, H / 2), rng.uniform(2, W / 2))
    if kind == 1:
        return rect(size, int(rng.integers(0, H - 2)), int(rng.integers(0, W - 2)), int(rng.integers(2, H)), int(rng.integers(2, W)))
    if kind == 2:
        return stripes(size, int(rng.integers(1, 5)), int(rng.integers(0, 4)), bool(rng.integers(0, 2))) & \
            rect(size, 0, 0, int(rng.integers(3, H + 1)), int(rng.integers(3, W + 1)))
    if kind == 3:
        return checkerboard(size, int(rng.integers(0, 2))) & ellipse(size, H / 2, W / 2, H / 2.5, W / 2.5)
    if kind == 4:
        return ellipse(size, H / 2, W / 2, H / 3, W / 3) ^ rect(size, H // 3, W // 3, H // 4, W // 4)
    return rng.random(size) < 0.3


def _perturbed(mask, rng):
    """A detection for a ground-truth mask: the mask itself, a shifted or a grown / shrunk one, or something else."""
    size = mask.shape
    how = rng.integers(0, 6)
    if how == 0:
        return mask.copy()
    if how in (1, 2):
        return np.roll(mask, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (0, 1))
    if how == 3:
        return mask & rect(size, 0, 0, int(rng.integers(size[0] // 2, size[0] + 1)), size[1])
    if how == 4:
        return mask | np.roll(mask, 1, 1)
    return _random_mask(size, rng)


def dataset(seed, images, string_counts=False, scale_areas=(1, 1, 1, 3, 20)):
    """A ground truth dict and a detection list.  ``images``: one (size, {category: (gt_count, dt_count)}) per image, ids
    counting from 1; the categories are 1..5 always (one may stay without annotations).  Every detection carries ``bbox``
    and ``segmentation``.  Scores come from twentieths, so they tie inside an image and across images.  A GT's ``area`` is
    its pixel count times a factor of ``scale_areas``: with images this small that is what puts GT into the medium and
    large ranges, and leaves detections of them outside."""
    from pegasus_amd.coco_eval import rle_string_encode                     # (pinned on its own in test_coco_eval_host.py)
    rng = np.random.default_rng(seed)
    gt = {"images": [], "annotations": [], "categories": [{"id": c, "name": str(c), "supercategory": "case"} for c in range(1, 6)]}
    dt = []

    def seg(mask):
        counts = rle_of(mask)
        return {"counts": rle_string_encode(counts) if string_counts else counts, "size": [mask.shape[0], mask.shape[1]]}
    for n, (size, per_cat) in enumerate(images):
        image_id = n + 1
        gt["images"].append({"id": image_id, "width": size[1], "height": size[0], "file_name": f"rgb/{image_id:06d}.png"})
        for cat, (n_gt, n_dt) in sorted(per_cat.items()):
            masks = []
            for _ in range(n_gt):
                m = _random_mask(size, rng)
                masks.append(m)
                area = int(m.sum()) * int(rng.choice(scale_areas))
                gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": image_id, "category_id": cat,
                                          "iscrowd": int(rng.random() < 0.15), "area": area, "bbox": _bbox(m),
                                          "segmentation": {"counts": rle_of(m), "size": list(size)},
                                          "ignore": bool(rng.random() < 0.2), "width": size[1], "height": size[0]})
            for _ in range(n_dt):
                m = _perturbed(masks[int(rng.integers(0, n_gt))], rng) if n_gt and rng.random() < 0.8 else _random_mask(size, rng)
                box = _bbox(m)
                if rng.random() < 0.5:
                    box = [box[0] + rng.uniform(-1, 1), box[1] + rng.uniform(-1, 1), box[2] * rng.uniform(0.8, 1.2), box[3] * rng.uniform(0.8, 1.2)]
                dt.append({"image_id": image_id, "category_id": cat, "score": float(rng.integers(1, 21)) / 20.0, "bbox": box,
                           "segmentation": seg(m)})
    order = rng.permutation(len(dt))                                        # a results file is in no particular order
    return gt, [dt[k] for k in order]


def edges_images():
    """The group sizes the issue names: gt_count 0, 1, 2, 63, 64, 65; dt_count 0, 1, 100, 101, 130; an image without
    anything; category 4 without detections anywhere; category 5 is made to have no small GT by ``edges``."""
    return [(SMALL, {1: (1, 1), 2: (2, 100), 3: (0, 5), 4: (2, 0)}),
            (SMALL, {1: (63, 101), 2: (64, 0), 3: (65, 130)}),
            (SMALL, {}),
            (LARGE, {1: (0, 3), 2: (3, 4), 5: (2, 3)}),
            (LARGE, {1: (2, 2), 3: (1, 10), 5: (1, 1)})]


@functools.lru_cache(maxsize=None)
def edges(string_counts=False):
    """The ``edges_images`` set, with areas exactly at 32^2 and 96^2 and category 5 without a GT in the small range."""
    gt, dt = dataset(11, edges_images(), string_counts)
    cat5 = [a for a in gt["annotations"] if a["category_id"] == 5]
    for a, area in zip(cat5, (32 ** 2 + 1, 96 ** 2, 96 ** 2 + 5)):
        a["area"], a["iscrowd"], a["ignore"] = area, 0, False
    cat2 = [a for a in gt["annotations"] if a["category_id"] == 2 and a["image_id"] == 4]
    cat2[0]["area"], cat2[1]["area"] = 32 ** 2, 96 ** 2                     # in two ranges at once: the bounds are inclusive
    # detections whose own area is exactly 32^2 (a 32 x 32 block) and, for boxes, exactly 96^2
    for r in [r for r in dt if r["image_id"] == 4 and r["category_id"] == 2][:2]:
        m = rect(LARGE, 5, 7, 32, 32)
        from pegasus_amd.coco_eval import rle_string_encode
        counts = rle_of(m)
        r["segmentation"] = {"counts": rle_string_encode(counts) if string_counts else counts, "size": list(LARGE)}
        r["bbox"] = [7.0, 5.0, 96.0, 96.0]
    return gt, dt


@functools.lru_cache(maxsize=None)
def random_set(seed, string_counts=False):
    rng = np.random.default_rng(1000 + seed)
    images = []
    for _ in range(6):
        size = SMALL if rng.random() < 0.7 else LARGE
        images.append((size, {int(c): (int(rng.integers(0, 5)), int(rng.integers(0, 7))) for c in rng.choice([1, 2, 3, 4], 3, replace=False)}))
    return dataset(seed, images, string_counts)


def evaluation_sets():
    """name -> (gt, dt) with list counts."""
    return {"edges": edges(), "random 0": random_set(0), "random 1": random_set(1), "random 2": random_set(2)}
