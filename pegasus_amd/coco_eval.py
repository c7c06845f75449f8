"""COCO detection and segmentation scores of the BOP 2D tasks on the GPU: the BOP toolkit's scripts/eval_bop22_coco.py,
which runs pycocotools.COCOeval over a BOP22 results file and the dataset's ``scene_gt_coco*.json``.

    python -m pegasus_amd.coco_eval --results <json> --dataset <dir> [--ann_type segm|bbox] [--bbox_type amodal|modal]
                                    [--targets <json>] [--use_ignore_field] [--out <dir>]

prints AP, AP50, AP75, AP_small/medium/large, AR1/10/100 and AR_small/medium/large and writes
``scores_bop22_coco_<ann_type>[_modal].json``.

pycocotools is not a requirement of this project: parity with it is pinned by the written rule at the top of
pegasus_amd/csrc/cocoeval.hip.h and by hand-worked known answers, not by recorded outputs.  The IoU,
the matching and the accumulation run on the device from run lists and boxes, never from pixels; forming the groups, the
stable order by score and the twelve means is host-side plumbing here.

Two quirks of COCOeval are kept.  Its ``_prepare`` overwrites every annotation's ``ignore`` with ``iscrowd``, so the
``ignore`` that scene_gt_coco.json carries for ``visib_fract < 0.1`` has no effect under the toolkit's script;
``Params.use_ignore_field`` ORs it in.  And a compressed ``counts`` string (``rleToString``) is decoded here on the host
(``rle_string_decode``); ``pegasus_amd.coco.rle_decode`` keeps refusing it.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib, bop_dataset as BD
from .coco import coco_file_name, rle_counts, rle_flatten, rle_lists

STAT_NAMES = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "AR100", "AR_small", "AR_medium",
              "AR_large")
GROUP_DTYPE = np.dtype([("dt_begin", "<i4"), ("dt_count", "<i4"), ("gt_begin", "<i4"), ("gt_count", "<i4"),
                        ("iou_offset", "<i8")])
assert GROUP_DTYPE.itemsize == C.sizeof(_lib.PgrCocoGroup)


# ---- compressed counts (pycocotools rleToString / rleFrString) -----------------------------------------------------------
def rle_string_encode(counts) -> str:
    """``rleToString``: per count x, from the fourth on minus counts[i-2]; then 5-bit groups, low group first, bit 0x20 set
    while more follow (more follow when ``x != -1`` after a group with bit 0x10, ``x != 0`` after one without), each group
    written as chr(group + 48)."""
    counts = [int(c) for c in counts]
    out = []
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def rle_string_decode(s) -> list:
    """``rleFrString``: the inverse of ``rle_string_encode`` (sign-extended from bit 0x10 of a count's last group, then
    counts[i-2] added back from the fourth count on)."""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p >= len(s):
                raise ValueError("compressed RLE string ends inside a count")
            c = ord(s[p]) - 48
            if not 0 <= c < 64:
                raise ValueError(f"character {s[p]!r} is not part of a compressed RLE string")
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


# ---- parameters and result ------------------------------------------------------------------------------------------------
@dataclass
class Params:
    """COCOeval's Params for ``bbox`` / ``segm``.  ``img_ids`` / ``cat_ids`` None: every image / category of the ground
    truth, ascending.  ``use_ignore_field``: also ignore GT whose ``ignore`` is set (COCOeval reads ``iscrowd`` only)."""
    iou_thrs: np.ndarray = field(default_factory=lambda: np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1))
    rec_thrs: np.ndarray = field(default_factory=lambda: np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1))
    max_dets: Sequence[int] = (1, 10, 100)
    area_rng: Sequence[Sequence[float]] = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
    area_rng_lbl: Sequence[str] = ("all", "small", "medium", "large")
    img_ids: Optional[Sequence[int]] = None
    cat_ids: Optional[Sequence[int]] = None
    use_ignore_field: bool = False


@dataclass
class CocoScores:
    precision: np.ndarray        # [T,R,K,A,M], -1 where the category has no GT that counts
    recall: np.ndarray           # [T,K,A,M]
    scores: np.ndarray           # [T,R,K,A,M]
    stats: np.ndarray            # the twelve of COCOeval.stats
    params: Params

    def as_dict(self) -> dict:
        return {k: float(v) for k, v in zip(STAT_NAMES, self.stats)}


def summarize(precision, recall, params: Params) -> np.ndarray:
    """``COCOeval.summarize``: each statistic is the mean of the selected entries > -1, -1 without any."""
    iou_thrs = np.asarray(params.iou_thrs, np.float64)
    lbl, dets = list(params.area_rng_lbl), list(params.max_dets)

    def one(ap, iou_thr=None, area="all", max_det=dets[-1]):
        if area not in lbl or max_det not in dets:
            return -1.0
        a, m = lbl.index(area), dets.index(max_det)
        s = precision[:, :, :, a, m] if ap else recall[:, :, a, m]
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    last = dets[-1]
    return np.array([one(1), one(1, .5), one(1, .75), one(1, area="small"), one(1, area="medium"), one(1, area="large"),
                     one(0, max_det=dets[0]), one(0, max_det=dets[1] if len(dets) > 1 else last),
                     one(0, max_det=dets[2] if len(dets) > 2 else last), one(0, area="small"), one(0, area="medium"),
                     one(0, area="large")], np.float64)


# ---- host side: the problem as arrays -------------------------------------------------------------------------------------
@dataclass
class Problem:
    """One evaluation as flat host arrays.  GT sorted by (image, category), stable: file order inside a group.  Detections
    sorted by (image, category, -score), stable, every group cut to maxDets[-1]."""
    iou_type: str
    params: Params
    img_ids: list
    cat_ids: list
    groups: np.ndarray                     # GROUP_DTYPE, ascending by (image, category); only groups with a GT or a detection
    group_image: np.ndarray                # index into img_ids, per group
    iou_total: int
    gt_area: np.ndarray                    # the annotations' `area`
    gt_crowd: np.ndarray
    gt_flag: np.ndarray                    # iscrowd, or iscrowd | ignore
    gt_cat: np.ndarray                     # index into cat_ids
    dt_score: np.ndarray
    dt_cat: np.ndarray
    dt_rank: np.ndarray
    gt_shapes: list                        # per GT: counts as an int64 array (segm) or [x,y,w,h] (bbox)
    dt_shapes: list
    sizes: list                            # (H, W) per image of img_ids (segm)


def prepare(gt: dict, dt: Sequence[dict], iou_type: str = "segm", params: Optional[Params] = None) -> Problem:
    """COCOeval._prepare and the grouping of computeIoU, on the host.  Raises ValueError naming the reason for a detection
    whose image or category the ground truth does not know, and (segm) for an RLE whose size differs from its image's or
    whose counts do not sum to H*W."""
    if iou_type not in ("segm", "bbox"):
        raise ValueError(f"iou_type {iou_type!r}: 'segm' or 'bbox'")
    params = params or Params()
    max_dets = [int(m) for m in params.max_dets]
    if not max_dets or sorted(max_dets) != max_dets or max_dets[0] < 0 or len(max_dets) > _lib.PGR_COCO_MAX_MAXDETS:
        raise ValueError(f"max_dets {params.max_dets}: 1..{_lib.PGR_COCO_MAX_MAXDETS} ascending values")
    if len(params.area_rng) != len(params.area_rng_lbl):
        raise ValueError("area_rng and area_rng_lbl differ in length")
    if len(params.area_rng) * len(params.iou_thrs) > _lib.PGR_COCO_MAX_LANES or not len(params.iou_thrs) or not len(params.area_rng):
        raise ValueError(f"at least one and at most {_lib.PGR_COCO_MAX_LANES} (area range, IoU threshold) pairs")
    known_imgs = {int(i["id"]): i for i in gt["images"]}
    known_cats = {int(c["id"]) for c in gt["categories"]}
    img_ids = sorted(known_imgs) if params.img_ids is None else sorted({int(i) for i in params.img_ids})
    cat_ids = sorted(known_cats) if params.cat_ids is None else sorted({int(c) for c in params.cat_ids})
    img_at, cat_at = {v: k for k, v in enumerate(img_ids)}, {v: k for k, v in enumerate(cat_ids)}
    sizes = [(int(known_imgs[i]["height"]), int(known_imgs[i]["width"])) if i in known_imgs else (0, 0) for i in img_ids]
    key = "segmentation" if iou_type == "segm" else "bbox"

    def shape_of(entry, what, image):
        if iou_type == "bbox":
            box = [float(v) for v in entry["bbox"]]
            if len(box) != 4:
                raise ValueError(f"{what}: bbox must be [x, y, w, h]")
            return box
        seg = entry.get(key)
        if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
            raise ValueError(f"{what}: segmentation must be an RLE dict with counts and size")
        size = (int(seg["size"][0]), int(seg["size"][1]))
        if size != sizes[image]:
            raise ValueError(f"{what}: RLE size {list(size)} differs from its image's {list(sizes[image])}")
        return rle_counts(seg["counts"], size, f"{what}: RLE counts", rle_string_decode)

    gi, gc, garea, gcrowd, gflag, gshape = [], [], [], [], [], []
    for n, a in enumerate(gt["annotations"]):
        i, c = int(a["image_id"]), int(a["category_id"])
        if i not in known_imgs or c not in known_cats:
            raise ValueError(f"annotation {a.get('id', n)}: image {i} or category {c} is not in the ground truth")
        if i not in img_at or c not in cat_at:
            continue
        crowd = int(a.get("iscrowd", 0)) != 0
        gi.append(img_at[i]); gc.append(cat_at[c]); garea.append(float(a["area"])); gcrowd.append(crowd)
        gflag.append(crowd or (params.use_ignore_field and bool(a.get("ignore", 0))))
        gshape.append(shape_of(a, f"annotation {a.get('id', n)}", img_at[i]))
    di, dc, dscore, dshape = [], [], [], []
    for n, d in enumerate(dt):
        i, c = int(d["image_id"]), int(d["category_id"])
        if i not in known_imgs:
            raise ValueError(f"detection {n}: image_id {i} is not in the ground truth")
        if c not in known_cats:
            raise ValueError(f"detection {n}: category_id {c} is not in the ground truth")
        if i not in img_at or c not in cat_at:
            continue
        di.append(img_at[i]); dc.append(cat_at[c]); dscore.append(float(d["score"]))
        dshape.append(shape_of(d, f"detection {n}", img_at[i]))
    gi, gc, di, dc = (np.asarray(v, np.int64) for v in (gi, gc, di, dc))
    dscore = np.asarray(dscore, np.float64)
    K = max(len(cat_ids), 1)
    g_order = np.argsort(gi * K + gc, kind="mergesort")
    d_order = np.lexsort((-dscore, di * K + dc)) if len(di) else np.zeros(0, np.int64)      # lexsort is stable
    g_key, d_key = (gi * K + gc)[g_order], (di * K + dc)[d_order]
    # rank inside the group, then the cut to maxDets[-1]
    first = np.r_[True, d_key[1:] != d_key[:-1]] if len(d_key) else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(len(d_key)), 0)) if len(d_key) else np.zeros(0, np.int64)
    rank = np.arange(len(d_key)) - start
    keep = rank < max_dets[-1]
    d_order, d_key, rank = d_order[keep], d_key[keep], rank[keep]
    keys = np.union1d(g_key, d_key)
    groups = np.zeros(len(keys), GROUP_DTYPE)
    groups["gt_begin"] = np.searchsorted(g_key, keys, "left")
    groups["gt_count"] = np.searchsorted(g_key, keys, "right") - groups["gt_begin"]
    groups["dt_begin"] = np.searchsorted(d_key, keys, "left")
    groups["dt_count"] = np.searchsorted(d_key, keys, "right") - groups["dt_begin"]
    cells = groups["dt_count"].astype(np.int64) * groups["gt_count"]
    groups["iou_offset"] = np.cumsum(cells) - cells
    take = lambda seq, order: [seq[k] for k in order]
    return Problem(iou_type, params, img_ids, cat_ids, groups, (keys // K).astype(np.int64), int(cells.sum()),
                   np.asarray(garea, np.float64)[g_order], np.asarray(gcrowd, np.uint8)[g_order],
                   np.asarray(gflag, np.uint8)[g_order], gc[g_order].astype(np.int32), dscore[d_order],
                   dc[d_order].astype(np.int32), rank.astype(np.int32), take(gshape, g_order), take(dshape, d_order), sizes)


def npig(prob: Problem) -> np.ndarray:
    """int32 [K,A]: the GT of each category that are not ignored for each area range."""
    rng = np.asarray(prob.params.area_rng, np.float64).reshape(-1, 2)
    out = np.zeros((len(prob.cat_ids), len(rng)), np.int32)
    for a, (lo, hi) in enumerate(rng):
        counted = (prob.gt_flag == 0) & ~(prob.gt_area < lo) & ~(prob.gt_area > hi)
        np.add.at(out[:, a], prob.gt_cat[counted], 1)
    return out


# ---- the device calls -------------------------------------------------------------------------------------------------
def _device(device):
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("coco_eval needs a HIP device; there is no CPU path")
    return dev


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _groups(groups) -> np.ndarray:
    """A group table as GROUP_DTYPE: that already, or rows (dt_begin, dt_count, gt_begin, gt_count[, iou_offset]); without the
    last column the matrices follow each other."""
    if isinstance(groups, np.ndarray) and groups.dtype == GROUP_DTYPE:
        return np.ascontiguousarray(groups)
    rows = np.asarray(groups, np.int64).reshape(len(groups), -1)
    if rows.shape[1] not in (4, 5):
        raise ValueError("groups: rows of (dt_begin, dt_count, gt_begin, gt_count[, iou_offset])")
    out = np.zeros(len(rows), GROUP_DTYPE)
    for k, name in enumerate(("dt_begin", "dt_count", "gt_begin", "gt_count")):
        out[name] = rows[:, k]
    cells = rows[:, 1] * rows[:, 3]
    out["iou_offset"] = rows[:, 4] if rows.shape[1] == 5 else np.cumsum(cells) - cells
    return out


def _group_ptr(groups: np.ndarray):
    return groups.ctypes.data_as(C.POINTER(_lib.PgrCocoGroup))


def _iou_total(groups: np.ndarray) -> int:
    if not len(groups):
        return 0
    return int((groups["iou_offset"] + groups["dt_count"].astype(np.int64) * groups["gt_count"]).max())


def _rle_iou_call(dt_lists, gt_lists, crowd, size, groups, iou_total, inter, iou, dev):
    """pgr_rle_iou over host count lists of ONE image size, as ``coco.rle_counts`` checked them against it; fills the groups'
    cells of ``inter`` / ``iou`` and returns (dt_area, gt_area) int64 on the device."""
    import torch
    H, W = size
    dc, do, dtot = rle_flatten(dt_lists, dev)
    gc, go, gtot = rle_flatten(gt_lists, dev)
    crowd_dev = _to_dev(np.asarray(crowd, np.uint8), dev)
    dt_area = torch.empty(len(dt_lists), dtype=torch.int64, device=dev)
    gt_area = torch.empty(len(gt_lists), dtype=torch.int64, device=dev)
    ws = _lib.workspace("pgr_rle_iou", dev, len(groups), dtot, gtot)
    _lib.call("pgr_rle_iou", dev, _lib.ptr(dc), _lib.ptr(do), len(dt_lists), dtot, _lib.ptr(gc), _lib.ptr(go), len(gt_lists),
              gtot, _lib.ptr(crowd_dev), W, H, _group_ptr(groups), len(groups), iou_total, _lib.ptr(inter), _lib.ptr(iou),
              _lib.ptr(dt_area), _lib.ptr(gt_area), _lib.ptr(ws), ws.numel())
    return dt_area, gt_area


def rle_ious(dt_rles, gt_rles, groups, crowd=None, size=None, device="cuda"):
    """Mask IoU inside groups, from run lists: ``dt_rles`` / ``gt_rles`` are segmentation dicts or count lists (or compressed
    strings) of one image size, ``groups`` rows of (dt_begin, dt_count, gt_begin, gt_count[, iou_offset]), ``crowd`` one flag
    per GT.  Returns device tensors (iou float64 [total], inter int64 [total], dt_area int64, gt_area int64); a group's
    matrix is ``iou[iou_offset:][:dt_count * gt_count].reshape(dt_count, gt_count)``."""
    import torch
    dev = _device(device)
    both, size = rle_lists(list(dt_rles) + list(gt_rles), size, rle_string_decode)
    dt_lists, gt_lists = both[:len(dt_rles)], both[len(dt_rles):]
    groups = _groups(groups)
    crowd = np.zeros(len(gt_lists), np.uint8) if crowd is None else np.asarray(crowd, np.uint8)
    if len(crowd) != len(gt_lists):
        raise ValueError("one crowd flag per ground-truth mask")
    total = _iou_total(groups)
    inter = torch.zeros(total, dtype=torch.int64, device=dev)
    iou = torch.zeros(total, dtype=torch.float64, device=dev)
    dt_area, gt_area = _rle_iou_call(dt_lists, gt_lists, crowd, size, groups, total, inter, iou, dev)
    return iou, inter, dt_area, gt_area


def box_ious(dt_boxes, gt_boxes, groups, crowd=None, device="cuda"):
    """Box IoU inside groups: boxes [n,4] = x, y, w, h (float64).  Returns the device tensor iou float64 [total]."""
    import torch
    dev = _device(device)
    d, g = (_to_dev(np.asarray(b, np.float64).reshape(-1, 4), dev) for b in (dt_boxes, gt_boxes))
    groups = _groups(groups)
    crowd = np.zeros(len(g), np.uint8) if crowd is None else np.asarray(crowd, np.uint8)
    if len(crowd) != len(g):
        raise ValueError("one crowd flag per ground-truth box")
    crowd_dev = _to_dev(crowd, dev)
    total = _iou_total(groups)
    iou = torch.zeros(total, dtype=torch.float64, device=dev)
    ws = _lib.workspace("pgr_box_iou", dev, len(groups))
    _lib.call("pgr_box_iou", dev, _lib.ptr(d), len(d), _lib.ptr(g), len(g), _lib.ptr(crowd_dev), _group_ptr(groups), len(groups),
              total, _lib.ptr(iou), _lib.ptr(ws), ws.numel())
    return iou


def problem_ious(prob: Problem, device="cuda"):
    """Stage 1: (iou float64 [iou_total], dt_area float64 [n_dt]) on the device.  Masks go to pgr_rle_iou one image size at a
    time (a call takes one H x W); a detection's area is its set pixels (segm) or w*h (bbox)."""
    import torch
    dev = _device(device)
    if prob.iou_type == "bbox":
        iou = box_ious(prob.dt_shapes, prob.gt_shapes, prob.groups, prob.gt_crowd, dev)
        boxes = np.asarray(prob.dt_shapes, np.float64).reshape(-1, 4)
        return iou, torch.from_numpy(boxes[:, 2] * boxes[:, 3]).to(dev)
    inter = torch.zeros(prob.iou_total, dtype=torch.int64, device=dev)
    iou = torch.zeros(prob.iou_total, dtype=torch.float64, device=dev)
    dt_area = torch.zeros(len(prob.dt_shapes), dtype=torch.float64, device=dev)
    group_size = [prob.sizes[i] for i in prob.group_image]
    for size in sorted(set(group_size)):
        sel = np.flatnonzero([s == size for s in group_size])
        sub = prob.groups[sel].copy()
        d_idx = np.concatenate([np.arange(g["dt_begin"], g["dt_begin"] + g["dt_count"]) for g in sub]).astype(np.int64)
        g_idx = np.concatenate([np.arange(g["gt_begin"], g["gt_begin"] + g["gt_count"]) for g in sub]).astype(np.int64)
        sub["dt_begin"] = np.cumsum(sub["dt_count"]) - sub["dt_count"]
        sub["gt_begin"] = np.cumsum(sub["gt_count"]) - sub["gt_count"]
        a_d, _ = _rle_iou_call([prob.dt_shapes[k] for k in d_idx], [prob.gt_shapes[k] for k in g_idx], prob.gt_crowd[g_idx],
                               size, sub, prob.iou_total, inter, iou, dev)
        dt_area[torch.from_numpy(d_idx).to(dev)] = a_d.to(torch.float64)
    return iou, dt_area


def problem_match(prob: Problem, iou, dt_area, device="cuda"):
    """Stage 2: pgr_coco_match.  Returns (dt_match int32 [A,T,n_dt], dt_ignore uint8 [A,T,n_dt], gt_match int32 [A,T,n_gt],
    gt_ignore uint8 [A,n_gt]) on the device."""
    import torch
    dev = _device(device)
    P = prob.params
    thr = np.ascontiguousarray(P.iou_thrs, np.float64)
    rng = np.ascontiguousarray(np.asarray(P.area_rng, np.float64).reshape(-1, 2))
    A, T, n_dt, n_gt = len(rng), len(thr), len(prob.dt_score), len(prob.gt_area)
    gt_area, gt_flag, gt_crowd = (_to_dev(a, dev) for a in (prob.gt_area, prob.gt_flag, prob.gt_crowd))
    dt_match = torch.full((A, T, n_dt), -1, dtype=torch.int32, device=dev)
    dt_ignore = torch.zeros((A, T, n_dt), dtype=torch.uint8, device=dev)
    gt_match = torch.full((A, T, n_gt), -1, dtype=torch.int32, device=dev)
    gt_ignore = torch.zeros((A, n_gt), dtype=torch.uint8, device=dev)
    ws = _lib.workspace("pgr_coco_match", dev, len(prob.groups), n_gt, A)
    _lib.call("pgr_coco_match", dev, _group_ptr(prob.groups), len(prob.groups), prob.iou_total, _lib.ptr(iou), _lib.ptr(dt_area),
              n_dt, _lib.ptr(gt_area), _lib.ptr(gt_flag), _lib.ptr(gt_crowd), n_gt, thr.ctypes.data_as(C.POINTER(C.c_double)), T,
              rng.ctypes.data_as(C.POINTER(C.c_double)), A, _lib.ptr(dt_match), _lib.ptr(dt_ignore), _lib.ptr(gt_match),
              _lib.ptr(gt_ignore), _lib.ptr(ws), ws.numel())
    return dt_match, dt_ignore, gt_match, gt_ignore


def problem_accumulate(prob: Problem, dt_match, dt_ignore, device="cuda"):
    """Stage 3: the stable order by (category, -score) with torch.sort, then pgr_coco_accumulate.  Returns (precision
    [T,R,K,A,M], scores [T,R,K,A,M], recall [T,K,A,M]) float64 on the device."""
    import torch
    dev = _device(device)
    P = prob.params
    A, T, R, M, K = len(P.area_rng), len(P.iou_thrs), len(P.rec_thrs), len(P.max_dets), len(prob.cat_ids)
    n_dt = len(prob.dt_score)
    score, cat, rank = (_to_dev(a, dev) for a in (prob.dt_score, prob.dt_cat.astype(np.int64), prob.dt_rank))
    by_score = torch.sort(-score, stable=True).indices
    perm = by_score[torch.sort(cat[by_score], stable=True).indices].contiguous()
    seg = np.zeros(K + 1, np.int64)
    np.cumsum(np.bincount(prob.dt_cat, minlength=K)[:K], out=seg[1:])
    seg_dev, npig_dev, rec = (_to_dev(a, dev) for a in (seg, npig(prob), np.asarray(P.rec_thrs, np.float64)))
    max_dets = (C.c_int32 * M)(*[int(m) for m in P.max_dets])
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    scores = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
    ws = _lib.workspace("pgr_coco_accumulate", dev, n_dt, A, M)
    _lib.call("pgr_coco_accumulate", dev, _lib.ptr(perm), _lib.ptr(seg_dev), K, _lib.ptr(rank), _lib.ptr(dt_match),
              _lib.ptr(dt_ignore), _lib.ptr(score), n_dt, _lib.ptr(npig_dev), max_dets, M, _lib.ptr(rec), R, T, A,
              _lib.ptr(precision), _lib.ptr(scores), _lib.ptr(recall), _lib.ptr(ws), ws.numel())
    return precision, scores, recall


def evaluate(gt: dict, dt: Sequence[dict], iou_type: str = "segm", params: Optional[Params] = None, device="cuda") -> CocoScores:
    """COCOeval(gt, dt, iou_type).evaluate(); accumulate(); summarize().  ``gt``: a COCO dict (images, annotations,
    categories); ``dt``: result dicts (image_id, category_id, score and ``bbox`` or an RLE ``segmentation`` whose counts are
    a list or a compressed string)."""
    prob = prepare(gt, dt, iou_type, params)
    iou, dt_area = problem_ious(prob, device)
    dt_match, dt_ignore, _, _ = problem_match(prob, iou, dt_area, device)
    precision, scores, recall = (t.cpu().numpy() for t in problem_accumulate(prob, dt_match, dt_ignore, device))
    return CocoScores(precision, recall, scores, summarize(precision, recall, prob.params), prob.params)


# ---- the BOP22 files ------------------------------------------------------------------------------------------------------
def write_results(path, results) -> None:
    """``inout.save_coco_results`` (bop22): ``results`` are dicts with scene_id, im_id, obj_id, score and optionally bbox,
    segmentation, run_time."""
    out = [{"scene_id": int(r["scene_id"]), "image_id": int(r["im_id"]), "category_id": int(r["obj_id"]),
            "score": float(r["score"]), "bbox": list(r["bbox"]) if "bbox" in r else [],
            "segmentation": r["segmentation"] if "segmentation" in r else {}, "time": r["run_time"] if "run_time" in r else -1}
           for r in results]
    Path(path).write_text(json.dumps(out))


def results_from_gt(dataset_dir, split: str = "train", bbox_type: str = "amodal", score: float = 1.0) -> list:
    """The dataset's own scene_gt_coco annotations as ``write_results`` input: every annotation a detection of ``score``."""
    out = []
    for scene in BD.scene_dirs(dataset_dir, split, coco_file_name(bbox_type)):
        doc = BD.BopScene(scene).read_json(coco_file_name(bbox_type))
        out += [{"scene_id": int(scene.name), "im_id": a["image_id"], "obj_id": a["category_id"], "score": score,
                 "bbox": a["bbox"], "segmentation": a["segmentation"], "run_time": 0.0} for a in doc["annotations"]]
    return out


def merge_scenes(scenes: Sequence[tuple]):
    """``pycoco_utils.merge_coco_annotations`` / ``merge_coco_results`` over (scene_coco dict, scene results) pairs, in order:
    the image ids of a later scene are shifted by max id + 1 of what is merged so far, its annotation ids by the largest
    annotation id + 1 (0 without annotations), its detections follow their images.  Returns (gt dict, results, offsets)."""
    merged, results, offsets = None, [], []
    for doc, res in scenes:
        doc = {**doc, "images": [dict(i) for i in doc["images"]], "annotations": [dict(a) for a in doc["annotations"]],
               "categories": [dict(c) for c in doc["categories"]]}
        res = [dict(r) for r in res]
        if merged is None:
            merged, offset = doc, 0
        else:
            for c in doc["categories"]:
                if c not in merged["categories"]:
                    merged["categories"].append(c)
            offset = max(i["id"] for i in merged["images"]) + 1
            ann_offset = max(a["id"] for a in merged["annotations"]) + 1 if merged["annotations"] else 0
            for i in doc["images"]:
                i["id"] += offset
            for a in doc["annotations"]:
                a["id"] += ann_offset
                a["image_id"] += offset
            for r in res:
                r["image_id"] += offset
            merged["images"] += doc["images"]
            merged["annotations"] += doc["annotations"]
        results += res
        offsets.append(offset)
    return merged, results, offsets


def average_time_per_image(results: Sequence[dict]) -> float:
    """The toolkit's rule: -1 if any result has ``time`` < 0; an error when two results of one image differ by more than
    0.001; else the mean over images."""
    times = {}
    for r in results:
        k = (int(r["scene_id"]), int(r["image_id"]))
        if r["time"] < 0:
            return -1.0
        if k in times:
            if abs(times[k] - r["time"]) > 0.001:
                raise ValueError(f"The running time for scene {k[0]} and image {k[1]} is not the same for all estimates.")
        else:
            times[k] = r["time"]
    return float(np.mean(list(times.values())))


def scores_file_name(ann_type: str, bbox_type: str = "amodal") -> str:
    return f"scores_bop22_coco_{ann_type}{'_modal' if ann_type == 'bbox' and bbox_type == 'modal' else ''}.json"


def load_dataset(results, dataset_dir, ann_type="segm", bbox_type="amodal", targets=None, split="train"):
    """Lines 96-139 of eval_bop22_coco.py on the host: (merged gt dict, merged results).  ``results``: the loaded results
    list; ``targets``: a test_targets_bop19.json-style list (scene_id, im_id) or None for every image of every scene."""
    if ann_type not in ("segm", "bbox") or bbox_type not in ("amodal", "modal"):
        raise ValueError(f"ann_type {ann_type!r} / bbox_type {bbox_type!r}")
    root = Path(dataset_dir) / split
    per_scene = {}
    for r in results:
        if (ann_type == "bbox" and r.get("bbox")) or (ann_type == "segm" and r.get("segmentation")):
            per_scene.setdefault(int(r["scene_id"]), []).append(r)
    name = coco_file_name(bbox_type if ann_type == "bbox" else "amodal")
    if targets is None:
        wanted = {int(p.name): None for p in BD.scene_dirs(dataset_dir, split, name) if p.name.isdigit()}
    else:
        wanted = {}
        for t in targets:
            wanted.setdefault(int(t["scene_id"]), set()).add(int(t["im_id"]))
    scenes = []
    for sid, ims in wanted.items():
        path = BD.scene_dir(dataset_dir, split, sid) / name
        if not path.exists():
            raise FileNotFoundError(f"{path} is missing (python -m pegasus_amd.coco writes it)")
        doc = json.loads(path.read_text())
        res = per_scene.get(sid, [])
        if ims is not None:
            doc["images"] = [i for i in doc["images"] if i["id"] in ims]
            doc["annotations"] = [a for a in doc["annotations"] if a["image_id"] in ims]
            res = [r for r in res if r["image_id"] in ims]
        scenes.append((doc, res))
    if not scenes:
        raise ValueError(f"no scene with {name} under {root}")
    gt, dt, _ = merge_scenes(scenes)
    return gt, dt


def evaluate_dataset(results_path, dataset_dir, ann_type="segm", bbox_type="amodal", targets=None, split="train",
                     params: Optional[Params] = None, out=None, device="cuda") -> dict:
    """scripts/eval_bop22_coco.py for one results file: the twelve scores and ``average_time_per_image``, written to
    ``<out>/scores_bop22_coco_<ann_type>[_modal].json`` (``out`` None: beside the results file).  ``targets``: a path or a
    loaded list."""
    results = json.loads(Path(results_path).read_text())
    if isinstance(targets, (str, Path)):
        targets = json.loads(Path(targets).read_text())
    gt, dt = load_dataset(results, dataset_dir, ann_type, bbox_type, targets, split)
    scores = evaluate(gt, dt, ann_type, params, device).as_dict()
    scores["average_time_per_image"] = average_time_per_image(results)
    out = Path(results_path).parent if out is None else Path(out)
    out.mkdir(parents=True, exist_ok=True)
    (out / scores_file_name(ann_type, bbox_type)).write_text(json.dumps(scores))
    return scores


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.coco_eval", description=__doc__.split("\n\n")[0])
    p.add_argument("--results", required=True, help="BOP22 COCO results: scene_id, image_id, category_id, score, bbox, segmentation, time")
    p.add_argument("--dataset", required=True)
    p.add_argument("--split", default="train")
    p.add_argument("--ann_type", default="segm", choices=["segm", "bbox"])
    p.add_argument("--bbox_type", default="amodal", choices=["amodal", "modal"])
    p.add_argument("--targets", default=None, help="test_targets_bop19.json-style list; default: every image")
    p.add_argument("--use_ignore_field", action="store_true", help="also ignore GT whose `ignore` is set (COCOeval does not)")
    p.add_argument("--out", default=None, help="where the scores file is written; default: beside the results")
    a = p.parse_args(argv)
    scores = evaluate_dataset(a.results, a.dataset, a.ann_type, a.bbox_type, a.targets, a.split,
                              Params(use_ignore_field=a.use_ignore_field), a.out)
    for k, v in scores.items():
        print(f"{k}: {v:.4f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
