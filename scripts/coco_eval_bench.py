"""Times pegasus_amd.coco_eval.evaluate against the path it replaces.

    python scripts/coco_eval_bench.py [--images 1000] [--gt 8] [--dt 30] [--width 640] [--height 480] [--repeats 5]
                                      [--host-repeats 5]

A seeded synthetic set: per image --gt ellipses over 10 categories and about --dt detections (perturbed copies of the ground
truth and false positives), as run lists and boxes.
  device   evaluate(gt, dt, type): the host-side grouping, the uploads, the four device stages, the copy of the tables back
           and the twelve means, host clock until everything has arrived; and the stages alone between device events
  host     tests/coco_eval_reference.py: the NumPy / Python restatement of COCOeval that decodes masks to pixels
Warm, the median of the repeats each with the range; the two results are compared for equality first.  Prints one JSON line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def ellipse_runs(H, W, cx, cy, rx, ry):
    """(run list in column-major order, [x, y, w, h], area) of a filled ellipse; one set run per column it crosses, with a
    zero-length run between neighbours where a column is filled to its ends (legal anywhere)."""
    xs = np.arange(max(int(np.ceil(cx - rx)), 0), min(int(np.floor(cx + rx)), W - 1) + 1)
    half = ry * np.sqrt(np.maximum(1.0 - ((xs - cx) / rx) ** 2, 0.0))
    y0, y1 = np.maximum(np.ceil(cy - half), 0).astype(np.int64), np.minimum(np.floor(cy + half), H - 1).astype(np.int64)
    keep = y0 <= y1
    xs, y0, y1 = xs[keep], y0[keep], y1[keep]
    if not len(xs):
        return [H * W], [0.0, 0.0, 0.0, 0.0], 0
    start, stop = xs * H + y0, xs * H + y1 + 1
    edges = np.stack([start, stop], 1).reshape(-1)
    counts = np.diff(np.r_[0, edges, H * W])
    area = int((stop - start).sum())
    return counts.tolist(), [float(xs[0]), float(y0.min()), float(xs[-1] - xs[0] + 1), float(y1.max() - y0.min() + 1)], area


def synthetic(n_images, n_gt, n_dt, W, H, seed=5):
    rng = np.random.default_rng(seed)
    gt = {"images": [], "annotations": [], "categories": [{"id": c} for c in range(1, 11)]}
    dt = []
    for image_id in range(1, n_images + 1):
        gt["images"].append({"id": image_id, "width": W, "height": H})
        shapes = []
        for _ in range(n_gt):
            e = (rng.uniform(0, W), rng.uniform(0, H), rng.uniform(8, W / 5), rng.uniform(8, H / 5))
            cat = int(rng.integers(1, 11))
            counts, box, area = ellipse_runs(H, W, *e)
            if area == 0:
                continue
            shapes.append((e, cat))
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": image_id, "category_id": cat, "iscrowd": int(rng.random() < 0.03),
                                      "area": area, "bbox": box, "segmentation": {"counts": counts, "size": [H, W]},
                                      "ignore": bool(rng.random() < 0.1)})
        for _ in range(int(rng.poisson(n_dt))):
            if shapes and rng.random() < 0.8:
                (cx, cy, rx, ry), cat = shapes[int(rng.integers(0, len(shapes)))]
                e = (cx + rng.normal(0, 0.15 * rx), cy + rng.normal(0, 0.15 * ry), rx * rng.uniform(0.8, 1.2), ry * rng.uniform(0.8, 1.2))
            else:
                e, cat = (rng.uniform(0, W), rng.uniform(0, H), rng.uniform(8, W / 5), rng.uniform(8, H / 5)), int(rng.integers(1, 11))
            counts, box, area = ellipse_runs(H, W, *e)
            dt.append({"image_id": image_id, "category_id": cat, "score": float(rng.random()), "bbox": box,
                       "segmentation": {"counts": counts, "size": [H, W]}})
    return gt, dt


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--gt", type=int, default=8)
    ap.add_argument("--dt", type=int, default=30)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import coco_eval_reference as CR
    from pegasus_amd import coco_eval as CE
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    gt, dt = synthetic(a.images, a.gt, a.dt, a.width, a.height)
    out = {"images": a.images, "annotations": len(gt["annotations"]), "detections": len(dt), "width": a.width, "height": a.height,
           "runs": int(sum(len(r["segmentation"]["counts"]) for r in dt) + sum(len(r["segmentation"]["counts"]) for r in gt["annotations"])),
           "repeats": a.repeats, "host_repeats": a.host_repeats}

    def timed(fn, repeats):
        fn()                                                       # warm
        times = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return res, times

    def stages(prob):
        """ms between device events: IoU (with its uploads), matching, the sort and the accumulation."""
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        marks[0].record()
        iou, dt_area = CE.problem_ious(prob)
        marks[1].record()
        dt_match, dt_ignore, _, _ = CE.problem_match(prob, iou, dt_area)
        marks[2].record()
        CE.problem_accumulate(prob, dt_match, dt_ignore)
        marks[3].record()
        marks[3].synchronize()
        return [marks[k].elapsed_time(marks[k + 1]) for k in range(3)]

    for iou_type in ("segm", "bbox"):
        got, t_dev = timed(lambda: CE.evaluate(gt, dt, iou_type), a.repeats)
        ref, t_host = timed(lambda: CR.evaluate(gt, dt, iou_type), a.host_repeats)
        for key in ("precision", "recall", "scores", "stats"):
            assert getattr(got, key).tobytes() == np.ascontiguousarray(ref[key], np.float64).tobytes(), f"{iou_type}: {key} differs"
        t0 = time.perf_counter()
        prob = CE.prepare(gt, dt, iou_type)
        prepare_ms = 1e3 * (time.perf_counter() - t0)
        stages(prob)
        split = np.median([stages(prob) for _ in range(a.repeats)], axis=0)
        out[iou_type] = {"AP": float(got.stats[0]), "iou_cells": prob.iou_total, "groups": len(prob.groups),
                         "device_evaluate_ms_median": statistics.median(t_dev), "device_evaluate_ms_all": t_dev,
                         "host_prepare_ms": prepare_ms, "events_ms_iou_match_accumulate": [float(v) for v in split],
                         "host_reference_ms_median": statistics.median(t_host), "host_reference_ms_all": t_host}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
