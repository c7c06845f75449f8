"""Times the radius-outlier filter (pegasus_amd.outliers) beside the host path it replaces.

    python scripts/outlier_bench.py [--repeats 5] [--host-repeats 5] [--scale 1.0] [--workers 16] [--no-exact]

Two of the project's synthetic scenes, positions only: the 150 k-Gaussian object (scenes.scene_c2) and the 2 M-Gaussian merged
scene (scenes.scene_c3), each at the reference's two settings (16, 0.03) and (16, 0.05), and each a second time with 8 floaters
added 50 .. 500 m away (the cost must not depend on the bounding box).
  device   radius_outlier_mask on positions already on the device: ms between device events, and the host clock around the
           call until the mask is there (its domain check reads one scalar back)
  host     what a user does today: positions to the host, scipy's cKDTree, query_ball_point(.., workers, return_length=True),
           the mask back to the device; host clock
  exact    radius_neighbor_count with cap=None, once per scene at 0.03 (the filter itself never runs it)
The device calls warm; the median of the repeats, with all values; whether the two masks are equal is reported.  Prints one
JSON line (and every case on stderr as it finishes)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SETTINGS = ((16, 0.03), (16, 0.05))


def floaters(count=8, seed=8):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(count, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(50.0, 500.0, (count, 1))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks both scenes (rehearsals)")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-exact", action="store_true")
    a = ap.parse_args()
    import torch
    from scipy.spatial import cKDTree
    from pegasus_amd import outliers, scenes
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda:0")
    clouds = {"object_150k": scenes.scene_c2(n=int(150_000 * a.scale), n_views=1)[0].xyz,
              "scene_2m": scenes.scene_c3(n_views=1, scale=a.scale)[0].xyz}

    def device_ms(fn, repeats):
        fn()                                                       # warm
        events, wall = [], []
        for _ in range(repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            res = fn()
            e1.record()
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            events.append(e0.elapsed_time(e1))
        return res, events, wall

    def host_mask(pts, nb_points, radius):
        p = pts.cpu().numpy().astype(np.float64)
        counts = cKDTree(p).query_ball_point(p, radius, workers=a.workers, return_length=True)
        return torch.from_numpy(counts > nb_points).to(pts.device)

    def host_ms(fn, repeats):                                      # (nothing to warm: every call builds its tree anew)
        times = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return res, times

    out = {"repeats": a.repeats, "host_repeats": a.host_repeats, "workers": a.workers, "scale": a.scale, "cases": []}
    for name, xyz in clouds.items():
        for with_floaters in (False, True):
            pts = torch.from_numpy(np.vstack([xyz, floaters()]) if with_floaters else np.ascontiguousarray(xyz)).to(dev)
            extent = float((pts.max(0).values - pts.min(0).values).max())
            for nb_points, radius in SETTINGS:
                mask, events, wall = device_ms(lambda: outliers.radius_outlier_mask(pts, nb_points, radius), a.repeats)
                ref, host = host_ms(lambda: host_mask(pts, nb_points, radius), a.host_repeats)
                # (scipy counts d <= r with sums of its own: equal unless a pair sits on a tie, which is reported, not hidden)
                out["cases"].append({"scene": name, "points": int(pts.shape[0]), "floaters": with_floaters, "extent_m": extent,
                                     "nb_points": nb_points, "radius": radius, "kept": int(mask.sum()),
                                     "kept_host": int(ref.sum()), "masks_equal": bool(torch.equal(mask, ref)),
                                     "device_events_ms_median": statistics.median(events), "device_events_ms_all": events,
                                     "device_wall_ms_median": statistics.median(wall), "device_wall_ms_all": wall,
                                     "host_ms_median": statistics.median(host), "host_ms_all": host})
                print(json.dumps(out["cases"][-1]), file=sys.stderr, flush=True)
            if not a.no_exact and not with_floaters:
                counts, events, _ = device_ms(lambda: outliers.radius_neighbor_count(pts, 0.03), min(a.repeats, 3))
                out.setdefault("exact", []).append({"scene": name, "radius": 0.03, "mean_count": float(counts.float().mean()),
                                                    "max_count": int(counts.max()),
                                                    "device_events_ms_median": statistics.median(events),
                                                    "device_events_ms_all": events})
                print(json.dumps(out["exact"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
