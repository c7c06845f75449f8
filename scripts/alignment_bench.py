"""Times the ground-plane kernels (pegasus_amd.alignment) beside NumPy computing the same scores.

    python scripts/alignment_bench.py [--repeats 7] [--host-repeats 3] [--scale 1.0] [--workers 16] [--iterations 1000]
        [--out profiles/alignment_bench.json]

Two configurations on the project's synthetic merged scene (scenes.scene_c3), positions only, posed by a rotation of 40
degrees and an offset of metres so that the ground is no coordinate plane, threshold 0.01, ``--iterations`` hypotheses:
  mixed_150k   150 k rows drawn from the whole scene (ground and objects)
  env_1360k    the 1.36 M centres of the environment
For each:
  hypotheses   pgr_plane_hypotheses
  score        pgr_plane_score: every hypothesis on every point           | NumPy float64: |P n + d| < t per chunk of 16 k
  inliers      pgr_plane_inliers under the best hypothesis, with the mask  |   points, counts and sums of squares, the chunks
  fit          the whole fit_ground_plane call, host clock                 |   on ``--workers`` threads, one BLAS thread each
Device times are milliseconds between device events around calls that warmed first; host times the host clock; the median
of the repeats with all values.  Whether the device's counts equal NumPy's is reported (NumPy's matrix product does not round
as the rule does: a point within an ulp of the threshold may differ).  Prints one JSON line, writes it to ``--out``, and
prints every case on stderr as it finishes."""
import argparse
import contextlib
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

try:
    import threadpoolctl
    BLAS_PINNED = True
except ImportError:
    BLAS_PINNED = False

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CHUNK = 16384


def posed(points):
    from scipy.spatial.transform import Rotation as Rot
    R = Rot.from_rotvec(np.radians(40.0) * np.array([0.6, -0.64, 0.48])).as_matrix()
    return (points.astype(np.float64) @ R.T + np.array([2.5, -1.75, 3.25])).astype(np.float32)


def blas_single_threaded():
    """One BLAS thread inside every worker, so that ``workers`` threads run and not ``workers`` x the BLAS pool; without
    threadpoolctl nothing is pinned (BLAS_PINNED says which)."""
    return threadpoolctl.threadpool_limits(limits=1, user_api="blas") if BLAS_PINNED else contextlib.nullcontext()


def host_scores(points, planes, threshold, workers):
    """counts int64 [H], sumsq float64 [H] in NumPy float64, chunks of points on a thread pool."""
    normals, d = np.ascontiguousarray(planes[:, :3].T), planes[:, 3]

    def chunk(at):
        dist = np.abs(points[at:at + CHUNK].astype(np.float64) @ normals + d)
        inl = dist < threshold
        return inl.sum(axis=0), np.where(inl, dist * dist, 0.0).sum(axis=0)

    with blas_single_threaded(), ThreadPoolExecutor(max_workers=workers) as pool:
        parts = list(pool.map(chunk, range(0, len(points), CHUNK)))
    return sum(p[0] for p in parts), sum(p[1] for p in parts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks both configurations (rehearsals)")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "alignment_bench.json"))
    a = ap.parse_args()
    import torch
    from pegasus_amd import alignment, scenes
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda:0")
    workers = min(a.workers, 16)

    scene = scenes.scene_c3(n_views=1, scale=a.scale)[0].xyz
    n_env = int(1_360_000 * a.scale)
    rows = np.random.default_rng(5).choice(len(scene), int(150_000 * a.scale), replace=False)
    configs = {"mixed_150k": posed(scene[rows]), "env_1360k": posed(scene[:n_env])}

    def device_ms(fn, repeats):
        fn()
        times = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return times

    def host_ms(fn, repeats):
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = fn()
            times.append(1e3 * (time.perf_counter() - t0))
        return res, times

    def entry(times):
        return {"ms_median": statistics.median(times), "ms_all": times}

    out = {"repeats": a.repeats, "host_repeats": a.host_repeats, "workers": workers, "scale": a.scale, "threshold": a.threshold,
           "iterations": a.iterations, "host_blas_threads_per_worker": 1 if BLAS_PINNED else "not pinned",
           "device": torch.cuda.get_device_name(0), "cases": []}
    L, p = alignment._lib, alignment._lib.ptr
    for name, points in configs.items():
        n, h = len(points), a.iterations
        pts = torch.from_numpy(points).to(dev)
        tri = torch.from_numpy(alignment.draw_triples(n, h, 0)).to(dev)
        planes, valid = alignment.plane_hypotheses(pts, tri)
        counts = torch.empty((h,), dtype=torch.int32, device=dev)
        sumsq = torch.empty((h,), dtype=torch.float64, device=dev)
        ws = L.workspace("pgr_plane_score", dev, n, h)
        case = {"config": name, "points": n, "hypotheses": h, "valid_hypotheses": int(valid.sum())}
        case["hypotheses_ms"] = entry(device_ms(lambda: L.call("pgr_plane_hypotheses", dev, n, p(pts), h, p(tri), p(planes),
                                                              p(valid)), a.repeats))
        case["score"] = entry(device_ms(lambda: L.call("pgr_plane_score", dev, n, p(pts), h, p(planes), a.threshold, p(counts),
                                                       p(sumsq), p(ws), ws.numel()), a.repeats))
        case["score_gdist_per_s"] = n * h / case["score"]["ms_median"] * 1e-6
        best = alignment.choose_best(counts.cpu().numpy(), sumsq.cpu().numpy(), valid.cpu().numpy())
        plane = planes[best].cpu().numpy()
        pivot = points[int(tri[best, 0])].astype(np.float64)
        case["inliers"] = entry(device_ms(lambda: alignment.plane_inliers(pts, plane, pivot, a.threshold), a.repeats))
        torch.cuda.synchronize()
        fit, times = host_ms(lambda: alignment.fit_ground_plane(pts, a.threshold, h, 0), a.repeats)
        case["fit_ground_plane_host_clock"] = entry(times)
        case["fitness"], case["inlier_rmse"], case["best_count"] = fit.fitness, fit.inlier_rmse, int(counts[best])
        print(json.dumps(case), file=sys.stderr, flush=True)
        planes_host = planes.cpu().numpy()
        (host_counts, host_sumsq), times = host_ms(lambda: host_scores(points, planes_host, a.threshold, workers), a.host_repeats)
        case["host_numpy_score"] = entry(times)
        got = counts.cpu().numpy()
        case["counts_equal_host"] = bool(np.array_equal(got, host_counts))
        case["counts_largest_difference"] = int(np.abs(got - host_counts).max())
        case["sumsq_largest_relative_difference"] = float((np.abs(sumsq.cpu().numpy() - host_sumsq) /
                                                           np.maximum(host_sumsq, 1e-300)).max())
        out["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(out)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
