"""Times the registration kernels (pegasus_amd.registration) beside scipy's k-d tree doing the same queries.

    python scripts/registration_bench.py [--repeats 7] [--host-repeats 3] [--scale 1.0] [--workers 16] [--max_distance 0.02]

Two configurations on the project's synthetic scenes, positions only:
  halves_100k   the cracker-box object (scenes.scene_c2) drawn with 286 k points: the even rows above the 30 % quantile of z
                are the target, the odd rows below the 70 % quantile the source (about 100 k each), the source displaced by
                3 degrees and (3, -2, 2.5) mm
  150k_vs_2m    the 2 M-Gaussian merged scene (scenes.scene_c3) is the target, 150 k rows of its first two objects, displaced
                the same way, the source
For each:
  grid          pgr_nn_grid_build over the target                                   | cKDTree(target)
  order         pgr_nn_source_order (once per registration)
  iteration     pgr_nn_correspond + pgr_icp_sums, with the lanes in cell order and  | tree.query(posed source, 1,
                in row order, the two alternating                                   |   distance_upper_bound, workers)
  normals       estimate_normals(target, max_distance)                              | tree.query_ball_point(target, r, workers,
                                                                                    |   return_length=True): the search alone,
                                                                                    |   no covariance and no eigenvectors
Device times are milliseconds between device events around calls that warmed first; host times the host clock; the median
of the repeats with all values.  Whether the device's indices equal the tree's is reported.  Prints one JSON line (and every
case on stderr as it finishes)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def displacement():
    """3 degrees about (1.8, -1.5, 1.9) and (3, -2, 2.5) mm, as a 4x4."""
    from scipy.spatial.transform import Rotation as Rot
    T = np.eye(4)
    T[:3, :3] = Rot.from_rotvec(np.radians([1.8, -1.5, 1.9])).as_matrix()
    T[:3, 3] = (0.003, -0.002, 0.0025)
    return T


def moved(points, T):
    inv = np.linalg.inv(T)
    return (points.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks both configurations (rehearsals)")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--max_distance", type=float, default=0.02)
    a = ap.parse_args()
    import torch
    from scipy.spatial import cKDTree
    from pegasus_amd import registration, scenes
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda:0")
    pose = displacement()

    box = scenes.scene_c2(n=int(286_000 * a.scale), n_views=1)[0].xyz
    z = box[:, 2]
    top, bottom = box[0::2][z[0::2] > np.quantile(z, 0.3)], box[1::2][z[1::2] < np.quantile(z, 0.7)]
    scene = scenes.scene_c3(n_views=1, scale=a.scale)[0].xyz
    n_objects = 8 * int(80_000 * a.scale)
    configs = {"halves_100k": (moved(bottom, pose), np.ascontiguousarray(top)),
               "150k_vs_2m": (moved(scene[len(scene) - n_objects:][:int(150_000 * a.scale)], pose), np.ascontiguousarray(scene))}

    def device_ms(fns, repeats):
        """The calls of ``fns`` alternating, each warmed once: {name: [ms]}."""
        for fn in fns.values():
            fn()
        times = {k: [] for k in fns}
        for _ in range(repeats):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
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

    out = {"repeats": a.repeats, "host_repeats": a.host_repeats, "workers": a.workers, "scale": a.scale,
           "max_distance": a.max_distance, "cases": []}
    for name, (source, target) in configs.items():
        s, t = torch.from_numpy(source).to(dev), torch.from_numpy(target).to(dev)
        T = np.eye(4)
        normals = registration.estimate_normals(t, a.max_distance)
        pairs = {order: registration._Pair(s, t, a.max_distance, "bench", init=T, target_normals=normals, cell_order=order == "cells")
                 for order in ("cells", "rows")}
        cells = pairs["cells"]

        def iteration(pair):
            pair.correspond(T)
            pair.reduce(T)

        case = {"config": name, "source_points": len(source), "target_points": len(target)}
        times = device_ms({order: (lambda p=p: iteration(p)) for order, p in pairs.items()}, a.repeats)
        case["iteration_cell_order"], case["iteration_row_order"] = entry(times["cells"]), entry(times["rows"])
        times = device_ms({"correspond": lambda: cells.correspond(T), "sums": lambda: cells.reduce(T)}, a.repeats)
        case["correspond_cell_order"], case["sums"] = entry(times["correspond"]), entry(times["sums"])
        grid_ws = registration._lib.workspace("pgr_nn_grid_build", dev, len(target))
        order_ws = registration._lib.workspace("pgr_nn_source_order", dev, len(source))
        order_out = torch.empty((len(source),), dtype=torch.int32, device=dev)
        times = device_ms({
            "grid": lambda: registration._lib.call("pgr_nn_grid_build", dev, len(target), registration._lib.ptr(t), a.max_distance,
                                                   registration._lib.ptr(grid_ws), grid_ws.numel()),
            "order": lambda: registration._lib.call("pgr_nn_source_order", dev, len(source), registration._lib.ptr(s),
                                                    registration._c_matrix(T), a.max_distance, registration._lib.ptr(order_out),
                                                    registration._lib.ptr(order_ws), order_ws.numel()),
            "normals": lambda: registration.estimate_normals(t, a.max_distance)}, a.repeats)
        case["grid_build"], case["source_order"], case["normals"] = entry(times["grid"]), entry(times["order"]), entry(times["normals"])
        fitness, rmse, _ = cells.evaluate(T)
        case["fitness"], case["rmse"] = fitness, rmse
        print(json.dumps(case), file=sys.stderr, flush=True)
        # the host doing the same queries
        t64, s64 = target.astype(np.float64), source.astype(np.float64)
        tree, times = host_ms(lambda: cKDTree(t64), a.host_repeats)
        case["host_tree_build"] = entry(times)
        (_, j), times = host_ms(lambda: tree.query(s64, 1, distance_upper_bound=a.max_distance, workers=a.workers), a.host_repeats)
        case["host_query"] = entry(times)
        index = cells.index.cpu().numpy()
        case["indices_equal_host"] = bool(np.array_equal(np.where(j < len(target), j, -1), index))
        _, times = host_ms(lambda: tree.query_ball_point(t64, a.max_distance, workers=a.workers, return_length=True), 1)
        case["host_normals_search_only"] = entry(times)
        out["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
