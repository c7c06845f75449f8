"""Times the BOP pose errors on the GPU against their float64 NumPy restatement on the CPU (not part of bench.py).

    python scripts/pose_error_bench.py [--pairs 4096] [--vertices 5000 20000] [--symmetries 1 8 630] [--cpu-pairs 2]

For every V x S: one object of V random model points (millimetres) with S symmetry transforms (the identity and S - 1
rotations about one axis), P (estimate, ground truth) pairs with small pose errors.  The models and the job inputs are
built once.  pose_errors(mssd, mspd, add, proj, re, te: one pgr_pose_errors call) and pose_errors(adi: one pgr_pose_adi
call, once per V) are timed with a hipEvent pair around the whole Python call (job array, launches, read-back), the median
of 5 repeats after 2 warm-up calls.  The CPU figure runs tests/pose_error_reference.errors_f64 / adi_f64 (the stand-in for
the toolkit, which it equals to 1e-9) on the first --cpu-pairs pairs, one thread.

One JSON line per shape: pairs per second on the GPU and on the CPU, and the kernels' lane-operation rate against the VALU
peak of 78.6 T lane-operations/s (half the 157.3 TFLOPS of FP32 FMA: 32 lanes per clock per SIMD).  Operations are
counted from the source statements: 24 per vertex for the estimate (18 for the point, 6 for the projection), 39 per (vertex,
symmetry) (18 point, 8 distance, 6 projection, 5 pixel distance, 2 maxima), 9 per (query, point) for ADI; a symmetry slot
that a chunk leaves unused is computed too and is not counted."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

VALU_PEAK = 78.6e12
OPS_PER_VERTEX, OPS_PER_VERTEX_SYM, OPS_PER_ADI_PAIR = 24, 39, 9
WARMUP, REPEATS = 2, 5


def rotation(axis, angle):
    d = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * k.dot(k)


def inputs(V, S, P, seed):
    rng = np.random.default_rng(seed)
    pts = (rng.normal(size=(V, 3)) * np.array([40.0, 25.0, 60.0])).astype(np.float32)
    syms = [dict(R=rotation((0, 0, 1), 2 * np.pi * s / S), t=np.zeros((3, 1))) for s in range(S)]
    R_gt = np.stack([rotation(rng.normal(size=3), rng.uniform(0, np.pi)) for _ in range(P)])
    t_gt = np.stack([rng.uniform(-150, 150, P), rng.uniform(-100, 100, P), rng.uniform(500, 1400, P)], axis=1)
    R_est = np.stack([rotation(rng.normal(size=3), rng.uniform(0, 0.1)).dot(R) for R in R_gt])
    t_est = t_gt + rng.normal(0, 3.0, (P, 3))
    return pts, syms, R_est, t_est, R_gt, t_gt


def gpu_seconds(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--vertices", type=int, nargs="+", default=[5000, 20000])
    ap.add_argument("--symmetries", type=int, nargs="+", default=[1, 8, 630])
    ap.add_argument("--cpu-pairs", type=int, default=2)
    a = ap.parse_args()
    import pose_error_reference as PR
    from pegasus_amd import pose_error as PE
    K = np.array([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]])
    P = a.pairs
    main_errors = ("mssd", "mspd", "add", "proj", "re", "te")
    for V in a.vertices:
        for n, S in enumerate(a.symmetries):
            pts, syms, R_est, t_est, R_gt, t_gt = inputs(V, S, P, 7 * V + S)
            models = PE.PoseErrorModels.from_points(pts, syms)
            obj = np.zeros(P, np.int64)
            sec = gpu_seconds(lambda: PE.pose_errors(models, obj, R_est, t_est, R_gt, t_gt, K, main_errors))
            sym_R = np.stack([s["R"] for s in syms])
            sym_t = np.stack([s["t"].reshape(3) for s in syms])
            t0 = time.perf_counter()
            for p in range(a.cpu_pairs):
                PR.errors_f64(pts, sym_R, sym_t, R_est[p], t_est[p], R_gt[p], t_gt[p], K)
            cpu = (time.perf_counter() - t0) / a.cpu_pairs
            ops = P * V * (OPS_PER_VERTEX + OPS_PER_VERTEX_SYM * S)
            print(json.dumps(dict(call="pose_errors", V=V, S=S, P=P, gpu_ms=round(sec * 1e3, 3), gpu_pairs_per_s=round(P / sec, 1),
                                  cpu_pairs_per_s=round(1.0 / cpu, 3), speedup=round(cpu * P / sec, 1),
                                  lane_ops_per_s=float(f"{ops / sec:.4g}"), valu_peak_fraction=round(ops / sec / VALU_PEAK, 4))), flush=True)
            if n == 0:
                sec = gpu_seconds(lambda: PE.pose_errors(models, obj, R_est, t_est, R_gt, t_gt, None, ("adi",)))
                t0 = time.perf_counter()
                for p in range(a.cpu_pairs):
                    PR.adi_f64(pts, R_est[p], t_est[p], R_gt[p], t_gt[p])
                cpu = (time.perf_counter() - t0) / a.cpu_pairs
                ops = P * V * V * OPS_PER_ADI_PAIR
                print(json.dumps(dict(call="adi", V=V, P=P, gpu_ms=round(sec * 1e3, 3), gpu_pairs_per_s=round(P / sec, 1),
                                      cpu_pairs_per_s=round(1.0 / cpu, 3), speedup=round(cpu * P / sec, 1),
                                      lane_ops_per_s=float(f"{ops / sec:.4g}"), valu_peak_fraction=round(ops / sec / VALU_PEAK, 4))),
                      flush=True)


if __name__ == "__main__":
    main()
