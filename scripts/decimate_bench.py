"""Times mesh decimation by vertex clustering (pegasus_amd.decimate) and what it buys the pose errors.

    python scripts/decimate_bench.py [out.json]        (default: profiles/decimate_bench.json)

Input: mesh.extract_mesh of the 40 000-Gaussian box object at grids 128 and 256.  Per grid: the voxel simplify_to finds for
ratio 0.025 (the toolkit's TargetPerc) and its count passes; pgr_mesh_cluster_count and pgr_mesh_cluster_emit at that voxel on
data already on the device, warm, the median of 5 between device events; the NumPy reference of tests/decimate_reference.py on
the same mesh and voxel (host clock) and whether the device result equals it; and for random pose pairs MSSD, ADD and ADI on
the full model against the decimated one: mean and maximum absolute difference in units of the diameter, and the two
evaluation times (wall clock, synchronised).  ADI on the full model is quadratic in the vertices: at grid 256 it runs on
ADI_PAIRS_FULL of the pairs only.  Prints every stage as it finishes."""
import json
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from decimate_reference import cluster_reference          # noqa: E402
from pegasus_amd import decimate as D                     # noqa: E402
from pegasus_amd import mesh as M                         # noqa: E402
from pegasus_amd.mesh_render import MeshSet               # noqa: E402
from pegasus_amd.pose_error import PoseErrorModels, pose_errors        # noqa: E402

DEV = torch.device("cuda")
REPS = 5
RATIO = 0.025
PAIRS = 64
ADI_PAIRS_FULL = {128: 64, 256: 4}


def stage(msg):
    print(msg, flush=True)


def events(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return dict(min_ms=out[0], median_ms=out[len(out) // 2], max_ms=out[-1], reps=REPS)


def box_model():
    from pegasus_amd import scenes
    from pegasus_amd.gaussian_model import GaussianModel
    cloud = scenes.box_object(np.random.default_rng(11), 40_000, (0.06, 0.16, 0.21), math.log(0.002), 0.4, 0.15, object_id=1)
    return GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling,
                                     cloud.rotation)


def random_poses(rng, n, diameter):
    """Ground-truth poses half a metre out and estimates a few degrees and a few percent of the diameter off."""
    def rot(axis_angle):
        a = np.linalg.norm(axis_angle)
        k = axis_angle / a
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * Kx @ Kx
    R_gt = np.stack([rot(rng.normal(size=3)) for _ in range(n)])
    t_gt = rng.normal(size=(n, 3)) * 0.05 + [0.0, 0.0, 0.5]
    R_est = np.stack([rot(rng.normal(size=3) * math.radians(4.0)) @ R for R in R_gt])
    t_est = t_gt + rng.normal(size=(n, 3)) * 0.03 * diameter
    return R_est, t_est, R_gt, t_gt


def timed_errors(models, poses, errors, n):
    ids = np.ones(n, np.int64)
    args = [a[:n] for a in poses]
    pose_errors(models, ids[:1], *[a[:1] for a in poses], errors=errors)          # warm
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = pose_errors(models, ids, *args, errors=errors)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def measure(model, resolution):
    stage(f"grid {resolution}: extracting")
    mesh = M.extract_mesh(model, resolution=resolution)
    nv, nf = len(mesh.vertices), len(mesh.faces)
    rec = dict(grid=resolution, vertices=nv, faces=nf, ratio=RATIO, target_faces=int(RATIO * nf))
    t = time.perf_counter()
    small, voxel = D.simplify_to(mesh, rec["target_faces"])
    rec["simplify_to_wall_s"] = time.perf_counter() - t
    rec.update(voxel=voxel, out_vertices=len(small.vertices), out_faces=len(small.faces))
    stage(f"grid {resolution}: {nf} -> {len(small.faces)} faces at voxel {voxel:.6g} in {rec['simplify_to_wall_s']:.3f} s")
    c = D._clustering_of(mesh, DEV)
    rec["workspace_bytes"] = c.ws.numel()
    lo = c.lo_pt - voxel / 2.0
    grid = (voxel, float(lo[0]), float(lo[1]), float(lo[2]))
    L = D._lib
    rec["count"] = events(lambda: L.call("pgr_mesh_cluster_count", DEV, nv, L.ptr(c.vertices), nf, L.ptr(c.faces), *grid,
                                         L.ptr(c.ws), c.ws.numel(), L.ptr(c.counts)))
    k, f = c.count(voxel)
    out = [torch.empty((k, 3), dtype=torch.float64, device=DEV), torch.empty((f, 3), dtype=torch.int32, device=DEV),
           torch.empty(nv, dtype=torch.int32, device=DEV), torch.empty(k, dtype=torch.uint8, device=DEV)]
    for name, code in D.CONTRACTIONS.items():
        rec[f"emit_{name}"] = events(lambda: L.call("pgr_mesh_cluster_emit", DEV, nv, L.ptr(c.vertices), nf, L.ptr(c.faces),
                                                    *grid, code, L.ptr(c.ws), c.ws.numel(), k, f, *[L.ptr(o) for o in out]))
    stage(f"grid {resolution}: count {rec['count']} emit {rec['emit_quadric']}")
    t = time.perf_counter()
    ref = cluster_reference(mesh.vertices, mesh.faces, voxel)
    rec["numpy_reference_s"] = time.perf_counter() - t
    rec["equals_reference"] = bool(np.array_equal(out[1].cpu().numpy(), ref.faces) and
                                   np.array_equal(out[0].cpu().numpy(), ref.vertices) and
                                   np.array_equal(out[3].cpu().numpy(), ref.used_quadric))
    rec["used_quadric_fraction"] = float(ref.used_quadric.mean())
    stage(f"grid {resolution}: numpy {rec['numpy_reference_s']:.3f} s, equal {rec['equals_reference']}")
    # the pose errors on the full model against the decimated one
    full = PoseErrorModels(MeshSet({1: mesh}, device=DEV))
    coarse = PoseErrorModels(MeshSet({1: small}, device=DEV))
    diameter = M.models_info(small)["diameter"]
    rec["diameter_eval"] = diameter
    poses = random_poses(np.random.default_rng(4), PAIRS, diameter)
    for errors, n in ((("mssd", "add"), PAIRS), (("adi",), ADI_PAIRS_FULL[resolution])):
        a, ta = timed_errors(full, poses, errors, n)
        b, tb = timed_errors(coarse, poses, errors, n)
        for name in errors:
            d = np.abs(a[name] - b[name]) / diameter
            rec[name] = dict(pairs=n, mean_abs_diff_over_diameter=float(d.mean()), max_abs_diff_over_diameter=float(d.max()),
                             mean_error_over_diameter=float(a[name].mean() / diameter))
        rec["_".join(errors) + "_seconds"] = dict(pairs=n, models=ta, models_eval=tb)
        stage(f"grid {resolution}: {errors} full {ta:.4f} s, eval {tb:.4f} s")
    stage(json.dumps(rec))
    return rec


if __name__ == "__main__":
    model = box_model()
    records = [measure(model, r) for r in (128, 256)]
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "decimate_bench.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(records, indent=1) + "\n")
