"""Times of the collision kernels on one GPU ("Measured"): pgr_mesh_sdf at 96^3 for collision meshes of
5 k and 25 k faces, one pgr_sdf_sweep call, and a six-object drop.  Medians after a warm-up: device events around the library
call for the kernels, a host clock around synchronised work for what includes a read-back.  The float64 host reference
(tests/collision_reference.py) is timed at 24^3 x 320 faces, where it finishes, and scaled by points x faces.

    python scripts/collision_bench.py [--out profiles/collision_bench.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np


def event_ms(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), reps=reps)


def wall_ms(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), reps=reps)


def nested_spheres(outer, inner):
    """Two icospheres, one inside the other: 20 (4^outer + 4^inner) faces in one bounding box."""
    import collision_cases as CC
    v0, f0 = CC.icosphere(outer)
    v1, f1 = CC.icosphere(inner, 0.3)
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)]).astype(np.int32)


def main(argv=None):
    import torch
    import collision_cases as CC
    import collision_reference as CR
    from pegasus_amd import collision as COL
    from pegasus_amd.mesh import Mesh
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--out", default=str(ROOT / "profiles" / "collision_bench.json"))
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("collision_bench needs a HIP device; a CPU run says nothing about the kernels")
    dev, out = torch.device("cuda"), {}
    for label, (v, f) in (("5k", CC.icosphere(4)), ("25k", nested_spheres(5, 4))):
        grid = COL.MeshSDF.from_mesh(Mesh(v, f), resolution=96).grid
        dv, df = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        r = event_ms(lambda: COL.mesh_sdf(dv, df, grid), 2, 10)
        r.update(faces=len(f), points=grid.nx * grid.ny * grid.nz, grid=[grid.nx, grid.ny, grid.nz])
        r["pairs_per_s"] = r["faces"] * r["points"] / (1e-3 * r["median_ms"])
        out[f"mesh_sdf_96_{label}"] = r
    # six bodies of 5120 faces (2562 shell points), fields of 96^3: the sweep of the sixth against five placed ones and the
    # plane (11 jobs), and the whole placement with given orientations (the loop, not the host's hull code)
    bodies = [COL.CollisionBody.from_mesh(Mesh(*CC.icosphere(4)), resolution=96) for _ in range(6)]
    eye = [np.eye(3)] * 6
    poses, reports = COL.drop(bodies, orientations=eye, seed=0, radius=0.6)
    jobs = COL._sweep_jobs(5, range(5), (0.0, 0.0, -1.0), True)
    lifted = poses.copy()
    lifted[5, 2, 3] += 1.0
    plane = COL.unit_plane((0, 0, 1, 0))
    out["sweep_11_jobs_device"] = event_ms(lambda: COL.sweep_words(bodies, lifted, jobs, plane, 1e-4, 5.0, 128), 3, 50)
    out["sweep_11_jobs_with_16_byte_readback"] = wall_ms(
        lambda: COL._unsigned_min(COL.sweep_words(bodies, lifted, jobs, plane, 1e-4, 5.0, 128)).cpu(), 3, 50)
    out["drop_six_objects"] = dict(wall_ms(lambda: COL.drop(bodies, orientations=eye, seed=0, radius=0.6), 1, 7),
                                   rounds=[r["rounds"] for r in reports], settled=[bool(r["settled"]) for r in reports])
    v, f = CC.icosphere()
    pts = CR.grid_points(CR.body_grid(v, 24)).reshape(-1, 3)
    t = time.perf_counter()
    CR.mesh_distance(pts, v, f)
    host = time.perf_counter() - t
    pairs = len(pts) * len(f)
    big = out["mesh_sdf_96_25k"]
    out["host_reference"] = dict(seconds=host, points=len(pts), faces=len(f), pairs_per_s=pairs / host,
                                 scaled_to_96_25k_seconds=host * big["points"] * big["faces"] / pairs)
    out["device"] = torch.cuda.get_device_name(0)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
