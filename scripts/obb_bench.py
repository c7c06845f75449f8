"""Times the minimal-oriented-box and diameter kernels (pegasus_amd.obb) beside the host hull and NumPy.

    python scripts/obb_bench.py [out.json]

Two inputs: 100 000 points on a turned 6 x 16 x 20 cm ellipsoid (every point is a hull vertex) and the vertices of
mesh.extract_mesh at its defaults on the 40 000-Gaussian box object.  Per input: scipy's hull on the host (host clock);
pgr_obb_candidates and pgr_point_diameter on the hull, on data already on the device, warm, REPS repeats between device events
(min, median, max); the wall time of obb.minimal_oriented_box and obb.diameter, hull and transfers included; the NumPy
reference of tests/obb_reference.py on 64 of the candidates and mesh._diameter's rule on 512 rows, scaled up to all of them.
Prints every stage as it finishes and one JSON record per input."""
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

import obb_cases as OC                    # noqa: E402
import obb_reference as OR                # noqa: E402
from pegasus_amd import _lib, obb          # noqa: E402

DEV = torch.device("cuda")
REPS = 7


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


def stage(msg):
    print(msg, flush=True)


def measure(name, cloud):
    stage(f"{name}: start, {len(cloud)} points")
    rec = dict(name=name, n_points=len(cloud))
    t = time.perf_counter()
    hv, ht = obb.convex_hull(cloud, robust=False)
    rec["hull_s"] = time.perf_counter() - t
    rec["hull_vertices"], rec["hull_triangles"] = len(hv), len(ht)
    jobs = (_lib.PgrObbJob * 1)(_lib.PgrObbJob(0, len(hv), 0, len(ht)))
    d_p, d_t = torch.from_numpy(hv).to(DEV), torch.from_numpy(ht).to(DEV)
    vol = torch.empty(len(ht), dtype=torch.float64, device=DEV)
    best = torch.empty(1, dtype=torch.int32, device=DEV)
    lohi = torch.empty(6, dtype=torch.float64, device=DEV)
    ws = _lib.workspace("pgr_obb_candidates", DEV, 1, jobs)
    rec["obb_workspace_bytes"] = ws.numel()
    rec["obb"] = events(lambda: _lib.call("pgr_obb_candidates", DEV, _lib.ptr(d_p), len(hv), _lib.ptr(d_t), len(ht), None, 1, jobs,
                                          _lib.ptr(vol), _lib.ptr(best), _lib.ptr(lohi), _lib.ptr(ws), ws.numel()))
    rec["projections"] = len(hv) * len(ht)
    stage(f"{name}: obb {rec['obb']}")
    pair = torch.empty(2, dtype=torch.int32, device=DEV)
    d2 = torch.empty(1, dtype=torch.float64, device=DEV)
    ws2 = _lib.workspace("pgr_point_diameter", DEV, 1, jobs)
    rec["diameter"] = events(lambda: _lib.call("pgr_point_diameter", DEV, _lib.ptr(d_p), len(hv), 1, jobs, _lib.ptr(pair),
                                               _lib.ptr(d2), _lib.ptr(ws2), ws2.numel()))
    stage(f"{name}: diameter {rec['diameter']}")
    t = time.perf_counter()
    box = obb.minimal_oriented_box(cloud, device=DEV)
    rec["minimal_oriented_box_wall_s"] = time.perf_counter() - t
    t = time.perf_counter()
    rec["diameter_value"] = obb.diameter(cloud, device=DEV)
    rec["diameter_wall_s"] = time.perf_counter() - t
    rec["volume"], rec["extent"] = box.volume, box.extent.tolist()
    p64 = cloud.astype(np.float64)
    rec["aabb_volume"] = float(np.prod(p64.max(0) - p64.min(0)))
    stage(f"{name}: python layer done")
    # the NumPy reference on a subsample of the candidates, scaled to all of them
    sub = min(64, len(ht))
    pick = np.random.default_rng(0).choice(len(ht), sub, replace=False)
    t = time.perf_counter()
    ref_lohi, ref_vol, q_bound = OR.candidates(hv, ht[pick], block=8)
    dt = time.perf_counter() - t
    rec["numpy_candidates_s_scaled"], rec["numpy_candidates_subsample"] = dt * len(ht) / sub, sub
    v = vol.cpu().numpy()[pick]
    rec["subsample_volume_error_over_bound_max"] = float(np.max(np.abs(v - ref_vol) / OR.volume_bound(ref_lohi, q_bound)))
    rows = min(512, len(hv))
    t = time.perf_counter()
    h64 = hv.astype(np.float64)
    for i0 in range(0, rows, 256):                      # mesh._diameter's rule in chunks of 256 x V
        d = h64[i0:i0 + 256, None, :] - h64[None, :, :]
        float((d * d).sum(-1).max())
    rec["numpy_diameter_s_scaled"], rec["numpy_diameter_rows"] = (time.perf_counter() - t) * len(hv) / rows, rows
    stage(json.dumps(rec))
    return rec


def ellipsoid(n=100_000):
    d = np.random.default_rng(1).normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return ((d * [0.03, 0.08, 0.10]) @ OC.rotation(5).T).astype(np.float32)


def extracted_box():
    from pegasus_amd import scenes
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.mesh import extract_mesh
    cloud = scenes.box_object(np.random.default_rng(11), 40_000, (0.06, 0.16, 0.21), math.log(0.002), 0.4, 0.15, object_id=1)
    model = GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling,
                                      cloud.rotation)
    return extract_mesh(model).vertices


if __name__ == "__main__":
    out = [measure("ellipsoid_100k", ellipsoid()),
           measure("extract_mesh_box", np.ascontiguousarray(extracted_box(), np.float32))]
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(json.dumps(out, indent=1))
