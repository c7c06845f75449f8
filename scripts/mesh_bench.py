#!/usr/bin/env python3
"""Per-stage GPU times of mesh extraction (pegasus_amd.mesh.extract_mesh) for the 150 k-Gaussian object of
scenes.scene_c2: render (96 views, depth + alpha), integrate (TSDF fusion), count (count + scan) and emit, at 256^3
and 512^3 grids.  One JSON line per resolution; the first, untimed pass warms the allocator and the kernels.
    python scripts/mesh_bench.py [--resolutions 256 512] [--n_views 96] [--image_size 512] [--repeats 3]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--n_views", type=int, default=96)
    ap.add_argument("--image_size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pegasus_amd import scenes
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.mesh import extract_mesh
    cloud, _views = scenes.scene_c2()
    model = GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling,
                                      cloud.rotation)
    extract_mesh(model, resolution=min(a.resolutions), n_views=a.n_views, image_size=a.image_size)     # warm-up
    for res in a.resolutions:
        runs = []
        for _ in range(a.repeats):
            ms = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh = extract_mesh(model, resolution=res, n_views=a.n_views, image_size=a.image_size, stage_ms=ms)
            ms["wall"] = 1e3 * (time.perf_counter() - t0)
            runs.append(ms)
        med = {k: float(np.median([r[k] for r in runs])) for k in ("render", "integrate", "count", "emit", "wall")}
        print(json.dumps(dict(object="scene_c2", gaussians=cloud.n, resolution=res, n_views=a.n_views,
                              image_size=a.image_size, vertices=len(mesh.vertices), faces=len(mesh.faces),
                              volume=mesh.volume(), stage_ms={k: round(v, 3) for k, v in med.items()})), flush=True)


if __name__ == "__main__":
    main()
