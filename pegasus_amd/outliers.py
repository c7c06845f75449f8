"""Radius outlier removal (open3d's ``remove_radius_outlier``: the reference's ``load_ply(clean_pcd=True)`` and
``denoise_point_cloud``, /root/reference/src/gs/gaussian_model.py:238-247,633-651) on the HIP library's sparse grid
(``pgr_radius_count``).

The rule: point i is kept iff count_i > nb_points, where count_i is the number of points j, i itself
included, with ((dx*dx) + dy*dy) + dz*dz < radius*radius in float64, compared strictly.

    python -m pegasus_amd.outliers --in model.ply --out cleaned.ply [--nb_points 16] [--radius 0.03]
"""
from __future__ import annotations

import argparse
import math
from typing import Optional, Sequence

import torch

from . import _lib

CELL_LIMIT = float(1 << 30)          # include/pegasus_raster.h: |x| / radius stays below it


def radius_neighbor_count(points: torch.Tensor, radius: float, cap: Optional[int] = None) -> torch.Tensor:
    """points [N,3] float32 on a HIP device -> int32 [N]: min(count, cap), count = the points within ``radius`` (the point
    itself included).  ``cap=None``: exact counts.  There is no CPU path."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be [N,3]")
    if points.dtype != torch.float32:
        raise ValueError("points must be float32")
    radius = float(radius)
    if not (math.isfinite(radius) and radius > 0.0):
        raise ValueError("radius must be finite and positive")
    if cap is not None and int(cap) < 1:
        raise ValueError("cap must be at least 1")
    if points.device.type != "cuda":
        raise RuntimeError("radius_neighbor_count needs a tensor on a HIP device (torch device 'cuda'); there is no CPU path")
    pts = points.detach().contiguous()
    n = int(pts.shape[0])
    counts = torch.empty((n,), dtype=torch.int32, device=pts.device)
    if n == 0:
        return counts
    # the library's contract, which it cannot check itself: one reduction (NaN and inf fail the comparison)
    if not float(pts.abs().max()) / radius < CELL_LIMIT:
        raise ValueError("points must be finite with |x| / radius < 2^30")
    ws = _lib.workspace("pgr_radius_count", pts.device, n)
    _lib.call("pgr_radius_count", pts.device, n, _lib.ptr(pts), radius, n if cap is None else min(int(cap), n),
              _lib.ptr(counts), _lib.ptr(ws), ws.numel())
    return counts


def radius_outlier_mask(points: torch.Tensor, nb_points: int, radius: float) -> torch.Tensor:
    """bool [N]: True where a point has MORE than ``nb_points`` points within ``radius``, itself included."""
    if int(nb_points) < 1:
        raise ValueError("nb_points must be at least 1")
    return radius_neighbor_count(points, radius, cap=int(nb_points) + 1) > int(nb_points)


def remove_radius_outlier(points: torch.Tensor, nb_points: int, radius: float):
    """(kept points [M,3], ind int64 [M] ascending): open3d's ``PointCloud.remove_radius_outlier``."""
    ind = torch.nonzero(radius_outlier_mask(points, nb_points, radius)).squeeze(1)
    return points[ind], ind


def clean_ply(src, dst, nb_points: int = 16, radius: float = 0.03, device="cuda"):
    """Copies the vertex rows of ``src`` that pass the filter to ``dst`` (every property kept, as float32); returns
    (rows kept, rows read)."""
    import numpy as np

    from .ply_io import read_ply_vertices, write_ply_vertices
    v = read_ply_vertices(src)
    xyz = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float32)
    mask = radius_outlier_mask(torch.from_numpy(xyz).to(device), nb_points, radius).cpu().numpy()
    write_ply_vertices(dst, {k: v[k][mask] for k in v.dtype.names})
    return int(mask.sum()), len(v)


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.outliers", description=__doc__.split("\n\n")[0])
    p.add_argument("--in", dest="src", required=True, help="a Gaussian PLY (any vertex PLY with x, y, z)")
    p.add_argument("--out", required=True)
    p.add_argument("--nb_points", type=int, default=16)
    p.add_argument("--radius", type=float, default=0.03)
    a = p.parse_args(argv)
    kept, n = clean_ply(a.src, a.out, a.nb_points, a.radius)
    print(f"kept {kept} of {n} rows, written to {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
