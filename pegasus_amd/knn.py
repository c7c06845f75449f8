"""Mean squared distance to the 3 nearest neighbours (the reference's `simple_knn._C.distCUDA2`,
/root/reference/src/gs/gaussian_model.py:25,147) on the HIP library's grid search (`pgr_knn_mean_dist2`)."""
from __future__ import annotations

import torch

from . import _lib


def dist2(points: torch.Tensor) -> torch.Tensor:
    """points [N,3] float32 on a HIP device -> [N] float32: mean of the squared distances to the 3 nearest other
    points.  There is no CPU path."""
    if points.device.type != "cuda":
        raise RuntimeError("distCUDA2 needs a tensor on a HIP device (torch device 'cuda'); there is no CPU path")
    pts = points.detach().to(torch.float32).contiguous()
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("points must be [N,3]")
    n = int(pts.shape[0])
    out = torch.empty((n,), dtype=torch.float32, device=pts.device)
    if n == 0:
        return out
    ws = _lib.workspace("pgr_knn", pts.device, n)
    _lib.call("pgr_knn_mean_dist2", pts.device, n, _lib.ptr(pts), _lib.ptr(out), _lib.ptr(ws), ws.numel())
    return out


distCUDA2 = dist2
