"""Registering and merging two scans of one object: normals by radius, nearest-neighbour correspondences and ICP on the HIP
library's sparse grid (``pgr_nn_grid_build``, ``pgr_nn_correspond``, ``pgr_icp_sums``, ``pgr_radius_normals``), and the model
layer on top: ``register_models`` and ``merge_models`` for an object that was scanned from the top and, turned over, from the
bottom (/root/reference/README.md:114-118).  The functions follow open3d's ``estimate_normals``, ``evaluate_registration`` and
``registration_icp``, which the reference's marker alignment uses
(/root/reference/submodules/aruco-estimator/aruco_estimator/utils.py:82-98); open3d itself is not needed.  DESIGN.md
section 17 holds the rules.  Device tensors in; there is no CPU path.

    python -m pegasus_amd.registration --target up.ply --source down.ply
        (--init T.txt | --points_target a.txt --points_source b.txt)
        [--max_distance 0.02] [--normals_radius R] [--estimation point_to_plane|point_to_point]
        [--max_iteration 30] [--min_opacity 0.5] [--drop_within D] --out fused.ply
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

CELL_LIMIT = float(1 << 30)          # include/pegasus_raster.h: |x| / max_distance stays below it
SUMS = 48                            # include/pegasus_raster.h PGR_ICP_SUMS, and where each sum lies in it
JTJ, JTR, COUNT, D2, SUM_S, SUM_Q, SUM_SQ, SUM_SS = 0, 21, 27, 28, 29, 32, 35, 44
PLANE_SLICE, POINT_SLICE = slice(0, 32), slice(16, 48)          # the 32 numbers each estimator fetches per iteration
ESTIMATIONS = ("point_to_plane", "point_to_point")
SINGULAR = 1e-12                     # a system whose smallest eigen- or singular value is below this share of the largest
ROTATION_TOL = 1e-6                  # how far R^T R may lie from the identity, and det R from 1


@dataclass
class RegistrationResult:
    """open3d's ``RegistrationResult``, and how many updates ICP made."""
    transformation: np.ndarray                   # float64 [4,4]
    fitness: float                               # correspondences / source points
    inlier_rmse: float                           # sqrt(sum d2 / correspondences), 0 without any
    correspondence_set: torch.Tensor             # int64 [M,2] (source row, target row), in source order
    iterations: int = 0


# ---- argument checks
def _clouds(fn, **clouds):
    """The named clouds, detached and contiguous: shapes and types first, then where they live."""
    for what, points in clouds.items():
        if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"{what} must be a tensor [N,3]")
        if points.dtype != torch.float32:
            raise ValueError(f"{what} must be float32")
    for points in clouds.values():
        if points.device.type != "cuda":
            raise RuntimeError(f"{fn} needs tensors on a HIP device (torch device 'cuda'); there is no CPU path")
    return [points.detach().contiguous() for points in clouds.values()]


def _distance(value, what):
    value = float(value)
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"{what} must be finite and positive")
    return value


def _matrix(T, what="transformation"):
    if T is None:
        return np.eye(4)
    if torch.is_tensor(T):
        T = T.detach().cpu().numpy()
    T = np.array(T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError(f"{what} must be 4x4")
    if not np.isfinite(T).all():
        raise ValueError(f"{what} must be finite")
    return T


def _rigid(T, what="transformation"):
    """A 4x4 whose 3x3 block is a rotation, or ValueError (a similarity with a scale other than 1 among them)."""
    T = _matrix(T, what)
    R = T[:3, :3]
    if np.abs(R.T @ R - np.eye(3)).max() > ROTATION_TOL or abs(np.linalg.det(R) - 1.0) > ROTATION_TOL:
        scale = float(np.cbrt(abs(np.linalg.det(R))))
        raise ValueError(f"the 3x3 block of {what} is not a rotation (scale {scale:.6g}); scaling a model is not supported here "
                         "(pegasus_amd.alignment.transform_model applies a similarity)")
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"the last row of {what} must be 0 0 0 1")
    return T


def _abs_max(points) -> float:
    """The library's contract, which it cannot check itself: one reduction (NaN and inf fail the comparisons made with it)."""
    return float(points.abs().max()) if points.shape[0] else 0.0


def _c_matrix(T):
    return (C.c_double * 16)(*np.ascontiguousarray(T, dtype=np.float64).reshape(-1))


# ---- normals
def estimate_normals(points: torch.Tensor, radius: float, return_counts: bool = False):
    """points [N,3] float32 on a HIP device -> float64 [N,3]: open3d's ``estimate_normals(KDTreeSearchParamRadius(radius))``.
    The unit eigenvector of the smallest eigenvalue of the covariance of the points strictly within ``radius`` (the point
    itself included), its component of largest magnitude positive; (0,0,1) with fewer than 3 neighbours.
    ``return_counts``: also int32 [N], the neighbours.  There is no CPU path."""
    radius = _distance(radius, "radius")
    pts, = _clouds("estimate_normals", points=points)
    n = int(pts.shape[0])
    normals = torch.empty((n, 3), dtype=torch.float64, device=pts.device)
    counts = torch.empty((n,), dtype=torch.int32, device=pts.device)
    if n:
        if not _abs_max(pts) / radius < CELL_LIMIT:
            raise ValueError("points must be finite with |x| / radius < 2^30")
        ws = _lib.workspace("pgr_radius_normals", pts.device, n)
        _lib.call("pgr_radius_normals", pts.device, n, _lib.ptr(pts), radius, _lib.ptr(normals), _lib.ptr(counts), _lib.ptr(ws),
                  ws.numel())
    return (normals, counts) if return_counts else normals


# ---- correspondences and sums
class _Pair:
    """A source and a target cloud at one distance: the target's grid (built once: the target does not move), the lane order
    and the buffers every evaluation reuses."""

    def __init__(self, source, target, max_distance, fn, init=None, target_normals=None, cell_order=True):
        self.source, self.target = _clouds(fn, source=source, target=target)
        if self.source.device != self.target.device:
            raise ValueError("source and target must be on the same device")
        self.max_distance = _distance(max_distance, "max_correspondence_distance")
        self.device = dev = self.source.device
        self.ns, self.nt = int(self.source.shape[0]), int(self.target.shape[0])
        self.normals = None
        if target_normals is not None:
            if (not torch.is_tensor(target_normals) or tuple(target_normals.shape) != (self.nt, 3) or
                    target_normals.dtype != torch.float64 or target_normals.device != dev):
                raise ValueError("target_normals must be float64 [Nt,3] on the target's device")
            self.normals = target_normals.detach().contiguous()
        self.source_max = _abs_max(self.source)
        if not _abs_max(self.target) / self.max_distance < CELL_LIMIT:
            raise ValueError("target must be finite with |x| / max_distance < 2^30")
        self.index = torch.empty((self.ns,), dtype=torch.int32, device=dev)
        self.d2 = torch.empty((self.ns,), dtype=torch.float64, device=dev)
        self.sums = torch.zeros((SUMS,), dtype=torch.float64, device=dev)
        self.grid = self.order = self.sums_ws = None
        if self.nt:
            self.grid = _lib.workspace("pgr_nn_grid_build", dev, self.nt)
            _lib.call("pgr_nn_grid_build", dev, self.nt, _lib.ptr(self.target), self.max_distance, _lib.ptr(self.grid),
                      self.grid.numel())
        if self.ns:
            self.sums_ws = _lib.workspace("pgr_icp_sums", dev, self.ns)
        if cell_order and self.ns and self.nt:
            T = _matrix(init)
            self._check_posed(T)
            self.order = torch.empty((self.ns,), dtype=torch.int32, device=dev)
            ws = _lib.workspace("pgr_nn_source_order", dev, self.ns)
            _lib.call("pgr_nn_source_order", dev, self.ns, _lib.ptr(self.source), _c_matrix(T), self.max_distance,
                      _lib.ptr(self.order), _lib.ptr(ws), ws.numel())

    def _check_posed(self, T):
        # |s'_k| <= sum_j |R_kj| max|s| + |t_k|: a host bound from the one reduction made at the start
        bound = (np.abs(T[:3, :3]).sum(axis=1) * self.source_max + np.abs(T[:3, 3])).max()
        if not bound / self.max_distance < CELL_LIMIT:
            raise ValueError("source must be finite with |R s + t| / max_distance < 2^30")

    def correspond(self, T):
        """Fills ``index`` and ``d2`` for the pose ``T``; no synchronisation."""
        if not self.ns:
            return
        self._check_posed(T)
        _lib.call("pgr_nn_correspond", self.device, self.ns, _lib.ptr(self.source), _lib.ptr(self.order), _c_matrix(T), self.nt,
                  self.max_distance, _lib.ptr(self.grid), self.grid.numel() if self.grid is not None else 0,
                  _lib.ptr(self.index), _lib.ptr(self.d2))

    def reduce(self, T):
        """The sums of the current correspondences under ``T`` into ``sums`` (device); no synchronisation."""
        _lib.call("pgr_icp_sums", self.device, self.ns, _lib.ptr(self.source), _c_matrix(T), _lib.ptr(self.index),
                  _lib.ptr(self.d2), self.nt, _lib.ptr(self.target), _lib.ptr(self.normals), _lib.ptr(self.sums),
                  _lib.ptr(self.sums_ws), self.sums_ws.numel() if self.sums_ws is not None else 0)

    def evaluate(self, T, fetch=slice(0, SUMS)):
        """(fitness, rmse, sums as a host float64 [48] of which ``fetch`` is filled): the one device-to-host copy."""
        self.correspond(T)
        self.reduce(T)
        host = np.zeros(SUMS)
        host[fetch] = self.sums[fetch].cpu().numpy()
        count = host[COUNT]
        fitness = count / self.ns if self.ns else 0.0
        rmse = math.sqrt(host[D2] / count) if count > 0 else 0.0
        return fitness, rmse, host

    def correspondence_set(self):
        rows = torch.nonzero(self.index >= 0).squeeze(1)
        return torch.stack([rows, self.index[rows].to(torch.int64)], dim=1)


def nearest_neighbors(source: torch.Tensor, target: torch.Tensor, max_distance: float, transformation=None):
    """(index int32 [Ns], d2 float64 [Ns]): for every source point posed by ``transformation`` (4x4, default the identity) the
    nearest target point strictly within ``max_distance`` (the lowest row among equally near ones) and the squared distance;
    -1 and 0 where there is none."""
    T = _matrix(transformation)
    pair = _Pair(source, target, max_distance, "nearest_neighbors", init=T)
    pair.correspond(T)
    return pair.index, pair.d2


def evaluate_registration(source, target, max_correspondence_distance, transformation=None) -> RegistrationResult:
    """open3d's ``evaluate_registration``: fitness, inlier RMSE and the correspondences at ``transformation``."""
    T = _matrix(transformation)
    pair = _Pair(source, target, max_correspondence_distance, "evaluate_registration", init=T)
    fitness, rmse, _ = pair.evaluate(T)
    return RegistrationResult(T, fitness, rmse, pair.correspondence_set())


# ---- the updates (host, float64)
def vec6_to_matrix(x) -> np.ndarray:
    """(alpha, beta, gamma, tx, ty, tz) -> Rz(gamma) Ry(beta) Rx(alpha) with the translation (tx, ty, tz), 4x4 float64."""
    a, b, g = (float(v) for v in x[:3])
    ca, sa, cb, sb, cg, sg = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(g), math.sin(g)
    T = np.eye(4)
    T[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                 [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                 [-sb, cb * sa, cb * ca]]
    T[:3, 3] = [float(v) for v in x[3:6]]
    return T


def point_to_plane_update(sums) -> np.ndarray:
    """Solves J^T J x = -J^T r from the sums; the identity with fewer than 6 correspondences or a singular system."""
    if sums[COUNT] < 6:
        return np.eye(4)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[JTJ:JTJ + 21]
    A = A + np.triu(A, 1).T
    b = -np.asarray(sums[JTR:JTR + 6])
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return np.eye(4)
    w = np.linalg.eigvalsh(A)
    if not (w[-1] > 0.0 and w[0] > SINGULAR * w[-1]):
        return np.eye(4)
    return vec6_to_matrix(np.linalg.solve(A, b))


def point_to_point_update(sums) -> np.ndarray:
    """Kabsch without scale from the sums; the identity with fewer than 3 correspondences or a cross-covariance of rank < 2."""
    n = sums[COUNT]
    if n < 3:
        return np.eye(4)
    mu_s, mu_q = np.asarray(sums[SUM_S:SUM_S + 3]) / n, np.asarray(sums[SUM_Q:SUM_Q + 3]) / n
    H = np.asarray(sums[SUM_SQ:SUM_SQ + 9]).reshape(3, 3) / n - np.outer(mu_s, mu_q)        # sum (s' - mu_s)(q - mu_q)^T / n
    if not np.isfinite(H).all():
        return np.eye(4)
    U, S, Vt = np.linalg.svd(H)
    if not (S[0] > 0.0 and S[1] > SINGULAR * S[0]):
        return np.eye(4)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) > 0 else -1.0])
    T = np.eye(4)
    T[:3, :3] = Vt.T @ D @ U.T
    T[:3, 3] = mu_q - T[:3, :3] @ mu_s
    return T


def registration_icp(source, target, max_correspondence_distance, init=None, estimation="point_to_plane", target_normals=None,
                     max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, normals_radius=None) -> RegistrationResult:
    """open3d's ``registration_icp``: evaluate at ``init``; up to ``max_iteration`` times compute the
    update from the current correspondences, set T <- update @ T and evaluate again; stop when the fitness and the RMSE both
    changed by less than ``relative_fitness`` / ``relative_rmse`` (absolute differences, as open3d compares them).  Point to
    plane needs ``target_normals`` (float64 [Nt,3]) or ``normals_radius`` to estimate them with.  Every iteration poses the
    stored float32 source by the cumulative float64 T and fetches 32 numbers from the device."""
    if estimation not in ESTIMATIONS:
        raise ValueError(f"estimation must be one of {ESTIMATIONS}")
    if int(max_iteration) < 0:
        raise ValueError("max_iteration must not be negative")
    T = _matrix(init, "init")
    plane = estimation == "point_to_plane"
    if plane and target_normals is None:
        if normals_radius is None:
            raise ValueError("point_to_plane needs target_normals or normals_radius")
        target_normals = estimate_normals(target, normals_radius)
    pair = _Pair(source, target, max_correspondence_distance, "registration_icp", init=T,
                 target_normals=target_normals if plane else None)
    fetch, update = (PLANE_SLICE, point_to_plane_update) if plane else (POINT_SLICE, point_to_point_update)
    fitness, rmse, sums = pair.evaluate(T, fetch)
    iterations = 0
    for _ in range(int(max_iteration)):
        T = update(sums) @ T
        before = (fitness, rmse)
        fitness, rmse, sums = pair.evaluate(T, fetch)
        iterations += 1
        if abs(before[0] - fitness) < relative_fitness and abs(before[1] - rmse) < relative_rmse:
            break
    return RegistrationResult(T, fitness, rmse, pair.correspondence_set(), iterations)


# ---- picked or marker points (host, float64)
def kabsch_umeyama(pointset_A, pointset_B):
    """(R, c, t) with A ~ t + c R B in the least-squares sense (Umeyama 1991): R a proper rotation (never a reflection), c the
    scale, t the translation; [N,d] arrays of corresponding rows."""
    A, B = np.asarray(pointset_A, dtype=np.float64), np.asarray(pointset_B, dtype=np.float64)
    if A.ndim != 2 or A.shape != B.shape:
        raise ValueError("the point sets must be [N,d] arrays of one shape")
    n, m = A.shape
    mean_a, mean_b = A.mean(axis=0), B.mean(axis=0)
    a, b = A - mean_a, B - mean_b
    var_b = (b * b).sum() / n
    U, D, Vt = np.linalg.svd(a.T @ b / n)
    S = np.ones(m)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[-1] = -1.0
    R = U @ np.diag(S) @ Vt
    c = float((D * S).sum() / var_b)
    t = mean_a - c * R @ mean_b
    return R, c, t


def align_point_set(point_set_A, point_set_B):
    """(A, B moved onto A, [R, c, t])."""
    R, c, t = kabsch_umeyama(np.asarray(point_set_A), np.asarray(point_set_B))
    moved = t + c * np.asarray(point_set_B, dtype=np.float64) @ R.T
    return point_set_A, moved, [R, c, t]


# ---- Gaussian models
def _centres(model, min_opacity):
    xyz = model.get_xyz.detach()
    if min_opacity > 0.0:
        xyz = xyz[model.get_opacity.detach()[:, 0] >= min_opacity]
    return xyz.contiguous()


def register_models(target_model, source_model, init, max_correspondence_distance=0.02, normals_radius=None, min_opacity=0.0,
                    **icp) -> RegistrationResult:
    """ICP of the source model's Gaussian centres onto the target model's, over those whose activated opacity is at least
    ``min_opacity``.  ``init`` must be rigid; ``normals_radius`` defaults to the correspondence distance; ``icp``: the other
    arguments of ``registration_icp``."""
    T = _rigid(init, "init")
    if normals_radius is None:
        normals_radius = max_correspondence_distance
    return registration_icp(_centres(source_model, float(min_opacity)), _centres(target_model, float(min_opacity)),
                            max_correspondence_distance, init=T, normals_radius=normals_radius, **icp)


_ROWS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def merge_models(target_model, source_model, transformation, drop_within=None):
    """A new model: the target's Gaussians followed by the source's, posed by x' = R x + t (about the ORIGIN, splat
    orientations and SH rotated with them, one device pass).  ``drop_within=d``: posed source Gaussians with a target Gaussian
    strictly within ``d`` are left out, so that where both scans saw the surface only the target's remain."""
    from . import compose
    from .gaussian_model import GaussianModel
    T = _rigid(transformation)
    if drop_within is not None:
        drop_within = _distance(drop_within, "drop_within")
    with torch.no_grad():
        src = {k: getattr(source_model, k).detach().contiguous() for k in _ROWS}
        if src["_xyz"].device.type != "cuda":
            raise RuntimeError("merge_models needs models on a HIP device (torch device 'cuda'); there is no CPU path")
        posed = dict(src)
        posed["_xyz"], posed["_rotation"] = torch.empty_like(src["_xyz"]), torch.empty_like(src["_rotation"])
        posed["_features_rest"] = torch.empty_like(src["_features_rest"])
        if src["_xyz"].shape[0]:
            compose.compose_object(src["_xyz"], src["_rotation"], src["_features_rest"], compose.make_pose(T, np.zeros(3)),
                                   posed["_xyz"], posed["_rotation"], posed["_features_rest"])
        if drop_within is not None:
            index, _ = nearest_neighbors(posed["_xyz"], target_model.get_xyz.detach(), drop_within)
            keep = index < 0
            posed = {k: v[keep] for k, v in posed.items()}
        merged = GaussianModel(target_model.max_sh_degree, target_model.device)
        merged.active_sh_degree = target_model.active_sh_degree
        for rows in ({k: getattr(target_model, k).detach() for k in _ROWS}, posed):
            part = GaussianModel(target_model.max_sh_degree, target_model.device)
            for k, v in rows.items():
                setattr(part, k, v)
            merged.merge_gaussians(part)
    return merged


# ---- command line
def _parser():
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.registration", description=__doc__.split("\n\n")[0])
    p.add_argument("--target", required=True, help="the Gaussian PLY that stays where it is (the top scan)")
    p.add_argument("--source", required=True, help="the Gaussian PLY that is moved onto it (the bottom scan)")
    p.add_argument("--init", help="a text file with the initial 4x4 source-to-target transformation")
    p.add_argument("--points_target", help="N x 3 text file of picked or marker points in the target")
    p.add_argument("--points_source", help="the same points in the source, row for row")
    p.add_argument("--max_distance", type=float, default=0.02)
    p.add_argument("--normals_radius", type=float, default=None)
    p.add_argument("--estimation", choices=ESTIMATIONS, default="point_to_plane")
    p.add_argument("--max_iteration", type=int, default=30)
    p.add_argument("--min_opacity", type=float, default=0.5)
    p.add_argument("--drop_within", type=float, default=None)
    p.add_argument("--out", required=True)
    return p


def main(argv: Optional[Sequence[str]] = None) -> int:
    from .gaussian_model import GaussianModel
    p = _parser()
    a = p.parse_args(argv)
    if (a.init is None) == (a.points_target is None and a.points_source is None):
        p.error("give either --init or --points_target with --points_source")
    if a.init is None and (a.points_target is None or a.points_source is None):
        p.error("--points_target and --points_source go together")
    if a.init is not None:
        init = np.loadtxt(a.init, dtype=np.float64).reshape(4, 4)
    else:
        R, c, t = kabsch_umeyama(np.loadtxt(a.points_target, ndmin=2), np.loadtxt(a.points_source, ndmin=2))
        if abs(c - 1.0) > 0.01:
            raise SystemExit(f"the picked points give a scale of {c:.6g} between the two scans: more than 1 % from 1, and "
                             "scaling a model is not supported here (pegasus_amd.alignment.transform_model applies a "
                             "similarity)")
        init = np.eye(4)
        init[:3, :3], init[:3, 3] = R, t
    target, source = GaussianModel(3), GaussianModel(3)
    target.load_ply(a.target)
    source.load_ply(a.source)
    tgt, src = _centres(target, a.min_opacity), _centres(source, a.min_opacity)
    before = evaluate_registration(src, tgt, a.max_distance, init)
    print(f"before: fitness {before.fitness:.6f}, inlier RMSE {before.inlier_rmse:.6g}")
    result = register_models(target, source, init, a.max_distance, a.normals_radius, a.min_opacity, estimation=a.estimation,
                             max_iteration=a.max_iteration)
    print(f"after {result.iterations} iterations: fitness {result.fitness:.6f}, inlier RMSE {result.inlier_rmse:.6g}")
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    merged = merge_models(target, source, result.transformation, a.drop_within)
    merged.save_ply(out)
    np.savetxt(out.parent / "transformation_b2a.txt", result.transformation)
    print(f"{merged.get_xyz.shape[0]} Gaussians written to {out}, the transformation to {out.parent / 'transformation_b2a.txt'}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
