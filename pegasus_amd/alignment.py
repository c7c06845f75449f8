"""Aligning a reconstruction to its ground plane: the dominant plane of a point cloud by RANSAC on the HIP library
(``pgr_plane_hypotheses``, ``pgr_plane_score``, ``pgr_plane_inliers``), a least-squares refit, and the similarity
x' = s R x + t that puts the plane on z = 0 with the scene centred over it -- applied to a COLMAP model on disk
(``ReconstructionAlignment``, the reference's surface: /root/reference/src/reconstruction/environment_reconstruction.py:53-66)
or to a trained Gaussian model (``transform_model``).  ``segment_plane`` has open3d's call shape; open3d itself is not needed.
DESIGN.md section 18 holds the rules.  Device tensors in; there is no CPU path.

    python -m pegasus_amd.alignment --project <colmap dir> [--scale s] [--plane_normal x y z] [--threshold t]
        [--iterations H] [--seed k]
    python -m pegasus_amd.alignment --model in.ply --out out.ply [--scale s] [--plane_normal x y z] [--threshold t]
        [--iterations H] [--seed k] [--min_opacity 0.5] [--crop 2.0]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import shutil
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

SUMS = _lib.PGR_PLANE_SUMS           # include/pegasus_raster.h PGR_PLANE_SUMS, and where each sum lies in it
COUNT, SUM_Q, SUM_QQ, SUM_D2 = 0, 1, 4, 10
EIGEN_GAP_MIN = 1e-12                # a refit whose (l1 - l0) / l2 is not above it keeps the hypothesis plane
SIMILARITY_TOL = 1e-6                # how far the 3x3 block of a similarity may lie from s times a rotation


@dataclass
class PlaneFit:
    """What ``fit_ground_plane`` found."""
    plane: np.ndarray                # float64 [4]: (nx, ny, nz, d) refitted and oriented
    hypothesis_plane: np.ndarray     # float64 [4]: the best triple's plane, as the kernel wrote it
    best_index: int                  # the best hypothesis
    count: int                       # inliers of ``plane``
    fitness: float                   # count / points
    inlier_rmse: float               # sqrt(sum dist^2 / count) under ``plane``
    centroid: np.ndarray             # float64 [3]: the mean of the inliers of ``plane``
    inliers: Optional[torch.Tensor] = None       # int64 [count], device: their rows, ascending
    hypothesis_count: int = 0        # inliers of the best hypothesis


# ---- argument checks
def _points(fn, points):
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be a tensor [N,3]")
    if points.dtype != torch.float32:
        raise ValueError("points must be float32")
    if points.device.type != "cuda":
        raise RuntimeError(f"{fn} needs tensors on a HIP device (torch device 'cuda'); there is no CPU path")
    return points.detach().contiguous()


def _threshold(value):
    value = float(value)
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError("distance_threshold must be finite and positive")
    return value


def _vector(v, what, size=3):
    v = np.array(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1)
    if v.shape != (size,) or not np.isfinite(v).all():
        raise ValueError(f"{what} must be {size} finite numbers")
    return v


def _check_finite(pts):
    """The library's contract, which it cannot check itself: one reduction (NaN and inf fail the comparison)."""
    if pts.shape[0] and not float(pts.abs().max()) < math.inf:
        raise ValueError("points must be finite")


# ---- the three entries
def draw_triples(n: int, num_iterations: int, seed: int) -> np.ndarray:
    """int32 [H,3]: the rows of every hypothesis, from numpy's default generator on the host.  A triple with a repeated row is
    an invalid hypothesis, not a redraw."""
    if n < 1:
        return np.zeros((int(num_iterations), 3), dtype=np.int32)
    return np.random.default_rng(seed).integers(0, n, size=(int(num_iterations), 3)).astype(np.int32)


def plane_hypotheses(points: torch.Tensor, triples):
    """(planes float64 [H,4], valid uint8 [H]) on the device: the plane through rows (i0, i1, i2) of every triple (int32 [H,3];
    a host array or a device tensor).  Rows outside [0, N), repeated rows and collinear points give four zeros and valid 0."""
    pts = _points("plane_hypotheses", points)
    if not torch.is_tensor(triples):
        triples = torch.from_numpy(np.array(triples, dtype=np.int32))           # (a copy: the array may be read-only)
    tri = triples.to(device=pts.device, dtype=torch.int32).contiguous()
    if tri.dim() != 2 or tri.shape[1] != 3:
        raise ValueError("triples must be [H,3]")
    h = int(tri.shape[0])
    planes = torch.empty((h, 4), dtype=torch.float64, device=pts.device)
    valid = torch.empty((h,), dtype=torch.uint8, device=pts.device)
    _lib.call("pgr_plane_hypotheses", pts.device, int(pts.shape[0]), _lib.ptr(pts), h, _lib.ptr(tri), _lib.ptr(planes),
              _lib.ptr(valid))
    return planes, valid


def plane_scores(points: torch.Tensor, planes: torch.Tensor, distance_threshold: float):
    """(counts int32 [H], sumsq float64 [H]) on the device: every plane (float64 [H,4]) against every point; a point is an
    inlier iff |n . p + d| < distance_threshold, strictly."""
    pts = _points("plane_scores", points)
    thr = _threshold(distance_threshold)
    if (not torch.is_tensor(planes) or planes.dim() != 2 or planes.shape[1] != 4 or planes.dtype != torch.float64 or
            planes.device != pts.device):
        raise ValueError("planes must be float64 [H,4] on the points' device")
    planes = planes.detach().contiguous()
    n, h = int(pts.shape[0]), int(planes.shape[0])
    counts = torch.empty((h,), dtype=torch.int32, device=pts.device)
    sumsq = torch.empty((h,), dtype=torch.float64, device=pts.device)
    ws = _lib.workspace("pgr_plane_score", pts.device, n, h)
    _lib.call("pgr_plane_score", pts.device, n, _lib.ptr(pts), h, _lib.ptr(planes), thr, _lib.ptr(counts), _lib.ptr(sumsq),
              _lib.ptr(ws), ws.numel())
    return counts, sumsq


def plane_inliers(points: torch.Tensor, plane, pivot, distance_threshold: float, return_mask: bool = True):
    """(mask uint8 [N] or None, sums float64 [12]) on the device: the inliers of one plane (4 host numbers) and, with
    q = p - pivot (3 host numbers): the count, sum q, the upper triangle of sum q q^T, sum dist^2, 0."""
    pts = _points("plane_inliers", points)
    thr = _threshold(distance_threshold)
    plane, pivot = _vector(plane, "plane", 4), _vector(pivot, "pivot")
    n = int(pts.shape[0])
    mask = torch.empty((n,), dtype=torch.uint8, device=pts.device) if return_mask else None
    sums = torch.empty((SUMS,), dtype=torch.float64, device=pts.device)
    ws = _lib.workspace("pgr_plane_inliers", pts.device, n)
    _lib.call("pgr_plane_inliers", pts.device, n, _lib.ptr(pts), (C.c_double * 4)(*plane), (C.c_double * 3)(*pivot), thr,
              _lib.ptr(mask), _lib.ptr(sums), _lib.ptr(ws), ws.numel())
    return mask, sums


# ---- the host side of the rule (float64)
def choose_best(counts, sumsq, valid) -> int:
    """The valid hypothesis of largest count, among equal counts of smallest sumsq, then of lowest index; -1 without one."""
    counts, sumsq, valid = np.asarray(counts), np.asarray(sumsq), np.asarray(valid).astype(bool)
    if not valid.any():
        return -1
    rows = np.nonzero(valid)[0]
    order = np.lexsort((rows, sumsq[rows], -counts[rows].astype(np.int64)))
    return int(rows[order[0]])


def refit_plane(sums, pivot, hypothesis_plane) -> np.ndarray:
    """The least-squares plane of the inliers from their sums about ``pivot``; the hypothesis plane with fewer than 3 inliers
    or a covariance whose two smallest eigenvalues do not differ by more than 1e-12 of the largest."""
    sums, pivot = np.asarray(sums, dtype=np.float64), np.asarray(pivot, dtype=np.float64)
    count = sums[COUNT]
    if count < 3:
        return np.array(hypothesis_plane, dtype=np.float64)
    m = sums[SUM_Q:SUM_Q + 3] / count
    S = np.zeros((3, 3))
    S[np.triu_indices(3)] = sums[SUM_QQ:SUM_QQ + 6]
    S = S + np.triu(S, 1).T
    cov = S / count - np.outer(m, m)
    if not np.isfinite(cov).all():
        return np.array(hypothesis_plane, dtype=np.float64)
    w, v = np.linalg.eigh(cov)
    if not (w[2] > 0.0 and (w[1] - w[0]) / w[2] > EIGEN_GAP_MIN):
        return np.array(hypothesis_plane, dtype=np.float64)
    normal = v[:, 0] / np.linalg.norm(v[:, 0])
    return np.array([normal[0], normal[1], normal[2], -float(normal @ (pivot + m))])


def orient_plane(plane, plane_normal=None, camera_centers=None) -> np.ndarray:
    """The plane or its negative: with ``plane_normal``, n . plane_normal >= 0; else with camera centres, at least half of
    them at a positive signed distance; else the normal's component of largest magnitude (the first among equal ones)
    positive."""
    plane = np.array(plane, dtype=np.float64)
    n = plane[:3]
    if plane_normal is not None:
        flip = float(n @ _vector(plane_normal, "plane_normal")) < 0.0
    elif camera_centers is not None and len(camera_centers):
        centres = np.asarray(camera_centers, dtype=np.float64).reshape(-1, 3)
        flip = 2 * int((centres @ n + plane[3] > 0.0).sum()) < len(centres)
    else:
        flip = n[int(np.argmax(np.abs(n)))] < 0.0
    return -plane if flip else plane


def rotation_to_z(normal) -> np.ndarray:
    """The smallest rotation that takes the unit vector ``normal`` to +z: Rodrigues about normal x z; the identity for +z and
    a half turn about x for -z."""
    n = np.asarray(normal, dtype=np.float64)
    v = np.array([n[1], -n[0], 0.0])                             # n x z
    if v[0] == 0.0 and v[1] == 0.0:
        return np.eye(3) if n[2] > 0.0 else np.diag([1.0, -1.0, -1.0])
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return np.eye(3) + K + K @ K / (1.0 + n[2])


def plane_transformation(fit: PlaneFit, scale: float = 1.0) -> np.ndarray:
    """Row-major float64 4x4 of x' = s R x + t: R takes the plane's normal to +z, the inlier centroid projected onto the plane
    lands on the origin, ``scale`` is the caller's metric scale (applied first: the fit's threshold is in the input's units)."""
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError("scale must be finite and positive")
    plane, c = np.asarray(fit.plane, dtype=np.float64), np.asarray(fit.centroid, dtype=np.float64)
    n = plane[:3]
    origin = c - (float(n @ c) + plane[3]) * n
    R = rotation_to_z(n)
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = -scale * (R @ origin)
    return T


def _similarity(T, what="transformation"):
    """(s, R, t) of a 4x4 whose 3x3 block is s > 0 times a rotation, or ValueError."""
    if torch.is_tensor(T):
        T = T.detach().cpu().numpy()
    T = np.array(T, dtype=np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError(f"{what} must be a finite 4x4")
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"the last row of {what} must be 0 0 0 1")
    A = T[:3, :3]
    det = float(np.linalg.det(A))
    if not det > 0.0:
        raise ValueError(f"the 3x3 block of {what} is not a positive scale times a rotation")
    s = float(np.cbrt(det))
    R = A / s
    if np.abs(R.T @ R - np.eye(3)).max() > SIMILARITY_TOL:
        raise ValueError(f"the 3x3 block of {what} is not a scale times a rotation")
    return s, R, T[:3, 3].copy()


# ---- the fit
def fit_ground_plane(points: torch.Tensor, distance_threshold: float = 0.01, num_iterations: int = 1000, seed: int = 0,
                     plane_normal=None, camera_centers=None) -> PlaneFit:
    """The dominant plane of ``points`` (float32 [N,3] on a HIP device), DESIGN.md section 18: ``num_iterations`` triples drawn
    on the host, every one scored on every point, the best (most inliers, then the smallest sum of squares, then the lowest
    index) refitted by least squares over its inliers, oriented, and its inliers counted again.  ValueError without a valid
    hypothesis."""
    pts = _points("fit_ground_plane", points)
    thr = _threshold(distance_threshold)
    n, h = int(pts.shape[0]), int(num_iterations)
    if h < 1:
        raise ValueError("num_iterations must be positive")
    if n < 3:
        raise ValueError("a plane needs at least 3 points")
    _check_finite(pts)
    triples = draw_triples(n, h, seed)
    planes, valid = plane_hypotheses(pts, triples)
    counts, sumsq = plane_scores(pts, planes, thr)
    best = choose_best(counts.cpu().numpy(), sumsq.cpu().numpy(), valid.cpu().numpy())
    if best < 0:
        raise ValueError(f"none of the {h} hypotheses is a plane (repeated rows or collinear points)")
    hypothesis = planes[best].cpu().numpy()
    pivot = pts[int(triples[best, 0])].cpu().numpy().astype(np.float64)
    _, sums = plane_inliers(pts, hypothesis, pivot, thr, return_mask=False)
    sums = sums.cpu().numpy()
    plane = refit_plane(sums, pivot, hypothesis)
    mask, after = plane_inliers(pts, plane, pivot, thr)
    after = after.cpu().numpy()
    count = int(after[COUNT])
    centroid = pivot + after[SUM_Q:SUM_Q + 3] / count if count else pivot.copy()
    return PlaneFit(plane=orient_plane(plane, plane_normal, camera_centers), hypothesis_plane=hypothesis, best_index=best,
                    count=count, fitness=count / n, inlier_rmse=math.sqrt(after[SUM_D2] / count) if count else 0.0,
                    centroid=centroid, inliers=torch.nonzero(mask).squeeze(1), hypothesis_count=int(sums[COUNT]))


def segment_plane(points: torch.Tensor, distance_threshold: float = 0.01, ransac_n: int = 3, num_iterations: int = 1000,
                  seed: int = 0):
    """open3d's ``segment_plane``: (plane_model float64 [4], inliers int64 tensor).  Only ``ransac_n = 3``."""
    if int(ransac_n) != 3:
        raise ValueError("ransac_n must be 3")
    fit = fit_ground_plane(points, distance_threshold, num_iterations, seed)
    return fit.plane, fit.inliers


# ---- applying the transformation
def transform_points(xyz, T) -> np.ndarray:
    """x' = s R x + t of host points [N,3], float64."""
    T = np.asarray(T, dtype=np.float64)
    return np.asarray(xyz, dtype=np.float64).reshape(-1, 3) @ T[:3, :3].T + T[:3, 3]


def transform_colmap(cameras, images, xyz, T):
    """(images', xyz') of a COLMAP model under x' = s R x + t: every image gets R_img' = R_img R^T and
    t_img' = s t_img - R_img' t, which scales camera space by s, so that no pixel projection changes; the points get x'.
    ``cameras`` (the intrinsics) stay as they are."""
    from .colmap_io import ColmapImage, qvec2rotmat, rotmat2qvec
    s, R, t = _similarity(T)
    moved = {}
    for key, im in images.items():
        R_new = qvec2rotmat(im.qvec) @ R.T
        moved[key] = ColmapImage(im.id, rotmat2qvec(R_new), s * np.asarray(im.tvec, dtype=np.float64) - R_new @ t,
                                 im.camera_id, im.name)
    return moved, transform_points(xyz, T)


_ROWS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def transform_model(model, T):
    """A new Gaussian model under the similarity x' = s R x + t (s > 0): centres x', log-scales plus ln s, splat orientations
    and SH bands 1-3 rotated by R (one device pass, about the origin); opacities and DC colour untouched.  A matrix whose 3x3
    block is not s times a rotation within 1e-6 is refused."""
    from . import compose
    from .gaussian_model import GaussianModel
    s, R, t = _similarity(T)
    rigid = np.eye(4)
    rigid[:3, :3], rigid[:3, 3] = R, t
    with torch.no_grad():
        src = {k: getattr(model, k).detach().contiguous() for k in _ROWS}
        if src["_xyz"].device.type != "cuda":
            raise RuntimeError("transform_model needs a model on a HIP device (torch device 'cuda'); there is no CPU path")
        out = dict(src)
        out["_xyz"], out["_rotation"] = torch.empty_like(src["_xyz"]), torch.empty_like(src["_rotation"])
        out["_features_rest"] = torch.empty_like(src["_features_rest"])
        out["_scaling"] = src["_scaling"] + math.log(s)
        out["_features_dc"], out["_opacity"] = src["_features_dc"].clone(), src["_opacity"].clone()
        if src["_xyz"].shape[0]:
            compose.compose_object((src["_xyz"] * s).contiguous(), src["_rotation"], src["_features_rest"],
                                   compose.make_pose(rigid, np.zeros(3)), out["_xyz"], out["_rotation"], out["_features_rest"])
        moved = GaussianModel(model.max_sh_degree, model.device)
        moved.active_sh_degree = model.active_sh_degree
        for k, v in out.items():
            setattr(moved, k, v)
    return moved


# ---- the reference's surface
class ReconstructionAlignment:
    """The COLMAP model of a project (``<project>/sparse/0``): ``scale_scene_by_const`` and ``align2plane`` build the
    transformation, ``save`` rewrites the model.  The plane is fitted on the model's points as they are on disk, so the
    threshold is in their units; the scale is part of the transformation that ``save`` applies."""

    def __init__(self, project_path, device="cuda"):
        from . import colmap_io
        self.project_path = Path(project_path)
        self.sparse_dir = colmap_io._sparse_dir(self.project_path)
        self.cameras, self.images = colmap_io.read_model(self.project_path)
        self.binary = (self.sparse_dir / "points3D.bin").exists()
        if self.binary:
            self.xyz, self.rgb = colmap_io.read_points3D_binary(self.sparse_dir / "points3D.bin")
        elif (self.sparse_dir / "points3D.txt").exists():
            self.xyz, self.rgb = colmap_io.read_points3D_text(self.sparse_dir / "points3D.txt")
        else:
            raise FileNotFoundError(f"no points3D.bin / .txt under {self.sparse_dir}")
        self.device = torch.device(device)
        self.scale = 1.0
        self.fit: Optional[PlaneFit] = None
        self.plane_size = None
        self._transformation, self._pending = np.eye(4), False

    @property
    def transformation(self) -> np.ndarray:
        """The 4x4 that ``save`` applies; setting one (a similarity from elsewhere) makes it pending."""
        return self._transformation

    @transformation.setter
    def transformation(self, T):
        self._transformation, self._pending = np.array(T, dtype=np.float64), True

    def camera_centers(self) -> np.ndarray:
        from .colmap_io import qvec2rotmat
        return np.array([-qvec2rotmat(im.qvec).T @ np.asarray(im.tvec, dtype=np.float64) for im in self.images.values()]
                        ).reshape(-1, 3)

    def scale_scene_by_const(self, scale: float):
        scale = float(scale)
        if not (math.isfinite(scale) and scale > 0.0):
            raise ValueError("scale must be finite and positive")
        self.scale *= scale
        self.transformation = plane_transformation(self.fit, self.scale) if self.fit else np.diag([self.scale] * 3 + [1.0])

    def align2plane(self, plane_size=2., plane_normal=None, debug=False, distance_threshold=0.01, num_iterations=1000, seed=0):
        """Fits the ground plane on the model's points and sets the transformation that puts it on z = 0.  Without
        ``plane_normal`` the cameras decide which side is up.  ``plane_size`` is recorded and crops nothing; ``debug`` opened a
        viewer in the reference and is ignored."""
        points = torch.as_tensor(np.asarray(self.xyz, dtype=np.float32), device=self.device)
        self.fit = fit_ground_plane(points, distance_threshold, num_iterations, seed, plane_normal=plane_normal,
                                    camera_centers=None if plane_normal is not None else self.camera_centers())
        self.plane_size = float(plane_size)
        self.transformation = plane_transformation(self.fit, self.scale)
        return self.transformation

    def save(self):
        """Rewrites the sparse model under the transformation, keeps the original beside it with ``_unaligned`` appended to the
        directory's name (``sparse/0_unaligned``; ``sparse_unaligned`` for a project whose model lies in ``sparse`` itself; an
        earlier original is not overwritten), removes the cached ``points3D.ply`` and writes ``<project>/alignment.json``.
        ``colmap_io.write_colmap_model`` writes 2D points and tracks EMPTY: the observations of a real COLMAP model survive
        only in the kept original.  Afterwards nothing is pending: the object holds the moved model with scale 1, and another
        ``save()`` without a new ``scale_scene_by_const`` or ``align2plane`` is a RuntimeError, so that ``alignment.json`` is
        not overwritten by an identity record."""
        if not self._pending:
            raise RuntimeError("nothing to save: call scale_scene_by_const or align2plane first")
        from . import colmap_io
        images, xyz = transform_colmap(self.cameras, self.images, self.xyz, self.transformation)
        backup = self.sparse_dir.with_name(self.sparse_dir.name + "_unaligned")
        if not backup.exists():
            shutil.copytree(self.sparse_dir, backup)
        colmap_io.write_colmap_model(self.sparse_dir, self.cameras, images, xyz, self.rgb, binary=self.binary)
        (self.sparse_dir / "points3D.ply").unlink(missing_ok=True)
        record = {"transformation": self.transformation.tolist(), "scale": self.scale, "plane_size": self.plane_size,
                  "plane": None, "fitness": None, "inlier_rmse": None}
        if self.fit is not None:
            record.update(plane=[float(v) for v in self.fit.plane], fitness=self.fit.fitness, inlier_rmse=self.fit.inlier_rmse,
                          inliers=self.fit.count, best_index=self.fit.best_index)
        (self.project_path / "alignment.json").write_text(json.dumps(record, indent=2) + "\n")
        self.images, self.xyz = images, xyz
        self.scale, self.fit, self._transformation, self._pending = 1.0, None, np.eye(4), False


# ---- command line
def _parser():
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.alignment", description=__doc__.split("\n\n")[0])
    p.add_argument("--project", help="a COLMAP project (with sparse/0), rewritten in place")
    p.add_argument("--model", help="a Gaussian PLY, with --out")
    p.add_argument("--out", help="where the aligned Gaussian PLY goes")
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--plane_normal", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    p.add_argument("--threshold", type=float, default=0.01)
    p.add_argument("--iterations", type=int, default=1000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--min_opacity", type=float, default=0.5)
    p.add_argument("--crop", type=float, default=None, help="keep the Gaussians with |x'|, |y'| <= crop / 2")
    return p


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = _parser()
    a = p.parse_args(argv)
    if (a.project is None) == (a.model is None):
        p.error("give either --project or --model with --out")
    if a.model is not None and a.out is None:
        p.error("--model needs --out")
    if a.project is not None and (a.out is not None or a.crop is not None):
        p.error("--out and --crop go with --model")
    if not (math.isfinite(a.scale) and a.scale > 0.0):
        p.error("--scale must be finite and positive")
    if not (math.isfinite(a.threshold) and a.threshold > 0.0):
        p.error("--threshold must be finite and positive")
    if a.iterations < 1:
        p.error("--iterations must be positive")
    if a.crop is not None and not (math.isfinite(a.crop) and a.crop > 0.0):
        p.error("--crop must be finite and positive")
    if a.project is not None:
        reco = ReconstructionAlignment(a.project)
        reco.scale_scene_by_const(a.scale)
        reco.align2plane(plane_normal=a.plane_normal, distance_threshold=a.threshold, num_iterations=a.iterations, seed=a.seed)
        fit = reco.fit
        reco.save()
        print(f"plane {fit.plane.tolist()}: fitness {fit.fitness:.6f}, inlier RMSE {fit.inlier_rmse:.6g}; "
              f"{reco.sparse_dir} rewritten, alignment.json written")
        return 0
    from .gaussian_model import GaussianModel
    model = GaussianModel(3)
    model.load_ply(a.model)
    xyz = model.get_xyz.detach()
    if a.min_opacity > 0.0:
        xyz = xyz[model.get_opacity.detach()[:, 0] >= a.min_opacity]
    fit = fit_ground_plane(xyz.contiguous(), a.threshold, a.iterations, a.seed, plane_normal=a.plane_normal)
    T = plane_transformation(fit, a.scale)
    moved = transform_model(model, T)
    if a.crop is not None:
        moved.mask_points((moved.get_xyz[:, :2].abs() <= a.crop / 2).all(dim=1))
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    moved.save_ply(out)
    np.savetxt(out.with_suffix(".transformation.txt"), T)
    print(f"plane {fit.plane.tolist()}: fitness {fit.fitness:.6f}, inlier RMSE {fit.inlier_rmse:.6g}; "
          f"{moved.get_xyz.shape[0]} Gaussians written to {out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
