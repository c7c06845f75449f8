"""Minimal oriented bounding boxes and model diameters on the HIP library (``pgr_obb_candidates``, ``pgr_point_diameter``).

The reference's scene_gt writer takes ``mesh.get_minimal_oriented_bounding_box(robust=True)`` from open3d and stores its
corners in NDDS order (src/tools/pegasus_working.py:469-495, 546-576).  open3d's rule, which DESIGN.md section 16 writes
out: one candidate box per triangle of the convex hull, the extents of all hull vertices in the triangle's frame, the smallest
volume wins (the lowest triangle index among equal ones).  The hull is taken on the host (scipy, as ``mesh._diameter`` does);
the F x V projections run on the GPU in float64.  A candidate whose volume is not finite is never chosen, which open3d does
not promise.  The diameter is the toolkit's ``misc.calc_pts_diameter``: the largest distance between two points, brute force.

    python -m pegasus_amd.obb --models <dir> [--robust]                 writes <dir>/models_boxes.json
    python -m pegasus_amd.obb --dataset <dir> --models <dir> [...]      also rewrites the box fields of every scene_gt.json
"""
from __future__ import annotations

import argparse
import json
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib, bop_dataset as BD

NDDS_ORDER = (0, 2, 5, 3, 1, 7, 4, 6)           # pegasus_working.py:488-495, rows of open3d's GetBoxPoints


@dataclass
class OrientedBox:
    """``center`` [3], ``R`` [3,3] (columns: the box axes, right-handed), ``extent`` [3]: float64."""
    center: np.ndarray
    R: np.ndarray
    extent: np.ndarray

    @property
    def volume(self) -> float:
        return float(self.extent[0] * self.extent[1] * self.extent[2])

    def box_points(self) -> np.ndarray:
        """[8,3] in the order of open3d's ``OrientedBoundingBox::GetBoxPoints``."""
        x, y, z = (self.R * (self.extent * 0.5)).T
        c = self.center
        return np.stack([c - x - y - z, c + x - y - z, c - x + y - z, c - x - y + z,
                         c + x + y + z, c - x + y + z, c + x - y + z, c + x + y - z])

    def ndds_corners(self) -> np.ndarray:
        """[8,3] in the NDDS order the reference writes."""
        return self.box_points()[list(NDDS_ORDER)]

    def contains(self, points, tol: float = 0.0) -> np.ndarray:
        """bool [N]: the point lies in the box grown by ``tol`` on every side."""
        q = (np.asarray(points, np.float64).reshape(-1, 3) - self.center) @ self.R
        return (np.abs(q) <= self.extent * 0.5 + tol).all(axis=1)


def _f32_points(points) -> np.ndarray:
    p = np.ascontiguousarray(points, np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be [N,3]")
    return p


def _jobs(point_counts, tri_counts):
    jobs = (_lib.PgrObbJob * max(1, len(point_counts)))()
    p0 = t0 = 0
    for k, (n_p, n_t) in enumerate(zip(point_counts, tri_counts)):
        jobs[k] = _lib.PgrObbJob(p0, n_p, t0, n_t)
        p0 += n_p
        t0 += n_t
    return jobs


def candidate_boxes(point_sets: Sequence, triangle_sets: Sequence, device=None):
    """One ``pgr_obb_candidates`` call over all sets.  ``point_sets[k]`` [P_k,3] float32, ``triangle_sets[k]`` [F_k,3] int32
    over them.  Returns (volumes: list of float64 [F_k], best int32 [K], lohi float64 [K,6]) on the host.  Every triangle index
    is checked here and again by the entry (which gets the host copy): the kernels clamp nothing."""
    import torch
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError("candidate_boxes needs a HIP device (torch device 'cuda'); there is no CPU path")
    pts = [_f32_points(p) for p in point_sets]
    tris = [np.ascontiguousarray(t, np.int32).reshape(-1, 3) for t in triangle_sets]
    if len(pts) != len(tris):
        raise ValueError("one triangle list per point set")
    K = len(pts)
    for k, (p, t) in enumerate(zip(pts, tris)):
        if len(t) and (t.min() < 0 or t.max() >= len(p)):
            raise ValueError(f"set {k}: a triangle names a point outside 0..{len(p) - 1}")
    if K == 0:
        return [], np.zeros((0,), np.int32), np.zeros((0, 6), np.float64)
    all_p = np.concatenate(pts) if sum(map(len, pts)) else np.zeros((0, 3), np.float32)
    all_t = np.ascontiguousarray(np.concatenate(tris)) if sum(map(len, tris)) else np.zeros((0, 3), np.int32)
    jobs = _jobs([len(p) for p in pts], [len(t) for t in tris])
    d_p = torch.from_numpy(all_p).to(device)
    d_t = torch.from_numpy(all_t).to(device)
    volumes = torch.empty((len(all_t),), dtype=torch.float64, device=device)
    best = torch.empty((K,), dtype=torch.int32, device=device)
    lohi = torch.empty((K, 6), dtype=torch.float64, device=device)
    ws = _lib.workspace("pgr_obb_candidates", device, K, jobs)
    _lib.call("pgr_obb_candidates", device, _lib.ptr(d_p), len(all_p), _lib.ptr(d_t), len(all_t),
              all_t.ctypes.data if len(all_t) else None, K, jobs, _lib.ptr(volumes), _lib.ptr(best), _lib.ptr(lohi),
              _lib.ptr(ws), ws.numel())
    vol = volumes.cpu().numpy()
    edges = np.cumsum([0] + [len(t) for t in tris])
    return [vol[edges[k]:edges[k + 1]] for k in range(K)], best.cpu().numpy(), lohi.cpu().numpy()


def point_diameters(point_sets: Sequence, device=None):
    """One ``pgr_point_diameter`` call: (pair int32 [K,2], d2 float64 [K]) on the host."""
    import torch
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError("point_diameters needs a HIP device (torch device 'cuda'); there is no CPU path")
    pts = [_f32_points(p) for p in point_sets]
    K = len(pts)
    if K == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0,), np.float64)
    all_p = np.concatenate(pts) if sum(map(len, pts)) else np.zeros((0, 3), np.float32)
    jobs = _jobs([len(p) for p in pts], [0] * K)
    d_p = torch.from_numpy(all_p).to(device)
    pair = torch.empty((K, 2), dtype=torch.int32, device=device)
    d2 = torch.empty((K,), dtype=torch.float64, device=device)
    ws = _lib.workspace("pgr_point_diameter", device, K, jobs)
    _lib.call("pgr_point_diameter", device, _lib.ptr(d_p), len(all_p), K, jobs, _lib.ptr(pair), _lib.ptr(d2), _lib.ptr(ws),
              ws.numel())
    return pair.cpu().numpy(), d2.cpu().numpy()


def frame_of(points, triangle) -> tuple:
    """(a, R): the frame of a triangle by the rule, float64; R's columns are u, v, w."""
    p = np.asarray(points, np.float32).astype(np.float64)
    a = p[triangle[0]]
    u, v = p[triangle[1]] - a, p[triangle[2]] - a
    w = np.cross(u, v)
    v = np.cross(w, u)
    return a, np.stack([u / np.linalg.norm(u), v / np.linalg.norm(v), w / np.linalg.norm(w)], axis=1)


def box_from_candidate(points, triangle, lohi) -> OrientedBox:
    a, R = frame_of(points, triangle)
    lo, hi = np.asarray(lohi[:3], np.float64), np.asarray(lohi[3:], np.float64)
    return OrientedBox(center=a + R @ ((lo + hi) * 0.5), R=R, extent=hi - lo)


def convex_hull(points, robust: bool = False):
    """(hull vertices [V,3] float32, triangles int32 [F,3] over them): scipy's qhull, ``Qt`` (open3d's robust=False) or
    ``QJ`` (robust=True)."""
    from scipy.spatial import ConvexHull, QhullError
    p = _f32_points(points)
    if not np.isfinite(p).all():
        raise ValueError("points must be finite")
    try:
        hull = ConvexHull(p.astype(np.float64), qhull_options="QJ" if robust else None)
    except (QhullError, ValueError) as e:
        raise ValueError(f"no convex hull of these {len(p)} points (fewer than 4, or all in one plane?): {e}") from e
    index = np.full(len(p), -1, np.int64)
    index[hull.vertices] = np.arange(len(hull.vertices))
    return p[hull.vertices], index[hull.simplices].astype(np.int32)


def minimal_oriented_boxes(point_sets: Sequence, robust: bool = False, device=None) -> list:
    """One OrientedBox per point set: one hull per set on the host, one device call for all."""
    hulls = [convex_hull(p, robust) for p in point_sets]
    _, best, lohi = candidate_boxes([h[0] for h in hulls], [h[1] for h in hulls], device)
    out = []
    for k, (v, t) in enumerate(hulls):
        if best[k] < 0:
            raise ValueError(f"set {k}: no hull triangle gives a finite box (every triangle is degenerate)")
        out.append(box_from_candidate(v, t[best[k]], lohi[k]))
    return out


def minimal_oriented_box(points, robust: bool = False, device=None) -> OrientedBox:
    return minimal_oriented_boxes([points], robust, device)[0]


def from_mesh(mesh, robust: bool = True, device=None) -> OrientedBox:
    """The box of a ``mesh.Mesh``'s vertices, as the reference asks open3d for it (robust=True)."""
    return minimal_oriented_box(mesh.vertices, robust, device)


def diameters(point_sets: Sequence, hull: bool = True, device=None) -> list:
    """The largest distance between two points of every set (float64).  ``hull``: search the convex hull's vertices only,
    where the farthest pair lies (sets without a hull are searched whole)."""
    sets = []
    for p in point_sets:
        p = _f32_points(p)
        if hull and len(p) > 4:
            try:
                p = convex_hull(p)[0]
            except ValueError:
                pass
        sets.append(p)
    pair, _ = point_diameters(sets, device)
    return [float(np.linalg.norm(p[j].astype(np.float64) - p[i].astype(np.float64))) if i >= 0 else 0.0
            for p, (i, j) in zip(sets, pair)]


def diameter(points, hull: bool = True, device=None) -> float:
    return diameters([points], hull, device)[0]


def boxes_for(meshes, robust: bool = True) -> dict:
    """{obj_id: (NDDS corners [8,3], vertex mean [3], box centre [3])} of a ``mesh_render.MeshSet`` in its scaled units: the
    third element is what ``bop_pose.scene_gt_entry`` projects as ``projected_center``, the second what it stores as
    ``3d_bounding_center`` (the reference writes mesh.get_center() there)."""
    ids = sorted(meshes.ranges)
    verts = [meshes.mesh(i)[0] for i in ids]
    boxes = minimal_oriented_boxes(verts, robust, meshes.device)
    return {i: (b.ndds_corners(), v.astype(np.float64).mean(0), b.center) for i, v, b in zip(ids, verts, boxes)}


# ---- files ----------------------------------------------------------------------------------------------------------
def models_boxes(models_dir, robust: bool = True, device="cuda") -> dict:
    """{obj_id: {"center", "R", "extent", "ndds_corners", "diameter"}} of every obj_NNNNNN.ply under ``models_dir``, in the
    files' own units."""
    from .ply_io import read_ply_mesh
    files = BD.model_files(models_dir)
    ids = sorted(files)
    verts = [read_ply_mesh(files[i])[0] for i in ids]
    boxes = minimal_oriented_boxes(verts, robust, device)
    diam = diameters(verts, True, device)
    return {str(i): {"center": b.center.tolist(), "R": b.R.tolist(), "extent": b.extent.tolist(),
                     "ndds_corners": b.ndds_corners().tolist(), "diameter": d} for i, b, d in zip(ids, boxes, diam)}


def rewrite_dataset(dataset_dir, models_dir, translation_scale: float = 1.0, robust: bool = True, device="cuda"):
    """Rewrites ``3d_bounding_box_model_coord``, ``3d_bounding_center``, ``projected_points`` and ``projected_center`` of every
    scene_gt.json entry under <dataset>/train from the meshes of ``models_dir`` (millimetres), the entry's ``cam_R_m2c`` /
    ``cam_t_m2c`` and scene_camera.json's ``cam_K``.  ``translation_scale`` is what the translations were written with."""
    from . import bop_pose
    from .mesh_render import MeshSet
    boxes = boxes_for(MeshSet.from_dir(models_dir, device=device, scale=BD.unit_of(translation_scale)), robust)
    scenes = BD.scene_dirs(dataset_dir, "train")
    for scene in map(BD.BopScene, scenes):
        for image, entries in scene.gt.items():
            K = BD.cam_K(scene.camera[image])
            for e in entries:
                if int(e["obj_id"]) not in boxes:
                    raise KeyError(f"{scene.path}: object {e['obj_id']} has no mesh under {models_dir}")
                corners, mean, center = boxes[int(e["obj_id"])]
                T = np.eye(4)
                T[:3, :3], T[:3, 3] = BD.pose_of(e)
                e["3d_bounding_box_model_coord"] = corners.tolist()
                e["3d_bounding_center"] = mean.tolist()
                e["projected_points"] = bop_pose.project_points(K, T, corners).tolist()
                e["projected_center"] = bop_pose.project_points(K, T, center[None]).tolist()
        scene.write_json(BD.SCENE_GT, scene.gt)
    return scenes


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.obb", description=__doc__.split("\n\n")[0])
    p.add_argument("--models", required=True, help="a BOP models directory (obj_NNNNNN.ply)")
    p.add_argument("--dataset", default=None, help="also rewrite the box fields of every scene_gt.json under <dataset>/train")
    p.add_argument("--robust", action="store_true", help="joggled hulls (qhull QJ), open3d's robust=True")
    p.add_argument("--translation_scale", type=float, default=1.0,
                   help="what scene_gt's translations were written with: 1 = metres, 1000 = millimetres")
    a = p.parse_args(argv)
    out = Path(a.models) / "models_boxes.json"
    out.write_text(json.dumps(models_boxes(a.models, a.robust), indent=1))
    print(f"wrote {out}")
    if a.dataset:
        scenes = rewrite_dataset(a.dataset, a.models, a.translation_scale, a.robust)
        print(f"rewrote the box fields of {len(scenes)} scene(s)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
