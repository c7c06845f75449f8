"""Mesh decimation by vertex clustering on the GPU (after open3d's ``TriangleMesh.simplify_vertex_clustering``), and the
``models_eval`` directory of a BOP dataset: the step between "extract a mesh" and "evaluate or simulate with it".

The rule (pegasus_amd/csrc/decimate.hip.h): a grid of cells of edge ``voxel`` whose origin lies half a
cell below the smallest coordinate; every occupied cell becomes one vertex, the mean of the cell's vertices or the minimiser
of its faces' plane quadrics where that is well conditioned and lies in the cell; a face survives if its corners fall into
three different cells, rotated so that its smallest index comes first, duplicates removed, in lexicographic order.  The
result need NOT be closed or manifold: removing duplicates breaks the cycle property, so volumes, centres of mass and inertia
tensors keep coming from the full mesh.  Parity with open3d is not pinned.

    python -m pegasus_amd.decimate --models <dir> [--out <dir>] [--ratio r | --faces n | --voxel v]
                                   [--contraction average|quadric] [--normals]
                                   [--texture -m <model dir> [--obj_id N] [--texel_cell 16] [--scale 1000]]

writes ``<models>/../models_eval`` (the directory the BOP toolkit evaluates on: every ``obj_NNNNNN.ply`` at 2.5 % of its
faces by default, the toolkit's ``TargetPerc``, with a recomputed ``models_info.json`` that keeps the symmetries).  With
``--texture`` the decimated mesh of the object a trained Gaussian model shows gets a texture baked from that model
(``mesh.bake_texture``: a per-face atlas): the PLY carries ``texcoord`` lists and names ``obj_NNNNNN.png``
beside it.
"""
from __future__ import annotations

import argparse
import json
import math
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, bop_dataset as BD
from .mesh import Mesh

CONTRACTIONS = {"average": 0, "quadric": 1}      # include/pegasus_raster.h PGR_CONTRACTION_*
CELL_LIMIT = float(1 << 20)                      # include/pegasus_raster.h: (max - min) / voxel + 1 stays below it per axis
MAX_COUNT_PASSES = 24                            # simplify_to: count passes at the most


class _Clustering:
    """One mesh on the device, checked once; ``count(voxel)`` is one pass of pgr_mesh_cluster_count and one host wait,
    ``emit(contraction)`` the second pass at the voxel last counted."""

    def __init__(self, vertices: torch.Tensor, faces: torch.Tensor):
        if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
            raise ValueError("vertices must be float32 [V,3]")
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
            raise ValueError("faces must be int32 [F,3]")
        if vertices.device.type != "cuda" or faces.device != vertices.device:
            raise RuntimeError("vertex clustering needs both tensors on one HIP device (torch device 'cuda'); there is no CPU path")
        self.vertices, self.faces = vertices.detach().contiguous(), faces.detach().contiguous()
        self.device = vertices.device
        self.nv, self.nf = int(vertices.shape[0]), int(faces.shape[0])
        if self.nv == 0:
            raise ValueError("a mesh without vertices cannot be clustered")
        # the library's contract, which it cannot check itself: one reduction each (NaN and inf fail the comparisons)
        self.lo_pt = self.vertices.min(dim=0).values.double().cpu().numpy()
        self.hi_pt = self.vertices.max(dim=0).values.double().cpu().numpy()
        if not (np.isfinite(self.lo_pt).all() and np.isfinite(self.hi_pt).all()):
            raise ValueError("vertices must be finite")
        if self.nf and not (int(self.faces.min()) >= 0 and int(self.faces.max()) < self.nv):
            raise ValueError("face indices must lie in [0, V)")
        self.ws = _lib.workspace("pgr_mesh_cluster", self.device, self.nv, self.nf)
        self.counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.grid = None

    def count(self, voxel: float):
        """(K, F') at ``voxel``."""
        voxel = float(voxel)
        if not (math.isfinite(voxel) and voxel > 0.0):
            raise ValueError("voxel must be finite and positive")
        if not ((self.hi_pt - self.lo_pt) / voxel + 1.0 < CELL_LIMIT).all():
            raise ValueError("voxel too small for the mesh: (max - min) / voxel + 1 must stay below 2^20 per axis")
        lo = self.lo_pt - voxel / 2.0
        self.grid = (voxel, float(lo[0]), float(lo[1]), float(lo[2]))
        _lib.call("pgr_mesh_cluster_count", self.device, self.nv, _lib.ptr(self.vertices), self.nf, _lib.ptr(self.faces),
                  *self.grid, _lib.ptr(self.ws), self.ws.numel(), _lib.ptr(self.counts))
        k, f = (int(x) for x in self.counts.cpu())
        self.k, self.f = k, f
        return k, f

    def emit(self, contraction: str):
        if contraction not in CONTRACTIONS:
            raise ValueError(f"contraction must be one of {sorted(CONTRACTIONS)}, got {contraction!r}")
        if self.grid is None:
            raise RuntimeError("count() comes first")
        k, f = self.k, self.f
        out_v = torch.empty((k, 3), dtype=torch.float64, device=self.device)
        out_f = torch.empty((f, 3), dtype=torch.int32, device=self.device)
        cov = torch.empty((self.nv,), dtype=torch.int32, device=self.device)
        used = torch.empty((k,), dtype=torch.uint8, device=self.device)
        _lib.call("pgr_mesh_cluster_emit", self.device, self.nv, _lib.ptr(self.vertices), self.nf, _lib.ptr(self.faces),
                  *self.grid, CONTRACTIONS[contraction], _lib.ptr(self.ws), self.ws.numel(), k, f, _lib.ptr(out_v),
                  _lib.ptr(out_f), _lib.ptr(cov), _lib.ptr(used))
        return out_v, out_f, cov, used


def cluster_vertices(vertices: torch.Tensor, faces: torch.Tensor, voxel: float, contraction: str = "quadric"):
    """vertices float32 [V,3] and faces int32 [F,3] on a HIP device -> (vertices float64 [K,3], faces int32 [F',3],
    cluster_of_vertex int32 [V], used_quadric uint8 [K]) on that device.  The result need not be closed or manifold."""
    if contraction not in CONTRACTIONS:
        raise ValueError(f"contraction must be one of {sorted(CONTRACTIONS)}, got {contraction!r}")
    c = _Clustering(vertices, faces)
    c.count(voxel)
    return c.emit(contraction)


def _clustering_of(mesh: Mesh, device) -> _Clustering:
    return _Clustering(torch.from_numpy(np.ascontiguousarray(mesh.vertices, np.float32)).to(device),
                       torch.from_numpy(np.ascontiguousarray(mesh.faces, np.int32)).to(device))


def _mesh_of(emitted) -> Mesh:
    out_v, out_f, _cov, _used = emitted
    return Mesh(out_v.cpu().numpy().astype(np.float32), out_f.cpu().numpy())           # rounded to float32 once


def simplify_vertex_clustering(mesh: Mesh, voxel_size: float, contraction: str = "quadric", device="cuda") -> Mesh:
    """open3d's call shape: ``mesh`` with every occupied cell of edge ``voxel_size`` contracted to one vertex (rounded to
    float32 once).  The result need not be closed or manifold."""
    c = _clustering_of(mesh, device)
    c.count(voxel_size)
    return _mesh_of(c.emit(contraction))


def simplify_to(mesh: Mesh, target_faces: int, contraction: str = "quadric", device="cuda"):
    """(Mesh, voxel): ``mesh`` clustered with the finest voxel found whose face count is at most ``target_faces``.  The voxel is
    bisected over the count pass alone, at most 24 passes in all, starting from the bounding box's extent; the emit pass runs once
    (after one more count pass when the last voxel tried was not the one returned).  The face count is not monotone in the
    voxel, so "finest found" is what the bisection saw, not a minimum."""
    target_faces = int(target_faces)
    if target_faces < 0:
        raise ValueError("target_faces must not be negative")
    if contraction not in CONTRACTIONS:
        raise ValueError(f"contraction must be one of {sorted(CONTRACTIONS)}, got {contraction!r}")
    c = _clustering_of(mesh, device)
    extent = float((c.hi_pt - c.lo_pt).max())
    good = extent if extent > 0.0 else 1.0
    _k, f = c.count(good)
    passes, last = 1, good
    while f > target_faces:                         # at the extent the box spans two cells per axis; at twice that, one
        good *= 2.0
        _k, f = c.count(good)
        passes, last = passes + 1, good
    bad = 0.0                                       # no voxel: every face kept (or the domain's edge)
    floor_voxel = extent / (CELL_LIMIT / 2.0)       # the domain's edge, with a factor 2 to spare
    while passes < MAX_COUNT_PASSES - 1 and good - bad > 1e-3 * good:
        mid = 0.5 * (good + bad)
        if mid <= floor_voxel:
            break
        _k, f = c.count(mid)
        passes, last = passes + 1, mid
        if f <= target_faces:
            good = mid
        else:
            bad = mid
    if last != good:
        c.count(good)                               # emit reads what the last count pass left in the workspace
    return _mesh_of(c.emit(contraction)), good


def write_models_eval(models_dir, out_dir=None, ratio: Optional[float] = 0.025, faces: Optional[int] = None,
                      voxel: Optional[float] = None, contraction: str = "quadric", device="cuda",
                      normals: bool = False, texture_model=None, texture_obj_id: Optional[int] = None, texel_cell: int = 16,
                      model_scale: float = 1000.0, n_views: int = 96, image_size: int = 512) -> dict:
    """For every ``obj_NNNNNN.ply`` under ``models_dir`` a decimated PLY under ``out_dir`` (default
    ``<models_dir>/../models_eval``) and a ``models_info.json`` there: diameter and box recomputed on the decimated mesh, the
    symmetries copied from the source.  The size is set by ``voxel`` (a cell edge), else ``faces`` (a face count), else
    ``ratio`` (of the source's faces; default the toolkit's TargetPerc).  ``normals``: every decimated mesh is written with
    vertex normals recomputed on it (mesh.vertex_normals), as the toolkit's remeshing script does.  ``texture_model``: a
    GaussianModel of object ``texture_obj_id`` (default: the directory's only object) in units ``model_scale`` times smaller
    than the files' (1000: metres against millimetres); that object's decimated mesh is written textured (mesh.bake_texture
    with ``texel_cell``, ``n_views``, ``image_size``).  Returns {obj_id: (faces before, faces after, voxel)}."""
    from .mesh import bake_texture, models_info, vertex_normals, write_ply
    from .ply_io import read_ply_mesh, write_ply_mesh
    models_dir = Path(models_dir)
    out_dir = Path(out_dir) if out_dir is not None else models_dir.parent / "models_eval"
    if voxel is None and faces is None and not (ratio is not None and 0.0 < float(ratio) <= 1.0):
        raise ValueError("ratio must lie in (0, 1]")
    source_info = BD.read_models_info(models_dir)
    info, report = {}, {}
    files = BD.model_files(models_dir)
    if texture_model is not None:
        if texture_obj_id is None and len(files) != 1:
            raise ValueError(f"{models_dir} holds {len(files)} objects: name the one the Gaussian model shows (obj_id)")
        texture_obj_id = int(next(iter(files)) if texture_obj_id is None else texture_obj_id)
        if texture_obj_id not in {int(k) for k in files}:
            raise ValueError(f"object {texture_obj_id} is not in {models_dir}")
    for obj_id, path in files.items():
        v, f = read_ply_mesh(path)
        full = Mesh(v, f)
        if voxel is not None:
            small, used_voxel = simplify_vertex_clustering(full, voxel, contraction, device), float(voxel)
        else:
            target = int(faces) if faces is not None else int(math.floor(float(ratio) * len(f)))
            small, used_voxel = simplify_to(full, target, contraction, device)
        small_normals = vertex_normals(small, device=device) if normals else None
        if texture_model is not None and int(obj_id) == texture_obj_id:
            baked = bake_texture(texture_model, small.scaled(1.0 / model_scale), cell=texel_cell, n_views=n_views, image_size=image_size)
            write_ply(out_dir / f"{BD.model_stem(obj_id)}.ply", Mesh(small.vertices, small.faces, normals=small_normals,
                                                                     corner_uv=baked.corner_uv, texture=baked.texture))
        elif normals:
            write_ply(out_dir / f"{BD.model_stem(obj_id)}.ply", Mesh(small.vertices, small.faces, normals=small_normals))
        else:
            write_ply_mesh(out_dir / f"{BD.model_stem(obj_id)}.ply", small.vertices, small.faces)
        src = source_info.get(str(obj_id), {})
        info[str(obj_id)] = models_info(small, src.get("symmetries_discrete"), src.get("symmetries_continuous"))
        report[obj_id] = (len(f), len(small.faces), used_voxel)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / BD.MODELS_INFO).write_text(json.dumps(dict(sorted(info.items(), key=lambda kv: int(kv[0]))), indent=2) + "\n")
    return report


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.decimate", description=__doc__.split("\n\n")[0])
    p.add_argument("--models", required=True, help="a BOP models directory: obj_NNNNNN.ply and models_info.json")
    p.add_argument("--out", default=None, help="default: <models>/../models_eval")
    size = p.add_mutually_exclusive_group()
    size.add_argument("--ratio", type=float, default=None, help="faces kept, as a fraction of the source's (default 0.025)")
    size.add_argument("--faces", type=int, default=None, help="faces kept at the most")
    size.add_argument("--voxel", type=float, default=None, help="the cell edge, in the models' units")
    p.add_argument("--contraction", choices=sorted(CONTRACTIONS), default="quadric")
    p.add_argument("--normals", action="store_true", help="write nx ny nz, recomputed on every decimated mesh")
    p.add_argument("--texture", action="store_true", help="bake a texture for the decimated mesh from the Gaussian model of -m")
    p.add_argument("-m", "--model_path", default=None, help="with --texture: the trained model directory of the object")
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--obj_id", type=int, default=None, help="with --texture: the object the model shows (default: the only one)")
    p.add_argument("--texel_cell", type=int, default=16, help="texels on the side of the atlas cell two faces share")
    p.add_argument("--scale", type=float, default=1000.0, help="model units -> the files' units (default: m -> mm)")
    p.add_argument("--n_views", type=int, default=96)
    p.add_argument("--image_size", type=int, default=512)
    a = p.parse_args(argv)
    ratio = a.ratio if a.ratio is not None else 0.025
    gaussians = None
    if a.texture:
        if a.model_path is None:
            p.error("--texture needs -m <model dir>")
        from .mesh import load_model
        gaussians = load_model(a.model_path, a.iteration)
    report = write_models_eval(a.models, a.out, ratio=ratio, faces=a.faces, voxel=a.voxel, contraction=a.contraction,
                               normals=a.normals, texture_model=gaussians, texture_obj_id=a.obj_id, texel_cell=a.texel_cell,
                               model_scale=a.scale, n_views=a.n_views, image_size=a.image_size)
    for obj_id, (before, after, used_voxel) in sorted(report.items()):
        print(f"{BD.model_stem(obj_id)}: {before} -> {after} faces at voxel {used_voxel:.6g}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
