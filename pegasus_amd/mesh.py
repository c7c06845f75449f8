"""Watertight object meshes from trained Gaussian models: the step between training and physics / BOP records.

The reference builds an object's mesh and URDF from the trained model's point cloud with an open3d alpha shape.  Here
the model is rendered from a sphere of views (depth and alpha from one ``forward_views`` batch), the views are fused
into a truncated signed distance field with space carving (``pgr_tsdf_integrate``), and marching tetrahedra extracts
the closed outer surface (``pgr_march_count`` / ``pgr_march_emit``).  A density level set would not do: a trained
3DGS object is a shell of surface Gaussians, and its level set is two nested surfaces.

    python -m pegasus_amd.mesh -m <model dir> --out <dir> --obj_id N [--scale 1000] [--mass 0.1] [--resolution 256]
                               [--collision_faces N [--texture [--texel_cell 16]]] [--vertex_colors]

writes ``<out>/models/obj_NNNNNN.ply`` (scaled: BOP models are in mm; with ``--vertex_colors`` also ``nx ny nz red green
blue`` per vertex, from the views the mesh is fused from: ``pgr_mesh_vertex_normals`` / ``pgr_mesh_vertex_colors``,
DESIGN.md section 21) with its ``models_info.json`` entry, and
``<out>/urdf/obj_NNNNNN.{obj,urdf}`` in the model's own units for pybullet; with ``--collision_faces`` also
``<out>/urdf/obj_NNNNNN_collision.obj``, the mesh decimated by vertex clustering (``pegasus_amd.decimate``), as the URDF's
collision geometry; with ``--texture`` that mesh also gets a texture baked from the same sphere of views (``bake_texture``: a
per-face atlas, ``pgr_mesh_atlas_points`` / ``pgr_mesh_atlas_pack``), written as
``<out>/urdf/obj_NNNNNN_textured.{obj,mtl,png}`` and named in the URDF's ``<visual>``.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import xml.etree.ElementTree as ET
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib, bop_dataset as BD
from .ply_io import write_ply_mesh, write_ply_model

NEAR_Z = 0.2                 # pgr_common.h: the renderer culls everything closer than this
MAX_AXIS = 1024
MAX_VIEWS = 256


@dataclass
class Grid:
    """Grid point (i,j,k) sits at origin + voxel*(i,j,k); fields over it are [nz,ny,nx], x fastest."""
    nx: int
    ny: int
    nz: int
    origin: tuple
    voxel: float

    @property
    def shape(self):
        return (self.nz, self.ny, self.nx)

    def struct(self) -> _lib.PgrGrid:
        return _lib.PgrGrid(nx=int(self.nx), ny=int(self.ny), nz=int(self.nz),
                            origin=(C.c_float * 3)(*[float(x) for x in self.origin]), voxel=float(self.voxel))

    @staticmethod
    def around(lo, hi, resolution: int) -> "Grid":
        """The grid over the box [lo, hi] with ``resolution`` points on its longest axis, centred on the box."""
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        ext = hi - lo
        voxel = float(ext.max()) / (resolution - 1)
        n = [int(min(MAX_AXIS, max(2, math.ceil(e / voxel - 1e-9) + 1))) for e in ext]
        center = 0.5 * (lo + hi)
        origin = tuple(float(c - 0.5 * voxel * (k - 1)) for c, k in zip(center, n))
        return Grid(n[0], n[1], n[2], origin, voxel)


@dataclass
class Mesh:
    vertices: np.ndarray         # float32 [V,3]
    faces: np.ndarray            # int32 [F,3], outward winding
    normals: Optional[np.ndarray] = None     # float32 [V,3], unit length or 0 (vertex_normals)
    colors: Optional[np.ndarray] = None      # float32 [V,3] in 0..1 (vertex_colors)
    corner_uv: Optional[np.ndarray] = None   # float32 [F,3,2]: (u, v) per face corner, v = 0 at the image's bottom row
    texture: Optional[np.ndarray] = None     # uint8 [H,W,3] (bake_texture)

    def _tets(self):
        v = self.vertices.astype(np.float64)[self.faces]                  # [F,3,3]: tetrahedra (0, a, b, c)
        return v, np.einsum("fi,fi->f", v[:, 0], np.cross(v[:, 1], v[:, 2])) / 6.0

    def volume(self) -> float:
        """Enclosed volume (divergence theorem over the closed mesh)."""
        return float(self._tets()[1].sum())

    def center_of_mass(self) -> np.ndarray:
        v, vol = self._tets()
        return (vol[:, None] * v.sum(axis=1) / 4.0).sum(axis=0) / vol.sum()

    def inertia(self, mass: float) -> np.ndarray:
        """3x3 inertia tensor about the centre of mass, uniform density, total ``mass``."""
        v, vol = self._tets()
        s = v.sum(axis=1)
        second = (vol[:, None, None] / 20.0 * (np.einsum("fki,fkj->fij", v, v) + s[:, :, None] * s[:, None, :])).sum(axis=0)
        c = self.center_of_mass()
        cov = mass / vol.sum() * second - mass * np.outer(c, c)
        return np.trace(cov) * np.eye(3) - cov

    def largest_component(self) -> "Mesh":
        """The connected piece that encloses the most volume (a cavity's inward faces count negative), vertices
        renumbered in their old order."""
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        nv = len(self.vertices)
        if len(self.faces) == 0:
            return self
        f = self.faces.astype(np.int64)
        adj = coo_matrix((np.ones(2 * len(f)), (np.r_[f[:, 0], f[:, 1]], np.r_[f[:, 1], f[:, 2]])), shape=(nv, nv))
        n, label = connected_components(adj, directed=False)
        if n == 1:
            return self
        face_label = label[f[:, 0]]
        keep = face_label == np.bincount(face_label, weights=self._tets()[1], minlength=n).argmax()
        used = np.zeros(nv, bool)
        used[f[keep].ravel()] = True
        remap = np.cumsum(used) - 1
        return Mesh(self.vertices[used], remap[f[keep]].astype(np.int32),
                    normals=None if self.normals is None else self.normals[used],
                    colors=None if self.colors is None else self.colors[used])

    def scaled(self, scale: float) -> "Mesh":
        return Mesh((self.vertices.astype(np.float64) * scale).astype(np.float32), self.faces, normals=self.normals,
                    colors=self.colors, corner_uv=self.corner_uv, texture=self.texture)


# ---- the two GPU stages ---------------------------------------------------------------------------------------------
def integrate(depth, final_T, views, grid: Grid, truncation: float, alpha_min: float):
    """TSDF fusion with space carving (pgr_tsdf_integrate): float32 sdf [nz,ny,nx] on the device, positive outside.
    ``depth`` (normalised, depth mode 1) and ``final_T`` are device [V,H,W] (or [V,1,H,W]); ``views`` the V ViewSpecs
    (or GaussianRasterizationSettings) they were rendered with."""
    import torch
    from .rasterizer import camera_structs
    if not (1 <= len(views) <= MAX_VIEWS):
        raise ValueError(f"integrate takes 1..{MAX_VIEWS} views, got {len(views)}")
    device = depth.device
    if device.type != "cuda":
        raise RuntimeError("integrate needs tensors on a HIP device; there is no CPU path")
    V = len(views)
    depth = depth.reshape(V, *depth.shape[-2:]).float().contiguous()
    final_T = final_T.reshape(V, *final_T.shape[-2:]).float().contiguous()
    if depth.shape != final_T.shape or depth.shape[1:] != (int(views[0].image_height), int(views[0].image_width)):
        raise ValueError("depth and final_T must be [V,H,W] of the views' image size")
    cams, keep = camera_structs(views, device)
    sdf = torch.empty(grid.shape, dtype=torch.float32, device=device)
    g = grid.struct()
    _lib.call("pgr_tsdf_integrate", device, C.byref(g), V, cams, _lib.ptr(depth), _lib.ptr(final_T), float(truncation),
              float(alpha_min), _lib.ptr(sdf))
    del keep
    return sdf


def march(sdf, grid: Grid, stage_ms: Optional[dict] = None) -> Mesh:
    """Marching tetrahedra over a device sdf [nz,ny,nx] (inside: sdf < 0).  Reads the two counts once between the
    count and the emit pass: the only host wait.  ``stage_ms``: a dict that receives the GPU milliseconds of the
    "count" (count + scan) and "emit" passes."""
    import torch
    device = sdf.device
    if device.type != "cuda":
        raise RuntimeError("march needs a tensor on a HIP device; there is no CPU path")
    if tuple(sdf.shape) != grid.shape:
        raise ValueError(f"sdf is {tuple(sdf.shape)}, the grid {grid.shape}")
    sdf = sdf.float().contiguous()
    g = grid.struct()
    ws = _lib.workspace("pgr_march", device, grid.nx, grid.ny, grid.nz)
    stream_t = torch.cuda.current_stream(device)
    counts = torch.zeros(2, dtype=torch.int64, device=device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if stage_ms is not None else None
    if ev:
        ev[0].record(stream_t)
    _lib.call("pgr_march_count", device, C.byref(g), _lib.ptr(sdf), _lib.ptr(ws), ws.numel(), _lib.ptr(counts))
    if ev:
        ev[1].record(stream_t)
    nv, nf = (int(x) for x in counts.cpu())
    if nv >= 2 ** 31 or nf >= 2 ** 31:
        raise ValueError(f"{nv} vertices / {nf} faces: more than int32 indices hold; use a coarser grid")
    vertices = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=device)
    faces = torch.empty((max(nf, 1), 3), dtype=torch.int32, device=device)
    _lib.call("pgr_march_emit", device, C.byref(g), _lib.ptr(sdf), _lib.ptr(ws), ws.numel(), _lib.ptr(vertices),
              _lib.ptr(faces))
    if ev:
        ev[2].record(stream_t)
    out = Mesh(vertices[:nv].cpu().numpy(), faces[:nf].cpu().numpy())
    if ev:
        stage_ms["count"] = ev[0].elapsed_time(ev[1])
        stage_ms["emit"] = ev[1].elapsed_time(ev[2])
    return out


# ---- vertex attributes ----------------------------------------------------------------------------------------------
def _device_mesh(mesh_or_arrays, device):
    """(vertices float32 [V,3], faces int32 [F,3]) of a Mesh or a (vertices, faces) pair as contiguous tensors on
    ``device``; tensors are used where they are, and a host tensor is refused."""
    import torch
    v, f = (mesh_or_arrays.vertices, mesh_or_arrays.faces) if hasattr(mesh_or_arrays, "vertices") else mesh_or_arrays
    out = []
    for a, dt in ((v, torch.float32), (f, torch.int32)):
        if isinstance(a, torch.Tensor):
            if a.device.type != "cuda":
                raise RuntimeError("vertex attributes need tensors on a HIP device; there is no CPU path")
            out.append(a.to(dt).reshape(-1, 3).contiguous())
        else:
            if torch.device(device).type != "cuda":
                raise RuntimeError("vertex attributes need a HIP device; there is no CPU path")
            a = np.ascontiguousarray(a, np.float32 if dt == torch.float32 else np.int32).reshape(-1, 3)
            out.append(torch.from_numpy(a).to(device))
    return out


def vertex_normals_device(vertices, faces):
    """pgr_mesh_vertex_normals on device tensors: float32 [V,3] on the same device, enqueued on the current stream."""
    import torch
    if vertices.device.type != "cuda" or faces.device.type != "cuda":
        raise RuntimeError("vertex_normals needs tensors on a HIP device; there is no CPU path")
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    normals = torch.empty((V, 3), dtype=torch.float32, device=vertices.device)
    if V == 0:
        return normals
    ws = _lib.workspace("pgr_mesh_vertex_normals", vertices.device, V)
    _lib.call("pgr_mesh_vertex_normals", vertices.device, V, _lib.ptr(vertices), F, _lib.ptr(faces), _lib.ptr(normals),
              _lib.ptr(ws), ws.numel())
    return normals


def vertex_normals(mesh_or_arrays, device="cuda") -> np.ndarray:
    """Per-vertex normals float32 [V,3] of a Mesh or a (vertices, faces) pair by the rule of mesh_render.vertex_normals
    (the faces' unit normals summed per vertex, normalised), on the GPU and identical from run to run: the sums are
    64-bit integers of 2^-30 (pgr_mesh_vertex_normals).  A vertex of no face gets 0."""
    v, f = _device_mesh(mesh_or_arrays, device)
    return vertex_normals_device(v, f).cpu().numpy()


def vertex_colors(mesh, color, depth, final_T, views, *, depth_tol: float, alpha_min: float = 0.5, cos_min: float = 0.3,
                  fill=(0.5, 0.5, 0.5), on_device: bool = False):
    """(colors float32 [V,3] in 0..1, seen int32 [V]) of ``mesh`` from rendered views (pgr_mesh_vertex_colors); host arrays, or
    with ``on_device`` the device tensors (``mesh`` is anything with ``vertices`` and optionally ``normals``, arrays or
    tensors: bake_texture hands in the atlas' texel points).  ``color``
    [V,3,H,W] (rendered over a ZERO background), ``depth`` (normalised, depth mode 1) and ``final_T`` [V,H,W] are device
    tensors of ``views``.  A view counts for a vertex when the vertex projects into it, the pixel is opaque (alpha >=
    ``alpha_min``), its depth lies within ``depth_tol`` of the vertex's and, when the mesh has normals, the vertex faces
    the camera (cosine > ``cos_min``); the views that count are averaged with weight cosine^2.  ``seen`` is the number of
    views that counted; a vertex no view sees gets ``fill``."""
    import torch
    from .rasterizer import camera_structs
    if not (1 <= len(views) <= MAX_VIEWS):
        raise ValueError(f"vertex_colors takes 1..{MAX_VIEWS} views, got {len(views)}")
    device = depth.device
    if device.type != "cuda" or color.device.type != "cuda" or final_T.device.type != "cuda":
        raise RuntimeError("vertex_colors needs tensors on a HIP device; there is no CPU path")
    n = len(views)
    H, W = int(views[0].image_height), int(views[0].image_width)
    color = color.reshape(n, 3, *color.shape[-2:]).float().contiguous()
    depth = depth.reshape(n, *depth.shape[-2:]).float().contiguous()
    final_T = final_T.reshape(n, *final_T.shape[-2:]).float().contiguous()
    if tuple(depth.shape) != (n, H, W) or final_T.shape != depth.shape or tuple(color.shape) != (n, 3, H, W):
        raise ValueError("color must be [V,3,H,W], depth and final_T [V,H,W], of the views' image size")
    to_device = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float32))) \
        .to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
    vert = to_device(mesh.vertices)
    normals = getattr(mesh, "normals", None)
    if normals is not None:
        normals = to_device(normals)
        if normals.shape != vert.shape:
            raise ValueError("normals must be [V,3]")
    V = int(vert.shape[0])
    cams, keep = camera_structs(views, device)
    out = torch.empty((V, 3), dtype=torch.float32, device=device)
    seen = torch.empty((V,), dtype=torch.int32, device=device)
    fill_c = (C.c_float * 3)(*[float(x) for x in fill])
    _lib.call("pgr_mesh_vertex_colors", device, V, _lib.ptr(vert), _lib.ptr(normals), n, cams, _lib.ptr(color),
              _lib.ptr(depth), _lib.ptr(final_T), float(depth_tol), float(alpha_min), float(cos_min), fill_c, _lib.ptr(out),
              _lib.ptr(seen))
    result = (out, seen) if on_device else (out.cpu().numpy(), seen.cpu().numpy())
    del keep
    return result


def fill_unseen(mesh, colors, seen) -> np.ndarray:
    """``colors`` with every unseen vertex (``seen`` == 0) given the mean of its already-coloured edge neighbours, again and
    again until none is left or nothing changes (host plumbing: a sparse adjacency product in float64).  What stays
    unreachable keeps its colour."""
    from scipy.sparse import coo_matrix
    colors = np.asarray(colors, np.float32).reshape(-1, 3)
    nv = len(colors)
    known = np.asarray(seen).reshape(-1) > 0
    if known.all() or not known.any() or len(mesh.faces) == 0:
        return colors.copy()
    f = np.asarray(mesh.faces, np.int64).reshape(-1, 3)
    a, b = np.r_[f[:, 0], f[:, 1], f[:, 2]], np.r_[f[:, 1], f[:, 2], f[:, 0]]
    adj = coo_matrix((np.ones(2 * len(a)), (np.r_[a, b], np.r_[b, a])), shape=(nv, nv)).tocsr()
    adj.data[:] = 1.0                                                   # an edge counts once, however many faces share it
    out = colors.astype(np.float64)
    while not known.all():
        k = known.astype(np.float64)
        count = adj @ k
        reach = ~known & (count > 0)
        if not reach.any():
            break
        total = adj @ (out * k[:, None])
        out[reach] = total[reach] / count[reach, None]
        known = known | reach
    return out.astype(np.float32)


# ---- from a Gaussian model ------------------------------------------------------------------------------------------
def default_bounds(xyz: np.ndarray, opacity: np.ndarray):
    """Per axis the 0.5-99.5 percentile of the means of Gaussians with opacity >= 0.1, padded on every side by 10 % of
    the longest extent (a Gaussian reaches beyond its mean; a thin axis keeps the same margin as the long ones)."""
    sel = np.asarray(opacity).reshape(-1) >= 0.1
    pts = np.asarray(xyz, np.float64)[sel] if sel.any() else np.asarray(xyz, np.float64)
    lo, hi = np.percentile(pts, 0.5, axis=0), np.percentile(pts, 99.5, axis=0)
    pad = 0.1 * max(float((hi - lo).max()), 1e-6)
    return lo - pad, hi + pad


def sphere_views(center, half_diag: float, n_views: int, image_size: int):
    """The full Fibonacci sphere of look-at views around ``center`` at r = max(2.5 h, NEAR_Z + 2 h), with the field of
    view that holds the sphere of radius h (which holds the box) and a 5 % margin.  Returns (ViewSpecs, radius, fov)."""
    import torch
    from . import graphics as G
    from .rasterizer import ViewSpec
    from .scenes import make_view
    h = float(half_diag)
    r = max(2.5 * h, NEAR_Z + 2.0 * h)
    fov = 2.0 * math.atan(1.05 * h / math.sqrt(r * r - h * h))
    center = np.asarray(center, np.float64)
    specs = []
    for R, t in G.hemisphere_views(n_views, r, elev_range=(-0.5 * math.pi, 0.5 * math.pi)):
        eye = -R.T @ t + center
        v = make_view(R, -R @ eye, image_size, image_size, fovx=fov, fovy=fov)
        dev = lambda a: torch.as_tensor(np.asarray(a, np.float32), device="cuda")
        specs.append(ViewSpec(image_size, image_size, v.tanfovx, v.tanfovy, dev(np.zeros(3)), dev(v.world_view_transform),
                              dev(v.full_proj_transform), dev(v.camera_center), depth_mode=_lib.PGR_DEPTH_NORMALIZED))
    return specs, r, fov


def render_views(gaussians, views, stage_ms: Optional[dict] = None, want_color: bool = False):
    """Normalised depth and final_T [V,H,W] of ``views``, rendered in batches sized to the free device memory.
    ``want_color``: also the colour images [V,3,H,W] of the same renders, as a third value (over the views' background:
    sphere_views renders over zero, which vertex_colors needs)."""
    import torch
    from .rasterizer import forward_views
    xyz = gaussians.get_xyz.detach()
    n = int(xyz.shape[0])
    H, W = int(views[0].image_height), int(views[0].image_width)
    per_view = _lib.lib().pgr_batch_workspace_bytes(n, W, H, max(1 << 20, 6 * n), 1) + 6 * 4 * H * W
    free, _total = torch.cuda.mem_get_info(xyz.device)
    batch = int(max(1, min(32, len(views), (free // 4) // max(per_view, 1))))
    depth = torch.empty((len(views), H, W), dtype=torch.float32, device=xyz.device)
    final_T = torch.empty_like(depth)
    color = torch.empty((len(views), 3, H, W), dtype=torch.float32, device=xyz.device) if want_color else None
    kw = dict(shs=gaussians.get_features.detach(), scales=gaussians.get_scaling.detach(),
              rotations=gaussians.get_rotation.detach(), sh_degree=int(gaussians.active_sh_degree))
    opac = gaussians.get_opacity.detach()
    start = torch.cuda.Event(enable_timing=True) if stage_ms is not None else None
    if start:
        start.record()
    for b in range(0, len(views), batch):
        outs = forward_views(xyz, opac, views[b:b + batch], want_radii=False, want_aux=True, **kw)
        for k, r in enumerate(outs):
            depth[b + k] = r["depth"][0]
            final_T[b + k] = r["final_T"]
            if want_color:
                color[b + k] = r["color"]
    if start:
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        end.synchronize()
        stage_ms["render"] = start.elapsed_time(end)
    return (depth, final_T, color) if want_color else (depth, final_T)


def _model_bounds(gaussians, bounds):
    if bounds is None:
        bounds = default_bounds(gaussians.get_xyz.detach().cpu().numpy(), gaussians.get_opacity.detach().cpu().numpy())
    return tuple(np.asarray(b, np.float64) for b in bounds)


def _attributes(mesh: Mesh, color, depth, final_T, views, depth_tol: float, alpha_min: float, cos_min: float,
                stage_ms: Optional[dict] = None, info: Optional[dict] = None) -> Mesh:
    """``mesh`` with normals (vertex_normals) and colours (vertex_colors, then fill_unseen) from the rendered views."""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if stage_ms is not None else None
    if ev:
        ev[0].record()
    normals = vertex_normals(mesh, device=depth.device)
    if ev:
        ev[1].record()
    with_normals = Mesh(mesh.vertices, mesh.faces, normals=normals)
    colors, seen = vertex_colors(with_normals, color, depth, final_T, views, depth_tol=depth_tol, alpha_min=alpha_min,
                                 cos_min=cos_min)
    if ev:
        ev[2].record()
        ev[2].synchronize()
        stage_ms["normals"] = ev[0].elapsed_time(ev[1])
        stage_ms["colors"] = ev[1].elapsed_time(ev[2])
    if info is not None:
        info["unseen"] = int((seen == 0).sum())
        info["vertices"] = int(len(seen))
    with_normals.colors = fill_unseen(mesh, colors, seen)
    return with_normals


def extract_mesh(gaussians, *, resolution: int = 256, n_views: int = 96, image_size: int = 512, alpha_min: float = 0.5,
                 truncation_voxels: float = 4.0, bounds=None, stage_ms: Optional[dict] = None, colors: bool = False,
                 depth_tol_voxels: float = 2.0, cos_min: float = 0.3, info: Optional[dict] = None) -> Mesh:
    """The closed outer surface of a GaussianModel (read through its activated getters), in the model's units.
    ``bounds``: (lo[3], hi[3]) of the grid, default default_bounds().  ``resolution``: grid points on the longest axis.
    ``stage_ms``: a dict that receives the GPU milliseconds of the render, integrate, count and emit stages (and of the
    normals and colors stages with ``colors``).
    ``colors``: the mesh also carries ``normals`` and ``colors``, taken from the same renders (the views are rendered once):
    a view colours a vertex when its depth there lies within ``depth_tol_voxels`` voxels of the vertex and the vertex faces
    it by more than ``cos_min``; vertices no view sees take their neighbours' colours (fill_unseen).  Vertices and faces are
    the same either way.  ``info``: a dict that receives the number of ``vertices`` and of those ``unseen`` before the fill."""
    import torch
    if not (2 <= resolution <= MAX_AXIS):
        raise ValueError(f"resolution must be 2..{MAX_AXIS}")
    lo, hi = _model_bounds(gaussians, bounds)
    grid = Grid.around(lo, hi, resolution)
    views, _r, _fov = sphere_views(0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo)), n_views, image_size)
    if len(views) > MAX_VIEWS:
        raise ValueError(f"n_views: at most {MAX_VIEWS} views are fused")
    color = None
    if colors:
        depth, final_T, color = render_views(gaussians, views, stage_ms, want_color=True)
    else:
        depth, final_T = render_views(gaussians, views, stage_ms)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if stage_ms is not None else None
    if ev:
        ev[0].record()
    sdf = integrate(depth, final_T, views, grid, truncation_voxels * grid.voxel, alpha_min)
    if ev:
        ev[1].record()
    mesh = march(sdf, grid, stage_ms)
    if ev:
        stage_ms["integrate"] = ev[0].elapsed_time(ev[1])
    # a trained shell has gaps: rays through them carve pockets inside, and an unseen speck may stay outside; the body
    # is the largest closed piece
    mesh = mesh.largest_component()
    if colors:
        mesh = _attributes(mesh, color, depth, final_T, views, depth_tol_voxels * grid.voxel, alpha_min, cos_min, stage_ms,
                           info)
    return mesh


def colorize(gaussians, mesh: Mesh, *, n_views: int = 96, image_size: int = 512, alpha_min: float = 0.5,
             depth_tol: Optional[float] = None, cos_min: float = 0.3, bounds=None, stage_ms: Optional[dict] = None,
             info: Optional[dict] = None) -> Mesh:
    """``mesh`` (in the model's frame: an extracted mesh, or one decimated from it) with normals and colours from renders of
    ``gaussians`` on the sphere of views extract_mesh uses.  ``depth_tol``: how far a view's depth may lie from a vertex, in
    the model's units; default 2 voxels of extract_mesh's default grid (the longest side of the bounds / 255)."""
    lo, hi = _model_bounds(gaussians, bounds)
    if depth_tol is None:
        depth_tol = 2.0 * float((hi - lo).max()) / 255.0
    views, _r, _fov = sphere_views(0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo)), n_views, image_size)
    if len(views) > MAX_VIEWS:
        raise ValueError(f"n_views: at most {MAX_VIEWS} views are used")
    depth, final_T, color = render_views(gaussians, views, stage_ms, want_color=True)
    return _attributes(Mesh(mesh.vertices, mesh.faces), color, depth, final_T, views, depth_tol, alpha_min, cos_min, stage_ms,
                       info)


# ---- a texture for a (decimated) mesh: a per-face atlas baked from the views ---------------------------------------------
MAX_ATLAS_SIDE = 8192
MIN_ATLAS_CELL = 4


def texture_atlas_layout(n_faces: int, cell: int):
    """(width, height, cols, rows, corner_uv float32 [F,3,2]) of the per-face atlas (the layout pinned in csrc/meshattr.hip.h;
    this is the one place it is computed, the library checks the size it is handed against its own).  Two faces share a cell
    of ``cell`` x ``cell`` texels as two right triangles with legs of ``cell`` - 3 texels; face f lies in cell f >> 1, half
    f & 1.  Corner UVs are u = X / width, v = 1 - Y / height of the corners' texel-centre coordinates (X right, Y down from the
    top-left), computed in float64 and rounded once."""
    F, s = int(n_faces), int(cell)
    if F < 1:
        raise ValueError("a texture atlas needs at least one face")
    if s < MIN_ATLAS_CELL:
        raise ValueError(f"cell must be at least {MIN_ATLAS_CELL} texels, got {s}")
    cells = (F + 1) // 2
    cols = math.isqrt(cells - 1) + 1
    rows = -(-cells // cols)
    if cols * s > MAX_ATLAS_SIDE:
        raise ValueError(f"{F} faces at cell {s} need an atlas {cols * s} texels wide; at most {MAX_ATLAS_SIDE}: the largest "
                         f"cell that fits is {MAX_ATLAS_SIDE // cols}" + ("" if MAX_ATLAS_SIDE // cols >= MIN_ATLAS_CELL else
                                                                          f" (below {MIN_ATLAS_CELL}: decimate the mesh first)"))
    width, height, L = cols * s, rows * s, s - 3
    f = np.arange(F)
    c, half = f >> 1, (f & 1)[:, None]
    origin = np.stack([(c % cols) * s, (c // cols) * s], 1).astype(np.float64)                      # [F,2]
    local0 = np.array([[0.5, 0.5], [0.5 + L, 0.5], [0.5, 0.5 + L]])
    local = np.where(half[:, :, None] == 0, local0[None], s - local0[None])                          # [F,3,2]
    xy = origin[:, None, :] + local
    corner_uv = np.stack([xy[..., 0] / width, 1.0 - xy[..., 1] / height], -1).astype(np.float32)
    return width, height, cols, rows, corner_uv


def atlas_points(vertices, faces, cell: int):
    """pgr_mesh_atlas_points on device tensors (vertices float32 [V,3], faces int32 [F,3]): (points float32 [H*W,3], normals
    float32 [H*W,3], face_of_texel int32 [H*W]) of every atlas texel, on the same device, and (width, height)."""
    import torch
    if vertices.device.type != "cuda" or faces.device.type != "cuda":
        raise RuntimeError("atlas_points needs tensors on a HIP device; there is no CPU path")
    width, height = texture_atlas_layout(int(faces.shape[0]), cell)[:2]
    n = width * height
    points = torch.empty((n, 3), dtype=torch.float32, device=vertices.device)
    normals = torch.empty_like(points)
    owner = torch.empty((n,), dtype=torch.int32, device=vertices.device)
    _lib.call("pgr_mesh_atlas_points", vertices.device, int(vertices.shape[0]), _lib.ptr(vertices), int(faces.shape[0]), _lib.ptr(faces),
              int(cell), width, height, _lib.ptr(points), _lib.ptr(normals), _lib.ptr(owner))
    return points, normals, owner, (width, height)


def atlas_pack(n_faces: int, cell: int, face_of_texel, colors, seen, face_fill=None, fill=(128, 128, 128)):
    """pgr_mesh_atlas_pack on device tensors: (texture uint8 [H,W,3], face_seen int32 [F]) on the same device.  ``face_fill``:
    uint8 [F,3] (array or tensor) for the faces no view sees, else ``fill``."""
    import torch
    device = colors.device
    if device.type != "cuda":
        raise RuntimeError("atlas_pack needs tensors on a HIP device; there is no CPU path")
    width, height = texture_atlas_layout(n_faces, cell)[:2]
    colors = colors.to(torch.float32).reshape(-1, 3).contiguous()
    seen = seen.to(torch.int32).reshape(-1).contiguous()
    face_of_texel = face_of_texel.to(torch.int32).reshape(-1).contiguous()
    if not (colors.shape[0] == seen.shape[0] == face_of_texel.shape[0] == width * height):
        raise ValueError(f"colors, seen and face_of_texel must hold the atlas' {width} x {height} texels")
    if face_fill is not None:
        face_fill = torch.as_tensor(np.ascontiguousarray(face_fill, np.uint8) if not isinstance(face_fill, torch.Tensor) else face_fill)
        face_fill = face_fill.to(device=device, dtype=torch.uint8).reshape(-1, 3).contiguous()
        if face_fill.shape[0] != n_faces:
            raise ValueError("face_fill must be [F,3]")
    texture = torch.empty((height, width, 3), dtype=torch.uint8, device=device)
    face_seen = torch.empty((n_faces,), dtype=torch.int32, device=device)
    fill_c = (C.c_uint8 * 3)(*[int(x) for x in fill])
    _lib.call("pgr_mesh_atlas_pack", device, int(n_faces), int(cell), width, height, _lib.ptr(face_of_texel), _lib.ptr(colors),
              _lib.ptr(seen), _lib.ptr(face_fill), fill_c, _lib.ptr(texture), _lib.ptr(face_seen))
    return texture, face_seen


def bake_views(mesh: Mesh, color, depth, final_T, views, *, cell: int = 16, depth_tol: float, alpha_min: float = 0.5,
               cos_min: float = 0.3, stage_ms: Optional[dict] = None, info: Optional[dict] = None) -> Mesh:
    """``mesh`` with ``corner_uv`` and ``texture`` baked from rendered views (the tensors vertex_colors takes): the texels'
    surface points (pgr_mesh_atlas_points), coloured by the per-point rule of the vertex colours (pgr_mesh_vertex_colors,
    unchanged: same views, tolerances and weights), quantised and filled per face (pgr_mesh_atlas_pack).  Faces no view sees
    take the mean of the mesh's own vertex colours when it has them, else mid grey.  ``info`` receives ``face_seen`` (int32
    [F]: the seen texels of every face) and ``atlas`` = (width, height); ``stage_ms`` the milliseconds of the three stages."""
    import torch
    from types import SimpleNamespace
    device = depth.device
    vert, faces = _device_mesh(mesh, device)
    F = int(faces.shape[0])
    corner_uv = texture_atlas_layout(F, cell)[4]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if stage_ms is not None else None
    if ev:
        ev[0].record()
    points, normals, owner, _size = atlas_points(vert, faces, cell)
    if ev:
        ev[1].record()
    colors, seen = vertex_colors(SimpleNamespace(vertices=points, normals=normals), color, depth, final_T, views, depth_tol=depth_tol,
                                 alpha_min=alpha_min, cos_min=cos_min, on_device=True)
    if ev:
        ev[2].record()
    face_fill = None
    if mesh.colors is not None:
        mean = np.asarray(mesh.colors, np.float64).reshape(-1, 3)[np.asarray(mesh.faces, np.int64)].mean(1)
        face_fill = np.rint(255.0 * np.clip(mean, 0.0, 1.0)).astype(np.uint8)
    texture, face_seen = atlas_pack(F, cell, owner, colors, seen, face_fill)
    if ev:
        ev[3].record()
        ev[3].synchronize()
        for k, name in enumerate(("atlas_points", "atlas_colors", "atlas_pack")):
            stage_ms[name] = ev[k].elapsed_time(ev[k + 1])
    texture = texture.cpu().numpy()
    if info is not None:
        info["face_seen"] = face_seen.cpu().numpy()
        info["atlas"] = (int(texture.shape[1]), int(texture.shape[0]))
    return Mesh(mesh.vertices, mesh.faces, normals=mesh.normals, colors=mesh.colors, corner_uv=corner_uv, texture=texture)


def bake_texture(gaussians, mesh: Mesh, *, cell: int = 16, n_views: int = 96, image_size: int = 512, alpha_min: float = 0.5,
                 depth_tol: Optional[float] = None, cos_min: float = 0.3, bounds=None, stage_ms: Optional[dict] = None,
                 info: Optional[dict] = None) -> Mesh:
    """``mesh`` (in the model's frame; typically decimated) with a texture baked from renders of ``gaussians``: colorize's
    arguments, sphere of views and default ``depth_tol``, but the appearance goes into ``cell`` x ``cell`` texels per pair of
    faces (bake_views) instead of one colour per vertex.  Returns the mesh with ``corner_uv`` [F,3,2] and ``texture`` uint8
    [H,W,3]; ``info`` receives ``face_seen``."""
    texture_atlas_layout(len(mesh.faces), cell)                         # refuse an atlas that cannot be built before rendering
    lo, hi = _model_bounds(gaussians, bounds)
    if depth_tol is None:
        depth_tol = 2.0 * float((hi - lo).max()) / 255.0
    views, _r, _fov = sphere_views(0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo)), n_views, image_size)
    if len(views) > MAX_VIEWS:
        raise ValueError(f"n_views: at most {MAX_VIEWS} views are used")
    depth, final_T, color = render_views(gaussians, views, stage_ms, want_color=True)
    return bake_views(mesh, color, depth, final_T, views, cell=cell, depth_tol=depth_tol, alpha_min=alpha_min, cos_min=cos_min,
                      stage_ms=stage_ms, info=info)


# ---- files ----------------------------------------------------------------------------------------------------------
def write_ply(path, mesh: Mesh, scale: float = 1.0):
    """Binary PLY with vertex and face elements; vertices multiplied by ``scale`` (1000: metres -> BOP millimetres).  A mesh
    with normals or colours is written in the property order of a BOP model file (ply_io.write_ply_model): normals as
    float, colours as uchar = rint(255 c).  A mesh that carries a texture is written with its corner UVs as the face
    element's ``texcoord`` list, a ``comment TextureFile <stem>.png`` line, and the image as ``<stem>.png`` beside the file."""
    textured = getattr(mesh, "texture", None) is not None and getattr(mesh, "corner_uv", None) is not None
    if mesh.normals is None and mesh.colors is None and not textured:
        write_ply_mesh(path, mesh.scaled(scale).vertices, mesh.faces)
        return
    colors = mesh.colors
    if colors is not None:
        colors = np.rint(255.0 * np.clip(np.asarray(colors, np.float64), 0.0, 1.0)).astype(np.uint8)
    if not textured:
        write_ply_model(path, mesh.scaled(scale).vertices, mesh.faces, normals=mesh.normals, colors=colors)
        return
    path = Path(path)
    write_ply_model(path, mesh.scaled(scale).vertices, mesh.faces, normals=mesh.normals, colors=colors,
                    texture_uv_face=np.asarray(mesh.corner_uv, np.float32).reshape(-1, 6), texture_file=path.stem + ".png")
    path.with_suffix(".png").write_bytes(BD.encode_png(np.ascontiguousarray(mesh.texture, np.uint8)))


def write_obj_textured(path, mesh: Mesh, texture_name: str):
    """Wavefront OBJ with texture coordinates: ``v``, one ``vt`` per face corner, ``f a/ta b/tb c/tc``, and ``<stem>.mtl``
    beside it whose ``map_Kd`` names ``texture_name`` (relative to the OBJ).  The image itself is neither read nor written
    here: whoever passes the name puts it there."""
    if getattr(mesh, "corner_uv", None) is None:
        raise ValueError("write_obj_textured needs a mesh with corner_uv")
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    uv = np.asarray(mesh.corner_uv, np.float32).reshape(-1, 2)
    f = np.asarray(mesh.faces, np.int64).reshape(-1, 3) + 1
    t = np.arange(1, 3 * len(f) + 1).reshape(-1, 3)
    with open(path, "w") as fh:
        fh.write(f"# closed mesh extracted from a Gaussian model, textured\nmtllib {path.stem}.mtl\nusemtl material_0\n")
        np.savetxt(fh, mesh.vertices, fmt="v %.9g %.9g %.9g")
        np.savetxt(fh, uv, fmt="vt %.9g %.9g")
        np.savetxt(fh, np.stack([f, t], 2).reshape(-1, 6), fmt="f %d/%d %d/%d %d/%d")
    path.with_suffix(".mtl").write_text(f"newmtl material_0\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {texture_name}\n")


def write_obj(path, mesh: Mesh):
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        f.write("# closed mesh extracted from a Gaussian model\n")
        np.savetxt(f, mesh.vertices, fmt="v %.9g %.9g %.9g")
        np.savetxt(f, mesh.faces.astype(np.int64) + 1, fmt="f %d %d %d")


def write_urdf(path, mesh_filename: str, mesh: Mesh, mass: float, collision_filename: Optional[str] = None,
               visual_filename: Optional[str] = None):
    """One link: visual and collision are the mesh file, the inertial block holds the mesh's centre of mass, ``mass``
    and inertia about the centre of mass at uniform density.  ``collision_filename``: another (coarser) mesh file for the
    ``<collision>`` element only; ``visual_filename``: another (textured) one for ``<visual>`` only; the inertial block
    still comes from ``mesh``."""
    c = mesh.center_of_mass()
    I = mesh.inertia(mass)
    robot = ET.Element("robot", name=Path(mesh_filename).stem)
    link = ET.SubElement(robot, "link", name="base_link")
    inertial = ET.SubElement(link, "inertial")
    ET.SubElement(inertial, "origin", xyz=" ".join(f"{x:.9g}" for x in c), rpy="0 0 0")
    ET.SubElement(inertial, "mass", value=f"{mass:.9g}")
    ET.SubElement(inertial, "inertia", ixx=f"{I[0, 0]:.9g}", ixy=f"{I[0, 1]:.9g}", ixz=f"{I[0, 2]:.9g}",
                  iyy=f"{I[1, 1]:.9g}", iyz=f"{I[1, 2]:.9g}", izz=f"{I[2, 2]:.9g}")
    for tag in ("visual", "collision"):
        e = ET.SubElement(link, tag)
        ET.SubElement(e, "origin", xyz="0 0 0", rpy="0 0 0")
        filename = collision_filename if tag == "collision" and collision_filename is not None else mesh_filename
        if tag == "visual" and visual_filename is not None:
            filename = visual_filename
        ET.SubElement(ET.SubElement(e, "geometry"), "mesh", filename=str(filename), scale="1 1 1")
    ET.indent(robot)
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text('<?xml version="1.0"?>\n' + ET.tostring(robot, encoding="unicode") + "\n")


def _diameter(points: np.ndarray) -> float:
    from scipy.spatial import ConvexHull
    p = np.asarray(points, np.float64)
    if len(p) >= 4:
        try:
            p = p[ConvexHull(p).vertices]
        except Exception:          # flat or degenerate point set: every point is a candidate
            pass
    best = 0.0
    for a in range(0, len(p), 1024):
        d2 = ((p[a:a + 1024, None, :] - p[None, :, :]) ** 2).sum(axis=-1)
        best = max(best, float(d2.max()))
    return math.sqrt(best)


def models_info(mesh: Mesh, symmetries_discrete=None, symmetries_continuous=None) -> dict:
    """The BOP models_info.json fields of ``mesh`` (in its units): diameter (largest distance between two vertices of
    the convex hull), min_x/y/z and size_x/y/z of the bounding box.  ``symmetries_discrete`` (a list of 4x4 transforms as 16
    numbers, row-major, whose 3x3 part must be a rotation to 1e-6) and ``symmetries_continuous`` (a list of {'axis': [3],
    'offset': [3]}, or of 6 numbers ax ay az ox oy oz) are passed through in the toolkit's layout when given."""
    v = mesh.vertices.astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    info = {"diameter": _diameter(v)}
    for a, name in enumerate("xyz"):
        info[f"min_{name}"] = float(lo[a])
    for a, name in enumerate("xyz"):
        info[f"size_{name}"] = float(hi[a] - lo[a])
    if symmetries_discrete:
        out = []
        for sym in symmetries_discrete:
            m = np.asarray(sym, np.float64).reshape(-1)
            if m.size != 16:
                raise ValueError(f"a discrete symmetry is 16 numbers (4x4, row-major), got {m.size}")
            R = m.reshape(4, 4)[:3, :3]
            if np.abs(R.dot(R.T) - np.eye(3)).max() > 1e-6 or abs(np.linalg.det(R) - 1.0) > 1e-6:
                raise ValueError("the 3x3 part of a discrete symmetry must be a rotation (to 1e-6)")
            out.append([float(x) for x in m])
        info["symmetries_discrete"] = out
    if symmetries_continuous:
        out = []
        for sym in symmetries_continuous:
            if isinstance(sym, dict):
                axis, offset = sym["axis"], sym["offset"]
            else:
                flat = np.asarray(sym, np.float64).reshape(-1)
                if flat.size != 6:
                    raise ValueError(f"a continuous symmetry is 6 numbers (axis, offset), got {flat.size}")
                axis, offset = flat[:3], flat[3:]
            axis, offset = [float(x) for x in axis], [float(x) for x in offset]
            if len(axis) != 3 or len(offset) != 3 or not any(axis):
                raise ValueError("a continuous symmetry needs a non-zero axis [3] and an offset [3]")
            out.append({"axis": axis, "offset": offset})
        info["symmetries_continuous"] = out
    return info


# ---- CLI ------------------------------------------------------------------------------------------------------------
def load_model(model_dir, iteration: int = -1, clean_pcd: bool = False):
    """The GaussianModel saved under <model_dir>/point_cloud/iteration_N/point_cloud.ply (N = the largest for -1);
    ``clean_pcd``: without its floaters (GaussianModel.load_ply)."""
    from .gaussian_model import GaussianModel
    from .ply_io import read_ply_vertices
    from .scene import searchForMaxIteration
    pc = os.path.join(model_dir, "point_cloud")
    it = searchForMaxIteration(pc) if iteration == -1 else iteration
    path = os.path.join(pc, f"iteration_{it}", "point_cloud.ply")
    n_rest = sum(1 for n in read_ply_vertices(path).dtype.names if n.startswith("f_rest_"))
    degree = int(round(math.sqrt((n_rest + 3) / 3))) - 1
    g = GaussianModel(degree)
    g.load_ply(path, clean_pcd=clean_pcd)
    return g


def _parser():
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.mesh", description=__doc__.split("\n\n")[0])
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--out", required=True)
    p.add_argument("--obj_id", type=int, required=True)
    p.add_argument("--scale", type=float, default=1000.0, help="model units -> BOP units (default: m -> mm)")
    p.add_argument("--mass", type=float, default=0.1, help="kg, for the URDF")
    p.add_argument("--resolution", type=int, default=256)
    p.add_argument("--n_views", type=int, default=96)
    p.add_argument("--image_size", type=int, default=512)
    p.add_argument("--clean_pcd", action="store_true",
                   help="drop the model's floaters first: the radius-outlier filter (16 points, 0.03) of load_ply")
    p.add_argument("--collision_faces", type=int, default=None, metavar="N",
                   help="also write urdf/<name>_collision.obj, the mesh decimated to at most N faces by vertex clustering "
                        "(pegasus_amd.decimate.simplify_to), and name it in the URDF's <collision> element")
    p.add_argument("--vertex_colors", action="store_true",
                   help="models/<name>.ply also carries nx ny nz red green blue, from the views the mesh is fused from")
    p.add_argument("--texture", action="store_true",
                   help="with --collision_faces: bake a texture for the decimated mesh from the same sphere of views (bake_texture) and "
                        "write urdf/<name>_textured.{obj,mtl,png}, named in the URDF's <visual> element")
    p.add_argument("--texel_cell", type=int, default=16, help="with --texture: texels on the side of the atlas cell two faces share")
    p.add_argument("--sym_continuous", type=float, nargs=6, action="append", metavar=("AX", "AY", "AZ", "OX", "OY", "OZ"),
                   help="a continuous rotational symmetry: axis and a point on it, in model units (repeatable)")
    p.add_argument("--sym_discrete", type=float, nargs=16, action="append", metavar="M",
                   help="a discrete symmetry: a 4x4 transform, row-major, in model units (repeatable)")
    return p


def scaled_symmetries(sym_discrete, sym_continuous, scale: float):
    """The command line's symmetries (model units) in the units of the written model: translations and offsets times scale."""
    disc = []
    for m in sym_discrete or []:
        m = np.asarray(m, np.float64).reshape(4, 4).copy()
        m[:3, 3] *= scale
        disc.append(m.reshape(16).tolist())
    cont = [{"axis": list(c[:3]), "offset": [float(o) * scale for o in c[3:]]} for c in sym_continuous or []]
    return disc or None, cont or None


def main(argv: Optional[Sequence[str]] = None) -> int:
    parser = _parser()
    a = parser.parse_args(argv)
    if a.texture and a.collision_faces is None:
        parser.error("--texture textures the decimated mesh: it needs --collision_faces")
    gaussians = load_model(a.model_path, a.iteration, a.clean_pcd)
    mesh = extract_mesh(gaussians, resolution=a.resolution, n_views=a.n_views, image_size=a.image_size, colors=a.vertex_colors)
    name = BD.model_stem(a.obj_id)
    out = Path(a.out)
    write_ply(out / "models" / f"{name}.ply", mesh, scale=a.scale)
    info = BD.read_models_info(out / "models")
    disc, cont = scaled_symmetries(a.sym_discrete, a.sym_continuous, a.scale)
    info[str(a.obj_id)] = models_info(mesh.scaled(a.scale), disc, cont)
    (out / "models" / BD.MODELS_INFO).write_text(json.dumps(dict(sorted(info.items(), key=lambda kv: int(kv[0]))), indent=2) + "\n")
    write_obj(out / "urdf" / f"{name}.obj", mesh)
    collision = None
    if a.collision_faces is not None:
        from .decimate import simplify_to
        coarse, _voxel = simplify_to(mesh, a.collision_faces)
        collision = f"{name}_collision.obj"
        write_obj(out / "urdf" / collision, coarse)
    visual = None
    if a.texture:
        baked = bake_texture(gaussians, coarse, cell=a.texel_cell, n_views=a.n_views, image_size=a.image_size)
        visual = f"{name}_textured.obj"
        write_obj_textured(out / "urdf" / visual, baked, f"{name}_textured.png")
        (out / "urdf" / f"{name}_textured.png").write_bytes(BD.encode_png(baked.texture))
    write_urdf(out / "urdf" / f"{name}.urdf", f"{name}.obj", mesh, a.mass, collision_filename=collision, visual_filename=visual)
    print(f"{name}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces, volume {mesh.volume():.6g}, "
          f"written under {out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
