"""The reconstructed environment as collision geometry: what the reference's ``PybulletEngine`` gets when ``pegasus.py`` calls
``add_object(select_env, ...)`` -- the environment's alpha-shape mesh as a static body, so that objects land on the table, the
counter or the clutter of the scan and not on a bare plane.  Here the environment is a signed distance field over a grid in
world coordinates: depth renders of the environment's Gaussian model are fused into a carved volume (``mesh.render_views``,
``mesh.integrate``) and ``pgr_sdf_from_tsdf`` turns that volume into a distance field over the whole grid, which
``pegasus_amd.dynamics`` takes as the ground and ``pegasus_amd.collision`` as one more body.  The rule stands at the top of
pegasus_amd/csrc/envfield.hip.h and in DESIGN.md section 25.

    python -m pegasus_amd.environment -m <model dir> --out env.npz [--bounds x0 y0 z0 x1 y1 z1 | --plane_size 2.0 --height 1.0]
                                      [--voxel 0.01] [--views 128] [--image_size 512] [--mesh env.ply]
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .mesh import MAX_VIEWS, Grid, Mesh

FLOOR_VOXELS = 4                 # the default bounds reach this many voxels below z = 0
TRUNCATION_VOXELS = 4.0


def sdf_from_tsdf(tsdf, grid: Grid, want_dist2: bool = False):
    """``pgr_sdf_from_tsdf``: the signed distance field float32 [nz,ny,nx] of a carved volume (device float32 [nz,ny,nx], inside
    where negative), and with ``want_dist2`` the exact squared distances int32 [nz,ny,nx] in voxels (-1: no point of the other
    sign).  Enqueued on the current stream."""
    import torch
    if not isinstance(tsdf, torch.Tensor) or tsdf.device.type != "cuda":
        raise RuntimeError("sdf_from_tsdf needs a tensor on a HIP device; there is no CPU path")
    if tuple(tsdf.shape) != grid.shape:
        raise ValueError(f"the volume is {tuple(tsdf.shape)}, the grid {grid.shape}")
    tsdf = tsdf.to(torch.float32).contiguous()
    sdf = torch.empty_like(tsdf)
    dist2 = torch.empty(grid.shape, dtype=torch.int32, device=tsdf.device) if want_dist2 else None
    ws = _lib.workspace("pgr_sdf_from_tsdf", tsdf.device, grid.nx, grid.ny, grid.nz)
    g = grid.struct()
    _lib.call("pgr_sdf_from_tsdf", tsdf.device, C.byref(g), _lib.ptr(tsdf), _lib.ptr(sdf), _lib.ptr(dist2), _lib.ptr(ws), ws.numel())
    return (sdf, dist2) if want_dist2 else sdf


def default_bounds(plane_size: float = 2.0, height: float = 1.0, voxel: float = 0.01):
    """The square of the reference's ``align2plane(plane_size)`` over z = 0, from four voxels below it to ``height`` above."""
    half = 0.5 * float(plane_size)
    return np.array([-half, -half, -FLOOR_VOXELS * float(voxel)]), np.array([half, half, float(height)])


def bounds_grid(lo, hi, voxel: float) -> Grid:
    """The grid of spacing ``voxel`` whose first point is ``lo`` and whose last reaches ``hi``."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all() and np.isfinite(voxel) and voxel > 0):
        raise ValueError("bounds must be finite with hi > lo, the voxel positive")
    n = [max(2, int(math.ceil(float(e) / voxel - 1e-9)) + 1) for e in hi - lo]
    if max(n) > 1024:
        raise ValueError(f"{n} grid points: at most 1024 per axis; use a larger voxel or tighter bounds")
    return Grid(n[0], n[1], n[2], tuple(float(x) for x in lo), float(voxel))


def _view_spec(camera, image_size: Optional[int] = None):
    """A ``rasterizer.ViewSpec`` with normalised depth of a ViewSpec, or of a ``cameras.Camera`` (``image_size``: its longer side in
    the render, the field of view kept)."""
    import torch
    from .rasterizer import ViewSpec
    if isinstance(camera, ViewSpec):
        return ViewSpec(camera.image_height, camera.image_width, camera.tanfovx, camera.tanfovy, camera.bg, camera.viewmatrix,
                        camera.projmatrix, camera.campos, depth_mode=_lib.PGR_DEPTH_NORMALIZED)
    W, H = int(camera.image_width), int(camera.image_height)
    if image_size:
        s = float(image_size) / max(W, H)
        W, H = max(1, round(W * s)), max(1, round(H * s))
    dev = camera.world_view_transform.device
    return ViewSpec(H, W, math.tan(0.5 * camera.FoVx), math.tan(0.5 * camera.FoVy), torch.zeros(3, device=dev),
                    camera.world_view_transform.float().contiguous(), camera.full_proj_transform.float().contiguous(),
                    camera.camera_center.float().contiguous(), depth_mode=_lib.PGR_DEPTH_NORMALIZED)


def subsample(items: Sequence, most: int) -> list:
    """At most ``most`` of ``items``, evenly spaced, the first and (for more than one) the last among them."""
    items = list(items)
    if len(items) <= most:
        return items
    if most == 1:
        return items[:1]
    return [items[int(round(k * (len(items) - 1) / (most - 1)))] for k in range(most)]


@dataclass
class EnvironmentField:
    """The environment's signed distance field in world coordinates: ``field`` float32 [nz,ny,nx] on the device, positive
    outside; ``friction`` is what the plane's friction is for the plane.  ``tsdf``: the carved volume it came from, where there
    is one."""
    field: object
    grid: Grid
    friction: float = 0.5
    tsdf: object = None

    def __post_init__(self):
        import torch
        if not isinstance(self.field, torch.Tensor) or self.field.device.type != "cuda":
            raise RuntimeError("EnvironmentField needs its field on a HIP device; there is no CPU path")
        if tuple(self.field.shape) != self.grid.shape:
            raise ValueError(f"the field is {tuple(self.field.shape)}, the grid {self.grid.shape}")
        if not (np.isfinite(self.friction) and self.friction >= 0):
            raise ValueError("friction must not be negative")
        self.field = self.field.to(torch.float32).contiguous()
        self.friction = float(self.friction)

    # ---- construction ---------------------------------------------------------------------------------------------------
    @staticmethod
    def from_tsdf(tsdf, grid: Grid, friction: float = 0.5) -> "EnvironmentField":
        """From a carved volume on the device (``mesh.integrate``'s): inside where negative."""
        return EnvironmentField(sdf_from_tsdf(tsdf, grid), grid, friction, tsdf)

    @staticmethod
    def from_gaussians(gaussians, cameras, bounds=None, voxel: float = 0.01, truncation: Optional[float] = None,
                       alpha_min: float = 0.5, max_views: int = MAX_VIEWS, image_size: Optional[int] = None,
                       friction: float = 0.5) -> "EnvironmentField":
        """Renders the model from ``cameras`` (ViewSpecs or ``cameras.Camera``s, subsampled evenly to ``max_views`` <= 256, all
        of one image size), fuses the depth into a carved volume over ``bounds`` (lo, hi; default: ``default_bounds``) and takes
        its distance field.  ``truncation`` defaults to four voxels."""
        from . import mesh as M
        if not 1 <= max_views <= MAX_VIEWS:
            raise ValueError(f"max_views must be 1..{MAX_VIEWS}")
        views = [_view_spec(c, image_size) for c in subsample(cameras, max_views)]
        if not views:
            raise ValueError("no cameras")
        lo, hi = default_bounds(voxel=voxel) if bounds is None else bounds
        grid = bounds_grid(lo, hi, voxel)
        depth, final_T = M.render_views(gaussians, views)
        tsdf = M.integrate(depth, final_T, views, grid, TRUNCATION_VOXELS * voxel if truncation is None else truncation, alpha_min)
        return EnvironmentField.from_tsdf(tsdf, grid, friction)

    @staticmethod
    def from_mesh(mesh, resolution: int = 96, padding: Optional[float] = None, friction: float = 0.5,
                  device="cuda") -> "EnvironmentField":
        """From a closed, outward-wound mesh in world coordinates, through ``collision.MeshSDF.from_mesh``."""
        from .collision import MeshSDF
        s = MeshSDF.from_mesh(mesh, resolution, padding, device)
        return EnvironmentField(s.field, s.grid, friction)

    # ---- queries ----------------------------------------------------------------------------------------------------------
    def signed_distance(self, points, gradient: bool = False):
        """``pgr_sdf_sample`` of the field at device ``points`` [...,3] (world coordinates)."""
        from .collision import sdf_sample
        return sdf_sample(self.field, self.grid, points, gradient)

    @property
    def voxel(self) -> float:
        return float(self.grid.voxel)

    def box(self):
        """(lo, hi) of the grid's box, float64."""
        lo = np.asarray(self.grid.origin, np.float64)
        return lo, lo + self.voxel * (np.array([self.grid.nx, self.grid.ny, self.grid.nz]) - 1.0)

    def top_under(self, xy_lo, xy_hi) -> float:
        """The z of the highest solid grid point whose (x, y) lies in the rectangle grown by a voxel; -inf without one."""
        lo, hi = self.box()
        g = self.grid
        x = lo[0] + self.voxel * np.arange(g.nx)
        y = lo[1] + self.voxel * np.arange(g.ny)
        mx = (x >= xy_lo[0] - self.voxel) & (x <= xy_hi[0] + self.voxel)
        my = (y >= xy_lo[1] - self.voxel) & (y <= xy_hi[1] + self.voxel)
        if not (mx.any() and my.any()):
            return -math.inf
        solid = (self.field < 0)[:, my][:, :, mx].any(dim=2).any(dim=1).cpu().numpy()
        k = np.flatnonzero(solid)
        return float(lo[2] + self.voxel * k[-1]) if len(k) else -math.inf

    def as_collision_body(self):
        """The environment as a ``collision.CollisionBody`` without shell points: a target of sweeps at the identity pose."""
        import torch
        from .collision import CollisionBody, MeshSDF
        empty = Mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
        return CollisionBody(empty, MeshSDF(self.grid, self.field), shell=torch.zeros((0, 3), dtype=torch.float32, device=self.field.device))

    def struct(self) -> _lib.PgrRigidGround:
        return _lib.PgrRigidGround(grid=self.grid.struct(), sdf=self.field.data_ptr(), friction=self.friction)

    def surface_mesh(self) -> Mesh:
        """``mesh.march`` on the carved volume (on the field where there is none): what the field's zero set looks like."""
        from .mesh import march
        return march(self.field if self.tsdf is None else self.tsdf, self.grid)

    # ---- files ------------------------------------------------------------------------------------------------------------
    def save(self, path) -> Path:
        """One .npz: the float32 field, the grid and the friction."""
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        g = self.grid
        with open(path, "wb") as f:
            np.savez_compressed(f, field=self.field.cpu().numpy(), shape=np.array([g.nx, g.ny, g.nz], np.int32),
                                origin=np.asarray(g.origin, np.float64), voxel=np.float64(g.voxel), friction=np.float64(self.friction))
        return path

    @staticmethod
    def load(path, device="cuda") -> "EnvironmentField":
        import torch
        with np.load(Path(path)) as z:
            nx, ny, nz = (int(v) for v in z["shape"])
            grid = Grid(nx, ny, nz, tuple(float(v) for v in z["origin"]), float(z["voxel"]))
            field = np.ascontiguousarray(z["field"], np.float32)
            friction = float(z["friction"])
        if field.shape != grid.shape:
            raise ValueError(f"{path}: the field is {field.shape}, the grid {grid.shape}")
        return EnvironmentField(torch.from_numpy(field).to(device), grid, friction)


def _parser():
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.environment", description=__doc__.split("\n\n")[0])
    p.add_argument("-m", "--model_path", required=True, help="the environment's model directory (point_cloud/, cameras.json)")
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--out", required=True, help="the .npz to write")
    p.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    p.add_argument("--plane_size", type=float, default=2.0, help="side of the square over z = 0 (without --bounds)")
    p.add_argument("--height", type=float, default=1.0, help="how far above z = 0 the grid reaches (without --bounds)")
    p.add_argument("--voxel", type=float, default=0.01)
    p.add_argument("--views", type=int, default=128, help="cameras of cameras.json used, evenly subsampled (at most 256)")
    p.add_argument("--image_size", type=int, default=512, help="the longer side of the depth renders")
    p.add_argument("--friction", type=float, default=0.5)
    p.add_argument("--mesh", default=None, metavar="PLY", help="also write the marched surface of the carved volume")
    return p


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = _parser().parse_args(argv)
    if not 1 <= a.views <= MAX_VIEWS:
        raise SystemExit(f"--views must be 1..{MAX_VIEWS}")
    from .mesh import load_model, write_ply
    from .scene import cameras_from_json
    cams = cameras_from_json(Path(a.model_path) / "cameras.json")
    if not cams:
        raise SystemExit("cameras.json holds no camera")
    sizes = {(c.image_width, c.image_height) for c in cams}
    if len(sizes) > 1:
        raise SystemExit(f"the cameras have {len(sizes)} image sizes; one is needed")
    bounds = (a.bounds[:3], a.bounds[3:]) if a.bounds else default_bounds(a.plane_size, a.height, a.voxel)
    env = EnvironmentField.from_gaussians(load_model(a.model_path, a.iteration), cams, bounds, a.voxel, max_views=a.views,
                                          image_size=a.image_size, friction=a.friction)
    env.save(a.out)
    g = env.grid
    solid = int((env.field < 0).sum())
    print(f"environment: {g.nx} x {g.ny} x {g.nz} points of {g.voxel:.6g}, {solid} solid -> {a.out}")
    if a.mesh:
        m = env.surface_mesh()
        write_ply(a.mesh, m)
        print(f"surface: {len(m.vertices)} vertices, {len(m.faces)} faces -> {a.mesh}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
