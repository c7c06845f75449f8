"""The inputs of the mesh tests, built in NumPy alone so that the host tests run both references on exactly what the
device tests feed the kernels: the TSDF cases (grid, views, depth, final_T, thresholds, and the branches each case is
there to reach) and the sdf fields of the marching cases."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

import mesh_reference as R
from pegasus_amd import graphics as G
from pegasus_amd.mesh import Grid
from pegasus_amd.scenes import make_view


# ---- views ----------------------------------------------------------------------------------------------------------
def raw_views_around(center, dist, n, width, height, fovx, fovy):
    """n look-at views on the full Fibonacci sphere of radius ``dist`` around ``center`` (scenes.View, NumPy)."""
    raw = []
    for Rm, t in G.hemisphere_views(n, dist, elev_range=(-0.5 * math.pi, 0.5 * math.pi))[:n]:
        eye = -Rm.T @ t + np.asarray(center, np.float64)
        raw.append(make_view(Rm, -Rm @ eye, width, height, fovx=fovx, fovy=fovy))
    return raw


def looking_away(view):
    """The same camera turned half round about its y axis: the whole scene ``view`` looks at is behind it."""
    R_w2c = np.diag([-1.0, 1.0, -1.0]) @ view.R_c2w.T
    eye = -view.R_c2w @ view.t_w2c
    return make_view(R_w2c, -R_w2c @ eye, view.width, view.height, fovx=view.fovx, fovy=view.fovy)


# ---- TSDF cases -----------------------------------------------------------------------------------------------------
@dataclass
class TsdfCase:
    grid: Grid
    raw: list                    # scenes.View per view
    depth: np.ndarray            # [V,H,W] float32
    final_T: np.ndarray          # [V,H,W] float32
    truncation: float
    alpha_min: float = 0.5
    reaches: tuple = ()          # the census keys (mesh_reference.CENSUS_KEYS) this case is there for: each must be > 0
    blind_views: tuple = ()      # views that must hold no grid point in their image

    def reference_args(self):
        return (self.grid, [v.world_view_transform.reshape(16) for v in self.raw], [v.tanfovx for v in self.raw],
                [v.tanfovy for v in self.raw], self.depth, self.final_T, self.truncation, self.alpha_min)


def grid_center(grid):
    return np.array([grid.origin[a] + 0.5 * grid.voxel * (n - 1) for a, n in enumerate((grid.nx, grid.ny, grid.nz))])


def smooth_images(rng, V, H, W, surface_depth, see_through=0.08):
    """A wavy depth around ``surface_depth`` with pixel noise, and final_T that is see-through (0.9) on a random
    ``see_through`` share of the pixels and 0 .. 0.3 elsewhere: far from alpha_min = 0.5 on either side."""
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.empty((V, H, W), np.float32)
    final_T = np.empty((V, H, W), np.float32)
    for v in range(V):
        depth[v] = surface_depth + 0.1 * np.sin(0.3 * xx + v) * np.cos(0.2 * yy) + 0.02 * rng.standard_normal((H, W))
        final_T[v] = np.where(rng.uniform(size=(H, W)) < see_through, 0.9, 0.3 * rng.uniform(size=(H, W)))
    return depth, final_T


def disc_images(rng, V, H, W, surface_depth, radius):
    """An object that fills the disc of ``radius`` (in units of the shorter image side) round the image centre and
    is see-through outside it: most of the grid is carved by the first few views."""
    yy, xx = np.mgrid[0:H, 0:W]
    rr = np.hypot(xx - (W - 1) / 2, yy - (H - 1) / 2) / min(W, H)
    depth = (surface_depth + 0.02 * rng.standard_normal((V, H, W))).astype(np.float32)
    final_T = np.where(rr[None] < radius, 0.3 * rng.uniform(size=(V, H, W)), 0.9).astype(np.float32)
    return depth, final_T


SYNTHETIC_GRID = (41, 33, 29, (-0.41, -0.3, -0.27), 0.02)       # ragged against the 8x8x4 brick in every axis


def synthetic_tsdf_case(W=37, H=29, n_views=7, grid=SYNTHETIC_GRID, dist=1.6, fov_deg=(50.0, 40.0)):
    """The first device case: 7 views 1.6 away from a 41x33x29 grid that every view holds whole."""
    rng = np.random.default_rng(7)
    grid = Grid(*grid)
    raw = raw_views_around(grid_center(grid), dist, n_views, W, H, math.radians(fov_deg[0]), math.radians(fov_deg[1]))
    depth, final_T = smooth_images(rng, len(raw), H, W, dist - 0.25)
    return TsdfCase(grid, raw, depth, final_T, 3.0 * grid.voxel, 0.5, reaches=("carved", "behind", "fused"))


def _with_blind_view(at):
    c = synthetic_tsdf_case()
    at = at if at >= 0 else len(c.raw) + 1 + at
    rng = np.random.default_rng(70 + at)
    c.raw.insert(at, looking_away(c.raw[min(at, len(c.raw) - 1)]))
    # the blind view's images would fuse and carve if anything were read from them
    d, t = smooth_images(rng, 1, c.depth.shape[1], c.depth.shape[2], 1.6 - 0.25, see_through=0.5)
    c.depth = np.insert(c.depth, at, d[0], axis=0)
    c.final_T = np.insert(c.final_T, at, t[0], axis=0)
    c.reaches = ("near", "carved", "behind", "fused")
    c.blind_views = (at,)
    return c


def _ring_through_grid():
    """Cameras on a sphere of radius 0.3 inside a grid box of 0.8 x 0.64 x 0.56, 20 x 16 degrees wide: part of the grid is
    behind every camera or nearer than NEAR_Z, and most of the rest projects outside the image on every side."""
    rng = np.random.default_rng(8)
    grid = Grid(*SYNTHETIC_GRID)
    W, H = 37, 29
    raw = raw_views_around(grid_center(grid) + np.array([0.013, -0.007, 0.011]), 0.3, 7, W, H, math.radians(20.0),
                           math.radians(16.0))
    depth, final_T = smooth_images(rng, len(raw), H, W, 0.45)
    return TsdfCase(grid, raw, depth, final_T, 3.0 * grid.voxel, 0.5,
                    reaches=("near", "left", "right", "top", "bottom", "carved", "behind", "fused"))


def _many_views(n):
    """n views of 23x17 pixels round a 19x17x13 grid.  The object fills a disc in every image, so a point outside
    the visual hull is carved after a few views and only the hull's points walk all n."""
    rng = np.random.default_rng(100 + n)
    grid = Grid(19, 17, 13, (-0.093, -0.081, -0.062), 0.01)
    W, H = 23, 17
    raw = raw_views_around(grid_center(grid), 0.6, n, W, H, math.radians(40.0), math.radians(30.0))
    assert len(raw) == n
    depth, final_T = disc_images(rng, n, H, W, 0.6 - 0.03, 0.22)
    return TsdfCase(grid, raw, depth, final_T, 3.0 * grid.voxel, 0.5,
                    reaches=("carved", "behind", "fused"))


def _thin_image(W, H):
    """One pixel column, one row or one pixel, 10 x 8 degrees wide: the grid spills over every side of it."""
    c = synthetic_tsdf_case(W=W, H=H, fov_deg=(10.0, 8.0))
    c.reaches = ("left", "right", "top", "bottom", "fused")
    return c


def _carve_order(reverse):
    """Six views that only fuse, then one that carves a third of what it sees; ``reverse`` walks them backwards."""
    c = synthetic_tsdf_case()
    rng = np.random.default_rng(9)
    c.final_T[:-1] = (0.3 * rng.uniform(size=c.final_T[:-1].shape)).astype(np.float32)
    c.final_T[-1] = np.where(rng.uniform(size=c.final_T[-1].shape) < 0.33, 0.95, 0.1).astype(np.float32)
    if reverse:
        c.raw, c.depth, c.final_T = c.raw[::-1], c.depth[::-1].copy(), c.final_T[::-1].copy()
    c.reaches = ("carved", "behind", "fused")
    return c


def _small_grid(nx, ny, nz):
    """A grid of a few points in the middle of the synthetic case's views."""
    vox = 0.02
    origin = tuple(0.003 * (a + 1) - 0.5 * vox * (n - 1) for a, n in enumerate((nx, ny, nz)))
    big = Grid(*SYNTHETIC_GRID)
    origin = tuple(float(o + c) for o, c in zip(origin, grid_center(big)))
    c = synthetic_tsdf_case()
    c.grid = Grid(nx, ny, nz, origin, vox)
    c.reaches = ("fused",) if min(nx, ny, nz) > 3 else ()
    return c


def _odd_depth(kind):
    """The synthetic case with one depth value replaced wherever a pattern of pixels says so: +inf, NaN, or 0 at the
    see-through pixels (whose depth the rules never read)."""
    c = synthetic_tsdf_case()
    yy, xx = np.mgrid[0:c.depth.shape[1], 0:c.depth.shape[2]]
    pattern = ((xx + 2 * yy) % 5 == 0)[None] & np.ones((len(c.raw), 1, 1), bool)
    if kind == "zero_where_transparent":
        c.final_T = np.where(c.final_T > 0.5, np.float32(1.0), c.final_T)
        c.depth = np.where(c.final_T == 1.0, np.float32(0.0), c.depth)
    else:
        c.depth = np.where(pattern & (c.final_T < 0.5), np.float32(np.inf if kind == "inf" else np.nan), c.depth)
    return c


TSDF_CASES = {
    "synthetic-41x33x29-7views": synthetic_tsdf_case,
    "ring-through-grid-fov20": _ring_through_grid,
    "blind-view-first": lambda: _with_blind_view(0),
    "blind-view-middle": lambda: _with_blind_view(3),
    "blind-view-last": lambda: _with_blind_view(-1),
    "views-1": lambda: _many_views(1),
    "views-2": lambda: _many_views(2),
    "views-255": lambda: _many_views(255),
    "views-256": lambda: _many_views(256),
    "image-1xH": lambda: _thin_image(1, 29),
    "image-Wx1": lambda: _thin_image(37, 1),
    "image-1x1": lambda: _thin_image(1, 1),
    "carve-after-fusing": lambda: _carve_order(False),
    "carve-before-fusing": lambda: _carve_order(True),
    "grid-16x16x8-brick-aligned": lambda: _small_grid(16, 16, 8),
    "grid-3x3x3": lambda: _small_grid(3, 3, 3),
    "grid-2x2x2-no-interior": lambda: _small_grid(2, 2, 2),
    "depth-inf": lambda: _odd_depth("inf"),
    "depth-zero-where-transparent": lambda: _odd_depth("zero_where_transparent"),
    "depth-nan": lambda: _odd_depth("nan"),
}


def check_against_oracle(case, got=None):
    """The float64 oracle against the float32 transcription (or a device result): equal outside the oracle's mask to
    its tolerance, masked share at most 1 % of the interior points; the census reaches what the case names."""
    want32 = R.tsdf_reference(*case.reference_args()) if got is None else got
    sdf, masked, tol, census = R.tsdf_oracle(*case.reference_args())
    inside = R.interior(case.grid)
    share = masked.sum() / max(int(inside.sum()), 1)
    print(f"masked {masked.sum()} of {inside.sum()} interior points ({share:.5f}), largest tolerance {tol.max():.3g}")
    assert share <= 0.01, share
    assert not masked[~inside].any()
    diff = np.abs(want32.astype(np.float64) - sdf)
    bad = ~masked & ~(diff <= tol)
    assert not bad.any(), (int(bad.sum()), float(diff[bad].max()))
    for key in case.reaches:
        assert census[key] > 0, (key, census)
    for v in case.blind_views:
        assert census["in_image_per_view"][v] == 0
    return census


# ---- marching fields ------------------------------------------------------------------------------------------------
def unit_grid(nx, ny, nz):
    return Grid(nx, ny, nz, (-0.37, 0.11, 0.05), 0.0125)


def n_tiles(grid, tile=1024):
    return (grid.nx * grid.ny * grid.nz + tile - 1) // tile


def gyroid(grid, periods=1.7, level=0.15):
    """sin x cos y + sin y cos z + sin z cos x - level with ``periods`` periods along the longest axis, at least a
    third of a period on a short one: a surface in every part of the grid, through its border too."""
    n = max(grid.nx, grid.ny, grid.nz)
    ax = []
    for a, m in enumerate((grid.nx, grid.ny, grid.nz)):
        step = 2.0 * math.pi * periods / n if m > 4 else 2.0 * math.pi / 3.1
        ax.append(step * np.arange(m) + 0.4 + 0.9 * a)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return (np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x) - level).astype(np.float32)


def off_centre_sphere(n=32, r=0.8, center=(0.6, 0.0, 0.0), half=1.0):
    """A sphere that leaves the grid through the +x face (the host test's field, without the forced outer layer)."""
    g = Grid(n, n, n, (-half, -half, -half), 2.0 * half / (n - 1))
    ax = [np.float32(-half) + np.float32(g.voxel) * np.arange(n, dtype=np.float32) - np.float32(c) for c in center]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - np.float32(r)).astype(np.float32), g


def force_outer_layer(sdf):
    sdf = sdf.copy()
    sdf[:, :, 0] = sdf[:, :, -1] = sdf[:, 0, :] = sdf[:, -1, :] = sdf[0] = sdf[-1] = 1.0
    return sdf


RAGGED = (37, 35, 33)            # 42735 points: 41 full tiles and one of 751


def _hostile_magnitudes(rng, shape):
    """Magnitudes in [0.1, 1] with a share of denormals, of the smallest normal, and of values a few ulp apart from a
    neighbour's (so that fa - fb is tiny against fa)."""
    mag = rng.uniform(0.1, 1.0, size=shape).astype(np.float32)
    pick = rng.uniform(size=shape)
    mag = np.where(pick < 0.03, np.float32(1e-41), mag)                          # denormal
    mag = np.where((pick >= 0.03) & (pick < 0.05), np.float32(1.17549435e-38), mag)
    mag = np.where((pick >= 0.05) & (pick < 0.08), np.float32(0.25) * (1 + np.float32(2.0 ** -22)), mag)
    mag = np.where((pick >= 0.08) & (pick < 0.11), np.float32(0.25), mag)
    return mag.astype(np.float32)


def checkerboard(shape=RAGGED, seed=21):
    """Inside where i+j+k is odd: every axis edge is crossed and every cell holds 12 triangles."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    mag = rng.uniform(0.1, 1.0, size=(nz, ny, nx)).astype(np.float32)
    return np.where((i + j + k) % 2 == 1, -mag, mag).astype(np.float32), unit_grid(*shape)


def random_signs(shape=RAGGED, seed=22):
    """Independent fair signs on hostile magnitudes; the points that hold +0.0 and -0.0 are outside (sdf < 0 is false)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    mag = _hostile_magnitudes(rng, (nz, ny, nx))
    sdf = np.where(rng.uniform(size=mag.shape) < 0.5, -mag, mag).astype(np.float32)
    pick = rng.uniform(size=mag.shape)
    sdf = np.where(pick < 0.02, np.float32(0.0), sdf)
    sdf = np.where((pick >= 0.02) & (pick < 0.04), np.float32(-0.0), sdf)
    return sdf.astype(np.float32), unit_grid(*shape)


def inside_on_border(shape=(21, 19, 17), seed=23):
    """A random-sign field with no forced layer: inside values on every face, edge and corner of the grid."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    mag = rng.uniform(0.1, 1.0, size=(nz, ny, nx)).astype(np.float32)
    return np.where(rng.uniform(size=mag.shape) < 0.5, -mag, mag).astype(np.float32), unit_grid(*shape)


def boundary_planes_hold_open_edges(vertices, faces, grid, tol_voxels=1e-4):
    """Every directed edge without its reverse has both vertices on a boundary plane of the grid."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    nv = len(vertices)
    key, rev = e[:, 0] * nv + e[:, 1], e[:, 1] * nv + e[:, 0]
    open_edges = e[~np.isin(key, rev)]
    lo = np.array([np.float32(o) for o in grid.origin], np.float64)
    hi = np.array([float(np.float32(o) + np.float32(grid.voxel) * np.float32(n - 1))
                   for o, n in zip(grid.origin, (grid.nx, grid.ny, grid.nz))])
    v = vertices.astype(np.float64)
    on_plane = (np.abs(v - lo) <= tol_voxels * grid.voxel) | (np.abs(v - hi) <= tol_voxels * grid.voxel)     # [V,3]
    both = on_plane[open_edges[:, 0]] & on_plane[open_edges[:, 1]]                # the same plane holds both ends
    return len(open_edges), bool(both.any(axis=1).all())
