"""Grids, carved volumes and worlds of the environment tests: procedural, no fixture files.  The field kernel's cases are the
smallest shapes at which it can go wrong (line lengths 2, 3, 63/64/65 and beyond one workgroup's lanes on each axis in turn);
the worlds are the unit bodies of tests/dynamics_cases.py over a 24 x 24 x 16 ground that holds "a table on a floor".  Every
reference value (tests/environment_reference.py) is computed once per process and shared, unchanged."""
import functools

import numpy as np

import collision_reference as CR
import dynamics_cases as DC
import dynamics_reference as DR
import environment_reference as ER

TRUNCATION_VOXELS = 3.0
FIELD_GRIDS = ((5, 4, 3), (17, 9, 6), (65, 3, 2), (2, 257, 3), (3, 2, 130), (24, 24, 24))           # (nx, ny, nz)
ANALYTIC = ("sphere", "plane", "table")
CONTENTS = ANALYTIC + ("random", "all_inside", "all_outside", "corner", "nan_and_zero")
VOXEL = 0.05
ORIGIN = (-0.31, 0.17, -0.06)


def field_grid(shape):
    nx, ny, nz = shape
    return CR.RefGrid(nx, ny, nz, ORIGIN, VOXEL)


def _extent(g):
    return g.voxel * (g.n - 1.0)


# ---- exact distances --------------------------------------------------------------------------------------------------------
def sphere_of(g):
    """(centre off the grid's points, radius): a ball that fills about a third of the grid's shortest side and at least 1.6 voxels."""
    e = _extent(g)
    return g.origin + e * np.array([0.47, 0.53, 0.51]) + g.voxel * np.array([0.31, -0.23, 0.17]), max(0.33 * e.min(), 1.6 * g.voxel)


def plane_of(g):
    """(unit normal, offset) of a tilted plane through the grid's middle."""
    n = np.array([0.28, -0.19, 0.94])
    n /= np.linalg.norm(n)
    return n, float(n @ (g.origin + 0.5 * _extent(g))) + 0.13 * g.voxel


def table_of(g):
    """(floor height, box lo [3], box hi [3]): a box standing on the half space z <= floor."""
    e = _extent(g)
    floor = g.origin[2] + 0.27 * e[2]
    lo = np.array([g.origin[0] + 0.29 * e[0], g.origin[1] + 0.31 * e[1], floor])
    hi = np.array([g.origin[0] + 0.71 * e[0], g.origin[1] + 0.68 * e[1], g.origin[2] + 0.63 * e[2]])
    return float(floor), lo, hi


def _rect(a, b, c, d):
    return [np.array([a, b, c]), np.array([a, c, d])]


def table_surface(floor, lo, hi, far=1.0e3):
    """Triangles [T,3,3] of the table's surface: the box's top and sides and the floor around its footprint out to ``far``."""
    x0, y0, _ = lo
    x1, y1, z1 = hi
    P = lambda x, y, z: np.array([x, y, z], np.float64)
    tris = _rect(P(x0, y0, z1), P(x1, y0, z1), P(x1, y1, z1), P(x0, y1, z1))
    for (ax, ay), (bx, by) in (((x0, y0), (x1, y0)), ((x1, y0), (x1, y1)), ((x1, y1), (x0, y1)), ((x0, y1), (x0, y0))):
        tris += _rect(P(ax, ay, floor), P(bx, by, floor), P(bx, by, z1), P(ax, ay, z1))
    for (ax, ay), (bx, by) in (((-far, -far), (far, y0)), ((-far, y1), (far, far)), ((-far, y0), (x0, y1)), ((x1, y0), (far, y1))):
        tris += _rect(P(ax, ay, floor), P(bx, ay, floor), P(bx, by, floor), P(ax, by, floor))
    return np.stack(tris)


def table_distance(points, floor, lo, hi):
    """The exact signed distance of points [N,3] to the table: negative in the half space or the box."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    d = np.full(len(p), np.inf)
    for a, b, c in table_surface(floor, lo, hi):
        d = np.minimum(d, CR.point_triangle_distance(p, a, b, c))
    solid = (p[:, 2] <= floor) | ((p >= lo) & (p <= hi)).all(1)
    return np.where(solid, -d, d)


def exact_distance(name, g, points=None):
    """[nz,ny,nx] (or [N]): the exact signed distance of the grid's points (or ``points``) to the analytic shape."""
    p = CR.grid_points(g).reshape(-1, 3) if points is None else np.asarray(points, np.float64).reshape(-1, 3)
    if name == "sphere":
        c, r = sphere_of(g)
        d = np.linalg.norm(p - c, axis=1) - r
    elif name == "plane":
        n, off = plane_of(g)
        d = p @ n - off
    elif name == "table":
        d = table_distance(p, *table_of(g))
    else:
        raise KeyError(name)
    return d.reshape(g.shape) if points is None else d


# ---- carved volumes ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def volume(content, shape):
    """float32 [nz,ny,nx], read-only: the carved volume of a case."""
    g = field_grid(shape)
    rng = np.random.default_rng([CONTENTS.index(content), *shape])
    if content in ANALYTIC:
        t = np.clip(exact_distance(content, g) / (TRUNCATION_VOXELS * g.voxel), -1.0, 1.0)
    elif content == "random":
        t = rng.uniform(-1.0, 1.0, g.shape)
    elif content == "all_inside":
        t = np.full(g.shape, -1.0)
    elif content == "all_outside":
        t = np.full(g.shape, 1.0)
    elif content == "corner":
        t = np.full(g.shape, 1.0)
        t[0, 0, 0] = -0.25
    elif content == "nan_and_zero":
        t = rng.uniform(-1.0, 1.0, g.shape)
        flat = t.reshape(-1)
        flat[len(flat) // 3] = np.nan
        flat[(2 * len(flat)) // 3] = 0.0
    else:
        raise KeyError(content)
    t = t.astype(np.float32)
    t.setflags(write=False)
    return t


def field_cases():
    """(content, shape) of every field case: everything on the small grids; on 24^3 the analytic volumes and the random one."""
    return [(c, s) for s in FIELD_GRIDS for c in CONTENTS if s != (24, 24, 24) or c in ANALYTIC + ("random",)]


@functools.lru_cache(maxsize=None)
def reference_field(content, shape):
    """(dist2 int64, phi32 float32, phi64) of a case, read-only."""
    t = volume(content, shape)
    d2 = ER.dist2(t)
    out = (d2, ER.phi32(t, VOXEL, d2), ER.phi64(t, VOXEL, d2))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the ground of the worlds -----------------------------------------------------------------------------------------------
GROUND_SHAPE = (24, 24, 16)
GROUND_VOXEL = 0.125
GROUND_ORIGIN = (-1.4375, -1.4375, -0.4375)          # 23 voxels: x, y in [-1.4375, 1.4375]; z up to 1.4375
FLOOR, TABLE_LO, TABLE_HI = 0.0, np.array([-1.1, -0.7, 0.0]), np.array([0.1, 0.7, 0.55])
TABLE_HEIGHT = 0.55
BODY = "small_cube"                                  # side 0.6: the grid leaves room for it beside the table
GROUND_FRICTION = 0.5


def ground_grid():
    return CR.RefGrid(*GROUND_SHAPE, GROUND_ORIGIN, GROUND_VOXEL)


def ground_distance(points):
    """The exact signed distance to the analytic table of the worlds."""
    return table_distance(points, FLOOR, TABLE_LO, TABLE_HI)


@functools.lru_cache(maxsize=None)
def ground_volume(kind="table"):
    """float32 [16,24,24]: clip(d / truncation) of the table (or of the flat floor z = 0 alone), the outermost layer of points
    outside as pgr_tsdf_integrate leaves it, so the solid closes inside the grid."""
    g = ground_grid()
    p = CR.grid_points(g).reshape(-1, 3)
    d = ground_distance(p) if kind == "table" else p[:, 2] - FLOOR
    t = np.clip(d.reshape(g.shape) / (TRUNCATION_VOXELS * g.voxel), -1.0, 1.0).astype(np.float32)
    for ax in range(3):
        idx = [slice(None)] * 3
        for edge in (0, -1):
            idx[ax] = edge
            t[tuple(idx)] = 1.0
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def ground_reference(kind="table"):
    """ER.RefGround on the reference's own float64 field of the ground's volume."""
    return ER.RefGround(ER.phi64(ground_volume(kind), GROUND_VOXEL), ground_grid(), GROUND_FRICTION)


def z_field():
    """float32 [16,24,24]: the field z sampled on the ground's grid; the trilinear rule reproduces it exactly."""
    return CR.grid_points(ground_grid())[..., 2].astype(np.float32)


def ground_params(types, **kw):
    """dynamics_cases.params with the ground's friction in the plane's place and a margin that covers the ground's voxel."""
    kw.setdefault("plane_friction", GROUND_FRICTION)
    return DC.params(types, **kw)


ON_TABLE = np.array([-0.5, 0.02, 1.3])               # the tilted cube's start over the table top
BESIDE_TABLE = np.array([0.78, 0.05, 1.3])           # .. and beside it, over the floor (inside the grid box)


def cube_start(at, world=0):
    """[1,7]: the cube in dynamics_cases' start orientation of the tilted cube of ``world``, at ``at``."""
    pose = DC.start_poses("cube_tilted", world)
    pose[0, :3] = at
    return pose


def touching(xy, surface, world, depth):
    """[1,7]: that cube over (x, y) with its lowest shell point ``depth`` below the height ``surface``."""
    pose = cube_start((xy[0], xy[1], 0.0), world)
    low = float((DC.shell(BODY).astype(np.float64) @ DR.rotation(pose[0, 3:] / np.linalg.norm(pose[0, 3:])).T)[:, 2].min())
    pose[0, 2] = surface - low - depth
    return pose


# the tilted cube against the table: in the air, on the table top, over the table's edge, on the floor, at the side wall
CONTACT_SPOTS = (((-0.5, 0.02), TABLE_HEIGHT, 0, -0.6), ((-0.5, 0.02), TABLE_HEIGHT, 0, 0.02), ((-0.45, -0.1), TABLE_HEIGHT, 1, 0.05),
                 ((-0.02, 0.3), TABLE_HEIGHT, 2, 0.03), ((0.78, 0.05), FLOOR, 3, 0.02), ((0.7, -0.6), FLOOR, 4, 0.06),
                 ((0.42, 0.1), FLOOR, 5, 0.01), ((-0.6, 0.25), TABLE_HEIGHT, 6, 0.0), ((-0.3, -0.3), TABLE_HEIGHT, 7, 0.08),
                 ((0.9, 0.4), FLOOR, 1, 0.04))


@functools.lru_cache(maxsize=None)
def contact_states():
    """[S,1,13] float64 of float32 numbers, read-only."""
    types = [DC.ref_type(BODY)]
    out = DR.f32(np.stack([DC.state_of(types, touching(xy, surface, w, depth)) for xy, surface, w, depth in CONTACT_SPOTS]))
    out.setflags(write=False)
    return out
