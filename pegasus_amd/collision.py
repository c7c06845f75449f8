"""Collision geometry on the HIP library: signed distance fields of triangle meshes (``pgr_mesh_sdf``), their samples
(``pgr_sdf_sample``), distance and sweep queries between posed bodies (``pgr_sdf_sweep``), and a placement routine that lowers
objects, one after the other, onto a ground plane and onto each other until they touch.

The reference gets its object poses from pybullet (src/engine/physical_simulation.py) and stores them in
``simulation_steps.json``; ``PegasusSetup.static_object_pose`` reads the last step of that file, so a one-step file is a valid
static scene.  ``drop`` produces such poses from geometry alone; ``write_simulation_steps`` writes them in that layout.  Nothing
here integrates velocities or contact forces: a body placed on the ground in one of its ``resting_orientations`` keeps its pose,
a body lowered onto another body is in contact but not necessarily stable -- letting it roll off is a simulator's job.

The rules stand at the top of pegasus_amd/csrc/meshsdf.hip.h and in DESIGN.md section 22.  The field is brute force, grid points
x faces: it is meant for the collision meshes the project writes (``mesh --collision_faces``, ``models_eval``: a few 10^4 faces),
not for the 10^6-face originals.

    python -m pegasus_amd.collision --models <dir> --objects 1 2 5 [--count k] [--seed s] [--radius r] --out <simulation_steps.json>
    python -m pegasus_amd.collision --check <dataset dir> --models <dir>
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import re
import warnings
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib, bop_dataset as BD
from .mesh import Grid, Mesh

WARN_FACES = 50_000              # above: pgr_mesh_sdf is brute force, a 96^3 field of such a mesh takes seconds
MAX_FACES = 400_000              # above: refused; decimate first (pegasus_amd.decimate, mesh --collision_faces)


def _cuda(device, what: str):
    import torch
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"{what} needs a HIP device (torch device 'cuda'); there is no CPU path")
    return device


def _device_points(points, what: str):
    import torch
    if not isinstance(points, torch.Tensor) or points.device.type != "cuda":
        raise RuntimeError(f"{what} needs a tensor on a HIP device; there is no CPU path")
    if points.shape[-1] != 3:
        raise ValueError("points must be [...,3]")
    return points.to(torch.float32).reshape(-1, 3).contiguous()


# ---- fields -----------------------------------------------------------------------------------------------------------
def mesh_sdf(vertices, faces, grid: Grid, winding: bool = False):
    """``pgr_mesh_sdf`` on device tensors (float32 [V,3], int32 [F,3]): the float32 field [nz,ny,nx] on the same device, and the
    winding number with ``winding``.  Enqueued on the current stream."""
    import torch
    if not all(isinstance(a, torch.Tensor) and a.device.type == "cuda" for a in (vertices, faces)):
        raise RuntimeError("mesh_sdf needs tensors on a HIP device; there is no CPU path")
    device = vertices.device
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    faces = faces.to(torch.int32).reshape(-1, 3).contiguous()
    sdf = torch.empty(grid.shape, dtype=torch.float32, device=device)
    wn = torch.empty(grid.shape, dtype=torch.float32, device=device) if winding else None
    g = grid.struct()
    _lib.call("pgr_mesh_sdf", device, len(vertices), _lib.ptr(vertices) if len(vertices) else None, len(faces),
              _lib.ptr(faces) if len(faces) else None, C.byref(g), _lib.ptr(sdf), _lib.ptr(wn))
    return (sdf, wn) if winding else sdf


def sdf_sample(field, grid: Grid, points, gradient: bool = False):
    """``pgr_sdf_sample``: the field's value at device ``points`` [...,3] (float32 [...]), and its gradient [...,3] with
    ``gradient``."""
    import torch
    if not isinstance(field, torch.Tensor) or field.device.type != "cuda":
        raise RuntimeError("sdf_sample needs a field on a HIP device; there is no CPU path")
    shape = tuple(points.shape[:-1]) if hasattr(points, "shape") else ()
    pts = _device_points(points, "sdf_sample")
    if tuple(field.shape) != grid.shape:
        raise ValueError(f"the field is {tuple(field.shape)}, the grid {grid.shape}")
    field = field.to(torch.float32).contiguous()
    values = torch.empty((len(pts),), dtype=torch.float32, device=field.device)
    grads = torch.empty((len(pts), 3), dtype=torch.float32, device=field.device) if gradient else None
    g = grid.struct()
    _lib.call("pgr_sdf_sample", field.device, C.byref(g), _lib.ptr(field), len(pts), _lib.ptr(pts) if len(pts) else None,
              _lib.ptr(values) if len(pts) else None, _lib.ptr(grads) if gradient and len(pts) else None)
    values = values.reshape(shape)
    return (values, grads.reshape(shape + (3,))) if gradient else values


@dataclass
class MeshSDF:
    """The signed distance field of a mesh over a grid that encloses it: ``field`` float32 [nz,ny,nx] on the device, positive
    outside."""
    grid: Grid
    field: object

    @staticmethod
    def from_mesh(mesh, resolution: int = 96, padding: Optional[float] = None, device="cuda") -> "MeshSDF":
        """The field of ``mesh`` (a ``mesh.Mesh`` or a (vertices, faces) pair) on ``Grid.around`` its bounding box grown by
        ``padding`` on every side (default: two voxels), ``resolution`` points along the longest axis."""
        import torch
        device = _cuda(device, "MeshSDF.from_mesh")
        v, f = (mesh.vertices, mesh.faces) if hasattr(mesh, "vertices") else mesh
        v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
        if len(v) == 0:
            raise ValueError("a mesh without vertices has no bounding box to build a grid around")
        if len(f) > MAX_FACES:
            raise ValueError(f"{len(f)} faces: the distance field is brute force (grid points x faces) and meant for collision "
                             f"meshes of a few 10^4 faces; decimate first (pegasus_amd.decimate, mesh --collision_faces)")
        if len(f) > WARN_FACES:
            warnings.warn(f"{len(f)} faces: the distance field is brute force (grid points x faces); a collision mesh of a few "
                          "10^4 faces (mesh --collision_faces) is what it is meant for")
        lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
        if padding is None:
            if resolution < 6:
                raise ValueError("resolution must be at least 6 with the default padding of two voxels")
            padding = 2.0 * float((hi - lo).max()) / (resolution - 5)        # voxel = (extent + 2 padding) / (resolution - 1)
        if not (hi - lo).max() + 2 * padding > 0:
            raise ValueError("the mesh has no extent: give a padding")
        grid = Grid.around(lo - padding, hi + padding, resolution)
        field = mesh_sdf(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), grid)
        return MeshSDF(grid, field)

    def signed_distance(self, points, gradient: bool = False):
        """The trilinear field value at device ``points`` [...,3].  Outside the grid: the distance to the grid's box and
        max(field, 0) at the clamped point added in quadrature, a lower bound of the distance to the surface."""
        return sdf_sample(self.field, self.grid, points, gradient)


@dataclass
class CollisionBody:
    """A mesh, its field and its shell: the points of the body that are tested against other bodies' fields (default: the
    mesh's vertices).  ``shell`` becomes a float32 [n,3] tensor on the field's device."""
    mesh: Mesh
    sdf: MeshSDF
    shell: object = None

    def __post_init__(self):
        import torch
        device = self.sdf.field.device
        if self.shell is None:
            self.shell = self.mesh.vertices
        if isinstance(self.shell, torch.Tensor):
            if self.shell.device.type != "cuda":
                raise RuntimeError("CollisionBody needs its shell on a HIP device; there is no CPU path")
            self.shell = self.shell.to(torch.float32).reshape(-1, 3).contiguous()
        else:
            self.shell = torch.from_numpy(np.ascontiguousarray(self.shell, np.float32).reshape(-1, 3)).to(device)

    @staticmethod
    def from_mesh(mesh: Mesh, resolution: int = 96, padding: Optional[float] = None, device="cuda") -> "CollisionBody":
        return CollisionBody(mesh, MeshSDF.from_mesh(mesh, resolution, padding, device))

    @property
    def voxel(self) -> float:
        return float(self.sdf.grid.voxel)


def read_obj(path) -> Mesh:
    """The ``v`` and triangular ``f`` records of a Wavefront file, as ``mesh.write_obj`` writes them."""
    v, f = [], []
    for line in Path(path).read_text().splitlines():
        p = line.split()
        if not p:
            continue
        if p[0] == "v":
            v.append([float(x) for x in p[1:4]])
        elif p[0] == "f":
            if len(p) != 4:
                raise ValueError(f"{path}: only triangles are read")
            f.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    return Mesh(np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3))


def mesh_files(models_dir) -> dict:
    """{obj_id: path}: the obj_NNNNNN.ply of a ``models/`` or ``models_eval/`` directory, or, where there is none, the
    obj_NNNNNN_collision.obj that ``mesh --collision_faces`` writes into ``urdf/`` (``models_dir`` or its ``urdf`` child)."""
    d = Path(models_dir)
    try:
        return BD.model_files(d)
    except FileNotFoundError:
        pass
    for sub in (d, d / "urdf"):
        files = {int(m.group(1)): p for p in sorted(sub.glob("*_collision.obj")) if (m := re.fullmatch(r"obj_(\d+)_collision", p.stem))}
        if files:
            return files
    raise FileNotFoundError(f"no obj_NNNNNN.ply and no obj_NNNNNN_collision.obj under {models_dir}")


def bodies_from_dir(models_dir, scale: float = 1.0, objects: Optional[Sequence[int]] = None, resolution: int = 96,
                    device="cuda") -> dict:
    """{obj_id: CollisionBody} of a directory (``mesh_files``), vertices multiplied by ``scale`` (0.001: BOP millimetres ->
    metres)."""
    from .ply_io import read_ply_model
    files = mesh_files(models_dir)
    out = {}
    for i in (sorted(files) if objects is None else objects):
        if int(i) not in files:
            raise KeyError(f"object {i} has no mesh under {models_dir}")
        path = files[int(i)]
        if path.suffix == ".obj":
            mesh = read_obj(path)
        else:
            model = read_ply_model(path)
            mesh = Mesh(np.asarray(model["pts"], np.float32), np.asarray(model["faces"], np.int32).reshape(-1, 3))
        out[int(i)] = CollisionBody.from_mesh(mesh.scaled(scale) if scale != 1.0 else mesh, resolution, device=device)
    return out


# ---- queries ----------------------------------------------------------------------------------------------------------
PLANE = _lib.PGR_SWEEP_PLANE


def _body_table(bodies: Sequence[CollisionBody], poses):
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    if len(poses) != len(bodies):
        raise ValueError("one 4x4 pose per body")
    table = (_lib.PgrSdfBody * max(1, len(bodies)))()
    for k, (b, T) in enumerate(zip(bodies, poses)):
        table[k] = _lib.PgrSdfBody(grid=b.sdf.grid.struct(), sdf=b.sdf.field.data_ptr(), shell=b.shell.data_ptr() if len(b.shell) else None,
                                   n_shell=len(b.shell), R=(C.c_float * 9)(*T[:3, :3].reshape(-1)), t=(C.c_float * 3)(*T[:3, 3]))
    return table


def _job_table(jobs, plane):
    n = np.zeros(4) if plane is None else np.asarray(plane, np.float64).reshape(4)
    table = (_lib.PgrSweepJob * max(1, len(jobs)))()
    for k, (a, b, d) in enumerate(jobs):
        if b == PLANE and plane is None:
            raise ValueError("a job against the plane needs a plane")
        table[k] = _lib.PgrSweepJob(mover=int(a), target=int(b), dir=(C.c_float * 3)(*d), plane=(C.c_float * 4)(*n))
    return table


def unit_plane(plane):
    """(n, d) of the plane n.x = d with n of unit length, float64."""
    p = np.asarray(plane, np.float64).reshape(4)
    norm = float(np.linalg.norm(p[:3]))
    if not norm > 0 or not np.isfinite(p).all():
        raise ValueError("the plane needs a finite normal that is not zero")
    return p / norm


def sweep_words(bodies: Sequence[CollisionBody], poses, jobs, plane=None, tol: float = 1e-4, max_travel: float = 0.0,
                max_steps: int = 0):
    """One ``pgr_sdf_sweep`` call.  ``jobs``: (mover, target or PLANE, direction) triples.  Returns the int64 [n_jobs,2] device
    tensor that holds the entry's unsigned words (``decode_words`` reads them on the host)."""
    import torch
    if not bodies:
        raise ValueError("no bodies")
    device = bodies[0].sdf.field.device
    out = torch.empty((len(jobs), 2), dtype=torch.int64, device=device)
    _lib.call("pgr_sdf_sweep", device, len(bodies), _body_table(bodies, poses), len(jobs), _job_table(jobs, plane), float(tol),
              float(max_travel), int(max_steps), _lib.ptr(out) if len(jobs) else None)
    return out


def decode_words(words):
    """(value float32 [...], index int64 [...]) of words  order_bits(value) << 32 | index  (a host int64 / uint64 array); a word
    with all bits set, a job without shell points, reads as (+inf, -1)."""
    w = np.ascontiguousarray(words).view(np.uint64)
    bits = (w >> np.uint64(32)).astype(np.uint32)
    raw = np.where(bits & np.uint32(0x80000000), bits ^ np.uint32(0x80000000), ~bits)
    value = raw.astype(np.uint32).view(np.float32).copy()
    index = (w & np.uint64(0xFFFFFFFF)).astype(np.int64)
    empty = w == np.uint64(0xFFFFFFFFFFFFFFFF)
    value[empty] = np.inf
    index[empty] = -1
    return value, index


def _with_environment(bodies, poses, environment, environment_pose=None):
    """(bodies, poses) with the environment (an ``environment.EnvironmentField``) as one more body without shell points, at the
    identity pose unless one is given; unchanged without an environment."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    if environment is None:
        return list(bodies), poses
    T = np.eye(4) if environment_pose is None else np.asarray(environment_pose, np.float64).reshape(4, 4)
    return list(bodies) + [environment.as_collision_body()], np.concatenate([poses, T[None]])


def min_distances(bodies: Sequence[CollisionBody], poses, plane=None, environment=None, environment_pose=None) -> np.ndarray:
    """float32 [B, B+1]: entry [a, b] is the smallest value of body b's field over body a's shell points at these poses (the
    deepest interpenetration where negative), column B the same against the plane n.x = d (+inf without one); the diagonal is
    +inf.  One ``pgr_sdf_sweep`` call with max_steps = 0.  With an ``environment`` (an ``environment.EnvironmentField``, at the
    identity pose unless ``environment_pose`` gives one) the result is [B, B+2] and column B+1 holds the same against its field."""
    B = len(bodies)
    out = np.full((B, B + (1 if environment is None else 2)), np.inf, np.float32)
    if B == 0:
        return out
    down = (0.0, 0.0, -1.0)
    jobs = [(a, b, down) for a in range(B) for b in range(B) if a != b]
    if environment is not None:
        bodies, poses = _with_environment(bodies, poses, environment, environment_pose)
        jobs += [(a, B, down) for a in range(B)]
    if plane is not None:
        plane = unit_plane(plane)
        jobs += [(a, PLANE, down) for a in range(B)]
    if not jobs:
        return out
    value, _ = decode_words(sweep_words(bodies, poses, jobs, plane, 0.0, 0.0, 0).cpu().numpy())
    for (a, b, _d), phi in zip(jobs, value[:, 0]):
        out[a, B if b == PLANE else (B + 1 if b == B else b)] = phi
    return out


def _sweep_jobs(mover: int, others, direction, with_plane: bool):
    d = tuple(float(x) for x in direction)
    back = tuple(-x for x in d)
    jobs = []
    for b in others:
        jobs += [(mover, b, d), (b, mover, back)]
    if with_plane:
        jobs.append((mover, PLANE, d))
    return jobs


def _unsigned_min(words):
    """The minimum over the jobs of each word, as unsigned numbers: device int64 [2] (flipping the top bit makes the signed order
    the unsigned one)."""
    top = -(1 << 63)
    return (words ^ top).amin(dim=0) ^ top


def sweep(bodies: Sequence[CollisionBody], poses, mover: int, direction, others: Optional[Sequence[int]] = None, plane=None,
          tol: float = 1e-4, max_travel: float = 10.0, max_steps: int = 128, environment=None) -> dict:
    """How far body ``mover`` can travel along ``direction`` before one of its shell points comes within ``tol`` of another
    body's field or of the plane (forward jobs), or another body's shell point within ``tol`` of its own field (reverse jobs: the
    other's shell moved by -direction).  Returns {"travel", "phi0": the deepest field value at the start, "jobs", "travels",
    "phi0s", "points"}: per job the minimum and the shell point that gives it.  The travel is conservative: every step of the
    sphere tracing was at most the sampled free distance.  ``environment``: an ``environment.EnvironmentField`` whose field the
    mover is also traced against (a forward job whose target is the index len(bodies))."""
    direction = np.asarray(direction, np.float64).reshape(3)
    direction = direction / np.linalg.norm(direction)
    others = [b for b in range(len(bodies)) if b != mover] if others is None else [int(b) for b in others]
    if plane is not None:
        plane = unit_plane(plane)
    jobs = _sweep_jobs(int(mover), others, direction, plane is not None)
    if environment is not None:
        jobs.append((int(mover), len(bodies), tuple(float(x) for x in direction)))
        bodies, poses = _with_environment(bodies, poses, environment)
    if not jobs:
        return dict(travel=float(max_travel), phi0=float("inf"), jobs=[], travels=np.zeros(0, np.float32),
                    phi0s=np.zeros(0, np.float32), points=np.zeros((0, 2), np.int64))
    value, index = decode_words(sweep_words(bodies, poses, jobs, plane, tol, max_travel, max_steps).cpu().numpy())
    return dict(travel=float(value[:, 1].min()), phi0=float(value[:, 0].min()), jobs=jobs, travels=value[:, 1], phi0s=value[:, 0],
                points=index)


# ---- placement ----------------------------------------------------------------------------------------------------------
def _hull_faces(points):
    """The planar faces of the convex hull: a list of (outward unit normal, [triangles [T,3,3]]) with coplanar simplices merged."""
    from scipy.spatial import ConvexHull
    p = np.asarray(points, np.float64).reshape(-1, 3)
    hull = ConvexHull(p)
    size = float(np.linalg.norm(p.max(0) - p.min(0)))
    inside = p[hull.vertices].mean(0)
    faces = {}
    for simplex, eq in zip(hull.simplices, hull.equations):
        tri = p[simplex]
        n = eq[:3]
        if np.dot(np.cross(tri[1] - tri[0], tri[2] - tri[0]), n) < 0:
            tri = tri[::-1]
        if np.dot(tri[0] - inside, n) < 0:
            n = -n
        key = tuple(np.round(np.r_[n, eq[3] / size] / 1e-6).astype(np.int64))
        faces.setdefault(key, (n, []))[1].append(tri)
    return [(n, np.stack(tris)) for n, tris in faces.values()]


def _solid_angle(tri, c) -> float:
    a, b, d = tri[0] - c, tri[1] - c, tri[2] - c
    la, lb, ld = np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(d)
    num = np.dot(a, np.cross(b, d))
    den = la * lb * ld + np.dot(a, b) * ld + np.dot(a, d) * lb + np.dot(b, d) * la
    return abs(2.0 * np.arctan2(num, den))


def _in_triangle(tri, q, slack: float) -> bool:
    n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    for k in range(3):
        e = tri[(k + 1) % 3] - tri[k]
        if np.dot(np.cross(e, q - tri[k]), n) < -slack * np.dot(n, n) ** 0.5 * np.linalg.norm(e):
            return False
    return True


def rotation_onto(a, b) -> np.ndarray:
    """The rotation about a x b that takes unit vector a to unit vector b (about a fixed perpendicular axis where a = -b)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    v, c = np.cross(a, b), float(np.dot(a, b))
    if c < -1 + 1e-12:
        axis = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.9 else [0.0, 1.0, 0.0])
        axis /= np.linalg.norm(axis)
        return 2.0 * np.outer(axis, axis) - np.eye(3)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + K + K @ K / (1.0 + c)


def resting_orientations(mesh, up=(0.0, 0.0, 1.0)):
    """(rotations float64 [K,3,3], weights float64 [K], normals float64 [K,3]): one orientation per face of the convex hull over
    which the centre of mass (``Mesh.center_of_mass``) projects inside the face -- the poses an object keeps when it lies on the
    ground on that face.  Rotation k turns the face's outward normal (normals[k], mesh frame) to -up; the weights are the faces'
    solid angles from the centre of mass, normalised to sum 1.  Host code (scipy's hull, as ``obb.py`` uses it).  A body resting
    on another body is in contact but not necessarily stable: that is a simulator's job."""
    up = np.asarray(up, np.float64) / np.linalg.norm(up)
    v = np.asarray(mesh.vertices, np.float64)
    c = np.asarray(mesh.center_of_mass(), np.float64)
    size = float(np.linalg.norm(v.max(0) - v.min(0)))
    rotations, weights, normals = [], [], []
    for n, tris in _hull_faces(v):
        q = c - np.dot(c - tris[0, 0], n) * n                    # the centre of mass projected into the face's plane
        if not any(_in_triangle(t, q, 1e-9 * size) for t in tris):
            continue
        rotations.append(rotation_onto(n, -up))
        weights.append(sum(_solid_angle(t, c) for t in tris))
        normals.append(n)
    if not rotations:
        raise ValueError("no hull face lies under the centre of mass (is the mesh closed and outward wound?)")
    w = np.asarray(weights)
    return np.stack(rotations), w / w.sum(), np.stack(normals)


def _plane_frame(n):
    """(u, v) with u x v = n; (x, y) for n = +z."""
    u = np.cross([0.0, 1.0, 0.0] if abs(n[1]) < 0.9 else [0.0, 0.0, 1.0], n)
    u /= np.linalg.norm(u)
    return u, np.cross(n, u)


def _rotation_about(axis, angle) -> np.ndarray:
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def start_height(vertices, R, placed_tops, n, margin: float) -> float:
    """The height along n of a body's origin at which its lowest point is ``margin`` above everything placed so far."""
    below = float((np.asarray(vertices, np.float64) @ R.T @ n).min())
    return max([0.0] + list(placed_tops)) + margin - below


def environment_start_height(environment, vertices, R, at, margin: float) -> float:
    """The z of a body's origin, over the point ``at``, at which its lowest point is ``margin`` above the environment's highest
    solid grid point under its footprint (the bounding rectangle of its vertices); -inf where nothing solid is under it."""
    w = np.asarray(vertices, np.float64) @ np.asarray(R, np.float64).T
    top = environment.top_under(w[:, :2].min(0) + np.asarray(at, np.float64)[:2], w[:, :2].max(0) + np.asarray(at, np.float64)[:2])
    return top + environment.voxel + margin - float(w[:, 2].min())


def drop(bodies: Sequence[CollisionBody], order: Optional[Sequence[int]] = None, orientations=None, xy=None,
         plane=(0.0, 0.0, 1.0, 0.0), radius: Optional[float] = None, seed: int = 0, tol: float = 1e-4, max_rounds: int = 8,
         max_steps: int = 128, environment=None):
    """Places the bodies one after the other on the plane n.x = d and on each other.  Body k takes an orientation
    (``orientations[k]`` [3,3], or one of its ``resting_orientations`` drawn by weight with a random turn about n, from the
    generator seeded with ``seed``), a position over the plane (``xy[k]`` in the plane's (u, v) frame, or drawn uniformly from the
    disc of ``radius``, default: the largest body's half diagonal) and a height above everything placed so far.  It is then
    lowered along -n by the minimum of all forward and reverse sweep travels against the bodies placed before it and the plane,
    until that minimum is <= ``tol`` or ``max_rounds`` are spent; each round reads back 16 bytes.

    Returns (poses float64 [B,4,4] indexed like ``bodies``, reports: per body {"order", "rounds", "settled", "travel",
    "touches": the bodies ("plane" for the plane) whose field -- or whose shell, in the body's own field -- is within 2 tol at the
    end, "phi0": the smallest field value at the end}).  Orientation and lateral position are never changed by the lowering.

    ``environment``: an ``environment.EnvironmentField`` (the plane must then be z = d) that every body is also traced against;
    a body starts above the environment's highest solid point under its footprint, and "environment" is named in its touches."""
    B = len(bodies)
    order = list(range(B)) if order is None else [int(k) for k in order]
    if sorted(order) != list(range(B)):
        raise ValueError("order must name every body once")
    p = unit_plane(plane)
    n, d = p[:3], float(p[3])
    u, v = _plane_frame(n)
    rng = np.random.default_rng(seed)
    sizes = [float(np.linalg.norm(np.ptp(b.mesh.vertices.astype(np.float64), axis=0))) for b in bodies]
    if radius is None:
        radius = 0.5 * max(sizes, default=0.0)
    margin = 2.0 * max([b.voxel for b in bodies] + ([environment.voxel] if environment is not None else []), default=0.0) + 2.0 * tol
    if environment is not None and not np.allclose(n, (0.0, 0.0, 1.0)):
        raise ValueError("with an environment the plane must be z = d")
    poses = np.tile(np.eye(4), (B, 1, 1))
    reports = [None] * B
    placed, tops = [], []
    for rank, k in enumerate(order):
        body = bodies[k]
        if orientations is not None and orientations[k] is not None:
            R = np.asarray(orientations[k], np.float64).reshape(3, 3)
        else:
            rots, w, _ = resting_orientations(body.mesh, n)
            R = _rotation_about(n, rng.uniform(0.0, 2.0 * np.pi)) @ rots[rng.choice(len(rots), p=w)]
        if xy is not None and xy[k] is not None:
            a, b2 = (float(x) for x in xy[k])
        else:
            r, phi = radius * np.sqrt(rng.uniform()), rng.uniform(0.0, 2.0 * np.pi)
            a, b2 = r * np.cos(phi), r * np.sin(phi)
        h = start_height(body.mesh.vertices, R, tops, n, margin)
        if environment is not None:
            h = max(h, environment_start_height(environment, body.mesh.vertices, R, d * n + a * u + b2 * v, margin) - d)
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = d * n + a * u + b2 * v + h * n
        poses[k] = T
        active = placed + [k]
        sub = [bodies[i] for i in active]
        jobs = _sweep_jobs(len(active) - 1, range(len(placed)), -n, True)
        if environment is not None:
            jobs.append((len(active) - 1, len(active), tuple(float(x) for x in -n)))
            sub = sub + [environment.as_collision_body()]
        max_travel = h + sizes[k] + margin
        rounds, settled, travel = 0, False, float("inf")
        while rounds < max_rounds:
            words = sweep_words(sub, _active_poses(poses, active, environment), jobs, p, tol, max_travel, max_steps)
            travel = float(decode_words(_unsigned_min(words).cpu().numpy())[0][1])          # 16 bytes
            rounds += 1
            if travel <= tol:
                settled = True
                break
            poses[k, :3, 3] -= travel * n
        value, _ = decode_words(sweep_words(sub, _active_poses(poses, active, environment), jobs, p, tol, 0.0, 0).cpu().numpy())
        touches = sorted({"plane" if b == PLANE else "environment" if b == len(active) else active[b if a == len(active) - 1 else a]
                          for (a, b, _), phi in zip(jobs, value[:, 0]) if phi <= 2.0 * tol}, key=str)
        reports[k] = dict(order=rank, rounds=rounds, settled=settled, travel=travel, touches=touches, phi0=float(value[:, 0].min()))
        placed.append(k)
        world = body.mesh.vertices.astype(np.float64) @ poses[k, :3, :3].T + poses[k, :3, 3]
        tops.append(float((world @ n).max()) - d)
    return poses, reports


def _active_poses(poses, active, environment):
    return poses[active] if environment is None else np.concatenate([poses[active], np.eye(4)[None]])


# ---- files ------------------------------------------------------------------------------------------------------------
def reference_translation(T, center) -> np.ndarray:
    """The ``t`` the reference's file holds for a mesh-frame pose (R, T): it applies a pose about the cloud mean mu,
    R (x - mu) + mu + t, so t = T - mu + R mu."""
    T = np.asarray(T, np.float64)
    mu = np.asarray(center, np.float64)
    return T[:3, 3] - mu + T[:3, :3] @ mu


def write_simulation_steps(path, names, class_names, object_ids, poses, centers=None, steps: int = 1) -> dict:
    """Writes poses in the layout of the reference's ``simulation_steps.json``: ``asset_infos`` (per object name its
    ``bullet_id`` list, ``center_of_mass``, ``class_name`` and ``object_ID``; the ground as body 0 of the environment) and
    ``trajectory[str(bullet id)][str(step)] = {"t", "q"}`` with q in x, y, z, w; ``steps`` equal steps.  Body k of the list gets
    bullet id k + 1.  ``centers`` [B,3]: the points the reference applies each pose about (its cloud means; default: the
    origin), see ``reference_translation``.  Returns the document."""
    from scipy.spatial.transform import Rotation
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    B = len(poses)
    if not (len(names) == len(class_names) == len(object_ids) == B):
        raise ValueError("one name, class name and object id per pose")
    if steps < 1:
        raise ValueError("at least one step")
    centers = np.zeros((B, 3)) if centers is None else np.asarray(centers, np.float64).reshape(B, 3)
    objects, trajectory = {}, {"0": {str(s): {"t": [0.0, 0.0, 0.0], "q": [0.0, 0.0, 0.0, 1.0]} for s in range(steps)}}
    for k in range(B):
        entry = objects.setdefault(str(names[k]), {"bullet_id": [], "center_of_mass": centers[k].tolist(),
                                                   "class_name": str(class_names[k]), "object_ID": int(object_ids[k])})
        entry["bullet_id"].append(k + 1)
        t = reference_translation(poses[k], centers[k]).tolist()
        q = Rotation.from_matrix(poses[k, :3, :3]).as_quat().tolist()
        trajectory[str(k + 1)] = {str(s): {"t": t, "q": q} for s in range(steps)}
    doc = {"asset_infos": {"environment": {"plane": {"bullet_id": [0], "class_name": "plane"}}, "object": objects},
           "trajectory": trajectory}
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(doc))
    return doc


def read_simulation_steps(path, step: int = -1):
    """{bullet id: [7] float64 (t, q in x,y,z,w)} of one step of a file in that layout (default: the last, as the reference's
    static mode reads it); ``trajectory.absolute_pose(row[None], 0)`` turns a row into the 4x4."""
    doc = json.loads(Path(path).read_text())
    out = {}
    for key, traj in doc["trajectory"].items():
        last = list(traj.keys())[step]
        out[int(key)] = np.asarray(list(traj[last]["t"]) + list(traj[last]["q"]), np.float64)
    return out


def check_dataset(dataset_dir, models_dir, translation_scale: float = 1.0, split: str = "train", resolution: int = 96,
                  device="cuda", environment=None) -> dict:
    """{scene path: {image id: the deepest interpenetration of the image's scene_gt poses}}: the smallest entry of
    ``min_distances`` between its objects (model-to-camera poses, so no plane), in scene_gt's unit; +inf for fewer than two.
    ``environment``: an ``environment.EnvironmentField`` in metres and world coordinates; the objects are then also held against
    its field, placed by the image's cam_R_w2c / cam_t_w2c of scene_camera.json (an image without them is an error)."""
    if environment is not None:
        from .environment import EnvironmentField
        from .mesh import Grid
        g, k = environment.grid, float(translation_scale)
        environment = EnvironmentField(environment.field * k, Grid(g.nx, g.ny, g.nz, tuple(float(o) * k for o in g.origin), g.voxel * k),
                                       environment.friction)
    scenes = BD.scene_dirs(dataset_dir, split)
    cache, out = {}, {}
    unit = BD.unit_of(translation_scale)
    for scene in map(BD.BopScene, scenes):
        per_image = {}
        for image, entries in scene.gt.items():
            ids = [int(e["obj_id"]) for e in entries]
            for i in ids:
                if i not in cache:
                    cache.update(bodies_from_dir(models_dir, unit, [i], resolution, device))
            poses = []
            for e in entries:
                T = np.eye(4)
                T[:3, :3], T[:3, 3] = BD.pose_of(e)
                poses.append(T)
            env_pose = None
            if environment is not None:
                cam = scene.camera[str(image)]
                if "cam_R_w2c" not in cam or "cam_t_w2c" not in cam:
                    raise ValueError(f"{scene.path} image {image}: scene_camera.json has no cam_R_w2c / cam_t_w2c to place the environment")
                env_pose = np.eye(4)
                env_pose[:3, :3] = np.asarray(cam["cam_R_w2c"], np.float64).reshape(3, 3)
                env_pose[:3, 3] = np.asarray(cam["cam_t_w2c"], np.float64).reshape(3)
            D = min_distances([cache[i] for i in ids], np.asarray(poses).reshape(-1, 4, 4), environment=environment,
                              environment_pose=env_pose)
            per_image[str(image)] = float(D.min()) if D.size else float("inf")
        out[str(scene.path)] = per_image
    return out


def _parser():
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.collision", description=__doc__.split("\n\n")[0])
    p.add_argument("--models", required=True, help="a models/ or models_eval/ directory (obj_NNNNNN.ply), or the urdf/ "
                                                   "directory of mesh --collision_faces (obj_NNNNNN_collision.obj)")
    p.add_argument("--objects", type=int, nargs="+", default=None, help="object ids to place (default: all)")
    p.add_argument("--count", type=int, default=1, help="instances of every object")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--radius", type=float, default=None, help="radius of the disc the objects are dropped over (default: the "
                                                              "largest object's half diagonal)")
    p.add_argument("--scale", type=float, default=1.0, help="what the mesh files' vertices are multiplied by (0.001: BOP "
                                                            "millimetres -> metres)")
    p.add_argument("--resolution", type=int, default=96, help="grid points along a field's longest axis")
    p.add_argument("--tol", type=float, default=1e-4)
    p.add_argument("--steps", type=int, default=1, help="equal steps written to the file")
    p.add_argument("--out", default=None, help="the simulation_steps.json to write")
    p.add_argument("--check", default=None, metavar="DATASET", help="report the deepest interpenetration of every image's "
                                                                    "scene_gt poses instead of placing anything")
    p.add_argument("--environment", default=None, metavar="NPZ", help="the environment's field (python -m pegasus_amd.environment): "
                                                                      "objects are placed on it, or with --check held against it")
    p.add_argument("--translation_scale", type=float, default=1.0,
                   help="--check: what scene_gt's translations were written with: 1 = metres, 1000 = millimetres")
    return p


def _load_environment(a):
    if not a.environment:
        return None
    from .environment import EnvironmentField
    return EnvironmentField.load(a.environment)


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = _parser().parse_args(argv)
    if a.check:
        report = check_dataset(a.check, a.models, a.translation_scale, resolution=a.resolution, environment=_load_environment(a))
        for scene, images in report.items():
            for image, depth in images.items():
                print(f"{scene} {image}: {depth:.6g}")
        worst = min((x for images in report.values() for x in images.values()), default=float("inf"))
        print(f"deepest interpenetration: {worst:.6g}")
        return 0
    if not a.out:
        raise SystemExit("--out is required unless --check is given")
    by_id = bodies_from_dir(a.models, a.scale, a.objects, a.resolution)
    ids = [i for i in by_id for _ in range(max(1, a.count))]
    bodies = [by_id[i] for i in ids]
    poses, reports = drop(bodies, radius=a.radius, seed=a.seed, tol=a.tol, environment=_load_environment(a))
    centers = [b.mesh.vertices.astype(np.float64).mean(0) for b in bodies]
    names = [BD.model_stem(i) for i in ids]
    write_simulation_steps(a.out, names, names, ids, poses, centers, a.steps)
    for i, r in zip(ids, reports):
        print(f"object {i}: rounds {r['rounds']} settled {r['settled']} touches {r['touches']}")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
