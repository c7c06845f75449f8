"""Rigid-body drops on the HIP library: what the reference's ``PybulletEngine.simulate()`` (src/engine/physical_simulation.py)
does with pybullet -- objects fall under gravity (0, 0, -50) in 1 ms steps onto a plane and onto each other, and every body's
``{t, q}`` per step goes to ``simulation_steps.json`` -- as batches of independent worlds on the GPU.  Contacts come from the
collision geometry of ``pegasus_amd.collision`` (mesh distance fields and shell points), a sequential-impulse solver with
friction steps them (``pgr_rigid_contacts``, ``pgr_rigid_simulate``).  The rule stands at the top of
pegasus_amd/csrc/rigid.hip.h and in DESIGN.md section 24; parity with pybullet's own trajectories is not pinned.

    python -m pegasus_amd.dynamics --models <dir> --objects 1 2 5 --scenes 10 --steps 4000 --seed 0 --out <dir>

writes <dir>/scene_NNNNNN/simulation_steps.json for every scene; all scenes run as one batch of worlds.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib, bop_dataset as BD, collision as COL

MAX_BODIES = _lib.PGR_RIGID_MAX_BODIES
MAX_TYPES = _lib.PGR_RIGID_MAX_TYPES
WORDS = _lib.PGR_RIGID_WORDS
STATE = _lib.PGR_RIGID_STATE


@dataclass
class RigidBody:
    """A body type: collision geometry with mass, centre of mass and inverse inertia (mesh frame), friction and the bounding
    radius max |shell - com|."""
    body: COL.CollisionBody
    mass: float
    friction: float
    com: np.ndarray
    inv_inertia: np.ndarray
    radius: float

    @staticmethod
    def from_collision(body: COL.CollisionBody, mass: float = 1.0, friction: float = 0.5) -> "RigidBody":
        """Uniform density: centre of mass and inertia from ``Mesh.center_of_mass`` / ``Mesh.inertia``."""
        if not (np.isfinite(mass) and mass > 0):
            raise ValueError("mass must be positive")
        if not (np.isfinite(friction) and friction >= 0):
            raise ValueError("friction must not be negative")
        com = np.asarray(body.mesh.center_of_mass(), np.float64)
        inertia = np.asarray(body.mesh.inertia(float(mass)), np.float64)
        if not (np.isfinite(com).all() and np.isfinite(inertia).all() and np.linalg.eigvalsh(inertia).min() > 0):
            raise ValueError("the mesh gives no positive inertia (is it closed and outward wound?)")
        shell = body.shell.detach().cpu().numpy().astype(np.float64)
        radius = float(np.linalg.norm(shell - com, axis=1).max()) if len(shell) else 0.0
        return RigidBody(body, float(mass), float(friction), com, np.linalg.inv(inertia), radius)

    def struct(self) -> _lib.PgrRigidType:
        b = self.body
        return _lib.PgrRigidType(grid=b.sdf.grid.struct(), sdf=b.sdf.field.data_ptr(), shell=b.shell.data_ptr() if len(b.shell) else None,
                                 n_shell=len(b.shell), mass=self.mass, com=(C.c_float * 3)(*self.com),
                                 inv_inertia=(C.c_float * 9)(*np.asarray(self.inv_inertia).reshape(-1)), friction=self.friction,
                                 radius=self.radius)


@dataclass
class Params:
    """The parameters of a step.  h, gravity, friction and damping are the reference's (pybullet's defaults where it sets none);
    the others are this project's choice.  ``margin`` None: the largest voxel in play."""
    h: float = 1e-3
    gravity: Sequence[float] = (0.0, 0.0, -50.0)
    plane: Sequence[float] = (0.0, 0.0, 1.0, 0.0)
    plane_friction: float = 0.5
    lin_damp: float = 0.04
    ang_damp: float = 0.04
    iterations: int = 10
    beta: float = 0.2
    slop: float = 2e-4
    margin: Optional[float] = None
    v_sleep: float = 0.02
    w_sleep: float = 0.4
    sleep_steps: int = 50

    def struct(self, bodies: Sequence[RigidBody]) -> _lib.PgrRigidParams:
        margin = max((b.body.voxel for b in bodies), default=0.0) if self.margin is None else self.margin
        plane = COL.unit_plane(self.plane)
        return _lib.PgrRigidParams(h=self.h, gravity=(C.c_float * 3)(*self.gravity), plane=(C.c_float * 4)(*plane),
                                   plane_friction=self.plane_friction, lin_damp=self.lin_damp, ang_damp=self.ang_damp,
                                   iterations=int(self.iterations), beta=self.beta, slop=self.slop, margin=margin,
                                   v_sleep=self.v_sleep, w_sleep=self.w_sleep, sleep_steps=int(self.sleep_steps))


def _rotation(q) -> np.ndarray:
    """R(q) [...,3,3] of unit quaternions [...,4] in x, y, z, w."""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def _table(bodies: Sequence[RigidBody]):
    if not 1 <= len(bodies) <= MAX_TYPES:
        raise ValueError(f"1..{MAX_TYPES} body types, got {len(bodies)}")
    table = (_lib.PgrRigidType * len(bodies))()
    for k, b in enumerate(bodies):
        table[k] = b.struct()
    return table


def _types(types, n_types: int) -> np.ndarray:
    t = np.asarray(types, np.int64)
    if t.ndim == 1:
        t = t[None]
    if t.ndim != 2 or t.shape[1] > MAX_BODIES:
        raise ValueError(f"types must be [S,B] with B <= {MAX_BODIES}")
    if (t >= n_types).any():
        raise ValueError("a type index outside the table")
    return np.where(t < 0, -1, t).astype(np.int32)


def states_from_poses(bodies: Sequence[RigidBody], types, poses0, velocities=None) -> np.ndarray:
    """float32 [S,B,13]: the state (centre of mass x = t + R com, q, v, omega) of mesh-frame poses [S,B,7] (t, q in x,y,z,w; q is
    normalised); ``velocities`` [S,B,6] (v, omega) default to rest."""
    t = _types(types, len(bodies))
    poses = np.asarray(poses0, np.float64).reshape(t.shape + (7,))
    if not np.isfinite(poses).all():
        raise ValueError("poses must be finite")
    norm = np.linalg.norm(poses[..., 3:], axis=-1, keepdims=True)
    if (norm[t >= 0] <= 0).any():
        raise ValueError("a zero quaternion")
    q = poses[..., 3:] / np.where(norm > 0, norm, 1.0)
    com = np.stack([b.com for b in bodies])[np.maximum(t, 0)]
    state = np.zeros(t.shape + (STATE,), np.float64)
    state[..., 0:3] = poses[..., :3] + np.einsum("...ij,...j->...i", _rotation(q), com)
    state[..., 3:7] = q
    if velocities is not None:
        state[..., 7:13] = np.asarray(velocities, np.float64).reshape(t.shape + (6,))
    state[t < 0] = 0.0
    state[t < 0, 6] = 1.0
    return state.astype(np.float32)


def _device_of(bodies):
    return bodies[0].body.sdf.field.device


def _ground_arg(ground):
    """(the PgrRigidGround pointer the *_ground entries take, what keeps it alive); NULL for no ground."""
    if ground is None:
        return None, None
    g = ground.struct()
    return C.byref(g), (g, ground)


def contacts(bodies: Sequence[RigidBody], types, state, params: Optional[Params] = None, ground=None):
    """``pgr_rigid_contacts``: the contact words int64 [S, B*B, 7] (device; ``collision.decode_words`` reads them on the host)
    of a state [S,B,13].  ``ground``: an ``environment.EnvironmentField`` that takes the plane's place
    (``pgr_rigid_contacts_ground``)."""
    import torch
    params = params or Params()
    t = _types(types, len(bodies))
    S, B = t.shape
    device = _device_of(bodies)
    d_type = torch.from_numpy(t).to(device)
    d_state = torch.as_tensor(np.asarray(state, np.float32).reshape(S, B, STATE)).to(device).contiguous()
    words = torch.empty((S, B * B, WORDS), dtype=torch.int64, device=device)
    if S == 0 or B == 0:
        return words
    ws = _lib.workspace("pgr_rigid", device, S, B)
    p = params.struct(bodies)
    g, keep = _ground_arg(ground)
    _lib.call("pgr_rigid_contacts_ground", device, C.byref(p), g, len(bodies), _table(bodies), S, B, _lib.ptr(d_type),
              _lib.ptr(d_state), _lib.ptr(words), _lib.ptr(ws), ws.numel())
    del keep
    return words


def simulate(bodies: Sequence[RigidBody], types, poses0=None, steps: int = 1000, params: Optional[Params] = None,
             record_every: int = 1, velocities=None, state=None, return_state: bool = False, ground=None):
    """``pgr_rigid_simulate``: S worlds of B slots (``types`` [S,B], -1 = empty) from mesh-frame poses ``poses0`` [S,B,7] (or a
    full ``state`` [S,B,13]) for ``steps`` steps, all enqueued on the current stream.  Returns device tensors: trajectory float32
    [S, steps // record_every, B, 7] (mesh-frame t, q in x,y,z,w after every record_every-th step), rest_step int32 [S] (-1: never
    came to rest), status int32 [S] (1: the state stopped being finite; the world stays at its last finite state); with
    ``return_state`` also the final state [S,B,13].  ``ground``: an ``environment.EnvironmentField`` the bodies fall onto instead
    of the plane (``pgr_rigid_simulate_ground``); outside its grid box nothing is below a body."""
    import torch
    params = params or Params()
    if steps < 0 or record_every < 1:
        raise ValueError("steps >= 0 and record_every >= 1")
    t = _types(types, len(bodies))
    S, B = t.shape
    if state is None:
        if poses0 is None:
            raise ValueError("poses0 or state")
        state = states_from_poses(bodies, t, poses0, velocities)
    device = _device_of(bodies)
    d_type = torch.from_numpy(t).to(device)
    d_state = torch.as_tensor(np.asarray(state, np.float32).reshape(S, B, STATE)).to(device).contiguous().clone()
    n_records = steps // record_every
    traj = torch.zeros((S, n_records, B, 7), dtype=torch.float32, device=device)
    rest = torch.full((S,), -1, dtype=torch.int32, device=device)
    status = torch.zeros((S,), dtype=torch.int32, device=device)
    if S and B:
        ws = _lib.workspace("pgr_rigid", device, S, B)
        p = params.struct(bodies)
        g, keep = _ground_arg(ground)
        _lib.call("pgr_rigid_simulate_ground", device, C.byref(p), g, len(bodies), _table(bodies), S, B, _lib.ptr(d_type),
                  _lib.ptr(d_state), int(steps), int(record_every), _lib.ptr(traj) if n_records else None, _lib.ptr(rest),
                  _lib.ptr(status), _lib.ptr(ws), ws.numel())
        del keep
    return (traj, rest, status, d_state) if return_state else (traj, rest, status)


# ---- start states ---------------------------------------------------------------------------------------------------------
def start_quaternion(rng) -> np.ndarray:
    """The reference's start orientation: four uniform(0, 1) draws, normalised (x, y, z, w)."""
    q = rng.uniform(0.0, 1.0, 4)
    while not np.linalg.norm(q) > 0:
        q = rng.uniform(0.0, 1.0, 4)
    return q / np.linalg.norm(q)


def start_states(bodies: Sequence[RigidBody], types, seed: int, radius: Optional[float] = None, gap: Optional[float] = None,
                 plane=(0.0, 0.0, 1.0, 0.0), ground=None) -> np.ndarray:
    """Mesh-frame start poses float64 [S,B,7] from the generator seeded with ``seed``: per slot the reference's start orientation,
    a position in the disc of ``radius`` (default: the largest body's half diagonal) over the plane, and a height
    (``collision.start_height``) that puts its lowest point ``gap`` (default: two of the largest voxel) above everything placed
    before it in its world.  With a ``ground`` (an ``environment.EnvironmentField``; the plane must be z = d) also above the
    ground's highest solid point under the body's footprint."""
    t = _types(types, len(bodies))
    p = COL.unit_plane(plane)
    n, d = p[:3], float(p[3])
    u, v = COL._plane_frame(n)
    rng = np.random.default_rng(seed)
    verts = [b.body.mesh.vertices.astype(np.float64) for b in bodies]
    if radius is None:
        radius = 0.5 * max(float(np.linalg.norm(np.ptp(x, axis=0))) for x in verts)
    if gap is None:
        gap = 2.0 * max(b.body.voxel for b in bodies)
    poses = np.zeros(t.shape + (7,))
    poses[..., 6] = 1.0
    for w in range(t.shape[0]):
        tops = []
        for k in range(t.shape[1]):
            if t[w, k] < 0:
                continue
            q = start_quaternion(rng)
            R = _rotation(q)
            r, phi = radius * np.sqrt(rng.uniform()), rng.uniform(0.0, 2.0 * np.pi)
            h = COL.start_height(verts[t[w, k]], R, tops, n, gap)
            at = d * n + r * np.cos(phi) * u + r * np.sin(phi) * v
            if ground is not None:
                h = max(h, COL.environment_start_height(ground, verts[t[w, k]], R, at, gap) - d)
            poses[w, k, :3] = at + h * n
            poses[w, k, 3:] = q
            tops.append(float((verts[t[w, k]] @ R.T @ n).max()) + h)
    return poses


# ---- files ------------------------------------------------------------------------------------------------------------------
def write_trajectory(path, names, class_names, object_ids, trajectory, centers=None, environment: Optional[str] = None) -> dict:
    """``collision.write_simulation_steps``' layout with a pose per step: ``trajectory`` [n_steps, B, 7] holds mesh-frame poses
    (t, q in x,y,z,w); body k gets bullet id k + 1 and its ``t`` is converted by ``collision.reference_translation`` about
    ``centers[k]`` (default: the origin).  ``environment``: the name body 0 gets in ``asset_infos.environment`` instead of the
    plane's.  Returns the document."""
    traj = np.asarray(trajectory, np.float64)
    if traj.ndim != 3 or traj.shape[2] != 7 or traj.shape[0] < 1:
        raise ValueError("trajectory must be [n_steps >= 1, B, 7]")
    n_steps, B = traj.shape[:2]
    if not (len(names) == len(class_names) == len(object_ids) == B):
        raise ValueError("one name, class name and object id per body")
    if not np.isfinite(traj).all():
        raise ValueError("the trajectory holds values that are not finite")
    centers = np.zeros((B, 3)) if centers is None else np.asarray(centers, np.float64).reshape(B, 3)
    objects = {}
    doc_traj = {"0": {str(s): {"t": [0.0, 0.0, 0.0], "q": [0.0, 0.0, 0.0, 1.0]} for s in range(n_steps)}}
    for k in range(B):
        entry = objects.setdefault(str(names[k]), {"bullet_id": [], "center_of_mass": centers[k].tolist(),
                                                   "class_name": str(class_names[k]), "object_ID": int(object_ids[k])})
        entry["bullet_id"].append(k + 1)
        steps = {}
        R = _rotation(traj[:, k, 3:] / np.linalg.norm(traj[:, k, 3:], axis=-1, keepdims=True))
        for s in range(n_steps):
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R[s], traj[s, k, :3]
            steps[str(s)] = {"t": COL.reference_translation(T, centers[k]).tolist(), "q": traj[s, k, 3:].tolist()}
        doc_traj[str(k + 1)] = steps
    env = {"plane": {"bullet_id": [0], "class_name": "plane"}} if environment is None else \
        {str(environment): {"bullet_id": [0], "class_name": "environment"}}
    doc = {"asset_infos": {"environment": env, "object": objects}, "trajectory": doc_traj}
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(doc))
    return doc


def outside_ground(ground, poses) -> np.ndarray:
    """bool [...]: the mesh-frame poses [...,7] whose origin lies outside the ground's grid box, where nothing is below a body."""
    lo, hi = ground.box()
    t = np.asarray(poses, np.float64)[..., :3]
    return ((t < lo) | (t > hi)).any(axis=-1)


@dataclass
class Engine:
    """The surface of the reference's ``PybulletEngine``: ``add_object(object_instance, start_pos, start_orientation_euler)``
    and ``simulate()``, which writes ``output_path_json`` in the reference's layout.  ``bodies``: {object id: RigidBody}.  An
    object instance has ``TYPE`` ('environment': the ground, recorded as body 0 -- the plane, or the instance's ``field``, an
    ``environment.EnvironmentField``, where it has one; 'object'), and for an object ``ID`` and optionally ``urdf_file_name``.  As in the reference the Euler angles are not used: an object starts in four uniform(0, 1)
    draws, normalised -- here from the generator seeded with ``seed``."""
    bodies: dict
    output_path_json: str = "simulation_steps.json"
    simulation_steps: int = 1000
    seed: int = 0
    params: Params = field(default_factory=Params)
    record_every: int = 1
    ground: object = None
    environment_name: Optional[str] = None

    def __post_init__(self):
        if self.simulation_steps < 1 or self.record_every < 1 or self.simulation_steps // self.record_every < 1:
            raise ValueError("simulation_steps and record_every must give at least one record")
        self._rng = np.random.default_rng(self.seed)
        self._objects = []                # (name, class name, object id, start pose [7])

    def add_object(self, object_instance, start_pos=(0.0, 0.0, 0.0), start_orientation_euler=(0.0, 0.0, 0.0)):
        kind = getattr(object_instance, "TYPE", None)
        if kind == "environment":
            if getattr(object_instance, "field", None) is not None:
                self.ground = object_instance.field
                self.environment_name = str(getattr(object_instance, "urdf_file_name", "environment")).split(".")[0]
            return
        if kind != "object":
            raise ValueError(f"Wrong entity - {kind}")
        obj_id = int(object_instance.ID)
        if obj_id not in self.bodies:
            raise KeyError(f"object {obj_id} has no body")
        if len(self._objects) >= MAX_BODIES:
            raise ValueError(f"a world holds at most {MAX_BODIES} bodies")
        pos = np.asarray(start_pos, np.float64).reshape(-1)
        if pos.shape != (3,) or not np.isfinite(pos).all():
            raise ValueError("start_pos must be three finite numbers")
        name = str(getattr(object_instance, "urdf_file_name", BD.model_stem(obj_id))).split(".")[0]
        self._objects.append((name, object_instance.__class__.__name__, obj_id, np.concatenate([pos, start_quaternion(self._rng)])))

    def simulate(self):
        """Runs the drop (one world) and writes the file.  Returns (trajectory [n_records,B,7], rest_step, status) on the host."""
        if not self._objects:
            raise ValueError("no object was added")
        ids = sorted({o[2] for o in self._objects})
        if len(ids) > MAX_TYPES:
            raise ValueError(f"at most {MAX_TYPES} different objects")
        table = [self.bodies[i] for i in ids]
        types = [[ids.index(o[2]) for o in self._objects]]
        # start_pos is where pybullet puts the link frame's origin, which is the mesh frame's here
        poses = np.stack([o[3] for o in self._objects])[None]
        traj, rest, status = simulate(table, types, poses, self.simulation_steps, self.params, self.record_every, ground=self.ground)
        traj = traj[0].cpu().numpy()
        centers = [self.bodies[o[2]].body.mesh.vertices.astype(np.float64).mean(0) for o in self._objects]
        write_trajectory(self.output_path_json, [o[0] for o in self._objects], [o[1] for o in self._objects],
                         [o[2] for o in self._objects], traj, centers,
                         environment=(self.environment_name or "environment") if self.ground is not None else None)
        return traj, int(rest[0]), int(status[0])


def bodies_from_dir(models_dir, scale: float = 1.0, objects=None, resolution: int = 96, mass: float = 1.0, friction: float = 0.5,
                    device="cuda") -> dict:
    """{obj_id: RigidBody} of a models directory (``collision.bodies_from_dir``)."""
    return {i: RigidBody.from_collision(b, mass, friction)
            for i, b in COL.bodies_from_dir(models_dir, scale, objects, resolution, device).items()}


def _parser():
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.dynamics", description=__doc__.split("\n\n")[0])
    p.add_argument("--models", required=True, help="a models/ or models_eval/ directory (obj_NNNNNN.ply), or the urdf/ directory "
                                                   "of mesh --collision_faces (obj_NNNNNN_collision.obj)")
    p.add_argument("--objects", type=int, nargs="+", required=True, help="object ids dropped in every scene, in this order")
    p.add_argument("--scenes", type=int, default=1, help="independent scenes: one batch of worlds")
    p.add_argument("--steps", type=int, default=4000)
    p.add_argument("--record_every", type=int, default=1)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--scale", type=float, default=1.0, help="what the mesh files' vertices are multiplied by (0.001: BOP "
                                                            "millimetres -> metres)")
    p.add_argument("--resolution", type=int, default=96, help="grid points along a field's longest axis")
    p.add_argument("--radius", type=float, default=None, help="radius of the disc the objects start over")
    p.add_argument("--mass", type=float, default=1.0)
    p.add_argument("--friction", type=float, default=0.5)
    p.add_argument("--environment", default=None, metavar="NPZ", help="the ground as a field (python -m pegasus_amd.environment) "
                                                                      "instead of the plane z = 0")
    p.add_argument("--out", required=True, help="directory: scene_NNNNNN/simulation_steps.json per scene")
    return p


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = _parser().parse_args(argv)
    if a.scenes < 1 or a.steps < 1 or a.record_every < 1 or a.steps // a.record_every < 1:
        raise SystemExit("--scenes, --steps and --record_every must be positive and give at least one record")
    if len(a.objects) > MAX_BODIES:
        raise SystemExit(f"at most {MAX_BODIES} objects per scene")
    ids = sorted(set(a.objects))
    if len(ids) > MAX_TYPES:
        raise SystemExit(f"at most {MAX_TYPES} different objects")
    by_id = bodies_from_dir(a.models, a.scale, ids, a.resolution, a.mass, a.friction)
    table = [by_id[i] for i in ids]
    types = np.tile(np.array([ids.index(i) for i in a.objects], np.int32), (a.scenes, 1))
    ground = None
    if a.environment:
        from .environment import EnvironmentField
        ground = EnvironmentField.load(a.environment)
    poses = start_states(table, types, a.seed, a.radius, ground=ground)
    traj, rest, status = simulate(table, types, poses, a.steps, record_every=a.record_every, ground=ground)
    traj, rest, status = traj.cpu().numpy(), rest.cpu().numpy(), status.cpu().numpy()
    names = [BD.model_stem(i) for i in a.objects]
    centers = [by_id[i].body.mesh.vertices.astype(np.float64).mean(0) for i in a.objects]
    for w in range(a.scenes):
        path = Path(a.out) / f"scene_{w:06d}" / "simulation_steps.json"
        write_trajectory(path, names, names, a.objects, traj[w], centers,
                         environment=Path(a.environment).stem if ground is not None else None)
        state = "not finite, frozen" if status[w] else (f"at rest after step {rest[w]}" if rest[w] >= 0 else "still moving")
        if ground is not None and outside_ground(ground, traj[w, -1]).any():
            state += "; a body left the environment's grid box (nothing is below it there)"
        print(f"scene {w}: {state} -> {path}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
