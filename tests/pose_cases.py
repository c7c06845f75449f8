"""Inputs of the posing tests, built in NumPy only and shared by tests/test_pose_host.py (CPU) and tests/test_pose_gpu.py:
rotations at the edges of pose_prepare_kernel's branch rule, clouds at the edges of the block and partition sizes, and job
tables for one pgr_pose_objects call.  Every array is float32: exactly what the kernels get."""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

XYZ, ROT, SH = 0, 1, 2                                   # PgrPoseKind
SIZES = (0, 1, 31, 32, 33, 255, 256, 257, 8191, 8192, 8193)      # 256-row blocks, 32 partitions of the mean
BIG = 2_000_003
FAR = np.array([1000.0, -2000.0, 500.0])
QUAT_NORMS = (1.0, 0.2, 3.0, 1e-10, 1e-13, 1e-18, 1e-25, 0.0)
N_RESTS = (0, 3, 8, 15)
JOB_COUNTS = (1, 15, 16, 17, 32, 33, 48)


@dataclass
class RotationCase:
    name: str
    R: np.ndarray                                        # [3,3] float32
    reach: Tuple[str, ...] = ()                          # census keys (pose_reference.census) the case is there to reach


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def half_turn(axis):
    """180 degrees about an axis with integer components: 2 a a^T / (a.a) - I, exact zeros and exact ties."""
    a = np.asarray(axis, np.float64)
    return 2.0 * np.outer(a, a) / (a @ a) - np.eye(3)


def _axis_with_largest(rng, k):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    j = int(np.argmax(np.abs(a)))
    a[[k, j]] = a[[j, k]]
    return a


def _random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def accumulated_rotation(steps=1000, seed=77):
    """A product of float32 delta rotations, every product rounded to float32: slightly non-orthonormal, as an accumulated
    trajectory is."""
    rng = np.random.default_rng(seed)
    R = np.eye(3, dtype=np.float32)
    for _ in range(steps):
        d = rodrigues(rng.normal(size=3), rng.normal(0, 0.05)).astype(np.float32)
        R = (d @ R).astype(np.float32)
    return R


def rotation_cases():
    rng = np.random.default_rng(4242)
    P = lambda rows: np.array(rows, np.float64)
    cases = [
        RotationCase("identity", np.eye(3), ("trace",)),
        RotationCase("90x", P([[1, 0, 0], [0, 0, -1], [0, 1, 0]]), ("trace", "tr==m00", "m11==m22")),
        RotationCase("90y", P([[0, 0, 1], [0, 1, 0], [-1, 0, 0]]), ("trace", "tr==m11", "m00==m22")),
        RotationCase("90z", P([[0, -1, 0], [1, 0, 0], [0, 0, 1]]), ("trace", "tr==m22", "m00==m11")),
        RotationCase("120_111", P([[0, 0, 1], [1, 0, 0], [0, 1, 0]]),
                     ("trace", "tr==m00", "tr==m11", "tr==m22", "m00==m11", "m00==m22", "m11==m22")),
        RotationCase("180x", half_turn([1, 0, 0]), ("x", "m11==m22")),
        RotationCase("180y", half_turn([0, 1, 0]), ("y", "m00==m22")),
        RotationCase("180z", half_turn([0, 0, 1]), ("z", "m00==m11")),
        RotationCase("180_110", half_turn([1, 1, 0]), ("x", "m00==m11")),
        RotationCase("180_111", half_turn([1, 1, 1]), ("x", "m00==m11", "m00==m22", "m11==m22")),
        # not in the issue's list, added: the y branch entered THROUGH its tie, and the x branch through m00 == m22
        RotationCase("180_011", half_turn([0, 1, 1]), ("y", "m11==m22")),
        RotationCase("180_101", half_turn([1, 0, 1]), ("x", "m00==m22")),
    ]
    for short, below in (("1e-3", 1e-3), ("1e-6", 1e-6)):
        for k, b in enumerate("xyz"):
            cases.append(RotationCase(f"180-{short}_{b}", rodrigues(_axis_with_largest(rng, k), np.pi - below), (b,)))
    cases.append(RotationCase("angle_1e-4", rodrigues(rng.normal(size=3), 1e-4), ("trace",)))
    cases.append(RotationCase("angle_1e-8", rodrigues(rng.normal(size=3), 1e-8), ("trace",)))
    cases.append(RotationCase("accumulated_1000", accumulated_rotation(), ()))
    for k in range(32):
        cases.append(RotationCase(f"random_{k}", _random_rotation(rng), ()))
    for c in cases:
        c.R = np.ascontiguousarray(c.R, dtype=np.float32)
    return cases


def cloud(n, far=False, seed=0):
    """[n,3] float32: a cloud of extent ~0.3 at the origin, or of extent 0.1 at FAR (centre precision, cancellation)."""
    rng = np.random.default_rng(1000 + seed)
    x = FAR + rng.uniform(-0.05, 0.05, (n, 3)) if far else rng.normal(0, 0.3, (n, 3)) + rng.normal(0, 0.2, 3)
    return np.ascontiguousarray(x, dtype=np.float32)


def quats(n, seed=0):
    """[n,4] float32 rows whose norms cycle through QUAT_NORMS."""
    rng = np.random.default_rng(2000 + seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    norms = np.array(QUAT_NORMS)[(np.arange(n) + seed) % len(QUAT_NORMS)]
    return np.ascontiguousarray(q * norms[:, None], dtype=np.float32)


def coefficients(n, n_rest, seed=0):
    return np.ascontiguousarray(np.random.default_rng(3000 + seed).normal(size=(n, n_rest, 3)), dtype=np.float32)


def unit_rows(n_rest=15):
    """[n_rest, n_rest, 3]: row k holds e_k in every colour channel; an SH job on it returns the columns of D1, D2, D3."""
    e = np.zeros((n_rest, n_rest, 3), np.float32)
    e[np.arange(n_rest), np.arange(n_rest), :] = 1.0
    return e


@dataclass
class Job:
    kind: int
    src: np.ndarray                                      # [n,3] | [n,4] | [n,n_rest,3] float32
    R: Optional[np.ndarray] = None                       # [3,3] float32 or None (NULL: identity)
    t: Optional[np.ndarray] = None                       # [3] float32 or None (NULL: zero)
    about_origin: bool = False
    R_row_stride: int = 0                                # 0 (the ABI's default: 3), 3, or 4 = the corner of a 4x4
    t_stride: int = 0                                    # 0 (default: 1), 1, or 4 = the last column of a 4x4
    in_place: bool = False                               # src == dst
    hostile: bool = False                                # rows of NaN / Inf: checked only for leaving other jobs alone
    note: str = ""
    n_rest: int = field(init=False, default=0)

    def __post_init__(self):
        self.n_rest = int(self.src.shape[1]) if self.kind == SH else 0

    @property
    def n(self):
        return int(self.src.shape[0])


def job_table(count, seed, empty=()):
    """``count`` jobs of seeded interleaved kinds; ``empty``: positions whose job has n = 0.  Sizes, rotations, strides and the
    XYZ variants (NULL R with t, NULL R and NULL t, about_origin with and without t, src == dst) cycle with seeded offsets."""
    rng = np.random.default_rng(9000 + seed)
    rots = rotation_cases()
    kinds = rng.integers(0, 3, count)
    if count >= 3:
        kinds[rng.permutation(count)[:3]] = (XYZ, ROT, SH)           # every kind in every table of three or more
    sizes = [s for s in SIZES if s]
    o_size, o_rot, o_var = (int(v) for v in rng.integers(0, 64, 3))
    jobs = []
    for k in range(count):
        n = 0 if k in empty else sizes[(k + o_size) % len(sizes)]
        rc = rots[(k * 5 + o_rot) % len(rots)]
        rs, ts = (0, 3, 4)[(k + seed) % 3], (0, 1, 4)[(k // 3 + seed) % 3]
        in_place = (k + o_var) % 4 == 0
        s = 100 * seed + k
        if kinds[k] == XYZ:
            var = (k + o_var) % 6
            t = np.random.default_rng(s).normal(0, 0.2, 3).astype(np.float32)
            src = cloud(n, far=(k + o_var) % 2 == 1, seed=s)
            if var == 0:
                j = Job(XYZ, src, None, t, t_stride=ts, note="NULL R with t")
            elif var == 1:
                j = Job(XYZ, src, None, None, note="NULL R and NULL t")
            elif var == 2:
                j = Job(XYZ, src, rc.R, t, about_origin=True, R_row_stride=rs, t_stride=ts, note=f"about origin, {rc.name}")
            elif var == 3:
                j = Job(XYZ, src, rc.R, None, about_origin=True, R_row_stride=rs, note=f"about origin, no t, {rc.name}")
            elif var == 4:
                j = Job(XYZ, src, rc.R, None, R_row_stride=rs, note=f"no t, {rc.name}")
            else:
                j = Job(XYZ, src, rc.R, t, R_row_stride=rs, t_stride=ts, note=rc.name)
        elif kinds[k] == ROT:
            j = Job(ROT, quats(n, seed=s), rc.R, None, R_row_stride=rs, note=rc.name)
        else:
            j = Job(SH, coefficients(n, (3, 8, 15)[(k + o_var) % 3], seed=s), rc.R, None, R_row_stride=rs, note=rc.name)
        j.in_place = in_place
        jobs.append(j)
    return jobs


def hostile_rows(n, width, seed=0):
    x = np.random.default_rng(seed).normal(size=(n, width)).astype(np.float32)
    x[0::3, 0] = np.nan
    x[1::3, -1] = np.inf
    x[2::3, 1 % width] = -np.inf
    return x


def job_tables():
    """name -> jobs of one pgr_pose_objects call.  POSE_JOBS_PER_LAUNCH = 16: 17, 33 and 48 jobs reach the second and third
    launch's workspace segment and first_block table."""
    tables = {
        "1": job_table(1, 1),
        "15": job_table(15, 2),
        "16": job_table(16, 3, empty=(15,)),                                   # empty last
        "17": job_table(17, 4, empty=(0,)),                                    # empty first; the 17th job alone in its launch
        "32": job_table(32, 5, empty=(7, 8, 20)),                              # empty in the middle
        "33": job_table(33, 6, empty=(16, 32)),                                # a launch's first job and the call's last
        "48": job_table(48, 7, empty=tuple(range(16, 32))),                    # the second launch entirely empty
    }
    # one job of NaN / Inf rows per kind among ordinary ones: the neighbours' rows must not notice
    t15 = tables["15"]
    R = rotation_cases()[-1].R
    t15[4] = Job(XYZ, hostile_rows(300, 3, 1), R, np.ones(3, np.float32), hostile=True, note="NaN/Inf rows")
    t15[9] = Job(ROT, hostile_rows(300, 4, 2), R, None, hostile=True, note="NaN/Inf rows")
    t15[12] = Job(SH, hostile_rows(300, 45, 3).reshape(300, 15, 3), R, None, hostile=True, note="NaN/Inf rows")
    return tables


# ---- the POSED branch of the preprocess: per-view pose tables inside forward_views(..., posed=...) -------------------------

POSED_EDGE = ("180x", "180y", "180z", "180_110", "180_111", "180_011", "180_101", "90x", "90y", "90z", "120_111",
              "180-1e-3_x", "180-1e-3_y", "180-1e-3_z", "180-1e-6_x", "180-1e-6_y", "180-1e-6_z", "angle_1e-8",
              "accumulated_1000", "identity", "random_0", "random_1", "random_2", "random_3")


@dataclass
class PosedCase:
    """A merged scene whose rows carry object ids (0 = environment, never posed), three views and one [K,20] pose table per
    view (compose.pose_table rows), filled from the edge rotations above so that every view poses with half turns and every
    branch case.  ``parts``: id -> (row indices, float32 centre)."""
    act: dict
    object_id: np.ndarray
    views: list
    tables: np.ndarray                                   # [3, K, 20] float32
    parts: dict
    poses: list                                          # per view: {id: (R float32 [3,3], t float32 [3])}


def posed_case(K, seed=3):
    """K = 1: one object (id 1) among rows of id 0.  K = 300: the scene's 8 objects cut into 18 parts each, with the ODD ids
    1, 3, ... 287 (even ids and 289..300 have table rows but no Gaussian: ids that skip values).

    Shares measured on the CPU with the oracle alone (tests/test_pose_host.py asserts them: ambig <= 1 %, content >= 20 %):
      K = 1:    ambig 0 / 0 / 0 % of the pixels per view, content (color > 0.05) 46.0 / 53.6 / 64.4 % of the values
      K = 300:  ambig 0 / 0 / 0 %, content 54.9 / 55.2 / 65.6 %"""
    from pegasus_amd import scenes
    from pegasus_amd.compose import pose_table
    assert K in (1, 300)
    cloud, views = scenes.scene_c3(seed=seed, scale=0.01, n_views=3, width=320, height=240)
    act = cloud.activated()
    oid = np.asarray(cloud.object_id).astype(np.int32)
    if K == 1:
        ids = np.where(oid == 1, 1, 0).astype(np.int32)
    else:
        rank = np.zeros_like(oid)
        for k in range(1, int(oid.max()) + 1):
            sel = np.nonzero(oid == k)[0]
            rank[sel] = np.arange(len(sel)) % 18
        ids = np.where(oid > 0, 2 * ((oid - 1) * 18 + rank) + 1, 0).astype(np.int32)
        assert ids.max() == 287
    parts = {}
    for k in np.unique(ids[ids > 0]):
        sel = np.nonzero(ids == k)[0]
        parts[int(k)] = (sel, act["means3d"][sel].astype(np.float64).mean(0).astype(np.float32))
    rots = {c.name: c.R for c in rotation_cases()}
    rng = np.random.default_rng(500 + K)
    tables, poses = [], []
    for v in range(3):
        rows, per_id = [], {}
        for k in range(1, K + 1):
            R = rots[POSED_EDGE[(k // 2 + 3 * v) % len(POSED_EDGE)]]           # (k // 2: the odd ids walk the whole list)
            t = rng.normal(0, 0.02, 3).astype(np.float32)
            T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
            center = parts[k][1] if k in parts else np.zeros(3, np.float32)
            rows.append((T, center))
            per_id[k] = (R, t)
        tables.append(pose_table(rows))
        poses.append(per_id)
    return PosedCase(act, ids, list(views), np.stack(tables).astype(np.float32), parts, poses)
