"""Inputs of the registration tests (tests/test_registration_host.py, tests/test_registration_gpu.py), all seeded, and their
reference results, computed once per process (tests/registration_reference.py) and handed out read-only.

The floors.  A random case is valid only if no decision of it sits near a tie:
  DISTANCE_MARGIN_MIN  coordinates are <= 0.1 m, where a float64 ulp is 1.4e-17; a few hundred operations and iterations stay
                       below 1e-13, which leaves 100 x headroom under 1e-11 m.  Held by |d - max_distance| of every source
                       point and by the gap between the nearest and the second nearest target of every accepted one.
  EIGEN_GAP_MIN        a normal is compared only where (l1 - l0) / l2 of its covariance exceeds it: the eigenvector's
                       condition is the reciprocal of that gap.
The tolerance on ICP's final transformation, T_TOL, is the reference's own error: 100 x the largest element-wise difference
between its run in numpy.longdouble and its run in float64 over the ICP cases below (both estimators), floor 1e-13.  Measured:
see T_TOL_MEASURED; tests/test_registration_host.py::test_transformation_tolerance_is_the_references_own_error measures the
small case again."""
import functools

import numpy as np

import registration_reference as RR

DISTANCE_MARGIN_MIN = 1e-11
EIGEN_GAP_MIN = 0.05
SIZES = (1, 255, 256, 257, 4099)
SUM_SIZES = (1, 257, 4099)
MAX_DISTANCE = 0.01
# largest |T_longdouble - T_float64| over {small, large} x {point_to_plane, point_to_point}: see the module docstring
T_TOL_MEASURED = {("small", "point_to_plane"): 1.6e-16, ("small", "point_to_point"): 1.8e-15,
                  ("large", "point_to_plane"): 1.1e-16, ("large", "point_to_point"): 1.8e-15}
T_TOL = max(1e-13, 100 * max(T_TOL_MEASURED.values()))                       # 1.8e-13
POSE_DEG_MAX, POSE_M_MAX = 0.5, 0.5e-3                  # how near the reference itself must come to the known pose
ICP_CASES = {"small": (4000, 0.012), "large": (20000, 0.006)}      # name -> (points drawn per scan, normals radius)
ESTIMATIONS = ("point_to_plane", "point_to_point")


def _frozen(a):
    a.setflags(write=False)
    return a


def rigid(rotvec_deg, translation):
    """4x4 float64 from a rotation vector in degrees (Rodrigues) and a translation."""
    v = np.radians(np.asarray(rotvec_deg, dtype=np.float64))
    angle = np.linalg.norm(v)
    T = np.eye(4)
    if angle > 0:
        k = v / angle
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    T[:3, 3] = translation
    return T


def bumpy_surface(count, seed):
    """``count`` points on a bumpy closed surface of about 0.1 m without any symmetry: a sphere of radius 0.05 m whose radius
    varies by up to +-50 % with direction, stretched along x, squeezed along y and shifted; float64."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x, y, z = d.T
    r = 0.05 * (1.0 + 0.20 * np.sin(5.0 * x + 1.0) * np.cos(4.0 * y) + 0.16 * np.cos(6.0 * z + 2.0 * x) + 0.14 * x * y
                + 0.12 * np.sin(7.0 * y - 3.0 * z + 0.5))
    return d * r[:, None] * np.array([1.3, 0.8, 1.0]) + np.array([0.004, -0.003, 0.002])


KNOWN_POSE = _frozen(rigid((1.8, -1.5, 1.9), (0.003, -0.002, 0.0025)))       # 3.0 degrees, (3, -2, 2.5) mm


@functools.lru_cache(maxsize=None)
def scans(name):
    """(source float32 [Ns,3], target float32 [Nt,3]) of an ICP case: the target is the top of the object (z > -0.03 m), the
    source its bottom (z < 0.03 m) from ANOTHER random sample, moved by the inverse of KNOWN_POSE -- the transformation that
    registers the source to the target is KNOWN_POSE (up to the float32 rounding of the moved points)."""
    count, _ = ICP_CASES[name]
    top, bottom = bumpy_surface(count, 1000 + count), bumpy_surface(count, 2000 + count)
    top, bottom = top[top[:, 2] > -0.03], bottom[bottom[:, 2] < 0.03]
    inv = np.linalg.inv(KNOWN_POSE)
    moved = bottom @ inv[:3, :3].T + inv[:3, 3]
    return _frozen(moved.astype(np.float32)), _frozen(top.astype(np.float32))


@functools.lru_cache(maxsize=None)
def target_normals(name):
    """(normals, counts, gap ratio) of an ICP case's target at its normals radius."""
    return tuple(_frozen(a) for a in RR.normals(scans(name)[1], ICP_CASES[name][1]))


@functools.lru_cache(maxsize=None)
def reference_icp(name, estimation, dtype="float64"):
    source, target = scans(name)
    return RR.icp(source, target, MAX_DISTANCE, None, estimation, target_normals(name)[0], dtype=getattr(np, dtype))


@functools.lru_cache(maxsize=None)
def reference_evaluation(name, with_normals=True):
    """The reference's evaluation of an ICP case at POSE_NEAR (with every sum)."""
    source, target = scans(name)
    return RR.evaluate(source, target, MAX_DISTANCE, POSE_NEAR, target_normals(name)[0] if with_normals else None)


POSE_NEAR = _frozen(rigid((0.7, 1.1, -0.9), (0.001, 0.0015, -0.0008)))       # a non-trivial pose for single evaluations


@functools.lru_cache(maxsize=None)
def pair(ns, nt):
    """The first ``ns`` rows of the small case's source against the first ``nt`` rows of its target (the generator's rows are
    in random order, so any prefix covers the object)."""
    source, target = scans("small")
    source, target = np.tile(source, (2, 1)), np.tile(target, (2, 1))           # 4099 > one scan
    jitter = np.random.default_rng(ns * 7919 + nt).normal(0.0, 1e-4, (len(source), 3)).astype(np.float32)
    return _frozen(np.ascontiguousarray(source[:ns] + jitter[:ns])), _frozen(np.ascontiguousarray(target[:nt] - jitter[:nt]))


@functools.lru_cache(maxsize=None)
def reference_pair(ns, nt):
    source, target = pair(ns, nt)
    return RR.nearest(source, target, MAX_DISTANCE, POSE_NEAR)


def tie_345():
    """A source point and a target point exactly 5 * 2^-7 apart (every product and sum exact) and that distance."""
    return (np.array([[0, 0, 0]], dtype=np.float32), np.array([[3 * 2.0 ** -7, 4 * 2.0 ** -7, 0]], dtype=np.float32),
            5 * 2.0 ** -7)


def equidistant():
    """A source point midway between two targets (every coordinate a small dyadic number: both d2 are the same float64), with a
    farther third target; and the distance to search within."""
    source = np.array([[0.25, 0.5, -0.125]], dtype=np.float32)
    target = np.array([[0.25 + 2.0 ** -6, 0.5, -0.125], [0.25 - 2.0 ** -6, 0.5, -0.125], [0.25, 0.5 + 2.0 ** -5, -0.125]],
                      dtype=np.float32)
    return source, target, 2.0 ** -4


R_LATTICE = 2.0 ** -5


def lattice(side, spacing, centre):
    """side^3 float32 points at centre + spacing * (i, j, k), the indices centred on 0 (exact in float32 around the origin,
    rounded to float32 far from it)."""
    k = np.arange(-(side // 2), side - side // 2, dtype=np.float64) * spacing
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(centre, dtype=np.float64)
    return g.astype(np.float32)


def wall_lattice(centre, hair):
    """(source, target, max_distance): a source lattice of spacing 2a and the target lattice offset from it by a along x, with
    a = R_LATTICE (1 - hair): every source point has a target a hair inside max_distance = R_LATTICE on either side, most of
    them in another cell (the cell edge is 1.0001 R_LATTICE).  Around the origin every coordinate is exact in float32 and the
    two are exactly equidistant."""
    a = R_LATTICE * (1.0 - hair)
    source = lattice(5, 2 * a, centre)
    target = lattice(6, 2 * a, np.asarray(centre, dtype=np.float64) + (a, 0.0, 0.0))
    return source, target, R_LATTICE


def lattice_centres():
    """[(centre, hair)]: the origin (cell walls and negative coordinates around 0), a negative and a large centre; the hair is a
    few float32 ulps of the coordinates there."""
    return [((0.0, 0.0, 0.0), 2.0 ** -20), ((-37.3 * R_LATTICE, -5.1 * R_LATTICE, -1001.7 * R_LATTICE), 2.0 ** -12),
            ((3000.2 * R_LATTICE, -70001.4 * R_LATTICE, 12.9 * R_LATTICE), 2.0 ** -6)]


def coincident(count=300):
    return np.tile(np.array([[0.1, -0.2, 0.3]], dtype=np.float32), (count, 1))


def planar_patch(count=600, seed=5):
    """Points on the plane through (0.02, -0.01, 0.03) with the normal (2, -1, 2) / 3, within 0.02 m of that point; float32
    (so only near the plane) and the unit normal."""
    rng = np.random.default_rng(seed)
    n = np.array([2.0, -1.0, 2.0]) / 3.0
    u = np.cross(n, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    ab = rng.uniform(-0.02, 0.02, (count, 2))
    pts = np.array([0.02, -0.01, 0.03]) + ab[:, :1] * u + ab[:, 1:] * v
    return pts.astype(np.float32), n
