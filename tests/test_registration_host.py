"""Registration without a device: the new entries are declared, exported and prototyped and decide their arguments on the host;
the float64 reference (tests/registration_reference.py) against hand-worked answers, against scipy's k-d tree and against the
known pose of the ICP cases; the margin census; the tolerance on the final transformation measured again; the host-side
updates, Kabsch-Umeyama and the argument checks of pegasus_amd/registration.py."""
import ctypes as C
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))

import registration_cases as RC          # noqa: E402
import registration_reference as RR      # noqa: E402
from pegasus_amd import registration     # noqa: E402  (without the feature nothing in this file runs)

NAMES = ("pgr_nn_grid_build_workspace_bytes", "pgr_nn_grid_build", "pgr_nn_source_order_workspace_bytes", "pgr_nn_source_order",
         "pgr_nn_correspond", "pgr_icp_sums_workspace_bytes", "pgr_icp_sums", "pgr_radius_normals_workspace_bytes",
         "pgr_radius_normals")
FAKE = 0x10000                           # a non-NULL, 16-byte aligned address that is never dereferenced on the host
EYE = (C.c_double * 16)(*np.eye(4).reshape(-1))


@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import _lib, build
    build.build()
    return _lib.lib()


def _matrix(values):
    return (C.c_double * 16)(*np.asarray(values, dtype=np.float64).reshape(-1))


# ---- the entries
def test_symbols_are_declared_exported_and_prototyped(lib):
    from pegasus_amd import _lib
    header = (ROOT / "include" / "pegasus_raster.h").read_text()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        if name.endswith("_workspace_bytes"):
            assert _lib.SYMBOLS[name] == (C.c_size_t, [C.c_int32])
    assert lib.pgr_abi_version() == 4
    assert int(re.search(r"#define PGR_ICP_SUMS (\d+)", header).group(1)) == registration.SUMS == RR.SUMS
    assert (registration.JTJ, registration.JTR, registration.COUNT, registration.D2, registration.SUM_S, registration.SUM_Q,
            registration.SUM_SQ, registration.SUM_SS) == (RR.JTJ, RR.JTR, RR.COUNT, RR.D2, RR.SUM_S, RR.SUM_Q, RR.SUM_SQ, RR.SUM_SS)
    for what in (registration.PLANE_SLICE, registration.POINT_SLICE):
        assert what.stop - what.start == 32 and what.start <= RR.COUNT and RR.D2 < what.stop
    assert registration.PLANE_SLICE.start == RR.JTJ and registration.PLANE_SLICE.stop >= RR.JTR + 6
    assert registration.POINT_SLICE.stop > RR.SUM_SS


def test_workspace_sizes(lib):
    for name in NAMES:
        if not name.endswith("_workspace_bytes"):
            continue
        size = getattr(lib, name)
        assert size(-1) == 0 and size(-(1 << 31)) == 0 and size(1) > 0
        sizes = [size(n) for n in (0, 1, 255, 256, 257, 4099, 65537, 2_000_000, (1 << 31) - 1)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (name, sizes)
        assert all(s % 256 == 0 for s in sizes)
    assert lib.pgr_nn_grid_build_workspace_bytes(4099) == lib.pgr_radius_count_workspace_bytes(4099)      # the same grid
    assert lib.pgr_icp_sums_workspace_bytes(2_000_000) <= 2_000_000 // 256 * 48 * 8 + 48 * 8 + 256


def _calls(lib):
    """name -> a call with good arguments except for the keywords given."""
    def grid(n=4, xyz=FAKE, d=0.01, ws=FAKE, ws_bytes=None):
        return lib.pgr_nn_grid_build(n, xyz, d, ws, lib.pgr_nn_grid_build_workspace_bytes(max(n, 0)) if ws_bytes is None else ws_bytes, None)

    def order(n=4, xyz=FAKE, T=EYE, d=0.01, out=FAKE, ws=FAKE, ws_bytes=None):
        return lib.pgr_nn_source_order(n, xyz, T, d, out, ws,
                                       lib.pgr_nn_source_order_workspace_bytes(max(n, 0)) if ws_bytes is None else ws_bytes, None)

    def correspond(n=4, xyz=FAKE, T=EYE, nt=4, d=0.01, ws=FAKE, ws_bytes=None, index=FAKE, d2=FAKE):
        return lib.pgr_nn_correspond(n, xyz, None, T, nt, d, ws,
                                     lib.pgr_nn_grid_build_workspace_bytes(max(nt, 0)) if ws_bytes is None else ws_bytes, index, d2,
                                     None)

    def sums(n=4, xyz=FAKE, T=EYE, index=FAKE, d2=FAKE, nt=4, tgt=FAKE, out=FAKE, ws=FAKE, ws_bytes=None):
        return lib.pgr_icp_sums(n, xyz, T, index, d2, nt, tgt, None, out, ws,
                                lib.pgr_icp_sums_workspace_bytes(max(n, 0)) if ws_bytes is None else ws_bytes, None)

    def normals(n=4, xyz=FAKE, d=0.01, out=FAKE, counts=FAKE, ws=FAKE, ws_bytes=None):
        return lib.pgr_radius_normals(n, xyz, d, out, counts, ws,
                                      lib.pgr_radius_normals_workspace_bytes(max(n, 0)) if ws_bytes is None else ws_bytes, None)
    return dict(grid=grid, order=order, correspond=correspond, sums=sums, normals=normals)


def test_invalid_arguments_are_refused_before_any_launch(lib):
    from pegasus_amd import _lib
    bad = _lib.PGR_ERR_INVALID_ARGUMENT
    call = _calls(lib)
    for name, fn in call.items():
        assert fn(n=-1) == bad, name
        assert fn(xyz=None) == bad, name
        if name != "correspond":
            assert fn(ws=None) == bad and fn(ws=FAKE + 8) == bad, name
        if name != "sums":
            for d in (0.0, -0.01, math.nan, math.inf, -math.inf):
                assert fn(d=d) == bad, (name, d)
                assert fn(n=0, d=d) == bad, (name, d)
    not_finite = np.eye(4)
    not_finite[1, 3] = np.nan
    for name in ("order", "correspond", "sums"):
        assert call[name](T=None) == bad, name
        assert call[name](T=_matrix(not_finite)) == bad, name
        assert call[name](n=0, T=None) == bad, name
    assert call["order"](out=None) == bad
    assert call["correspond"](nt=-1) == bad and call["correspond"](index=None) == bad and call["correspond"](d2=None) == bad
    assert call["correspond"](ws=None) == bad and call["correspond"](ws=FAKE + 8) == bad
    assert call["sums"](nt=-1) == bad and call["sums"](index=None) == bad and call["sums"](d2=None) == bad
    assert call["sums"](tgt=None) == bad and call["sums"](out=None) == bad
    assert call["normals"](out=None) == bad and call["normals"](counts=None) == bad


def test_short_workspaces_are_refused_and_no_points_are_ok(lib):
    from pegasus_amd import _lib
    call = _calls(lib)
    sizes = dict(grid=lib.pgr_nn_grid_build_workspace_bytes, order=lib.pgr_nn_source_order_workspace_bytes,
                 sums=lib.pgr_icp_sums_workspace_bytes, normals=lib.pgr_radius_normals_workspace_bytes)
    for name, size in sizes.items():
        for n in (1, 257, 4099):
            assert call[name](n=n, ws_bytes=size(n) - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL, (name, n)
            assert call[name](n=n, ws_bytes=0) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL, (name, n)
    for nt in (1, 4099):
        assert call["correspond"](nt=nt, ws_bytes=lib.pgr_nn_grid_build_workspace_bytes(nt) - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert call["grid"](n=0, xyz=None, ws=None, ws_bytes=0) == _lib.PGR_OK
    assert call["order"](n=0, xyz=None, out=None, ws=None, ws_bytes=0) == _lib.PGR_OK
    assert call["correspond"](n=0, xyz=None, ws=None, ws_bytes=0, index=None, d2=None) == _lib.PGR_OK
    assert call["normals"](n=0, xyz=None, out=None, counts=None, ws=None, ws_bytes=0) == _lib.PGR_OK


# ---- the package's argument checks
def test_python_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    pts = torch.zeros((4, 3))
    for fn, args in ((registration.estimate_normals, (pts, 0.01)), (registration.nearest_neighbors, (pts, pts, 0.01)),
                     (registration.evaluate_registration, (pts, pts, 0.01)),
                     (registration.registration_icp, (pts, pts, 0.01, None, "point_to_point"))):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            fn(*args)
    for bad in (pts.double(), pts[:, :2], pts.reshape(-1), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError):
            registration.estimate_normals(bad, 0.01)
        with pytest.raises(ValueError):
            registration.nearest_neighbors(bad, pts, 0.01)
        with pytest.raises(ValueError):
            registration.nearest_neighbors(pts, bad, 0.01)
    for radius in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            registration.estimate_normals(pts, radius)
    with pytest.raises(ValueError, match="estimation"):
        registration.registration_icp(pts, pts, 0.01, estimation="colored")
    with pytest.raises(ValueError, match="max_iteration"):
        registration.registration_icp(pts, pts, 0.01, estimation="point_to_point", max_iteration=-1)
    with pytest.raises(ValueError, match="normals_radius"):
        registration.registration_icp(pts, pts, 0.01)
    with pytest.raises(ValueError, match="4x4"):
        registration.nearest_neighbors(pts, pts, 0.01, np.eye(3))
    with pytest.raises(ValueError, match="finite"):
        registration.nearest_neighbors(pts, pts, 0.01, np.full((4, 4), np.nan))


def test_a_pose_that_is_not_rigid_is_refused():
    T = RC.rigid((10.0, -20.0, 30.0), (0.1, 0.2, 0.3))
    assert np.array_equal(registration._rigid(T), T)
    scaled = T.copy()
    scaled[:3, :3] *= 1.02
    with pytest.raises(ValueError, match="scale 1.02"):
        registration.register_models(None, None, scaled)
    with pytest.raises(ValueError, match="not a rotation"):
        registration.merge_models(None, None, np.diag([1.0, 1.0, -1.0, 1.0]))
    sheared = T.copy()
    sheared[0, 1] += 0.01
    with pytest.raises(ValueError, match="not a rotation"):
        registration.register_models(None, None, sheared)


def test_command_line_arguments():
    p = registration._parser()
    a = p.parse_args(["--target", "up.ply", "--source", "down.ply", "--init", "T.txt", "--out", "fused.ply"])
    assert (a.max_distance, a.normals_radius, a.estimation, a.max_iteration, a.min_opacity, a.drop_within) == \
        (0.02, None, "point_to_plane", 30, 0.5, None)
    for argv in (["--target", "a", "--source", "b", "--out", "c"],
                 ["--target", "a", "--source", "b", "--out", "c", "--points_target", "p"],
                 ["--target", "a", "--source", "b", "--out", "c", "--init", "T", "--points_target", "p", "--points_source", "q"]):
        with pytest.raises(SystemExit):
            registration.main(argv)


# ---- the updates
@pytest.mark.parametrize("vec6", [registration.vec6_to_matrix, RR.vec6_to_matrix])
def test_vec6_to_matrix_on_hand_worked_cases(vec6):
    h = math.pi / 2
    cases = [((h, 0, 0, 1, 2, 3), [[1, 0, 0], [0, 0, -1], [0, 1, 0]]),                   # Rx
             ((0, h, 0, 0, 0, 0), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]),                   # Ry
             ((0, 0, h, 0, 0, 0), [[0, -1, 0], [1, 0, 0], [0, 0, 1]]),                   # Rz
             ((h, h, 0, 0, 0, 0), [[0, 1, 0], [0, 0, -1], [-1, 0, 0]]),                  # Ry Rx, not Rx Ry
             ((h, h, h, -1, 0, 5), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]])]                  # Rz Ry Rx
    for x, R in cases:
        T = np.asarray(vec6(x), dtype=np.float64)
        assert T.shape == (4, 4) and np.abs(T[:3, :3] - np.array(R)).max() < 1e-15, x
        assert T[:3, 3].tolist() == [float(v) for v in x[3:]] and T[3].tolist() == [0, 0, 0, 1]
    x = (0.3, -0.2, 0.5, 0.01, 0.02, -0.03)
    assert np.abs(registration.vec6_to_matrix(x) - RR.vec6_to_matrix(x)).max() < 1e-15


def test_updates_equal_the_references_and_refuse_what_cannot_be_solved():
    ev = RC.reference_evaluation("small")
    assert np.abs(registration.point_to_plane_update(ev.sums) - RR.plane_update(ev.sums)).max() < 1e-12
    assert np.abs(registration.point_to_point_update(ev.sums) - RR.point_update(ev.sums)).max() < 1e-12
    assert np.abs(RR.plane_update(ev.sums) - np.eye(4)).max() > 1e-4 and np.abs(RR.point_update(ev.sums) - np.eye(4)).max() > 1e-4
    assert np.abs(RR.point_update(ev.sums.astype(np.longdouble), np.longdouble) - RR.point_update(ev.sums)).max() < 1e-13
    for plane, point in ((registration.point_to_plane_update, registration.point_to_point_update), (RR.plane_update, RR.point_update)):
        few = ev.sums.copy()
        few[RR.COUNT] = 5
        assert np.array_equal(plane(few), np.eye(4))
        few[RR.COUNT] = 2
        assert np.array_equal(point(few), np.eye(4))
        assert np.array_equal(plane(np.zeros(RR.SUMS)), np.eye(4)) and np.array_equal(point(np.zeros(RR.SUMS)), np.eye(4))
    # all points on the plane z = 0.02 with the normal (0, 0, 1): J = (y, -x, 0, 0, 0, 1) spans two dimensions of six
    rng = np.random.default_rng(3)
    flat = np.concatenate([rng.uniform(-0.05, 0.05, (50, 2)), np.full((50, 1), 0.02)], axis=1).astype(np.float32)
    up = np.tile([0.0, 0.0, 1.0], (50, 1))
    lifted = flat + np.array([0, 0, 0.001], dtype=np.float32)
    v, _ = RR.sums(lifted, flat, up, np.eye(4), np.arange(50), np.full(50, 1e-6))
    assert v[RR.COUNT] == 50 and abs(v[RR.JTR + 5]) > 1e-3
    assert np.array_equal(RR.plane_update(v), np.eye(4)) and np.array_equal(registration.point_to_plane_update(v), np.eye(4))
    # all points on one line: the cross-covariance has rank 1
    line = (np.linspace(-1, 1, 20)[:, None] * np.array([[0.03, 0.01, -0.02]])).astype(np.float32)
    v, _ = RR.sums(line, line, None, np.eye(4), np.arange(20), np.zeros(20))
    assert np.array_equal(RR.point_update(v), np.eye(4)) and np.array_equal(registration.point_to_point_update(v), np.eye(4))


# ---- Kabsch-Umeyama
def test_kabsch_umeyama_recovers_a_similarity_and_never_reflects():
    rng = np.random.default_rng(8)
    B = rng.normal(size=(12, 3))
    T = RC.rigid((25.0, -40.0, 70.0), (0.3, -1.2, 2.0))
    for scale in (1.0, 0.37, 2.5):
        A = scale * B @ T[:3, :3].T + T[:3, 3]
        R, c, t = registration.kabsch_umeyama(A, B)
        assert R.shape == (3, 3) and np.ndim(c) == 0 and t.shape == (3,)
        assert np.abs(R - T[:3, :3]).max() < 1e-13 and abs(c - scale) < 1e-13 and np.abs(t - T[:3, 3]).max() < 1e-13
        a, moved, (R2, c2, t2) = registration.align_point_set(A, B)
        assert a is A and moved.shape == B.shape and np.abs(moved - A).max() < 1e-12
        assert np.array_equal(R2, R) and c2 == c and np.array_equal(t2, t)
    # a mirror image: the best orthogonal fit is a reflection, the answer is the best ROTATION
    mirrored = B * np.array([1.0, 1.0, -1.0])
    R, c, t = registration.kabsch_umeyama(mirrored, B)
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and c > 0
    U, _, Vt = np.linalg.svd((mirrored - mirrored.mean(0)).T @ (B - B.mean(0)))
    assert np.linalg.det(U @ Vt) < 0
    with pytest.raises(ValueError):
        registration.kabsch_umeyama(B, B[:5])
    planar = [[0, 0], [1, 0], [0, 2.0]]
    R, c, t = registration.kabsch_umeyama(planar, planar)
    assert R.shape == (2, 2) and t.shape == (2,) and abs(c - 1) < 1e-15


# ---- the reference
def test_reference_on_hand_worked_neighbours():
    source, target, distance = RC.tie_345()
    assert distance * distance == 25 * 2.0 ** -14                                  # d2 and the threshold are one float64
    assert RR.nearest(source, target, distance).index.tolist() == [-1]
    nb = RR.nearest(source, target, float(np.nextafter(distance, np.inf)))
    assert nb.index.tolist() == [0] and nb.d2.tolist() == [25 * 2.0 ** -14]
    source, target, distance = RC.equidistant()
    assert RR.nearest(source, target, distance).index.tolist() == [0]
    assert RR.nearest(source, target[[1, 0, 2]], distance).index.tolist() == [0]
    assert RR.nearest(source, target[[2, 1, 0]], distance).index.tolist() == [1]
    assert RR.nearest(source, RC.coincident(300), 1e-3, RC.rigid((0, 0, 0), (0.1, -0.2, 0.3))).index.tolist() == [-1]
    assert RR.nearest(RC.coincident(2), RC.coincident(300), 1e-3).index.tolist() == [0, 0]
    moved = RR.pose(np.array([[1, 2, 3]], dtype=np.float32), [[0, -1, 0, 0.5], [1, 0, 0, 0.25], [0, 0, 1, -1], [0, 0, 0, 1]])
    assert moved.tolist() == [[-1.5, 1.25, 2.0]]


@pytest.mark.parametrize("ns,nt", [(257, 4099), (4099, 4099)])
def test_reference_equals_scipy_nearest_neighbour(ns, nt):
    from scipy.spatial import cKDTree
    source, target = RC.pair(ns, nt)
    nb = RC.reference_pair(ns, nt)
    assert nb.distance_margin > RC.DISTANCE_MARGIN_MIN and nb.gap_margin > RC.DISTANCE_MARGIN_MIN
    d, j = cKDTree(target.astype(np.float64)).query(RR.pose(source, RC.POSE_NEAR), distance_upper_bound=RC.MAX_DISTANCE)
    want = np.where(np.isfinite(d), j, -1)
    assert np.array_equal(nb.index, want) and 0 < (want >= 0).sum() < ns
    assert np.abs(np.sqrt(nb.d2[want >= 0]) - d[want >= 0]).max() < 1e-15


def test_reference_normals_on_a_plane_and_a_lonely_point():
    pts, n = RC.planar_patch()
    got, counts, ratio = RR.normals(pts, 0.01)
    assert counts.min() >= 3 and (np.abs(got @ n) > 1 - 1e-9).all() and (got[:, 0] > 0).all()       # +n: its x leads, (2,-1,2)/3
    lonely = np.vstack([pts, [[5.0, 5.0, 5.0]]]).astype(np.float32)
    got, counts, ratio = RR.normals(lonely, 0.01)
    assert counts[-1] == 1 and got[-1].tolist() == [0.0, 0.0, 1.0] and ratio[-1] == np.inf


@pytest.mark.parametrize("name", sorted(RC.ICP_CASES))
def test_reference_recovers_the_known_pose(name):
    """Point to plane, the default and what the cases were designed on.  (Point to point on disjoint samples of two halves
    settles about 0.9 degrees and 1.2 mm away at either size; it is held to the reference's result, not to the known pose.)"""
    n, counts, ratio = RC.target_normals(name)
    print(name, "neighbours >=", counts.min(), "eigen-gap ratio >=", ratio.min())
    assert counts.min() >= 3 and ratio.min() > RC.EIGEN_GAP_MIN
    got = RC.reference_icp(name, "point_to_plane")
    T = got.transformation
    deg = RR.rotation_angle_deg(T[:3, :3], RC.KNOWN_POSE[:3, :3])
    metres = float(np.linalg.norm(T[:3, 3] - RC.KNOWN_POSE[:3, 3]))
    print(name, "iterations", got.iterations, "fitness", got.fitness, "rmse", got.rmse, "rotation error", deg, "deg, translation error",
          metres, "m; margins", got.distance_margin, got.gap_margin)
    assert deg < RC.POSE_DEG_MAX and metres < RC.POSE_M_MAX
    assert 1 <= got.iterations < 30                                                # the stopping rule was met
    assert got.distance_margin > RC.DISTANCE_MARGIN_MIN and got.gap_margin > RC.DISTANCE_MARGIN_MIN


@pytest.mark.parametrize("estimation", RC.ESTIMATIONS)
def test_transformation_tolerance_is_the_references_own_error(estimation):
    a = RC.reference_icp("small", estimation)
    b = RC.reference_icp("small", estimation, "longdouble")
    assert b.transformation.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
    assert a.iterations == b.iterations and np.array_equal(a.index, b.index) and a.fitness == b.fitness
    assert a.distance_margin > RC.DISTANCE_MARGIN_MIN and a.gap_margin > RC.DISTANCE_MARGIN_MIN
    diff = float(np.abs(b.transformation - a.transformation.astype(np.longdouble)).max())
    print(estimation, "largest |T longdouble - T float64| =", diff, "recorded", RC.T_TOL_MEASURED[("small", estimation)])
    assert 100 * diff <= RC.T_TOL
    assert RC.T_TOL == max(1e-13, 100 * max(RC.T_TOL_MEASURED.values())) and RC.T_TOL < 1e-12
