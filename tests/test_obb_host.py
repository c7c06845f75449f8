"""What the minimal-oriented-box work promises without a GPU: the reference of tests/obb_reference.py holds the properties of
a minimal box on scipy hulls, the corner orders are open3d's and NDDS's, scene_gt_entry takes the third tuple element, both
entries refuse bad arguments before touching a device, and the command lines name what they miss."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import obb_cases as OC                   # noqa: E402
import obb_reference as OR               # noqa: E402


# ---- the reference itself
@pytest.mark.parametrize("seed,n,offset", [(0, 40, (0, 0, 0)), (1, 300, (0, 0, 0)), (2, 120, tuple(OC.OFFSET))])
def test_reference_on_scipy_hulls(seed, n, offset):
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(seed)
    cloud = ((rng.normal(size=(n, 3)) * [0.3, 0.8, 1.0]) @ OC.rotation(seed + 30).T + np.asarray(offset)).astype(np.float32)
    hull = ConvexHull(cloud.astype(np.float64))
    index = np.full(n, -1)
    index[hull.vertices] = np.arange(len(hull.vertices))
    pts, tri = cloud[hull.vertices], index[hull.simplices]
    lohi, vol, q_bound = OR.candidates(pts, tri)
    b = OR.argmin_finite(vol)
    center, R, extent = OR.box(pts, tri[b], lohi[b])
    # rebuilding the centre, p - c and the dot product: 8 roundings on at most max |p|_1 (the cloud may sit far from the origin)
    tol = q_bound[b] + 8 * OR.EPS * np.abs(cloud.astype(np.float64)).sum(axis=1).max()
    assert OR.contains(center, R, extent, cloud, tol).all()                # every point, not only the hull's
    assert not OR.contains(center, R, extent * 0.99, cloud, tol).all()
    aabb = np.prod(cloud.astype(np.float64).max(0) - cloud.astype(np.float64).min(0))
    assert np.prod(extent) <= aabb
    assert (np.prod(extent) <= vol[np.isfinite(vol)]).all() and np.prod(extent) == vol[b]
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0


def test_reference_rules_for_ties_and_volumes_that_are_not_finite():
    assert OR.argmin_finite([np.nan, 3.0, -np.inf, 2.0, 2.0, np.inf]) == 3
    assert OR.argmin_finite([np.nan, np.inf, -np.inf]) == -1 and OR.argmin_finite([]) == -1
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    _, vol, _ = OR.candidates(pts, np.array([[1, 1, 3], [0, 1, 2], [0, 1, 3]]))
    assert not np.isfinite(vol[:2]).any() and vol[2] == 2.0
    pts[4, 2] = np.nan
    assert not np.isfinite(OR.candidates(pts, np.array([[0, 1, 3]]))[1]).any()
    assert OR.minimal_box(pts, np.array([[0, 1, 3]])) is None


def test_reference_diameter_keeps_the_lowest_pair():
    square = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]] * 3, np.float32)
    assert OR.diameter(square) == (2.0, (0, 2))
    assert OR.diameter(square[:1]) == (0.0, None)
    cloud = OC.ball_cloud(700, seed=9)
    d2, (i, j) = OR.diameter(cloud)
    p = cloud.astype(np.float64)
    full = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    assert i < j and full[i, j] == full.max() and abs(d2 - full.max()) <= OR.K_D2 * OR.EPS * d2


# ---- corner orders, worked by hand: the box [0,4] x [0,2] x [0,1], first triangle (0,0,0), (4,0,0), (0,2,0)
HAND_POINTS = np.array([[x, y, z] for x in (0, 4) for y in (0, 2) for z in (0, 1)], np.float32)
HAND_TRIANGLE = (0, 4, 2)                # u = +x, w = u x v0 = +z, v = w x u = +y: R is the identity, centre (2, 1, 0.5)
HAND_BOX_POINTS = [[0, 0, 0], [4, 0, 0], [0, 2, 0], [0, 0, 1], [4, 2, 1], [0, 2, 1], [4, 0, 1], [4, 2, 0]]
HAND_NDDS = [[0, 0, 0], [0, 2, 0], [0, 2, 1], [0, 0, 1], [4, 0, 0], [4, 2, 0], [4, 2, 1], [4, 0, 1]]


def test_corner_orders_by_hand():
    from pegasus_amd import obb
    lohi, vol, _ = OR.candidates(HAND_POINTS, [HAND_TRIANGLE])
    assert lohi[0].tolist() == [0, 0, 0, 4, 2, 1] and vol[0] == 8.0
    center, R, extent = OR.box(HAND_POINTS, HAND_TRIANGLE, lohi[0])
    assert center.tolist() == [2, 1, 0.5] and np.array_equal(R, np.eye(3)) and extent.tolist() == [4, 2, 1]
    assert OR.box_points(center, R, extent).tolist() == HAND_BOX_POINTS
    assert OR.ndds_corners(center, R, extent).tolist() == HAND_NDDS
    box = obb.box_from_candidate(HAND_POINTS, HAND_TRIANGLE, lohi[0])
    assert box.box_points().tolist() == HAND_BOX_POINTS and box.ndds_corners().tolist() == HAND_NDDS
    assert box.volume == 8.0 and box.center.tolist() == [2, 1, 0.5]
    assert box.contains(HAND_POINTS).all() and not box.contains([[4.001, 1, 0.5]]).any() and box.contains([[4.001, 1, 0.5]], 0.01).all()
    assert obb.NDDS_ORDER == OR.NDDS_ORDER == (0, 2, 5, 3, 1, 7, 4, 6)


def test_a_turned_box_keeps_the_orders():
    from pegasus_amd import obb
    R0 = OC.rotation(3)
    pts = (HAND_POINTS.astype(np.float64) @ R0.T + [5, 6, 7]).astype(np.float32)
    lohi, _, _ = OR.candidates(pts, [HAND_TRIANGLE])
    want = np.array(HAND_NDDS, np.float64) @ R0.T + [5, 6, 7]
    # the float32 points lie within delta of the exact ones; u (length 4) turns by 2 delta / 4, w by 2 delta (1/4 + 1/2), v by
    # both; a face moves by delta and turns about a point at most the diagonal sqrt(21) away; three faces meet in a corner
    delta = 2.0 ** -24 * np.abs(want).sum(axis=1).max()
    tol = 3 * (2 * delta + (2 * delta / 4 + 2 * delta * 0.75) * np.sqrt(21.0))
    assert np.abs(obb.box_from_candidate(pts, HAND_TRIANGLE, lohi[0]).ndds_corners() - want).max() <= tol
    assert np.abs(OR.ndds_corners(*OR.box(pts, HAND_TRIANGLE, lohi[0])) - want).max() <= tol


# ---- scene_gt_entry
def test_scene_gt_entry_with_two_and_three_element_boxes():
    from pegasus_amd import bop_pose
    K = bop_pose.camera_K(0.9, 0.7, 640, 480)
    R_c2w, t_w2c = OC.rotation(1), np.array([0.1, -0.2, 3.0])
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = OC.rotation(2), [0.3, 0.2, 0.1]
    corners = np.array(HAND_NDDS, np.float64) * 0.1
    mean, center = np.array([0.21, 0.1, 0.05]), np.array([0.2, 0.1, 0.05])
    two = bop_pose.scene_gt_entry(R_c2w, t_w2c, {4: pose}, K=K, boxes={4: (corners, mean)})[0]
    three = bop_pose.scene_gt_entry(R_c2w, t_w2c, {4: pose}, K=K, boxes={4: (corners, mean, center)})[0]
    # what the writer gave before it took a third element: P = K @ T[:3] on homogeneous points, divided by the last row
    T = bop_pose.world_to_camera(R_c2w, t_w2c) @ pose
    P = K @ T[:3]

    def project(x):
        h = P @ np.append(x, 1.0)
        return [h[0] / h[2], h[1] / h[2]]
    assert two["3d_bounding_box_model_coord"] == corners.tolist() and two["3d_bounding_center"] == mean.tolist()
    assert np.allclose(two["projected_points"], [project(c) for c in corners], rtol=0, atol=1e-9)
    assert np.allclose(two["projected_center"], [project(mean)], rtol=0, atol=1e-9)
    assert two["projected_center"] == bop_pose.project_points(K, T, mean[None]).tolist()
    assert list(two) == list(three)
    for key in two:
        if key != "projected_center":
            assert two[key] == three[key], key
    assert three["projected_center"] == bop_pose.project_points(K, T, center[None]).tolist() != two["projected_center"]
    assert "projected_points" not in bop_pose.scene_gt_entry(R_c2w, t_w2c, {4: pose})[0]


# ---- the entries' argument checks: fake pointers, no device
@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import _lib, build
    build.build()
    return _lib.lib()


FAKE = C.c_void_p(0x1000)                # 16-byte aligned, never dereferenced: every call below returns before a launch


def _job(*fields):
    from pegasus_amd import _lib
    return (_lib.PgrObbJob * 1)(_lib.PgrObbJob(*fields))


def test_obb_candidates_refuses_bad_arguments_before_any_launch(lib):
    from pegasus_amd import _lib
    BAD, SMALL = _lib.PGR_ERR_INVALID_ARGUMENT, _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    tri = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    host = tri.ctypes.data

    def rc(jobs=_job(0, 4, 0, 2), n_jobs=1, points=FAKE, n_points=4, tris=FAKE, n_tris=2, tris_host=host, volumes=FAKE,
           best=FAKE, lohi=FAKE, ws=FAKE, ws_bytes=1 << 20):
        return lib.pgr_obb_candidates(points, n_points, tris, n_tris, tris_host, n_jobs, jobs, volumes, best, lohi, ws, ws_bytes,
                                      None)
    assert rc(n_jobs=0) == _lib.PGR_OK and rc(n_jobs=0, jobs=None, points=None, tris=None) == _lib.PGR_OK
    assert rc(n_jobs=-1) == BAD and rc(jobs=None) == BAD
    assert rc(n_points=-1) == BAD and rc(n_tris=-1) == BAD
    for fields in ((-1, 4, 0, 2), (0, -1, 0, 2), (0, 4, -1, 2), (0, 4, 0, -1), (1, 4, 0, 2), (0, 5, 0, 2), (0, 4, 1, 2),
                   (0, 4, 0, 3), (0, 0, 0, 2), (2 ** 31 - 1, 4, 0, 2), (0, 4, 2 ** 31 - 1, 2)):
        assert rc(jobs=_job(*fields)) == BAD, fields
    for name in ("points", "tris", "volumes", "best", "lohi", "ws"):
        assert rc(**{name: None}) == BAD, name
    assert rc(ws=C.c_void_p(0x1008)) == BAD                               # not 16-byte aligned
    need = lib.pgr_obb_candidates_workspace_bytes(1, _job(0, 4, 0, 2))
    assert need > 0 and rc(ws_bytes=need - 1) == SMALL
    # indices: checked against the job's point_count when the host copy is there
    assert rc(jobs=_job(0, 3, 0, 2)) == BAD                               # index 3 of 3 points
    low = np.array([[0, -1, 2], [1, 2, 3]], np.int32)
    assert rc(tris_host=low.ctypes.data) == BAD
    assert rc(jobs=_job(0, 3, 1, 1), n_points=4) == BAD                   # the second triangle names point 3


def test_point_diameter_refuses_bad_arguments_before_any_launch(lib):
    from pegasus_amd import _lib
    BAD, SMALL = _lib.PGR_ERR_INVALID_ARGUMENT, _lib.PGR_ERR_WORKSPACE_TOO_SMALL

    def rc(jobs=_job(0, 4, 0, 0), n_jobs=1, points=FAKE, n_points=4, pair=FAKE, d2=FAKE, ws=FAKE, ws_bytes=1 << 20):
        return lib.pgr_point_diameter(points, n_points, n_jobs, jobs, pair, d2, ws, ws_bytes, None)
    assert rc(n_jobs=0) == _lib.PGR_OK and rc(n_jobs=0, jobs=None, points=None) == _lib.PGR_OK
    assert rc(n_jobs=-1) == BAD and rc(jobs=None) == BAD and rc(n_points=-1) == BAD
    for fields in ((-1, 4, 0, 0), (0, -1, 0, 0), (1, 4, 0, 0), (0, 5, 0, 0), (2 ** 31 - 1, 4, 0, 0)):
        assert rc(jobs=_job(*fields)) == BAD, fields
    for name in ("points", "pair", "d2", "ws"):
        assert rc(**{name: None}) == BAD, name
    assert rc(ws=C.c_void_p(0x1008)) == BAD
    need = lib.pgr_point_diameter_workspace_bytes(1, _job(0, 4, 0, 0))
    assert need > 0 and rc(ws_bytes=need - 1) == SMALL


def test_workspace_sizes_are_zero_for_bad_arguments(lib):
    for fn in (lib.pgr_obb_candidates_workspace_bytes, lib.pgr_point_diameter_workspace_bytes):
        assert fn(0, _job(0, 4, 0, 2)) == 0 and fn(-1, _job(0, 4, 0, 2)) == 0 and fn(1, None) == 0
        assert fn(1, _job(0, -1, 0, 2)) == 0
        assert fn(1, _job(0, 4, 0, 2)) > 0 and fn(1, _job(0, 0, 0, 0)) > 0
    assert lib.pgr_obb_candidates_workspace_bytes(1, _job(0, 4, 0, -1)) == 0
    assert lib.pgr_obb_candidates_workspace_bytes(1, _job(0, 0, 0, 2)) == 0          # triangles over no points
    # the partial extremes: 6 float64 per (triangle, chunk of points); few triangles over many points are cut into chunks
    one = lib.pgr_obb_candidates_workspace_bytes(1, _job(0, OC.TP, 0, 12))
    many = lib.pgr_obb_candidates_workspace_bytes(1, _job(0, 100003, 0, 12))
    assert one == 768 and many >= 12 * 6 * 8 * 2 and many % 256 == 0


def test_tiles_in_the_header_are_the_ones_python_binds():
    from pegasus_amd import _lib
    assert (OC.TF, OC.TP, OC.TD) == (_lib.PGR_OBB_TRI_TILE, _lib.PGR_OBB_POINT_TILE, _lib.PGR_DIAMETER_TILE)
    assert C.sizeof(_lib.PgrObbJob) == 16


# ---- command lines
def test_generate_names_the_option_that_oriented_boxes_need(tmp_path, capsys):
    from pegasus_amd import generate
    with pytest.raises(SystemExit) as e:
        generate.main(["--out", str(tmp_path), "--boxes", "oriented"])
    assert e.value.code == 2 and "--gt-from-meshes" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        generate.main(["--out", str(tmp_path), "--boxes", "tight"])
    assert e.value.code == 2 and "--boxes" in capsys.readouterr().err


def test_obb_command_line_argument_errors(tmp_path, capsys):
    from pegasus_amd import obb
    with pytest.raises(SystemExit) as e:
        obb.main(["--dataset", str(tmp_path)])
    assert e.value.code == 2 and "--models" in capsys.readouterr().err
    with pytest.raises(FileNotFoundError, match="obj_NNNNNN.ply"):
        obb.main(["--models", str(tmp_path)])
