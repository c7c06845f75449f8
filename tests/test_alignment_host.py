"""Ground-plane alignment without a device: the three pgr_plane_* entries are declared, exported and prototyped and decide
their arguments on the host; the float64 reference (tests/alignment_reference.py) against hand-worked planes and against the
known plane of the cases; the validity of every case; the tolerance on the 4x4 measured again; the host side of
pegasus_amd/alignment.py -- the choice, the refit, the orientation, the transformation, COLMAP models, the command line."""
import ctypes as C
import json
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))

import alignment_cases as AC             # noqa: E402
import alignment_reference as AR         # noqa: E402
from pegasus_amd import alignment        # noqa: E402  (without the feature nothing in this file runs)

NAMES = ("pgr_plane_hypotheses", "pgr_plane_score_workspace_bytes", "pgr_plane_score", "pgr_plane_inliers_workspace_bytes",
         "pgr_plane_inliers")
FAKE = 0x10000                           # a non-NULL, 16-byte aligned address that is never dereferenced on the host
PLANE = (C.c_double * 4)(0.0, 0.0, 1.0, -0.5)
PIVOT = (C.c_double * 3)(0.0, 0.0, 0.5)


@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import _lib, build
    build.build()
    return _lib.lib()


# ---- the entries
def test_symbols_are_declared_exported_and_prototyped(lib):
    from pegasus_amd import _lib
    header = (ROOT / "include" / "pegasus_raster.h").read_text()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.pgr_abi_version() == 4
    assert int(re.search(r"#define PGR_PLANE_SUMS (\d+)", header).group(1)) == alignment.SUMS == AR.SUMS == _lib.PGR_PLANE_SUMS
    assert int(re.search(r"#define PGR_PLANE_TILE (\d+)", header).group(1)) == AC.TILE == _lib.PGR_PLANE_TILE
    assert (alignment.COUNT, alignment.SUM_Q, alignment.SUM_QQ, alignment.SUM_D2) == (AR.COUNT, AR.SUM_Q, AR.SUM_QQ, AR.SUM_D2)
    assert AC.PLANE_HYP_BATCH * 4 <= AC.PLANE_BLOCK and AC.PLANE_BLOCK % 64 == 0


def test_workspace_sizes(lib):
    score, inliers = lib.pgr_plane_score_workspace_bytes, lib.pgr_plane_inliers_workspace_bytes
    for bad in ((-1, 1), (1, -1), (-(1 << 31), 1), (1, -(1 << 31)), (-1, -1)):
        assert score(*bad) == 0
    assert inliers(-1) == 0 and inliers(-(1 << 31)) == 0
    for size in (inliers, lambda n: score(n, 1000), lambda n: score(n, 1)):
        sizes = [size(n) for n in (0, 1, 255, 256, 257, AC.TILE, AC.TILE + 1, 65537, 2_000_000, (1 << 31) - 1)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert all(s % 256 == 0 for s in sizes)
    # one partial of 12 bytes per hypothesis and tile of points; 12 doubles per workgroup of the inlier pass
    blocks = 1_360_000 // AC.TILE + 1
    assert blocks * 1000 * 12 <= score(1_360_000, 1000) <= blocks * 1000 * 12 + 512
    assert score(AC.TILE, 7) == score(1, 7) < score(AC.TILE + 1, 70000)
    assert inliers(2_000_000) <= (2_000_000 // AC.PLANE_BLOCK + 1) * 12 * 8 + 256


def _calls(lib):
    """name -> a call with good arguments except for the keywords given."""
    def hypotheses(n=4, xyz=FAKE, h=4, triples=FAKE, planes=FAKE, valid=FAKE):
        return lib.pgr_plane_hypotheses(n, xyz, h, triples, planes, valid, None)

    def score(n=4, xyz=FAKE, h=4, planes=FAKE, d=0.01, counts=FAKE, sumsq=FAKE, ws=FAKE, ws_bytes=None):
        size = lib.pgr_plane_score_workspace_bytes(max(n, 0), max(h, 0)) if ws_bytes is None else ws_bytes
        return lib.pgr_plane_score(n, xyz, h, planes, d, counts, sumsq, ws, size, None)

    def inliers(n=4, xyz=FAKE, plane=PLANE, pivot=PIVOT, d=0.01, mask=FAKE, sums=FAKE, ws=FAKE, ws_bytes=None):
        size = lib.pgr_plane_inliers_workspace_bytes(max(n, 0)) if ws_bytes is None else ws_bytes
        return lib.pgr_plane_inliers(n, xyz, plane, pivot, d, mask, sums, ws, size, None)
    return dict(hypotheses=hypotheses, score=score, inliers=inliers)


def test_invalid_arguments_are_refused_before_any_launch(lib):
    from pegasus_amd import _lib
    bad = _lib.PGR_ERR_INVALID_ARGUMENT
    call = _calls(lib)
    for name, fn in call.items():
        assert fn(n=-1) == bad and fn(n=-(1 << 31)) == bad, name
        assert fn(xyz=None) == bad, name
    for name in ("hypotheses", "score"):
        assert call[name](h=-1) == bad and call[name](planes=None) == bad, name
    assert call["hypotheses"](triples=None) == bad and call["hypotheses"](valid=None) == bad
    assert call["hypotheses"](n=0, xyz=None, triples=None) == bad                # rows to write, nothing to write them from
    for name in ("score", "inliers"):
        for d in (0.0, -0.01, math.nan, math.inf, -math.inf):
            assert call[name](d=d) == bad, (name, d)
            assert call[name](n=0, d=d) == bad, (name, d)
        assert call[name](ws=None) == bad and call[name](ws=FAKE + 8) == bad, name
    assert call["score"](h=0, d=math.nan) == bad
    assert call["score"](counts=None) == bad and call["score"](sumsq=None) == bad
    assert call["score"](n=0, counts=None) == bad and call["score"](n=0, sumsq=None) == bad
    assert call["inliers"](plane=None) == bad and call["inliers"](pivot=None) == bad and call["inliers"](sums=None) == bad
    assert call["inliers"](n=0, sums=None) == bad and call["inliers"](n=0, plane=None) == bad
    for k in range(4):
        for v in (math.nan, math.inf):
            plane = [0.0, 0.0, 1.0, -0.5]
            plane[k] = v
            assert call["inliers"](plane=(C.c_double * 4)(*plane)) == bad
    assert call["inliers"](pivot=(C.c_double * 3)(0.0, math.nan, 0.0)) == bad


def test_short_workspaces_are_refused_and_no_rows_are_ok(lib):
    from pegasus_amd import _lib
    call = _calls(lib)
    for n in (1, 257, AC.TILE + 1):
        for h in (1, 65):
            size = lib.pgr_plane_score_workspace_bytes(n, h)
            assert call["score"](n=n, h=h, ws_bytes=size - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
            assert call["score"](n=n, h=h, ws_bytes=0) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
        size = lib.pgr_plane_inliers_workspace_bytes(n)
        assert call["inliers"](n=n, ws_bytes=size - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
        assert call["inliers"](n=n, ws_bytes=0) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    # no hypothesis: nothing to write, nothing is launched and nothing else is looked at
    assert call["hypotheses"](h=0, xyz=None, triples=None, planes=None, valid=None) == _lib.PGR_OK
    assert call["score"](h=0, xyz=None, planes=None, counts=None, sumsq=None, ws=None, ws_bytes=0) == _lib.PGR_OK


# ---- the reference against hand-worked answers
def test_reference_hypotheses_by_hand():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2], [2, 0, 0], [3, 0, 0], [1, 0, 0]], dtype=np.float32)
    tri = [[0, 1, 2], [0, 2, 1], [3, 1, 2], [0, 1, 4], [1, 6, 2], [0, 0, 1], [0, 1, 7], [-1, 1, 2]]
    planes, valid = AR.hypotheses(pts, tri)
    np.testing.assert_array_equal(valid, [1, 1, 1, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(planes[0], [0, 0, 1, 0])
    np.testing.assert_array_equal(planes[1], [0, 0, -1, 0])
    # through (0,0,2), (1,0,0), (0,1,0): 2x + 2y + z = 2, the normal (2, 2, 1) / 3
    np.testing.assert_allclose(planes[2], [2 / 3, 2 / 3, 1 / 3, -2 / 3], rtol=0, atol=1e-16)
    assert not planes[3:].any()                                  # collinear, coincident, repeated, outside


def test_reference_scores_and_choice_by_hand():
    z = np.array([0.0, 0.001, -0.002, 0.009, 0.01, 0.011, 0.5], dtype=np.float32)
    pts = np.stack([np.arange(len(z), dtype=np.float32), np.ones(len(z), dtype=np.float32), z], axis=1)
    planes = np.array([[0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 1, -0.5], [0, 0, -1, 0]], dtype=np.float64)
    sc = AR.scores(pts, planes, 0.01)
    z64 = z.astype(np.float64)
    inside = np.abs(z64) < 0.01
    assert inside.tolist() == [True, True, True, True, True, False, False]        # float32(0.01) < 0.01
    np.testing.assert_array_equal(sc.counts, [5, 0, 1, 5])
    assert sc.sumsq[0] == sc.sumsq[3] == pytest.approx((z64[inside] ** 2).sum(), rel=1e-15) and sc.sumsq[1] == 0.0
    assert AR.choose(sc.counts, sc.sumsq, [1, 1, 1, 1]) == (0, 3)                # equal in both: the lower index
    assert AR.choose(sc.counts, sc.sumsq, [0, 1, 1, 1]) == (3, 2)
    assert AR.choose(sc.counts, [2.0, 0.0, 0.0, 1.0], [1, 1, 1, 1]) == (3, 0)    # equal counts: the smaller sum
    assert AR.choose(sc.counts, sc.sumsq, [0, 0, 0, 0]) == (-1, -1)
    for args in ((sc.counts, sc.sumsq, [1, 1, 1, 1]), (sc.counts, sc.sumsq, [0, 1, 1, 1]),
                 (sc.counts, [2.0, 0.0, 0.0, 1.0], [1, 1, 1, 1]), (sc.counts, sc.sumsq, [0, 0, 0, 0])):
        assert alignment.choose_best(*args) == AR.choose(*args)[0]


def test_reference_inlier_sums_and_refit_by_hand():
    # a 3 x 3 lattice in the plane z = 0.5 and two points off it
    xy = np.array([[x, y] for x in (-1, 0, 1) for y in (-1, 0, 1)], dtype=np.float32)
    pts = np.concatenate([np.concatenate([xy, np.full((9, 1), 0.5, dtype=np.float32)], axis=1),
                          np.array([[0, 0, 0.75], [5, 5, 0.25]], dtype=np.float32)])
    r = AR.inlier_sums(pts, [0, 0, 1, -0.5], [1, 1, 0.5], 0.125)
    np.testing.assert_array_equal(r.mask, [1] * 9 + [0, 0])
    np.testing.assert_array_equal(r.sums, [9, -9, -9, 0, 15, 9, 0, 15, 0, 0, 0, 0])       # q = p - (1, 1, 0.5)
    plane, gap = AR.refit(r.sums, [1, 1, 0.5], [0, 0, 1, -0.5])
    assert gap == pytest.approx(1.0)                                             # eigenvalues 0, 2/3, 2/3
    np.testing.assert_allclose(AR.orient(plane), [0, 0, 1, -0.5], rtol=0, atol=1e-15)
    # three points on a line: l0 == l1 == 0, the hypothesis plane stays
    line = AR.inlier_sums(pts[[1, 4, 7]], [0, 0, 1, -0.5], [0, 0, 0.5], 0.125)
    assert line.sums[0] == 3
    for got in (AR.refit(line.sums, [0, 0, 0.5], [0, 0, 1, -0.5])[0], alignment.refit_plane(line.sums, [0, 0, 0.5], [0, 0, 1, -0.5])):
        assert got.tolist() == [0, 0, 1, -0.5]
    pts[:9, 0] *= 2                                                              # now 8/3 : 2/3 : 0
    tilted = [0.0, math.sin(0.01), math.cos(0.01), -0.5 * math.cos(0.01)]
    r = AR.inlier_sums(pts, tilted, [0, 0, 0.5], 0.125)
    for fn in (AR.refit, lambda *a: (alignment.refit_plane(*a), None)):
        plane, _ = fn(r.sums, [0, 0, 0.5], tilted)
        np.testing.assert_allclose(AR.orient(plane), [0, 0, 1, -0.5], rtol=0, atol=1e-15)
    assert AR.refit([2] + [0] * 11, [0, 0, 0], tilted)[0].tolist() == tilted     # fewer than 3 inliers
    assert alignment.refit_plane([2] + [0] * 11, [0, 0, 0], tilted).tolist() == tilted


def test_orientation():
    plane = np.array([0.6, 0.0, -0.8, 0.25])
    for mod in (AR.orient, alignment.orient_plane):
        np.testing.assert_array_equal(mod(plane), -plane)                        # the largest component becomes positive
        np.testing.assert_array_equal(mod(plane, plane_normal=[0, 0, -1]), plane)
        np.testing.assert_array_equal(mod(plane, plane_normal=[0, 0, 1]), -plane)
        np.testing.assert_array_equal(mod(plane, plane_normal=[0, 1, 0]), plane)  # n . plane_normal = 0 counts as >= 0
        below, above = [[0, 0, 5.0]], [[0, 0, -5.0]]                              # signed distances -3.75 and 4.25
        np.testing.assert_array_equal(mod(plane, camera_centers=above), plane)
        np.testing.assert_array_equal(mod(plane, camera_centers=below), -plane)
        np.testing.assert_array_equal(mod(plane, camera_centers=above + below), plane)        # exactly half: stays
        np.testing.assert_array_equal(mod(plane, camera_centers=above + below + below), -plane)
        np.testing.assert_array_equal(mod(plane, camera_centers=np.zeros((0, 3))), -plane)


def test_rotation_to_z_and_transformation():
    rng = np.random.default_rng(3)
    normals = [np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, -1.0]), np.array([1.0, 0.0, 0.0])]
    normals += [v / np.linalg.norm(v) for v in rng.normal(size=(20, 3))]
    for n in normals:
        for fn in (AR.rotation_to_z, alignment.rotation_to_z):
            R = fn(n)
            np.testing.assert_allclose(R @ n, [0, 0, 1], rtol=0, atol=1e-14)
            np.testing.assert_allclose(R.T @ R, np.eye(3), rtol=0, atol=1e-14)
            assert abs(np.linalg.det(R) - 1.0) < 1e-14
            # the smallest rotation: its angle is the angle between n and z
            assert math.acos(min(1.0, max(-1.0, (np.trace(R) - 1) / 2))) == pytest.approx(math.acos(n[2]), abs=1e-7)
    np.testing.assert_array_equal(alignment.rotation_to_z([0, 0, 1.0]), np.eye(3))
    np.testing.assert_array_equal(alignment.rotation_to_z([0, 0, -1.0]), np.diag([1.0, -1.0, -1.0]))
    n = normals[5]
    centroid = np.array([1.0, -2.0, 0.5])
    fit = alignment.PlaneFit(plane=np.append(n, 0.3), hypothesis_plane=np.zeros(4), best_index=0, count=3, fitness=1.0,
                             inlier_rmse=0.0, centroid=centroid)
    for s in (1.0, 2.5):
        T = alignment.plane_transformation(fit, s)
        np.testing.assert_allclose(T, AR.transformation(fit.plane, centroid, s), rtol=0, atol=1e-15)
        on_plane = centroid - (n @ centroid + 0.3) * n
        np.testing.assert_allclose(T[:3, :3] @ on_plane + T[:3, 3], 0, atol=1e-14)           # lands on the origin
        other = on_plane + np.cross(n, [1.0, 2.0, 3.0])                                        # another point of the plane
        moved = T[:3, :3] @ other + T[:3, 3]
        assert abs(moved[2]) < 1e-14 and np.linalg.norm(moved) == pytest.approx(s * np.linalg.norm(other - on_plane))
        assert (T[:3, :3] @ (on_plane + n) + T[:3, 3])[2] == pytest.approx(s)                 # the normal's side is +z
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            alignment.plane_transformation(fit, bad)


# ---- the cases
@pytest.mark.parametrize("shape", AC.SHAPES)
def test_cases_are_valid_and_the_reference_finds_the_ground(shape):
    n, h = shape
    ref = AC.reference_fit(n, h)                                 # asserts the margin and the choice
    _, known, _, offset = AC.scene(n)
    assert ref.margin >= AC.MARGIN_MIN and ref.sumsq_gap > AC.SUMSQ_GAP_MIN
    assert ref.eigen_gap > 0.5
    assert AR.plane_angle_deg(ref.plane, known) < AC.PLANE_DEG_MAX
    assert abs(float(ref.plane[:3] @ offset + ref.plane[3])) < AC.PLANE_M_MAX
    assert ref.plane[:3] @ known[:3] > 0                         # the cameras are on the blobs' side
    assert AR.plane_angle_deg(ref.plane, known) < AR.plane_angle_deg(ref.hypothesis_plane, known)
    assert 0.55 < ref.fitness < 0.7


def test_every_kernel_case_is_valid():
    for n in AC.SCORE_NS:
        AC.score_case(n, AC.SCORE_H)
        AC.inlier_case(n)
    for h in AC.BATCH_HS:
        AC.score_case(AC.BATCH_N, h, source=(AC.BATCH_N, AC.SCORE_H))
    for blocks in AC.FINAL_BLOCKS:
        points, _, ref = AC.final_case(blocks)
        assert (len(points) + AC.TILE - 1) // AC.TILE == blocks
    assert ref.counts.max() > 1000
    # the launch arithmetic: every case above gives a workgroup one batch; the grouped case two, the second of the last short
    assert all(AC.score_launch(n, AC.SCORE_H)[1] == 1 for n in AC.SCORE_NS)
    assert AC.score_launch(1_360_000, 1000) == (665, 8, 2) and AC.score_launch(150_000, 1000) == (74, 2, 8)
    points, planes, ref = AC.grouped_case()                      # asserts its margin
    assert AC.score_launch(len(points), len(planes))[1:] == (2, (len(planes) + 2 * AC.PLANE_HYP_BATCH - 1) // (2 * AC.PLANE_HYP_BATCH))
    points, tri, thr, want = AC.strictness()
    planes, valid = AR.hypotheses(points, tri)
    assert valid.tolist() == [1] and planes[0].tolist() == [0, 0, 1, 0]
    np.testing.assert_array_equal(AR.inlier_sums(points, planes[0], points[0], thr).mask, want)
    degenerate, valid = AR.hypotheses(AC.degenerate_points(257), AC.degenerate_triples(257))
    assert valid.tolist() == [0] * 13 + [1, 0] and not degenerate[valid == 0].any()


@pytest.mark.parametrize("shape", AC.END_TO_END)
def test_transformation_tolerance_is_the_references_own_error(shape):
    """Both shapes measured again, each against its OWN recorded figure.  Twice the figure is allowed: it is one machine's
    roundings (NumPy's pairwise sums depend on its vector width), and T_TOL takes a hundred times it."""
    n, h = shape
    a, b = AC.reference_fit(n, h), AC.reference_fit(n, h, "longdouble")
    assert b.transformation.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
    assert a.best_index == b.best_index and np.array_equal(a.mask, b.mask)
    diff = float(np.abs(b.transformation - a.transformation.astype(np.longdouble)).max())
    print(shape, "largest |T longdouble - T float64| =", diff, "recorded", AC.T_TOL_MEASURED[shape])
    assert diff <= 2 * AC.T_TOL_MEASURED[shape]
    assert AC.T_TOL == max(1e-13, 100 * max(AC.T_TOL_MEASURED.values())) and AC.T_TOL < 1e-12


# ---- COLMAP models
def _colmap_model(rng, n_images=4, n_points=40):
    """Cameras 3 - 5 m from the origin that look at it, with a random roll, and points within 1 m of it: every point lies in
    front of every camera."""
    from scipy.spatial.transform import Rotation as Rot
    from pegasus_amd import colmap_io
    cameras = {1: colmap_io.ColmapCamera(1, "PINHOLE", 640, 480, np.array([500.0, 510.0, 320.0, 240.0])),
               2: colmap_io.ColmapCamera(2, "SIMPLE_PINHOLE", 320, 240, np.array([300.0, 160.0, 120.0]))}
    images = {}
    for k in range(n_images):
        eye = rng.normal(size=3)
        eye *= rng.uniform(3.0, 5.0) / np.linalg.norm(eye)
        z = -eye / np.linalg.norm(eye)
        x = np.cross(z, rng.normal(size=3))
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])                                     # world to camera, z forward
        q = Rot.from_matrix(R).as_quat()
        images[k + 1] = colmap_io.ColmapImage(k + 1, np.array([q[3], q[0], q[1], q[2]]), -R @ eye, 1 + k % 2,
                                              f"frame_{k:03d}.png")
    xyz = rng.normal(size=(n_points, 3))
    xyz *= (rng.uniform(0.0, 1.0, (n_points, 1)) / np.linalg.norm(xyz, axis=1, keepdims=True))
    return cameras, images, xyz, rng.integers(0, 256, (n_points, 3)).astype(np.uint8)


def _pixels(cameras, images, xyz):
    from pegasus_amd.colmap_io import qvec2rotmat
    out = []
    for im in images.values():
        cam = cameras[im.camera_id]
        fx, fy = cam.focal
        cx, cy = cam.params[-2:]
        x = xyz @ qvec2rotmat(im.qvec).T + im.tvec
        out.append(np.stack([fx * x[:, 0] / x[:, 2] + cx, fy * x[:, 1] / x[:, 2] + cy], axis=1))
    return np.array(out)


def _random_similarity(rng, s):
    from scipy.spatial.transform import Rotation as Rot
    T = np.eye(4)
    T[:3, :3] = s * Rot.random(random_state=int(rng.integers(1 << 30))).as_matrix()
    T[:3, 3] = rng.uniform(-4, 4, 3)
    return T


def test_transform_colmap_leaves_every_projection_where_it_was():
    from pegasus_amd.colmap_io import qvec2rotmat
    rng = np.random.default_rng(17)
    cameras, images, xyz, _ = _colmap_model(rng)
    for s in (1.0, 2.5, 0.01):
        T = _random_similarity(rng, s)
        moved, xyz2 = alignment.transform_colmap(cameras, images, xyz, T)
        np.testing.assert_allclose(xyz2, xyz @ T[:3, :3].T + T[:3, 3], rtol=0, atol=1e-12)
        before, after = _pixels(cameras, images, xyz), _pixels(cameras, moved, xyz2)
        assert np.abs(before).max() < 1e3 and np.abs(after - before).max() < 1e-9
        for key, im in images.items():
            new = moved[key]
            assert (new.id, new.camera_id, new.name) == (im.id, im.camera_id, im.name)
            assert abs(np.linalg.norm(new.qvec) - 1.0) < 1e-12
            centre = -qvec2rotmat(im.qvec).T @ im.tvec                           # the camera centre moves like a point
            np.testing.assert_allclose(-qvec2rotmat(new.qvec).T @ new.tvec, T[:3, :3] @ centre + T[:3, 3], rtol=0, atol=1e-9)
    for bad in (np.diag([1.0, 2.0, 1.0, 1.0]), np.diag([1.0, 1.0, -1.0, 1.0]), np.zeros((4, 4)), np.eye(3)):
        with pytest.raises(ValueError):
            alignment.transform_colmap(cameras, images, xyz, bad)


@pytest.mark.parametrize("binary", (True, False))
def test_reconstruction_alignment_save_round_trip(tmp_path, binary):
    from pegasus_amd import colmap_io
    rng = np.random.default_rng(29)
    cameras, images, xyz, rgb = _colmap_model(rng)
    sparse = tmp_path / "sparse" / "0"
    colmap_io.write_colmap_model(sparse, cameras, images, xyz, rgb, binary=binary)
    cached = colmap_io.fetch_point_cloud(tmp_path)                               # writes sparse/0/points3D.ply
    assert (sparse / "points3D.ply").exists()
    original = {p.name: p.read_bytes() for p in sparse.iterdir() if p.suffix != ".ply"}

    reco = alignment.ReconstructionAlignment(tmp_path)
    np.testing.assert_array_equal(reco.xyz, xyz)
    for bad in (0.0, -2.0, math.nan):
        with pytest.raises(ValueError):
            reco.scale_scene_by_const(bad)
    reco.scale_scene_by_const(2.5)
    np.testing.assert_array_equal(reco.transformation, np.diag([2.5, 2.5, 2.5, 1.0]))
    T = _random_similarity(rng, 2.5)
    reco.transformation, reco.plane_size = T, 2.0
    reco.save()

    assert not (sparse / "points3D.ply").exists()
    backup = tmp_path / "sparse" / "0_unaligned"
    assert {p.name: p.read_bytes() for p in backup.iterdir() if p.suffix != ".ply"} == original
    cameras2, images2 = colmap_io.read_model(tmp_path)
    read_points = colmap_io.read_points3D_binary if binary else colmap_io.read_points3D_text
    xyz2, rgb2 = read_points(sparse / ("points3D.bin" if binary else "points3D.txt"))
    assert (sparse / "points3D.bin").exists() == binary
    want_images, want_xyz = alignment.transform_colmap(cameras, images, xyz, T)
    np.testing.assert_array_equal(xyz2, want_xyz)
    np.testing.assert_array_equal(rgb2, rgb)
    assert set(images2) == set(images) and set(cameras2) == set(cameras)
    for key in images:
        np.testing.assert_array_equal(images2[key].qvec, want_images[key].qvec)
        np.testing.assert_array_equal(images2[key].tvec, want_images[key].tvec)
        assert images2[key].name == images[key].name
    assert np.abs(_pixels(cameras2, images2, xyz2) - _pixels(cameras, images, xyz)).max() < 1e-6
    record = json.loads((tmp_path / "alignment.json").read_text())
    np.testing.assert_array_equal(np.array(record["transformation"]), T)
    assert record["scale"] == 2.5 and record["plane_size"] == 2.0 and record["plane"] is None
    rebuilt = colmap_io.fetch_point_cloud(tmp_path)                              # the cache is rebuilt from the moved points
    np.testing.assert_allclose(rebuilt.points, want_xyz.astype(np.float32), rtol=0, atol=0)
    assert np.abs(rebuilt.points - cached.points).max() > 0.1
    with pytest.raises(RuntimeError, match="nothing to save"):                   # save() left nothing pending
        reco.save()
    assert json.loads((tmp_path / "alignment.json").read_text()) == record
    # a second save keeps the FIRST original
    again = alignment.ReconstructionAlignment(tmp_path)
    with pytest.raises(RuntimeError, match="nothing to save"):
        again.save()
    again.scale_scene_by_const(2.0)
    again.save()
    assert {p.name: p.read_bytes() for p in backup.iterdir() if p.suffix != ".ply"} == original


# ---- the package's argument checks
def test_python_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    pts = torch.zeros((4, 3))
    planes = torch.zeros((2, 4), dtype=torch.float64)
    for fn, args in ((alignment.segment_plane, (pts,)), (alignment.fit_ground_plane, (pts,)),
                     (alignment.plane_hypotheses, (pts, np.zeros((2, 3), dtype=np.int32))),
                     (alignment.plane_scores, (pts, planes, 0.01)),
                     (alignment.plane_inliers, (pts, [0, 0, 1, 0], [0, 0, 0], 0.01))):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            fn(*args)
    for bad in (pts.double(), pts[:, :2], pts.reshape(-1), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError):
            alignment.fit_ground_plane(bad)
    for ransac_n in (2, 4, 0):
        with pytest.raises(ValueError, match="ransac_n"):
            alignment.segment_plane(pts, ransac_n=ransac_n)
    bad_T = np.eye(4)
    bad_T[0, 0] = 2.0
    for T in (bad_T, np.diag([1.0, 1.0, -1.0, 1.0]), np.eye(3), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError):
            alignment.transform_model(None, T)
    shear = np.eye(4)
    shear[0, 1] = 1e-5
    with pytest.raises(ValueError):
        alignment.transform_model(None, shear)
    n = 1000
    tri = alignment.draw_triples(n, 50, 11)
    assert tri.dtype == np.int32 and tri.shape == (50, 3)
    np.testing.assert_array_equal(tri, np.random.default_rng(11).integers(0, n, size=(50, 3)))
    np.testing.assert_array_equal(tri, AC.triples(n, 50))


def test_command_line_argument_errors(capsys):
    for argv in ([], ["--project", "a", "--model", "b.ply", "--out", "c.ply"], ["--model", "b.ply"],
                 ["--project", "a", "--out", "c.ply"], ["--project", "a", "--crop", "2"], ["--project", "a", "--scale", "0"],
                 ["--project", "a", "--scale", "nan"], ["--project", "a", "--threshold", "-1"],
                 ["--project", "a", "--iterations", "0"], ["--model", "b.ply", "--out", "c.ply", "--crop", "0"],
                 ["--project", "a", "--plane_normal", "0", "1"], ["--project", "a", "--seed", "x"]):
        with pytest.raises(SystemExit) as e:
            alignment.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    with pytest.raises(FileNotFoundError):
        alignment.main(["--project", "/nonexistent/project"])
