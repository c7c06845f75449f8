"""Minimal oriented boxes and diameters on the GPU (pegasus_amd/obb.py over pgr_obb_candidates and pgr_point_diameter)
against the float64 restatement of tests/obb_reference.py, within the bounds derived there; the choice of the box, the
repeatability and the independence of the batch and of the point split bit for bit; guard words round every buffer.

Largest error / bound ratios seen on an MI355X over all cases: volumes 0.0156 (257 triangles over 511 points), lohi 0.0207
(255 triangles over 3 points), diameter 0 (the device's pair was the reference's in every case)."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import obb_cases as OC                   # noqa: E402
import obb_reference as OR               # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256                               # bytes on either side of every buffer
FILL = 0xA5


class Guarded:
    """A device buffer of ``n`` elements with GUARD bytes of FILL on either side."""

    def __init__(self, dev, n, dtype):
        import torch
        self.item = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((n * self.item + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.n, self.dtype = n, dtype

    @property
    def ptr(self):
        import ctypes as C
        return C.c_void_p(self.raw.data_ptr() + GUARD)

    def intact(self):
        return bool((self.raw[:GUARD] == FILL).all()) and bool((self.raw[GUARD + self.n * self.item:] == FILL).all())

    def host(self):
        return self.raw[GUARD:GUARD + self.n * self.item].clone().view(self.dtype).cpu().numpy()


def _jobs(sets):
    from pegasus_amd import _lib
    jobs = (_lib.PgrObbJob * max(1, len(sets)))()
    p0 = t0 = 0
    for k, (p, t) in enumerate(sets):
        jobs[k] = _lib.PgrObbJob(p0, len(p), t0, len(t))
        p0, t0 = p0 + len(p), t0 + len(t)
    return jobs


def run_candidates(dev, sets, host_copy=True):
    """pgr_obb_candidates over ``sets`` [(points, triangles)] on guarded buffers: (status, volumes per set, best, lohi)."""
    import torch
    from pegasus_amd import _lib
    K = len(sets)
    pts = np.concatenate([p for p, _ in sets] + [np.zeros((0, 3), np.float32)])
    tri = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32).reshape(-1, 3) for _, t in sets] +
                                              [np.zeros((0, 3), np.int32)]))
    jobs = _jobs(sets)
    need = int(_lib.lib().pgr_obb_candidates_workspace_bytes(K, jobs)) if K else 0
    d_p, d_t = torch.from_numpy(pts).to(dev), torch.from_numpy(tri).to(dev)
    vol, best, lohi = Guarded(dev, len(tri), torch.float64), Guarded(dev, K, torch.int32), Guarded(dev, 6 * K, torch.float64)
    ws = Guarded(dev, need, torch.uint8)
    status = _lib.enqueue("pgr_obb_candidates", dev, _lib.ptr(d_p), len(pts), _lib.ptr(d_t), len(tri),
                          tri.ctypes.data if host_copy and len(tri) else None, K, jobs, vol.ptr, best.ptr, lohi.ptr, ws.ptr, need)
    torch.cuda.synchronize()
    for name, g in (("volumes", vol), ("best", best), ("lohi", lohi), ("workspace", ws)):
        assert g.intact(), f"guard words of {name} were written"
    v = vol.host()
    edges = np.cumsum([0] + [len(t) for _, t in sets])
    return status, [v[edges[k]:edges[k + 1]] for k in range(K)], best.host(), lohi.host().reshape(K, 6)


def run_diameter(dev, sets):
    """pgr_point_diameter over point sets on guarded buffers: (status, pair [K,2], d2 [K])."""
    import torch
    from pegasus_amd import _lib
    K = len(sets)
    pts = np.concatenate(list(sets) + [np.zeros((0, 3), np.float32)])
    jobs = _jobs([(p, ()) for p in sets])
    need = int(_lib.lib().pgr_point_diameter_workspace_bytes(K, jobs)) if K else 0
    d_p = torch.from_numpy(pts).to(dev)
    pair, d2, ws = Guarded(dev, 2 * K, torch.int32), Guarded(dev, K, torch.float64), Guarded(dev, need, torch.uint8)
    status = _lib.enqueue("pgr_point_diameter", dev, _lib.ptr(d_p), len(pts), K, jobs, pair.ptr, d2.ptr, ws.ptr, need)
    torch.cuda.synchronize()
    for name, g in (("pair", pair), ("d2", d2), ("workspace", ws)):
        assert g.intact(), f"guard words of {name} were written"
    return status, pair.host().reshape(K, 2), d2.host()


def lowest_finite_minimum(volumes):
    """The lowest index attaining the smallest finite value, bit for bit; -1 if none is finite."""
    ok = np.isfinite(volumes)
    return int(np.nonzero(ok & (volumes == volumes[ok].min()))[0][0]) if ok.any() else -1


CASES = OC.all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_candidates_against_the_reference(gpu_device, name):
    from pegasus_amd import _lib
    pts, tri = CASES[name]
    status, (vol,), best, lohi = run_candidates(gpu_device, [(pts, tri)])
    assert status == _lib.PGR_OK
    ref_lohi, ref_vol, q_bound = OR.candidates(pts, tri)
    v_bound = OR.volume_bound(ref_lohi, q_bound)
    fin = np.isfinite(ref_vol)
    assert np.array_equal(np.isfinite(vol), fin)
    ratio = np.abs(vol[fin] - ref_vol[fin]) / v_bound[fin]
    print(f"{name}: F={len(tri)} P={len(pts)} volume error/bound max {ratio.max():.3g}")
    assert (ratio <= 1.0).all(), (name, int(np.argmax(ratio)), float(ratio.max()))
    b = int(best[0])
    assert b == lowest_finite_minimum(vol)
    r = OR.argmin_finite(ref_vol)
    assert ref_vol[b] - ref_vol[r] <= v_bound[b] + v_bound[r]
    lohi_ratio = np.abs(lohi[0] - ref_lohi[b]) / q_bound[b]
    print(f"{name}: lohi error/bound max {lohi_ratio.max():.3g}")
    assert (lohi_ratio <= 1.0).all(), (name, lohi[0].tolist(), ref_lohi[b].tolist(), float(q_bound[b]))


def test_degenerate_triangles_are_never_chosen(gpu_device):
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [3, 2, 1]], np.float32)
    repeated, collinear, good = [1, 1, 3], [0, 1, 2], [0, 1, 3]            # (0,0,0), (1,0,0), (2,0,0) lie on one line exactly
    _, (vol,), best, lohi = run_candidates(gpu_device, [(pts, np.array([repeated, collinear, good, good], np.int32))])
    assert not np.isfinite(vol[:2]).any() and np.isfinite(vol[2:]).all()
    assert best[0] == 2                                                    # the same triangle twice: the lower index
    assert vol[2].tobytes() == vol[3].tobytes() and vol[2] == 3.0 * 2.0 * 1.0
    assert lohi[0].tolist() == [0.0, 0.0, 0.0, 3.0, 2.0, 1.0]
    _, (vol,), best, lohi = run_candidates(gpu_device, [(pts, np.array([repeated, collinear, [4, 4, 4]], np.int32))])
    assert not np.isfinite(vol).any() and best[0] == -1 and np.isnan(lohi).all()


def test_a_coplanar_cloud_has_volume_zero_at_the_lowest_index(gpu_device):
    rng = np.random.default_rng(8)
    pts = np.concatenate([rng.integers(-50, 50, size=(40, 2)), np.full((40, 1), 7)], axis=1).astype(np.float32)
    pts[:3] = [[0, 0, 7], [5, 0, 7], [0, 3, 7]]
    tri = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)          # small integers in the plane z = 7: w is exactly z
    _, (vol,), best, lohi = run_candidates(gpu_device, [(pts, tri)])
    assert vol[0] == 0.0 and best[0] == 0 and lohi[0, 2] == 0.0 and lohi[0, 5] == 0.0
    assert not np.signbit(lohi[0][lohi[0] == 0]).any()                    # a zero is written as +0


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_point_that_is_not_finite_gives_none(gpu_device, bad):
    pts, tri = OC.affine_icosphere(1)
    for where in (0, len(pts) - 1):
        p = pts.copy()
        p[where, 1] = bad
        _, (vol,), best, lohi = run_candidates(gpu_device, [(p, tri)])
        assert not np.isfinite(vol).any() and best[0] == -1 and np.isnan(lohi).all()
    big = OC.split_case()[0].copy()                                       # the point sits in one chunk of many
    big[77777, 2] = bad
    _, (vol,), best, _ = run_candidates(gpu_device, [(big, OC.split_case()[1])])
    assert not np.isfinite(vol).any() and best[0] == -1


def test_a_batch_equals_its_jobs_one_by_one_and_itself(gpu_device):
    from pegasus_amd import _lib
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    no_triangles = (OC.tetrahedron()[0], np.zeros((0, 3), np.int32))
    sets = [empty, CASES["icosphere2_offset"], no_triangles, CASES["rotated_box"], CASES[f"random_F{OC.TF + 1}_P{OC.TP + 1}"],
            OC.split_case(), empty]
    status, vols, best, lohi = run_candidates(gpu_device, sets)
    assert status == _lib.PGR_OK
    again = run_candidates(gpu_device, sets)
    for k, one in enumerate(sets):
        _, (v,), b, l = run_candidates(gpu_device, [one])
        assert v.tobytes() == vols[k].tobytes() == again[1][k].tobytes(), k
        assert b[0] == best[k] == again[2][k], k
        assert l.tobytes() == lohi[k].tobytes() == again[3][k].tobytes(), k
    assert [int(best[k]) for k in (0, 2, 6)] == [-1, -1, -1] and np.isnan(lohi[[0, 2, 6]]).all()
    assert run_candidates(gpu_device, [])[0] == _lib.PGR_OK               # n_jobs == 0
    assert run_candidates(gpu_device, [empty, empty])[2].tolist() == [-1, -1]


def test_more_jobs_than_one_launch_takes(gpu_device):
    sets = [OC.random_case(5, 9, seed=k) for k in range(70)]               # 64 jobs per launch
    _, vols, best, lohi = run_candidates(gpu_device, sets)
    for k in (0, 63, 64, 69):
        _, (v,), b, l = run_candidates(gpu_device, [sets[k]])
        assert v.tobytes() == vols[k].tobytes() and b[0] == best[k] and l.tobytes() == lohi[k].tobytes()


def test_the_point_split_does_not_change_a_byte(gpu_device):
    pts, tri = OC.split_case()
    _, (alone,), best, lohi = run_candidates(gpu_device, [(pts, tri)])
    pts, many, where = OC.split_case_embedded()
    _, (among,), _, _ = run_candidates(gpu_device, [(pts, many)])
    assert among[where].tobytes() == alone.tobytes()
    only = np.full(len(many), np.inf)
    only[where] = among[where]
    assert where[int(best[0])] == lowest_finite_minimum(only)


def test_the_entry_checks_indices_given_a_host_copy(gpu_device):
    from pegasus_amd import _lib
    pts, tri = OC.tetrahedron()
    for bad in (-1, 4):
        t = tri.copy()
        t[2, 1] = bad
        status, (vol,), best, _ = run_candidates(gpu_device, [(pts, t)])
        assert status == _lib.PGR_ERR_INVALID_ARGUMENT
        assert (vol.view(np.uint8) == FILL).all() and (best.view(np.uint8) == FILL).all()          # nothing was launched


# ---- diameter
def check_diameter(dev, pts):
    from pegasus_amd import _lib
    status, pair, d2 = run_diameter(dev, [pts])
    assert status == _lib.PGR_OK
    ref_d2, ref_pair = OR.diameter(pts)
    i, j = (int(x) for x in pair[0])
    if len(pts) < 2:
        assert (i, j) == ((0, 0) if len(pts) else (-1, -1)) and d2[0] == 0.0
        return
    assert 0 <= i < j < len(pts)
    got = OR.d2_of(pts, i, j)
    ratio = (ref_d2 - got) / (OR.K_D2 * OR.EPS * ref_d2) if ref_d2 > 0 else 0.0
    print(f"diameter P={len(pts)}: pair {(i, j)} reference {ref_pair} error/bound {ratio:.3g}")
    assert 0.0 <= ref_d2 - got <= OR.K_D2 * OR.EPS * ref_d2
    assert abs(d2[0] - got) <= OR.K_D2 * OR.EPS * ref_d2


@pytest.mark.parametrize("n", OC.DIAMETER_P)
def test_diameter_sizes(gpu_device, n):
    check_diameter(gpu_device, np.ascontiguousarray(OC.ball_cloud(20011)[:n]))


def test_diameter_of_the_offset_cloud(gpu_device):
    check_diameter(gpu_device, OC.ball_cloud(2 * OC.TD + 1, seed=4, offset=OC.OFFSET))
    check_diameter(gpu_device, OC.split_case()[0][:3000])


def test_diameter_of_equal_points_and_ties(gpu_device):
    _, pair, d2 = run_diameter(gpu_device, [np.full((300, 3), 0.25, np.float32)])
    assert pair[0].tolist() == [0, 1] and d2[0] == 0.0
    square = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]] * 100, np.float32)      # both diagonals, many times
    _, pair, d2 = run_diameter(gpu_device, [square])
    assert pair[0].tolist() == [0, 2] and d2[0] == 2.0


def test_diameter_batch_equals_its_jobs(gpu_device):
    from pegasus_amd import _lib
    cloud = OC.ball_cloud(20011)
    sets = [np.zeros((0, 3), np.float32), cloud[:1], cloud[:OC.TD + 1], cloud, cloud[5:700]]
    status, pair, d2 = run_diameter(gpu_device, sets)
    assert status == _lib.PGR_OK and pair[0].tolist() == [-1, -1] and pair[1].tolist() == [0, 0]
    again = run_diameter(gpu_device, sets)
    assert pair.tobytes() == again[1].tobytes() and d2.tobytes() == again[2].tobytes()
    for k, one in enumerate(sets):
        _, p, d = run_diameter(gpu_device, [one])
        assert p[0].tolist() == pair[k].tolist() and d.tobytes() == d2[k:k + 1].tobytes(), k
    assert run_diameter(gpu_device, [])[0] == _lib.PGR_OK


# ---- the Python layer
def test_minimal_oriented_box_of_the_rotated_box(gpu_device):
    from pegasus_amd import obb
    pts, _ = OC.rotated_box()
    box = obb.minimal_oriented_box(pts, device=gpu_device)
    _, grow, shrink = OC.box_rounding_allowance(OC.BOX_DIMS, OC.box_corners_exact())
    exact = float(np.prod(OC.BOX_DIMS))
    print(f"rotated box: volume {box.volume!r} exact {exact!r} allowed -{shrink:.3g} +{np.prod(OC.BOX_DIMS + grow) - exact:.3g}")
    assert exact - shrink <= box.volume <= np.prod(OC.BOX_DIMS + grow)
    # an axis is within (7 kappa + 7) EPS of its direction (tests/obb_reference.py), kappa <= face diagonal / shortest edge
    # < 4.4 here: 38 EPS; two axes and the three roundings of their product: 79 -> 128 EPS
    assert np.abs(box.R.T @ box.R - np.eye(3)).max() <= 128 * OR.EPS and np.linalg.det(box.R) > 0
    corners, true = box.box_points(), OC.box_corners_exact()
    dist = np.linalg.norm(corners[:, None, :] - true[None, :, :], axis=2)
    nearest = dist.argmin(axis=1)
    assert sorted(nearest.tolist()) == list(range(8))                     # as a set: every true corner exactly once
    assert dist.min(axis=1).max() <= 3 * grow                             # `grow` per axis, three axes
    # contains: lohi is within q_bound of the projections this frame gives; rebuilding the centre (3 roundings on |a|-sized
    # sums), p - c (1) and the dot product (3) act on at most max |p|_1: 8 EPS of it
    hull_pts, hull_tri = obb.convex_hull(pts)
    q_bound = OR.candidates(hull_pts, hull_tri)[2]
    tol = q_bound[np.isfinite(q_bound)].max() + 8 * OR.EPS * np.abs(pts.astype(np.float64)).sum(axis=1).max()
    assert box.contains(pts, tol).all()
    assert not box.contains(pts + np.float32(1.0), 0.0).all()
    assert np.array_equal(box.ndds_corners(), corners[list(OR.NDDS_ORDER)])


def _reference_boxes_near_the_minimum(points, tris):
    """Every candidate whose reference volume is within the bound of the smallest: ties (an inversion-symmetric hull has
    them in pairs) may fall either way on the device."""
    lohi, vol, q_bound = OR.candidates(points, tris)
    v_bound = OR.volume_bound(lohi, q_bound)
    r = OR.argmin_finite(vol)
    near = np.nonzero(np.isfinite(vol) & (vol - vol[r] <= v_bound + v_bound[r]))[0]
    return [(OR.box(points, tris[f], lohi[f]), q_bound[f]) for f in near]


def test_boxes_for_a_mesh_set_and_the_scene_gt_fields(gpu_device):
    from scipy.spatial import ConvexHull
    from pegasus_amd import bop_pose, obb
    from pegasus_amd.mesh_render import MeshSet
    ico_v, ico_f = OC.affine_icosphere(2, offset=(0.01, -0.02, 0.03))
    box_v, box_f = OC.rotated_box()
    inner = OC.split_case()[0][8:400]                                      # a cloud round the box: a hull without symmetry
    meshes = MeshSet({3: SimpleNamespace(vertices=ico_v * 1000, faces=ico_f),
                      7: SimpleNamespace(vertices=np.concatenate([box_v, inner]), faces=box_f)}, device=gpu_device, scale=0.001)
    boxes = obb.boxes_for(meshes)
    assert sorted(boxes) == [3, 7]
    K = bop_pose.camera_K(0.9, 0.7, 640, 480)
    R_c2w, t_w2c = OC.rotation(21), np.array([0.1, -0.2, 2.5])
    poses = {3: np.eye(4), 7: np.eye(4)}
    poses[3][:3, :3], poses[3][:3, 3] = OC.rotation(22), [0.2, 0.1, 0.0]
    poses[7][:3, 3] = -meshes.mesh(7)[0].astype(np.float64).mean(0)
    entries = {e["bullet_obj_id"]: e for e in bop_pose.scene_gt_entry(R_c2w, t_w2c, poses, K=K, boxes=boxes)}
    for obj_id in (3, 7):
        verts = meshes.mesh(obj_id)[0]
        hull = ConvexHull(verts.astype(np.float64), qhull_options="QJ")
        index = np.full(len(verts), -1)
        index[hull.vertices] = np.arange(len(hull.vertices))
        hv, ht = verts[hull.vertices], index[hull.simplices]
        corners, mean, center = boxes[obj_id]
        assert np.array_equal(mean, verts.astype(np.float64).mean(0))
        scale = np.abs(verts.astype(np.float64)).sum(axis=1).max()
        matches = [3 * qb + 16 * OR.EPS * scale for (c, R, e), qb in _reference_boxes_near_the_minimum(hv, ht)
                   if np.abs(OR.ndds_corners(c, R, e) - corners).max() <= 3 * qb + 16 * OR.EPS * scale
                   and np.abs(c - center).max() <= 3 * qb + 16 * OR.EPS * scale]
        assert matches, obj_id
        e = entries[obj_id]
        T = bop_pose.world_to_camera(R_c2w, t_w2c) @ poses[obj_id]
        assert np.array_equal(np.array(e["3d_bounding_box_model_coord"]), corners)
        assert np.array_equal(np.array(e["3d_bounding_center"]), mean)
        assert np.array_equal(np.array(e["projected_points"]), bop_pose.project_points(K, T, corners))
        assert np.array_equal(np.array(e["projected_center"]), bop_pose.project_points(K, T, center[None]))
        assert not np.array_equal(np.array(e["projected_center"]), bop_pose.project_points(K, T, mean[None]))


def test_the_python_layer_refuses_what_the_kernels_would_not_check(gpu_device):
    from pegasus_amd import obb
    pts, tri = OC.tetrahedron()
    bad = tri.copy()
    bad[0, 0] = 4
    with pytest.raises(ValueError, match="outside"):
        obb.candidate_boxes([pts], [bad], gpu_device)
    with pytest.raises(ValueError, match="finite"):
        obb.minimal_oriented_box(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, np.nan]], np.float32), device=gpu_device)
    with pytest.raises(ValueError, match="hull"):
        obb.minimal_oriented_box(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32), device=gpu_device)
    with pytest.raises(RuntimeError, match="HIP device"):
        obb.candidate_boxes([pts], [tri], "cpu")
    ico = OC.affine_icosphere(1)[0]
    a, b = obb.from_mesh(SimpleNamespace(vertices=ico), device=gpu_device), obb.minimal_oriented_box(ico, True, gpu_device)
    assert np.array_equal(a.box_points(), b.box_points())                 # from_mesh: the vertices, robust hull
    q_bound = OR.candidates(*obb.convex_hull(ico, True))[2]               # as in the rotated-box test above
    assert a.contains(ico, q_bound.max() + 8 * OR.EPS * np.abs(ico.astype(np.float64)).sum(axis=1).max()).all()
    assert obb.diameter(pts, device=gpu_device) == pytest.approx(np.sqrt(OR.diameter(pts)[0]), rel=1e-15)
    assert obb.diameter(OC.ball_cloud(3000), hull=True, device=gpu_device) == obb.diameter(OC.ball_cloud(3000), hull=False,
                                                                                            device=gpu_device)
