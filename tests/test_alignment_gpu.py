"""Ground-plane alignment on the device against the float64 brute force of tests/alignment_reference.py (DESIGN.md section
18).  Hypotheses: planes bit for bit, validity equal, no row outside the points read.  Scores and the inlier pass: counts and
masks equal, sums within 1e-12 of the sum of the absolute terms, equal bytes from call to call, at every launch edge (one
point, the wave, the tile, several workgroups, the hypothesis batch).  End to end: the choice, the inlier set, the refitted
normal to |n . n_ref| >= 1 - 1e-10, the 4x4 within the reference's own error.  A Gaussian model under a similarity renders
what it rendered before through the transformed camera."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import alignment_cases as AC             # noqa: E402
import alignment_reference as AR         # noqa: E402

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-12                          # of the sum of the absolute terms (DESIGN.md section 17's bar for this reduction)


def dev_t(dev, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)            # (a copy: the cases are read-only)


def _assert_sums(got, want, mag):
    got, want, mag = (np.asarray(a, dtype=np.float64) for a in (got, want, mag))
    err = np.abs(got - want)
    used = err[mag > 0] / (SUM_TOL * mag[mag > 0])
    print("largest sum error as a share of what is allowed:", float(used.max(initial=0.0)))
    assert (err <= SUM_TOL * mag).all(), (err, SUM_TOL * mag)


# ---- hypotheses
@pytest.mark.parametrize("n_hyp", AC.HYPOTHESIS_HS)
def test_hypotheses_are_the_references_bit_for_bit(gpu_device, n_hyp):
    from pegasus_amd import alignment
    points = AC.scene(1025)[0]
    tri = AC.triples(len(points), n_hyp)
    want, want_valid = AR.hypotheses(points, tri)
    planes, valid = alignment.plane_hypotheses(dev_t(gpu_device, points), tri)
    assert planes.shape == (n_hyp, 4) and valid.shape == (n_hyp,)
    np.testing.assert_array_equal(valid.cpu().numpy(), want_valid)
    assert planes.cpu().numpy().tobytes() == want.tobytes()
    assert want_valid.sum() >= n_hyp - 2


def test_degenerate_hypotheses_are_invalid_and_read_nothing(gpu_device):
    """Repeated rows, collinear and coincident points, rows -1, n, INT_MIN and INT_MAX: four zeros and valid = 0.  The points
    are handed over as the leading rows of a larger buffer filled with NaN, so a read of row n would show; rows far outside
    would fault."""
    import torch
    from pegasus_amd import alignment
    n = 257
    points = AC.degenerate_points(n)
    tri = AC.degenerate_triples(n)
    want, want_valid = AR.hypotheses(points, tri)
    assert want_valid.tolist() == [0] * 13 + [1, 0]
    padded = torch.full((n + 64, 3), math.nan, dtype=torch.float32, device=gpu_device)
    padded[:n] = dev_t(gpu_device, points)
    planes, valid = alignment.plane_hypotheses(padded[:n], tri)
    np.testing.assert_array_equal(valid.cpu().numpy(), want_valid)
    assert planes.cpu().numpy().tobytes() == want.tobytes()
    # such planes score nothing
    counts, sumsq = alignment.plane_scores(padded[:n], planes, AC.THRESHOLD)
    ref = AR.scores(points, want, AC.THRESHOLD)
    np.testing.assert_array_equal(counts.cpu().numpy(), ref.counts)
    assert not counts.cpu().numpy()[want_valid == 0].any() and not sumsq.cpu().numpy()[want_valid == 0].any()
    # no points at all: every triple is outside
    planes, valid = alignment.plane_hypotheses(padded[:0], tri)
    assert not planes.cpu().numpy().any() and not valid.cpu().numpy().any()


# ---- scores
def _check_scores(gpu_device, points, planes, ref):
    from pegasus_amd import alignment
    pts, pl = dev_t(gpu_device, points), dev_t(gpu_device, planes)
    counts, sumsq = alignment.plane_scores(pts, pl, AC.THRESHOLD)
    assert counts.dtype.itemsize == 4 and sumsq.dtype.itemsize == 8
    np.testing.assert_array_equal(counts.cpu().numpy(), ref.counts)
    _assert_sums(sumsq.cpu().numpy(), ref.sumsq, ref.sumsq)
    again_counts, again_sumsq = alignment.plane_scores(pts, pl, AC.THRESHOLD)
    assert again_counts.cpu().numpy().tobytes() == counts.cpu().numpy().tobytes()
    assert again_sumsq.cpu().numpy().tobytes() == sumsq.cpu().numpy().tobytes()


@pytest.mark.parametrize("n", AC.SCORE_NS)
def test_scores_at_the_point_edges(gpu_device, n):
    points, planes, ref = AC.score_case(n, AC.SCORE_H)
    assert len(points) == n and len(planes) == AC.SCORE_H
    _check_scores(gpu_device, points, planes, ref)


@pytest.mark.parametrize("n_hyp", AC.BATCH_HS)
def test_scores_at_the_batch_edges(gpu_device, n_hyp):
    points, planes, ref = AC.score_case(AC.BATCH_N, n_hyp, source=(AC.BATCH_N, AC.SCORE_H))
    assert len(planes) == n_hyp and ref.counts.max() > 10
    _check_scores(gpu_device, points, planes, ref)


@pytest.mark.parametrize("blocks", AC.FINAL_BLOCKS)
def test_scores_over_several_workgroups(gpu_device, blocks):
    points, planes, ref = AC.final_case(blocks)
    assert len(points) == (blocks - 1) * AC.TILE + 1 and len(planes) == AC.FINAL_H
    _check_scores(gpu_device, points, planes, ref)


def test_scores_over_several_batches_in_one_workgroup(gpu_device):
    """Few tiles and many hypotheses: every workgroup walks two batches through the same LDS, the last one a full batch and
    then a batch of one hypothesis.  (Up to PLANE_SCORE_MIN_BLOCKS / tiles batches every group has one batch of its own, which
    is all the other cases reach.)  The default of 1000 hypotheses takes this path from about 131 k points on."""
    points, planes, ref = AC.grouped_case()
    tiles, per_group, groups = AC.score_launch(len(points), len(planes))
    assert (tiles, per_group) == (max(AC.FINAL_BLOCKS), 2) and len(planes) % AC.PLANE_HYP_BATCH == 1
    assert AC.score_launch(1_360_000, 1000)[1] >= 2 and AC.score_launch(150_000, 1000)[1] >= 2
    assert (ref.counts > 0).mean() > 0.9 and ref.counts[-1] > 0 and ref.counts[-2] > 0
    _check_scores(gpu_device, points, planes, ref)


def test_zero_planes_and_no_points_score_nothing(gpu_device):
    import torch
    from pegasus_amd import alignment
    points, planes, ref = AC.score_case(65, AC.SCORE_H)
    planes = np.array(planes)
    planes[[0, 7, 64]] = 0.0
    counts, sumsq = alignment.plane_scores(dev_t(gpu_device, points), dev_t(gpu_device, planes), AC.THRESHOLD)
    want = ref.counts.copy()
    want[[0, 7, 64]] = 0
    assert ref.counts[7] > 0
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    assert not sumsq.cpu().numpy()[[0, 7, 64]].any()
    empty = torch.empty((0, 3), dtype=torch.float32, device=gpu_device)
    counts, sumsq = alignment.plane_scores(empty, dev_t(gpu_device, planes), AC.THRESHOLD)
    assert not counts.cpu().numpy().any() and not sumsq.cpu().numpy().any()


def test_the_comparison_is_strict(gpu_device):
    from pegasus_amd import alignment
    points, tri, threshold, want = AC.strictness()
    pts = dev_t(gpu_device, points)
    planes, valid = alignment.plane_hypotheses(pts, tri)
    assert valid.cpu().numpy().tolist() == [1] and planes.cpu().numpy().tolist() == [[0, 0, 1, 0]]
    counts, sumsq = alignment.plane_scores(pts, planes, threshold)
    assert counts.cpu().numpy().tolist() == [int(want.sum())]
    mask, sums = alignment.plane_inliers(pts, [0, 0, 1, 0], [0, 0, 0], threshold)
    np.testing.assert_array_equal(mask.cpu().numpy(), want)
    z2 = (points[want == 1, 2].astype(np.float64) ** 2)
    assert sumsq.cpu().numpy()[0] == pytest.approx(z2.sum(), rel=1e-15) == sums.cpu().numpy()[AR.SUM_D2]


# ---- the inlier pass
@pytest.mark.parametrize("n", AC.SCORE_NS)
def test_inlier_pass_at_the_point_edges(gpu_device, n):
    from pegasus_amd import alignment
    points, plane, pivot, ref = AC.inlier_case(n)
    pts = dev_t(gpu_device, points)
    mask, sums = alignment.plane_inliers(pts, plane, pivot, AC.THRESHOLD)
    np.testing.assert_array_equal(mask.cpu().numpy(), ref.mask)
    got = sums.cpu().numpy()
    assert got[AR.COUNT] == ref.sums[AR.COUNT] == ref.mask.sum() and got[11] == 0.0
    _assert_sums(got, ref.sums, ref.mag)
    none, without = alignment.plane_inliers(pts, plane, pivot, AC.THRESHOLD, return_mask=False)      # mask = NULL
    assert none is None and without.cpu().numpy().tobytes() == got.tobytes()
    _, again = alignment.plane_inliers(pts, plane, pivot, AC.THRESHOLD)
    assert again.cpu().numpy().tobytes() == got.tobytes()


def test_inlier_pass_of_a_zero_plane_and_of_no_points(gpu_device):
    import torch
    from pegasus_amd import alignment
    points, plane, pivot, _ = AC.inlier_case(65)
    mask, sums = alignment.plane_inliers(dev_t(gpu_device, points), [0, 0, 0, 0], pivot, AC.THRESHOLD)
    assert not mask.cpu().numpy().any() and not sums.cpu().numpy().any()
    empty = torch.empty((0, 3), dtype=torch.float32, device=gpu_device)
    mask, sums = alignment.plane_inliers(empty, plane, pivot, AC.THRESHOLD)
    assert mask.shape == (0,) and not sums.cpu().numpy().any()


# ---- end to end
@pytest.mark.parametrize("shape", AC.END_TO_END)
def test_fit_ground_plane_end_to_end(gpu_device, shape):
    from pegasus_amd import alignment
    n, h = shape
    points, known, _, offset = AC.scene(n)
    ref = AC.reference_fit(n, h)
    fit = alignment.fit_ground_plane(dev_t(gpu_device, points), AC.THRESHOLD, h, AC.TRIPLE_SEED,
                                     camera_centers=AC.cameras_above(n))
    assert fit.best_index == ref.best_index
    assert fit.hypothesis_plane.tobytes() == ref.hypothesis_plane.tobytes()
    assert fit.hypothesis_count == ref.hypothesis_count and fit.count == ref.count
    np.testing.assert_array_equal(fit.inliers.cpu().numpy(), ref.inliers)
    assert fit.inliers.dtype.itemsize == 8
    assert fit.fitness == ref.fitness and fit.inlier_rmse == pytest.approx(ref.inlier_rmse, rel=1e-12)
    alignment_of_normals = float(fit.plane[:3] @ ref.plane[:3])
    print("n . n_ref - 1:", alignment_of_normals - 1.0, "eigen-gap ratio", ref.eigen_gap)
    assert alignment_of_normals >= 1 - 1e-10
    T = alignment.plane_transformation(fit, AC.SCALE)
    diff = float(np.abs(T - ref.transformation).max())
    print("largest |T - T_ref|:", diff, "allowed", AC.T_TOL)
    assert diff <= AC.T_TOL
    np.testing.assert_array_equal(T[3], [0, 0, 0, 1])
    # the known plane
    angle, off = AR.plane_angle_deg(fit.plane, known), abs(float(fit.plane[:3] @ offset + fit.plane[3]))
    print("against the known plane:", angle, "degrees,", off * 1e3, "mm")
    assert angle < AC.PLANE_DEG_MAX and off < AC.PLANE_M_MAX
    # the ground lands on z = 0 and the scene is centred over it
    moved = points[ref.inliers].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert np.abs(moved[:, 2]).max() < AC.SCALE * AC.THRESHOLD and np.abs(moved[:, :2].mean(axis=0)).max() < 1e-9


def test_segment_plane_and_orientation(gpu_device):
    from pegasus_amd import alignment
    n, h = AC.END_TO_END[1]
    points, known, _, _ = AC.scene(n)
    pts = dev_t(gpu_device, points)
    above = AC.cameras_above(n)
    up = alignment.fit_ground_plane(pts, AC.THRESHOLD, h, AC.TRIPLE_SEED, camera_centers=above)
    assert float(up.plane[:3] @ known[:3]) > 0.999                       # cameras above the ground: their side is up
    T = alignment.plane_transformation(up)
    assert ((above @ T[:3, :3].T + T[:3, 3])[:, 2] > 0.9).all()            # +z after alignment
    down = alignment.fit_ground_plane(pts, AC.THRESHOLD, h, AC.TRIPLE_SEED, plane_normal=-known[:3], camera_centers=above)
    np.testing.assert_array_equal(down.plane, -up.plane)                  # a plane_normal the other way flips it
    T = alignment.plane_transformation(down)
    assert ((above @ T[:3, :3].T + T[:3, 3])[:, 2] < -0.9).all()
    same = alignment.fit_ground_plane(pts, AC.THRESHOLD, h, AC.TRIPLE_SEED, plane_normal=known[:3])
    np.testing.assert_array_equal(same.plane, up.plane)
    # open3d's call shape, oriented by the largest component
    model, inliers = alignment.segment_plane(pts, AC.THRESHOLD, 3, h, AC.TRIPLE_SEED)
    lead = model[int(np.argmax(np.abs(model[:3])))]
    assert lead > 0 and (np.array_equal(model, up.plane) or np.array_equal(model, -up.plane))
    np.testing.assert_array_equal(inliers.cpu().numpy(), up.inliers.cpu().numpy())
    # no valid hypothesis is an error
    with pytest.raises(ValueError, match="hypotheses"):
        alignment.fit_ground_plane(dev_t(gpu_device, np.tile(points[:1], (50, 1))), AC.THRESHOLD, 20, 0)
    with pytest.raises(ValueError, match="finite"):
        bad = np.array(points[:50])
        bad[7, 1] = np.inf
        alignment.fit_ground_plane(dev_t(gpu_device, bad), AC.THRESHOLD, 20, 0)


# ---- a Gaussian model under a similarity
def _render(model, view, dev):
    import torch
    from pegasus_amd import rasterizer
    spec = rasterizer.ViewSpec(view.height, view.width, view.tanfovx, view.tanfovy, torch.zeros(3, device=dev),
                               *(torch.from_numpy(a).to(dev) for a in
                                 (view.world_view_transform, view.full_proj_transform, view.camera_center)))
    r = rasterizer.forward_views(model.get_xyz, model.get_opacity, [spec], shs=model.get_features, scales=model.get_scaling,
                                 rotations=model.get_rotation, sh_degree=3)[0]
    torch.cuda.synchronize()
    return r["color"].cpu().numpy(), r["depth"].cpu().numpy()


def test_transform_model_renders_the_same_through_the_transformed_camera(gpu_device):
    import torch
    from scipy.spatial.transform import Rotation as Rot
    from pegasus_amd import alignment, graphics, scenes
    from pegasus_amd.gaussian_model import GaussianModel
    s = AC.SCALE
    rng = np.random.default_rng(41)
    cloud = scenes.box_object(rng, 6000, (0.3, 0.2, 0.25), math.log(0.006), 0.3, 0.2, 1)
    model = GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling,
                                      cloud.rotation, device=gpu_device)
    T = np.eye(4)
    R = Rot.from_rotvec([0.4, -0.7, 0.5]).as_matrix()
    T[:3, :3], T[:3, 3] = s * R, [0.3, -0.2, 0.45]
    moved = alignment.transform_model(model, T)
    # log-scales by exactly ln s in float32; opacity and DC colour untouched; the source model is not changed
    want_scaling = model._scaling + torch.tensor(np.float32(math.log(s)), device=gpu_device)
    assert torch.equal(moved._scaling, want_scaling) and moved._scaling.dtype == torch.float32
    assert torch.equal(moved._opacity, model._opacity) and torch.equal(moved._features_dc, model._features_dc)
    np.testing.assert_array_equal(model._xyz.cpu().numpy(), cloud.xyz)
    want_xyz = cloud.xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert np.abs(moved._xyz.cpu().numpy() - want_xyz).max() < 1e-5
    # camera C, 1.2 m from the box; the transformed camera sees camera space scaled by s
    R_w2c, t_w2c = graphics.look_at_opencv((0.7, -0.8, 0.55), (0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))
    R_new = np.asarray(R_w2c) @ R.T
    t_new = s * np.asarray(t_w2c) - R_new @ T[:3, 3]
    view = scenes.make_view(R_w2c, t_w2c, 200, 160, fx=600.0, fy=600.0)
    view_new = scenes.make_view(R_new, t_new, 200, 160, fx=600.0, fy=600.0)
    depth_of = lambda xyz, Rm, t: (xyz @ np.asarray(Rm).T + t)[:, 2]
    assert depth_of(cloud.xyz.astype(np.float64), R_w2c, t_w2c).min() > 0.2 * max(1.0, s)       # the near cull decides nothing
    assert depth_of(want_xyz, R_new, t_new).min() > 0.2 * max(1.0, s)
    color, depth = _render(model, view, gpu_device)
    color_new, depth_new = _render(moved, view_new, gpu_device)
    print("mean |d color|", float(np.abs(color_new - color).mean()), "mean |d depth / s|", float(np.abs(depth_new / s - depth).mean()))
    assert (color > 0.05).mean() > 0.2 and (depth > 0.2).mean() > 0.1                           # visible content
    assert np.abs(color_new - color).mean() < 1e-4
    assert np.abs(depth_new / s - depth).mean() < 1e-4
    # and it is the rotation that does it: the unrotated SH of the source would not
    assert np.abs(moved._features_rest.cpu().numpy() - cloud.features_rest).max() > 1e-2


# ---- the command line, both forms
def _posed_ground_scene(n_ground=3000, n_box=1500, seed=53):
    """A SplatCloud of a 2 x 2 m ground (+-4 mm) with a box on it, posed by scene(1025)'s rotation and offset; and that pose."""
    from pegasus_amd import scenes
    rng = np.random.default_rng(seed)
    ground = scenes.ground_plane(rng, n_ground, 2.0, math.log(0.01), 0.3, 0.1, 0.004)
    box = scenes.rigid_transform(scenes.box_object(rng, n_box, (0.2, 0.3, 0.25), math.log(0.01), 0.3, 0.2, 1), np.eye(3),
                                 np.array([0.3, -0.2, 0.125 + 0.02]))
    _, _, R, offset = AC.scene(1025)
    return scenes.rigid_transform(scenes.SplatCloud.concat([ground, box]), np.array(R), np.array(offset)), R, offset


def test_command_line_aligns_and_crops_a_model(gpu_device, tmp_path, capsys):
    from pegasus_amd import alignment
    from pegasus_amd.gaussian_model import GaussianModel
    cloud, R, offset = _posed_ground_scene()
    GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling, cloud.rotation,
                              device=gpu_device).save_ply(tmp_path / "in.ply")
    up = (R @ np.array([0.0, 0.0, 1.0])).tolist()
    args = ["--model", str(tmp_path / "in.ply"), "--out", str(tmp_path / "out" / "aligned.ply"), "--min_opacity", "0",
            "--iterations", "128", "--seed", "3", "--scale", "2", "--plane_normal", *map(str, up)]
    assert alignment.main(args) == 0
    assert "fitness" in capsys.readouterr().out
    whole = GaussianModel(3, gpu_device)
    whole.load_ply(tmp_path / "out" / "aligned.ply")
    xyz = whole.get_xyz.cpu().numpy()
    assert len(xyz) == len(cloud.xyz)
    T = np.loadtxt(tmp_path / "out" / "aligned.transformation.txt")
    assert np.abs(xyz - (cloud.xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3])).max() < 1e-5
    ground, box = xyz[:3000], xyz[3000:]
    assert np.abs(ground[:, 2]).max() < 2 * 0.004 * 1.5                         # the ground on z = 0, in the scaled units
    assert box[:, 2].min() > 0.02 and box[:, 2].max() == pytest.approx(2 * 0.27, abs=0.01)       # the box above it, twice as tall
    # centred over the origin; the square's corners 2 * sqrt(2) m away (the rotation about z is whatever the smallest one leaves)
    assert np.abs(ground[:, :2].mean(axis=0)).max() < 0.1
    assert np.linalg.norm(ground[:, :2], axis=1).max() == pytest.approx(2.0 * math.sqrt(2.0), abs=0.2)
    assert alignment.main(args + ["--crop", "2.0"]) == 0
    cropped = GaussianModel(3, gpu_device)
    cropped.load_ply(tmp_path / "out" / "aligned.ply")
    kept = cropped.get_xyz.cpu().numpy()
    inside = (np.abs(xyz[:, :2]) <= 1.0).all(axis=1)
    assert 0.15 < inside.mean() < 0.6
    np.testing.assert_array_equal(kept, xyz[inside])


def test_command_line_aligns_a_colmap_project(gpu_device, tmp_path, capsys):
    import json
    from pegasus_amd import alignment, colmap_io, graphics
    from pegasus_amd.colmap_io import qvec2rotmat, rotmat2qvec
    n = 1025
    points, known, R, offset = AC.scene(n)
    cameras = {1: colmap_io.ColmapCamera(1, "PINHOLE", 640, 480, np.array([500.0, 500.0, 320.0, 240.0]))}
    images = {}
    for k, eye in enumerate(AC.cameras_above(n)):
        R_w2c, t_w2c = graphics.look_at_opencv(eye, offset, up=R[:, 2])
        images[k + 1] = colmap_io.ColmapImage(k + 1, rotmat2qvec(R_w2c), t_w2c, 1, f"{k}.png")
    rgb = np.full((n, 3), 128, dtype=np.uint8)
    colmap_io.write_colmap_model(tmp_path / "sparse" / "0", cameras, images, points.astype(np.float64), rgb)
    assert alignment.main(["--project", str(tmp_path), "--scale", str(AC.SCALE), "--iterations", "65",
                           "--seed", str(AC.TRIPLE_SEED)]) == 0
    assert "alignment.json written" in capsys.readouterr().out
    record = json.loads((tmp_path / "alignment.json").read_text())
    ref = AC.reference_fit(n, 65)                                # oriented by the same cameras, the same scale
    T = np.array(record["transformation"])
    camera_centres = np.array([-qvec2rotmat(im.qvec).T @ im.tvec for im in images.values()])
    np.testing.assert_allclose(camera_centres, AC.cameras_above(n), rtol=0, atol=1e-12)
    # (the centres went through a quaternion: they may differ from the reference's in the last bits, the orientation not)
    assert np.abs(T - ref.transformation).max() <= AC.T_TOL
    assert record["scale"] == AC.SCALE and record["plane_size"] == 2.0 and record["inliers"] == ref.count
    assert record["fitness"] == ref.fitness and record["best_index"] == ref.best_index
    xyz, _ = colmap_io.read_points3D_binary(tmp_path / "sparse" / "0" / "points3D.bin")
    np.testing.assert_allclose(xyz, points.astype(np.float64) @ T[:3, :3].T + T[:3, 3], rtol=0, atol=1e-12)
    assert np.abs(xyz[ref.inliers, 2]).max() < AC.SCALE * AC.THRESHOLD
    _, moved = colmap_io.read_model(tmp_path)
    for im in moved.values():                                    # the cameras look down from above
        assert (-qvec2rotmat(im.qvec).T @ im.tvec)[2] > 0.9 * AC.SCALE
    assert (tmp_path / "sparse" / "0_unaligned" / "points3D.bin").exists()
