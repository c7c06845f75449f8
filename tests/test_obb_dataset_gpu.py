"""The command lines around the minimal oriented boxes: ``generate --boxes oriented --gt-from-meshes`` writes the reference's
four box fields from the meshes' boxes, the default ``--boxes aabb`` writes what it wrote without the option, and
``python -m pegasus_amd.obb --dataset`` rewrites a dataset on disk to the same fields."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import obb_cases as OC                   # noqa: E402
import obb_reference as OR               # noqa: E402

pytestmark = pytest.mark.gpu

FLAGS = ["--frames", "2", "--batch", "2", "--workload", "c2", "--scale", "0.02", "--size", "96"]
BOX_FIELDS = ("3d_bounding_box_model_coord", "3d_bounding_center", "projected_points", "projected_center")


def _scene_gt(root):
    return json.loads((root / "train" / "000000" / "scene_gt.json").read_text())


def test_generate_with_oriented_boxes_and_the_dataset_rewrite(gpu_device, tmp_path):
    from pegasus_amd import bop_pose, generate, obb
    from pegasus_amd.mesh_render import MeshSet
    from pegasus_amd.ply_io import write_ply_mesh
    plain, default, oriented, models = (tmp_path / n for n in ("plain", "default", "oriented", "models"))
    generate.main(["--out", str(plain), *FLAGS])
    ids = sorted({e["obj_id"] for e in _scene_gt(plain)["0"]})
    assert ids
    models.mkdir()
    exact_mm = {k: OC.box_corners_exact(R=OC.rotation(50 + k), t=np.array([3.0, -2.0, 1.0]) * k) for k in ids}
    for k in ids:                                                          # a tilted box per object, in millimetres
        write_ply_mesh(models / f"obj_{k:06d}.ply", exact_mm[k].astype(np.float32), OC.BOX_TRIANGLES)
    generate.main(["--out", str(default), *FLAGS, "--gt-from-meshes", str(models), "--boxes", "aabb"])
    generate.main(["--out", str(oriented), *FLAGS, "--gt-from-meshes", str(models), "--boxes", "oriented"])
    gt_plain, gt_default, gt_oriented = _scene_gt(plain), _scene_gt(default), _scene_gt(oriented)
    assert gt_default == gt_plain                                          # the default boxes do not depend on the meshes
    boxes = obb.boxes_for(MeshSet.from_dir(models, device=gpu_device, scale=0.001))
    cam = json.loads((oriented / "train" / "000000" / "scene_camera.json").read_text())
    for image, entries in gt_oriented.items():
        K = np.array(cam[image]["cam_K"]).reshape(3, 3)
        for e, was in zip(entries, gt_plain[image]):
            assert {k: v for k, v in e.items() if k not in BOX_FIELDS} == {k: v for k, v in was.items() if k not in BOX_FIELDS}
            corners, mean, center = boxes[e["obj_id"]]
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = np.array(e["cam_R_m2c"]).reshape(3, 3), e["cam_t_m2c"]
            assert np.array_equal(np.array(e["3d_bounding_box_model_coord"]), corners)
            assert np.array_equal(np.array(e["3d_bounding_center"]), mean)
            for key, want in (("projected_points", bop_pose.project_points(K, T, corners)),
                              ("projected_center", bop_pose.project_points(K, T, center[None]))):
                # the same T and K element for element: only the order of a few float64 operations may differ
                assert np.abs(np.array(e[key]) - want).max() <= 64 * OR.EPS * np.abs(want).max(), key
            # the box is the mesh's own, in metres (the millimetre corners rounded to float32, scaled, rounded again)
            exact = exact_mm[e["obj_id"]] * 1e-3
            _, grow, shrink = OC.box_rounding_allowance(OC.BOX_DIMS * 1e-3, exact, roundings=2)
            dist = np.linalg.norm(corners[:, None] - exact[None], axis=2).min(axis=1)
            assert dist.max() <= 3 * grow
            R, extent = _frame(corners)
            V = np.prod(OC.BOX_DIMS * 1e-3)
            assert V - shrink <= np.prod(extent) <= np.prod(OC.BOX_DIMS * 1e-3 + grow)
            # NDDS order: the corners are c -+ x -+ y -+ z of their own frame in that order, to the rounding of rebuilding them
            assert np.abs(corners - OR.ndds_corners(center, R, extent)).max() <= 64 * OR.EPS * np.abs(corners).max()
    # the rewrite of a dataset on disk: from the default dataset to the oriented one's fields
    assert obb.main(["--models", str(models), "--dataset", str(default), "--robust"]) == 0
    rewritten = _scene_gt(default)
    for image, entries in gt_oriented.items():
        for e, r in zip(entries, rewritten[image]):
            assert list(r) == list(e)
            for key in e:
                a, b = np.array(r[key], float), np.array(e[key], float)
                assert np.abs(a - b).max() <= 64 * OR.EPS * max(1.0, np.abs(b).max()), key
    info = json.loads((models / "models_boxes.json").read_text())
    assert sorted(info) == [str(k) for k in ids]
    for k in ids:                                                          # the files' own units: millimetres
        delta, grow, shrink = OC.box_rounding_allowance(OC.BOX_DIMS, exact_mm[k])
        V = np.prod(OC.BOX_DIMS)
        assert V - shrink <= np.prod(info[str(k)]["extent"]) <= np.prod(OC.BOX_DIMS + grow)
        assert abs(info[str(k)]["diameter"] - np.linalg.norm(OC.BOX_DIMS)) <= 2 * delta       # both ends move by delta
        assert np.array(info[str(k)]["ndds_corners"]).shape == (8, 3) and np.array(info[str(k)]["R"]).shape == (3, 3)


def _frame(ndds):
    """(R, extent) read back from corners in NDDS order: rows 0, 4, 1, 3 are c-x-y-z, c+x-y-z, c-x+y-z, c-x-y+z."""
    axes = np.stack([ndds[4] - ndds[0], ndds[1] - ndds[0], ndds[3] - ndds[0]], axis=1)
    extent = np.linalg.norm(axes, axis=0)
    return axes / extent, extent
