"""Camera refinement while training (``--pose_lr``): the 32-view cube dataset of tests/test_train_gpu.py with every training
pose perturbed (seeded, 1 degree about a random axis and 1 % of the distance), trained with 4 views per step for 2000 steps
with and without pose refinement.  With it the median rotation error of the training cameras -- after the best similarity
alignment (Umeyama) of their centres to the true ones: joint refinement is free to move the whole rig -- is at most half
the initial one, the train PSNR is higher, cameras_refined.json loads and the model opens with Scene(load_iteration=-1)."""
import json
import math
import random
from types import SimpleNamespace

import numpy as np
import pytest

from test_train_gpu import _write_dataset

pytestmark = pytest.mark.gpu
DIST = 3.0


def _perturb(src, seed=11):
    from pegasus_amd import colmap_io as cio
    cams, imgs = cio.read_model(str(src))
    d = cio._sparse_dir(str(src))
    xyz, rgb = cio.read_points3D_binary(d / "points3D.bin")
    rng = np.random.default_rng(seed)
    true, out = {}, {}
    for k, im in imgs.items():
        R, t = cio.qvec2rotmat(im.qvec), np.asarray(im.tvec, np.float64)
        true[im.name.split(".")[0]] = (R, t)
        ax = rng.normal(size=3)
        ax *= math.radians(1.0) / np.linalg.norm(ax)
        th = np.linalg.norm(ax)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]]) / th
        dR = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
        dt = rng.normal(size=3)
        dt *= 0.01 * DIST / np.linalg.norm(dt)
        out[k] = cio.ColmapImage(im.id, cio.rotmat2qvec(dR @ R), dR @ t + dt, im.camera_id, im.name)
    cio.write_colmap_model(d, cams, out, xyz, rgb, binary=True)
    return true


def _umeyama(src, dst):
    """(s, Q, t) minimising |dst - (s Q src + t)|^2 over similarity transforms."""
    mu_s, mu_d = src.mean(0), dst.mean(0)
    xs, xd = src - mu_s, dst - mu_d
    U, S, Vt = np.linalg.svd(xd.T @ xs / len(src))
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1
    Q = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / xs.var(0).sum()
    return s, Q, mu_d - s * Q @ mu_s


def _median_rotation_error(poses, true):
    """poses / true: {name: (R_w2c, t_w2c)}; the median angle (degrees) after aligning the centres."""
    names = sorted(true)
    centre = lambda R, t: -R.T @ t
    src = np.stack([centre(*poses[n]) for n in names])
    dst = np.stack([centre(*true[n]) for n in names])
    _, Q, _ = _umeyama(src, dst)
    errs = []
    for n in names:
        M = true[n][0].T @ poses[n][0] @ Q.T
        errs.append(math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(M) - 1) / 2)))))
    return float(np.median(errs))


def test_training_refines_perturbed_camera_poses(gpu_device, tmp_path):
    import torch
    from pegasus_amd import colmap_io as cio
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.scene import Scene
    from pegasus_amd.train import training
    src = tmp_path / "data"
    _write_dataset(src, gpu_device)
    true = _perturb(src)
    start = {c.image_name: (c.R.T, c.T) for c in cio.camera_infos(str(src))}
    initial = _median_rotation_error(start, true)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    res = {}
    for pose_lr in (0.0, 1e-4):
        random.seed(0)
        torch.manual_seed(0)
        out = tmp_path / f"model_{pose_lr}"
        dataset = SimpleNamespace(sh_degree=3, source_path=str(src), model_path=str(out), images="images", resolution=-1,
                                  white_background=False, data_device="cuda", eval=False)
        opt = SimpleNamespace(iterations=2000, densify_from_iter=100, densify_until_iter=1500, densification_interval=100,
                              position_lr_max_steps=2000, pose_lr=pose_lr)
        res[pose_lr] = training(dataset, opt, pipe, [2000], [2000], [2000], None, -1, quiet=True, batch_size=4)
    plain, refined = res[0.0], res[1e-4]
    assert "refined_cameras" not in plain
    assert not (tmp_path / "model_0.0" / "cameras_refined.json").exists()
    assert not (tmp_path / "model_0.0" / "chkpnt2000_poses.pth").exists()
    out = tmp_path / "model_0.0001"
    poses = {c.image_name: (np.asarray(c.R).T, np.asarray(c.T)) for c in refined["refined_cameras"]}
    after = _median_rotation_error(poses, true)
    p0, p1 = plain["reports"][2000]["train"]["psnr"], refined["reports"][2000]["train"]["psnr"]
    print(f"\nPOSE-TRAIN median rotation error {initial:.3f} -> {after:.3f} deg; train PSNR {p0:.2f} (plain) vs {p1:.2f} dB")
    assert after <= 0.5 * initial, (initial, after)
    assert p1 > p0, (p0, p1)
    cams = json.loads((out / "cameras_refined.json").read_text())
    assert len(cams) == 32 and {"position", "rotation", "fx", "fy", "img_name"} <= set(cams[0])
    deltas = torch.load(out / "chkpnt2000_poses.pth", weights_only=False)
    assert len(deltas) == 32 and all(tuple(d.shape) == (6,) for d in deltas.values())
    g = GaussianModel(3)
    scene = Scene(SimpleNamespace(model_path=str(out), data_device="cuda"), g, load_iteration=-1)
    assert scene.loaded_iter == 2000 and g.get_xyz.shape[0] == refined["num_gaussians"]
