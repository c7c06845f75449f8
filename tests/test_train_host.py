"""Training, host side (no GPU): COLMAP readers (.txt / .bin), camera conventions, the eval split, the camera extent,
the points3D -> PLY cache, the optimisation arguments and the position learning-rate schedule."""
import math
import sys
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """World-to-camera rotation (OpenCV axes: x right, y down, z forward) and translation of a camera at ``eye``."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R_w2c = np.stack([x, y, z])
    return R_w2c, -R_w2c @ eye


def synthetic_model(n_images=17, seed=0):
    from pegasus_amd import colmap_io as cio
    rng = np.random.default_rng(seed)
    cams = {1: cio.ColmapCamera(1, "PINHOLE", 64, 48, np.array([70.0, 72.5, 32.0, 24.0])),
            2: cio.ColmapCamera(2, "SIMPLE_PINHOLE", 40, 30, np.array([50.0, 20.0, 15.0]))}
    imgs, eyes = {}, []
    for k in range(n_images):
        eye = np.array([3.0 * math.cos(0.4 * k), 3.0 * math.sin(0.4 * k), 0.5 + 0.1 * k])
        R, t = _look_at(eye)
        eyes.append(eye)
        # ids deliberately out of name order: the readers sort by name
        imgs[100 - k] = cio.ColmapImage(100 - k, cio.rotmat2qvec(R), t, 1 + (k % 2), f"img_{k:03d}.png")
    xyz = rng.normal(size=(50, 3))
    rgb = rng.integers(0, 256, size=(50, 3)).astype(np.uint8)
    return cams, imgs, xyz, rgb, np.array(eyes)


def _write(tmp_path, name, binary):
    from pegasus_amd import colmap_io as cio
    cams, imgs, xyz, rgb, eyes = synthetic_model()
    src = tmp_path / name
    cio.write_colmap_model(src / "sparse" / "0", cams, imgs, xyz, rgb, binary=binary)
    return src, cams, imgs, xyz, rgb, eyes


def test_colmap_text_and_binary_read_back_the_same_cameras(tmp_path):
    from pegasus_amd import colmap_io as cio
    src_b = _write(tmp_path, "bin", True)[0]
    src_t = _write(tmp_path, "txt", False)[0]
    assert (src_b / "sparse/0/images.bin").exists() and (src_t / "sparse/0/images.txt").exists()
    cb, ib = cio.read_model(src_b)
    ct, it = cio.read_model(src_t)
    assert cb.keys() == ct.keys() and ib.keys() == it.keys()
    for k in cb:
        assert (cb[k].model, cb[k].width, cb[k].height) == (ct[k].model, ct[k].width, ct[k].height)
        np.testing.assert_array_equal(cb[k].params, ct[k].params)
    for k in ib:
        assert (ib[k].name, ib[k].camera_id) == (it[k].name, it[k].camera_id)
        np.testing.assert_array_equal(ib[k].qvec, it[k].qvec)
        np.testing.assert_array_equal(ib[k].tvec, it[k].tvec)
    infos_b, infos_t = cio.camera_infos(src_b), cio.camera_infos(src_t)
    assert [c.image_name for c in infos_b] == [c.image_name for c in infos_t] == [f"img_{k:03d}" for k in range(17)]
    for a, b in zip(infos_b, infos_t):
        np.testing.assert_array_equal(a.R, b.R)
        np.testing.assert_array_equal(a.T, b.T)
        assert (a.FoVx, a.FoVy, a.width, a.height, a.uid) == (b.FoVx, b.FoVy, b.width, b.height, b.uid)
    xb, rb = cio.read_points3D_binary(src_b / "sparse/0/points3D.bin")
    xt, rt = cio.read_points3D_text(src_t / "sparse/0/points3D.txt")
    np.testing.assert_array_equal(xb, xt)
    np.testing.assert_array_equal(rb, rt)


def test_camera_conventions_split_and_extent(tmp_path):
    import torch
    from pegasus_amd import colmap_io as cio
    from pegasus_amd.cameras import Camera
    src, cams, imgs, _, _, eyes = _write(tmp_path, "bin", True)
    infos = cio.camera_infos(src)
    for k, info in enumerate(infos):
        R_w2c, t = _look_at(eyes[k])
        np.testing.assert_allclose(info.R, R_w2c.T, atol=1e-12)               # R: camera-to-world
        np.testing.assert_allclose(info.T, t, atol=1e-12)                     # T: world-to-camera translation
        cam = cams[1 + (k % 2)]
        fx, fy = (cam.params[0], cam.params[1]) if cam.model == "PINHOLE" else (cam.params[0], cam.params[0])
        assert info.FoVx == pytest.approx(2 * math.atan(cam.width / (2 * fx)), rel=1e-12)
        assert info.FoVy == pytest.approx(2 * math.atan(cam.height / (2 * fy)), rel=1e-12)
        c = Camera(colmap_id=info.uid, R=info.R, T=info.T, FoVx=info.FoVx, FoVy=info.FoVy, image=None,
                   gt_alpha_mask=None, image_name=info.image_name, uid=info.uid, data_device="cpu",
                   image_width=info.width, image_height=info.height)
        np.testing.assert_allclose(c.camera_center.double().numpy(), eyes[k], atol=1e-4)
        # a point straight ahead of the camera lands in front of it (positive view-space z)
        p = torch.tensor([0.0, 0.0, 0.0, 1.0]) @ c.world_view_transform
        assert float(p[2]) > 0
    train, test = cio.split_train_test(infos, True)
    assert [c.image_name for c in test] == ["img_000", "img_008", "img_016"]
    assert len(train) == 14 and not {c.image_name for c in train} & {c.image_name for c in test}
    assert cio.split_train_test(infos, False) == (infos, [])
    expect = 1.1 * np.linalg.norm(eyes - eyes.mean(0), axis=1).max()
    assert cio.camera_extent(infos) == pytest.approx(expect, rel=1e-6)      # (getWorld2View2 is fp32)


def test_unsupported_camera_models_raise(tmp_path):
    from pegasus_amd import colmap_io as cio
    cams, imgs, xyz, rgb, _ = synthetic_model(3)
    cams[2] = cio.ColmapCamera(2, "OPENCV", 40, 30, np.array([50.0, 50.0, 20.0, 15.0, 0.1, 0.0, 0.0, 0.0]))
    for binary in (True, False):
        d = tmp_path / ("b" if binary else "t")
        cio.write_colmap_model(d / "sparse" / "0", cams, imgs, xyz, rgb, binary=binary)
        with pytest.raises(cio.UnsupportedCameraModel, match="OPENCV"):
            cio.camera_infos(d)


def test_points3d_ply_cache_round_trip(tmp_path):
    from pegasus_amd import colmap_io as cio
    src, _, _, xyz, rgb, _ = _write(tmp_path, "txt", False)
    ply = src / "sparse/0/points3D.ply"
    assert not ply.exists()
    pcd = cio.fetch_point_cloud(src)
    assert ply.exists()
    np.testing.assert_allclose(pcd.points, xyz.astype(np.float32), rtol=0, atol=0)
    np.testing.assert_allclose(pcd.colors, rgb.astype(np.float32) / 255.0, rtol=1e-7)
    (src / "sparse/0/points3D.txt").unlink()                  # the cache alone serves the second read
    again = cio.fetch_point_cloud(src)
    np.testing.assert_array_equal(again.points, pcd.points)
    np.testing.assert_array_equal(again.colors, pcd.colors)


def test_load_camera_resolution_and_alpha(tmp_path):
    from PIL import Image
    from pegasus_amd import colmap_io as cio
    src, *_ = _write(tmp_path, "bin", True)
    info = cio.camera_infos(src)[0]                            # PINHOLE 64 x 48
    (src / "images").mkdir()
    a = np.zeros((48, 64, 4), dtype=np.uint8)
    a[..., 0] = 200
    a[:, :32, 3] = 255                                         # left half opaque red, right half transparent
    Image.fromarray(a, "RGBA").save(src / "images" / "img_000.png")
    full = cio.load_camera(info, -1, white_background=True, data_device="cpu")
    assert tuple(full.original_image.shape) == (3, 48, 64)
    assert float(full.original_image[0, 0, 0]) == pytest.approx(200 / 255, abs=1e-6)
    assert float(full.original_image[1, 0, 0]) == 0.0
    assert float(full.original_image[1, 0, 63]) == 1.0        # composited over white
    black = cio.load_camera(info, -1, white_background=False, data_device="cpu")
    assert float(black.original_image[1, 0, 63]) == 0.0
    half = cio.load_camera(info, 2, data_device="cpu")
    assert tuple(half.original_image.shape) == (3, 24, 32)
    assert half.FoVx == info.FoVx


def test_optimization_params_defaults():
    sys.path.insert(0, str(ROOT / "compat"))
    try:
        from arguments import ModelParams, OptimizationParams, PipelineParams
    finally:
        sys.path.remove(str(ROOT / "compat"))
    from pegasus_amd.train import OPTIMIZATION_DEFAULTS
    expect = dict(iterations=30_000, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                  position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005,
                  rotation_lr=0.001, percent_dense=0.01, lambda_dssim=0.2, densification_interval=100,
                  opacity_reset_interval=3000, densify_from_iter=500, densify_until_iter=15_000,
                  densify_grad_threshold=0.0002, random_background=False)
    assert OPTIMIZATION_DEFAULTS == expect
    parser = ArgumentParser()
    lp, op, pp = ModelParams(parser), OptimizationParams(parser), PipelineParams(parser)
    args = parser.parse_args([])
    got = op.extract(args)
    for k, v in expect.items():
        assert getattr(got, k) == v and type(getattr(got, k)) is type(v), k
    args = parser.parse_args(["--densify_until_iter", "1500", "--random_background", "--lambda_dssim", "0.5"])
    got = op.extract(args)
    assert (got.densify_until_iter, got.random_background, got.lambda_dssim) == (1500, True, 0.5)
    assert not hasattr(got, "sh_degree") and lp.extract(args).sh_degree == 3


def test_position_lr_schedule():
    from pegasus_amd.train_ops import get_expon_lr_func
    f = get_expon_lr_func(lr_init=1.6e-4, lr_final=1.6e-6, lr_delay_mult=0.01, max_steps=30_000)
    assert f(0) == pytest.approx(1.6e-4, rel=1e-12)
    assert f(30_000) == pytest.approx(1.6e-6, rel=1e-12)
    assert f(15_000) == pytest.approx(math.sqrt(1.6e-4 * 1.6e-6), rel=1e-12)        # log-linear: geometric mean
    assert f(60_000) == pytest.approx(1.6e-6, rel=1e-12)                            # clamped past max_steps
    assert f(-1) == 0.0
    vals = [f(s) for s in range(0, 30_001, 1000)]
    assert all(a > b for a, b in zip(vals, vals[1:]))
    g = get_expon_lr_func(1.0, 0.01, lr_delay_steps=100, lr_delay_mult=0.1, max_steps=1000)
    assert g(0) == pytest.approx(0.1, rel=1e-12)                                     # delay ramp starts at lr_delay_mult
    assert g(100) == pytest.approx(0.01 ** 0.1, rel=1e-12)
    assert get_expon_lr_func(0.0, 0.0)(5) == 0.0


def test_training_setup_builds_optimizer_groups_on_host():
    """training_setup no longer raises: six named groups with the 3DGS learning rates, parameters with storage of their own."""
    import copy
    import torch
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.train import _Options, OPTIMIZATION_DEFAULTS
    n = 10
    m = GaussianModel.from_arrays(np.zeros((n, 3)), np.zeros((n, 1, 3)), np.zeros((n, 15, 3)), np.zeros((n, 1)),
                                  np.zeros((n, 3)), np.tile([1.0, 0, 0, 0], (n, 1)), device="cpu")
    m = copy.deepcopy(m)                                       # row attributes now live in headroom buffers
    m.spatial_lr_scale = 2.5
    m.training_setup(_Options(None, OPTIMIZATION_DEFAULTS))
    groups = {g["name"]: g for g in m.optimizer.param_groups}
    assert list(groups) == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    assert groups["xyz"]["lr"] == pytest.approx(0.00016 * 2.5)
    assert groups["f_rest"]["lr"] == pytest.approx(0.0025 / 20)
    assert groups["xyz"]["params"][0] is m._xyz and isinstance(m._xyz, torch.nn.Parameter)
    assert "_rows" not in m.__dict__
    assert m.xyz_gradient_accum.shape == (n, 1) and m.denom.shape == (n, 1) and m.max_radii2D.shape == (n,)
    assert m.update_learning_rate(30_000) == pytest.approx(0.0000016 * 2.5)
    assert groups["xyz"]["eps"] == 1e-15


def test_train_cli_parses():
    from pegasus_amd.train import _parser
    a = _parser().parse_args(["-s", "data", "-m", "out", "--iterations", "10", "--eval", "-r", "2"])
    assert (a.source_path, a.model_path, a.iterations, a.eval, a.resolution) == ("data", "out", 10, True, 2)
    assert a.densify_grad_threshold == 0.0002 and a.sh_degree == 3 and a.white_background is False
