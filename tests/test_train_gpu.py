"""Training on the GPU: the fused image loss against float64 autograd, FusedAdam against torch.optim.Adam, the densification
statistics kernel, densify / prune with the optimizer state, and an end-to-end training run whose output opens with
Scene(..., load_iteration=-1)."""
import copy
import math
import random
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


# ---- loss -------------------------------------------------------------------------------------------------------------------
from train_reference import loss_f64 as _reference_loss      # noqa: E402  (float64 autograd, shared with the kernel tests)


@pytest.mark.parametrize("hw,lams", [((1, 1), (0.0, 0.2, 1.0)), ((17, 13), (0.0, 0.2, 1.0)), ((255, 257), (0.0, 0.2, 1.0)),
                                     ((256, 256), (0.2,)), ((800, 800), (0.2,))])
def test_image_loss_matches_float64_autograd(gpu_device, hw, lams):
    import torch
    from pegasus_amd.train_ops import ImageLoss, image_loss_terms
    H, W = hw
    gen = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.rand((3, H, W), generator=gen)
    y = (x + 0.15 * torch.randn((3, H, W), generator=gen)).clamp(0, 1)
    for lam in lams:
        ref_loss, ref_grad, ref_l1, ref_ssim = _reference_loss(x, y, lam)
        xd = x.to(gpu_device).requires_grad_(True)
        loss = ImageLoss.apply(xd, y.to(gpu_device), lam)
        loss.backward()
        got = float(loss.detach())
        assert abs(got - ref_loss) <= 1e-6 * max(1.0, abs(ref_loss)), (hw, lam, got, ref_loss)
        g = xd.grad.double().cpu()
        scale = float(ref_grad.abs().max())
        assert float((g - ref_grad).abs().max()) <= 1e-5 * scale, (hw, lam, float((g - ref_grad).abs().max()), scale)
        out, _ = image_loss_terms(x.to(gpu_device), y.to(gpu_device), lam, want_grad=False)
        out = out.cpu().double()
        assert abs(float(out[1]) - ref_l1) <= 1e-6 and abs(float(out[2]) - ref_ssim) <= 1e-6
        # deterministic: the same call twice gives the same bits
        again, _ = image_loss_terms(x.to(gpu_device), y.to(gpu_device), lam)
        first, _ = image_loss_terms(x.to(gpu_device), y.to(gpu_device), lam)
        assert torch.equal(again, first)


def test_image_loss_of_identical_images_is_zero(gpu_device):
    import torch
    from pegasus_amd.train_ops import ImageLoss
    for H, W in ((1, 1), (17, 13), (256, 256)):
        x = torch.rand((3, H, W), generator=torch.Generator().manual_seed(H)).to(gpu_device)
        for lam in (0.0, 0.2, 1.0):
            xd = x.clone().requires_grad_(True)
            loss = ImageLoss.apply(xd, x, lam)
            loss.backward()
            assert float(loss.detach()) == 0.0, (H, W, lam, float(loss.detach()))
            assert float(xd.grad.abs().max()) == 0.0, (H, W, lam)


def test_image_loss_scales_with_grad_output_and_helpers(gpu_device):
    import torch
    from pegasus_amd.train_ops import ImageLoss, l1_loss, ssim
    gen = torch.Generator().manual_seed(5)
    x = torch.rand((3, 40, 30), generator=gen).to(gpu_device)
    y = torch.rand((3, 40, 30), generator=gen).to(gpu_device)
    a = x.clone().requires_grad_(True)
    ImageLoss.apply(a, y, 0.2).backward()
    b = x.clone().requires_grad_(True)
    (3.0 * ImageLoss.apply(b, y, 0.2)).backward()
    torch.testing.assert_close(b.grad, 3.0 * a.grad, rtol=1e-6, atol=0)
    assert float(l1_loss(x, y)) == pytest.approx(float((x - y).abs().mean()), rel=1e-5)
    _, _, _, ref_ssim = _reference_loss(x, y, 1.0)
    assert float(ssim(x, y)) == pytest.approx(ref_ssim, abs=1e-6)


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    import torch
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = torch.where(ib < 0, -(ib & 0x7fffffff), ib)
    return (ia - ib).abs()


def test_fused_adam_matches_torch_adam(gpu_device):
    import torch
    from pegasus_amd.train_ops import FusedAdam
    sizes = [0, 1, 1000, 4097, 100_003, 7]
    lrs = [1e-3, 0.05, 0.0, 1.6e-4, 0.0025, 1e-2]
    gen = torch.Generator().manual_seed(0)
    init = [torch.randn(n, generator=gen) for n in sizes]
    ours = [torch.nn.Parameter(t.clone().to(gpu_device)) for t in init]
    ref = [torch.nn.Parameter(t.clone().to(gpu_device)) for t in init]
    opt = FusedAdam([{"params": [p], "lr": lr, "name": f"g{i}"} for i, (p, lr) in enumerate(zip(ours, lrs))], lr=0.0,
                    eps=1e-15)
    topt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(ref, lrs)], lr=0.0, eps=1e-15, foreach=False)
    mismatched = 0
    for step in range(20):
        for p, q in zip(ours, ref):
            g = (torch.randn(p.shape, generator=gen) * (10.0 ** ((step % 5) - 3))).to(gpu_device)
            p.grad, q.grad = g.clone(), g.clone()
        versions = [p._version for p in ours]
        opt.step()
        topt.step()
        assert all(p._version > v for p, v in zip(ours, versions))
        for p, q in zip(ours, ref):
            so, st = opt.state[p], topt.state[q]
            assert float(so["step"]) == float(st["step"]) == step + 1
            for a, b in ((p.data, q.data), (so["exp_avg"], st["exp_avg"]), (so["exp_avg_sq"], st["exp_avg_sq"])):
                if a.numel():
                    u = _ulps(a, b)
                    assert int(u.max()) <= 1, (step, int(u.max()))
                    mismatched += int((u > 0).sum())
                    b.copy_(a)          # (a 1-ulp difference must not compound into the next step's comparison)
    print(f"\nFusedAdam vs torch.optim.Adam(foreach=False): {mismatched} element values off by 1 ulp "
          f"over 20 steps x {sum(sizes)} elements x 3 tensors")
    assert mismatched == 0


def test_fused_adam_state_dict_round_trip(gpu_device):
    import torch
    from pegasus_amd.train_ops import FusedAdam
    gen = torch.Generator().manual_seed(1)
    a = [torch.nn.Parameter(torch.randn(n, generator=gen).to(gpu_device)) for n in (5, 300)]
    opt = FusedAdam([{"params": [a[0]], "lr": 0.01, "name": "x"}, {"params": [a[1]], "lr": 0.001, "name": "y"}], eps=1e-15)
    for _ in range(3):
        for p in a:
            p.grad = torch.randn(p.shape, generator=gen).to(gpu_device)
        opt.step()
    sd = opt.state_dict()
    assert [g["name"] for g in sd["param_groups"]] == ["x", "y"]
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 3
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    opt2 = FusedAdam([{"params": [b[0]], "lr": 0.5, "name": "x"}, {"params": [b[1]], "lr": 0.5, "name": "y"}], eps=1e-15)
    opt2.load_state_dict(copy.deepcopy(sd))      # (state_dict() hands out the live state tensors, as torch's does)
    assert opt2.param_groups[0]["lr"] == 0.01
    g = [torch.randn(p.shape, generator=gen).to(gpu_device) for p in a]
    for p, q, gg in zip(a, b, g):
        p.grad, q.grad = gg.clone(), gg.clone()
    opt.step()
    opt2.step()
    for p, q in zip(a, b):
        assert torch.equal(p, q)
        assert torch.equal(opt.state[p]["exp_avg_sq"], opt2.state[q]["exp_avg_sq"])


def _c1_model(device, n=3000):
    from pegasus_amd import scenes
    from pegasus_amd.gaussian_model import GaussianModel
    cloud, views = scenes.scene_c1(n=n)
    m = GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling,
                                  cloud.rotation, sh_degree=3, device=device)
    return m, views


def _camera(v, device, image=None):
    import torch
    from pegasus_amd.cameras import Camera
    return Camera(colmap_id=0, R=v.R_c2w, T=v.t_w2c, FoVx=v.fovx, FoVy=v.fovy, image=image, gt_alpha_mask=None,
                  image_name="v", uid=0, data_device=str(device), image_width=v.width, image_height=v.height)


def test_step_invalidates_kept_activations_of_no_grad_renders(gpu_device):
    """After FusedAdam.step(), a no-grad render shows the updated parameters (the kernel's raw writes bump the version
    counters that gaussian_renderer's activation cache is keyed on)."""
    import torch
    from pegasus_amd import gaussian_renderer as GR
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.train import _Options, OPTIMIZATION_DEFAULTS
    from pegasus_amd.train_ops import ImageLoss
    m, views = _c1_model(gpu_device)
    m.spatial_lr_scale = 1.0
    m.training_setup(_Options(None, OPTIMIZATION_DEFAULTS))
    cam = _camera(views[0], gpu_device)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device=gpu_device)
    with torch.no_grad():
        for _ in range(GR.SPLIT_RENDERS + 1):                 # the kept activations and the kept SH concatenation exist
            before = GR.render(cam, m, pipe, bg)["render"].clone()
    target = torch.rand_like(before)
    img = GR.render(cam, m, pipe, bg)["render"]
    ImageLoss.apply(img, target, 0.2).backward()
    m.optimizer.step()
    with torch.no_grad():
        after = GR.render(cam, m, pipe, bg)["render"]
        fresh = GaussianModel.from_arrays(*(t.detach().cpu().numpy() for t in (
            m._xyz, m._features_dc, m._features_rest, m._opacity, m._scaling, m._rotation)), device=gpu_device)
        expect = GR.render(cam, fresh, pipe, bg)["render"]
    assert float((after - before).abs().max()) > 1e-3                # the update is visible ...
    torch.testing.assert_close(after, expect, rtol=1e-5, atol=1e-5)  # ... and it is the updated model's image


# ---- densification statistics -------------------------------------------------------------------------------------------
def test_densify_stats_matches_torch(gpu_device):
    import torch
    from pegasus_amd.train_ops import densify_stats
    n = 100_000
    gen = torch.Generator().manual_seed(3)
    grad = torch.randn((n, 3), generator=gen).to(gpu_device)
    radii = (torch.randint(-2, 30, (n,), generator=gen).clamp_min(0)).to(torch.int32).to(gpu_device)
    accum = torch.rand((n, 1), generator=gen).to(gpu_device)
    denom = torch.randint(0, 5, (n, 1), generator=gen).float().to(gpu_device)
    maxr = (torch.rand(n, generator=gen) * 40).to(gpu_device)
    vis = radii > 0
    e_accum, e_denom, e_max = accum.clone(), denom.clone(), maxr.clone()
    e_accum[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
    e_denom[vis] += 1
    e_max[vis] = torch.max(e_max[vis], radii[vis].float())
    densify_stats(grad, radii, accum, denom, maxr)
    assert 0 < int(vis.sum()) < n
    torch.testing.assert_close(accum, e_accum, rtol=1e-6, atol=0)
    assert torch.equal(denom, e_denom) and torch.equal(maxr, e_max)


# ---- densify / prune --------------------------------------------------------------------------------------------------------
def _hand_built(device):
    """Five Gaussians: 0 high gradient + small (clone), 1 high gradient + large (split), 2 transparent (prune),
    3 large on screen (prune), 4 ordinary (kept)."""
    import torch
    from pegasus_amd.gaussian_model import GaussianModel, inverse_sigmoid
    from pegasus_amd.train import _Options, OPTIMIZATION_DEFAULTS
    n = 5
    xyz = np.arange(15, dtype=np.float32).reshape(5, 3)
    scale = np.log(np.array([[0.001] * 3, [0.05, 0.02, 0.01], [0.002] * 3, [0.002] * 3, [0.002] * 3], np.float32))
    opac = inverse_sigmoid(torch.tensor([[0.5], [0.5], [0.001], [0.5], [0.5]])).numpy()
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (n, 1))
    rng = np.random.default_rng(0)
    m = GaussianModel.from_arrays(xyz, rng.normal(size=(n, 1, 3)), rng.normal(size=(n, 15, 3)), opac, scale, rot,
                                  device=device)
    m.spatial_lr_scale = 1.0
    m.training_setup(_Options(None, OPTIMIZATION_DEFAULTS))
    gen = torch.Generator().manual_seed(1)
    for g in m.optimizer.param_groups:
        p = g["params"][0]
        m.optimizer.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.randn(p.shape, generator=gen).to(device),
                                "exp_avg_sq": torch.rand(p.shape, generator=gen).to(device)}
    m.xyz_gradient_accum = torch.tensor([[1e-3], [1e-3], [0.0], [0.0], [1e-5]], device=device)
    m.denom = torch.tensor([[1.0], [1.0], [1.0], [0.0], [1.0]], device=device)   # row 3: 0/0 counts as no gradient
    m.max_radii2D = torch.tensor([1.0, 1.0, 1.0, 30.0, 1.0], device=device)
    return m


def test_densify_and_prune_on_hand_built_state(gpu_device):
    import torch
    m = _hand_built(gpu_device)
    before = {g["name"]: (g["params"][0].detach().clone(), {k: v.clone() for k, v in m.optimizer.state[g["params"][0]].items()})
              for g in m.optimizer.param_groups}
    torch.manual_seed(0)
    m.densify_and_prune(0.0002, 0.005, 1.0, 20)
    # kept: 0, 3 (densification_postfix zeroes max_radii2D, as upstream), 4; appended: the clone of 0, then the two
    # samples of 1 (1 itself is replaced, 2 is transparent)
    n, kept = 6, [0, 3, 4]
    for g in m.optimizer.param_groups:
        p = g["params"][0]
        st = m.optimizer.state[p]
        assert p.shape[0] == n and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        old_p, old_st = before[g["name"]]
        for row, old in enumerate(kept):
            assert torch.equal(p[row], old_p[old])
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(st[k][row], old_st[k][old])          # kept rows keep their moments
        assert torch.equal(p[3], old_p[0])
        for k in ("exp_avg", "exp_avg_sq"):
            assert float(st[k][3:].abs().max()) == 0.0                  # new rows start with zero moments
        assert float(st["step"]) == 7.0
        assert p is getattr(m, dict(m._PARAM_NAMES)[g["name"]])
    expect_scale = torch.log(torch.tensor([0.05, 0.02, 0.01]) / 1.6).to(gpu_device)
    torch.testing.assert_close(m._scaling[4], expect_scale)
    torch.testing.assert_close(m._scaling[5], expect_scale)
    assert torch.equal(m._rotation[4], before["rotation"][0][1]) and torch.equal(m._opacity[5], before["opacity"][0][1])
    assert float((m._xyz[4:] - before["xyz"][0][1]).abs().max()) < 0.5 and not torch.equal(m._xyz[4], m._xyz[5])
    for t in (m.xyz_gradient_accum, m.denom):
        assert t.shape == (n, 1) and float(t.abs().max()) == 0.0
    assert m.max_radii2D.shape == (n,)


def test_prune_by_opacity_and_screen_radius(gpu_device):
    import torch
    m = _hand_built(gpu_device)
    old_xyz = m._xyz.detach().clone()
    old_m = m.optimizer.state[m._xyz]["exp_avg"].clone()
    m.prune_by(0.005, 1.0, 20)                  # 2: opacity 0.001 < 0.005; 3: 30 px on screen > 20
    assert torch.equal(m._xyz, old_xyz[[0, 1, 4]])
    assert torch.equal(m.optimizer.state[m._xyz]["exp_avg"], old_m[[0, 1, 4]])
    assert torch.equal(m.max_radii2D, torch.tensor([1.0, 1.0, 1.0], device=gpu_device))
    assert m.xyz_gradient_accum.shape == (3, 1) and m.denom.shape == (3, 1)
    m = _hand_built(gpu_device)
    m.prune_by(0.005, 0.2, None)                # without a screen limit only the opacity test applies
    assert m.get_xyz.shape[0] == 4
    m = _hand_built(gpu_device)
    m.prune_by(0.005, 0.2, 1000)                # 1 is larger than a tenth of a 0.2 scene
    assert torch.equal(m._xyz, old_xyz[[0, 3, 4]])


def test_split_only_and_clone_only(gpu_device):
    import torch
    m = _hand_built(gpu_device)
    grads = m.xyz_gradient_accum / m.denom
    grads[grads.isnan()] = 0.0
    m.densify_and_clone(grads, 0.0002, 1.0)
    assert m.get_xyz.shape[0] == 6 and torch.equal(m._xyz[5], m._xyz[0])
    m = _hand_built(gpu_device)
    grads = m.xyz_gradient_accum / m.denom
    grads[grads.isnan()] = 0.0
    m.densify_and_split(grads, 0.0002, 1.0)
    assert m.get_xyz.shape[0] == 6                                       # 5 - 1 + 2
    torch.testing.assert_close(m.get_scaling[4:], torch.tensor([[0.05, 0.02, 0.01]], device=gpu_device).repeat(2, 1) / 1.6)


def test_reset_opacity_capture_restore(gpu_device):
    import torch
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.train import _Options, OPTIMIZATION_DEFAULTS
    m = _hand_built(gpu_device)
    m.reset_opacity()
    assert float(m.get_opacity.max()) <= 0.01 + 1e-6
    st = m.optimizer.state[m._opacity]
    assert float(st["exp_avg"].abs().max()) == 0.0 and float(st["step"]) == 7.0
    captured = m.capture()
    r = GaussianModel(3, device=gpu_device)
    r.restore(captured, _Options(None, OPTIMIZATION_DEFAULTS))
    for _, attr in m._PARAM_NAMES:
        assert torch.equal(getattr(r, attr), getattr(m, attr))
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(r, k), getattr(m, k))
    for ga, gb in zip(m.optimizer.param_groups, r.optimizer.param_groups):
        assert ga["name"] == gb["name"] and ga["lr"] == gb["lr"]
        sa, sb = m.optimizer.state[ga["params"][0]], r.optimizer.state[gb["params"][0]]
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(sa[k], sb[k])
    assert r.spatial_lr_scale == m.spatial_lr_scale and r.active_sh_degree == m.active_sh_degree


# ---- end to end -------------------------------------------------------------------------------------------------------------
# PSNR gains (dB) over the initial model that a 2000-iteration run must reach.  Measured on an MI355X: +10.17 dB on the
# training views, +4.92 dB on the held-out views; the floors sit more than 3 dB below both.
TRAIN_PSNR_GAIN_FLOOR = 7.0
TEST_PSNR_GAIN_FLOOR = 1.5


def _write_dataset(root, device, n_views=32, size=256):
    """32 views of a seeded C1-style cube rendered with the project's forward path, as a COLMAP dataset with PNGs; the
    initial points are a noisy subset of the Gaussian means with their base colours."""
    import torch
    from PIL import Image
    from pegasus_amd import colmap_io as cio, graphics as G
    from pegasus_amd.gaussian_renderer import render
    from pegasus_amd.scenes import make_view
    from pegasus_amd.sh_utils import SH2RGB
    m, _ = _c1_model(device, n=10_000)
    fov = math.radians(50.0)
    focal = 0.5 * size / math.tan(0.5 * fov)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device=device)
    (root / "images").mkdir(parents=True)
    imgs = {}
    for k, eye in enumerate(G.fibonacci_sphere(n_views + 1, 3.0)[:n_views]):
        R, t = G.look_at_opencv(eye, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
        v = make_view(R, t, size, size, fx=focal, fy=focal)
        with torch.no_grad():
            img = render(_camera(v, device), m, pipe, bg)["render"].clamp(0, 1)
        arr = (img.permute(1, 2, 0).cpu().numpy() * 255.0 + 0.5).astype(np.uint8)
        Image.fromarray(arr, "RGB").save(root / "images" / f"view_{k:03d}.png")
        imgs[k + 1] = cio.ColmapImage(k + 1, cio.rotmat2qvec(R), t, 1, f"view_{k:03d}.png")
    cams = {1: cio.ColmapCamera(1, "PINHOLE", size, size, np.array([focal, focal, size / 2, size / 2]))}
    rng = np.random.default_rng(7)
    pick = rng.choice(m.get_xyz.shape[0], 2000, replace=False)
    xyz = m.get_xyz.detach().cpu().numpy()[pick] + rng.normal(scale=0.03, size=(2000, 3))
    rgb = (SH2RGB(m._features_dc.detach().cpu().numpy()[pick, 0]).clip(0, 1) * 255).astype(np.uint8)
    cio.write_colmap_model(root / "sparse" / "0", cams, imgs, xyz, rgb, binary=True)


def test_end_to_end_training_and_scene_reload(gpu_device, tmp_path):
    import torch
    from pegasus_amd import colmap_io as cio
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.scene import Scene
    from pegasus_amd.train import evaluate, training
    random.seed(0)
    torch.manual_seed(0)
    src, out = tmp_path / "data", tmp_path / "model"
    _write_dataset(src, gpu_device)
    dataset = SimpleNamespace(sh_degree=3, source_path=str(src), model_path=str(out), images="images", resolution=-1,
                              white_background=False, data_device="cuda", eval=True)
    opt = SimpleNamespace(iterations=2000, densify_from_iter=100, densify_until_iter=1500, densification_interval=100,
                          position_lr_max_steps=2000)           # every other field: the 3DGS default
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    res = training(dataset, opt, pipe, [1, 2000], [2000], [2000], None, -1, quiet=True)
    first, last = res["reports"][1], res["reports"][2000]
    gain_train = last["train"]["psnr"] - first["train"]["psnr"]
    gain_test = last["test"]["psnr"] - first["test"]["psnr"]
    print(f"\nend to end: initial 2000 Gaussians -> {res['num_gaussians']}; PSNR train {first['train']['psnr']:.2f} -> "
          f"{last['train']['psnr']:.2f} dB, test {first['test']['psnr']:.2f} -> {last['test']['psnr']:.2f} dB")
    assert gain_train >= TRAIN_PSNR_GAIN_FLOOR and gain_test >= TEST_PSNR_GAIN_FLOOR, (gain_train, gain_test)
    assert res["num_gaussians"] != 2000
    for f in ("cfg_args", "cameras.json", "input.ply", "chkpnt2000.pth", "point_cloud/iteration_2000/point_cloud.ply"):
        assert (out / f).exists(), f
    # the saved model opens with the render path's Scene and reproduces the trainer's final test PSNR
    g = GaussianModel(3)
    scene = Scene(SimpleNamespace(model_path=str(out), data_device="cuda"), g, load_iteration=-1)
    assert scene.loaded_iter == 2000 and len(scene.getTrainCameras()) == 32
    assert g.get_xyz.shape[0] == res["num_gaussians"]
    infos = cio.camera_infos(str(src))
    test_cams = [cio.load_camera(c) for c in cio.split_train_test(infos, True)[1]]
    _, p = evaluate(test_cams, g, pipe, torch.zeros(3, device=gpu_device))
    assert abs(p - last["test"]["psnr"]) < 1e-3, (p, last["test"]["psnr"])
    # a checkpoint restores into a model that continues from the same state
    model_params, it = torch.load(out / "chkpnt2000.pth", weights_only=False)
    r = GaussianModel(3)
    r.restore(model_params, opt)
    assert it == 2000 and torch.equal(r._xyz.detach(), res["model"]._xyz.detach())
