"""Multi-view training on the GPU: a batch pgr_backward against single-view pgr_backward calls (one view, and sums over
2 / 4 / 8 views), against the oracle, through render_batch's autograd, the per-view densification statistics of a batch step, and
an end-to-end training run with four views per step."""
import math
import random
from types import SimpleNamespace

import numpy as np
import pytest

from test_backward import tiny_scene
from test_train_gpu import TEST_PSNR_GAIN_FLOOR, TRAIN_PSNR_GAIN_FLOOR, _c1_model, _camera, _write_dataset

pytestmark = pytest.mark.gpu
PIPE = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)


def _views(V, W, H, dist=2.5, fov_deg=55.0):
    """V cameras on a ring around the origin, looking at it."""
    from pegasus_amd import graphics as G, scenes
    fov = math.radians(fov_deg)
    out = []
    for v in range(V):
        a = 0.35 * v - 0.1
        eye = (dist * math.sin(a), -0.1 + 0.05 * v, -dist * math.cos(a))
        R, t = G.look_at_opencv(eye, (0, 0, 0), up=(0, -1, 0))
        out.append(scenes.make_view(R, t, W, H, fovx=fov, fovy=fov * H / W))
    return out


def _settings(v, dev, bg, sh_degree):
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    return dgr.GaussianRasterizationSettings(v.height, v.width, v.tanfovx, v.tanfovy, f(bg), 1.0, f(v.world_view_transform),
                                             f(v.full_proj_transform), sh_degree, f(v.camera_center), False, False)


def _leaves(P, dev, mode):
    """Leaf tensors of the rasterizer's inputs.  mode: sh3 (degree 3, scales / rotations), sh0_cov (one coefficient,
    cov3D_precomp) or colors (colors_precomp, scales / rotations)."""
    import torch
    from pegasus_amd.gaussian_model import build_scaling_rotation, strip_symmetric
    tt = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev).requires_grad_(True)
    x = dict(means3D=tt(P["means3d"]), opacities=tt(np.asarray(P["opacities"]).reshape(-1, 1)))
    if mode == "sh0_cov":
        s = torch.as_tensor(np.asarray(P["scales"]), dtype=torch.float32, device=dev)
        r = torch.as_tensor(np.asarray(P["rotations"]), dtype=torch.float32, device=dev)
        Lm = build_scaling_rotation(s, r)
        x["cov3D_precomp"] = strip_symmetric(Lm @ Lm.transpose(1, 2)).detach().contiguous().requires_grad_(True)
        x["shs"] = tt(np.asarray(P["shs"])[:, :1])
        return x, 0
    x["scales"], x["rotations"] = tt(P["scales"]), tt(P["rotations"])
    if mode == "colors":
        x["colors_precomp"] = tt(np.clip(np.asarray(P["shs"])[:, 0] * 0.28 + 0.5, 0.05, 1.0))
        return x, 3
    x["shs"] = tt(P["shs"])
    return x, 3


def _weights(V, W, H, depth):
    rng = np.random.default_rng(7)
    return [(rng.normal(size=(3, H, W)).astype(np.float32),
             (rng.normal(size=(H, W)) * 0.5).astype(np.float32) if depth else None) for _ in range(V)]


def _single_grads(x, views, deg, dev, bgs, wts):
    """Per view: the drop-in single-view rasterizer (pgr_forward + pgr_backward), its gradients and its means2D.grad."""
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    per_view = []
    for v, bg, (wc, wd) in zip(views, bgs, wts):
        for t in x.values():
            t.grad = None
        m2d = torch.zeros_like(x["means3D"], requires_grad=True)
        kw = {k: t for k, t in x.items() if k not in ("means3D", "opacities")}
        color, radii, depth = dgr.GaussianRasterizer(_settings(v, dev, bg, deg))(x["means3D"], m2d, x["opacities"], **kw)
        loss = (color * torch.as_tensor(wc, device=dev)).sum()
        if wd is not None:
            loss = loss + (depth[0] * torch.as_tensor(wd, device=dev)).sum()
        loss.backward()
        per_view.append(({k: t.grad.clone() for k, t in x.items()}, m2d.grad.clone(), radii.clone()))
    return per_view


def _batch_grads(x, views, deg, dev, bgs, wts):
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    for t in x.values():
        t.grad = None
    m2d = torch.zeros((len(views),) + tuple(x["means3D"].shape), device=dev, requires_grad=True)
    kw = {k: t for k, t in x.items() if k not in ("means3D", "opacities")}
    color, radii, depth = dgr.rasterize_gaussians_batch(x["means3D"], m2d, x["opacities"],
                                                        [_settings(v, dev, bg, deg) for v, bg in zip(views, bgs)], **kw)
    assert color.shape == (len(views), 3, views[0].height, views[0].width) and depth.shape[1] == 1
    assert color.requires_grad and not radii.requires_grad
    loss = 0.0
    for k, (wc, wd) in enumerate(wts):
        loss = loss + (color[k] * torch.as_tensor(wc, device=dev)).sum()
        if wd is not None:
            loss = loss + (depth[k, 0] * torch.as_tensor(wd, device=dev)).sum()
    loss.backward()
    return {k: t.grad.clone() for k, t in x.items()}, m2d.grad.clone(), radii


def _close(got, ref, tol, what):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= tol * max(scale, 1e-12), (what, err, scale)


def _scene(case):
    if case == "tiny":
        P, _ = tiny_scene(3, n=40, W=80, H=64)
        return {k: np.asarray(a, np.float32) for k, a in P.items()}, (80, 64)
    from pegasus_amd import scenes
    cloud, _ = scenes.scene_c1(seed=4, n=3000)
    a = cloud.activated()
    return dict(means3d=a["means3d"], opacities=np.minimum(a["opacities"], 0.9).astype(np.float32), scales=a["scales"],
                rotations=a["rotations"], shs=a["shs"]), (256, 256)


CASES = [("tiny", "sh3", True), ("tiny", "sh0_cov", False), ("tiny", "colors", True), ("cube", "sh3", False),
         ("cube", "sh0_cov", True)]


@pytest.mark.parametrize("case,mode,depth", CASES)
def test_one_view_batch_matches_pgr_backward(gpu_device, case, mode, depth):
    import torch
    P, (W, H) = _scene(case)
    views = _views(1, W, H, dist=2.5 if case == "tiny" else 3.0)
    x, deg = _leaves(P, gpu_device, mode)
    bgs = [(0.2, 0.4, 0.1)]
    wts = _weights(1, W, H, depth)
    (ref, ref_m2d, ref_radii), = _single_grads(x, views, deg, gpu_device, bgs, wts)
    got, m2d, radii = _batch_grads(x, views, deg, gpu_device, bgs, wts)
    torch.cuda.synchronize()
    assert torch.equal(radii[0], ref_radii)
    # the two differ only in the order of the compositor's float atomics; on the 3 000-Gaussian cube that alone moves the
    # rotation gradient (formed through cancelling terms) by 1.1e-6 of its largest entry
    for k in ref:
        _close(got[k], ref[k], 3e-6, k)
    _close(m2d[0], ref_m2d, 3e-6, "means2d")
    assert float(ref["means3D"].abs().max()) > 0


@pytest.mark.parametrize("V", [1, 3])
def test_backward_leaves_the_saved_workspace_alone(gpu_device, V):
    """The forward's workspace is a tensor autograd saved for the backward: the backward only reads it (its per-view table
    and gradient rows live in its own scratch).  V = 1 through the drop-in GaussianRasterizer, V = 3 through
    rasterize_gaussians_batch; the workspace after loss.backward() equals its clone from before, byte for byte."""
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    P, (W, H) = _scene("tiny")
    views = _views(V, W, H)
    x, deg = _leaves(P, gpu_device, "sh3")
    kw = {k: t for k, t in x.items() if k not in ("means3D", "opacities")}
    sets = [_settings(v, gpu_device, (0.2, 0.4, 0.1), deg) for v in views]
    if V == 1:
        color, _, depth = dgr.GaussianRasterizer(sets[0])(x["means3D"], None, x["opacities"], **kw)
    else:
        color, _, depth = dgr.rasterize_gaussians_batch(x["means3D"], None, x["opacities"], sets, **kw)
    (ws,) = [t for t in color.grad_fn.saved_tensors if t.dtype == torch.uint8]
    assert ws.numel() > 0
    before = ws.clone()
    (color.square().sum() + depth.sum()).backward()
    torch.cuda.synchronize()
    assert float(x["means3D"].grad.abs().max()) > 0
    assert torch.equal(ws, before)


@pytest.mark.parametrize("V", [2, 4, 8])
@pytest.mark.parametrize("case,mode,depth", CASES)
def test_batch_sums_single_view_gradients(gpu_device, V, case, mode, depth):
    import torch
    P, (W, H) = _scene(case)
    views = _views(V, W, H, dist=2.5 if case == "tiny" else 3.0)
    x, deg = _leaves(P, gpu_device, mode)
    bgs = [(0.1 * v % 1.0, 0.4, 0.2) for v in range(V)]
    wts = _weights(V, W, H, depth)
    singles = _single_grads(x, views, deg, gpu_device, bgs, wts)
    got, m2d, radii = _batch_grads(x, views, deg, gpu_device, bgs, wts)
    torch.cuda.synchronize()
    for k in got:
        _close(got[k], sum(s[0][k] for s in singles), 1e-5, k)
    for v, (_, ref_m2d, ref_radii) in enumerate(singles):
        assert torch.equal(radii[v], ref_radii)
        _close(m2d[v], ref_m2d, 1e-5, f"means2d[{v}]")
        assert not m2d[v, :, 2].any()


@pytest.mark.parametrize("case", ["tiny", "cube"])
def test_batch_matches_oracle(oracle, gpu_device, case):
    import torch
    P, (W, H) = _scene(case)
    views = _views(3, W, H, dist=2.5 if case == "tiny" else 3.0)
    x, deg = _leaves(P, gpu_device, "sh3")
    bgs = [(0.2, 0.4, 0.1), (0.0, 0.0, 0.0), (1.0, 0.5, 0.25)]
    wts = _weights(3, W, H, True)
    got, m2d, _ = _batch_grads(x, views, deg, gpu_device, bgs, wts)
    torch.cuda.synchronize()
    ref = {}
    ref_m2d = []
    for v, bg, (wc, wd) in zip(views, bgs, wts):
        g = oracle.backward(**P, sh_degree=3, grad_color=wc, grad_depth=wd, **v.raster_kwargs(bg))
        for k in ("means3d", "opacities", "scales", "rotations", "shs"):
            ref[k] = ref.get(k, 0) + g[k]
        ref_m2d.append(g["means2d"])
    names = dict(means3d="means3D", opacities="opacities", scales="scales", rotations="rotations", shs="shs")
    for k, name in names.items():
        tg = got[name].cpu().numpy().reshape(ref[k].shape)
        err, scale = np.abs(tg - ref[k]).max(), max(1e-4, np.abs(ref[k]).max())
        assert err / scale < 2e-3, (k, err, scale)
    for v in range(3):
        err, scale = np.abs(m2d[v].cpu().numpy() - ref_m2d[v]).max(), max(1e-4, np.abs(ref_m2d[v]).max())
        assert err / scale < 2e-3, (v, err, scale)


def _model_and_cameras(dev, V, n=3000, images=False):
    import torch
    m, _ = _c1_model(dev, n=n)
    cams = []
    for v in _views(V, 256, 256, dist=3.0, fov_deg=50.0):
        img = torch.rand((3, 256, 256), generator=torch.Generator().manual_seed(len(cams))).to(dev) if images else None
        cams.append(_camera(v, dev, image=img))
    return m, cams


_PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


@pytest.mark.parametrize("cov_python", [False, True])
def test_render_batch_autograd_matches_per_view_render(gpu_device, cov_python):
    import torch
    from pegasus_amd.gaussian_renderer import render, render_batch
    m, cams = _model_and_cameras(gpu_device, 4)
    for a in _PARAMS:
        setattr(m, a, getattr(m, a).detach().clone().requires_grad_(True))
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=cov_python, debug=False)
    bg = torch.tensor([[0.1, 0.2, 0.3], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.1, 0.9]], device=gpu_device)
    wts = _weights(4, 256, 256, True)
    w = [(torch.as_tensor(wc, device=gpu_device), torch.as_tensor(wd, device=gpu_device)) for wc, wd in wts]
    ref = {a: 0 for a in _PARAMS}
    ref_vs = []
    for v, cam in enumerate(cams):
        pkg = render(cam, m, pipe, bg[v])
        ((pkg["render"] * w[v][0]).sum() + (pkg["depth"][0] * w[v][1]).sum()).backward()
        for a in _PARAMS:
            ref[a] = ref[a] + getattr(m, a).grad
            getattr(m, a).grad = None
        ref_vs.append(pkg["viewspace_points"].grad.clone())
    pkg = render_batch(cams, m, pipe, bg)
    assert pkg["render"].shape == (4, 3, 256, 256) and pkg["depth"].shape == (4, 1, 256, 256)
    assert pkg["viewspace_points"].shape == (4, 3000, 3) and pkg["viewspace_points"].is_leaf
    assert pkg["visibility_filter"].dtype == torch.bool and torch.equal(pkg["visibility_filter"], pkg["radii"] > 0)
    sum((pkg["render"][v] * w[v][0]).sum() + (pkg["depth"][v, 0] * w[v][1]).sum() for v in range(4)).backward()
    torch.cuda.synchronize()
    for a in _PARAMS:
        _close(getattr(m, a).grad, ref[a], 1e-5, a)
    for v in range(4):
        _close(pkg["viewspace_points"].grad[v], ref_vs[v], 1e-5, f"viewspace[{v}]")


def test_render_batch_contract_edges(gpu_device):
    import torch
    from pegasus_amd.gaussian_renderer import render_batch
    m, cams = _model_and_cameras(gpu_device, 2)
    m._xyz = m._xyz.detach().clone().requires_grad_(True)
    m._scaling = m._scaling.detach().clone().requires_grad_(True)
    bg = torch.zeros(3, device=gpu_device)
    # an in-place edit of an input between forward and backward raises
    pkg = render_batch(cams, m, PIPE, bg)
    with torch.no_grad():
        m._xyz.add_(0.01)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        pkg["render"].sum().backward()
    # mixed image sizes and host-evaluated SH are refused
    small = _camera(_views(1, 128, 128, dist=3.0, fov_deg=50.0)[0], gpu_device)
    with pytest.raises(ValueError, match="same image size"):
        render_batch([cams[0], small], m, PIPE, bg)
    with pytest.raises(ValueError, match="convert_SHs_python"):
        render_batch(cams, m, SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False), bg)
    with pytest.raises(ValueError, match="bg_color"):
        render_batch(cams, m, PIPE, torch.zeros((3, 3), device=gpu_device))
    # override colours, shared by the views
    with torch.no_grad():
        col = torch.full((3000, 3), 0.5, device=gpu_device)
        out = render_batch(cams, m, PIPE, bg, override_color=col)["render"]
    assert out.shape == (2, 3, 256, 256) and float(out.max()) <= 0.5 + 1e-5 and float(out.max()) > 0.1


def test_instance_overflow_retries_and_gives_correct_gradients(gpu_device, monkeypatch):
    """2 000 large Gaussians list ~0.5 M (Gaussian, tile) instances per view, above the first capacity of 2^18."""
    import torch
    from pegasus_amd import rasterizer
    rng = np.random.default_rng(11)
    n = 2000
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    P = dict(means3d=(rng.uniform(-0.4, 0.4, size=(n, 3))).astype(np.float32),
             opacities=rng.uniform(0.05, 0.2, size=n).astype(np.float32),
             scales=np.full((n, 3), 0.6, np.float32), rotations=q.astype(np.float32),
             shs=rng.normal(0, 0.3, size=(n, 16, 3)).astype(np.float32))
    views = _views(2, 256, 256)
    x, deg = _leaves(P, gpu_device, "sh3")
    bgs = [(0.2, 0.4, 0.1)] * 2
    wts = _weights(2, 256, 256, True)
    grown = []
    real = rasterizer.grown_capacity
    monkeypatch.setattr(rasterizer, "grown_capacity", lambda need, f: grown.append(need) or real(need, f))
    singles = _single_grads(x, views, deg, gpu_device, bgs, wts)
    n_single = len(grown)
    got, m2d, _ = _batch_grads(x, views, deg, gpu_device, bgs, wts)
    torch.cuda.synchronize()
    assert n_single >= 2 and len(grown) > n_single, grown          # both paths overflowed their first capacity
    for k in got:
        _close(got[k], sum(s[0][k] for s in singles), 1e-5, k)
    for v in range(2):
        _close(m2d[v], singles[v][1], 1e-5, f"means2d[{v}]")


def test_batch_step_densification_stats_match_single_views(gpu_device):
    import torch
    from pegasus_amd.gaussian_renderer import render
    from pegasus_amd.train import OPTIMIZATION_DEFAULTS, _Options, train_step_batch
    from pegasus_amd.train_ops import ImageLoss
    m, cams = _model_and_cameras(gpu_device, 4, images=True)
    m.spatial_lr_scale = 1.0
    m.training_setup(_Options(None, OPTIMIZATION_DEFAULTS))
    bg = torch.zeros(3, device=gpu_device)
    loss, pkg = train_step_batch(m, cams, PIPE, bg, 0.2)
    m.add_batch_render_stats(pkg["viewspace_points"], pkg["radii"], grad_scale=4)
    batch = [t.clone() for t in (m.xyz_gradient_accum, m.denom, m.max_radii2D)]
    batch_grads = [getattr(m, a).grad.clone() for a in _PARAMS]
    m.optimizer.zero_grad(set_to_none=True)
    for t in (m.xyz_gradient_accum, m.denom, m.max_radii2D):
        t.zero_()
    losses = []
    for cam in cams:
        p = render(cam, m, PIPE, bg)
        lv = ImageLoss.apply(p["render"], cam.original_image, 0.2)
        lv.backward()
        losses.append(float(lv.detach()))
        m.add_render_stats(p["viewspace_points"], p["radii"])
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - sum(losses) / 4) < 1e-6
    _close(batch[0], m.xyz_gradient_accum, 1e-5, "xyz_gradient_accum")
    assert torch.equal(batch[1], m.denom) and torch.equal(batch[2], m.max_radii2D)
    assert float(m.denom.max()) >= 2                    # Gaussians seen by several views count once per view
    for a, g in zip(_PARAMS, batch_grads):              # the step's gradient is the mean over the views
        _close(g * 4, getattr(m, a).grad, 1e-5, a)


def test_end_to_end_training_with_four_views_per_step(gpu_device, tmp_path):
    import torch
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.scene import Scene
    from pegasus_amd.train import training
    random.seed(0)
    torch.manual_seed(0)
    src, out = tmp_path / "data", tmp_path / "model"
    _write_dataset(src, gpu_device)
    dataset = SimpleNamespace(sh_degree=3, source_path=str(src), model_path=str(out), images="images", resolution=-1,
                              white_background=False, data_device="cuda", eval=True)
    opt = SimpleNamespace(iterations=2000, densify_from_iter=100, densify_until_iter=1500, densification_interval=100,
                          position_lr_max_steps=2000, batch_size=4)
    res = training(dataset, opt, PIPE, [1, 2000], [2000], [], None, -1, quiet=True)
    first, last = res["reports"][1], res["reports"][2000]
    gain_train = last["train"]["psnr"] - first["train"]["psnr"]
    gain_test = last["test"]["psnr"] - first["test"]["psnr"]
    print(f"\nend to end, 4 views per step: initial 2000 Gaussians -> {res['num_gaussians']}; PSNR train "
          f"{first['train']['psnr']:.2f} -> {last['train']['psnr']:.2f} dB (+{gain_train:.2f}), test "
          f"{first['test']['psnr']:.2f} -> {last['test']['psnr']:.2f} dB (+{gain_test:.2f})")
    assert gain_train >= TRAIN_PSNR_GAIN_FLOOR and gain_test >= TEST_PSNR_GAIN_FLOOR, (gain_train, gain_test)
    g = GaussianModel(3)
    scene = Scene(SimpleNamespace(model_path=str(out), data_device="cuda"), g, load_iteration=-1)
    assert scene.loaded_iter == 2000 and g.get_xyz.shape[0] == res["num_gaussians"]
