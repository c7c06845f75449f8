"""Differentiable alpha (1 - final_T) and training from object masks, on the GPU: the alpha output, its gradient through
pgr_backward's grad_alpha (one view and batches) against the oracle, the bit-equality of the NULL paths, the masked image loss
against float64 torch autograd, and a masked end-to-end training run.

The alpha-gradient reference is the unchanged oracle: image = C + T bg and alpha = 1 - T, so the gradient of
sum G image + sum g_a alpha with g_a = G[0] is the oracle's colour-only backward with background bg - (1, 0, 0)
(tests/test_alpha_masks_host.py pins that construction to finite differences)."""
import ctypes as C
import random
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import assert_grads_match
from test_backward_parity_gpu import (BG, DGR_ARG, ORACLE_KEY, ROUNDING_BOUNDS, _settings, _weights, mode_inputs,
                                      single_scene)

pytestmark = pytest.mark.gpu
E0 = np.array([1.0, 0.0, 0.0])


def _leaf(X, dev):
    import torch
    return {k: torch.from_numpy(a.reshape(-1, 1) if k == "opacities" else a).to(dev).requires_grad_(True)
            for k, a in X.items()}


def hip_alpha_backward(X, v, deg, mod, gC, gD, gA, dev, bg=BG):
    """loss = sum gC color + sum gD depth + sum gA alpha through the drop-in rasterizer (return_alpha=True); gA None: alpha
    is returned but takes no part in the loss.  Returns ({oracle key: gradient}, radii, alpha)."""
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    leaf = _leaf(X, dev)
    m2d = torch.zeros_like(leaf["means3d"], requires_grad=True)
    kw = {DGR_ARG[k]: t for k, t in leaf.items() if k in DGR_ARG}
    color, radii, depth, alpha = dgr.GaussianRasterizer(_settings(v, dev, deg, mod, bg))(
        leaf["means3d"], m2d, leaf["opacities"], **kw, return_alpha=True)
    assert alpha.shape == (1, v.height, v.width) and alpha.requires_grad
    loss = 0.0
    if gC is not None:
        loss = loss + (color * torch.from_numpy(gC).to(dev)).sum()
    if gD is not None:
        loss = loss + (depth[0] * torch.from_numpy(gD).to(dev)).sum()
    if gA is not None:
        loss = loss + (alpha[0] * torch.as_tensor(gA, device=dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = {ORACLE_KEY[k]: t.grad.detach().cpu().numpy().reshape(X[k].shape) for k, t in leaf.items()}
    got["means2d"] = m2d.grad.detach().cpu().numpy()
    return got, radii.cpu().numpy(), alpha.detach()


# ---- 1. the alpha output -------------------------------------------------------------------------------------------------
def test_alpha_output_is_one_minus_final_T_and_matches_oracle(oracle, gpu_device):
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    from pegasus_amd.gaussian_renderer import render
    from test_train_gpu import _c1_model, _camera
    P, v = single_scene("cube")
    X, deg = mode_inputs(P, "sh3_16")
    rs = _settings(v, gpu_device, deg, 1.0)
    t = {k: torch.from_numpy(a).to(gpu_device) for k, a in X.items()}
    args = (t["means3d"], None, t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, rs)
    with torch.no_grad():
        _, _, _, final_T, _ = dgr.rasterize_gaussians(*args, want_aux=True)
        out = dgr.GaussianRasterizer(rs)(t["means3d"], None, t["opacities"], shs=t["shs"], scales=t["scales"],
                                         rotations=t["rotations"], return_alpha=True)
    assert len(out) == 4 and torch.equal(out[3], (1.0 - final_T).unsqueeze(0))
    o = oracle.forward(**X, sh_degree=deg, **v.raster_kwargs(BG), num_threads=16, cull_mode=1)
    ok = ~o["ambig"].astype(bool)
    err = np.abs(out[3][0].cpu().numpy() - (1.0 - o["final_T"]))[ok]
    assert err.max() <= 1e-4, err.max()
    assert (1.0 - o["final_T"]).max() > 0.9
    # render(): "alpha" only when asked, bit for bit the want_aux final_T; the default dict keeps its five keys
    m, views = _c1_model(gpu_device)
    cam = _camera(views[0], gpu_device)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.tensor(BG, device=gpu_device)
    with torch.no_grad():
        plain = render(cam, m, pipe, bg)
        withA = render(cam, m, pipe, bg, return_alpha=True)
    assert set(plain) == {"render", "depth", "viewspace_points", "visibility_filter", "radii"}
    assert set(withA) == set(plain) | {"alpha"}
    for k in ("render", "depth", "radii"):
        assert torch.equal(plain[k], withA[k]), k
    g = render(cam, m, pipe, bg, return_alpha=True)          # the autograd path gives the same alpha
    assert torch.equal(g["alpha"].detach(), withA["alpha"]) and g["alpha"].requires_grad
    assert torch.equal(g["render"].detach(), plain["render"])


# ---- 2. the single-view alpha gradient against the oracle ---------------------------------------------------------------
ALPHA_CASES = ([(s, m) for s in ("tiny", "ragged", "cube", "opaque", "frustum") for m in ("sh3_16", "colors", "cov3d")] +
               [("px1x1", "sh3_16"), ("px17x3", "sh1_16"), ("tiny", "sh0_1"), ("opaque", "sh0_16")])


def check_alpha(oracle, X, v, deg, mod, dev, alpha_only=False, tag=""):
    gC, gD, o = _weights(oracle, X, v, deg, mod, 11)
    gA = gC[0].copy()
    if alpha_only:
        # alpha alone: with zero colours and bg = (1, 0, 0) the red image IS T = 1 - alpha, so the oracle's colour-only
        # backward with G = (g_a, 0, 0) is minus the alpha gradient (the colour inputs get none: alpha does not see them)
        gC = np.zeros_like(gC)
        gC[0] = gA
        got, radii, _ = hip_alpha_backward(X, v, deg, mod, None, None, gA, dev)
        Xo = {k: a for k, a in X.items() if k not in ("shs", "colors_precomp")}
        Xo["colors_precomp"] = np.zeros((X["means3d"].shape[0], 3), np.float32)
        ref = oracle.backward(**Xo, sh_degree=deg, scale_modifier=mod, grad_color=gC, grad_depth=np.zeros_like(gD),
                              **v.raster_kwargs(E0), num_threads=16)
        for k in ("shs", "colors"):
            if k in got:
                assert not got.pop(k).any(), "alpha does not depend on colour"
        ref = {k: -ref[k] for k in got}
    else:
        got, radii, _ = hip_alpha_backward(X, v, deg, mod, gC, gD, gA, dev)
        ref = oracle.backward(**X, sh_degree=deg, scale_modifier=mod, grad_color=gC, grad_depth=gD,
                              **v.raster_kwargs(np.asarray(BG) - E0), num_threads=16)
    np.testing.assert_array_equal(radii, o["radii"], err_msg=tag)
    ref = {k: ref[k] for k in got}
    for k, g in got.items():
        assert not g[radii == 0].any(), (tag, k)
    return got, ref, o


@pytest.mark.parametrize("scene,mode", ALPHA_CASES, ids=[f"{s}-{m}" for s, m in ALPHA_CASES])
def test_alpha_gradient_matches_oracle_per_element(oracle, gpu_device, scene, mode):
    P, v = single_scene(scene)
    X, deg = mode_inputs(P, mode)
    got, ref, o = check_alpha(oracle, X, v, deg, 1.0, gpu_device, tag=f"{scene}/{mode}")
    worst = assert_grads_match(got, ref, f"{scene}/{mode}", bounds=ROUNDING_BOUNDS)
    print(f"\nALPHA-RATIO {scene}/{mode}: " + " ".join(f"{k} {r:.3g}" for k, r in worst.items()))
    assert np.abs(ref["opacities"]).max() > 0


@pytest.mark.parametrize("scene", ["tiny", "opaque", "cube"])
def test_alpha_only_loss_matches_oracle(oracle, gpu_device, scene):
    P, v = single_scene(scene)
    X, deg = mode_inputs(P, "sh3_16")
    got, ref, _ = check_alpha(oracle, X, v, deg, 1.0, gpu_device, alpha_only=True, tag=scene)
    assert_grads_match(got, ref, f"alpha-only/{scene}", bounds=ROUNDING_BOUNDS)
    assert np.abs(ref["opacities"]).max() > 0


# ---- 3. consistency on arbitrary weights: bg = b with g_a = 0 equals bg = 0 with g_a = -(b . G) --------------------------
@pytest.mark.parametrize("scene", ["cube", "opaque", "c3"])
def test_background_equals_alpha_weight(gpu_device, scene):
    import torch
    if scene == "c3":               # the C3 scene at full size (2 M Gaussians, 800 x 800), one spread view
        from pegasus_amd import scenes
        cloud, views = scenes.scene_c3(n_views=512)
        act = cloud.activated()
        X = {k: np.ascontiguousarray(act[k], np.float32) for k in ("means3d", "opacities", "scales", "rotations", "shs")}
        v, deg = views[300], 3
    else:
        P, v = single_scene(scene)
        X, deg = mode_inputs(P, "sh3_16")
    rng = np.random.default_rng(3)
    G = rng.normal(size=(3, v.height, v.width)).astype(np.float32)
    b = np.array([0.3, 0.7, 0.45], np.float32)
    a, _, _ = hip_alpha_backward(X, v, deg, 1.0, G, None, None, gpu_device, bg=b)
    gA = -(b[:, None, None] * G).sum(0)
    c, _, _ = hip_alpha_backward(X, v, deg, 1.0, G, None, gA, gpu_device, bg=np.zeros(3, np.float32))
    worst = assert_grads_match(c, a, f"bg-vs-alpha/{scene}", rel=1e-3, floor=1e-5,
                               bounds=dict(rotations=15.0, scales=15.0) if scene == "c3" else ROUNDING_BOUNDS)
    print(f"\nBG-ALPHA {scene}: " + " ".join(f"{k} {r:.3g}" for k, r in worst.items()))
    torch.cuda.empty_cache()


# ---- 4. bit-equality of the NULL paths ------------------------------------------------------------------------------------
def _grads_via(X, v, deg, gC, gD, mode, dev):
    """mode: 'null' (pgr_backward with grad_alpha NULL), 'zero' (an all-zero grad_alpha)."""
    import torch
    ga = np.zeros((v.height, v.width), np.float32) if mode == "zero" else None
    got, _, _ = hip_alpha_backward(X, v, deg, 1.0, gC, gD, ga, dev)
    return {k: torch.from_numpy(g) for k, g in got.items()}


@pytest.mark.parametrize("scene", ["tiny", "cube", "opaque"])
def test_null_and_zero_alpha_are_bit_identical_to_pgr_backward(gpu_device, scene):
    import torch
    P, v = single_scene(scene)
    X, deg = mode_inputs(P, "sh3_16")
    rng = np.random.default_rng(1)
    gC = rng.normal(size=(3, v.height, v.width)).astype(np.float32)
    gD = rng.normal(size=(v.height, v.width)).astype(np.float32)
    # one Gaussian per pixel block at most on 'tiny' / a sorted walk: the atomics' order is fixed only where one entry
    # reaches a row per block; compare two runs of the SAME call first to know what is deterministic
    null = _grads_via(X, v, deg, gC, gD, "null", gpu_device)
    null2 = _grads_via(X, v, deg, gC, gD, "null", gpu_device)
    zero = _grads_via(X, v, deg, gC, gD, "zero", gpu_device)
    for k in null:
        if not torch.equal(null[k], null2[k]):        # float atomics in a different order: not comparable bit for bit
            torch.testing.assert_close(zero[k], null[k], rtol=1e-5, atol=1e-6 * float(null[k].abs().max()))
            continue
        assert torch.equal(zero[k], null[k]), (scene, k)


def test_masked_loss_with_unit_mask_is_pgr_image_loss(gpu_device):
    import torch
    from pegasus_amd.train_ops import image_loss_terms, masked_image_loss_terms
    g = torch.Generator(device="cpu").manual_seed(2)
    H, W = 37, 53
    x, y = torch.rand((3, H, W), generator=g).to(gpu_device), torch.rand((3, H, W), generator=g).to(gpu_device)
    a = torch.rand((1, H, W), generator=g).to(gpu_device)
    bg = torch.tensor([0.3, 0.2, 0.9], device=gpu_device)
    out, grad = image_loss_terms(x, y, 0.2)
    for alpha in (None, a):
        out4, grad4, ga = masked_image_loss_terms(x, alpha, y, torch.ones((H, W), device=gpu_device), bg, 0.2, 0.0)
        assert torch.equal(out4[:3], out) and torch.equal(grad4, grad)
        if alpha is not None:
            assert not ga.any()
    out4, grad4, ga = masked_image_loss_terms(x, None, y, None, None, 0.2, 0.0)
    assert torch.equal(out4[:3], out) and torch.equal(grad4, grad) and float(out4[3]) == 0.0 and ga is None


# ---- 5. batch ---------------------------------------------------------------------------------------------------------------
def _batch_setup(V):
    from test_batch_backward_gpu import _views
    from test_backward import tiny_scene
    P, _ = tiny_scene(3, n=40, W=80, H=64)
    return {k: np.asarray(a, np.float32) for k, a in P.items()}, _views(V, 80, 64, dist=2.5)


@pytest.mark.parametrize("V", [1, 2, 4, 8, 17])
def test_batch_ex_sums_single_view_ex(monkeypatch, gpu_device, V):
    """A batch pgr_backward against the sum of single-view pgr_backward calls; every third view hands the batch a NULL
    grad_alpha (its alpha takes no part in the loss), the others an alpha weight."""
    import torch
    from pegasus_amd import _lib
    from pegasus_amd import diff_gaussian_rasterization as dgr
    from test_batch_backward_gpu import _leaves, _settings as bsettings
    P, views = _batch_setup(V)
    x, deg = _leaves(P, gpu_device, "sh3")
    rng = np.random.default_rng(V)
    H, W = views[0].height, views[0].width
    wc = [rng.normal(size=(3, H, W)).astype(np.float32) for _ in range(V)]
    wa = [None if v % 3 == 2 else rng.normal(size=(H, W)).astype(np.float32) for v in range(V)]
    bgs = [(0.1 * v % 1.0, 0.4, 0.2) for v in range(V)]
    kw = {k: t for k, t in x.items() if k not in ("means3D", "opacities")}
    sums, m2ds = None, []
    for v in range(V):
        for t in x.values():
            t.grad = None
        m2d = torch.zeros_like(x["means3D"], requires_grad=True)
        color, _, _, alpha = dgr.GaussianRasterizer(bsettings(views[v], gpu_device, bgs[v], deg))(
            x["means3D"], m2d, x["opacities"], **kw, return_alpha=True)
        loss = (color * torch.as_tensor(wc[v], device=gpu_device)).sum()
        if wa[v] is not None:
            loss = loss + (alpha[0] * torch.as_tensor(wa[v], device=gpu_device)).sum()
        loss.backward()
        g = {k: t.grad.clone() for k, t in x.items()}
        sums = g if sums is None else {k: sums[k] + g[k] for k in g}
        m2ds.append(m2d.grad.clone())
    L = _lib.lib()
    real = L.pgr_backward
    seen = {}

    def with_nulls(call, stream):
        arr = (C.c_void_p * call.n_views)(*[None if wa[v] is None else call.grad_alpha[v] for v in range(call.n_views)])
        seen["nulls"] = sum(1 for v in range(call.n_views) if arr[v] is None)
        call.grad_alpha = arr
        return real(call, stream)
    monkeypatch.setattr(L, "pgr_backward", with_nulls, raising=False)
    for t in x.values():
        t.grad = None
    m2d = torch.zeros((V,) + tuple(x["means3D"].shape), device=gpu_device, requires_grad=True)
    color, _, _, alpha = dgr.rasterize_gaussians_batch(x["means3D"], m2d, x["opacities"],
                                                       [bsettings(vw, gpu_device, bg, deg) for vw, bg in zip(views, bgs)],
                                                       **kw, return_alpha=True)
    assert alpha.shape == (V, 1, H, W)
    loss = 0.0
    for v in range(V):
        loss = loss + (color[v] * torch.as_tensor(wc[v], device=gpu_device)).sum()
        if wa[v] is not None:
            loss = loss + (alpha[v, 0] * torch.as_tensor(wa[v], device=gpu_device)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert seen["nulls"] == sum(w is None for w in wa)
    for k, t in x.items():
        ref = sums[k]
        assert float((t.grad - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1e-12), k
    for v in range(V):
        ref = m2ds[v]
        assert float((m2d.grad[v] - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1e-12), v


# ---- 6. the masked loss -----------------------------------------------------------------------------------------------------
from train_reference import masked_loss_f64 as _reference_masked      # noqa: E402  (float64 autograd, shared)


@pytest.mark.parametrize("hw,lam,lam_a", [((37, 53), 0.2, 0.5), ((16, 16), 0.0, 1.0), ((70, 45), 1.0, 0.3),
                                          ((129, 97), 0.2, 0.0)])
def test_masked_loss_matches_float64_autograd(gpu_device, hw, lam, lam_a):
    import torch
    from pegasus_amd.train_ops import MaskedImageLoss
    H, W = hw
    g = torch.Generator(device="cpu").manual_seed(H * W)
    x = torch.rand((3, H, W), generator=g)
    y = torch.rand((3, H, W), generator=g)
    m = torch.clamp(torch.rand((1, H, W), generator=g) * 1.6 - 0.3, 0.0, 1.0)       # soft, with exact 0s and 1s
    a = torch.rand((1, H, W), generator=g)
    bg = torch.tensor([0.25, 0.6, 0.1])
    ref = _reference_masked(x, a, y, m, bg, lam, lam_a)
    xd, ad = x.to(gpu_device).requires_grad_(True), a.to(gpu_device).requires_grad_(True)
    loss = MaskedImageLoss.apply(xd, ad, y.to(gpu_device), m.to(gpu_device), bg.to(gpu_device), lam, lam_a)
    loss.backward()
    assert abs(float(loss) - ref[0]) <= 1e-5 * max(1.0, abs(ref[0]))
    gx, ga = xd.grad.cpu().double(), ad.grad.cpu().double()
    n = 3 * H * W
    assert float((gx - ref[4]).abs().max()) <= 1e-3 / n + 1e-4 * float(ref[4].abs().max())
    # sign(a - m) / (H W): exact up to the float factor, except where a == m (none here)
    assert float((ga - ref[5]).abs().max()) <= 1e-6 * max(float(ref[5].abs().max()), 1e-12) + 1e-12
    # determinism: a second run gives the same bits
    xd2, ad2 = x.to(gpu_device).requires_grad_(True), a.to(gpu_device).requires_grad_(True)
    loss2 = MaskedImageLoss.apply(xd2, ad2, y.to(gpu_device), m.to(gpu_device), bg.to(gpu_device), lam, lam_a)
    loss2.backward()
    assert torch.equal(loss2, loss) and torch.equal(xd2.grad, xd.grad) and torch.equal(ad2.grad, ad.grad)


def test_masked_loss_of_matching_target_is_zero(gpu_device):
    import torch
    from pegasus_amd.train_ops import masked_image_loss_terms
    g = torch.Generator(device="cpu").manual_seed(9)
    H, W = 45, 38
    m = (torch.rand((1, H, W), generator=g) > 0.4).float()
    y = torch.rand((3, H, W), generator=g)
    bg = torch.tensor([0.5, 0.1, 0.8])
    x = y * m + bg.reshape(3, 1, 1) * (1 - m)              # y' exactly (m is 0 / 1)
    out, gx, ga = masked_image_loss_terms(x.to(gpu_device), m.to(gpu_device), y.to(gpu_device), m.to(gpu_device),
                                          bg.to(gpu_device), 0.2, 0.5)
    assert float(out[0]) == 0.0 and float(out[3]) == 0.0 and abs(float(out[2]) - 1.0) < 1e-6
    assert not gx.any() and not ga.any()


# ---- 7. end to end: an object trained from masks over clutter -------------------------------------------------------------
# Measured on one MI355X (2000 steps, 32 views of the seeded C1 cube composited over clutter, 256 x 256, 4 held-out views):
#   masked B = 1:                        IoU 0.991, mean alpha outside the mask 0.0024, masked PSNR gain +4.92 dB
#   masked B = 4 (random_background):    IoU 0.992, outside 0.0027, gain +5.09 dB
#   unmasked B = 1 (same data):          IoU 0.219, outside 0.986 (it paints the clutter with opaque Gaussians)
# The floors sit far from the masked runs (IoU 0.8, outside 0.05, gain 2.5 dB) and from the unmasked one (0.2).
IOU_FLOOR = 0.80
OUTSIDE_CEIL = 0.05
UNMASKED_OUTSIDE_FLOOR = 0.2
PSNR_GAIN_FLOOR = 2.5


def _write_masked_dataset(root, device):
    """test_train_gpu's dataset, re-rendered with alpha and composited over a seeded clutter texture; the masks are
    alpha > 0.5, in a mask directory named like the images."""
    import torch
    from PIL import Image
    from pegasus_amd import colmap_io as cio
    from pegasus_amd.gaussian_renderer import render
    from test_train_gpu import _c1_model, _camera, _write_dataset
    _write_dataset(root, device)
    m, _ = _c1_model(device, n=10_000)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    cams, imgs = cio.read_model(str(root))
    (root / "masks").mkdir()
    rng = np.random.default_rng(17)
    for im in imgs.values():
        info = [c for c in cio.camera_infos(str(root)) if c.image_name == im.name.rsplit(".", 1)[0]][0]
        cam = cio.load_camera(info, data_device=str(device))
        with torch.no_grad():
            pkg = render(cam, m, pipe, torch.zeros(3, device=device), return_alpha=True)
        col = pkg["render"].clamp(0, 1).permute(1, 2, 0).cpu().numpy()
        a = pkg["alpha"][0].cpu().numpy()[..., None]
        h, w = a.shape[:2]
        blocks = rng.uniform(0.0, 1.0, size=(h // 16 + 1, w // 16 + 1, 3))
        clutter = np.kron(blocks, np.ones((16, 16, 1)))[:h, :w] * 0.6 + 0.2
        img = col + (1.0 - a) * clutter
        Image.fromarray((img.clip(0, 1) * 255.0 + 0.5).astype(np.uint8), "RGB").save(root / "images" / im.name)
        Image.fromarray(((a[..., 0] > 0.5) * 255).astype(np.uint8), "L").save(root / "masks" / im.name)


def _run(src, out, masks, batch_size, random_background=False):
    import torch
    from pegasus_amd.train import training
    random.seed(0)
    torch.manual_seed(0)
    dataset = SimpleNamespace(sh_degree=3, source_path=str(src), model_path=str(out), images="images", resolution=-1,
                              white_background=False, data_device="cuda", eval=True, masks=masks)
    opt = SimpleNamespace(iterations=2000, densify_from_iter=100, densify_until_iter=1500, densification_interval=100,
                          position_lr_max_steps=2000, random_background=random_background)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    res = training(dataset, opt, pipe, [1, 2000], [], [], None, -1, quiet=True, batch_size=batch_size)
    return res


def _outside(res, src, device):
    """(IoU, mean alpha outside the mask, masked PSNR) on the held-out views, evaluated against masks whatever the run."""
    import torch
    from pegasus_amd import colmap_io as cio
    from pegasus_amd.train import evaluate_masked
    from pegasus_amd.gaussian_renderer import render
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    test = [cio.load_camera(c, masks=str(src / "masks")) for c in cio.split_train_test(cio.camera_infos(str(src)), True)[1]]
    bg = torch.zeros(3, device=device)
    _, p, _, iou = evaluate_masked(test, res["model"], pipe, bg)
    outs = []
    with torch.no_grad():
        for cam in test:
            a = render(cam, res["model"], pipe, bg, return_alpha=True)["alpha"]
            out = cam.gt_mask <= 0.5
            outs.append(float(a[out].mean()))
    return iou, sum(outs) / len(outs), p


def test_end_to_end_training_from_masks(gpu_device, tmp_path):
    src = tmp_path / "data"
    _write_masked_dataset(src, gpu_device)
    r1 = _run(src, tmp_path / "m1", str(src / "masks"), 1)
    r4 = _run(src, tmp_path / "m4", str(src / "masks"), 4, random_background=True)
    r0 = _run(src, tmp_path / "m0", "", 1)
    first, last = r1["reports"][1]["test"], r1["reports"][2000]["test"]
    assert set(last) == {"l1", "psnr", "alpha_l1", "iou"} and set(r0["reports"][2000]["test"]) == {"l1", "psnr"}
    s1, s4, s0 = (_outside(r, src, gpu_device) for r in (r1, r4, r0))
    print(f"\nmasked end to end: B=1 IoU {s1[0]:.3f} outside {s1[1]:.4f} PSNR {s1[2]:.2f} (gain "
          f"{last['psnr'] - first['psnr']:.2f}); B=4 IoU {s4[0]:.3f} outside {s4[1]:.4f} PSNR {s4[2]:.2f} (gain "
          f"{r4['reports'][2000]['test']['psnr'] - r4['reports'][1]['test']['psnr']:.2f}); "
          f"unmasked IoU {s0[0]:.3f} outside {s0[1]:.4f}")
    for s, r in ((s1, r1), (s4, r4)):
        assert s[0] >= IOU_FLOOR and s[1] <= OUTSIDE_CEIL, s
        gain = r["reports"][2000]["test"]["psnr"] - r["reports"][1]["test"]["psnr"]
        assert gain >= PSNR_GAIN_FLOOR, gain
    assert s0[1] >= UNMASKED_OUTSIDE_FLOOR and s0[1] >= 4 * max(s1[1], s4[1]), (s0, s1, s4)
