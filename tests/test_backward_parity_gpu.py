"""The HIP backward (pgr_backward through the drop-in GaussianRasterizer, a batch pgr_backward through
rasterize_gaussians_batch) against the oracle's backward, PER ELEMENT, for every gradient the ABI returns, in every
input mode training and the drop-in surface use, at the edges of the model (opaque stacks that reach the 0.99 alpha clamp
and the T < 1e-4 stop, Gaussians past the frustum clamp and at the near plane, one-pixel and ragged images), on the
hostile fuzz scenes of test_fuzz_parity.py, and for batches of 16, 17 and 33 views.

Comparison rules
  - the loss weights are zeroed on the oracle forward's ``ambig`` pixels (where v_exp_f32 and glibc expf may decide a
    threshold differently): elsewhere both sides blend the same entries and differ by rounding only;
  - per element: |g_hip - g_ora| <= 1e-3 |g_ora| + 1e-5 max|g_ora of the group| (helpers.assert_grads_match);
  - a Gaussian with radii == 0 gets exactly 0 in every output, and no output holds NaN or Inf (NaN means included).
The oracle itself is pinned to finite differences of a float64 forward by tests/test_backward_fd_host.py."""
import math

import numpy as np
import pytest

from helpers import assert_grads_match
from test_backward import loss_weights, tiny_scene
from test_backward_fd_host import _cov3d, _frustum_scene, alpha_clamp_scene

pytestmark = pytest.mark.gpu
BG = (0.2, 0.4, 0.1)
SCENE_KEYS = ("means3d", "opacities", "scales", "rotations", "shs", "colors_precomp", "cov3d_precomp")
ORACLE_KEY = dict(means3d="means3d", opacities="opacities", scales="scales", rotations="rotations", shs="shs",
                  colors_precomp="colors", cov3d_precomp="cov3d")
DGR_ARG = dict(shs="shs", colors_precomp="colors_precomp", scales="scales", rotations="rotations",
               cov3d_precomp="cov3D_precomp")
# Rounding, not an error of the chain: the quaternion gradient of a strongly anisotropic Gaussian (axis ratios of 10 to
# 100 in the C1 cube and the C3 scene) is a small difference of large products of the cov3D gradient, and that gradient
# is itself built from the conic partials the compositor sums with fp32 atomics in no fixed order.  Measured worst
# ratio on MI355X: 0.67 (C1 cube, 3 000 Gaussians), 2.9 (C3 at full size); every other group stays below 0.25 on the
# scenes of this module.  The bound is 4 for rotations; the full-size test sets its own (test_full_size_properties.py).
ROUNDING_BOUNDS = dict(rotations=4.0)


def _f32(P):
    return {k: np.ascontiguousarray(np.asarray(a, np.float32)) for k, a in P.items()}


def mode_inputs(P, mode, mod=1.0):
    """The rasterizer inputs of one input mode from a scene with 16-coefficient SH: (inputs, sh_degree).
    shD_16: SH degree D with [n,16,3] coefficients (the trainer's layout at every degree); sh0_1: [n,1,3];
    colors: colors_precomp; cov3d: cov3D_precomp (with degree-3 SH)."""
    base = dict(means3d=P["means3d"], opacities=P["opacities"])
    if mode.startswith("sh") and mode.endswith("_16"):
        return _f32(dict(base, scales=P["scales"], rotations=P["rotations"], shs=P["shs"])), int(mode[2])
    if mode == "sh0_1":
        return _f32(dict(base, scales=P["scales"], rotations=P["rotations"], shs=np.asarray(P["shs"])[:, :1])), 0
    if mode == "colors":
        rgb = np.clip(np.asarray(P["shs"])[:, 0] * 0.28 + 0.5, 0.05, 1.0)
        return _f32(dict(base, scales=P["scales"], rotations=P["rotations"], colors_precomp=rgb)), 0
    if mode == "cov3d":
        return _f32(dict(base, cov3d_precomp=_cov3d(P, mod), shs=P["shs"])), 3
    raise KeyError(mode)


def _settings(v, dev, deg, mod, bg=BG):
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    return dgr.GaussianRasterizationSettings(v.height, v.width, v.tanfovx, v.tanfovy, f(bg), float(mod),
                                             f(v.world_view_transform), f(v.full_proj_transform), int(deg),
                                             f(v.camera_center), False, False)


def _weights(oracle, X, v, deg, mod, seed, bg=BG):
    """Random loss weights with the oracle's ambiguous pixels zeroed, and the oracle forward."""
    o = oracle.forward(**X, sh_degree=deg, scale_modifier=mod, **v.raster_kwargs(bg), num_threads=16, cull_mode=1)
    gC, gD = loss_weights(seed, v.width, v.height)
    amb = o["ambig"].astype(bool)
    gC[:, amb] = 0.0
    gD[amb] = 0.0
    return gC.astype(np.float32), gD.astype(np.float32), o


def hip_backward(X, v, deg, mod, gC, gD, dev, bg=BG):
    """loss.backward() through the drop-in rasterizer: {oracle key: gradient} (means2d included) and the radii."""
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    leaf = {k: torch.from_numpy(a.reshape(-1, 1) if k == "opacities" else a).to(dev).requires_grad_(True)
            for k, a in X.items()}
    m2d = torch.zeros_like(leaf["means3d"], requires_grad=True)
    kw = {DGR_ARG[k]: t for k, t in leaf.items() if k in DGR_ARG}
    color, radii, depth = dgr.GaussianRasterizer(_settings(v, dev, deg, mod, bg))(leaf["means3d"], m2d,
                                                                                  leaf["opacities"], **kw)
    loss = (color * torch.from_numpy(gC).to(dev)).sum() + (depth[0] * torch.from_numpy(gD).to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = {ORACLE_KEY[k]: t.grad.detach().cpu().numpy().reshape(X[k].shape) for k, t in leaf.items()}
    got["means2d"] = m2d.grad.detach().cpu().numpy()
    return got, radii.cpu().numpy()


def check_single(oracle, X, v, deg, mod, dev, seed=5, tag="", bounds=None, bg=BG):
    gC, gD, o = _weights(oracle, X, v, deg, mod, seed, bg)
    got, radii = hip_backward(X, v, deg, mod, gC, gD, dev, bg)
    np.testing.assert_array_equal(radii, o["radii"], err_msg=tag)
    ref = oracle.backward(**X, sh_degree=deg, scale_modifier=mod, grad_color=gC, grad_depth=gD, **v.raster_kwargs(bg),
                          num_threads=16)
    ref = {k: ref[k] for k in got}
    dead = radii == 0
    for k, g in got.items():
        assert not g[dead].any(), (tag, k, "a Gaussian with radii == 0 got a gradient")
    if "shs" in got:          # coefficients above the active degree get exactly 0
        assert not got["shs"][:, (deg + 1) ** 2:].any(), tag
    worst = assert_grads_match(got, ref, tag, bounds=ROUNDING_BOUNDS if bounds is None else bounds)
    print(f"\nBWD-RATIO {tag}: " + " ".join(f"{k} {r:.3g}" for k, r in worst.items()))
    return got, ref, o, worst


# ---- scenes ----------------------------------------------------------------------------------------------------------
def opaque_stack():
    """80 Gaussians piled in front of the camera, opacities in [0.9, 1], ten of them exactly 1: entries reach the 0.99
    alpha clamp and pixels stop at T < 1e-4 well before the end of their tile's list."""
    P, v = tiny_scene(21, n=80, W=80, H=64)
    rng = np.random.default_rng(21)
    P["opacities"] = rng.uniform(0.9, 1.0, size=80)
    P["opacities"][rng.choice(80, 10, replace=False)] = 1.0
    P["scales"] = P["scales"] * 1.6
    return P, v


def frustum_edge():
    """_frustum_scene (centres at 1.6 x the clamp whose splats reach into the image) plus two Gaussians straight ahead
    with t_z just above and just below the 0.2 near plane."""
    P, v, _ = _frustum_scene()
    R, t = v.R_c2w.T, v.t_w2c
    near = np.array([R.T @ (np.array([0.01, -0.01, z]) - t) for z in (0.203, 0.197)])
    rng = np.random.default_rng(9)
    P = dict(means3d=np.concatenate([P["means3d"], near]), opacities=np.concatenate([P["opacities"], [0.5, 0.5]]),
             scales=np.concatenate([P["scales"], np.full((2, 3), 0.004)]),
             rotations=np.concatenate([P["rotations"], [[1.0, 0, 0, 0], [0.6, 0.8, 0, 0]]]),
             shs=np.concatenate([P["shs"], rng.normal(0, 0.25, size=(2, 16, 3))]))
    return P, v


def single_scene(name):
    from pegasus_amd import scenes
    if name == "tiny":
        return tiny_scene(3, n=40, W=80, H=64)
    if name == "ragged":
        return tiny_scene(7, n=60, W=77, H=53)
    if name == "px1x1":
        return tiny_scene(8, n=30, W=1, H=1)
    if name == "px17x3":
        return tiny_scene(9, n=30, W=17, H=3)
    if name == "cube":
        cloud, views = scenes.scene_c1(seed=4, n=3000)
        a = cloud.activated()
        return dict(means3d=a["means3d"], opacities=a["opacities"], scales=a["scales"], rotations=a["rotations"],
                    shs=a["shs"]), views[0]
    if name == "opaque":
        return opaque_stack()
    if name == "frustum":
        return frustum_edge()
    raise KeyError(name)


MODES = ["sh0_16", "sh1_16", "sh2_16", "sh3_16", "sh0_1", "colors", "cov3d"]
SINGLE = ([(s, m, 1.0) for s in ("tiny", "ragged", "cube", "opaque", "frustum") for m in MODES] +
          [("px1x1", "sh3_16", 1.0), ("px1x1", "cov3d", 1.0), ("px17x3", "sh1_16", 1.0), ("px17x3", "colors", 1.0)] +
          [("tiny", "sh3_16", 0.3), ("tiny", "sh1_16", 2.5), ("ragged", "sh2_16", 0.3), ("cube", "sh3_16", 2.5),
           ("cube", "sh0_16", 0.3), ("opaque", "sh3_16", 2.5), ("frustum", "sh1_16", 2.5), ("frustum", "colors", 2.5)])


@pytest.mark.parametrize("scene,mode,mod", SINGLE, ids=[f"{s}-{m}-x{k}" for s, m, k in SINGLE])
def test_single_view_matches_oracle_per_element(oracle, gpu_device, scene, mode, mod):
    P, v = single_scene(scene)
    X, deg = mode_inputs(P, mode, mod)
    got, ref, o, _ = check_single(oracle, X, v, deg, mod, gpu_device, tag=f"{scene}/{mode}/x{mod}")
    assert np.abs(ref["means3d"]).max() > 0
    if scene == "opaque":       # the edges were reached
        nc = o["n_contrib"].astype(np.int64)
        lens = (o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0])
        gx = (v.width + 15) // 16
        ty, tx = np.mgrid[0:v.height, 0:v.width] // 16
        stopped = (o["final_T"] < 1e-3) & (nc < lens[ty * gx + tx])
        assert stopped.sum() >= 50, "no pixel stopped at T < 1e-4 before the end of its list"
        xy, co = o["xy"], o["conic_opacity"]
        ys, xs = np.mgrid[0:v.height, 0:v.width]
        hit = 0
        for i in np.flatnonzero((o["radii"] > 0) & (co[:, 3] >= 0.99)):
            dx, dy = xy[i, 0] - xs, xy[i, 1] - ys
            power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
            hit += int((co[i, 3] * np.exp(power) >= 0.99).sum())
        assert hit > 0, "no entry reached the 0.99 alpha clamp"
    if scene == "frustum":
        t = np.c_[X["means3d"], np.ones(len(X["means3d"]))] @ np.asarray(v.world_view_transform, np.float64)[:, :3]
        past = np.maximum(np.abs(t[:, 0] / t[:, 2]) / (1.3 * v.tanfovx), np.abs(t[:, 1] / t[:, 2]) / (1.3 * v.tanfovy))
        live = o["radii"] > 0
        assert (live & (past >= 1.5)).sum() >= 3, "no live Gaussian past the frustum clamp"
        assert live[-2] and not live[-1], "the near-plane pair must straddle t_z = 0.2"
        assert np.abs(got["means3d"][live & (past >= 1.5)]).max() > 0


def test_alpha_clamp_known_answer_on_hip(oracle, gpu_device):
    """The straight-through 0.99 clamp on the HIP side: one Gaussian of opacity 1 centred on a pixel."""
    P, v, gC, gD, bg, expect = alpha_clamp_scene()
    got, radii = hip_backward(_f32(P), v, 0, 1.0, gC, gD, gpu_device, bg)
    assert radii[0] > 0
    assert abs(float(got["opacities"][0]) - expect) <= 1e-5 * abs(expect), (got["opacities"], expect)


@pytest.mark.parametrize("block", range(3))
def test_fuzz_scenes_match_oracle_per_element(oracle, gpu_device, block):
    """24 of test_fuzz_parity.py's hostile scenes (NaN means, opacity 0 and 1, quaternions x 9, zero scales, depth ties,
    screen-filling splats, one-pixel images) through the single-view backward with a random loss."""
    from test_fuzz_parity import _case
    for seed in range(block * 8, block * 8 + 8):
        act, view, deg, mod, bg = _case(seed)
        X = _f32(act)
        tag = f"fuzz seed {seed}: n {X['means3d'].shape[0]}, {view.width}x{view.height}, degree {deg}, modifier {mod}"
        check_single(oracle, X, view, deg, mod, gpu_device, seed=200 + seed, tag=tag, bg=bg)


# ---- batch ------------------------------------------------------------------------------------------------------------
def _batch_views(V, W, H):
    """V cameras around the cube; view 1 looks away from it (sees nothing), the last one repeats view 0."""
    from pegasus_amd import graphics as G, scenes
    fov = math.radians(50)
    views = []
    for k in range(V - 1):
        a = 2 * math.pi * k / (V - 1)
        eye = (2.8 * math.sin(a), -0.4 - 0.03 * k, -2.8 * math.cos(a))
        target = (0, 0, 0) if k != 1 else (2 * eye[0], 2 * eye[1], 2 * eye[2])
        R, t = G.look_at_opencv(eye, target, up=(0, -1, 0))
        views.append(scenes.make_view(R, t, W, H, fovx=fov, fovy=fov))
    return views + [views[0]]


@pytest.mark.parametrize("V", [16, 17, 33])
def test_batch_matches_sum_of_oracle_views(oracle, gpu_device, V):
    """A batch pgr_backward beyond one per-view table chunk (16 views) and on the split-views preprocess (N <= 400 k,
    V >= 16): summed gradients against the sum of per-view oracle backwards, and every view's means2D."""
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr, scenes
    cloud, _ = scenes.scene_c1(seed=4, n=3000)
    a = cloud.activated()
    X, deg = mode_inputs(dict(means3d=a["means3d"], opacities=a["opacities"], scales=a["scales"],
                              rotations=a["rotations"], shs=a["shs"]), "sh1_16")
    W = H = 96
    views = _batch_views(V, W, H)
    dev = gpu_device
    wts, refs = [], []
    for k, v in enumerate(views):
        gC, gD, o = _weights(oracle, X, v, deg, 1.0, 300 + (k % (V - 1)))
        if k == 1:
            assert not (o["radii"] > 0).any(), "view 1 must see nothing"
        wts.append((gC, gD))
        refs.append(oracle.backward(**X, sh_degree=deg, grad_color=gC, grad_depth=gD, **v.raster_kwargs(BG),
                                    num_threads=16))
    leaf = {k: torch.from_numpy(a_.reshape(-1, 1) if k == "opacities" else a_).to(dev).requires_grad_(True)
            for k, a_ in X.items()}
    m2d = torch.zeros((V,) + tuple(leaf["means3d"].shape), device=dev, requires_grad=True)
    color, radii, depth = dgr.rasterize_gaussians_batch(leaf["means3d"], m2d, leaf["opacities"],
                                                        [_settings(v, dev, deg, 1.0) for v in views], shs=leaf["shs"],
                                                        scales=leaf["scales"], rotations=leaf["rotations"])
    loss = 0.0
    for k, (gC, gD) in enumerate(wts):
        loss = loss + (color[k] * torch.from_numpy(gC).to(dev)).sum() + (depth[k, 0] * torch.from_numpy(gD).to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = {ORACLE_KEY[k]: t.grad.detach().cpu().numpy().reshape(X[k].shape) for k, t in leaf.items()}
    ref = {k: sum(r[k].astype(np.float64) for r in refs) for k in got}
    seen = (radii.cpu().numpy() > 0).any(axis=0)
    for k, g in got.items():
        assert not g[~seen].any(), (V, k)
    assert not got["shs"][:, (deg + 1) ** 2:].any()
    worst = assert_grads_match(got, ref, f"batch V={V}", bounds=ROUNDING_BOUNDS)
    m2 = m2d.grad.detach().cpu().numpy()
    w2 = 0.0
    for k in range(V):
        w2 = max(w2, assert_grads_match({"means2d": m2[k]}, {"means2d": refs[k]["means2d"]}, f"batch V={V} view {k}")["means2d"])
    assert_grads_match({"means2d": m2[V - 1]}, {"means2d": m2[0]}, f"batch V={V}: the duplicated view")
    assert not m2[1].any()
    print(f"\nBWD-RATIO batch V={V}: " + " ".join(f"{k} {r:.3g}" for k, r in worst.items()) + f" means2d[v] {w2:.3g}")
