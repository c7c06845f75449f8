"""Camera gradients of the HIP rasterizer (pgr_backward with PgrBackwardCall.camera_grads, through the autograd surface)
and pose refinement on them (pegasus_amd/camera_pose.py).

  - per element: dL/d(viewmatrix, projmatrix, campos) against central differences of the dense float64 forward
    (oracle/dense_ref.py) with respect to each of the 35 numbers, bound |d| <= 1e-3 |fd| + 1e-5 max|fd of the group|
    (groups viewmatrix / projmatrix / campos); entries the forward never reads get exactly 0;
  - a batch view's camera gradient equals the single-view call's; requesting camera gradients moves no scene gradient, and
    without a camera tensor that requires grad no new entry point is called;
  - at full size (C3, 2 M Gaussians, 800 x 800) the camera gradient agrees with the scene gradient through the identities
    of tests/test_camera_pose_host.py (translation at SH degree 3, rotation about the centre at SH degree 0);
  - a frozen model rendered from a camera that requires grad gives it a gradient;
  - render-and-compare refinement recovers a perturbed pose of the C1 cube."""
import math

import numpy as np
import pytest

from test_backward import loss_weights, tiny_scene
from test_backward_fd_host import _case

pytestmark = pytest.mark.gpu
BG = (0.2, 0.4, 0.1)
EPS = 1e-6
REL, FLOOR = 1e-3, 1e-5
GROUPS = (("viewmatrix", 0, 16), ("projmatrix", 16, 32), ("campos", 32, 35))
NEVER_READ = dict(viewmatrix=[3, 7, 11, 15], projmatrix=[2, 6, 10, 14])
ARG = dict(means3d="means3D", opacities="opacities", shs="shs", colors_precomp="colors_precomp", scales="scales",
           rotations="rotations", cov3d_precomp="cov3D_precomp")


def _t(a, dev, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(np.asarray(a, np.float32)), device=dev, requires_grad=grad)


def _settings(v, dev, deg, mod, cams=None, bg=BG):
    """Settings of view ``v``; ``cams``: (viewmatrix, projmatrix, campos) tensors to use (else fresh constants)."""
    from pegasus_amd import diff_gaussian_rasterization as dgr
    vm, pm, cp = cams if cams is not None else (_t(v.world_view_transform, dev), _t(v.full_proj_transform, dev),
                                                 _t(v.camera_center, dev))
    return dgr.GaussianRasterizationSettings(v.height, v.width, v.tanfovx, v.tanfovy, _t(bg, dev), float(mod), vm, pm,
                                             int(deg), cp, False, False)


def _cam_leaves(v, dev):
    return (_t(v.world_view_transform, dev, True), _t(v.full_proj_transform, dev, True), _t(v.camera_center, dev, True))


def _scene_inputs(P, dev, grad=True):
    return {ARG[k]: _t(a, dev, grad) for k, a in P.items()}


def hip_single(P, v, deg, mod, gC, gD, gA, dev, cam_grad=True):
    """(camera gradient [35] or None, {scene input: grad}) of L = <color, gC> + <depth, gD> (+ <alpha, gA>)."""
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    cams = _cam_leaves(v, dev) if cam_grad else None
    X = _scene_inputs(P, dev)
    out = dgr.GaussianRasterizer(_settings(v, dev, deg, mod, cams))(means2D=None, return_alpha=gA is not None, **X)
    loss = (out[0] * _t(gC, dev)).sum() + (out[2][0] * _t(gD, dev)).sum()
    if gA is not None:
        loss = loss + (out[3][0] * _t(gA, dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    g = None if cams is None else torch.cat([c.grad.reshape(-1) for c in cams]).cpu().numpy().astype(np.float64)
    return g, {k: x.grad.cpu().numpy() for k, x in X.items()}


def fd_camera(P64, v, deg, mod, gC, gD, gA):
    """Central differences of the dense forward's loss with respect to the 35 camera numbers (NaN where the two sides
    took different discrete decisions)."""
    from oracle.dense_ref import dense_forward, same_decisions
    base = dict(viewmatrix=np.asarray(v.world_view_transform, np.float64).reshape(-1).copy(),
                projmatrix=np.asarray(v.full_proj_transform, np.float64).reshape(-1).copy(),
                campos=np.asarray(v.camera_center, np.float64).reshape(-1).copy())
    common = dict(width=v.width, height=v.height, tanfovx=v.tanfovx, tanfovy=v.tanfovy, scale_modifier=mod)

    def loss(cam):
        c, d, dec = dense_forward(sh_degree=deg, **P64, **common, **cam, bg=np.asarray(BG, np.float64),
                                  return_decisions=True)
        total = float((c * gC).sum() + (d * gD).sum())
        if gA is not None:       # alpha = the colour of white Gaussians on black
            Pw = {k: a for k, a in P64.items() if k not in ("shs", "colors_precomp")}
            a, _, _ = dense_forward(sh_degree=0, **Pw, colors_precomp=np.ones((P64["means3d"].shape[0], 3)), **common,
                                    **cam, bg=np.zeros(3), return_decisions=True)
            total += float((a[0] * gA).sum())
        return total, dec

    out = np.full(35, np.nan)
    for name, a, b in GROUPS:
        for j in range(b - a):
            cp, cm = {k: x.copy() for k, x in base.items()}, {k: x.copy() for k, x in base.items()}
            cp[name][j] += EPS
            cm[name][j] -= EPS
            (lp, dp), (lm, dm) = loss(cp), loss(cm)
            if same_decisions(dp, dm):
                out[a + j] = (lp - lm) / (2 * EPS)
    return out


def _ambig_free(oracle, P, v, deg, mod, *planes):
    """The loss weights with the oracle forward's ambiguous pixels zeroed (there v_exp_f32 and expf may decide a
    threshold differently)."""
    o = oracle.forward(**{k: np.asarray(a, np.float32) for k, a in P.items()}, sh_degree=deg, scale_modifier=mod,
                       **v.raster_kwargs(BG), num_threads=16, cull_mode=1)
    amb = o["ambig"].astype(bool)
    out = []
    for p in planes:
        if p is None:
            out.append(None)
            continue
        p = np.array(p, np.float64)
        p[..., amb] = 0.0
        out.append(p)
    return out


CASES = ["deg0", "deg1", "deg2", "deg3", "mod0.3", "mod2.5", "cov3d", "colors", "frustum", "depth_only", "alpha_only"]


@pytest.mark.parametrize("case", CASES)
def test_camera_gradient_matches_fd_per_element(oracle, gpu_device, case):
    P, v, deg, mod, gC, gD = _case("depth_only" if case == "alpha_only" else case)
    gA = None
    if case == "alpha_only":
        gD = np.zeros_like(gD)
        gA = np.random.default_rng(9).normal(size=(v.height, v.width))
    gC, gD, gA = _ambig_free(oracle, P, v, deg, mod, gC, gD, gA)
    g, _ = hip_single(P, v, deg, mod, gC, gD, gA, gpu_device)
    fd = fd_camera(P, v, deg, mod, gC, gD, gA)
    assert np.isfinite(g).all()
    kept = np.isfinite(fd)
    assert kept.sum() >= 0.9 * 35, ("discarded", int((~kept).sum()))
    worst = {}
    for name, a, b in GROUPS:
        for j in NEVER_READ.get(name, []):
            assert g[a + j] == 0.0, (name, j, g[a + j])
        ref, got = fd[a:b], g[a:b]
        m = np.isfinite(ref)
        scale = np.abs(ref[m]).max()
        if name == "campos" and ("shs" not in P or deg == 0 or not gC.any()):
            # no view-dependent colour in the loss: nothing depends on campos
            assert scale == 0 and not got.any(), (case, "campos", got, ref)
            continue
        assert scale > 0, (case, name)
        ratio = np.abs(got[m] - ref[m]) / (REL * np.abs(ref[m]) + FLOOR * scale)
        worst[name] = float(ratio.max())
        k = int(ratio.argmax())
        assert ratio[k] <= 1.0, (case, name, "entry", np.flatnonzero(m)[k], "hip", got[m][k], "fd", ref[m][k], ratio[k])
    print(f"\nCAMERA-FD-RATIO {case}: " + " ".join(f"{k} {r:.3g}" for k, r in worst.items()) +
          f" discarded {int((~kept).sum())}/35")


def _ring_views(n, W=48, H=32, dist=2.5):
    from pegasus_amd import graphics as G, scenes
    fov = math.radians(55)
    out = []
    for k in range(n):
        a = 2 * math.pi * k / n
        eye = (dist * math.sin(a) + 0.1, -0.2 + 0.05 * k % 3, -dist * math.cos(a))
        R, t = G.look_at_opencv(eye, (0, 0, 0), up=(0, -1, 0))
        out.append(scenes.make_view(R, t, W, H, fovx=fov, fovy=fov * H / W))
    return out


@pytest.mark.parametrize("V", [2, 16, 17])
def test_batch_camera_gradient_matches_single_view(gpu_device, V):
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    P, _ = tiny_scene(0)
    P = {k: np.asarray(a, np.float32) for k, a in P.items()}
    views = _ring_views(V)
    weights = [loss_weights(v, views[v].width, views[v].height) for v in range(V)]
    cams = [_cam_leaves(v, gpu_device) for v in views]
    X = _scene_inputs(P, gpu_device)
    sets = [_settings(v, gpu_device, 3, 1.0, c) for v, c in zip(views, cams)]
    color, _, depth = dgr.rasterize_gaussians_batch(X["means3D"], None, X["opacities"], sets, shs=X["shs"],
                                                    scales=X["scales"], rotations=X["rotations"])
    loss = sum((color[v] * _t(weights[v][0], gpu_device)).sum() + (depth[v, 0] * _t(weights[v][1], gpu_device)).sum()
               for v in range(V))
    loss.backward()
    for v in range(V):
        got = torch.cat([c.grad.reshape(-1) for c in cams[v]]).cpu().numpy()
        ref, _ = hip_single(P, views[v], 3, 1.0, weights[v][0], weights[v][1], None, gpu_device)
        for name, a, b in GROUPS:
            scale = np.abs(ref[a:b]).max()
            ratio = np.abs(got[a:b] - ref[a:b]) / (REL * np.abs(ref[a:b]) + FLOOR * scale + 1e-30)
            assert ratio.max() <= 1.0, (V, v, name, got[a:b], ref[a:b])


class _Spy:
    """The library with its backward calls recorded: (entry name, whether camera_grads was NULL)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("pgr_backward") or name.endswith("_bytes"):
            return f

        def wrapped(call, stream):
            self.calls.append((name, not call.camera_grads))
            return f(call, stream)
        return wrapped


@pytest.mark.parametrize("batch", [False, True])
def test_camera_gradients_move_nothing_else(gpu_device, monkeypatch, batch):
    import torch
    from pegasus_amd import _lib, diff_gaussian_rasterization as dgr
    from helpers import assert_grads_match
    P, v = tiny_scene(1)
    P = {k: np.asarray(a, np.float32) for k, a in P.items()}
    views = _ring_views(3) if batch else [v]
    gC, gD = loss_weights(1, views[0].width, views[0].height)
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: spy)

    def run(cam_grad):
        X = _scene_inputs(P, gpu_device)
        cams = [_cam_leaves(w, gpu_device) if cam_grad else None for w in views]
        sets = [_settings(w, gpu_device, 3, 1.0, c) for w, c in zip(views, cams)]
        if batch:
            color, _, depth = dgr.rasterize_gaussians_batch(X["means3D"], None, X["opacities"], sets, shs=X["shs"],
                                                            scales=X["scales"], rotations=X["rotations"])
            loss = (color * _t(gC, gpu_device)).sum() + (depth[:, 0] * _t(gD, gpu_device)).sum()
        else:
            color, _, depth = dgr.GaussianRasterizer(sets[0])(means2D=None, **X)
            loss = (color * _t(gC, gpu_device)).sum() + (depth[0] * _t(gD, gpu_device)).sum()
        loss.backward()
        torch.cuda.synchronize()
        return {k: x.grad.cpu().numpy() for k, x in X.items()}

    plain = run(False)
    assert spy.calls == [("pgr_backward", True)], spy.calls
    spy.calls.clear()
    with_cam = run(True)
    assert spy.calls == [("pgr_backward", False)], spy.calls
    assert_grads_match(with_cam, plain, "camera grads requested", bounds=dict(rotations=4.0))


def test_frozen_model_camera_gets_a_gradient(gpu_device):
    """Only the view matrix requires grad: the render still takes the differentiable path (at the parent commit it went
    through the no-grad forward and the view matrix got nothing)."""
    from pegasus_amd import diff_gaussian_rasterization as dgr
    P, v = tiny_scene(0)
    X = _scene_inputs(P, gpu_device, grad=False)
    vm = _t(v.world_view_transform, gpu_device, True)
    s = _settings(v, gpu_device, 3, 1.0, (vm, _t(v.full_proj_transform, gpu_device), _t(v.camera_center, gpu_device)))
    color, _, depth = dgr.GaussianRasterizer(s)(means2D=None, **X)
    (color.square().sum() + depth.sum()).backward()
    assert vm.grad is not None and vm.grad.shape == (4, 4) and vm.grad.abs().sum() > 0
    assert (vm.grad[:, 3] == 0).all()


# ---- full size ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def c3_cloud():
    from pegasus_amd import scenes
    cloud, views = scenes.scene_c3(n_views=512)
    return cloud.activated(), [views[i] for i in (100, 300)]


def _cameras(views, dev):
    from pegasus_amd.cameras import Camera
    return [Camera(colmap_id=k, R=v.R_c2w, T=v.t_w2c, FoVx=v.fovx, FoVy=v.fovy, image=None, gt_alpha_mask=None,
                   image_name=str(k), uid=k, data_device=dev, image_width=v.width, image_height=v.height)
            for k, v in enumerate(views)]


@pytest.mark.parametrize("n_views", [1, 2])
@pytest.mark.parametrize("identity", ["a", "b"])
def test_full_size_camera_gradient_identities(c3_cloud, gpu_device, n_views, identity):
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    from pegasus_amd.camera_pose import PosedCamera
    act, views = c3_cloud
    views = views[:n_views]
    deg = 3 if identity == "a" else 0
    dev = gpu_device
    for v in range(n_views):          # one loss per view, each its own backward: the identity holds view by view
        means = _t(act["means3d"], dev, True)
        rots = _t(act["rotations"], dev, True)
        deltas = [torch.zeros(6, device=dev, requires_grad=True) for _ in views]
        posed = [PosedCamera(c, d) for c, d in zip(_cameras(views, dev), deltas)]
        sets = [_settings(w, dev, deg, 1.0, (p.world_view_transform, p.full_proj_transform, p.camera_center))
                for w, p in zip(views, posed)]
        kw = dict(shs=_t(act["shs"], dev), scales=_t(act["scales"], dev), rotations=rots)
        gC, gD = loss_weights(v, views[v].width, views[v].height)
        if n_views == 1:
            color, _, depth = dgr.GaussianRasterizer(sets[0])(means3D=means, means2D=None,
                                                              opacities=_t(act["opacities"], dev), **kw)
        else:
            color, _, depth = dgr.rasterize_gaussians_batch(means, None, _t(act["opacities"], dev), sets, **kw)
            color, depth = color[v], depth[v]
        loss = (color * _t(gC, dev)).sum() + (depth[0] * _t(gD, dev)).sum()
        loss.backward()
        R = torch.tensor(np.asarray(views[v].R_c2w, np.float64).T, device=dev)      # world -> camera
        gp = means.grad.double()
        if identity == "a":
            a = deltas[v].grad[3:].double()
            b = R @ gp.sum(0)
        else:
            c = posed[v].camera_center.detach().double()
            q, gq = rots.detach().double(), rots.grad.double()
            w_means = torch.linalg.cross(means.detach().double() - c, gp, dim=1).sum(0)
            w_quat = 0.5 * (-gq[:, :1] * q[:, 1:] + q[:, :1] * gq[:, 1:] + torch.linalg.cross(q[:, 1:], gq[:, 1:], dim=1)).sum(0)
            a = deltas[v].grad[:3].double()
            b = R @ (w_means + w_quat)
        err = float((a - b).norm() / b.norm())
        print(f"\nIDENTITY-{identity} views {n_views} view {v}: |a - b| / |b| = {err:.3g}  a {a.cpu().numpy()} b {b.cpu().numpy()}")
        assert err <= 1e-3, (identity, n_views, v, err)


# ---- pose refinement ----------------------------------------------------------------------------------------------------

def _perturbation(seed, deg, frac, dist):
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    tr = rng.normal(size=3)
    return np.r_[ax / np.linalg.norm(ax) * math.radians(deg), tr / np.linalg.norm(tr) * frac * dist]


def test_refine_pose_recovers_c1_cube_pose(gpu_device):
    import torch
    from pegasus_amd import scenes
    from pegasus_amd.camera_pose import PosedCamera, refine_pose, rotation_error_deg
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.gaussian_renderer import render
    from types import SimpleNamespace
    cloud, views = scenes.scene_c1()
    model = GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling,
                                      cloud.rotation, sh_degree=3, device=gpu_device)
    true = _cameras(views, gpu_device)[0]
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    bg = torch.zeros(3, device=gpu_device)
    with torch.no_grad():
        tgt = render(true, model, pipe, bg, return_alpha=True)
    dist = 3.0
    R0, t0 = PosedCamera(true, torch.zeros(6, device=gpu_device)).pose()
    # the model-to-camera pose perturbed about the model's centre: R = dR R0, t = t0 + dt
    pivot = R0 @ model.get_xyz.detach().mean(0).double().cpu().numpy() + t0
    start = PosedCamera(true, torch.tensor(_perturbation(4, 3.0, 0.03, dist), dtype=torch.float32, device=gpu_device),
                        pivot).refined()
    Rs, ts = PosedCamera(start, torch.zeros(6, device=gpu_device)).pose()
    cam, (R, t), hist = refine_pose(model, start, tgt["render"], tgt["alpha"], iterations=300)
    rot_err, tr_err = rotation_error_deg(R, R0), float(np.linalg.norm(t - t0)) / dist
    print(f"\nREFINE-POSE start {rotation_error_deg(Rs, R0):.3f} deg {np.linalg.norm(ts - t0) / dist:.4f}; "
          f"after {len(hist)} steps {rot_err:.4f} deg {tr_err:.5f} of the distance; loss {hist[0]:.4g} -> {hist[-1]:.4g}")
    assert len(hist) == 300 and hist[-1] < hist[0]
    assert rot_err <= 0.1 and tr_err <= 0.002
    assert all(not p.requires_grad or p.grad is None for p in (model._xyz, model._opacity))
