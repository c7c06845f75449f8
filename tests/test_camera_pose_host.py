"""The pose parameterisation of camera refinement (pegasus_amd/camera_pose.py) on the host, and the construction the GPU
camera-gradient tests rest on (tests/test_camera_grad_gpu.py), checked with central differences of the dense float64
forward (oracle/dense_ref.py; eps = 1e-6, samples across a kink of the model discarded by ``same_decisions``):

  (a) moving the camera by tau (W2C' = exp((0, tau)) W2C) renders what moving every mean by R^T tau renders;
  (b) rotating the camera about its centre (W2C' = exp((omega, 0)) W2C), at SH degree 0, renders what rotating every mean
      about the centre and every quaternion (left multiplication) by Q = exp(R^T omega) renders."""
import math

import numpy as np
import pytest
import torch

from test_backward import loss_weights, tiny_scene

EPS = 1e-6


def _axis_angle_matrix(w, tau):
    """4x4 from the axis-angle form, written out directly (float64 numpy, unit axis k, angle th):
    R = cos I + sin [k]x + (1 - cos) k k^T,  t = V tau,  V = I + (1 - cos)/th [k]x + (th - sin)/th [k]x^2."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = math.cos(th) * np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * np.outer(k, k)
    V = np.eye(3) + (1 - math.cos(th)) / th * Kx + (th - math.sin(th)) / th * (Kx @ Kx)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, V @ np.asarray(tau, np.float64)
    return M


def _camera(v, device="cpu"):
    from pegasus_amd.cameras import Camera
    return Camera(colmap_id=0, R=v.R_c2w, T=v.t_w2c, FoVx=v.fovx, FoVy=v.fovy, image=None, gt_alpha_mask=None,
                  image_name="v", uid=0, data_device=device, image_width=v.width, image_height=v.height)


def test_se3_exp_identity_orthonormal_and_axis_angle():
    from pegasus_amd.camera_pose import se3_exp
    for dt in (torch.float32, torch.float64):
        assert torch.equal(se3_exp(torch.zeros(6, dtype=dt)), torch.eye(4, dtype=dt))
    rng = np.random.default_rng(0)
    for scale in (1e-5, 1e-3, 0.05, 0.09, 0.11, 0.5, 2.0, 3.0):
        for _ in range(4):
            w = rng.normal(size=3)
            w *= scale / np.linalg.norm(w)
            tau = rng.normal(size=3)
            ref = _axis_angle_matrix(w, tau)
            for dt, tol in ((torch.float64, 1e-12), (torch.float32, 2e-6)):
                M = se3_exp(torch.tensor(np.r_[w, tau], dtype=dt)).double().numpy()
                R = M[:3, :3]
                assert np.abs(R.T @ R - np.eye(3)).max() < tol * 4, (scale, dt)
                assert abs(np.linalg.det(R) - 1) < tol * 4
                assert np.abs(M - ref).max() < tol * max(1.0, np.abs(tau).max()) * 4, (scale, dt, np.abs(M - ref).max())
                assert np.array_equal(M[3], [0, 0, 0, 1])


def test_se3_exp_gradcheck():
    from pegasus_amd.camera_pose import se3_exp
    rng = np.random.default_rng(1)
    for scale in (0.0, 1e-4, 0.3, 1.7):
        w = rng.normal(size=3)
        w = w / np.linalg.norm(w) * scale
        x = torch.tensor(np.r_[w, rng.normal(size=3)], dtype=torch.float64, requires_grad=True)
        assert torch.autograd.gradcheck(se3_exp, (x,), eps=1e-7, atol=1e-6)


def test_posed_camera_at_zero_reproduces_camera():
    from pegasus_amd.camera_pose import PosedCamera
    P, v = tiny_scene(0)
    cam = _camera(v)
    pc = PosedCamera(cam, torch.zeros(6))
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        a, b = getattr(pc, name), getattr(cam, name)
        assert a.dtype == torch.float32 and a.shape == b.shape
        assert (a - b).abs().max() < 1e-6, name
    assert pc.image_width == cam.image_width and pc.FoVx == cam.FoVx
    r = pc.refined()
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert (getattr(r, name) - getattr(cam, name)).abs().max() < 1e-6, name


def test_posed_camera_gradcheck():
    from pegasus_amd.camera_pose import PosedCamera
    _, v = tiny_scene(0)
    cam = _camera(v)
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        f = lambda d: getattr(PosedCamera(cam, d), name)
        d = torch.tensor([0.01, -0.02, 0.03, 0.1, -0.05, 0.02], dtype=torch.float64, requires_grad=True)
        assert torch.autograd.gradcheck(f, (d,), eps=1e-7, atol=1e-6), name
        d0 = torch.zeros(6, dtype=torch.float64, requires_grad=True)
        assert torch.autograd.gradcheck(f, (d0,), eps=1e-7, atol=1e-6), name


# ---- the identities of the GPU tests, on the dense forward ---------------------------------------------------------------

def _loss(P, cam, delta, deg, gC, gD):
    from oracle.dense_ref import dense_forward
    from pegasus_amd.camera_pose import PosedCamera
    pc = PosedCamera(cam, torch.tensor(delta, dtype=torch.float64))
    kw = dict(width=cam.image_width, height=cam.image_height, tanfovx=math.tan(0.5 * cam.FoVx),
              tanfovy=math.tan(0.5 * cam.FoVy), viewmatrix=pc.world_view_transform.numpy(),
              projmatrix=pc.full_proj_transform.numpy(), campos=pc.camera_center.numpy(), bg=np.array([0.2, 0.4, 0.1]))
    c, d, dec = dense_forward(sh_degree=deg, **P, **kw, return_decisions=True)
    return float((c * gC).sum() + (d * gD).sum()), dec


def _quat_mul(a, b):
    r1, x1, y1, z1 = a
    r2, x2, y2, z2 = b.T
    return np.stack([r1 * r2 - x1 * x2 - y1 * y2 - z1 * z2, r1 * x2 + x1 * r2 + y1 * z2 - z1 * y2,
                     r1 * y2 - x1 * z2 + y1 * r2 + z1 * x2, r1 * z2 + x1 * y2 - y1 * x2 + z1 * r2], axis=1)


def _rot_quat(w):
    th = np.linalg.norm(w)
    return np.r_[math.cos(th / 2), math.sin(th / 2) * w / th] if th > 0 else np.array([1.0, 0, 0, 0])


@pytest.mark.parametrize("identity", ["a", "b"])
def test_camera_motion_equals_scene_motion_fd(identity):
    from oracle.dense_ref import same_decisions
    P, v = tiny_scene(0)
    P = {k: np.asarray(np.asarray(a, np.float32), np.float64) for k, a in P.items()}
    deg = 3 if identity == "a" else 0
    gC, gD = loss_weights(0, v.width, v.height)
    cam = _camera(v)
    w2c = np.asarray(cam.world_view_transform.double().numpy()).T
    Rw, c = w2c[:3, :3], -w2c[:3, :3].T @ w2c[:3, 3]
    kept = 0
    for k in range(3):
        e = np.zeros(3)
        e[k] = EPS
        if identity == "a":
            (lp, dp), (lm, dm) = _loss(P, cam, np.r_[0, 0, 0, e], deg, gC, gD), _loss(P, cam, np.r_[0, 0, 0, -e], deg, gC, gD)

            def moved(s):
                Q = dict(P)
                Q["means3d"] = P["means3d"] + s * (Rw.T @ e)
                return _loss(Q, cam, np.zeros(6), deg, gC, gD)
        else:
            (lp, dp), (lm, dm) = _loss(P, cam, np.r_[e, 0, 0, 0], deg, gC, gD), _loss(P, cam, np.r_[-e, 0, 0, 0], deg, gC, gD)

            def moved(s):
                ww = Rw.T @ (s * e)               # the world axis of Q = exp(R^T omega)
                Qm = _axis_angle_matrix(ww, np.zeros(3))[:3, :3]
                Q = dict(P)
                Q["means3d"] = c + (P["means3d"] - c) @ Qm.T
                Q["rotations"] = _quat_mul(_rot_quat(ww), P["rotations"])
                return _loss(Q, cam, np.zeros(6), deg, gC, gD)
        (sp, ep), (sm, em) = moved(1.0), moved(-1.0)
        if not (same_decisions(dp, dm) and same_decisions(ep, em)):
            continue
        kept += 1
        fd_cam, fd_scene = (lp - lm) / (2 * EPS), (sp - sm) / (2 * EPS)
        assert abs(fd_cam - fd_scene) <= 1e-4 * abs(fd_scene) + 1e-6, (identity, k, fd_cam, fd_scene)
        assert abs(fd_scene) > 1e-3, (identity, k, fd_scene)
    assert kept >= 2
