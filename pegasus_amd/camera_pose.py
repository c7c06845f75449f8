"""Differentiable camera poses: the one place that knows how a camera pose is parameterised for refinement.

A pose correction is a 6-vector ``delta = (omega, tau)`` (rotation vector, translation) in the CAMERA frame, applied on the
left of the camera's world-to-camera transform:  W2C' = se3_exp(delta) @ W2C.  ``PosedCamera`` exposes what
``gaussian_renderer.render`` / ``render_batch`` read from a camera, built from W2C' with torch operations, so the camera
gradient the rasterizer returns (PgrBackwardCall.camera_grads: viewmatrix, projmatrix, campos) reaches ``delta`` through autograd.

``refine_pose`` is render-and-compare pose refinement of a frozen model: rendering an object model alone from a camera whose
world frame is the model frame makes W2C' the BOP pose (cam_R_m2c, cam_t_m2c; ``pegasus_amd.bop_pose``)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from . import graphics as G
from .cameras import Camera

__all__ = ["se3_exp", "PosedCamera", "refine_pose", "rotation_error_deg"]

# below this theta^2 the Rodrigues coefficients are their Taylor series (the closed forms cancel catastrophically)
_SERIES_BELOW = {torch.float64: 1e-6, torch.float32: 1e-2, torch.float16: 1e-1, torch.bfloat16: 1e-1}


def _hat(w: torch.Tensor) -> torch.Tensor:
    z = torch.zeros_like(w[0])
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def se3_exp(xi: torch.Tensor) -> torch.Tensor:
    """4x4 rigid transform of the twist ``xi = (omega, tau)`` [6]: R = I + A K + B K^2, t = (I + B K + C K^2) tau with
    K = hat(omega), theta = |omega|, A = sin(theta)/theta, B = (1 - cos(theta))/theta^2, C = (theta - sin(theta))/theta^3
    (Rodrigues).  Near theta = 0 the coefficients are their series, so the map and its derivative are finite and smooth
    there.  Differentiable, any float dtype and device."""
    xi = xi.reshape(6)
    w, tau = xi[:3], xi[3:]
    th2 = (w * w).sum()
    small = th2 < _SERIES_BELOW.get(xi.dtype, 1e-2)
    th2s = torch.where(small, torch.ones_like(th2), th2)        # the closed forms only ever see a safe theta
    th = torch.sqrt(th2s)
    A = torch.where(small, 1 - th2 / 6 + th2 * th2 / 120, torch.sin(th) / th)
    B = torch.where(small, 0.5 - th2 / 24 + th2 * th2 / 720, (1 - torch.cos(th)) / th2s)
    Cc = torch.where(small, 1.0 / 6 - th2 / 120 + th2 * th2 / 5040, (th - torch.sin(th)) / (th2s * th))
    K = _hat(w)
    K2 = K @ K
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device)
    R = eye + A * K + B * K2
    V = eye + B * K + Cc * K2
    top = torch.cat([R, (V @ tau).reshape(3, 1)], dim=1)
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=xi.dtype, device=xi.device)
    return torch.cat([top, bottom], dim=0)


def _base_w2c(camera) -> np.ndarray:
    return G.getWorld2View2(camera.R, camera.T, getattr(camera, "trans", np.zeros(3)),
                            getattr(camera, "scale", 1.0)).astype(np.float64)


class PosedCamera:
    """``camera`` seen through the pose correction ``delta`` [6] (a leaf that requires grad while it is being refined).
    ``pivot`` (a camera-frame point [3], optional): the correction acts about it, W2C' = T(pivot) se3_exp(delta)
    T(-pivot) W2C -- refining an object's pose about the object's own centre keeps rotation and translation apart (about
    the camera centre, a small rotation and a sideways translation move a distant object's image nearly alike).

    ``world_view_transform``, ``full_proj_transform`` and ``camera_center`` are rebuilt from W2C' = se3_exp(delta) @ W2C at
    every access (transposed storage, as ``Camera``; camera_center = -R'^T t').  They are float64 when ``delta`` is, else
    float32.  Every other attribute (image size, FoV, the ground-truth image and mask, names) is the base camera's."""

    def __init__(self, camera, delta: torch.Tensor, pivot=None):
        self.base = camera
        self.delta = delta
        dev = delta.device
        self._w2c = torch.tensor(_base_w2c(camera), dtype=torch.float64, device=dev)
        self._pivot = None
        if pivot is not None:
            self._pivot = torch.eye(4, dtype=torch.float64, device=dev)
            self._pivot[:3, 3] = torch.as_tensor(np.asarray(pivot, np.float64).reshape(3), device=dev)
        proj = G.getProjectionMatrix(camera.znear, camera.zfar, camera.FoVx, camera.FoVy).T
        self._proj = torch.tensor(np.asarray(proj, np.float64), dtype=torch.float64, device=dev)

    def __getattr__(self, name):          # (only reached for what this class does not define)
        if name == "base":
            raise AttributeError(name)
        return getattr(self.base, name)

    @property
    def _out_dtype(self):
        return torch.float64 if self.delta.dtype == torch.float64 else torch.float32

    def w2c(self) -> torch.Tensor:
        """W2C' [4,4], float64 (differentiable in ``delta``)."""
        e = se3_exp(self.delta.to(torch.float64))
        if self._pivot is not None:
            e = self._pivot @ e @ torch.linalg.inv(self._pivot)
        return e @ self._w2c

    @property
    def world_view_transform(self) -> torch.Tensor:
        return self.w2c().T.contiguous().to(self._out_dtype)

    @property
    def projection_matrix(self) -> torch.Tensor:
        return self._proj.to(self._out_dtype)

    @property
    def full_proj_transform(self) -> torch.Tensor:
        return (self.w2c().T @ self._proj).to(self._out_dtype)

    @property
    def camera_center(self) -> torch.Tensor:
        m = self.w2c()
        return (-(m[:3, :3].T @ m[:3, 3])).to(self._out_dtype)

    def pose(self):
        """(R_w2c [3,3], t_w2c [3]) of W2C' as float64 numpy arrays (for an object-only model: cam_R_m2c, cam_t_m2c)."""
        m = self.w2c().detach().cpu().numpy()
        return m[:3, :3].copy(), m[:3, 3].copy()

    def refined(self) -> Camera:
        """The plain ``Camera`` W2C' describes (R = R'^T camera-to-world, T = t'; no extra translate / scale), with the base
        camera's image size, FoV, names, ground-truth image and mask."""
        R, t = self.pose()
        b = self.base
        cam = Camera(colmap_id=b.colmap_id, R=R.T.copy(), T=t, FoVx=b.FoVx, FoVy=b.FoVy, image=None, gt_alpha_mask=None,
                     image_name=b.image_name, uid=b.uid, data_device=str(b.data_device),
                     image_width=b.image_width, image_height=b.image_height)
        cam.original_image = b.original_image
        cam.gt_mask = getattr(b, "gt_mask", None)
        return cam


def rotation_error_deg(R_a, R_b) -> float:
    """Angle of R_a^T R_b in degrees."""
    M = np.asarray(R_a, np.float64).T @ np.asarray(R_b, np.float64)
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(M) - 1.0) / 2.0))))


def refine_pose(model, camera, target_image, target_mask=None, *, iterations=300, lr_rotation=5e-3, lr_translation=None,
                lambda_dssim=0.2, lambda_alpha=0.5, bg=None, lr_final_ratio=0.01):
    """Render-and-compare refinement of ``camera``'s pose against ``target_image`` [3,H,W] (and ``target_mask`` [1,H,W] or
    [H,W] in 0..1: the alpha of the render is then supervised too, and the image compared inside the mask) with the model
    FROZEN.  Each step renders through ``PosedCamera`` and takes the trainer's loss (MaskedImageLoss with a mask, else
    ImageLoss), then one Adam step on the 6-vector: rotation lr ``lr_rotation`` (radians), translation lr ``lr_translation``
    (default: lr_rotation x the distance from the camera centre to the model's centroid), both decayed exponentially to
    ``lr_final_ratio`` of that by the last step.

    The correction acts about the model's centroid (``PosedCamera``'s pivot).

    Returns (refined Camera, (R_m2c [3,3], t_m2c [3]) of the refined world-to-camera transform, loss history [iterations])."""
    from .gaussian_renderer import render
    from .train_ops import image_loss, masked_image_loss
    dev = target_image.device
    bg_t = torch.zeros(3, device=dev) if bg is None else torch.as_tensor(bg, dtype=torch.float32, device=dev)
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    centre = model.get_xyz.detach().mean(0).double().cpu().numpy()
    w2c = _base_w2c(camera)
    pivot = w2c[:3, :3] @ centre + w2c[:3, 3]                 # the centroid in the camera frame
    if lr_translation is None:
        lr_translation = lr_rotation * float(np.linalg.norm(pivot))
    # Adam steps are lr-sized per coordinate: the optimised vector u holds the translation in units of
    # lr_translation / lr_rotation, so one learning rate gives each part its own step size (delta = u * scale)
    k = lr_translation / lr_rotation
    scale = torch.tensor([1.0, 1.0, 1.0, k, k, k], device=dev)
    u = torch.zeros(6, dtype=torch.float32, device=dev, requires_grad=True)
    opt = torch.optim.Adam([u], lr=lr_rotation)
    target = target_image.to(dev, torch.float32)
    mask = None if target_mask is None else target_mask.to(dev, torch.float32)
    frozen = [(p, p.requires_grad) for p in _model_params(model)]
    history = []
    try:
        for p, _ in frozen:
            p.requires_grad_(False)
        for it in range(int(iterations)):
            for g in opt.param_groups:
                g["lr"] = lr_rotation * lr_final_ratio ** (it / max(1, int(iterations) - 1))
            opt.zero_grad(set_to_none=True)
            cam = PosedCamera(camera, u * scale, pivot)
            pkg = render(cam, model, pipe, bg_t, return_alpha=mask is not None)
            if mask is not None:
                loss = masked_image_loss(pkg["render"], pkg["alpha"], target, mask, bg_t, lambda_dssim, lambda_alpha)
            else:
                loss = image_loss(pkg["render"], target, lambda_dssim)
            loss.backward()
            opt.step()
            history.append(loss.detach())
    finally:
        for p, rg in frozen:
            p.requires_grad_(rg)
    final = PosedCamera(camera, (u * scale).detach(), pivot)
    return final.refined(), final.pose(), [float(h) for h in torch.stack(history).cpu()] if history else []


def _model_params(model):
    names = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
    return [t for t in (getattr(model, n, None) for n in names) if isinstance(t, torch.Tensor) and t.is_leaf]
