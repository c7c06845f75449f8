"""The training step's own kernels (pegasus_amd/csrc/train.hip.h) behind torch interfaces:

    ImageLoss / image_loss(x, y, lambda_dssim)   (1 - l) mean|x-y| + l (1 - mean SSIM), an autograd Function over
                                                 pgr_image_loss (value and dloss/dx in one call); l1_loss, ssim helpers
    MaskedImageLoss / masked_image_loss(x, alpha, y, mask, bg, lambda_dssim, lambda_alpha)
                                                 the same loss against y m + bg (1 - m), plus lambda_alpha mean|alpha - m|:
                                                 pgr_image_loss_masked, differentiable in x and alpha
    FusedAdam                                    a torch.optim.Optimizer whose step() is ONE pgr_adam_step launch for all
                                                 parameter groups, with torch.optim.Adam's state layout and arithmetic
    densify_stats(...)                           pgr_densify_stats: the densification statistics of one render

Everything is enqueued on torch's current stream; memory comes from torch's caching allocator.  There is no CPU path."""
from __future__ import annotations

import torch

from . import _lib

__all__ = ["ImageLoss", "image_loss", "image_loss_terms", "MaskedImageLoss", "masked_image_loss", "masked_image_loss_terms",
           "l1_loss", "ssim", "FusedAdam", "densify_stats"]


def _image(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] != 3:
        raise ValueError(f"{what}: expected a [3,H,W] tensor, got {getattr(t, 'shape', type(t))}")
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: the image loss runs on a HIP device (torch device 'cuda'); there is no CPU path")
    return t.detach().to(torch.float32).contiguous()


def image_loss_terms(x: torch.Tensor, y: torch.Tensor, lambda_dssim: float, want_grad: bool = True):
    """(out, grad): out = device tensor [loss, mean |x-y|, mean SSIM]; grad = dloss/dx [3,H,W] (None without want_grad)."""
    xc, yc = _image(x, "x"), _image(y, "y")
    if xc.shape != yc.shape or xc.device != yc.device:
        raise ValueError(f"image loss: x {tuple(xc.shape)} on {xc.device} vs y {tuple(yc.shape)} on {yc.device}")
    _, H, W = xc.shape
    out = torch.empty(3, dtype=torch.float32, device=xc.device)
    grad = torch.empty_like(xc) if want_grad else None
    ws = _lib.workspace("pgr_image_loss", xc.device, H, W)
    _lib.call("pgr_image_loss", xc.device, _lib.ptr(xc), _lib.ptr(yc), H, W, float(lambda_dssim), _lib.ptr(out), _lib.ptr(grad),
              _lib.ptr(ws), ws.numel())
    return out, grad


class ImageLoss(torch.autograd.Function):
    """loss = (1 - lambda_dssim) * mean|x - y| + lambda_dssim * (1 - mean SSIM(x, y)) over [3,H,W] images; differentiable
    in x (the render).  The loss is a scalar, so its gradient is final in the forward pass: backward only scales it."""

    @staticmethod
    def forward(ctx, x, y, lambda_dssim=0.2):
        out, grad = image_loss_terms(x, y, lambda_dssim, want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad if grad is not None else out)
        ctx.has_grad = grad is not None
        ctx.terms = out                                 # [loss, l1, ssim] for callers that log them
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_output):
        (g,) = ctx.saved_tensors
        if not ctx.has_grad:
            return None, None, None
        return g * grad_output, None, None


def image_loss(x, y, lambda_dssim: float = 0.2):
    return ImageLoss.apply(x, y, float(lambda_dssim))


def _plane(t: torch.Tensor, what: str, H: int, W: int, device) -> torch.Tensor:
    """A [H,W] / [1,H,W] map as the kernels read it: fp32, contiguous, [H,W]."""
    if not isinstance(t, torch.Tensor) or t.numel() != H * W or t.dim() not in (2, 3) or tuple(t.shape[-2:]) != (H, W):
        raise ValueError(f"{what}: expected a [H,W] or [1,H,W] tensor with H, W = {H}, {W}, got {getattr(t, 'shape', type(t))}")
    if t.device != device:
        raise ValueError(f"{what} is on {t.device}, the image on {device}")
    return t.detach().to(torch.float32).reshape(H, W).contiguous()


def masked_image_loss_terms(x, alpha, y, mask, bg, lambda_dssim: float, lambda_alpha: float, want_grad: bool = True,
                            want_grad_alpha: bool = True):
    """(out, grad, grad_alpha) of pgr_image_loss_masked: out = device tensor [loss, mean |x-y'|, mean SSIM(x,y'),
    mean |alpha-m|] with y' = y mask + bg (1 - mask); grad = dloss/dx [3,H,W], grad_alpha = dloss/dalpha [1,H,W] (None when
    not wanted).  ``alpha`` may be None when lambda_alpha = 0; ``mask`` None is the unmasked loss."""
    xc, yc = _image(x, "x"), _image(y, "y")
    if xc.shape != yc.shape or xc.device != yc.device:
        raise ValueError(f"image loss: x {tuple(xc.shape)} on {xc.device} vs y {tuple(yc.shape)} on {yc.device}")
    _, H, W = xc.shape
    dev = xc.device
    mc = None if mask is None else _plane(mask, "mask", H, W, dev)
    ac = None if alpha is None else _plane(alpha, "alpha", H, W, dev)
    bc = None
    if bg is not None:
        if not isinstance(bg, torch.Tensor) or bg.numel() != 3 or bg.device != dev:
            raise ValueError(f"bg: expected 3 values on {dev}, got {getattr(bg, 'shape', type(bg))}")
        bc = bg.detach().to(torch.float32).reshape(3).contiguous()
    out = torch.empty(4, dtype=torch.float32, device=dev)
    grad = torch.empty_like(xc) if want_grad else None
    grad_a = torch.empty((1, H, W), dtype=torch.float32, device=dev) if (want_grad_alpha and ac is not None) else None
    ws = _lib.workspace("pgr_image_loss_masked", dev, H, W)
    p = _lib.ptr
    _lib.call("pgr_image_loss_masked", dev, p(xc), p(yc), p(mc), p(bc), p(ac), H, W, float(lambda_dssim), float(lambda_alpha),
              p(out), p(grad), p(grad_a), p(ws), ws.numel())
    return out, grad, grad_a


class MaskedImageLoss(torch.autograd.Function):
    """loss = (1 - lambda_dssim) mean|x - y'| + lambda_dssim (1 - mean SSIM(x, y')) + lambda_alpha mean|alpha - mask|,
    y' = y mask + bg (1 - mask): the image loss of an object trained from a mask, against the step's own background.
    x [3,H,W] (the render), alpha [1,H,W] (the render's accumulated opacity; None if lambda_alpha = 0), y [3,H,W], mask
    [1,H,W] or [H,W] in 0..1, bg [3].  Differentiable in x and alpha; like ImageLoss the gradients are final in the forward
    pass.  ``ctx.terms`` holds [loss, l1, ssim, alpha_l1]."""

    @staticmethod
    def forward(ctx, x, alpha, y, mask, bg, lambda_dssim=0.2, lambda_alpha=0.5):
        out, grad, grad_a = masked_image_loss_terms(x, alpha, y, mask, bg, lambda_dssim, lambda_alpha,
                                                    want_grad=ctx.needs_input_grad[0],
                                                    want_grad_alpha=alpha is not None and ctx.needs_input_grad[1])
        ctx.save_for_backward(*(t for t in (grad, grad_a) if t is not None))
        ctx.has = (grad is not None, grad_a is not None)
        ctx.alpha_shape = None if alpha is None else tuple(alpha.shape)
        ctx.terms = out
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_output):
        saved = list(ctx.saved_tensors)
        gx = saved.pop(0) * grad_output if ctx.has[0] else None
        ga = (saved.pop(0) * grad_output).view(ctx.alpha_shape) if ctx.has[1] else None
        return gx, ga, None, None, None, None, None


def masked_image_loss(x, alpha, y, mask, bg, lambda_dssim: float = 0.2, lambda_alpha: float = 0.5):
    return MaskedImageLoss.apply(x, alpha, y, mask, bg, float(lambda_dssim), float(lambda_alpha))


def l1_loss(x, y):
    """mean |x - y| of [3,H,W] images (pgr_image_loss with lambda 0)."""
    return ImageLoss.apply(x, y, 0.0)


def ssim(x, y):
    """mean SSIM (11x11 Gaussian window) of [3,H,W] images, differentiable in x."""
    return 1.0 - ImageLoss.apply(x, y, 1.0)


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (no weight decay, no amsgrad) whose step() is one pgr_adam_step launch over every parameter of every
    group.  Same structure as torch's: param_groups carry "params", "lr", "betas", "eps" and any extra keys ("name");
    state[p] holds "step" (a CPU float32 tensor), "exp_avg" and "exp_avg_sq"; state_dict() / load_state_dict() are the
    base class's.  The arithmetic is that of torch's single-tensor Adam (foreach=False).

    The kernel writes through raw pointers, which autograd's version counters do not see: step() bumps the counter of every
    tensor it wrote, so that caches keyed on it (gaussian_renderer's kept activations) notice the update."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False):
        if weight_decay != 0.0 or amsgrad or maximize:
            raise ValueError("FusedAdam implements plain Adam: weight_decay = 0, amsgrad = False, maximize = False")
        if not 0.0 <= lr or not 0.0 <= eps or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"invalid Adam hyperparameters lr={lr} betas={betas} eps={eps}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0.0, amsgrad=False,
                                      maximize=False))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # one launch per (device, betas, eps) and per PGR_ADAM_MAX_GROUPS table entries -- one launch for a 3DGS model
        batches = {}
        written = []
        for group in self.param_groups:
            if group.get("weight_decay", 0.0) or group.get("amsgrad", False) or group.get("maximize", False):
                raise ValueError("FusedAdam implements plain Adam: weight_decay = 0, amsgrad = False, maximize = False")
            b1, b2 = (float(b) for b in group["betas"])
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdam does not support sparse gradients")
                if p.device.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdam: parameters must be contiguous float32 tensors on a HIP device")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                for t in (m, v):
                    if t.shape != p.shape or t.device != p.device or t.dtype != p.dtype or not t.is_contiguous():
                        raise RuntimeError("FusedAdam: optimizer state does not match its parameter (shape, device, dtype)")
                g = p.grad if p.grad.is_contiguous() and p.grad.dtype == torch.float32 else p.grad.float().contiguous()
                st["step"] += 1
                entry = _lib.PgrAdamGroup(param=p.data_ptr(), grad=g.data_ptr(), exp_avg=m.data_ptr(),
                                          exp_avg_sq=v.data_ptr(), n=p.numel(), lr=float(group["lr"]),
                                          step=int(st["step"].item()))
                batches.setdefault((p.device, b1, b2, float(group["eps"])), []).append((entry, g))
                written += [p, m, v]
        for (device, b1, b2, eps), entries in batches.items():
            for k in range(0, len(entries), _lib.PGR_ADAM_MAX_GROUPS):
                chunk = entries[k:k + _lib.PGR_ADAM_MAX_GROUPS]
                table = (_lib.PgrAdamGroup * len(chunk))(*(e for e, _ in chunk))
                _lib.call("pgr_adam_step", device, table, len(chunk), b1, b2, eps)
        if written:
            torch.autograd.graph.increment_version(written)
        return loss


def densify_stats(viewspace_grad: torch.Tensor, radii: torch.Tensor, grad_accum: torch.Tensor, denom: torch.Tensor,
                  max_radii2D: torch.Tensor) -> None:
    """For every Gaussian with radii > 0: grad_accum += ||viewspace_grad[:, :2]||, denom += 1,
    max_radii2D = max(max_radii2D, radii).  In place, one launch."""
    n = int(radii.shape[0])
    ok = (viewspace_grad.dim() == 2 and viewspace_grad.shape[0] == n and viewspace_grad.shape[1] >= 2
          and viewspace_grad.dtype == torch.float32 and viewspace_grad.is_contiguous() and radii.dtype == torch.int32
          and radii.is_contiguous())
    for t in (grad_accum, denom, max_radii2D):
        ok = ok and t.numel() == n and t.dtype == torch.float32 and t.is_contiguous() and t.device == radii.device
    if not ok or viewspace_grad.device != radii.device or radii.device.type != "cuda":
        raise ValueError("densify_stats: viewspace_grad [N,>=2] fp32, radii [N] int32, grad_accum / denom / max_radii2D "
                         "with N fp32 elements, all contiguous on one HIP device")
    _lib.call("pgr_densify_stats", radii.device, n, _lib.ptr(viewspace_grad), int(viewspace_grad.shape[1]), _lib.ptr(radii),
              _lib.ptr(grad_accum), _lib.ptr(denom), _lib.ptr(max_radii2D))
    torch.autograd.graph.increment_version([grad_accum, denom, max_radii2D])


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """The 3DGS position learning-rate schedule: log-linear from lr_init to lr_final over max_steps, optionally scaled by
    a sine ramp from lr_delay_mult to 1 over the first lr_delay_steps (with lr_delay_steps = 0, lr_delay_mult has no
    effect, as upstream)."""
    import numpy as np

    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        delay_rate = 1.0
        if lr_delay_steps > 0:
            delay_rate = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
        t = np.clip(step / max_steps, 0, 1)
        return float(delay_rate * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t))
    return helper
