"""The training step's own kernels (pegasus_amd/csrc/train.hip.h) behind torch interfaces:

    ImageLoss / image_loss(x, y, lambda_dssim)   (1 - l) mean|x-y| + l (1 - mean SSIM), an autograd Function over
                                                 pgr_image_loss (value and dloss/dx in one call); l1_loss, ssim helpers
    FusedAdam                                    a torch.optim.Optimizer whose step() is ONE pgr_adam_step launch for all
                                                 parameter groups, with torch.optim.Adam's state layout and arithmetic
    densify_stats(...)                           pgr_densify_stats: the densification statistics of one render

Everything is enqueued on torch's current stream; memory comes from torch's caching allocator.  There is no CPU path."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

__all__ = ["ImageLoss", "image_loss", "image_loss_terms", "l1_loss", "ssim", "FusedAdam", "densify_stats"]


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


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
    L = _lib.lib()
    _, H, W = xc.shape
    out = torch.empty(3, dtype=torch.float32, device=xc.device)
    grad = torch.empty_like(xc) if want_grad else None
    ws = torch.empty(L.pgr_image_loss_workspace_bytes(H, W), dtype=torch.uint8, device=xc.device)
    with torch.cuda.device(xc.device):
        _lib.check(L.pgr_image_loss(C.c_void_p(xc.data_ptr()), C.c_void_p(yc.data_ptr()), H, W, float(lambda_dssim),
                                    C.c_void_p(out.data_ptr()), None if grad is None else C.c_void_p(grad.data_ptr()),
                                    C.c_void_p(ws.data_ptr()), ws.numel(), _stream(xc.device)), "pgr_image_loss")
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
        L = _lib.lib()
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
                with torch.cuda.device(device):
                    _lib.check(L.pgr_adam_step(table, len(chunk), b1, b2, eps, _stream(device)), "pgr_adam_step")
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
    L = _lib.lib()
    with torch.cuda.device(radii.device):
        _lib.check(L.pgr_densify_stats(n, C.c_void_p(viewspace_grad.data_ptr()), int(viewspace_grad.shape[1]),
                                       C.c_void_p(radii.data_ptr()), C.c_void_p(grad_accum.data_ptr()),
                                       C.c_void_p(denom.data_ptr()), C.c_void_p(max_radii2D.data_ptr()),
                                       _stream(radii.device)), "pgr_densify_stats")
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
