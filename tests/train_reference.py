"""Plain restatements of the training-step kernels (pegasus_amd/csrc/train.hip.h) and of the 3-nearest-neighbour search
(knn.hip.h), for the tests; nothing here runs on a device.

    loss_f64 / masked_loss_f64   the loss in float64 through torch autograd (F.conv2d with the 11x11 window), evaluated on
                                 the float32 inputs the device holds: the oracle
    loss_torch_f32               the same 2-D convolution form in float32 (what the upstream training loop computes); only
                                 reported next to the measured bounds, never asserted
    loss_f32 / masked_loss_f32   a NumPy float32 transcription of the kernels' documented arithmetic: zero-padded halo,
                                 masked target fma(y, m, bg (1 - m)), separable 11 + 11 taps accumulated with
                                 fmaf(w, v, acc) from tap 0 to 10, s / A / B / C grouped as in the source, sums in double.
                                 It says how far correct float32 arithmetic of this formulation lies from float64; it is
                                 not a bit-for-bit model of the device (fmaf is emulated through float64, which rounds
                                 twice, and the compiler is free to contract a * b + c differently)
    adam_f32 / adam_f64          the five lines above adam_step_kernel, scalars formed as pgr_adam_step forms them
    densify_f64                  the densification statistics
    knn_f64                      mean of the three smallest squared distances to other points, in float64
"""
import math

import numpy as np

F32 = np.float32
SSIM_C1 = F32(0.01) * F32(0.01)                     # float products, as the constexpr in train.hip.h
SSIM_C2 = F32(0.03) * F32(0.03)


def window64():
    g = np.array([math.exp(-((k - 5) ** 2) / (2.0 * 1.5 * 1.5)) for k in range(11)], np.float64)
    return g / g.sum()


def window32():
    return window64().astype(F32)


# ---- float64 / float32 autograd (the 2-D convolution form) ------------------------------------------------------------------
def _autograd_loss(x, a, y, m, bg, lam, lam_a, dtype):
    """(loss, l1, ssim, alpha_l1, dloss/dx, dloss/dalpha or None); m None: the unmasked loss; a None: no alpha term."""
    import torch
    import torch.nn.functional as F
    xs = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    yt = y.detach().cpu().to(dtype)
    as_ = None if a is None else a.detach().cpu().to(dtype).clone().requires_grad_(True)
    if m is not None:
        md = m.detach().cpu().to(dtype).reshape(1, *m.shape[-2:])
        yt = yt * md + bg.detach().cpu().to(dtype).reshape(3, 1, 1) * (1.0 - md)
    k = torch.from_numpy(window64()).to(dtype)
    win = (k[:, None] * k[None, :]).expand(3, 1, 11, 11).contiguous()
    blur = lambda t: F.conv2d(t[None], win, padding=5, groups=3)[0]
    mx, my = blur(xs), blur(yt)
    sxx, syy, sxy = blur(xs * xs) - mx * mx, blur(yt * yt) - my * my, blur(xs * yt) - mx * my
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    ssim = smap.mean()
    l1 = (xs - yt).abs().mean()
    loss = (1 - lam) * l1 + lam * (1 - ssim)
    al1 = None
    if as_ is not None:
        al1 = (as_ - md).abs().mean()
        loss = loss + lam_a * al1
    loss.backward()
    return (float(loss.detach()), float(l1.detach()), float(ssim.detach()), 0.0 if al1 is None else float(al1.detach()),
            xs.grad, None if as_ is None else as_.grad)


def loss_f64(x, y, lam):
    """The 3DGS loss in float64 on the CPU: (loss, dloss/dx [3,H,W], mean |x-y|, mean SSIM)."""
    import torch
    loss, l1, ssim, _, gx, _ = _autograd_loss(x, None, y, None, None, lam, 0.0, torch.float64)
    return loss, gx, l1, ssim


def masked_loss_f64(x, a, y, m, bg, lam, lam_a):
    """The masked loss in float64: (loss, mean |x-y'|, mean SSIM, mean |a-m|, dloss/dx, dloss/da); a may be None."""
    import torch
    return _autograd_loss(x, a, y, m, bg, lam, lam_a, torch.float64)


def loss_torch_f32(x, a, y, m, bg, lam, lam_a):
    """masked_loss_f64's formulation in float32 (torch's 2-D convolution)."""
    import torch
    return _autograd_loss(x, a, y, m, bg, lam, lam_a, torch.float32)


# ---- the kernels' arithmetic in NumPy float32 -------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf emulated through float64: the product of two floats is exact in double, the sum rounds once there and once
    more to float."""
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
            + np.asarray(c, F32).astype(np.float64)).astype(F32)


def blur_f32(v):
    """[C,H,W] float32 through the window, zero padded: rows first (taps 0..10 into one accumulator), then columns."""
    w = window32()
    C, H, W = v.shape
    p = np.zeros((C, H + 10, W + 10), F32)
    p[:, 5:5 + H, 5:5 + W] = v
    acc = np.zeros((C, H + 10, W), F32)
    for k in range(11):
        acc = fma32(w[k], p[:, :, k:k + W], acc)
    out = np.zeros((C, H, W), F32)
    for k in range(11):
        out = fma32(w[k], acc[:, k:k + H, :], out)
    return out


def masked_target_f32(y, m, bg):
    """y' = fma(y, m, bg (1 - m)) per value; y [3,H,W], m [H,W], bg [3]."""
    y, m, bg = np.asarray(y, F32), np.asarray(m, F32), np.asarray(bg, F32)
    return fma32(y, m[None], bg[:, None, None] * (F32(1.0) - m[None]))


def masked_loss_f32(x, a, y, m, bg, lam, lam_a):
    """dict(out [4] float32 = loss, mean |x-y'|, mean SSIM, mean |a-m|; grad [3,H,W]; grad_alpha [H,W] or None; s the
    per-pixel SSIM map) by the kernels' arithmetic.  m None: the unmasked loss; a None: no alpha term."""
    x = np.ascontiguousarray(np.asarray(x, F32))
    y = np.ascontiguousarray(np.asarray(y, F32))
    _, H, W = x.shape
    if m is not None:
        m = np.asarray(m, F32).reshape(H, W)
        y = masked_target_f32(y, m, bg)
    two = F32(2.0)
    mu_x, mu_y = blur_f32(x), blur_f32(y)
    exx, eyy, exy = blur_f32(x * x), blur_f32(y * y), blur_f32(x * y)
    sxx, syy, sxy = exx - mu_x * mu_x, eyy - mu_y * mu_y, exy - mu_x * mu_y
    n1, d1 = (two * mu_x) * mu_y + SSIM_C1, (mu_x * mu_x + mu_y * mu_y) + SSIM_C1
    n2, d2 = two * sxy + SSIM_C2, (sxx + syy) + SSIM_C2
    d12 = d1 * d2
    s = (n1 * n2) / d12
    r1 = n1 / d1
    dmu = (two * n2) * (mu_y * d1 - mu_x * n1) / (d1 * d12)
    B = -s / d2
    Cc = (two * r1) / d2
    A = dmu + two * (mu_x * s - mu_y * r1) / d2
    for t in (s, A, B, Cc):
        assert t.dtype == F32
    n_values = 3.0 * H * W
    coef_s, coef_l1 = F32(-lam / n_values), F32((1.0 - lam) / n_values)
    bA, bB, bC = blur_f32(A), blur_f32(B), blur_f32(Cc)
    d = x - y
    g_ssim = (bA + (two * x) * bB) + y * bC
    grad = coef_s * g_ssim + coef_l1 * np.sign(d).astype(F32)
    assert grad.dtype == F32
    l1 = float(np.abs(d).astype(np.float64).sum()) * (1.0 / n_values)
    ss = float(s.astype(np.float64).sum()) * (1.0 / n_values)
    loss = (1.0 - lam) * l1 + lam * (1.0 - ss)
    am, grad_alpha = 0.0, None
    if a is not None:
        da = np.asarray(a, F32).reshape(H, W) - m
        am = float(np.abs(da).astype(np.float64).sum()) * (1.0 / (float(H) * float(W)))
        loss += lam_a * am
        grad_alpha = F32(lam_a / (float(H) * float(W))) * np.sign(da).astype(F32)
    return dict(out=np.array([loss, l1, ss, am], np.float64).astype(F32), grad=grad, grad_alpha=grad_alpha, s=s)


def loss_f32(x, y, lam):
    return masked_loss_f32(x, None, y, None, None, lam, 0.0)


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def adam_scalars(lr, beta1, beta2, eps, step):
    """The kernel's scalars as pgr_adam_step forms them: double arithmetic, one float rounding each."""
    bc1 = 1.0 - math.pow(beta1, float(step))
    bc2 = 1.0 - math.pow(beta2, float(step))
    return dict(neg_step_size=F32(-(lr / bc1)), inv_bc2_sqrt=F32(1.0 / math.pow(bc2, 0.5)), w1=F32(1.0 - beta1),
                beta2=F32(beta2), w2=F32(1.0 - beta2), eps=F32(eps))


def adam_f32(p, g, m, v, lr, beta1, beta2, eps, step):
    """One step of adam_step_kernel on float32 arrays: (p, m, v)."""
    p, g, m, v = (np.asarray(t, F32) for t in (p, g, m, v))
    k = adam_scalars(lr, beta1, beta2, eps, step)
    m = fma32(k["w1"], g - m, m)
    v = v * k["beta2"]
    v = fma32(k["w2"], g * g, v)
    denom = np.sqrt(v) * k["inv_bc2_sqrt"] + k["eps"]
    p = fma32(k["neg_step_size"], m / denom, p)
    assert p.dtype == m.dtype == v.dtype == F32
    return p, m, v


def adam_f64(p, g, m, v, lr, beta1, beta2, eps, step):
    """torch.optim.Adam's single-tensor step in float64 on the float32 inputs."""
    p, g, m, v = (np.asarray(t, F32).astype(np.float64) for t in (p, g, m, v))
    m = m + (1.0 - beta1) * (g - m)
    v = v * beta2 + (1.0 - beta2) * g * g
    denom = np.sqrt(v) / math.sqrt(1.0 - beta2 ** step) + eps
    p = p - (lr / (1.0 - beta1 ** step)) * (m / denom)
    return p, m, v


# ---- densification statistics ---------------------------------------------------------------------------------------------
def densify_f64(vgrad, radii, accum, denom, max_r):
    """(accum float64, denom float32, max_r float32) after one call, rows with radii <= 0 untouched."""
    vis = np.asarray(radii) > 0
    g = np.asarray(vgrad, F32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.asarray(accum, F32).astype(np.float64).reshape(-1).copy()
        norm = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
    acc[vis] = acc[vis] + norm[vis]
    den = np.asarray(denom, F32).reshape(-1).copy()
    den[vis] = den[vis] + F32(1.0)
    mr = np.asarray(max_r, F32).reshape(-1).copy()
    mr[vis] = np.maximum(mr[vis], np.asarray(radii)[vis].astype(F32))
    return acc, den, mr


# ---- kNN --------------------------------------------------------------------------------------------------------------------
def knn_f64(pts, queries=None, brute=False):
    """Mean of the three smallest squared distances from each point (or each of the points ``queries`` indexes) to the
    OTHER points, in float64 on the float32 coordinates.  n >= 4.  ``brute``: all pairs on the host (for coincident points,
    where the order in which a tree returns equal distances says nothing about which of them is the point itself)."""
    P = np.asarray(pts, F32).astype(np.float64)
    q = np.arange(len(P)) if queries is None else np.asarray(queries)
    assert len(P) >= 4
    if brute:
        out = np.empty(len(q))
        for k, i in enumerate(q):
            d2 = ((P - P[i]) ** 2).sum(axis=1)
            d2[i] = np.inf
            out[k] = np.sort(np.partition(d2, 2)[:3]).mean()
        return out
    from scipy.spatial import cKDTree
    tree = cKDTree(P, balanced_tree=False, compact_nodes=False)
    d, idx = tree.query(P[q], k=4)
    assert (d[:, 0] == 0.0).all()
    return (d[:, 1:] ** 2).mean(axis=1)


def ulps(a, b):
    """Distance in units in the last place between two float32 arrays of equal shape (as ordered integers)."""
    ia = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, F32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)
