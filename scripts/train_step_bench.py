"""Median ms per 3DGS training iteration at 800x800 on the C2 object (150 k Gaussians) and the C3 scene (2 M), split into
forward / loss / backward / stats / optimizer with HIP events, plus two same-box A/B pairs:
    loss:      pgr_image_loss (value + gradient, one call)  vs  the torch conv2d form of the same loss + its backward
    optimizer: FusedAdam (one pgr_adam_step launch)         vs  torch.optim.Adam(foreach=True)
Inputs are random (targets, gradients); every stage is warmed up first; each number is the median of 5 repeats.
--batch B ... adds multi-view steps (render_batch: B views per optimiser step, one pgr_forward and one
pgr_backward) with the same stage split, per step and per view; "backward" is the HIP-event time of loss.backward(),
i.e. of the backward kernels.  B = 1 is the single-view loop above (the default, whose output is unchanged).
--masks adds, beside every plain step, the same step trained from object masks (a seeded synthetic soft mask per camera):
render with return_alpha, MaskedImageLoss (pgr_image_loss_masked) against the step's background, backward with dL/dalpha
(PgrBackwardCall.grad_alpha); reported as "masked" next to the plain numbers.

    python scripts/train_step_bench.py [--iters 20] [--warmup 5] [--repeats 5] [--scenes c2 c3] [--batch 1 2 4 8]
                                       [--masks] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

STAGES = ("forward", "loss", "backward", "stats", "optimizer")


def torch_loss(x, y, lam=0.2):
    g = torch.tensor([math.exp(-((k - 5) ** 2) / (2 * 1.5 ** 2)) for k in range(11)], device=x.device)
    g = g / g.sum()
    w = (g[:, None] @ g[None, :]).expand(3, 1, 11, 11).contiguous()
    blur = lambda t: F.conv2d(t[None], w, padding=5, groups=3)[0]
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    s = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return (1 - lam) * (x - y).abs().mean() + lam * (1 - s.mean())


def model_and_cameras(name, dev):
    from pegasus_amd import scenes
    from pegasus_amd.cameras import Camera
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.train import OPTIMIZATION_DEFAULTS, _Options
    cloud, views = scenes.scene_c2() if name == "c2" else scenes.scene_c3(n_views=16)
    m = GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling,
                                  cloud.rotation, sh_degree=3, device=dev)
    m.spatial_lr_scale = 1.0
    m.training_setup(_Options(None, OPTIMIZATION_DEFAULTS))
    gen = torch.Generator().manual_seed(0)
    cams = [Camera(colmap_id=i, R=v.R_c2w, T=v.t_w2c, FoVx=v.fovx, FoVy=v.fovy,
                   image=torch.rand((3, v.height, v.width), generator=gen), gt_alpha_mask=None, image_name=str(i), uid=i,
                   data_device=str(dev)) for i, v in enumerate(views[:8])]
    return m, cams


def add_masks(cams, dev):
    """A seeded soft elliptical mask per camera (the object in the middle of the frame, a 12-pixel soft edge)."""
    gen = torch.Generator().manual_seed(3)
    for cam in cams:
        H, W = cam.image_height, cam.image_width
        c = torch.rand(4, generator=gen)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        cx, cy, rx, ry = W * (0.4 + 0.2 * c[0]), H * (0.4 + 0.2 * c[1]), W * (0.2 + 0.15 * c[2]), H * (0.2 + 0.15 * c[3])
        r = torch.sqrt(((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2)
        cam.gt_mask = torch.clamp((1.0 - r) * min(rx, ry) / 12.0 + 0.5, 0.0, 1.0)[None].to(dev)


def train_steps(m, cams, iters, dev, masked=False):
    """Per-stage event times (ms) of ``iters`` iterations, summed per stage."""
    from pegasus_amd.gaussian_renderer import render
    from pegasus_amd.train_ops import ImageLoss, MaskedImageLoss
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device=dev)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)] for _ in range(iters)]
    for i in range(iters):
        cam = cams[i % len(cams)]
        e = ev[i]
        e[0].record()
        pkg = render(cam, m, pipe, bg, return_alpha=masked)
        e[1].record()
        if masked:
            loss = MaskedImageLoss.apply(pkg["render"], pkg["alpha"], cam.original_image, cam.gt_mask, bg, 0.2, 0.5)
        else:
            loss = ImageLoss.apply(pkg["render"], cam.original_image, 0.2)
        e[2].record()
        loss.backward()
        e[3].record()
        with torch.no_grad():
            m.add_render_stats(pkg["viewspace_points"], pkg["radii"])
            e[4].record()
            m.optimizer.step()
            m.optimizer.zero_grad(set_to_none=True)
        e[5].record()
    torch.cuda.synchronize()
    per = {s: sum(e[k].elapsed_time(e[k + 1]) for e in ev) / iters for k, s in enumerate(STAGES)}
    per["total"] = sum(e[0].elapsed_time(e[-1]) for e in ev) / iters
    return per


def train_steps_batch(m, cams, B, iters, dev, masked=False):
    """train_steps with B views per optimiser step (render_batch; loss = the mean of the B per-view losses)."""
    from pegasus_amd.gaussian_renderer import render_batch
    from pegasus_amd.train_ops import ImageLoss, MaskedImageLoss
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device=dev)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)] for _ in range(iters)]
    for i in range(iters):
        batch = [cams[(i * B + k) % len(cams)] for k in range(B)]
        e = ev[i]
        e[0].record()
        pkg = render_batch(batch, m, pipe, bg, return_alpha=masked)
        e[1].record()
        if masked:
            loss = sum(MaskedImageLoss.apply(pkg["render"][k], pkg["alpha"][k], c.original_image, c.gt_mask, bg, 0.2, 0.5)
                       for k, c in enumerate(batch)) / B
        else:
            loss = sum(ImageLoss.apply(pkg["render"][k], c.original_image, 0.2) for k, c in enumerate(batch)) / B
        e[2].record()
        loss.backward()
        e[3].record()
        with torch.no_grad():
            m.add_batch_render_stats(pkg["viewspace_points"], pkg["radii"], grad_scale=B)
            e[4].record()
            m.optimizer.step()
            m.optimizer.zero_grad(set_to_none=True)
        e[5].record()
    torch.cuda.synchronize()
    per = {s: sum(e[k].elapsed_time(e[k + 1]) for e in ev) / iters for k, s in enumerate(STAGES)}
    per["total"] = sum(e[0].elapsed_time(e[-1]) for e in ev) / iters
    return per


def time_loop(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def loss_ab(dev, iters, warmup, repeats):
    from pegasus_amd.train_ops import ImageLoss
    gen = torch.Generator().manual_seed(1)
    x0 = torch.rand((3, 800, 800), generator=gen).to(dev)
    y = torch.rand((3, 800, 800), generator=gen).to(dev)

    def ours():
        x = x0.clone().requires_grad_(True)
        ImageLoss.apply(x, y, 0.2).backward()

    def theirs():
        x = x0.clone().requires_grad_(True)
        torch_loss(x, y).backward()
    out = {}
    for name, fn in (("pgr_image_loss", ours), ("torch_conv2d", theirs)):
        time_loop(fn, warmup)
    res = {"pgr_image_loss": [], "torch_conv2d": []}
    for _ in range(repeats):                                 # alternate the two in every repeat
        for name, fn in (("pgr_image_loss", ours), ("torch_conv2d", theirs)):
            res[name].append(time_loop(fn, iters))
    for k, v in res.items():
        out[k] = statistics.median(v)
    return out


def adam_ab(m, dev, iters, warmup, repeats):
    from pegasus_amd.train_ops import FusedAdam
    gen = torch.Generator().manual_seed(2)
    shapes = [t.shape for _, t in ((n, getattr(m, a)) for n, a in m._PARAM_NAMES)]
    lrs = [g["lr"] for g in m.optimizer.param_groups]

    def make(cls, **kw):
        ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen).to(dev)
        return cls([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)], lr=0.0, eps=1e-15, **kw)
    fused, ref = make(FusedAdam), make(torch.optim.Adam, foreach=True)
    for o in (fused, ref):
        time_loop(o.step, warmup)
    res = {"FusedAdam": [], "torch_Adam_foreach": []}
    for _ in range(repeats):
        for name, o in (("FusedAdam", fused), ("torch_Adam_foreach", ref)):
            res[name].append(time_loop(o.step, iters))
    out = {k: statistics.median(v) for k, v in res.items()}
    out["floats"] = sum(math.prod(s) for s in shapes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", nargs="+", default=["c2", "c3"])
    ap.add_argument("--batch", nargs="+", type=int, default=[1], help="views per optimiser step (1: the single-view loop)")
    ap.add_argument("--masks", action="store_true", help="also time the masked step (alpha + MaskedImageLoss)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_bench.py needs a HIP device (no CPU timing)")
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "size": "800x800"}
    report["loss_ab_ms"] = loss_ab(dev, a.iters, a.warmup, a.repeats)
    print("loss A/B (value + gradient, 800x800):", json.dumps(report["loss_ab_ms"]), flush=True)
    for name in a.scenes:
        m, cams = model_and_cameras(name, dev)
        if a.masks:
            add_masks(cams, dev)
        train_steps(m, cams, a.warmup, dev)
        reps = [train_steps(m, cams, a.iters, dev) for _ in range(a.repeats)]
        med = {k: statistics.median(r[k] for r in reps) for k in reps[0]}
        report[name] = {"gaussians": int(m.get_xyz.shape[0]), "ms_per_iter": med,
                        "adam_ab_ms": adam_ab(m, dev, a.iters, a.warmup, a.repeats)}
        if a.masks:
            train_steps(m, cams, a.warmup, dev, masked=True)
            reps = [train_steps(m, cams, a.iters, dev, masked=True) for _ in range(a.repeats)]
            report[name]["masked"] = {"ms_per_iter": {k: statistics.median(r[k] for r in reps) for k in reps[0]}}
        print(name, json.dumps(report[name]), flush=True)
        for B in (b for b in a.batch if b > 1):
            train_steps_batch(m, cams, B, a.warmup, dev)
            reps = [train_steps_batch(m, cams, B, a.iters, dev) for _ in range(a.repeats)]
            step = {k: statistics.median(r[k] for r in reps) for k in reps[0]}
            report[name].setdefault("batch", {})[str(B)] = {"ms_per_step": step,
                                                              "ms_per_view": {k: v / B for k, v in step.items()}}
            if a.masks:
                train_steps_batch(m, cams, B, a.warmup, dev, masked=True)
                reps = [train_steps_batch(m, cams, B, a.iters, dev, masked=True) for _ in range(a.repeats)]
                step = {k: statistics.median(r[k] for r in reps) for k in reps[0]}
                report[name]["batch"][str(B)]["masked"] = {"ms_per_step": step}
            print(f"{name} B={B}", json.dumps(report[name]["batch"][str(B)]), flush=True)
            torch.cuda.empty_cache()
        del m, cams
        torch.cuda.empty_cache()
    line = json.dumps(report)
    print(line)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
