#!/usr/bin/env python3
"""Cost of the camera gradient (camera_backward_kernel + camera_grad_finish_kernel): HIP-event time of loss.backward()
through the rasterizer with and without camera tensors that require grad, interleaved, on C2 (150 k Gaussians) and C3
(2 M), one view and a batch of 4 (800 x 800); the difference is the camera kernels.  Then the per-step time of refine_pose
on C2 (one 800 x 800 view, with a mask).
    python scripts/camera_grad_bench.py [--reps N] [--scenes c2,c3]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pegasus_amd import diff_gaussian_rasterization as dgr, scenes  # noqa: E402


def graphs(act, views, dev, cam_grad):
    t = lambda a, rg=False: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev, requires_grad=rg)
    X = dict(means3D=t(act["means3d"], True), opacities=t(act["opacities"].reshape(-1, 1), True), shs=t(act["shs"], True),
             scales=t(act["scales"], True), rotations=t(act["rotations"], True))
    sets = [dgr.GaussianRasterizationSettings(v.height, v.width, v.tanfovx, v.tanfovy, torch.zeros(3, device=dev), 1.0,
                                              t(v.world_view_transform, cam_grad), t(v.full_proj_transform, cam_grad), 3,
                                              t(v.camera_center, cam_grad), False, False) for v in views]
    rng = np.random.default_rng(0)
    wC = t(rng.uniform(-1, 1, (len(views), 3, views[0].height, views[0].width)))
    if len(views) == 1:
        color, _, _ = dgr.GaussianRasterizer(sets[0])(means2D=None, **X)
        loss = (color * wC[0]).sum()
    else:
        color, _, _ = dgr.rasterize_gaussians_batch(X["means3D"], None, X["opacities"], sets, shs=X["shs"],
                                                    scales=X["scales"], rotations=X["rotations"])
        loss = (color * wC).sum()
    return loss


def time_backward(loss, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss.backward(retain_graph=True)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scenes", default="c2,c3")
    ap.add_argument("--refine_steps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for name in args.scenes.split(","):
        cloud, views = scenes.scene_c2(n_views=4) if name == "c2" else scenes.scene_c3(n_views=4)
        act = cloud.activated()
        for B in (1, 4):
            plain, cam = graphs(act, views[:B], dev, False), graphs(act, views[:B], dev, True)
            time_backward(plain, 3), time_backward(cam, 3)
            tp, tc = [], []
            for _ in range(args.reps):          # interleaved
                tp += time_backward(plain, 1)
                tc += time_backward(cam, 1)
            mp, mc = float(np.median(tp)), float(np.median(tc))
            res[f"{name}_B{B}"] = dict(backward_ms=round(mp, 4), backward_with_camera_ms=round(mc, 4),
                                       camera_kernels_ms=round(mc - mp, 4))
            print(name, "B", B, res[f"{name}_B{B}"], flush=True)
            del plain, cam
            torch.cuda.empty_cache()
    # refine_pose per step on C2
    from types import SimpleNamespace
    from pegasus_amd.camera_pose import PosedCamera, refine_pose
    from pegasus_amd.cameras import Camera
    from pegasus_amd.gaussian_model import GaussianModel
    from pegasus_amd.gaussian_renderer import render
    cloud, views = scenes.scene_c2(n_views=4)
    model = GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling,
                                      cloud.rotation, sh_degree=3, device="cuda")
    v = views[0]
    cam = Camera(colmap_id=0, R=v.R_c2w, T=v.t_w2c, FoVx=v.fovx, FoVy=v.fovy, image=None, gt_alpha_mask=None,
                 image_name="0", uid=0, data_device="cuda", image_width=v.width, image_height=v.height)
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    with torch.no_grad():
        tgt = render(cam, model, pipe, torch.zeros(3, device=dev), return_alpha=True)
    start = PosedCamera(cam, torch.tensor([0.01, -0.02, 0.01, 0.05, 0.0, -0.03], device=dev)).refined()
    refine_pose(model, start, tgt["render"], tgt["alpha"], iterations=5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    refine_pose(model, start, tgt["render"], tgt["alpha"], iterations=args.refine_steps)
    torch.cuda.synchronize()
    res["c2_refine_pose_ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / args.refine_steps, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
