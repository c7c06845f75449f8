"""``training(dataset, opt, pipe, testing_iterations, saving_iterations, checkpoint_iterations, checkpoint, debug_from)``:
the 3DGS optimisation loop that PEGASUS's reconstruction scripts reach through train_gaussian_splatting_wrapper
(/root/reference/src/gs/gs_training.py:7,46), on this package's kernels:

    render (pgr_forward)  ->  ImageLoss (pgr_image_loss)  ->  backward (pgr_backward)  ->  densification statistics
    (pgr_densify_stats)  ->  densify / prune / opacity reset on their schedule (torch)  ->  FusedAdam (pgr_adam_step)

It reads a COLMAP dataset (pegasus_amd.colmap_io) and writes the model layout ``Scene(args, gaussians,
load_iteration=-1)`` opens: cfg_args, cameras.json, input.ply, point_cloud/iteration_N/point_cloud.ply, chkpntN.pth.

    python -m pegasus_amd.train -s <colmap dir> -m <output dir> [--iterations N] [--eval] [--batch_size B]
                                [--masks <mask dir> | --masks alpha] [--lambda_alpha L] ...

With --masks (an object trained from per-image masks, as PEGASUS's reconstruction scripts do) every step renders the
accumulated opacity too and takes MaskedImageLoss (pgr_image_loss_masked): the target is the image inside the mask over
the step's own background, plus lambda_alpha mean|alpha - mask|, whose gradient reaches the backward as dL/dalpha.

With --batch_size B > 1 a step renders B views in one render_batch (pgr_forward / pgr_backward) and the Adam
step, which touches every parameter whatever the number of views, is paid once per B views.

With --pose_lr > 0 the training cameras' poses are refined with the Gaussians (scans whose registration is slightly off):
every training camera gets a pose correction (pegasus_amd.camera_pose.PosedCamera), a 6-vector that the camera gradient
of the rasterizer (PgrBackwardCall.camera_grads) reaches through torch, updated by its own Adam (rotation lr pose_lr, translation lr
pose_lr x cameras_extent) with the Gaussian optimiser's step.  The train report renders the refined cameras, test cameras
keep their poses, every save writes cameras_refined.json and every checkpoint the corrections to chkpntN_poses.pth.
"""
from __future__ import annotations

import json
import math
import os
import random
import shutil
import sys
from argparse import ArgumentParser, Namespace

import torch

from . import colmap_io
from .gaussian_model import GaussianModel
from .scene import camera_to_JSON, searchForMaxIteration

# the 3DGS optimisation parameters and their defaults (compat/arguments OptimizationParams carries the same fields);
# training() reads every one with getattr(opt, name, default), so an options object that lacks a field still works
OPTIMIZATION_DEFAULTS = dict(
    iterations=30_000, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
    position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001,
    percent_dense=0.01, lambda_dssim=0.2, densification_interval=100, opacity_reset_interval=3000,
    densify_from_iter=500, densify_until_iter=15_000, densify_grad_threshold=0.0002, random_background=False)
MODEL_DEFAULTS = dict(sh_degree=3, source_path="", model_path="", images="images", resolution=-1,
                      white_background=False, data_device="cuda", eval=False)
# training from object masks (dataset.masks, opt.lambda_alpha; compat/arguments ModelParams / OptimizationParams carry them)
MASK_DEFAULTS = dict(masks="", lambda_alpha=0.5)
# camera pose refinement while training (opt.pose_lr; 0 = off)
POSE_DEFAULTS = dict(pose_lr=0.0)
MIN_OPACITY = 0.005                      # densify_and_prune's opacity floor
SCREEN_SIZE_LIMIT = 20                   # pixels: the screen-radius prune once the first opacity reset has happened


class _Options:
    """getattr(source, name, default) for every field of ``defaults``."""

    def __init__(self, source, defaults):
        for k, v in defaults.items():
            setattr(self, k, getattr(source, k, v) if source is not None else v)


class TrainingScene:
    """The dataset side of a training run: COLMAP cameras with their images, the train / test split, the camera extent,
    and the model directory (input.ply, cameras.json, point_cloud/iteration_N)."""

    def __init__(self, args, gaussians: GaussianModel, load_iteration=None, shuffle=True):
        self.model_path = args.model_path
        self.gaussians = gaussians
        self.loaded_iter = None
        if load_iteration:
            pc = os.path.join(self.model_path, "point_cloud")
            self.loaded_iter = searchForMaxIteration(pc) if load_iteration == -1 else load_iteration
        infos = colmap_io.camera_infos(args.source_path, args.images)
        train, test = colmap_io.split_train_test(infos, bool(args.eval))
        self.cameras_extent = colmap_io.camera_extent(train if train else infos)
        pcd = colmap_io.fetch_point_cloud(args.source_path)
        if not self.loaded_iter:
            os.makedirs(self.model_path, exist_ok=True)
            shutil.copyfile(os.path.join(colmap_io._sparse_dir(args.source_path), "points3D.ply"),
                            os.path.join(self.model_path, "input.ply"))
            json_cams = [camera_to_JSON(i, _JsonCamera(c)) for i, c in enumerate(test + train)]
            with open(os.path.join(self.model_path, "cameras.json"), "w") as f:
                json.dump(json_cams, f)
        if shuffle:
            random.shuffle(train)
            random.shuffle(test)
        masks = getattr(args, "masks", MASK_DEFAULTS["masks"]) or ""
        load = lambda c: colmap_io.load_camera(c, args.resolution, args.white_background, args.data_device, masks=masks)
        self.train_cameras = [load(c) for c in train]
        self.test_cameras = [load(c) for c in test]
        if self.loaded_iter:
            gaussians.load_ply(os.path.join(self.model_path, "point_cloud", f"iteration_{self.loaded_iter}",
                                            "point_cloud.ply"))
        else:
            gaussians.create_from_pcd(pcd, self.cameras_extent)

    def save(self, iteration):
        self.gaussians.save_ply(os.path.join(self.model_path, "point_cloud", f"iteration_{iteration}", "point_cloud.ply"))

    def getTrainCameras(self, scale=1.0):
        return self.train_cameras

    def getTestCameras(self, scale=1.0):
        return self.test_cameras


class _JsonCamera:
    """A CameraInfo seen through the attributes scene.camera_to_JSON reads (the dataset's own image size)."""

    def __init__(self, info):
        self.R, self.T, self.FoVx, self.FoVy = info.R, info.T, info.FoVx, info.FoVy
        self.image_name, self.image_width, self.image_height = info.image_name, info.width, info.height


def psnr(img, gt) -> float:
    mse = torch.mean((img.float() - gt.float()) ** 2).item()
    return float("inf") if mse == 0.0 else 20.0 * math.log10(1.0 / math.sqrt(mse))


def evaluate_masked(cameras, gaussians, pipe, background) -> tuple:
    """(mean L1, mean PSNR, mean alpha L1, mean silhouette IoU) of no-grad renders of cameras that carry ``gt_mask``: the
    target is the image inside the mask composited over ``background``; alpha L1 = mean|alpha - mask|, IoU of alpha > 0.5
    against mask > 0.5."""
    from .gaussian_renderer import render
    from .train_ops import l1_loss
    acc = [[], [], [], []]
    with torch.no_grad():
        for cam in cameras:
            pkg = render(cam, gaussians, pipe, background, return_alpha=True)
            image = torch.clamp(pkg["render"], 0.0, 1.0)
            m = cam.gt_mask.to(image.device)
            gt = torch.clamp(cam.original_image.to(image.device) * m + background.reshape(3, 1, 1) * (1.0 - m), 0.0, 1.0)
            alpha = pkg["alpha"]
            acc[0].append(float(l1_loss(image, gt).item()))
            acc[1].append(psnr(image, gt))
            acc[2].append(float(torch.mean(torch.abs(alpha - m)).item()))
            a, g = alpha > 0.5, m > 0.5
            union = int((a | g).sum().item())
            acc[3].append(1.0 if union == 0 else int((a & g).sum().item()) / union)
    return tuple(sum(v) / len(v) for v in acc) if cameras else (float("nan"),) * 4


def evaluate(cameras, gaussians, pipe, background) -> tuple:
    """(mean L1, mean PSNR) of no-grad renders of ``cameras`` against their images (renders clamped to 0..1)."""
    from .gaussian_renderer import render
    from .train_ops import l1_loss
    l1s, psnrs = [], []
    with torch.no_grad():
        for cam in cameras:
            image = torch.clamp(render(cam, gaussians, pipe, background)["render"], 0.0, 1.0)
            gt = torch.clamp(cam.original_image.to(image.device), 0.0, 1.0)
            l1s.append(float(l1_loss(image, gt).item()))
            psnrs.append(psnr(image, gt))
    return (sum(l1s) / len(l1s), sum(psnrs) / len(psnrs)) if cameras else (float("nan"), float("nan"))


def training_report(iteration, scene, gaussians, pipe, background, quiet=False, train_cameras=None) -> dict:
    """``train_cameras``: the training cameras to evaluate (default: the scene's; pose refinement passes its refined ones)."""
    train = scene.getTrainCameras() if train_cameras is None else train_cameras
    configs = {"test": scene.getTestCameras(), "train": [train[i % len(train)] for i in range(5, 30, 5)] if train else []}
    out = {}
    for name, cams in configs.items():
        if cams and all(getattr(c, "gt_mask", None) is not None for c in cams):
            l1, p, al1, iou = evaluate_masked(cams, gaussians, pipe, background)
            out[name] = {"l1": l1, "psnr": p, "alpha_l1": al1, "iou": iou}
            if not quiet:
                print(f"\n[ITER {iteration}] Evaluating {name}: L1 {l1} PSNR {p} alpha L1 {al1} IoU {iou}")
        elif cams:
            l1, p = evaluate(cams, gaussians, pipe, background)
            out[name] = {"l1": l1, "psnr": p}
            if not quiet:
                print(f"\n[ITER {iteration}] Evaluating {name}: L1 {l1} PSNR {p}")
    return out


def _gui_step(iteration, gaussians, pipe, background, opt, dataset):
    """Serves the remote viewer while one is connected (upstream's loop; nothing happens without a connection)."""
    from . import network_gui
    from .gaussian_renderer import render
    if network_gui.conn is None:
        network_gui.try_connect()
    while network_gui.conn is not None:
        try:
            cam, do_training, pipe.convert_SHs_python, pipe.compute_cov3D_python, keep_alive, scaling = network_gui.receive()
            net_image_bytes = None
            if cam is not None:
                with torch.no_grad():
                    img = render(cam, gaussians, pipe, background, scaling)["render"]
                net_image_bytes = memoryview((torch.clamp(img, 0, 1.0) * 255).byte().permute(1, 2, 0).contiguous().cpu()
                                             .numpy())
            network_gui.send(net_image_bytes, dataset.source_path)
            if do_training and ((iteration < int(opt.iterations)) or not keep_alive):
                break
        except Exception:
            network_gui.conn = None


def _pick_cameras(stack, train_cameras, k):
    """k distinct cameras popped at random from ``stack``; a stack that runs short is emptied, then refilled from
    ``train_cameras`` without the cameras already picked.  Returns (cameras, stack)."""
    if k > len(train_cameras):
        raise ValueError(f"batch_size {k} is larger than the {len(train_cameras)} training cameras")
    cams = []
    while len(cams) < k:
        if not stack:
            stack = [c for c in train_cameras if all(c is not d for d in cams)]
        cams.append(stack.pop(random.randint(0, len(stack) - 1)))
    return cams, stack


def train_step_batch(gaussians, cams, pipe, bg, lambda_dssim, lambda_alpha=None):
    """The forward and backward of one multi-view step: the B cameras in one render_batch, the loss = the mean of the B
    per-view image losses, loss.backward().  Returns (loss, render_batch's dict).  Each view's screen-space gradient in
    ``viewspace_points.grad`` then carries a factor 1/B: GaussianModel.add_batch_render_stats(..., grad_scale=B) undoes it.
    ``lambda_alpha`` (not None): the cameras carry ``gt_mask`` and each view takes MaskedImageLoss against its own
    background (``bg`` [3] or [B,3])."""
    from .gaussian_renderer import render_batch
    from .train_ops import ImageLoss, MaskedImageLoss
    if lambda_alpha is not None:
        pkg = render_batch(cams, gaussians, pipe, bg, return_alpha=True)
        image, alpha = pkg["render"], pkg["alpha"]
        bgs = [bg[v] if bg.dim() == 2 else bg for v in range(len(cams))]
        loss = sum(MaskedImageLoss.apply(image[v], alpha[v], cam.original_image, cam.gt_mask, bgs[v], float(lambda_dssim),
                                         float(lambda_alpha)) for v, cam in enumerate(cams)) / len(cams)
        loss.backward()
        return loss, pkg
    pkg = render_batch(cams, gaussians, pipe, bg)
    image = pkg["render"]
    loss = sum(ImageLoss.apply(image[v], cam.original_image, float(lambda_dssim)) for v, cam in enumerate(cams)) / len(cams)
    loss.backward()
    return loss, pkg


class PoseRefinement:
    """The pose corrections of the training cameras (``--pose_lr``): a zero 6-vector leaf per camera, stored in units that
    give one Adam learning rate the two step sizes (rotation pose_lr, translation pose_lr x extent), and the PosedCamera
    each step renders through."""

    def __init__(self, cameras, pose_lr: float, extent: float, device):
        from .camera_pose import PosedCamera
        self.cameras = list(cameras)
        self.scale = torch.tensor([1.0, 1.0, 1.0, extent, extent, extent], dtype=torch.float32, device=device)
        self.leaves = [torch.zeros(6, dtype=torch.float32, device=device, requires_grad=True) for _ in self.cameras]
        self.posed = {id(c): PosedCamera(c, torch.zeros(6, device=device)) for c in self.cameras}
        self._leaf = {id(c): u for c, u in zip(self.cameras, self.leaves)}
        self.optimizer = torch.optim.Adam(self.leaves, lr=float(pose_lr))

    def view(self, cam):
        """``cam`` through its current correction (differentiable in it)."""
        p = self.posed[id(cam)]
        p.delta = self._leaf[id(cam)] * self.scale
        return p

    def deltas(self):
        return {c.image_name: (u.detach() * self.scale).cpu() for c, u in zip(self.cameras, self.leaves)}

    def refined(self):
        """Plain Cameras of the refined poses (no gradient)."""
        from .camera_pose import PosedCamera
        return [PosedCamera(c, (u.detach() * self.scale)).refined() for c, u in zip(self.cameras, self.leaves)]

    def write_json(self, path):
        cams = self.refined()
        with open(path, "w") as f:
            json.dump([camera_to_JSON(i, c) for i, c in enumerate(cams)], f)

    def step(self):
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)


def training(dataset, opt, pipe, testing_iterations, saving_iterations, checkpoint_iterations, checkpoint, debug_from,
             quiet=False, batch_size=None):
    """Trains a Gaussian model on ``dataset.source_path`` (COLMAP) into ``dataset.model_path``.  Returns
    {"reports": {iteration: {"test"/"train": {"l1", "psnr"}}}, "num_gaussians": N, "model": GaussianModel}.

    ``batch_size`` (default: ``opt.batch_size`` if the options carry one, else 1) views per optimiser step.  With B > 1
    each step renders B distinct training cameras in one render_batch (one random background per view with
    random_background), the loss is the mean of the B per-view losses, and the densification statistics take each view's
    own loss gradient.  Every schedule -- learning rate, SH degree, densify / opacity reset, test / save / checkpoint
    iterations and ``iterations`` itself -- keeps counting OPTIMISER STEPS: a run with B views per step sees B times as many
    images; divide ``--iterations`` (and the schedules) by B for the same number of images.  Nothing is rescaled here."""
    from . import network_gui
    from .gaussian_renderer import render
    from .train_ops import ImageLoss, MaskedImageLoss
    if batch_size is None:
        batch_size = getattr(opt, "batch_size", 1)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if batch_size > 1 and getattr(pipe, "convert_SHs_python", False):
        raise ValueError("batch_size > 1 renders through render_batch, which takes the kernel-evaluated SH: "
                         "convert_SHs_python is not supported with it")
    masked = _Options(dataset, {"masks": MASK_DEFAULTS["masks"]}).masks or ""
    lambda_alpha = float(_Options(opt, {"lambda_alpha": MASK_DEFAULTS["lambda_alpha"]}).lambda_alpha)
    pose_lr = float(_Options(opt, POSE_DEFAULTS).pose_lr)
    if pose_lr < 0.0:
        raise ValueError(f"pose_lr must be >= 0, got {pose_lr}")
    if lambda_alpha < 0.0:
        raise ValueError(f"lambda_alpha must be >= 0, got {lambda_alpha}")
    opt = _Options(opt, OPTIMIZATION_DEFAULTS)
    dataset = _Options(dataset, MODEL_DEFAULTS)
    if masked:
        dataset.masks = masked          # (cfg_args and TrainingScene; an unmasked run writes what it wrote before)
    testing_iterations, saving_iterations = set(testing_iterations or ()), set(saving_iterations or ())
    checkpoint_iterations = set(checkpoint_iterations or ())
    os.makedirs(dataset.model_path, exist_ok=True)
    with open(os.path.join(dataset.model_path, "cfg_args"), "w") as f:
        f.write(str(Namespace(**vars(dataset))))
    gaussians = GaussianModel(dataset.sh_degree, device=dataset.data_device)
    scene = TrainingScene(dataset, gaussians)
    gaussians.training_setup(opt)
    first_iter = 0
    if checkpoint:
        model_params, first_iter = torch.load(checkpoint, weights_only=False)
        gaussians.restore(model_params, opt)
    dev = gaussians._xyz.device
    background = torch.tensor([1, 1, 1] if dataset.white_background else [0, 0, 0], dtype=torch.float32, device=dev)
    poses = PoseRefinement(scene.getTrainCameras(), pose_lr, scene.cameras_extent, dev) if pose_lr > 0.0 else None
    posed = (lambda c: c) if poses is None else poses.view
    iterations = int(opt.iterations)
    stack = None
    reports = {}
    for iteration in range(first_iter + 1, iterations + 1):
        if network_gui.conn is not None or network_gui._listener is not None:
            _gui_step(iteration, gaussians, pipe, background, opt, dataset)
        gaussians.update_learning_rate(iteration)
        if iteration % 1000 == 0:
            gaussians.oneupSHdegree()
        if batch_size == 1:
            if not stack:
                stack = scene.getTrainCameras().copy()
            cam = stack.pop(random.randint(0, len(stack) - 1))
            if iteration - 1 == debug_from:
                pipe.debug = True
            bg = torch.rand(3, device=dev) if opt.random_background else background
            pkg = render(posed(cam), gaussians, pipe, bg, return_alpha=bool(masked))
            image, viewspace, radii = pkg["render"], pkg["viewspace_points"], pkg["radii"]
            if masked:
                loss = MaskedImageLoss.apply(image, pkg["alpha"], cam.original_image, cam.gt_mask, bg,
                                             float(opt.lambda_dssim), lambda_alpha)
            else:
                loss = ImageLoss.apply(image, cam.original_image, float(opt.lambda_dssim))
            loss.backward()
        else:
            cams, stack = _pick_cameras(stack or [], scene.getTrainCameras(), batch_size)
            if iteration - 1 == debug_from:
                pipe.debug = True
            bg = torch.rand((batch_size, 3), device=dev) if opt.random_background else background
            loss, pkg = train_step_batch(gaussians, [posed(c) for c in cams], pipe, bg, opt.lambda_dssim,
                                         lambda_alpha if masked else None)
            viewspace, radii = pkg["viewspace_points"], pkg["radii"]
        with torch.no_grad():
            if iteration in testing_iterations:
                reports[iteration] = training_report(iteration, scene, gaussians, pipe, background, quiet,
                                                     None if poses is None else poses.refined())
            if iteration in saving_iterations:
                if not quiet:
                    print(f"\n[ITER {iteration}] Saving Gaussians")
                scene.save(iteration)
                if poses is not None:
                    poses.write_json(os.path.join(dataset.model_path, "cameras_refined.json"))
            if iteration < opt.densify_until_iter:
                if batch_size == 1:
                    gaussians.add_render_stats(viewspace, radii)
                else:
                    gaussians.add_batch_render_stats(viewspace, radii, grad_scale=batch_size)
                if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                    size_threshold = SCREEN_SIZE_LIMIT if iteration > opt.opacity_reset_interval else None
                    gaussians.densify_and_prune(opt.densify_grad_threshold, MIN_OPACITY, scene.cameras_extent,
                                                size_threshold)
                if iteration % opt.opacity_reset_interval == 0 or (dataset.white_background and
                                                                   iteration == opt.densify_from_iter):
                    gaussians.reset_opacity()
            if iteration < iterations:
                gaussians.optimizer.step()
                gaussians.optimizer.zero_grad(set_to_none=True)
                if poses is not None:
                    poses.step()
            if iteration in checkpoint_iterations:
                if not quiet:
                    print(f"\n[ITER {iteration}] Saving Checkpoint")
                torch.save((gaussians.capture(), iteration),
                           os.path.join(dataset.model_path, f"chkpnt{iteration}.pth"))
                if poses is not None:
                    torch.save(poses.deltas(), os.path.join(dataset.model_path, f"chkpnt{iteration}_poses.pth"))
    out = {"reports": reports, "num_gaussians": int(gaussians.get_xyz.shape[0]), "model": gaussians}
    if poses is not None:
        out["refined_cameras"] = poses.refined()
    return out


def _parser() -> ArgumentParser:
    p = ArgumentParser(description="Train a 3D Gaussian splatting model on a COLMAP dataset")
    short = {"source_path": "-s", "model_path": "-m", "images": "-i", "resolution": "-r", "white_background": "-w"}
    for k, v in {**MODEL_DEFAULTS, **OPTIMIZATION_DEFAULTS, **MASK_DEFAULTS, **POSE_DEFAULTS,
                 **dict(convert_SHs_python=False, compute_cov3D_python=False, debug=False)}.items():
        flags = ["--" + k] + ([short[k]] if k in short else [])
        if isinstance(v, bool):
            p.add_argument(*flags, action="store_true", default=v)
        else:
            p.add_argument(*flags, type=type(v), default=v)
    p.add_argument("--debug_from", type=int, default=-1)
    p.add_argument("--test_iterations", nargs="+", type=int, default=[7_000, 30_000])
    p.add_argument("--save_iterations", nargs="+", type=int, default=[7_000, 30_000])
    p.add_argument("--checkpoint_iterations", nargs="+", type=int, default=[])
    p.add_argument("--start_checkpoint", type=str, default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch_size", type=int, default=1,
                   help="views per optimiser step (schedules and --iterations count steps, not views)")
    p.add_argument("--quiet", action="store_true")
    return p


def main(argv=None) -> int:
    args = _parser().parse_args(argv)
    if not args.source_path or not args.model_path:
        print("both -s <colmap dir> and -m <output dir> are required", file=sys.stderr)
        return 2
    args.save_iterations = list(args.save_iterations) + [args.iterations]
    random.seed(args.seed)
    torch.manual_seed(args.seed)
    print("Optimizing " + args.model_path)
    training(args, args, args, args.test_iterations, args.save_iterations, args.checkpoint_iterations,
             args.start_checkpoint, args.debug_from, quiet=args.quiet, batch_size=args.batch_size)
    print("\nTraining complete.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
