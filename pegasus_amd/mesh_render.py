"""Object meshes rendered to depth on the GPU, and what the BOP toolkit builds on its depth renderer: ground-truth masks
(scripts/calc_gt_masks.py), scene_gt_info.json (scripts/calc_gt_info.py) and the VSD pose error (pose_error.vsd).

The meshes are the ``models/obj_NNNNNN.ply`` files ``pegasus_amd.mesh`` writes.  ``pgr_mesh_depth`` replaces the toolkit's
renderer (``renderer.render_object(obj_id, R, t, fx, fy, cx, cy)['depth']``), ``pgr_bop_gt_info`` the per-image sequence of
calc_gt_info.py; both are pinned in pegasus_amd/csrc/meshraster.hip.h.

    python -m pegasus_amd.mesh_render --dataset <dir> --models <dir> [--delta 15] [--translation_scale 1]

recomputes ``mask/``, ``mask_visib/`` and ``scene_gt_info.json`` of every scene under ``<dataset>/train`` from the meshes,
the poses in ``scene_gt.json`` and the depth images.
"""
from __future__ import annotations

import argparse
import ctypes as C
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib, bop_dataset as BD
from .bop_pose import broadcast_K, scene_gt_info_entry

MAX_CANVAS = 8192
DEFAULT_NEAR = 1e-3                  # model units; any positive value keeps the projection defined
DEFAULT_BUDGET = 1 << 30             # bytes of canvases per pgr_mesh_depth call
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


class MeshSet:
    """Triangle meshes by object id, uploaded once: ``vertices`` float32 [V,3] and ``faces`` int32 [F,3] (indices relative to
    the mesh's first vertex) shared by all, ``ranges[obj_id] = (vertex_first, vertex_count, face_first, face_count)``.
    ``meshes``: {obj_id: mesh.Mesh or a PLY path}; ``scale`` multiplies the vertices on load (BOP models are in millimetres:
    0.001 brings them to metres)."""

    def __init__(self, meshes: dict, device="cuda", scale: float = 1.0, diameters: Optional[dict] = None):
        import torch
        from .ply_io import read_ply_mesh
        vs, fs, self.ranges = [], [], {}
        v0 = f0 = 0
        for obj_id in sorted(meshes):
            m = meshes[obj_id]
            v, f = read_ply_mesh(m) if isinstance(m, (str, Path)) else (m.vertices, m.faces)
            v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
            f = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
            if scale != 1.0:
                v = (v.astype(np.float64) * scale).astype(np.float32)
            if len(f) and (f.min() < 0 or f.max() >= len(v)):
                raise ValueError(f"object {obj_id}: a face names a vertex outside 0..{len(v) - 1}")
            self.ranges[int(obj_id)] = (v0, len(v), f0, len(f))
            vs.append(v); fs.append(f)
            v0 += len(v); f0 += len(f)
        self.vertices = torch.from_numpy(np.concatenate(vs) if vs else np.zeros((0, 3), np.float32)).to(device)
        self.faces = torch.from_numpy(np.concatenate(fs) if fs else np.zeros((0, 3), np.int32)).to(device)
        self.diameters = {int(k): float(v) for k, v in (diameters or {}).items()}
        self.device = self.vertices.device

    @classmethod
    def from_dir(cls, models_dir, device="cuda", scale: float = 1.0) -> "MeshSet":
        """Every ``obj_NNNNNN.ply`` of a BOP models directory, diameters from its ``models_info.json`` (scaled alike)."""
        files = BD.model_files(models_dir)
        diam = {int(k): v["diameter"] * scale for k, v in BD.read_models_info(models_dir).items()}
        return cls(files, device=device, scale=scale, diameters=diam)

    def mesh(self, obj_id: int):
        """(vertices, faces) of one object as host arrays."""
        v0, nv, f0, nf = self.ranges[int(obj_id)]
        return self.vertices[v0:v0 + nv].cpu().numpy(), self.faces[f0:f0 + nf].cpu().numpy()


def mesh_jobs(meshes: MeshSet, jobs: Sequence, K, margin=(0, 0), slots: Optional[Sequence[int]] = None):
    """The PgrMeshJob array of ``jobs`` = [(obj_id, R [3,3], t [3]), ...]: pose and intrinsics rounded to float32, the
    principal point moved by the margin."""
    Ks = broadcast_K(K, len(jobs))
    arr = (_lib.PgrMeshJob * max(len(jobs), 1))()
    for k, (obj_id, R, t) in enumerate(jobs):
        if int(obj_id) not in meshes.ranges:
            raise KeyError(f"object {obj_id} is not in the mesh set")
        v0, nv, f0, nf = meshes.ranges[int(obj_id)]
        R32 = np.asarray(R, np.float64).reshape(9).astype(np.float32)
        t32 = np.asarray(t, np.float64).reshape(3).astype(np.float32)
        Kk = Ks[k]
        arr[k] = _lib.PgrMeshJob(vertex_first=v0, vertex_count=nv, face_first=f0, face_count=nf,
                                 R=(C.c_float * 9)(*R32.tolist()), t=(C.c_float * 3)(*t32.tolist()),
                                 fx=float(np.float32(Kk[0, 0])), fy=float(np.float32(Kk[1, 1])),
                                 cx=float(np.float32(Kk[0, 2] + margin[0])), cy=float(np.float32(Kk[1, 2] + margin[1])),
                                 slot=int(k if slots is None else slots[k]))
    return arr


def render_depth(meshes: MeshSet, jobs: Sequence, K, size, margin=(0, 0), near: float = DEFAULT_NEAR,
                 budget_bytes: int = DEFAULT_BUDGET, return_straddle: bool = False):
    """Depth images of ``jobs`` = [(obj_id, R, t), ...] (model to camera, in the meshes' units): float32 [J,Hc,Wc] on the
    meshes' device, camera z of the nearest surface, 0 where nothing is hit.  ``size`` = (W, H) of the image, ``margin`` =
    (mx, my) pixels added on every side (the canvas is W + 2 mx by H + 2 my, the principal point moves by the margin; the
    toolkit's truncation canvas is margin = size).  ``K``: one [3,3] or one per job.  Jobs go to the library in chunks whose
    canvases stay within ``budget_bytes``.  ``return_straddle``: also the number of faces dropped because they straddle
    ``near`` (an int32 tensor, not read back here)."""
    import torch
    W, H = int(size[0]), int(size[1])
    mx, my = int(margin[0]), int(margin[1])
    Wc, Hc = W + 2 * mx, H + 2 * my
    if not (1 <= Wc <= MAX_CANVAS and 1 <= Hc <= MAX_CANVAS) or mx < 0 or my < 0:
        raise ValueError(f"canvas {Wc} x {Hc}: each side must be 1..{MAX_CANVAS}")
    device = meshes.device
    if device.type != "cuda":
        raise RuntimeError("render_depth needs a mesh set on a HIP device; there is no CPU path")
    J = len(jobs)
    Ks = broadcast_K(K, J)
    out = torch.empty((J, Hc, Wc), dtype=torch.float32, device=device)
    straddle = torch.zeros(1, dtype=torch.int32, device=device)
    per_call = max(1, int(budget_bytes) // (4 * Hc * Wc))
    for j0 in range(0, J, per_call):
        chunk = jobs[j0:j0 + per_call]
        arr = mesh_jobs(meshes, chunk, Ks[j0:j0 + per_call], (mx, my))
        ws = _lib.workspace("pgr_mesh_depth", device, len(chunk), arr)
        count = torch.zeros(1, dtype=torch.int32, device=device)
        _lib.call("pgr_mesh_depth", device, _lib.ptr(meshes.vertices), meshes.vertices.shape[0], _lib.ptr(meshes.faces),
                  meshes.faces.shape[0], len(chunk), arr, Wc, Hc, float(near), _lib.ptr(out[j0:j0 + len(chunk)]), len(chunk),
                  _lib.ptr(count), _lib.ptr(ws), ws.numel())
        straddle += count
    return (out, straddle) if return_straddle else out


# ---- ground truth ---------------------------------------------------------------------------------------------------
def dist_image(depth, K):
    """misc.depth_im_to_dist_im_fast in torch: float64 [..., H, W] distances from the camera centre, the pixel taken at its
    integer index, 0 where the depth is 0.  ``K``: float64 [3,3] (or [..., 3, 3] broadcasting over the leading axes)."""
    import torch
    d = depth.to(torch.float64)
    H, W = d.shape[-2:]
    K = torch.as_tensor(np.asarray(K, np.float64) if not torch.is_tensor(K) else K, dtype=torch.float64, device=d.device)
    xs = torch.arange(W, dtype=torch.float64, device=d.device)
    ys = torch.arange(H, dtype=torch.float64, device=d.device)[:, None]
    pre_x = (xs - K[..., 0, 2, None, None]) / K[..., 0, 0, None, None]
    pre_y = (ys - K[..., 1, 2, None, None]) / K[..., 1, 1, None, None]
    X, Y = pre_x * d, pre_y * d
    return torch.sqrt((X * X + Y * Y) + d * d)


def visibility_mask(dist_test, dist_model, delta: float):
    """visibility._estimate_visib_mask, mode bop19: the difference of the distances in float32."""
    import torch
    diff = dist_model.to(torch.float32) - dist_test.to(torch.float32)
    return ((diff <= delta) | (dist_test == 0)) & (dist_model > 0)


def reduce_gt_info_torch(canvases, margin, scene_depth, frames, Ks, delta: float):
    """What pgr_bop_gt_info computes, restated in torch ops on the tensors' device (CPU included): (mask uint8 [J,H,W],
    mask_visib uint8 [J,H,W], stats int32 [J,11]) of canvases float32 [J,Hc,Wc] against scene_depth [F,H,W]; ``frames`` [J]
    names each job's image, ``Ks`` float64 [J,3,3]."""
    import torch
    mx, my = int(margin[0]), int(margin[1])
    J = canvases.shape[0]
    H, W = scene_depth.shape[-2:]
    dev = canvases.device
    frames = torch.as_tensor(np.asarray(frames, np.int64), device=dev)
    Ks = torch.as_tensor(np.asarray(Ks, np.float64), device=dev)
    window = canvases[:, my:my + H, mx:mx + W]
    dist_model = dist_image(window, Ks)
    dist_test = dist_image(scene_depth[frames], Ks)
    visib = visibility_mask(dist_test, dist_model, float(np.float32(delta)))
    mask = dist_model > 0
    large = canvases > 0
    stats = torch.empty((J, _lib.PGR_GT_INFO_STATS), dtype=torch.int64, device=dev)
    stats[:, 0] = large.flatten(1).sum(1)
    stats[:, 1] = (mask & (dist_test > 0)).flatten(1).sum(1)
    stats[:, 2] = visib.flatten(1).sum(1)

    def extent(m, ox, oy, col):
        h, w = m.shape[-2:]
        xs = torch.arange(w, device=dev) - ox
        ys = torch.arange(h, device=dev) - oy
        cols, rows = m.any(-2), m.any(-1)
        stats[:, col + 0] = torch.where(cols, xs, INT32_MAX).amin(-1)
        stats[:, col + 1] = torch.where(rows, ys, INT32_MAX).amin(-1)
        stats[:, col + 2] = torch.where(cols, xs, INT32_MIN).amax(-1)
        stats[:, col + 3] = torch.where(rows, ys, INT32_MIN).amax(-1)
    extent(large, mx, my, 3)
    extent(visib, 0, 0, 7)
    return mask.to(torch.uint8), visib.to(torch.uint8), stats.to(torch.int32)


def reduce_gt_info(canvases, margin, scene_depth, frames, Ks, delta: float):
    """pgr_bop_gt_info: like reduce_gt_info_torch, on a HIP device."""
    import torch
    dev = canvases.device
    if dev.type != "cuda":
        raise RuntimeError("reduce_gt_info needs tensors on a HIP device (reduce_gt_info_torch restates it for any device)")
    canvases = canvases.float().contiguous()
    scene_depth = scene_depth.to(dev).float().contiguous()
    J, Hc, Wc = canvases.shape
    F, H, W = scene_depth.shape
    Ks = np.asarray(Ks, np.float64).reshape(J, 3, 3)
    arr = (_lib.PgrGtInfoJob * max(J, 1))()
    for k in range(J):
        arr[k] = _lib.PgrGtInfoJob(slot=k, frame=int(frames[k]), fx=Ks[k, 0, 0], fy=Ks[k, 1, 1], cx=Ks[k, 0, 2], cy=Ks[k, 1, 2])
    mask = torch.empty((J, H, W), dtype=torch.uint8, device=dev)
    visib = torch.empty_like(mask)
    stats = torch.empty((J, _lib.PGR_GT_INFO_STATS), dtype=torch.int32, device=dev)
    _lib.call("pgr_bop_gt_info", dev, _lib.ptr(canvases), J, Wc, Hc, int(margin[0]), int(margin[1]), _lib.ptr(scene_depth),
              F, W, H, J, arr, float(delta), _lib.ptr(mask), _lib.ptr(visib), _lib.ptr(stats))
    return mask, visib, stats


def info_from_stats(stats) -> dict:
    """scene_gt_info fields from stats rows [..., 11] as calc_gt_info.py derives them: visib_fract = visible / all (0 without
    a silhouette), boxes (x, y, w, h) with w = x_max - x_min (misc.calc_2d_bbox), both [-1,-1,-1,-1] when nothing is
    visible.  Arrays shaped [...] (boxes [..., 4]), the layout bop_pose.scene_gt_info_entry takes."""
    s = np.asarray(stats.cpu() if hasattr(stats, "cpu") else stats).astype(np.int64)
    px_all, px_valid, px_visib = s[..., 0], s[..., 1], s[..., 2]
    seen = (px_visib > 0)[..., None]
    box = lambda c: np.stack([s[..., c], s[..., c + 1], s[..., c + 2] - s[..., c], s[..., c + 3] - s[..., c + 1]], -1)
    fract = np.where(px_all > 0, px_visib / np.maximum(px_all, 1).astype(np.float64), 0.0)
    return dict(px_count_all=px_all, px_count_valid=px_valid, px_count_visib=px_visib, visib_fract=fract,
                bbox_obj=np.where(seen, box(3), -1), bbox_visib=np.where(seen, box(7), -1))


def gt_from_meshes(meshes: MeshSet, scene_gt: dict, scene_camera: dict, depth, delta: float = 15.0,
                   translation_scale: float = 1.0, near: float = DEFAULT_NEAR, budget_bytes: int = DEFAULT_BUDGET):
    """BOP ground truth of a batch of frames from the objects' meshes, as calc_gt_info.py and calc_gt_masks.py compute it:
    every object of ``scene_gt[str(i)]`` is rendered at its pose on the toolkit's 3x canvas and tested against frame i of
    ``depth`` [B,H,W] (the depth images as written, times the frame's ``depth_scale``: millimetres).

    Units follow scene_gt: ``translation_scale`` is what its translations were written with (1000: millimetres, 1:
    metres -- the default here, in bop_pose and in the writer), the meshes are in that unit, the depth is brought to it, and ``delta`` (millimetres, the toolkit's 15) too.
    Returns (masks, masks_visib, info): per frame a uint8 device tensor [K_i,H,W] each, and the scene_gt_info list."""
    import torch
    dev = meshes.device
    depth = torch.as_tensor(depth).to(dev)
    B, H, W = depth.shape
    unit = BD.unit_of(translation_scale)
    scale = torch.tensor([BD.depth_unit(scene_camera[str(i)], unit) for i in range(B)], device=dev)
    scene = (depth.to(torch.float32) * scale.to(torch.float32)[:, None, None]).contiguous()
    jobs, frames, Ks = [], [], []
    for i in range(B):
        K = BD.cam_K(scene_camera[str(i)])
        for e in scene_gt[str(i)]:
            jobs.append((int(e["obj_id"]), *BD.pose_of(e)))
            frames.append(i); Ks.append(K)
    masks = [[] for _ in range(B)]
    visibs = [[] for _ in range(B)]
    rows = []
    per_call = max(1, int(budget_bytes) // (4 * 9 * H * W))
    for j0 in range(0, len(jobs), per_call):
        sl = slice(j0, j0 + per_call)
        canvases = render_depth(meshes, jobs[sl], np.stack(Ks[sl]), (W, H), margin=(W, H), near=near, budget_bytes=budget_bytes)
        m, v, s = reduce_gt_info(canvases, (W, H), scene, frames[sl], np.stack(Ks[sl]), delta * unit)
        rows.append(s)
        for k, i in enumerate(frames[sl]):
            masks[i].append(m[k]); visibs[i].append(v[k])
    stats = torch.cat(rows).cpu().numpy() if rows else np.zeros((0, _lib.PGR_GT_INFO_STATS), np.int32)
    info, at = [], 0
    empty = torch.zeros((0, H, W), dtype=torch.uint8, device=dev)
    for i in range(B):
        n = len(masks[i])
        info.append(scene_gt_info_entry(info_from_stats(stats[at:at + n]), slice(None)) if n else [])
        at += n
    stack = lambda l: torch.stack(l) if l else empty
    return [stack(m) for m in masks], [stack(v) for v in visibs], info


# ---- VSD ------------------------------------------------------------------------------------------------------------
def vsd_from_depths(depth_est, depth_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter, cost_type="step"):
    """pose_error.vsd after its two renders, in torch float64 on the tensors' device: depth_est [B,H,W], depth_gt and
    depth_test [H,W].  Returns float64 [B, len(taus)]."""
    import torch
    K = np.asarray(K, np.float64).reshape(3, 3)
    dist_test, dist_gt, dist_est = dist_image(depth_test, K), dist_image(depth_gt, K), dist_image(depth_est, K)
    visib_gt = visibility_mask(dist_test, dist_gt, delta)
    visib_est = visibility_mask(dist_test, dist_est, delta) | (visib_gt & (dist_est > 0))
    inter, union = visib_gt & visib_est, visib_gt | visib_est
    union_count = union.flatten(-2).sum(-1).to(torch.float64)
    comp_count = union_count - inter.flatten(-2).sum(-1)
    dists = (dist_gt - dist_est).abs()
    if normalized_by_diameter:
        dists = dists / diameter
    errors = []
    for tau in taus:
        if cost_type == "step":
            costs = (dists >= tau).to(torch.float64)
        elif cost_type == "tlinear":
            costs = (dists / tau).clamp(max=1.0)
        else:
            raise ValueError("Unknown pixel matching cost.")
        total = torch.where(inter, costs, torch.zeros_like(costs)).flatten(-2).sum(-1)
        errors.append(torch.where(union_count > 0, (total + comp_count) / union_count.clamp(min=1.0), torch.ones_like(total)))
    return torch.stack(errors, -1)


def vsd(R_est, t_est, R_gt, t_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter, meshes: MeshSet, obj_id,
        cost_type="step", near: float = DEFAULT_NEAR, render=None):
    """Visible Surface Discrepancy with pose_error.vsd's signature, the renderer replaced by the mesh set.  ``R_est`` [3,3]
    with ``t_est`` [3] / [3,1] gives the toolkit's list of errors (one per tau); a batch [B,3,3] / [B,3] against the one
    test image gives a float64 tensor [B, len(taus)].  The B + 1 renders are one pgr_mesh_depth call, the rest torch ops
    on the device.  ``render``: a callable (jobs, K, size) -> depths [J,H,W] used instead of render_depth."""
    import torch
    R_est = np.asarray(R_est, np.float64)
    single = R_est.ndim == 2
    R_est = R_est.reshape(-1, 3, 3)
    t_est = np.asarray(t_est, np.float64).reshape(-1, 3)
    depth_test = torch.as_tensor(depth_test)
    H, W = depth_test.shape
    jobs = [(obj_id, R, t) for R, t in zip(R_est, t_est)] + [(obj_id, np.asarray(R_gt, np.float64).reshape(3, 3),
                                                              np.asarray(t_gt, np.float64).reshape(3))]
    if render is None:
        depths = render_depth(meshes, jobs, K, (W, H), near=near)
    else:
        depths = torch.as_tensor(render(jobs, K, (W, H)))
    depth_test = depth_test.to(depths.device)
    errors = vsd_from_depths(depths[:-1], depths[-1], depth_test, K, delta, taus, normalized_by_diameter, diameter, cost_type)
    return [float(e) for e in errors[0].cpu()] if single else errors


# ---- a dataset on disk ----------------------------------------------------------------------------------------------
def recompute_dataset(dataset_dir, models_dir, delta: float = 15.0, translation_scale: float = 1.0, batch: int = 8,
                      device="cuda"):
    """mask/, mask_visib/ and scene_gt_info.json of every scene under <dataset>/train, from the meshes of ``models_dir``
    (millimetres), scene_gt.json, scene_camera.json and the depth images: calc_gt_info.py plus calc_gt_masks.py."""
    meshes = MeshSet.from_dir(models_dir, device=device, scale=BD.unit_of(translation_scale))
    scenes = BD.scene_dirs(dataset_dir, "train")
    for scene in map(BD.BopScene, scenes):
        gt, cam, ids = scene.gt, scene.camera, scene.image_ids
        info = {}
        scene.make_dirs(("mask", "mask_visib"))
        for b0 in range(0, len(ids), batch):
            chunk = ids[b0:b0 + batch]
            depth = np.stack([scene.read_png("depth", i).astype(np.float32) for i in chunk])
            masks, visibs, infos = gt_from_meshes(meshes, {str(k): gt[i] for k, i in enumerate(chunk)},
                                                  {str(k): cam[i] for k, i in enumerate(chunk)}, depth, delta=delta,
                                                  translation_scale=translation_scale)
            for k, i in enumerate(chunk):
                info[i] = infos[k]
                for name, stack in (("mask", masks[k]), ("mask_visib", visibs[k])):
                    for o, image in enumerate((stack * 255).cpu().numpy()):
                        scene.image_path(name, i, o).write_bytes(BD.encode_png(image))
        scene.write_json(BD.SCENE_GT_INFO, {k: info[k] for k in ids})
    return scenes


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.mesh_render", description=__doc__.split("\n\n")[0])
    p.add_argument("--dataset", required=True)
    p.add_argument("--models", required=True)
    p.add_argument("--delta", type=float, default=15.0, help="visibility tolerance in millimetres (calc_gt_masks.py's default)")
    p.add_argument("--translation_scale", type=float, default=1.0,
                   help="what scene_gt's translations were written with: 1 = metres, 1000 = millimetres")
    p.add_argument("--batch", type=int, default=8)
    a = p.parse_args(argv)
    scenes = recompute_dataset(a.dataset, a.models, a.delta, a.translation_scale, a.batch)
    print(f"recomputed mask/, mask_visib/ and scene_gt_info.json of {len(scenes)} scene(s)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
