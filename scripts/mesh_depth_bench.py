"""Times the mesh depth renderer and the BOP ground-truth reduction, and compares mesh-derived ground truth with the splat
masks (not part of bench.py).

    python scripts/mesh_depth_bench.py [--resolutions 64 128 256] [--objects 8] [--views 32] [--size 800] [--skip-compare]

Timing.  For every grid resolution: 8 objects x 32 views at 800^2, once on the toolkit's 3x canvas and once without margin.
The meshes are marching-tetrahedra surfaces of a bumpy sphere (mesh.march), 0.2 units across, seen from about 1 unit; a last
mesh, "box12", is a 12-face cube of side 0.5 at 0.6 to 0.9 units, whose faces all take the large path.  The job arrays, the
workspace and the outputs are built once; each figure is the median of 5 hipEvent pairs after a warm-up around the
pgr_mesh_depth calls of the batch (64 jobs per call) and around its pgr_bop_gt_info calls, nothing else in between.  One JSON
line per shape: triangles per second, milliseconds per frame (= per view, all objects), and the share of faces whose clipped
box holds more than 256 samples (a float64 estimate on the host over the first view's jobs, not the kernel's own count).

Comparison.  A merged scene of 8 Gaussian boxes on a ground plane (scenes.scene_c3) is rendered by FrameRenderer from 32
views; every object's mesh comes from mesh.extract_mesh of its own Gaussians.  mesh_render.gt_from_meshes runs on the depth
image as the dataset writer quantises it, at delta = 5 and 15 mm, and one JSON line per delta gives the IoU of its
mask_visib with the frames' splat masks, of its mask with the splat silhouettes, and the difference in visib_fract against
bop_pose.gt_info_from_masks."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def bumpy_sphere(resolution, seed):
    import torch
    from pegasus_amd import mesh
    rng = np.random.default_rng(seed)
    ax = torch.linspace(-1, 1, resolution, device="cuda")
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    a, b, c = rng.uniform(2, 5, 3)
    sdf = r - (0.7 + 0.08 * torch.sin(a * x + 1) * torch.sin(b * y + 2) * torch.sin(c * z + 3))
    m = mesh.march(sdf.contiguous(), mesh.Grid(resolution, resolution, resolution, (-1.0, -1.0, -1.0), 2.0 / (resolution - 1)))
    return mesh.Mesh((m.vertices * 0.1).astype(np.float32), m.faces)


def cube(side):
    from pegasus_amd import mesh
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32) * np.float32(0.5 * side)
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return mesh.Mesh(v, np.asarray(f, np.int32))


def large_share(meshes, jobs, K, W, H, margin):
    """Share of rasterised faces whose clipped box holds more than 256 samples, from the float64 projection on the host."""
    big = total = 0
    for obj_id, R, t in jobs:
        v, f = meshes.mesh(obj_id)
        p = v.astype(np.float64) @ np.asarray(R).T + t
        u = K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2] + margin[0] - 0.5
        w = K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2] + margin[1] - 0.5
        bw = np.clip(np.floor(u[f].max(1)), -1, W + 2 * margin[0] - 1) - np.clip(np.ceil(u[f].min(1)), 0, W + 2 * margin[0]) + 1
        bh = np.clip(np.floor(w[f].max(1)), -1, H + 2 * margin[1] - 1) - np.clip(np.ceil(w[f].min(1)), 0, H + 2 * margin[1]) + 1
        n = np.maximum(bw, 0) * np.maximum(bh, 0)
        big += int((n > 256).sum()); total += int((n > 0).sum())
    return big / max(total, 1)


def median_ms(fn, repeats=5):
    import torch
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def time_shape(meshes, jobs, frames, n_views, K, W, H, margin, chunk=64):
    """(render ms, gt_info ms) of the whole batch: the library calls alone, arguments prepared beforehand."""
    import torch
    from pegasus_amd import _lib, mesh_render as R
    L = _lib.lib()
    dev = meshes.device
    Wc, Hc = W + 2 * margin[0], H + 2 * margin[1]
    stream = _lib.stream_ptr(dev)
    out = torch.empty((chunk, Hc, Wc), dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    scene = torch.full((n_views, H, W), 2.0, device=dev)
    mask = torch.empty((chunk, H, W), dtype=torch.uint8, device=dev)
    visib = torch.empty_like(mask)
    stats = torch.empty((chunk, _lib.PGR_GT_INFO_STATS), dtype=torch.int32, device=dev)
    calls, keep = [], []
    for j0 in range(0, len(jobs), chunk):
        part = jobs[j0:j0 + chunk]
        arr = R.mesh_jobs(meshes, part, K, margin)
        nbytes = int(L.pgr_mesh_depth_workspace_bytes(len(part), arr))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        gj = (_lib.PgrGtInfoJob * len(part))(*[_lib.PgrGtInfoJob(slot=k, frame=int(frames[j0 + k]), fx=K[0, 0], fy=K[1, 1], cx=K[0, 2],
                                                                  cy=K[1, 2]) for k in range(len(part))])
        calls.append((len(part), arr, ws, nbytes, gj))
        keep.append(ws)

    def render():
        for n, arr, ws, nbytes, _gj in calls:
            _lib.check(L.pgr_mesh_depth(_lib.ptr(meshes.vertices), meshes.vertices.shape[0], _lib.ptr(meshes.faces),
                                        meshes.faces.shape[0], n, arr, Wc, Hc, float(R.DEFAULT_NEAR), _lib.ptr(out), chunk,
                                        _lib.ptr(count), _lib.ptr(ws), nbytes, stream), "pgr_mesh_depth")

    def reduce():
        for n, _arr, _ws, _nbytes, gj in calls:
            _lib.check(L.pgr_bop_gt_info(_lib.ptr(out), chunk, Wc, Hc, margin[0], margin[1], _lib.ptr(scene), n_views, W, H, n, gj,
                                         0.015, _lib.ptr(mask), _lib.ptr(visib), _lib.ptr(stats), stream), "pgr_bop_gt_info")
    return median_ms(render), median_ms(reduce)


def timing(a):
    from scipy.spatial.transform import Rotation as Rot
    from pegasus_amd import mesh_render as R
    W = H = a.size
    K = np.array([[1.2 * W, 0, W / 2], [0, 1.2 * W, H / 2], [0, 0, 1.0]])
    for res in list(a.resolutions) + ["box12"]:
        rng = np.random.default_rng(3)
        if res == "box12":
            meshes, spread, z_range = R.MeshSet({k + 1: cube(0.5) for k in range(a.objects)}), 0.1, (0.6, 0.9)
        else:
            meshes, spread, z_range = R.MeshSet({k + 1: bumpy_sphere(res, k) for k in range(a.objects)}), 0.4, (0.8, 1.3)
        jobs, frames = [], []
        for v in range(a.views):
            for k in range(a.objects):
                t = np.array([rng.uniform(-spread, spread), rng.uniform(-spread, spread), rng.uniform(*z_range)])
                jobs.append((k + 1, Rot.random(random_state=int(rng.integers(1 << 30))).as_matrix(), t)); frames.append(v)
        faces = sum(meshes.ranges[j[0]][3] for j in jobs)
        for name, margin in (("canvas3x", (W, H)), ("no_margin", (0, 0))):
            t_render, t_reduce = time_shape(meshes, jobs, frames, a.views, K, W, H, margin)
            print(json.dumps(dict(mesh=res, shape=name, jobs=len(jobs), faces_per_mesh=faces // len(jobs),
                                  render_ms=round(t_render, 3), gt_info_ms=round(t_reduce, 3),
                                  triangles_per_s=round(faces / (t_render * 1e-3)),
                                  render_ms_per_frame=round(t_render / a.views, 4),
                                  gt_info_ms_per_frame=round(t_reduce / a.views, 4),
                                  large_share=round(large_share(meshes, jobs[:a.objects], K, W, H, margin), 5))), flush=True)


def compare(a):
    """Mesh-derived ground truth against the splat masks of a FrameRenderer batch, at delta = 5 and 15 mm."""
    import torch
    from pegasus_amd import bop_pose, masks as M, mesh, mesh_render as R, scenes
    from pegasus_amd.frames import FrameRenderer
    from pegasus_amd.gaussian_model import GaussianModel
    W = H = a.size
    cloud, views = scenes.scene_c3(scale=a.compare_scale, n_views=a.views, width=W, height=H)
    act = cloud.activated()
    fr = FrameRenderer(act["means3d"], act["opacities"], act["scales"], act["rotations"], act["shs"], cloud.object_id)
    extracted = {}
    for k in range(1, fr.K + 1):                                  # the objects stand in the world frame: model = world
        s = cloud.object_id == k
        model = GaussianModel.from_arrays(cloud.xyz[s], cloud.features_dc[s], cloud.features_rest[s], cloud.opacity[s],
                                          cloud.scaling[s], cloud.rotation[s])
        extracted[k] = mesh.extract_mesh(model, resolution=a.compare_resolution)
    meshes = R.MeshSet(extracted)
    specs = [fr.view_spec(v) for v in views]
    frames = fr.render_frames(specs)
    sil = fr.render_silhouettes(specs)
    torch.cuda.synchronize()
    gt, cam = bop_pose.batch_pose_records(views, {k: np.eye(4) for k in range(1, fr.K + 1)})
    mm = M.pack_frames(depth=frames["depth"])["depth_mm"].to(torch.int32) & 0xFFFF        # the written depth image
    splat = bop_pose.gt_info_from_masks(frames["masks"], sil, mm != 0)
    splat_vis, splat_sil = frames["masks"].bool(), sil.bool()

    def iou(x, y):
        inter, union = (x & y).flatten(2).sum(2).double(), (x | y).flatten(2).sum(2).double()
        per = (inter / union.clamp(min=1))[union > 0].cpu().numpy()
        return dict(pooled=round(float(inter.sum() / union.sum()), 4), mean=round(float(per.mean()), 4),
                    median=round(float(np.median(per)), 4), min=round(float(per.min()), 4), pairs=int(per.size))
    for delta in (5.0, 15.0):
        masks, visibs, info = R.gt_from_meshes(meshes, gt, cam, mm, delta=delta, translation_scale=1.0)
        mesh_vis, mesh_sil = torch.stack(visibs).bool(), torch.stack(masks).bool()
        fract = np.array([[e["visib_fract"] for e in f] for f in info])
        px_all = np.array([[e["px_count_all"] for e in f] for f in info])
        whole = (px_all == mesh_sil.flatten(2).sum(2).cpu().numpy()) & (px_all > 0)       # silhouette wholly inside the image
        d = fract - splat["visib_fract"]
        stat = lambda x: dict(mean=round(float(x.mean()), 4), mean_abs=round(float(np.abs(x).mean()), 4),
                              max_abs=round(float(np.abs(x).max()), 4), pairs=int(x.size)) if x.size else dict(pairs=0)
        print(json.dumps(dict(compare="mesh vs splat", delta_mm=delta, views=a.views, objects=fr.K, gaussians=cloud.n,
                              mesh_resolution=a.compare_resolution, faces=[int(len(m.faces)) for m in extracted.values()],
                              iou_mask_visib=iou(mesh_vis, splat_vis), iou_mask=iou(mesh_sil, splat_sil),
                              visib_fract_mesh_minus_splat=stat(d), visib_fract_untruncated=stat(d[whole]),
                              visib_fract_mesh_mean=round(float(fract.mean()), 4),
                              visib_fract_splat_mean=round(float(splat["visib_fract"].mean()), 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-compare", action="store_true")
    ap.add_argument("--compare-scale", type=float, default=1.0, help="fraction of the merged scene's Gaussian counts")
    ap.add_argument("--compare-resolution", type=int, default=128, help="grid resolution of the extracted object meshes")
    a = ap.parse_args()
    if not a.skip_compare:
        compare(a)
    if not a.skip_timing:
        timing(a)


if __name__ == "__main__":
    main()
