"""Generates tests/golden/mesh_gt_info.npz and tests/golden/mesh_vsd.npz from the BOP toolkit of the reference checkout.

Run on the build machine only (``python tests/golden/make_golden_mesh_render.py``); nothing at test time reads the
reference.  Only inputs and the toolkit's OUTPUTS are stored, no reference source text.  The depth images come from the
tests' own NumPy rasterizer (tests/mesh_raster_reference.render_f32), the toolkit functions are called as its scripts call
them:
  mesh_gt_info   scripts/calc_gt_info.py:117-177 through misc.depth_im_to_dist_im_fast, visibility.estimate_visib_mask_gt
                 and misc.calc_2d_bbox, on the 3x canvas: a truncated object, a fully occluded one, one partly behind a
                 nearer scene, missing-depth holes, and depth differences exactly at delta and one float32 step either side
  mesh_vsd       pose_error.vsd with a stub renderer that returns those NumPy depth images: 12 (estimate, GT) pairs, both
                 cost types, several taus, with and without normalisation by the diameter
"""
import sys
import types
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))

import mesh_raster_cases as MC          # noqa: E402
import mesh_raster_reference as MR      # noqa: E402

NEAR = 1.0


def toolkit():
    assert REF.exists(), "reference checkout not present"
    sys.path.insert(0, str(REF))
    sys.path.insert(0, str(REF / "submodules" / "bop_toolkit"))
    for name in ("imageio", "png", "cv2"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
    from bop_toolkit_lib import misc, pose_error, visibility
    return misc, visibility, pose_error


def fresh(misc):
    misc.Precomputer.depth_im_shape = None       # its cache keys on shape and K separately; start every image clean
    misc.Precomputer.K = None


def own_dist(d, x, y, K):
    X, Y = (x - K[0, 2]) / K[0, 0] * np.float64(d), (y - K[1, 2]) / K[1, 1] * np.float64(d)
    return np.sqrt(X * X + Y * Y + np.float64(d) ** 2)


def depth_with_dist(target, x, y, K):
    """A float32 depth whose float32-rounded distance at pixel (x, y) is exactly ``target`` (None if there is none near)."""
    d = np.float32(np.float64(target) / own_dist(1.0, x, y, K))
    for _ in range(64):
        got = np.float32(own_dist(d, x, y, K))
        if got == target:
            return d
        d = np.nextafter(d, np.float32(np.inf if got < target else -np.inf))
    return None


def gt_info_golden():
    misc, visibility, _ = toolkit()
    rng = np.random.default_rng(71)
    W, H = 40, 30
    K = np.array([[60.0, 0, 20.0], [0, 60.0, 15.0], [0, 0, 1.0]])
    delta = 15.0
    v, f = MC.icosphere(2, 60.0)                                     # millimetres
    cases = []                                                       # (name, t, scene depth maker)
    cases.append(("free", (0, 0, 600), lambda m: np.where(m > 0, m + 40, 900)))
    cases.append(("truncated", (190, -120, 600), lambda m: np.full_like(m, 900)))
    cases.append(("occluded", (0, 0, 600), lambda m: np.full_like(m, 300)))
    cases.append(("partly", (10, 5, 600), lambda m: np.where(np.arange(W)[None, :] < 22, 350, 900).astype(np.float32) + 0 * m))
    cases.append(("holes", (-40, 20, 500), lambda m: np.where(rng.random(m.shape) < 0.3, 0, np.where(rng.random(m.shape) < 0.5, 300, 900))))
    cases.append(("at_delta", (0, 0, 600), None))
    cases.append(("outside", (2000, 0, 600), lambda m: np.full_like(m, 900)))
    out = dict(K=K, delta=np.float64(delta), size=np.asarray([W, H]), vertices=v, faces=f, names=np.asarray([c[0] for c in cases]),
               t=np.asarray([c[1] for c in cases], np.float64))
    canv, scenes, res = [], [], dict(px_count_all=[], px_count_valid=[], px_count_visib=[], visib_fract=[], bbox_obj=[],
                                     bbox_visib=[], mask=[], mask_visib=[])
    for name, t, maker in cases:
        R = MC.rotation((1, 2, 3), 0.7)
        large = MR.render_f32([MC.job(v, f, R, t, K[0, 0], K[1, 1], K[0, 2] + W, K[1, 2] + H)], 3 * W, 3 * H, NEAR)[0][0]
        depth_gt = large[H:2 * H, W:2 * W]
        if maker is not None:
            depth = np.asarray(maker(depth_gt), np.float32)
        else:
            # per silhouette pixel a scene depth whose float32 distance differs from the model's by exactly delta, or by the
            # float32 neighbours of that difference
            depth = np.full((H, W), 900, np.float32)
            ys, xs = np.nonzero(depth_gt > 0)
            for n, (y, x) in enumerate(zip(ys, xs)):
                dm = np.float32(own_dist(depth_gt[y, x], x, y, K))
                want = np.float32(dm - np.float32(delta))
                want = [want, np.nextafter(want, np.float32(0)), np.nextafter(want, np.float32(np.inf))][n % 3]
                d = depth_with_dist(want, x, y, K)
                if d is not None:
                    depth[y, x] = d
        fresh(misc)
        dist_gt = misc.depth_im_to_dist_im_fast(depth_gt, K)
        dist_im = misc.depth_im_to_dist_im_fast(depth, K)
        visib_gt = visibility.estimate_visib_mask_gt(dist_im, dist_gt, delta, visib_mode="bop19")
        obj_mask_gt_large = large > 0
        obj_mask_gt = dist_gt > 0
        px_all = int(np.sum(obj_mask_gt_large))
        px_valid = int(np.sum(dist_im[obj_mask_gt] > 0))
        px_visib = int(visib_gt.sum())
        bbox = bbox_visib = [-1, -1, -1, -1]
        if px_visib > 0:
            ys, xs = obj_mask_gt_large.nonzero()
            bbox = misc.calc_2d_bbox(xs - W, ys - H, (W, H))
            ys, xs = visib_gt.nonzero()
            bbox_visib = misc.calc_2d_bbox(xs, ys, (W, H))
        canv.append(large); scenes.append(depth)
        res["px_count_all"].append(px_all); res["px_count_valid"].append(px_valid); res["px_count_visib"].append(px_visib)
        res["visib_fract"].append(px_visib / float(px_all) if px_all > 0 else 0.0)
        res["bbox_obj"].append([int(e) for e in bbox]); res["bbox_visib"].append([int(e) for e in bbox_visib])
        res["mask"].append(obj_mask_gt); res["mask_visib"].append(visib_gt)
        print(name, px_all, px_valid, px_visib, bbox, bbox_visib)
    out["canvases"], out["scene_depth"] = np.stack(canv), np.stack(scenes)
    out["mask"] = np.packbits(np.stack(res.pop("mask")), axis=-1)
    out["mask_visib"] = np.packbits(np.stack(res.pop("mask_visib")), axis=-1)
    out.update({k: np.asarray(x) for k, x in res.items()})
    np.savez_compressed(OUT / "mesh_gt_info.npz", **out)


def vsd_golden():
    misc, _, pose_error = toolkit()
    rng = np.random.default_rng(72)
    W, H = 64, 48
    K = np.array([[90.0, 0, 31.5], [0, 92.0, 24.25], [0, 0, 1.0]])
    v, f = MC.icosphere(2, 55.0)
    v = (v * np.array([1.0, 0.7, 1.3], np.float32)).astype(np.float32)       # an ellipsoid: rotations matter
    diameter, delta, taus = 143.0, 15.0, [0.05, 0.2, 0.5, 20.0, 60.0]
    n = 12
    R_gt = np.stack([MC.rotation(rng.normal(size=3), rng.uniform(0, 3)) for _ in range(n)])
    t_gt = np.stack([[rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(450, 700)] for _ in range(n)])
    R_est = np.stack([MC.rotation(rng.normal(size=3), rng.uniform(0, 0.6)) @ R for R in R_gt])
    t_est = t_gt + rng.normal(0, 1, (n, 3)) * np.array([12, 12, 30]) * rng.uniform(0, 1, (n, 1))
    R_est[0], t_est[0] = R_gt[0], t_gt[0]                                     # a perfect estimate
    t_est[1] = t_gt[1] + np.array([800.0, 0, 0])                              # an estimate outside the image

    def render(R, t):
        return MR.render_f32([MC.job(v, f, R, t, K[0, 0], K[1, 1], K[0, 2], K[1, 2])], W, H, NEAR)[0][0]
    d_est = np.stack([render(R, t) for R, t in zip(R_est, t_est)])
    d_gt = np.stack([render(R, t) for R, t in zip(R_gt, t_gt)])
    test = np.where(d_gt > 0, d_gt + rng.normal(0, 3, d_gt.shape), 1000).astype(np.float32)
    test[:, :, :20][rng.random((n, H, 20)) < 0.5] = 380                      # an occluder over the left part
    test[rng.random(test.shape) < 0.05] = 0                                  # missing depth
    test[2] = 0                                                               # no depth at all

    class Stub:
        def __init__(self, est, gt):
            self.queue = [est, gt]

        def render_object(self, obj_id, R, t, fx, fy, cx, cy):
            return {"depth": self.queue.pop(0)}
    errs = {}
    for cost in ("step", "tlinear"):
        for norm in (False, True):
            rows = []
            for k in range(n):
                fresh(misc)
                rows.append(pose_error.vsd(R_est[k], t_est[k].reshape(3, 1), R_gt[k], t_gt[k].reshape(3, 1), test[k], K, delta,
                                           taus, norm, diameter, Stub(d_est[k], d_gt[k]), 1, cost))
            errs[f"errors_{cost}_{int(norm)}"] = np.asarray(rows, np.float64)
            print(cost, norm, np.round(errs[f"errors_{cost}_{int(norm)}"][:4], 3).tolist())
    np.savez_compressed(OUT / "mesh_vsd.npz", K=K, size=np.asarray([W, H]), vertices=v, faces=f, diameter=np.float64(diameter),
                        delta=np.float64(delta), taus=np.asarray(taus), R_est=R_est, t_est=t_est, R_gt=R_gt, t_gt=t_gt,
                        depth_test=test, depth_est=d_est, depth_gt=d_gt, **errs)


if __name__ == "__main__":
    gt_info_golden()
    vsd_golden()
    for p in ("mesh_gt_info.npz", "mesh_vsd.npz"):
        print(p, (OUT / p).stat().st_size, "bytes")
