"""Generates tests/golden/mesh_gt_info.npz, mesh_vsd.npz and mesh_vsd_edges.npz from the BOP toolkit of the reference checkout.

Run on the build machine only (``python tests/golden/make_golden_mesh_render.py``); nothing at test time reads the
reference.  Only inputs and the toolkit's OUTPUTS are stored, no reference source text.  The depth images come from the
tests' own NumPy rasterizer (tests/mesh_raster_reference.render_f32), the toolkit functions are called as its scripts call
them:
  mesh_gt_info   scripts/calc_gt_info.py:117-177 through misc.depth_im_to_dist_im_fast, visibility.estimate_visib_mask_gt
                 and misc.calc_2d_bbox, on the 3x canvas: a truncated object, a fully occluded one, one partly behind a
                 nearer scene, missing-depth holes, and depth differences exactly at delta and one float32 step either side
  mesh_vsd       pose_error.vsd with a stub renderer that returns those NumPy depth images: 12 (estimate, GT) pairs, both
                 cost types, several taus, with and without normalisation by the diameter
  mesh_vsd_edges pose_error.vsd through the same stub on hand-written depth images: an empty union (errors all 1), an estimate
                 wholly outside the image, an all-zero test image, a distance exactly equal to tau under 'step', 'tlinear'
                 clipping at 1, 1x1 images; both cost types, normalised and not
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


def vsd_edge_groups():
    """The inputs of mesh_vsd_edges.npz: groups of estimates against one ground-truth render and one test image, written by
    hand.  Per group: name, K, delta, taus, diameter, depth_gt [H,W], depth_test [H,W], depth_est [B,H,W] and the names of
    the estimates.  At the principal point (an integer pixel here) the distance IS the depth, so differences there are exact."""
    diameter = 143.0
    K = np.array([[90.0, 0, 4.0], [0, 92.0, 3.0], [0, 0, 1.0]])
    H, W = 6, 8
    blob = np.zeros((H, W), np.float32)
    blob[1:5, 2:7] = 600.0 + np.arange(20, dtype=np.float32).reshape(4, 5)
    centre = blob[3, 4]
    taus = [0.05, 20.0 / diameter, float(np.nextafter(20.0 / diameter, 1.0)), 0.5, 20.0, float(np.nextafter(20.0, 100.0)), 60.0]
    test = np.where(blob > 0, blob + 2.0, 1000.0).astype(np.float32)
    test[:, :3] = 380.0                                                       # an occluder over the left columns
    test[2, 5] = test[4, 6] = 0.0                                             # missing depth
    shifted = np.where(blob > 0, blob + 7.0, 0).astype(np.float32)
    shifted[3, 4] = centre + 20.0                                             # |dist_gt - dist_est| == 20 == tau exactly (step: >=)
    shifted[1, 2:7] = 0.0                                                     # the estimate misses a row
    far = np.where(blob > 0, blob + 10.0, 0).astype(np.float32)              # visible, and 10 away: tlinear 10 / 0.05 clips at 1,
    far[0, 1:4] = 590.0                                                       # 10 / 20 does not; and pixels the GT does not cover
    zeros = np.zeros((H, W), np.float32)
    groups = [dict(name="blob", K=K, delta=15.0, taus=taus, diameter=diameter, depth_gt=blob, depth_test=test,
                   depth_est=np.stack([zeros, shifted, far, blob]), est_names=["outside_the_image", "at_tau", "clipped", "perfect"]),
              dict(name="no_gt", K=K, delta=15.0, taus=taus, diameter=diameter, depth_gt=zeros, depth_test=test,
                   depth_est=np.stack([zeros, far, shifted]), est_names=["empty_union", "estimate_only", "estimate_only_2"]),
              dict(name="zero_test", K=K, delta=15.0, taus=taus, diameter=diameter, depth_gt=blob, depth_test=zeros,
                   depth_est=np.stack([shifted, zeros, far]), est_names=["at_tau", "outside_the_image", "clipped"])]
    one = lambda v: np.full((1, 1), v, np.float32)
    for name, K1 in (("pixel_on_axis", np.array([[50.0, 0, 0.0], [0, 50.0, 0.0], [0, 0, 1.0]])),
                     ("pixel_off_axis", np.array([[50.0, 0, 0.3], [0, 55.0, -0.4], [0, 0, 1.0]]))):
        groups.append(dict(name=name, K=K1, delta=15.0, taus=taus, diameter=diameter, depth_gt=one(600.0), depth_test=one(605.0),
                           depth_est=np.stack([one(620.0), one(0.0), one(600.0)]), est_names=["at_tau", "outside_the_image", "perfect"]))
    return groups


def vsd_edges_golden():
    """mesh_vsd_edges.npz: pose_error.vsd at its edges, through the same stub renderer.  errors [B, cost (step, tlinear),
    normalised (0, 1), tau] per group."""
    misc, _, pose_error = toolkit()

    class Stub:
        def __init__(self, est, gt):
            self.queue = [est, gt]

        def render_object(self, obj_id, R, t, fx, fy, cx, cy):
            return {"depth": self.queue.pop(0)}
    out = dict(groups=np.asarray([g["name"] for g in vsd_edge_groups()]))
    for g in vsd_edge_groups():
        rows = []
        for est in g["depth_est"]:
            per_cost = []
            for cost in ("step", "tlinear"):
                per_norm = []
                for norm in (False, True):
                    fresh(misc)
                    per_norm.append(pose_error.vsd(np.eye(3), np.zeros((3, 1)), np.eye(3), np.zeros((3, 1)), g["depth_test"].copy(), g["K"],
                                                   g["delta"], g["taus"], norm, g["diameter"], Stub(est.copy(), g["depth_gt"].copy()), 1, cost))
                per_cost.append(per_norm)
            rows.append(per_cost)
        errors = np.asarray(rows, np.float64)
        print(g["name"], errors.shape, np.round(errors[:, 1, 0], 4).tolist())
        for key in ("K", "depth_gt", "depth_test", "depth_est"):
            out[f"{g['name']}_{key}"] = g[key]
        out[f"{g['name']}_delta"] = np.float64(g["delta"])
        out[f"{g['name']}_taus"] = np.asarray(g["taus"], np.float64)
        out[f"{g['name']}_diameter"] = np.float64(g["diameter"])
        out[f"{g['name']}_est_names"] = np.asarray(g["est_names"])
        out[f"{g['name']}_errors"] = errors
    np.savez_compressed(OUT / "mesh_vsd_edges.npz", **out)


if __name__ == "__main__":
    gt_info_golden()
    vsd_golden()
    vsd_edges_golden()
    for p in ("mesh_gt_info.npz", "mesh_vsd.npz", "mesh_vsd_edges.npz"):
        print(p, (OUT / p).stat().st_size, "bytes")
