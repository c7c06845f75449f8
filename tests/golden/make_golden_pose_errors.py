"""Generates tests/golden/bop_pose_errors.npz from the BOP toolkit of the reference checkout.

Run on the build machine only (``python tests/golden/make_golden_pose_errors.py``); nothing at test time reads the
reference.  Only inputs and the toolkit's OUTPUTS are stored, no reference source text.  The toolkit functions are called
as its scripts call them:
  symmetries   misc.get_symmetry_transformations for the six sets of tests/pose_error_cases.GOLDEN_SETS
  errors       pose_error.mssd, mspd, add, adi, re, te and proj for 24 pairs (four per set: equal, composed with a symmetry,
               small, medium, a half-turn flip, farther than the diameter, cycling)
  matching     pose_matching.match_poses, pose_matching.match_poses_scene and score.calc_localization_scores on one
               synthetic scene: ties in score, an estimate that matches nothing, two instances of one object, an invalid
               ground truth
"""
import json
import sys
import types
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))

import pose_error_cases as PC          # noqa: E402

N_POINTS = 600
PAIRS_PER_SET = 4


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
    from bop_toolkit_lib import misc, pose_error, pose_matching, score
    return misc, pose_error, pose_matching, score


def matching_scene():
    """errs of one scene (im_id -> estimates), its ground truth and validity."""
    scene_gt = {0: [{"obj_id": 1}, {"obj_id": 1}, {"obj_id": 2}], 1: [{"obj_id": 2}, {"obj_id": 3}], 2: [{"obj_id": 1}]}
    scene_gt_valid = {0: [True, True, True], 1: [True, False], 2: [True]}
    errs = [
        # image 0, object 1: two instances, three estimates, the first two tied in score
        dict(im_id=0, obj_id=1, est_id=0, score=0.9, errors={0: [0.30], 1: [0.04]}),
        dict(im_id=0, obj_id=1, est_id=1, score=0.9, errors={0: [0.08], 1: [0.03]}),
        dict(im_id=0, obj_id=1, est_id=2, score=0.5, errors={0: [0.02], 1: [0.01]}),
        # image 0, object 2: the estimate matches nothing
        dict(im_id=0, obj_id=2, est_id=0, score=0.7, errors={2: [0.61]}),
        # image 1: object 2 found by the lower-scored estimate only, object 3's ground truth is invalid
        dict(im_id=1, obj_id=2, est_id=0, score=0.8, errors={0: [0.12]}),
        dict(im_id=1, obj_id=2, est_id=1, score=0.2, errors={0: [0.05]}),
        dict(im_id=1, obj_id=3, est_id=0, score=0.9, errors={1: [0.01]}),
        # image 2: an error exactly at the threshold does not match
        dict(im_id=2, obj_id=1, est_id=0, score=0.4, errors={0: [0.1]}),
    ]
    return scene_gt, scene_gt_valid, errs


def main():
    misc, pose_error, pose_matching, score = toolkit()
    out = {}
    pts = PC.points(N_POINTS, 11)
    out["pts"] = pts
    out["K"] = PC.K_SHARED
    out["set_names"] = np.asarray(list(PC.GOLDEN_SETS))
    out["model_infos"] = np.asarray(json.dumps({k: dict(info=v[0], step=v[1]) for k, v in PC.GOLDEN_SETS.items()}))
    diam = PC.diameter(pts)
    p64 = pts.astype(np.float64)
    rows = {k: [] for k in ("mssd", "mspd", "add", "adi", "re", "te", "proj")}
    pair_set, pair_kind, R_est, t_est, R_gt, t_gt = [], [], [], [], [], []
    for si, (name, (info, step)) in enumerate(PC.GOLDEN_SETS.items()):
        syms = misc.get_symmetry_transformations(info, step)
        sym_R = np.stack([np.asarray(s["R"], np.float64).reshape(3, 3) for s in syms])
        sym_t = np.stack([np.asarray(s["t"], np.float64).reshape(3) for s in syms])
        out[f"sym_R_{name}"], out[f"sym_t_{name}"] = sym_R, sym_t
        kinds = PC.KINDS[(si * PAIRS_PER_SET) % len(PC.KINDS):] + PC.KINDS[:(si * PAIRS_PER_SET) % len(PC.KINDS)]
        Re, te, Rg, tg, names = PC.make_pairs(PAIRS_PER_SET, 100 + si, sym_R, sym_t, diam, kinds)
        for k in range(PAIRS_PER_SET):
            a = (Re[k], te[k].reshape(3, 1), Rg[k], tg[k].reshape(3, 1))
            rows["mssd"].append(pose_error.mssd(*a, p64, syms))
            rows["mspd"].append(pose_error.mspd(*a, PC.K_SHARED, p64, syms))
            rows["add"].append(pose_error.add(*a, p64))
            rows["adi"].append(pose_error.adi(*a, p64))
            rows["re"].append(pose_error.re(Re[k], Rg[k]))
            rows["te"].append(pose_error.te(te[k].reshape(3, 1), tg[k].reshape(3, 1)))
            rows["proj"].append(pose_error.proj(*a, PC.K_SHARED, p64))
            pair_set.append(si); pair_kind.append(names[k])
            print(name, names[k], len(syms), *(f"{rows[e][-1]:.6g}" for e in rows))
        R_est.append(Re); t_est.append(te); R_gt.append(Rg); t_gt.append(tg)
    out.update(pair_set=np.asarray(pair_set), pair_kind=np.asarray(pair_kind), R_est=np.concatenate(R_est),
               t_est=np.concatenate(t_est), R_gt=np.concatenate(R_gt), t_gt=np.concatenate(t_gt))
    out.update({f"err_{k}": np.asarray(v, np.float64) for k, v in rows.items()})

    scene_gt, scene_gt_valid, errs = matching_scene()
    matching = {"scene_gt": {str(k): v for k, v in scene_gt.items()}, "scene_gt_valid": {str(k): v for k, v in scene_gt_valid.items()},
                "errs": [dict(e, errors={str(g): v for g, v in e["errors"].items()}) for e in errs], "results": []}
    for th, n_top in ((0.1, 0), (0.1, 1), (0.35, 0), (0.05, 2), (0.7, 0)):
        matches = pose_matching.match_poses_scene(7, scene_gt, scene_gt_valid, errs, [th], n_top)
        scores = score.calc_localization_scores([7], [1, 2, 3], matches, n_top, do_print=False)
        group = [e for e in errs if e["im_id"] == 0 and e["obj_id"] == 1]
        plain = pose_matching.match_poses(group, [th], n_top, scene_gt_valid[0])
        matching["results"].append({"th": th, "n_top": n_top, "matches": matches, "plain": plain,
                                    "scores": {k: ({str(i): x for i, x in v.items()} if isinstance(v, dict) else v)
                                               for k, v in scores.items()}})
        print(th, n_top, scores["recall"], scores["tp_count"], scores["targets_count"])
    out["matching"] = np.asarray(json.dumps(matching))
    np.savez_compressed(OUT / "bop_pose_errors.npz", **out)
    print("bop_pose_errors.npz", (OUT / "bop_pose_errors.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
