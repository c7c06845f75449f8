"""Evaluates a BOP results file against a dataset on the GPU: the toolkit's eval_calc_errors.py and eval_calc_scores.py for
MSSD and MSPD (and VSD on request), through ``pegasus_amd.pose_error``.

    python -m pegasus_amd.pose_eval --results <csv> --dataset <dir> --models <dir> [--split train] [--errors mssd mspd]
                                    [--translation_scale 1] [--vsd] [--out <dir>]

The results file has the header and rows ``scene_id,im_id,obj_id,score,R,t,time`` (R nine numbers, t three, separated by
spaces, t in millimetres).  Per scene every estimate is compared with every ground-truth instance of its object in its image,
one batched call per error type; ``errors_<type>.json`` is written per scene in the toolkit's layout, and the average
recalls over the BOP19 thresholds are printed.  A ground-truth instance is valid when its visib_fract is at least 0.1; per
(image, object) as many top-scored estimates count as there are valid instances.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import bop_dataset as BD, pose_error as PE

VISIB_GT_MIN = 0.1
VSD_DELTA = 15.0
VSD_TAUS = tuple(round(0.05 * k, 2) for k in range(1, 11))
VSD_THRESHOLDS = tuple(round(0.05 * k, 2) for k in range(1, 11))


def read_results(path) -> list:
    """The estimates of a BOP results file: [{'scene_id', 'im_id', 'obj_id', 'score', 'R' [3,3], 't' [3], 'time'}]."""
    ests = []
    lines = Path(path).read_text().splitlines()
    for n, line in enumerate(lines):
        if n == 0 and line.replace(" ", "").startswith("scene_id,im_id,obj_id,score,R,t,time"):
            continue
        if not line.strip():
            continue
        f = line.split(",")
        if len(f) != 7:
            raise ValueError(f"{path}:{n + 1}: 7 comma-separated fields expected, got {len(f)}")
        R = np.array(f[4].split(), np.float64)
        t = np.array(f[5].split(), np.float64)
        if R.size != 9 or t.size != 3:
            raise ValueError(f"{path}:{n + 1}: R needs 9 numbers and t 3")
        ests.append(dict(scene_id=int(f[0]), im_id=int(f[1]), obj_id=int(f[2]), score=float(f[3]), R=R.reshape(3, 3), t=t,
                         time=float(f[6])))
    return ests


def write_results(path, ests: Sequence[dict]) -> None:
    """The inverse of read_results."""
    rows = ["scene_id,im_id,obj_id,score,R,t,time"]
    for e in ests:
        R = " ".join(repr(float(x)) for x in np.asarray(e["R"], np.float64).reshape(9))
        t = " ".join(repr(float(x)) for x in np.asarray(e["t"], np.float64).reshape(3))
        rows.append(f"{e['scene_id']},{e['im_id']},{e['obj_id']},{float(e['score'])!r},{R},{t},{float(e.get('time', -1))!r}")
    Path(path).write_text("\n".join(rows) + "\n")


def save_errors(path, errs: Sequence[dict]) -> None:
    """errors_<type>.json in the toolkit's layout: a list of {im_id, obj_id, est_id, score, errors: {gt_id: [e, ...]}}."""
    rows = [dict(im_id=e["im_id"], obj_id=e["obj_id"], est_id=e["est_id"], score=e["score"],
                 errors={str(g): [float(x) for x in v] for g, v in e["errors"].items()}) for e in errs]
    Path(path).write_text(json.dumps(rows))


def load_errors(path) -> list:
    """The inverse of save_errors: the ground-truth ids are ints again."""
    rows = json.loads(Path(path).read_text())
    for e in rows:
        e["errors"] = {int(g): v for g, v in e["errors"].items()}
    return rows


def scene_pairs(ests: Sequence[dict], scene_gt: dict, unit: float):
    """Every (estimate, ground-truth instance of its object in its image) pair of one scene.  Returns (errs, index, arrays):
    ``errs`` the error records with est_id counted per (image, object) in file order, ``index`` [(record, gt_id)] per pair,
    ``arrays`` (obj_ids, R_est, t_est, R_gt, t_gt, im_ids) with the estimates' millimetres brought to the dataset's unit."""
    errs, index, cols = [], [], ([], [], [], [], [], [])
    counts = {}
    for e in ests:
        key = (e["im_id"], e["obj_id"])
        est_id = counts.get(key, 0)
        counts[key] = est_id + 1
        rec = dict(im_id=e["im_id"], obj_id=e["obj_id"], est_id=est_id, score=e["score"], errors={})
        errs.append(rec)
        for gt_id, gt in enumerate(scene_gt.get(str(e["im_id"]), [])):
            if int(gt["obj_id"]) != e["obj_id"]:
                continue
            index.append((len(errs) - 1, gt_id))
            for c, v in zip(cols, (e["obj_id"], e["R"], e["t"] * unit, *BD.pose_of(gt), e["im_id"])):
                c.append(v)
    return errs, index, cols


def evaluate(results, dataset, models_dir, split: str = "train", errors: Sequence[str] = ("mssd", "mspd"),
             translation_scale: float = 1.0, vsd: bool = False, out: Optional[str] = None, device="cuda",
             width: Optional[int] = None) -> dict:
    """The average recalls {'AR_MSSD', 'AR_MSPD', ('AR_VSD',) 'AR'} of a results file; see the module's text."""
    unit = BD.unit_of(translation_scale)
    models = PE.PoseErrorModels.from_dir(models_dir, device=device, scale=unit)
    ests = read_results(results)
    types = list(errors) + (["vsd"] if vsd else [])
    scene_ids = sorted({e["scene_id"] for e in ests})
    obj_ids = sorted(models.ranges)
    per_type = {t: {} for t in types}                 # type -> scene -> error records (normalised for the thresholds)
    gts, valid, n_tops = {}, {}, {}
    for sid in scene_ids:
        scene = BD.BopScene(BD.scene_dir(dataset, split, sid))
        scene_gt, cam, info = scene.gt, scene.camera, scene.read_json(BD.SCENE_GT_INFO)
        w = width or (scene.first_image_size() or (0, 0))[0] or 640          # MSPD is normalised to 640 px wide images
        gts[sid] = {int(i): [{"obj_id": int(g["obj_id"])} for g in v] for i, v in scene_gt.items()}
        valid[sid] = {int(i): [float(g["visib_fract"]) >= VISIB_GT_MIN for g in v] for i, v in info.items()}
        n_tops[sid] = {}
        for i, v in gts[sid].items():
            for g, gt in enumerate(v):
                key = (i, gt["obj_id"])
                n_tops[sid][key] = n_tops[sid].get(key, 0) + int(valid[sid][i][g])
        mine = [e for e in ests if e["scene_id"] == sid]
        errs, index, (objs, R_est, t_est, R_gt, t_gt, ims) = scene_pairs(mine, scene_gt, unit)
        values = {}
        plain = [t for t in types if t != "vsd"]
        if index and plain:
            K = np.stack([BD.cam_K(cam[str(i)]) for i in ims])
            values = PE.pose_errors(models, objs, np.stack(R_est), np.stack(t_est), np.stack(R_gt), np.stack(t_gt), K, plain)
        if index and vsd:
            values["vsd"] = _vsd_errors(models, scene, objs, R_est, t_est, R_gt, t_gt, ims, unit)
        for t in types:
            recs = [dict(e, errors={}) for e in errs]
            normed = [dict(e, errors={}) for e in errs]
            for p, (r, gt_id) in enumerate(index):
                v = np.atleast_1d(values[t][p]).astype(np.float64)
                if t in ("mssd", "add", "adi"):
                    written = v / unit                                   # millimetres, as the toolkit writes them
                    norm = v / models.diameters[objs[p]]
                elif t in ("mspd", "proj"):
                    written, norm = v, v * (640.0 / w)
                else:
                    written = norm = v
                recs[r]["errors"][gt_id] = written.tolist()
                normed[r]["errors"][gt_id] = norm.tolist()
            if out:
                d = Path(out) / BD.scene_name(sid)
                d.mkdir(parents=True, exist_ok=True)
                save_errors(d / f"errors_{t}.json", recs)
            per_type[t][sid] = normed
    scores = {}
    for t in types:
        recalls = []
        if t == "vsd":
            for k in range(len(VSD_TAUS)):
                for th in VSD_THRESHOLDS:
                    recalls.append(_recall(scene_ids, obj_ids, gts, valid, n_tops, per_type[t], th, element=k))
        else:
            ths = PE.MSPD_THRESHOLDS if t in ("mspd", "proj") else PE.MSSD_THRESHOLDS
            for th in ths:
                recalls.append(_recall(scene_ids, obj_ids, gts, valid, n_tops, per_type[t], th))
        scores[f"AR_{t.upper()}"] = float(np.mean(recalls)) if recalls else 0.0
    scores["AR"] = float(np.mean(list(scores.values()))) if scores else 0.0
    return scores


def _recall(scene_ids, obj_ids, gts, valid, n_tops, errs_by_scene, th, element: Optional[int] = None) -> float:
    matches = []
    for sid in scene_ids:
        errs = errs_by_scene[sid]
        if element is not None:
            errs = [dict(e, errors={g: [v[element]] for g, v in e["errors"].items()}) for e in errs]
        matches += PE.match_scene(sid, gts[sid], valid[sid], errs, [th], n_tops[sid])
    return PE.localization_recall(scene_ids, obj_ids, matches, n_top=-1)["recall"]


def _vsd_errors(models, scene: BD.BopScene, objs, R_est, t_est, R_gt, t_gt, ims, unit):
    """VSD of every pair through mesh_render.vsd (normalised by the diameter, one value per tau), pairs of one ground truth
    in one call."""
    from .mesh_render import vsd
    if models.meshes is None:
        raise ValueError("VSD needs models with faces (PoseErrorModels.from_dir)")
    out = np.zeros((len(objs), len(VSD_TAUS)))
    groups = {}
    for p in range(len(objs)):
        groups.setdefault((ims[p], objs[p], R_gt[p].tobytes(), t_gt[p].tobytes()), []).append(p)
    depth_of = {}
    for (im, obj, _, _), ps in groups.items():
        cam = scene.camera[str(im)]
        if im not in depth_of:
            depth_of[im] = scene.read_png("depth", im).astype(np.float32) * np.float32(BD.depth_unit(cam, unit))
        e = vsd(np.stack([R_est[p] for p in ps]), np.stack([t_est[p] for p in ps]), R_gt[ps[0]], t_gt[ps[0]], depth_of[im],
                BD.cam_K(cam), VSD_DELTA * unit, list(VSD_TAUS), True, models.diameters[obj], models.meshes, obj)
        out[ps] = e.cpu().numpy()
    return out


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.pose_eval", description=__doc__.split("\n\n")[0])
    p.add_argument("--results", required=True, help="BOP results file: scene_id,im_id,obj_id,score,R,t,time")
    p.add_argument("--dataset", required=True)
    p.add_argument("--models", required=True, help="obj_NNNNNN.ply and models_info.json, in millimetres")
    p.add_argument("--split", default="train")
    p.add_argument("--errors", nargs="+", default=["mssd", "mspd"], choices=["mssd", "mspd", "add", "adi", "proj"])
    p.add_argument("--translation_scale", type=float, default=1.0,
                   help="what scene_gt's translations were written with: 1 = metres, 1000 = millimetres")
    p.add_argument("--vsd", action="store_true", help="also AR_VSD, from the depth images")
    p.add_argument("--out", default=None, help="where errors_<type>.json are written, per scene")
    a = p.parse_args(argv)
    scores = evaluate(a.results, a.dataset, a.models, a.split, a.errors, a.translation_scale, a.vsd, a.out)
    for k, v in scores.items():
        print(f"{k}: {v:.4f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
