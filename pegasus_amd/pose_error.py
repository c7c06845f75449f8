"""The BOP pose errors on the GPU: MSSD, MSPD, ADD, ADI (ADD-S), proj, re and te with the object symmetries they rest on
(the toolkit's bop_toolkit_lib/pose_error.py and misc.get_symmetry_transformations), and the matching and recall of its
pose_matching.py / score.py.

``pgr_pose_errors`` computes mssd, mspd, add, proj, re and te of a batch of (estimate, ground truth) pairs in one call,
``pgr_pose_adi`` ADI by exact brute-force nearest neighbour; both are pinned in pegasus_amd/csrc/poseerr.hip.h.  The model
points are the vertices a ``mesh_render.MeshSet`` holds on the device, the symmetry sets come from ``models_info.json``:

    models = PoseErrorModels.from_dir("<dataset>/models")                      # millimetres
    e = pose_errors(models, obj_ids, R_est, t_est, R_gt, t_gt, K, errors=("mssd", "mspd", "adi"))

``python -m pegasus_amd.pose_eval`` evaluates a BOP results file with them.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .bop_dataset import read_models_info
from .bop_pose import broadcast_K
from .mesh_render import MeshSet

ERROR_NAMES = ("mssd", "mspd", "add", "adi", "proj", "re", "te")
SYM_CHUNK = _lib.PGR_POSE_SYM_CHUNK          # symmetries of a job that share one workgroup
MAX_JOBS_PER_CALL = 1 << 18                  # 240 B each: 60 MiB of host job array per library call
_COLUMN = {"mssd": 0, "mspd": 1, "add": 2, "proj": 3}

# the host layout of PgrPoseErrorJob (include/pegasus_raster.h), filled with array operations
JOB_DTYPE = np.dtype([("vertex_first", "<i4"), ("vertex_count", "<i4"), ("sym_first", "<i4"), ("sym_count", "<i4"),
                      ("R_est", "<f8", (9,)), ("t_est", "<f8", (3,)), ("R_gt", "<f8", (9,)), ("t_gt", "<f8", (3,)),
                      ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8")])
assert JOB_DTYPE.itemsize == C.sizeof(_lib.PgrPoseErrorJob)


# ---- symmetries -----------------------------------------------------------------------------------------------------
def _axis_rotation(angle: float, axis) -> np.ndarray:
    """Rodrigues' formula about the normalised axis: cos I + (1 - cos) d d^T + sin [d]x."""
    d = np.asarray(axis, np.float64).reshape(3)
    d = d / math.sqrt(float(np.dot(d, d)))
    s, c = math.sin(angle), math.cos(angle)
    R = np.diag([c, c, c]) + np.outer(d, d) * (1.0 - c)
    d = d * s
    return R + np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])


def symmetry_transformations(model_info: dict, max_sym_disc_step: float = 0.01):
    """The symmetry transformations of a ``models_info.json`` entry, as misc.get_symmetry_transformations lists them: float64
    (R [S,3,3], t [S,3]), the identity first, the discrete symmetries outermost, each continuous axis discretised into
    ceil(pi / max_sym_disc_step) rotations with t = -R offset + offset, and every discrete transform composed with every
    rotation (rotation after discrete)."""
    disc = [(np.eye(3), np.zeros(3))]
    for sym in model_info.get("symmetries_discrete", None) or []:
        m = np.asarray(sym, np.float64).reshape(4, 4)
        disc.append((m[:3, :3], m[:3, 3]))
    cont = []
    for sym in model_info.get("symmetries_continuous", None) or []:
        offset = np.asarray(sym["offset"], np.float64).reshape(3)
        steps = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / steps
        for i in range(steps):
            R = _axis_rotation(i * step, sym["axis"])
            cont.append((R, -R.dot(offset) + offset))
    if cont:
        pairs = [(Rc.dot(Rd), Rc.dot(td) + tc) for Rd, td in disc for Rc, tc in cont]
    else:
        pairs = disc
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def scaled_model_info(info: dict, scale: float) -> dict:
    """A models_info entry with its lengths (diameter, box, symmetry translations and offsets) multiplied by ``scale``."""
    out = dict(info)
    for k in ("diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z"):
        if k in out:
            out[k] = out[k] * scale
    if info.get("symmetries_discrete"):
        ms = []
        for sym in info["symmetries_discrete"]:
            m = np.asarray(sym, np.float64).reshape(4, 4).copy()
            m[:3, 3] *= scale
            ms.append(m.reshape(16).tolist())
        out["symmetries_discrete"] = ms
    if info.get("symmetries_continuous"):
        out["symmetries_continuous"] = [{"axis": list(s["axis"]), "offset": [float(o) * scale for o in s["offset"]]}
                                        for s in info["symmetries_continuous"]]
    return out


class PoseErrorModels:
    """What the pose errors need of every object, uploaded once: the vertices of a ``MeshSet`` and the objects' symmetry sets,
    ``syms`` float64 [S,12] (R row-major, then t) shared by all with ``sym_ranges[obj_id] = (sym_first, sym_count)``.
    ``models_info``: {obj_id: models_info.json entry} in the meshes' units; an object without an entry has the identity."""

    def __init__(self, meshes: MeshSet, models_info: Optional[dict] = None, max_sym_disc_step: float = 0.01):
        info = {int(k): v for k, v in (models_info or {}).items()}
        sets = {o: symmetry_transformations(info.get(o, {}), max_sym_disc_step) for o in sorted(meshes.ranges)}
        self._take(meshes.vertices, {o: r[:2] for o, r in meshes.ranges.items()}, sets)
        self.meshes = meshes
        self.diameters = dict(meshes.diameters)
        for o, e in info.items():
            if "diameter" in e:
                self.diameters.setdefault(o, float(e["diameter"]))

    def _take(self, vertices, ranges, sets):
        import torch
        self.vertices, self.ranges, self.device = vertices, ranges, vertices.device
        self.sym_ranges, rows, s0 = {}, [], 0
        for o in sorted(sets):
            R, t = sets[o]
            self.sym_ranges[o] = (s0, len(R))
            rows.append(np.concatenate([R.reshape(-1, 9), t.reshape(-1, 3)], axis=1))
            s0 += len(R)
        self.syms_host = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 12)), np.float64)
        self.syms = torch.from_numpy(self.syms_host).to(self.device)

    @classmethod
    def from_dir(cls, models_dir, device="cuda", scale: float = 1.0, max_sym_disc_step: float = 0.01) -> "PoseErrorModels":
        """The ``obj_NNNNNN.ply`` files and ``models_info.json`` of a BOP models directory; ``scale`` multiplies the vertices,
        the diameters and the symmetries' translations and offsets alike (0.001: millimetres to metres)."""
        meshes = MeshSet.from_dir(models_dir, device=device, scale=scale)
        info = read_models_info(models_dir)
        return cls(meshes, {int(k): scaled_model_info(v, scale) for k, v in info.items()}, max_sym_disc_step)

    @classmethod
    def from_points(cls, pts, syms: Optional[Sequence[dict]] = None, device="cuda", obj_id: int = 0) -> "PoseErrorModels":
        """One object from the toolkit's own arguments: ``pts`` [n,3] and ``syms`` a list of {'R': [3,3], 't': [3,1]}
        (None: the identity)."""
        import torch
        self = cls.__new__(cls)
        v = np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 3), np.float32)
        if syms is None:
            R, t = np.eye(3)[None], np.zeros((1, 3))
        else:
            R = np.stack([np.asarray(s["R"], np.float64).reshape(3, 3) for s in syms])
            t = np.stack([np.asarray(s["t"], np.float64).reshape(3) for s in syms])
        self._take(torch.from_numpy(v).to(device), {int(obj_id): (0, len(v))}, {int(obj_id): (R, t)})
        self.meshes, self.diameters = None, {}
        return self

    def symmetries(self, obj_id: int):
        """(R [S,3,3], t [S,3]) of one object as host arrays."""
        s0, ns = self.sym_ranges[int(obj_id)]
        rows = self.syms_host[s0:s0 + ns]
        return rows[:, :9].reshape(-1, 3, 3), rows[:, 9:]


# ---- the batched call -----------------------------------------------------------------------------------------------
def intrinsics(K, n: int) -> np.ndarray:
    """(fx, fy, cx, cy) float64 [n,4] of ``K`` [3,3] or [n,3,3]; a K with skew is refused."""
    K = broadcast_K(K, n)
    if np.any(K[:, 0, 1] != 0.0) or np.any(K[:, 1, 0] != 0.0) or np.any(K[:, 2, :2] != 0.0):
        raise ValueError("K with skew (or a third row other than 0 0 1) is not supported")
    return np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1)


def pose_jobs(models: PoseErrorModels, obj_ids, R_est, t_est, R_gt, t_gt, K=None) -> np.ndarray:
    """The PgrPoseErrorJob array (a structured NumPy array of JOB_DTYPE) of P pairs."""
    obj_ids = np.asarray(obj_ids, np.int64).reshape(-1)
    P = len(obj_ids)
    jobs = np.zeros(P, JOB_DTYPE)
    for name, a, shape in (("R_est", R_est, (P, 9)), ("t_est", t_est, (P, 3)), ("R_gt", R_gt, (P, 9)), ("t_gt", t_gt, (P, 3))):
        a = np.asarray(a, np.float64)
        if a.size != P * shape[1]:
            raise ValueError(f"{name}: {P} pairs need {P * shape[1]} numbers, got {a.size}")
        jobs[name] = a.reshape(shape)
    for o in np.unique(obj_ids):
        if int(o) not in models.ranges:
            raise KeyError(f"object {int(o)} is not in the models")
        sel = obj_ids == o
        jobs["vertex_first"][sel], jobs["vertex_count"][sel] = models.ranges[int(o)]
        jobs["sym_first"][sel], jobs["sym_count"][sel] = models.sym_ranges[int(o)]
    k = intrinsics(K, P) if K is not None else np.broadcast_to(np.array([1.0, 1.0, 0.0, 0.0]), (P, 4))
    jobs["fx"], jobs["fy"], jobs["cx"], jobs["cy"] = k[:, 0], k[:, 1], k[:, 2], k[:, 3]
    return jobs


def _job_ptr(jobs: np.ndarray):
    return jobs.ctypes.data_as(C.POINTER(_lib.PgrPoseErrorJob))


def pose_errors(models: PoseErrorModels, obj_ids, R_est, t_est, R_gt, t_gt, K=None, errors: Sequence[str] = ("mssd", "mspd")):
    """The errors named in ``errors`` (out of mssd, mspd, add, adi, proj, re, te) of P (estimate, ground truth) pairs:
    ``obj_ids`` [P], ``R_*`` [P,3,3], ``t_*`` [P,3] model to camera in the models' units, ``K`` [3,3] or [P,3,3] (needed by mspd
    and proj).  Returns {name: float64 [P]}; re in degrees.  One pgr_pose_errors call, plus one pgr_pose_adi call for adi."""
    import torch
    errors = tuple(errors)
    for name in errors:
        if name not in ERROR_NAMES:
            raise ValueError(f"unknown error {name!r}: one of {', '.join(ERROR_NAMES)}")
    if K is None and ("mspd" in errors or "proj" in errors):
        raise ValueError("mspd and proj need the camera matrix K")
    jobs = pose_jobs(models, obj_ids, R_est, t_est, R_gt, t_gt, K)
    P = len(jobs)
    dev = models.device
    if dev.type != "cuda":
        raise RuntimeError("pose_errors needs models on a HIP device; there is no CPU path")
    out = torch.empty((P, _lib.PGR_POSE_ERRORS), dtype=torch.float32, device=dev)
    re_te = torch.empty((P, 2), dtype=torch.float64, device=dev)
    adi = torch.empty(P, dtype=torch.float32, device=dev) if "adi" in errors else None
    main = any(n != "adi" for n in errors)
    for j0 in range(0, P, MAX_JOBS_PER_CALL):
        part = jobs[j0:j0 + MAX_JOBS_PER_CALL]
        n = len(part)
        if main:
            _lib.call("pgr_pose_errors", dev, _lib.ptr(models.vertices), models.vertices.shape[0], _lib.ptr(models.syms),
                      models.syms.shape[0], n, _job_ptr(part), _lib.ptr(out[j0:j0 + n]), _lib.ptr(re_te[j0:j0 + n]))
        if adi is not None:
            ws = _lib.workspace("pgr_pose_adi", dev, n, _job_ptr(part))
            _lib.call("pgr_pose_adi", dev, _lib.ptr(models.vertices), models.vertices.shape[0], n, _job_ptr(part),
                      _lib.ptr(adi[j0:j0 + n]), _lib.ptr(ws), ws.numel())
    res = {}
    host = out.cpu().numpy().astype(np.float64) if main else None
    host64 = re_te.cpu().numpy() if ("re" in errors or "te" in errors) else None
    for name in errors:
        if name == "adi":
            res[name] = adi.cpu().numpy().astype(np.float64)
        elif name in ("re", "te"):
            res[name] = host64[:, 0 if name == "re" else 1].copy()
        else:
            res[name] = host[:, _COLUMN[name]].copy()
    return res


# ---- the toolkit's scalar functions ---------------------------------------------------------------------------------
def _one(name, R_est, t_est, R_gt, t_gt, pts, syms=None, K=None, obj_id=None):
    if isinstance(pts, PoseErrorModels):
        models = pts
        obj = syms if (obj_id is None and name in ("mssd", "mspd")) else obj_id
        if obj is None:
            if len(models.ranges) != 1:
                raise ValueError("models hold several objects: name one with obj_id")
            obj = next(iter(models.ranges))
    else:
        models, obj = PoseErrorModels.from_points(pts, syms if name in ("mssd", "mspd") else None), 0
    e = pose_errors(models, [int(obj)], np.asarray(R_est, np.float64).reshape(1, 3, 3), np.asarray(t_est, np.float64).reshape(1, 3),
                    np.asarray(R_gt, np.float64).reshape(1, 3, 3), np.asarray(t_gt, np.float64).reshape(1, 3), K, (name,))
    return float(e[name][0])


def mssd(R_est, t_est, R_gt, t_gt, pts, syms):
    """Maximum Symmetry-Aware Surface Distance, pose_error.mssd.  ``pts`` [n,3] with ``syms`` a list of {'R', 't'}, or a
    PoseErrorModels with ``syms`` the object id."""
    return _one("mssd", R_est, t_est, R_gt, t_gt, pts, syms)


def mspd(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """Maximum Symmetry-Aware Projection Distance, pose_error.mspd (arguments as mssd, and the camera matrix)."""
    return _one("mspd", R_est, t_est, R_gt, t_gt, pts, syms, K=K)


def add(R_est, t_est, R_gt, t_gt, pts, obj_id=None):
    """Average Distance of Model Points, pose_error.add.  ``pts`` [n,3], or a PoseErrorModels with ``obj_id``."""
    return _one("add", R_est, t_est, R_gt, t_gt, pts, obj_id=obj_id)


def adi(R_est, t_est, R_gt, t_gt, pts, obj_id=None):
    """Average Distance of Model Points to the nearest neighbour (ADD-S), pose_error.adi."""
    return _one("adi", R_est, t_est, R_gt, t_gt, pts, obj_id=obj_id)


def proj(R_est, t_est, R_gt, t_gt, K, pts, obj_id=None):
    """Average distance of the projections of the model points in pixels, pose_error.proj."""
    return _one("proj", R_est, t_est, R_gt, t_gt, pts, K=K, obj_id=obj_id)


def re(R_est, R_gt):
    """Rotational error in degrees, pose_error.re, by the formula of pgr_pose_errors: acos of 0.5 (trace(R_est R_gt^T) - 1)
    clamped to [-1, 1].  Host float64; nine products need no device."""
    a, b = np.asarray(R_est, np.float64).reshape(3, 3), np.asarray(R_gt, np.float64).reshape(3, 3)
    trace = 0.0
    for i in range(3):
        trace += (a[i, 0] * b[i, 0] + a[i, 1] * b[i, 1]) + a[i, 2] * b[i, 2]
    return 180.0 * math.acos(min(1.0, max(-1.0, 0.5 * (float(trace) - 1.0)))) / math.pi


def te(t_est, t_gt):
    """Translational error, pose_error.te.  Host float64."""
    d = np.asarray(t_gt, np.float64).reshape(3) - np.asarray(t_est, np.float64).reshape(3)
    return math.sqrt(float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


# ---- matching and recall (host) -------------------------------------------------------------------------------------
def match_poses(errs: Sequence[dict], error_ths: Sequence[float], max_ests_count: int = 0, gt_valid_mask=None) -> list:
    """pose_matching.match_poses: estimates ({'est_id', 'score', 'errors': {gt_id: [e, ...]}}) are matched greedily to ground
    truths in the order of decreasing score (ties keep their order in ``errs``); an estimate takes the valid, still
    unmatched ground truth whose every error element is below the threshold and below the best so far.  Returns
    [{'est_id', 'gt_id', 'score', 'error', 'error_norm'}] for the matched estimates, in matching order."""
    ths = list(error_ths)
    ranked = sorted(errs, key=lambda e: e["score"], reverse=True)
    if max_ests_count > 0:
        ranked = ranked[:max_ests_count]
    taken, matches = set(), []
    for est in ranked:
        best_gt, best = -1, ths
        for gt_id, error in est["errors"].items():
            if gt_id in taken or (gt_valid_mask and not gt_valid_mask[gt_id]):
                continue
            if all(error[i] < best[i] for i in range(len(ths))):
                best_gt, best = gt_id, error
        if best_gt >= 0:
            taken.add(best_gt)
            matches.append({"est_id": est["est_id"], "gt_id": best_gt, "score": est["score"], "error": best,
                            "error_norm": [best[i] / float(ths[i]) for i in range(len(ths))]})
    return matches


def match_scene(scene_id, scene_gt: dict, scene_gt_valid: dict, scene_errs: Sequence[dict], correct_th, n_top) -> list:
    """pose_matching.match_poses_scene: one record per ground-truth instance of the scene ({'scene_id', 'im_id', 'obj_id',
    'gt_id', 'est_id', 'score', 'error', 'error_norm', 'valid'}, est_id -1 when unmatched).  ``scene_errs`` carry 'im_id' and
    'obj_id'; ``n_top``: an int, or {(im_id, obj_id): int}."""
    by_target = {}
    for e in scene_errs:
        by_target.setdefault((e["im_id"], e["obj_id"]), []).append(e)
    out = []
    for im_id, gts in scene_gt.items():
        rows = [{"scene_id": scene_id, "im_id": im_id, "obj_id": gt["obj_id"], "gt_id": g, "est_id": -1, "score": -1,
                 "error": -1, "error_norm": -1, "valid": scene_gt_valid[im_id][g]} for g, gt in enumerate(gts)]
        for obj_id in {gt["obj_id"] for gt in gts}:
            ests = by_target.get((im_id, obj_id))
            if not ests:
                continue
            top = n_top.get((im_id, obj_id), 0) if isinstance(n_top, dict) else n_top
            if isinstance(n_top, dict) and top <= 0:
                continue                         # no valid instance: nothing to match against
            for m in match_poses(ests, correct_th, top, scene_gt_valid[im_id]):
                rows[m["gt_id"]].update(est_id=m["est_id"], score=m["score"], error=m["error"], error_norm=m["error_norm"])
        out += rows
    return out


def localization_recall(scene_ids, obj_ids, matches: Sequence[dict], n_top: int) -> dict:
    """score.calc_localization_scores: recall overall, per object and per scene of ``matches`` (match_scene records).  The
    targets are the valid instances, at most ``n_top`` per (object, scene, image) when n_top > 0."""
    insts = {o: {s: {} for s in scene_ids} for o in obj_ids}
    for m in matches:
        if m["valid"]:
            d = insts[m["obj_id"]][m["scene_id"]]
            d[m["im_id"]] = d.get(m["im_id"], 0) + 1
    obj_tars, scene_tars = {o: 0 for o in obj_ids}, {s: 0 for s in scene_ids}
    tars = 0
    for o in obj_ids:
        for s in scene_ids:
            counts = insts[o][s].values()
            count = sum(min(n_top, c) for c in counts) if n_top > 0 else sum(counts)
            tars += count
            obj_tars[o] += count
            scene_tars[s] += count
    obj_tps, scene_tps = {o: 0 for o in obj_ids}, {s: 0 for s in scene_ids}
    tps = 0
    for m in matches:
        if m["valid"] and m["est_id"] != -1:
            tps += 1
            obj_tps[m["obj_id"]] += 1
            scene_tps[m["scene_id"]] += 1
    recall = lambda tp, n: tp / float(n) if n else 0.0
    obj_recalls = {o: recall(obj_tps[o], obj_tars[o]) for o in obj_ids}
    scene_recalls = {s: float(recall(scene_tps[s], scene_tars[s])) for s in scene_ids}
    return {"recall": float(recall(tps, tars)), "obj_recalls": obj_recalls,
            "mean_obj_recall": float(np.mean(list(obj_recalls.values()))), "scene_recalls": scene_recalls,
            "mean_scene_recall": float(np.mean(list(scene_recalls.values()))), "gt_count": len(matches),
            "targets_count": int(tars), "tp_count": int(tps)}


MSSD_THRESHOLDS = tuple(round(0.05 * k, 2) for k in range(1, 11))       # fractions of the object diameter (BOP19)
MSPD_THRESHOLDS = tuple(5.0 * k for k in range(1, 11))                  # pixels at an image width of 640 (BOP19)
