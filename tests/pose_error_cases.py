"""Inputs of the pose-error tests (tests/test_pose_error_host.py, tests/test_pose_error_gpu.py) and of the golden generator
(tests/golden/make_golden_pose_errors.py): model points in millimetres, symmetry entries as models_info.json holds them, and
(estimate, ground truth) pairs 400-1500 mm in front of the camera.  Everything is seeded."""
import numpy as np

K_SHARED = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
KINDS = ("equal", "symmetric", "small", "medium", "flip", "far")


def rotation(axis, angle):
    d = np.asarray(axis, np.float64)
    d = d / np.linalg.norm(d)
    k = np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * k.dot(k)


def points(n, seed, radii=(60.0, 35.0, 90.0)):
    """float32 [n,3]: a lumpy ellipsoid about (3, -2, 5) mm, no symmetry of its own."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * np.asarray(radii) * rng.uniform(0.6, 1.0, (n, 1)) + np.array([3.0, -2.0, 5.0])
    return p.astype(np.float32)


def diameter(pts):
    p = np.asarray(pts, np.float64)
    return float(np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1).max())) if len(p) > 1 else 1.0


def _m4(R, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m.reshape(16).tolist()


# exact entries (half turns and a quarter turn), with translations so that t matters
DISCRETE = [_m4(np.diag([1.0, -1.0, -1.0]), [0.0, 4.0, -2.0]), _m4(np.diag([-1.0, 1.0, -1.0]), [1.5, 0.0, 3.0]),
            _m4(np.diag([-1.0, -1.0, 1.0]), [-2.0, 1.0, 0.0]), _m4(np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), [0.5, 0.5, 0.0])]


def model_info(n_discrete=0, continuous=None):
    """A models_info entry with the first ``n_discrete`` DISCRETE symmetries and the continuous ones given as
    [(axis, offset), ...]."""
    info = {"diameter": 180.0}
    if n_discrete:
        info["symmetries_discrete"] = [list(m) for m in DISCRETE[:n_discrete]]
    if continuous:
        info["symmetries_continuous"] = [{"axis": list(a), "offset": list(o)} for a, o in continuous]
    return info


AXIS = ((0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
AXIS_OFFSET = ((1.0, 2.0, 2.0), (4.0, -3.0, 6.0))        # not normalised, off the origin

# the golden's symmetry sets: name -> (models_info entry, max_sym_disc_step)
GOLDEN_SETS = {
    "none": (model_info(), 0.01),
    "one_discrete": (model_info(1), 0.01),
    "three_discrete": (model_info(3), 0.01),
    "continuous_offset": (model_info(0, [AXIS_OFFSET]), 0.01),            # 315 rotations
    "continuous_coarse": (model_info(0, [AXIS]), 0.25),                   # 13
    "discrete_x_continuous": (model_info(1, [AXIS_OFFSET]), 0.01),        # 2 x 315 = 630
}


def info_with_count(s):
    """A models_info entry (at max_sym_disc_step 0.01) with exactly ``s`` transforms, for s in 1..5 and 630."""
    return GOLDEN_SETS["discrete_x_continuous"][0] if s == 630 else model_info(s - 1)


def make_pairs(n, seed, sym_R, sym_t, diam, kinds=KINDS):
    """n pairs cycling through ``kinds``: (R_est, t_est, R_gt, t_gt, kind names).  'symmetric' composes the ground truth with
    the symmetry that turns the farthest from the identity (and falls back to 'small' when there is only the identity)."""
    rng = np.random.default_rng(seed)
    far_sym = int(np.argmin(np.trace(sym_R, axis1=1, axis2=2)))
    R_est, t_est, R_gt, t_gt, names = [], [], [], [], []
    for k in range(n):
        kind = kinds[k % len(kinds)]
        if kind == "symmetric" and len(sym_R) == 1:
            kind = "small"
        Rg = rotation(rng.normal(size=3), rng.uniform(0, np.pi))
        tg = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(520, 1380)])
        if kind == "equal":
            Re, te = Rg.copy(), tg.copy()
        elif kind == "symmetric":
            Re, te = Rg.dot(sym_R[far_sym]), Rg.dot(sym_t[far_sym]) + tg
        elif kind == "small":
            Re, te = rotation(rng.normal(size=3), rng.uniform(0, 0.05)).dot(Rg), tg + rng.normal(0, 1.5, 3)
        elif kind == "medium":
            Re, te = rotation(rng.normal(size=3), rng.uniform(0.1, 0.6)).dot(Rg), tg + rng.normal(0, 10.0, 3)
        elif kind == "flip":
            Re, te = rotation(rng.normal(size=3), np.pi).dot(Rg), tg + rng.normal(0, 1.0, 3)
        else:                                                             # farther than the diameter
            Re, te = rotation(rng.normal(size=3), rng.uniform(0, 0.3)).dot(Rg), tg + np.array([1.2 * diam, -0.8 * diam, 60.0])
        R_est.append(Re); t_est.append(te); R_gt.append(Rg); t_gt.append(tg); names.append(kind)
    return np.stack(R_est), np.stack(t_est), np.stack(R_gt), np.stack(t_gt), names


def per_pair_K(n, seed):
    rng = np.random.default_rng(seed)
    K = np.tile(K_SHARED, (n, 1, 1))
    K[:, 0, 0] *= rng.uniform(0.8, 1.3, n)
    K[:, 1, 1] *= rng.uniform(0.8, 1.3, n)
    K[:, 0, 2] += rng.uniform(-30, 30, n)
    K[:, 1, 2] += rng.uniform(-30, 30, n)
    return K


# ---- the GPU tests' calls -------------------------------------------------------------------------------------------
V_SWEEP = (1, 63, 64, 65, 255, 256, 257, 1000)      # one lane, the wave edge, the workgroup / LDS-tile edge, several tiles


def s_sweep(chunk):
    return (1, 2, chunk - 1, chunk, chunk + 1, 630)


def _call(name, objects, order, seed, K):
    """objects: {obj_id: (pts, models_info entry)}; order: the object of every job.  Pairs cycle through KINDS per object."""
    from pegasus_amd.pose_error import symmetry_transformations
    order = np.asarray(order)
    P = len(order)
    out = dict(name=name, objects=objects, obj_ids=order, R_est=np.empty((P, 3, 3)), t_est=np.empty((P, 3)),
               R_gt=np.empty((P, 3, 3)), t_gt=np.empty((P, 3)), kinds=np.empty(P, dtype="U12"), K=K, syms={}, diameters={})
    for n, (o, (pts, info)) in enumerate(sorted(objects.items())):
        sym_R, sym_t = symmetry_transformations(info, 0.01)
        out["syms"][o], out["diameters"][o] = (sym_R, sym_t), diameter(pts)
        sel = np.nonzero(order == o)[0]
        Re, te, Rg, tg, kinds = make_pairs(len(sel), seed + n, sym_R, sym_t, out["diameters"][o])
        out["R_est"][sel], out["t_est"][sel], out["R_gt"][sel], out["t_gt"][sel], out["kinds"][sel] = Re, te, Rg, tg, kinds
    return out


def gpu_calls(chunk):
    """The three calls of tests/test_pose_error_gpu.py: a sweep over V, a sweep over S, and 257 jobs interleaved over three
    objects of different V and S with one K per pair."""
    calls = []
    objects = {10 + k: (points(v, 20 + k), info_with_count(5)) for k, v in enumerate(V_SWEEP)}
    calls.append(_call("v_sweep", objects, np.repeat(sorted(objects), len(KINDS)), 300, K_SHARED))
    objects = {10 + k: (points(257, 40 + k), info_with_count(s)) for k, s in enumerate(s_sweep(chunk))}
    calls.append(_call("s_sweep", objects, np.repeat(sorted(objects), len(KINDS)), 400, K_SHARED))
    objects = {1: (points(65, 60), info_with_count(630)), 2: (points(1000, 61), info_with_count(5)),
               3: (points(256, 62), info_with_count(2))}
    order = [2 if k % 16 == 7 else (1, 3)[k % 2] for k in range(257)]
    calls.append(_call("interleaved", objects, order, 500, per_pair_K(257, 501)))
    return calls


def subset(call, n):
    """The first n jobs of a call."""
    out = dict(call, name=f"{call['name']}[:{n}]")
    for k in ("obj_ids", "R_est", "t_est", "R_gt", "t_gt", "kinds"):
        out[k] = call[k][:n]
    if np.ndim(call["K"]) == 3:
        out["K"] = call["K"][:n]
    return out


# ---- a small dataset on disk for pegasus_amd.pose_eval ----------------------------------------------------------------
def make_eval_dataset(root):
    """Two objects (millimetre models, object 2 with a half-turn symmetry), one scene of two 640-wide images written in
    metres (translation_scale 1), and a results file: per ground truth a good estimate, for object 1 in image 0 also a bad one
    with the higher score, and for the symmetric object an estimate composed with its symmetry.  Returns the paths and the
    pieces a test needs to restate the errors."""
    import json
    from pathlib import Path
    from pegasus_amd.ply_io import write_ply_mesh
    root = Path(root)
    models = root / "models"
    scene = root / "data" / "train" / "000003"
    models.mkdir(parents=True)
    scene.mkdir(parents=True)
    pts = {1: points(300, 70), 2: points(200, 71)}
    infos = {1: dict(model_info(0), diameter=diameter(pts[1])), 2: dict(model_info(1), diameter=diameter(pts[2]))}
    for o, p in pts.items():
        write_ply_mesh(models / f"obj_{o:06d}.ply", p, np.array([[0, 1, 2]], np.int32))
    (models / "models_info.json").write_text(json.dumps({str(o): i for o, i in infos.items()}))
    rng = np.random.default_rng(72)
    gt, cam, info, rows = {}, {}, {}, []
    sym = np.asarray(DISCRETE[0]).reshape(4, 4)
    for im in (0, 1):
        gt[str(im)], info[str(im)] = [], []
        cam[str(im)] = dict(cam_K=K_SHARED.reshape(9).tolist(), depth_scale=1.0)
        for g, (o, visib) in enumerate(((1, 0.9), (2, 0.8), (1, 0.05)) if im == 0 else ((2, 0.7),)):
            R = rotation(rng.normal(size=3), rng.uniform(0, np.pi))
            t = np.array([rng.uniform(-100, 100), rng.uniform(-80, 80), rng.uniform(600, 1200)])       # millimetres
            gt[str(im)].append(dict(obj_id=o, cam_R_m2c=R.reshape(9).tolist(), cam_t_m2c=(t * 0.001).tolist()))
            info[str(im)].append(dict(visib_fract=visib))
            if o == 2:                                                        # the pose seen through the symmetry
                rows.append(dict(scene_id=3, im_id=im, obj_id=o, score=0.9, R=R.dot(sym[:3, :3]), t=R.dot(sym[:3, 3]) + t, time=-1))
            elif g == 0:
                rows.append(dict(scene_id=3, im_id=im, obj_id=o, score=0.9, R=rotation((1, 0, 0), 1.0).dot(R), t=t + 40.0, time=-1))
                rows.append(dict(scene_id=3, im_id=im, obj_id=o, score=0.6, R=rotation((0, 1, 0), 0.01).dot(R), t=t + 0.5, time=-1))
    from pegasus_amd.dataset_writer import encode_png
    (scene / "depth").mkdir()
    for im in (0, 1):                                                         # a wall 2 m away, behind every object
        (scene / "depth" / f"{im:06d}.png").write_bytes(encode_png(np.full((480, 640), 2000, np.uint16)))
    (scene / "scene_gt.json").write_text(json.dumps(gt))
    (scene / "scene_camera.json").write_text(json.dumps(cam))
    (scene / "scene_gt_info.json").write_text(json.dumps(info))
    return dict(models=models, dataset=root / "data", scene=scene, pts=pts, infos=infos, rows=rows, gt=gt)
