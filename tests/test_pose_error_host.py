"""pegasus_amd.pose_error without a GPU: the symmetry sets, the float64 restatement of the seven errors, matching and recall
against the toolkit's own outputs (tests/golden/bop_pose_errors.npz, made by tests/golden/make_golden_pose_errors.py), the
results file and errors_*.json, the entry points' argument checks, and models_info with symmetries."""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import pose_error_cases as PC            # noqa: E402
import pose_error_reference as PR        # noqa: E402

# re: the toolkit takes trace(R_est inv(R_gt)), the project trace(R_est R_gt^T).  For a rotation stored in float64 the two
# cosines differ by a few eps (at most ~8 eps = 1.8e-15: nine products and an inverse of a matrix with condition number 1);
# acos turns an error d of the cosine into at most sqrt(2 d) radians near 0 and 180 degrees: sqrt(3.6e-15) rad = 3.4e-6 deg.
RE_ABS_DEG = 3.4e-6


@pytest.fixture(scope="module")
def golden():
    return np.load(HERE / "golden" / "bop_pose_errors.npz")


def test_symmetry_transformations_equal_the_toolkit(golden):
    from pegasus_amd.pose_error import symmetry_transformations
    infos = json.loads(str(golden["model_infos"]))
    counts = {}
    for name in golden["set_names"]:
        R, t = symmetry_transformations(infos[name]["info"], infos[name]["step"])
        want_R, want_t = golden[f"sym_R_{name}"], golden[f"sym_t_{name}"]
        assert R.shape == want_R.shape and t.shape == want_t.shape and R.dtype == np.float64 and t.dtype == np.float64
        assert np.abs(R - want_R).max() <= 1e-12 and np.abs(t - want_t).max() <= 1e-12, name
        assert np.array_equal(R[0], np.eye(3)) and np.array_equal(t[0], np.zeros(3))
        counts[str(name)] = len(R)
    assert counts == dict(none=1, one_discrete=2, three_discrete=4, continuous_offset=315, continuous_coarse=13,
                          discrete_x_continuous=630)
    assert len(symmetry_transformations({}, 0.01)[0]) == 1
    assert len(symmetry_transformations(PC.info_with_count(5))[0]) == 5


def test_float64_restatement_equals_the_toolkit(golden):
    pts = golden["pts"].astype(np.float64)
    K = golden["K"]
    names = list(golden["set_names"])
    kinds = set()
    for k in range(len(golden["pair_set"])):
        name = names[int(golden["pair_set"][k])]
        args = (golden["R_est"][k], golden["t_est"][k], golden["R_gt"][k], golden["t_gt"][k])
        got = PR.errors_f64(pts, golden[f"sym_R_{name}"], golden[f"sym_t_{name}"], *args, K)
        got["adi"] = PR.adi_f64(pts, *args)
        kinds.add(str(golden["pair_kind"][k]))
        for e in ("mssd", "mspd", "add", "adi", "proj", "te", "re"):
            want = float(golden[f"err_{e}"][k])
            tol = 1e-9 * abs(want) + (RE_ABS_DEG if e == "re" else 0.0)
            assert abs(got[e] - want) <= tol, (name, str(golden["pair_kind"][k]), e, got[e], want)
    assert kinds == set(PC.KINDS)


def test_float32_restatement_is_exactly_zero_for_a_perfect_estimate(golden):
    pts = golden["pts"]
    for k in np.nonzero(golden["pair_kind"] == "equal")[0]:
        name = list(golden["set_names"])[int(golden["pair_set"][k])]
        args = (golden["R_est"][k], golden["t_est"][k], golden["R_gt"][k], golden["t_gt"][k])
        got = PR.errors_f32(pts, golden[f"sym_R_{name}"], golden[f"sym_t_{name}"], *args, golden["K"])
        assert got["mssd"] == got["mspd"] == got["add"] == got["proj"] == 0.0
        assert PR.adi_f32(pts, *args) == 0.0


def _ints(d):
    return {int(k): v for k, v in d.items()}


def test_matching_and_recall_equal_the_toolkit(golden):
    from pegasus_amd.pose_error import localization_recall, match_poses, match_scene
    m = json.loads(str(golden["matching"]))
    scene_gt, scene_valid = _ints(m["scene_gt"]), _ints(m["scene_gt_valid"])
    errs = [dict(e, errors=_ints(e["errors"])) for e in m["errs"]]
    assert len(m["results"]) == 5
    for r in m["results"]:
        matches = match_scene(7, scene_gt, scene_valid, errs, [r["th"]], r["n_top"])
        assert matches == r["matches"]
        group = [e for e in errs if e["im_id"] == 0 and e["obj_id"] == 1]
        assert match_poses(group, [r["th"]], r["n_top"], scene_valid[0]) == r["plain"]
        scores = localization_recall([7], [1, 2, 3], matches, r["n_top"])
        want = {k: (_ints(v) if isinstance(v, dict) else v) for k, v in r["scores"].items()}
        assert scores == want
    # the tie in score keeps the order of the input, and an error at the threshold does not match
    first = match_poses(errs[:3], [0.1], 0, scene_valid[0])
    assert [(x["est_id"], x["gt_id"]) for x in first] == [(0, 1), (1, 0)]
    assert match_poses([errs[7]], [0.1]) == []


def test_bop19_thresholds():
    from pegasus_amd import pose_error as PE
    assert PE.MSSD_THRESHOLDS == (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5)
    assert PE.MSPD_THRESHOLDS == (5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 35.0, 40.0, 45.0, 50.0)


def test_results_file_and_errors_json_round_trip(tmp_path):
    from pegasus_amd import pose_eval
    rng = np.random.default_rng(3)
    ests = [dict(scene_id=2, im_id=k // 2, obj_id=1 + k % 2, score=float(rng.uniform()), R=PC.rotation(rng.normal(size=3), 1.0 + k),
                 t=rng.normal(0, 300, 3), time=0.25) for k in range(5)]
    path = tmp_path / "est_results.txt"
    pose_eval.write_results(path, ests)
    assert path.read_text().splitlines()[0] == "scene_id,im_id,obj_id,score,R,t,time"
    back = pose_eval.read_results(path)
    assert len(back) == 5
    for a, b in zip(ests, back):
        assert (a["scene_id"], a["im_id"], a["obj_id"], a["score"], a["time"]) == (b["scene_id"], b["im_id"], b["obj_id"], b["score"], b["time"])
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"])
    path.write_text("scene_id,im_id,obj_id,score,R,t,time\n1,2,3,0.5,1 0 0 0 1 0 0 0,0 0 1,-1\n")
    with pytest.raises(ValueError, match="9 numbers"):
        pose_eval.read_results(path)
    # pairs: every estimate against every instance of its object in its image, est_id per (image, object) in file order
    scene_gt = {"0": [dict(obj_id=1, cam_R_m2c=np.eye(3).reshape(9).tolist(), cam_t_m2c=[0, 0, 1.0]),
                      dict(obj_id=2, cam_R_m2c=np.eye(3).reshape(9).tolist(), cam_t_m2c=[0, 0, 2.0]),
                      dict(obj_id=1, cam_R_m2c=np.eye(3).reshape(9).tolist(), cam_t_m2c=[0, 0, 3.0])],
                "1": [dict(obj_id=2, cam_R_m2c=np.eye(3).reshape(9).tolist(), cam_t_m2c=[0, 0, 4.0])]}
    errs, index, (objs, R_est, t_est, R_gt, t_gt, ims) = pose_eval.scene_pairs(ests, scene_gt, 0.001)
    assert [(e["im_id"], e["obj_id"], e["est_id"]) for e in errs] == [(0, 1, 0), (0, 2, 0), (1, 1, 0), (1, 2, 0), (2, 1, 0)]
    assert index == [(0, 0), (0, 2), (1, 1), (3, 0)]
    assert objs == [1, 1, 2, 2] and [t[2] for t in t_gt] == [1.0, 3.0, 2.0, 4.0]
    assert np.allclose(t_est[0], ests[0]["t"] * 0.001)
    # errors_<type>.json: the toolkit's layout, ground-truth ids as JSON keys
    for (r, g), v in zip(index, (1.5, 2.5, 3.5, 4.5)):
        errs[r]["errors"][g] = [v]
    pose_eval.save_errors(tmp_path / "errors_mssd.json", errs)
    raw = json.loads((tmp_path / "errors_mssd.json").read_text())
    assert raw[0] == dict(im_id=0, obj_id=1, est_id=0, score=ests[0]["score"], errors={"0": [1.5], "2": [2.5]})
    assert set(raw[2]) == {"im_id", "obj_id", "est_id", "score", "errors"} and raw[2]["errors"] == {}
    assert pose_eval.load_errors(tmp_path / "errors_mssd.json") == errs


def _job(**kw):
    from pegasus_amd import _lib
    eye = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    base = dict(vertex_first=0, vertex_count=10, sym_first=0, sym_count=1, R_est=eye, R_gt=eye, fx=1.0, fy=1.0)
    base.update(kw)
    return _lib.PgrPoseErrorJob(**base)


def test_pose_error_entry_points_validate_before_any_launch():
    """pgr_pose_errors / pgr_pose_adi: argument misuse is an integer status from host-side checks (fake non-NULL device
    pointers are never dereferenced; no device is touched)."""
    from pegasus_amd import _lib
    lib = _lib.lib()
    fake = C.c_void_p(0x1000)
    bad = _lib.PGR_ERR_INVALID_ARGUMENT
    assert C.sizeof(_lib.PgrPoseErrorJob) == 240 and _lib.PGR_POSE_SYM_CHUNK >= 2

    def errors_rc(job, vertices=fake, syms=fake, out=fake, n=1, n_vertices=100, n_syms=4):
        return lib.pgr_pose_errors(vertices, n_vertices, syms, n_syms, n, C.byref(job) if job is not None else None, out, None, None)

    def adi_rc(job, vertices=fake, out=fake, n=1, n_vertices=100, ws=fake, ws_bytes=1 << 20):
        return lib.pgr_pose_adi(vertices, n_vertices, n, C.byref(job) if job is not None else None, out, ws, ws_bytes, None)
    good = _job()
    assert errors_rc(good, n=0) == 0 and errors_rc(None, None, None, None, n=0) == 0       # nothing to do, no launch
    assert adi_rc(good, n=0) == 0 and adi_rc(None, None, None, n=0, ws=None, ws_bytes=0) == 0
    assert errors_rc(None) == bad and errors_rc(good, vertices=None) == bad and errors_rc(good, syms=None) == bad
    assert errors_rc(good, out=None) == bad and errors_rc(good, n=-1) == bad
    assert adi_rc(None) == bad and adi_rc(good, vertices=None) == bad and adi_rc(good, out=None) == bad and adi_rc(good, n=-1) == bad
    for job in (_job(vertex_count=0), _job(vertex_count=-3), _job(vertex_first=-1), _job(vertex_first=95),
                _job(vertex_first=2 ** 31 - 1, vertex_count=2 ** 31 - 1)):
        assert errors_rc(job) == bad and adi_rc(job) == bad
        assert lib.pgr_pose_adi_workspace_bytes(1, C.byref(job)) == 0 or job.vertex_count > 0
    for job in (_job(sym_count=0), _job(sym_count=-1), _job(sym_first=-1), _job(sym_first=4), _job(sym_first=2, sym_count=3)):
        assert errors_rc(job) == bad
        assert adi_rc(job, ws=None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL                   # ADI does not read the symmetry range
    # the workspace query is host-only: one float64 partial per 256 queries, 256-byte aligned
    jobs = (_lib.PgrPoseErrorJob * 2)(_job(vertex_count=257), _job(vertex_count=1))
    assert lib.pgr_pose_adi_workspace_bytes(2, jobs) == 256
    assert lib.pgr_pose_adi_workspace_bytes(0, jobs) == 0 and lib.pgr_pose_adi_workspace_bytes(2, None) == 0
    assert lib.pgr_pose_adi(fake, 300, 2, jobs, fake, fake, 255, None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL


def test_pose_errors_host_checks():
    from pegasus_amd import pose_error as PE
    eye = np.eye(3)[None]
    with pytest.raises(ValueError, match="need the camera matrix"):
        PE.pose_errors(None, [0], eye, np.zeros((1, 3)), eye, np.zeros((1, 3)), None, ("mssd", "mspd"))
    with pytest.raises(ValueError, match="need the camera matrix"):
        PE.pose_errors(None, [0], eye, np.zeros((1, 3)), eye, np.zeros((1, 3)), None, ("proj",))
    with pytest.raises(ValueError, match="unknown error"):
        PE.pose_errors(None, [0], eye, np.zeros((1, 3)), eye, np.zeros((1, 3)), None, ("vsd",))
    skew = PC.K_SHARED.copy()
    skew[0, 1] = 0.5
    with pytest.raises(ValueError, match="skew"):
        PE.intrinsics(skew, 2)
    with pytest.raises(ValueError, match=r"\[3,3\] or \[2,3,3\]"):
        PE.intrinsics(np.zeros((3, 3, 3)), 2)
    assert PE.intrinsics(PC.K_SHARED, 2).tolist() == [[572.4114, 573.57043, 325.2611, 242.04899]] * 2
    assert PE.SYM_CHUNK == 4
    # re / te on the host follow the restatement
    R = PC.rotation((1, 2, 3), 0.4)
    assert PE.re(R, np.eye(3)) == PR.re_f64(R, np.eye(3)) and abs(PE.re(R, np.eye(3)) - np.degrees(0.4)) < 1e-9
    assert PE.te([1, 2, 3], [[1], [2], [5]]) == 2.0
    # scaling a models_info entry scales lengths only
    info = PE.scaled_model_info(PC.GOLDEN_SETS["discrete_x_continuous"][0], 0.001)
    assert info["diameter"] == 0.18 and info["symmetries_continuous"][0]["axis"] == [1.0, 2.0, 2.0]
    assert np.allclose(info["symmetries_continuous"][0]["offset"], [0.004, -0.003, 0.006])
    m = np.asarray(info["symmetries_discrete"][0]).reshape(4, 4)
    assert np.array_equal(m[:3, :3], np.diag([1.0, -1.0, -1.0])) and np.allclose(m[:3, 3], [0.0, 0.004, -0.002])
    R0, t0 = PE.symmetry_transformations(PC.GOLDEN_SETS["discrete_x_continuous"][0])
    R1, t1 = PE.symmetry_transformations(info)
    assert np.allclose(R0, R1, atol=1e-15) and np.allclose(t0 * 0.001, t1, atol=1e-15)


def test_models_info_with_and_without_symmetries():
    from pegasus_amd import mesh as M
    import mesh_raster_cases as MC
    v, f = MC.icosphere(1, 0.05)
    mesh = M.Mesh(v, f)
    plain = M.models_info(mesh)
    assert list(plain) == ["diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z"]
    assert json.dumps(M.models_info(mesh, None, None)) == json.dumps(plain) == json.dumps(M.models_info(mesh, [], []))
    disc = [PC.DISCRETE[0], PC.DISCRETE[3]]
    info = M.models_info(mesh, disc, [dict(axis=[0, 0, 1], offset=[0.01, 0, 0]), [1, 0, 0, 0, 0.02, 0]])
    assert {k: info[k] for k in plain} == plain
    assert info["symmetries_discrete"] == disc
    assert info["symmetries_continuous"] == [dict(axis=[0.0, 0.0, 1.0], offset=[0.01, 0.0, 0.0]),
                                             dict(axis=[1.0, 0.0, 0.0], offset=[0.0, 0.02, 0.0])]
    json.dumps(info)
    from pegasus_amd.pose_error import symmetry_transformations
    assert len(symmetry_transformations(info, 0.25)[0]) == 3 * (13 + 13)
    not_rotation = list(PC.DISCRETE[0])
    not_rotation[0] = 1.00001
    mirror = np.eye(4)
    mirror[0, 0] = -1.0
    for bad in ([not_rotation], [mirror.reshape(16).tolist()], [[1.0] * 15]):
        with pytest.raises(ValueError):
            M.models_info(mesh, bad)
    with pytest.raises(ValueError):
        M.models_info(mesh, None, [[0, 0, 0, 1, 1, 1]])
    # the command line's symmetries are in model units: translations and offsets take the model's scale
    a = M._parser().parse_args(["-m", "x", "--out", "y", "--obj_id", "1", "--sym_continuous", "0", "0", "1", "0.01", "0", "0",
                                "--sym_discrete", *map(str, PC.DISCRETE[0]), "--sym_discrete", *map(str, PC.DISCRETE[1])])
    d, c = M.scaled_symmetries(a.sym_discrete, a.sym_continuous, 1000.0)
    assert c == [dict(axis=[0.0, 0.0, 1.0], offset=[10.0, 0.0, 0.0])] and len(d) == 2
    assert np.allclose(np.asarray(d[0]).reshape(4, 4)[:3, 3], [0.0, 4000.0, -2000.0])
    assert M.scaled_symmetries(None, None, 1000.0) == (None, None)


def _restated_pose_errors(models, obj_ids, R_est, t_est, R_gt, t_gt, K=None, errors=("mssd", "mspd")):
    """pose_errors through the float64 restatement, for the parts of pose_eval that need no device."""
    out = {e: np.empty(len(obj_ids)) for e in errors}
    verts = models.vertices.numpy().astype(np.float64)
    for p, o in enumerate(obj_ids):
        v0, nv = models.ranges[int(o)]
        Kp = None if K is None else (K if np.ndim(K) == 2 else K[p])
        e = PR.errors_f64(verts[v0:v0 + nv], *models.symmetries(o), R_est[p], t_est[p], R_gt[p], t_gt[p], Kp)
        for name in errors:
            out[name][p] = e[name]
    return out


def test_pose_eval_scores_a_small_dataset(tmp_path, monkeypatch, capsys):
    from pegasus_amd import pose_error as PE, pose_eval
    d = PC.make_eval_dataset(tmp_path)
    results = tmp_path / "est_results.txt"
    pose_eval.write_results(results, d["rows"])
    real_from_dir = PE.PoseErrorModels.from_dir.__func__
    monkeypatch.setattr(PE.PoseErrorModels, "from_dir", classmethod(lambda cls, path, device="cuda", **kw: real_from_dir(cls, path, device="cpu", **kw)))
    monkeypatch.setattr(PE, "pose_errors", _restated_pose_errors)
    out = tmp_path / "eval"
    assert pose_eval.main(["--results", str(results), "--dataset", str(d["dataset"]), "--models", str(d["models"]), "--out", str(out)]) == 0
    printed = dict(line.split(": ") for line in capsys.readouterr().out.strip().splitlines())
    # three valid targets (the instance with visib_fract 0.05 is not one).  Object 1 in image 0: one valid instance, so only the
    # top-scored estimate counts, and that is the bad one; both estimates of the symmetric object are right at every threshold
    assert set(printed) == {"AR_MSSD", "AR_MSPD", "AR"}
    assert float(printed["AR_MSSD"]) == pytest.approx(2 / 3, abs=1e-4) and float(printed["AR_MSPD"]) == pytest.approx(2 / 3, abs=1e-4)
    assert float(printed["AR"]) == pytest.approx(2 / 3, abs=1e-4)
    errs = pose_eval.load_errors(out / "000003" / "errors_mssd.json")
    assert [(e["im_id"], e["obj_id"], e["est_id"], sorted(e["errors"])) for e in errs] == [
        (0, 1, 0, [0, 2]), (0, 1, 1, [0, 2]), (0, 2, 0, [1]), (1, 2, 0, [0])]
    # millimetres, whatever unit the dataset is in: the good estimate is 0.5 mm off in every axis plus a 0.01 rad turn
    assert 0.5 < errs[1]["errors"][0][0] < 2.5 and errs[0]["errors"][0][0] > 40.0
    assert errs[2]["errors"][1][0] < 1e-6 and errs[3]["errors"][0][0] < 1e-6          # the symmetry is taken into account
    mspd = pose_eval.load_errors(out / "000003" / "errors_mspd.json")
    assert 0.0 < mspd[1]["errors"][0][0] < 3.0 and mspd[2]["errors"][1][0] < 1e-6
