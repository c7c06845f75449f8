"""pgr_pose_errors / pgr_pose_adi on the device against the float64 restatement (tests/pose_error_reference.py), at the
smallest shapes at which the kernels can go wrong (tests/pose_error_cases.gpu_calls): V in {1, 63, 64, 65, 255, 256, 257, 1000},
S in {1, 2, chunk - 1, chunk, chunk + 1, 630}, three objects interleaved over 257 jobs with one K per pair, P in {1, 2, 257}.

Tolerances.  The float64 restatement is evaluated on the float32 vertices the device holds.  Per error type the bound is 4 x
the largest deviation of the FLOAT32 RESTATEMENT (errors_f32 / adi_f32: reference against reference, never the kernel) from
the float64 restatement over exactly these calls, as ``python tests/test_pose_error_gpu.py`` measures it on the CPU:

    error   largest |f32 - f64|   bound (4 x)
    mssd    1.0073e-04 mm         4.029e-04
    mspd    5.5993e-05 px         2.240e-04
    add     5.6628e-05 mm         2.265e-04
    proj    2.3414e-05 px         9.366e-05
    adi     1.4004e-05 mm         5.602e-05

re and te are float64 on the device and held to 1e-9 (of max(1, value)).
"""
import sys
import types
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
if __name__ == "__main__":
    sys.path.insert(0, str(HERE.parent))

import pose_error_cases as PC            # noqa: E402
import pose_error_reference as PR        # noqa: E402

MEASURED = {"mssd": 1.0073e-04, "mspd": 5.5993e-05, "add": 5.6628e-05, "proj": 2.3414e-05, "adi": 1.4004e-05}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
TOL_F64 = 1e-9
ALL = ("mssd", "mspd", "add", "adi", "proj", "re", "te")


def chunk():
    from pegasus_amd.pose_error import SYM_CHUNK
    return SYM_CHUNK


def all_calls():
    calls = PC.gpu_calls(chunk())
    return calls + [PC.subset(calls[2], 1), PC.subset(calls[2], 2)]


def reference(call, restate=PR.errors_f64, restate_adi=PR.adi_f64):
    """{name: float64 [P]} of a call through a restatement."""
    P = len(call["obj_ids"])
    out = {k: np.empty(P) for k in ALL}
    for p in range(P):
        o = int(call["obj_ids"][p])
        pts = call["objects"][o][0]
        K = call["K"] if np.ndim(call["K"]) == 2 else call["K"][p]
        args = (call["R_est"][p], call["t_est"][p], call["R_gt"][p], call["t_gt"][p])
        e = restate(pts, *call["syms"][o], *args, K)
        e["adi"] = restate_adi(pts, *args)
        for k in ALL:
            out[k][p] = e[k]
    return out


@pytest.fixture(scope="module")
def calls():
    return {c["name"]: c for c in all_calls()}


@pytest.fixture(scope="module")
def references(calls):
    full = {n: reference(c) for n, c in calls.items() if "[" not in n}
    for n in calls:
        if "[" in n:
            k = len(calls[n]["obj_ids"])
            full[n] = {e: v[:k] for e, v in full[n.split("[")[0]].items()}
    return full


def build_models(call, pad=0):
    """PoseErrorModels of a call's objects; ``pad`` > 0 puts that many NaN rows before, between and after them (as objects no
    job names)."""
    from pegasus_amd.mesh_render import MeshSet
    from pegasus_amd.pose_error import PoseErrorModels
    mesh = lambda v: types.SimpleNamespace(vertices=v, faces=np.zeros((0, 3), np.int32))
    meshes = {2 * o: mesh(pts) for o, (pts, _) in call["objects"].items()}
    if pad:
        for o in list(meshes) + [max(meshes) + 2]:
            meshes[o - 1] = mesh(np.full((pad, 3), np.nan, np.float32))
    models = PoseErrorModels(MeshSet(meshes), {2 * o: info for o, (_, info) in call["objects"].items()})
    return models


def run(models, call, errors=ALL):
    from pegasus_amd.pose_error import pose_errors
    return pose_errors(models, 2 * np.asarray(call["obj_ids"]), call["R_est"], call["t_est"], call["R_gt"], call["t_gt"],
                       call["K"], errors)


def check(got, want, name):
    for e in ALL:
        assert got[e].dtype == np.float64 and got[e].shape == want[e].shape and np.isfinite(got[e]).all(), (name, e)
        dev = np.abs(got[e] - want[e])
        bound = TOL[e] if e in TOL else TOL_F64 * np.maximum(1.0, np.abs(want[e]))
        worst = int(np.argmax(dev - bound))
        print(f"{name:16s} {e:5s} largest deviation {dev.max():.4e} (bound {np.max(bound):.3e})")
        assert (dev <= bound).all(), (name, e, worst, got[e][worst], want[e][worst])


CALL_NAMES = ("v_sweep", "s_sweep", "interleaved", "interleaved[:1]", "interleaved[:2]")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CALL_NAMES)
def test_pose_errors_match_the_float64_restatement(calls, references, name):
    call = calls[name]
    got = run(build_models(call), call)
    check(got, references[name], name)
    kinds = call["kinds"]
    equal = kinds == "equal"
    for e in ("mssd", "mspd", "add", "proj", "adi"):
        assert (got[e][equal] == 0.0).all(), (name, e)                       # a perfect estimate: exactly zero
    sym = kinds == "symmetric"
    diam = np.array([call["diameters"][int(o)] for o in call["obj_ids"]])
    assert (got["mssd"][sym] <= TOL["mssd"]).all() and (got["mspd"][sym] <= TOL["mspd"]).all()
    assert (got["add"][sym] > 0.1 * diam[sym]).all()
    if len(kinds) > 2:
        assert equal.any() and sym.any()


@pytest.mark.gpu
def test_pose_errors_never_read_outside_a_job_and_repeat_bit_for_bit(calls, references):
    import torch
    call = calls["interleaved"]
    plain = run(build_models(call), call)
    models = build_models(call, pad=37)
    assert torch.isnan(models.vertices).any() and models.vertices.shape[0] == 65 + 1000 + 256 + 4 * 37
    padded = run(models, call)
    again = run(models, call)
    check(padded, references["interleaved"], "nan_padded")
    for e in ALL:
        assert np.array_equal(padded[e], plain[e]), e                        # the neighbours' rows are never read
        assert np.array_equal(padded[e], again[e]), e                        # fixed-order sums, order-free minimum


@pytest.mark.gpu
def test_adi_stays_inside_a_workspace_of_the_size_it_asks_for(calls, references):
    """pgr_pose_adi called directly, its workspace exactly pgr_pose_adi_workspace_bytes long between guard bytes and its output
    between guard values: eight jobs of the interleaved call, seven of one tile of queries and one of four (1000 vertices), so
    that a job's partial sums start where the previous job's end."""
    import torch
    from pegasus_amd import _lib
    from pegasus_amd.pose_error import _job_ptr, pose_jobs
    guard = 4096
    call = PC.subset(calls["interleaved"], 8)
    assert sorted(len(call["objects"][int(o)][0]) for o in set(call["obj_ids"])) == [65, 256, 1000]
    models = build_models(call)
    jobs = pose_jobs(models, 2 * np.asarray(call["obj_ids"]), call["R_est"], call["t_est"], call["R_gt"], call["t_gt"], call["K"])
    n, dev = len(jobs), models.device
    nbytes = int(_lib.lib().pgr_pose_adi_workspace_bytes(n, _job_ptr(jobs)))
    assert nbytes == 256                                                     # 11 float64 partial sums, one 256-byte unit
    ws = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((n + 2 * guard,), -7.0, dtype=torch.float32, device=dev)
    _lib.call("pgr_pose_adi", dev, _lib.ptr(models.vertices), models.vertices.shape[0], n, _job_ptr(jobs), _lib.ptr(out[guard:]),
              _lib.ptr(ws[guard:]), nbytes)
    torch.cuda.synchronize()
    assert (ws[:guard] == 0xA5).all() and (ws[guard + nbytes:] == 0xA5).all(), "workspace guard overwritten"
    assert (out[:guard] == -7.0).all() and (out[guard + n:] == -7.0).all(), "output guard overwritten"
    got = out[guard:guard + n].cpu().numpy().astype(np.float64)
    assert np.array_equal(got, run(models, call, ("adi",))["adi"])             # the wrapper's call, bit for bit
    assert (np.abs(got - references["interleaved"]["adi"][:n]) <= TOL["adi"]).all()


@pytest.mark.gpu
def test_scalar_functions_agree_with_the_batched_call(calls):
    from pegasus_amd import pose_error as PE
    call = calls["s_sweep"]
    models = build_models(call)
    got = run(models, call)
    obj = sorted(call["objects"])[2]                                         # S = chunk - 1
    pts = call["objects"][obj][0]
    syms = [dict(R=R, t=t.reshape(3, 1)) for R, t in zip(*call["syms"][obj])]
    K = call["K"]
    for p in np.nonzero(call["obj_ids"] == obj)[0][:3]:
        a = (call["R_est"][p], call["t_est"][p].reshape(3, 1), call["R_gt"][p], call["t_gt"][p].reshape(3, 1))
        assert PE.mssd(*a, pts, syms) == got["mssd"][p] == PE.mssd(*a, models, 2 * obj)
        assert PE.mspd(*a, K, pts, syms) == got["mspd"][p] == PE.mspd(*a, K, models, 2 * obj)
        assert PE.add(*a, pts) == got["add"][p] == PE.add(*a, models, obj_id=2 * obj)
        assert PE.adi(*a, pts) == got["adi"][p] == PE.adi(*a, models, obj_id=2 * obj)
        assert PE.proj(*a, K, pts) == got["proj"][p] == PE.proj(*a, K, models, obj_id=2 * obj)
        assert abs(PE.re(a[0], a[2]) - got["re"][p]) <= TOL_F64 * max(1.0, got["re"][p])
        assert abs(PE.te(a[1], a[3]) - got["te"][p]) <= TOL_F64 * max(1.0, got["te"][p])
    only = run(models, call, ("adi",))
    assert list(only) == ["adi"] and np.array_equal(only["adi"], got["adi"])


@pytest.mark.gpu
def test_pose_eval_scores_a_small_dataset_on_the_device(tmp_path):
    from pegasus_amd import pose_eval
    d = PC.make_eval_dataset(tmp_path)
    results = tmp_path / "est_results.txt"
    pose_eval.write_results(results, d["rows"])
    scores = pose_eval.evaluate(results, d["dataset"], d["models"], vsd=True, out=tmp_path / "eval")
    # three valid targets; the top-scored estimate of object 1 is the bad one, the symmetric object's two are right
    assert scores["AR_MSSD"] == pytest.approx(2 / 3) and scores["AR_MSPD"] == pytest.approx(2 / 3)
    assert 0.0 <= scores["AR_VSD"] <= 1.0 and scores["AR"] == pytest.approx((4 / 3 + scores["AR_VSD"]) / 3)
    errs = pose_eval.load_errors(tmp_path / "eval" / "000003" / "errors_mssd.json")
    assert 0.5 < errs[1]["errors"][0][0] < 2.5 and errs[2]["errors"][1][0] <= 1e-3 and len(errs) == 4
    vsd = pose_eval.load_errors(tmp_path / "eval" / "000003" / "errors_vsd.json")
    assert all(len(v) == len(pose_eval.VSD_TAUS) and all(0.0 <= x <= 1.0 for x in v) for e in vsd for v in e["errors"].values())


def measure():
    """The largest deviation of the float32 restatement from the float64 one over the tests' calls (CPU only)."""
    worst = {k: 0.0 for k in MEASURED}
    for c in all_calls():
        if "[" in c["name"]:
            continue                                                         # subsets of a call measured whole
        a, b = reference(c), reference(c, PR.errors_f32, PR.adi_f32)
        for k in worst:
            worst[k] = max(worst[k], float(np.abs(a[k] - b[k]).max()))
        eq = c["kinds"] == "equal"
        assert all((b[k][eq] == 0.0).all() for k in worst)
        assert np.array_equal(a["re"], b["re"]) and np.array_equal(a["te"], b["te"])
    for k, v in worst.items():
        print(f"{k:5s} {v:.4e}   x4 = {4 * v:.3e}")
    return worst


if __name__ == "__main__":
    measure()
