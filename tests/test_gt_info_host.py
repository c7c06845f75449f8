"""The BOP ground-truth reduction without a GPU: the NumPy reference (tests/gt_info_reference.py) against the toolkit's
recorded outputs, the torch restatement against the reference on every case of tests/gt_info_cases.py, the cases' own
discriminating properties, mutants of the restatement that the cases must catch, and pose_error.vsd at its edges."""
import re
from pathlib import Path

import numpy as np
import pytest

import gt_info_cases as GC
import gt_info_reference as GR

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = GC.all_cases()
_REF = {}


def ref(c):
    """The reference's outputs of a case: computed once, shared, read-only."""
    if c["name"] not in _REF:
        out = GC.reference(c)
        for a in out:
            a.setflags(write=False)
        _REF[c["name"]] = out
    return _REF[c["name"]]


def K33(K):
    out = np.zeros((len(K), 3, 3))
    out[:, 0, 0], out[:, 1, 1], out[:, 0, 2], out[:, 1, 2], out[:, 2, 2] = K[:, 0], K[:, 1], K[:, 2], K[:, 3], 1.0
    return out


def torch_reduce(c, slots=None, frames=None, margin=None, canvases=None):
    """reduce_gt_info_torch on a case; its signature has one canvas per job, so the slots are gathered first."""
    import torch
    from pegasus_amd import mesh_render as R
    canv = torch.from_numpy(c["canvases"] if canvases is None else canvases)[torch.as_tensor(c["slots"] if slots is None else slots).long()]
    m, v, s = R.reduce_gt_info_torch(canv, c["margin"] if margin is None else margin, torch.from_numpy(c["scene"]),
                                     c["frames"] if frames is None else frames, K33(c["K"]), c["delta"])
    return m.numpy(), v.numpy(), s.numpy()


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def test_launch_constants_are_the_headers():
    """The shapes the cases are built around are the #defines of include/pegasus_raster.h, not retyped values."""
    from pegasus_amd import _lib
    text = (Path(__file__).resolve().parents[1] / "include" / "pegasus_raster.h").read_text()
    defines = {k: int(v) for k, v in re.findall(r"^#define (PGR_GT_INFO_[A-Z_]+)\s+(\d+)", text, flags=re.M)}
    assert set(defines) == {"PGR_GT_INFO_JOBS_PER_LAUNCH", "PGR_GT_INFO_BLOCKS_X"}
    for name, value in defines.items():
        assert getattr(_lib, name) == value, name
    assert (GC.JPL, GC.BLOCKS_X, GC.GRID) == (defines["PGR_GT_INFO_JOBS_PER_LAUNCH"], defines["PGR_GT_INFO_BLOCKS_X"],
                                              defines["PGR_GT_INFO_BLOCKS_X"] * 256)
    kernel = (Path(__file__).resolve().parents[1] / "pegasus_amd" / "csrc" / "meshraster.hip.h").read_text()
    assert "GT_JOBS_PER_LAUNCH = PGR_GT_INFO_JOBS_PER_LAUNCH;" in kernel and "GT_BLOCKS_X = PGR_GT_INFO_BLOCKS_X;" in kernel
    assert GR.STATS == _lib.PGR_GT_INFO_STATS


def test_reference_reproduces_the_toolkit():
    """What pins the reference: the toolkit's own outputs on the 7 recorded jobs, exactly."""
    g = np.load(GOLDEN / "mesh_gt_info.npz")
    W, H = (int(x) for x in g["size"])
    n = len(g["canvases"])
    K = np.tile([g["K"][0, 0], g["K"][1, 1], g["K"][0, 2], g["K"][1, 2]], (n, 1))
    mask, visib, stats = GR.reduce(g["canvases"], (W, H), g["scene_depth"], np.arange(n), np.arange(n), K, float(g["delta"]))
    np.testing.assert_array_equal(mask, np.unpackbits(g["mask"], axis=-1)[..., :W])
    np.testing.assert_array_equal(visib, np.unpackbits(g["mask_visib"], axis=-1)[..., :W])
    info = GR.info(stats)
    for key in ("px_count_all", "px_count_valid", "px_count_visib", "bbox_obj", "bbox_visib", "visib_fract"):
        np.testing.assert_array_equal(np.asarray([e[key] for e in info]), g[key], err_msg=key)
    assert mask.any() and visib.any() and (mask != visib).any()


def test_the_case_list_is_what_the_kernel_needs():
    names = [c["name"] for c in CASES]
    J = GC.JPL
    assert [n for n in names if n.startswith("jobs_")] == [f"jobs_{n}" for n in (1, J - 1, J, J + 1, 2 * J + 1)]
    planes = sorted(c["canvases"][0].size for c in CASES if c["name"].startswith(("plane_", "grid_")))
    assert planes[:9] == [1, 29, 37, 63, 64, 65, 255, 256, 257] and planes[9] == GC.GRID and planes[10] == GC.GRID + 512
    assert planes[11] > 2 * GC.GRID
    assert {c["delta"] for c in CASES} >= {0.0, 15.0, np.inf}
    print(f"{len(CASES)} cases, {sum(len(c['K']) for c in CASES)} jobs")


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_case_holds_the_property_that_makes_it_discriminating(c):
    mask, visib, stats = ref(c)
    assert set(np.unique(mask)) <= {0, 1} and set(np.unique(visib)) <= {0, 1} and stats.dtype == np.int32
    c["check"](mask, visib, stats)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_torch_restatement_equals_the_reference(c):
    from pegasus_amd import mesh_render as R
    got = torch_reduce(c)
    want = ref(c)
    for name, a, b in zip(("mask", "mask_visib", "stats"), got, want):
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a, b, err_msg=f"{c['name']}: {name}")
    info, want_info = R.info_from_stats(want[2]), GR.info(want[2])
    for key in ("px_count_all", "px_count_valid", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib"):
        np.testing.assert_array_equal(info[key], np.asarray([e[key] for e in want_info]), err_msg=key)


def test_info_from_stats_on_sentinel_rows():
    from pegasus_amd import bop_pose, mesh_render as R
    c = next(c for c in CASES if c["name"] == "placement")
    stats = ref(c)[2]
    assert stats[0].tolist() == GC.EMPTY_ROW
    info = R.info_from_stats(stats)
    entries = bop_pose.scene_gt_info_entry(info, slice(None))
    assert entries[0] == dict(bbox_obj=[-1] * 4, bbox_visib=[-1] * 4, px_count_all=0, px_count_valid=0, px_count_visib=0, visib_fract=0.0)
    assert entries[1]["px_count_all"] == 16 and entries[1]["bbox_obj"] == [-1] * 4 and entries[1]["visib_fract"] == 0.0     # margin only
    assert entries[2]["px_count_all"] == 1 and entries[2]["bbox_obj"] == [-1] * 4                      # a canvas corner: nothing visible
    W, H = 8, 6
    assert entries[6] == dict(bbox_obj=[0, 0, 0, 0], bbox_visib=[0, 0, 0, 0], px_count_all=1, px_count_valid=1, px_count_visib=1,
                              visib_fract=1.0)
    assert entries[9]["bbox_obj"] == [W - 1, H - 1, 0, 0]
    assert entries[10]["bbox_obj"] == [-W, -H, 3 * W - 1, 3 * H - 1] and entries[10]["visib_fract"] == (W * H) / (9.0 * W * H)
    for e, want in zip(entries, GR.info(stats)):
        assert e == want and all(type(v) in (int, float, list) for v in e.values())
    # the fully occluded job: counts without a visible box
    occl = GR.info(ref(next(c for c in CASES if c["name"] == "visibility_waves"))[2])[1]
    assert occl["px_count_all"] == 70 and occl["px_count_visib"] == 0 and occl["bbox_obj"] == [-1] * 4


def test_mutants_of_the_restatement_are_caught(monkeypatch):
    """The cases discriminate: every mutant of the torch restatement -- each one a mistake the kernel or its launch could
    make -- differs from the reference on at least one case.  (Mutated kernels are never run on a device.)"""
    import torch
    from pegasus_amd import mesh_render as R

    def frames_ignored(c):
        return torch_reduce(c, frames=np.zeros_like(c["frames"]))

    def slots_ignored(c):
        return torch_reduce(c, slots=np.arange(len(c["slots"])) % len(c["canvases"]))

    def margins_swapped(c):
        (mx, my), (H, W), (Hc, Wc) = c["margin"], c["scene"].shape[1:], c["canvases"].shape[1:]
        return torch_reduce(c, margin=(my, mx)) if my + W <= Wc and mx + H <= Hc else None

    def with_visibility(name, rule):
        def run(c):
            with monkeypatch.context() as m:
                m.setattr(R, "visibility_mask", rule)
                return torch_reduce(c)
        run.__name__ = name
        return run
    diff = lambda dt, dm: dm.to(torch.float32) - dt.to(torch.float32)
    less_for_less_equal = with_visibility("less_for_less_equal", lambda dt, dm, delta: ((diff(dt, dm) < delta) | (dt == 0)) & (dm > 0))
    missing_depth_clause_dropped = with_visibility("missing_depth_clause_dropped", lambda dt, dm, delta: (diff(dt, dm) <= delta) & (dm > 0))

    def silhouette_inside_the_window_only(c):
        (mx, my), (H, W) = c["margin"], c["scene"].shape[1:]
        canv = np.zeros_like(c["canvases"])
        canv[:, my:my + H, mx:mx + W] = c["canvases"][:, my:my + H, mx:mx + W]
        return torch_reduce(c, canvases=canv)

    def rows_beyond_a_launch_written_at_k_minus_jpl(c):
        m, v, s = (a.copy() for a in torch_reduce(c))
        J = len(s)
        for k in range(GC.JPL, J):
            m[k - GC.JPL], v[k - GC.JPL], s[k - GC.JPL] = m[k], v[k], s[k]
        m[GC.JPL:], v[GC.JPL:], s[GC.JPL:] = 0, 0, np.asarray(GC.EMPTY_ROW, np.int32)
        return m, v, s

    def no_grid_stride(c):
        canv = c["canvases"].copy().reshape(len(c["canvases"]), -1)
        canv[:, GC.GRID:] = 0
        return torch_reduce(c, canvases=canv.reshape(c["canvases"].shape))
    mutants = [frames_ignored, slots_ignored, margins_swapped, less_for_less_equal, missing_depth_clause_dropped,
               silhouette_inside_the_window_only, rows_beyond_a_launch_written_at_k_minus_jpl, no_grid_stride]
    for mutant in mutants:
        caught = []
        for c in CASES:
            got = mutant(c)
            if got is not None and not same(got, ref(c)):
                caught.append(c["name"])
        print(f"{mutant.__name__}: caught by {len(caught)} case(s): {', '.join(caught)}")
        assert caught, f"no case notices the mutant '{mutant.__name__}'"
    assert same(torch_reduce(CASES[0]), ref(CASES[0]))                       # the patches are gone


# ---- VSD at its edges -------------------------------------------------------------------------------------------------
def vsd_edge_groups():
    g = np.load(GOLDEN / "mesh_vsd_edges.npz")
    return [{k: g[f"{name}_{k}"] for k in ("K", "depth_gt", "depth_test", "depth_est", "delta", "taus", "diameter", "est_names", "errors")}
            | {"name": str(name)} for name in g["groups"]]


def check_vsd_edges(device):
    """vsd_from_depths against the toolkit's recorded errors at the bound of test_vsd_equals_the_toolkit (1e-9); batches of 1
    and 3 equal the single calls bit for bit."""
    import torch
    from pegasus_amd import mesh_render as R
    groups = vsd_edge_groups()
    assert {str(n) for g in groups for n in g["est_names"]} >= {"empty_union", "outside_the_image", "at_tau", "clipped", "perfect"}
    assert {g["depth_gt"].shape for g in groups} >= {(1, 1), (6, 8)} and any(not g["depth_test"].any() for g in groups)
    dev = lambda a: torch.from_numpy(np.asarray(a)).to(device)
    for g in groups:
        taus = [float(t) for t in g["taus"]]
        est, gt, test = dev(g["depth_est"]), dev(g["depth_gt"]), dev(g["depth_test"])
        assert len(est) >= 3
        for ci, cost in enumerate(("step", "tlinear")):
            for norm in (0, 1):
                args = (g["K"], float(g["delta"]), taus, bool(norm), float(g["diameter"]), cost)
                want = g["errors"][:, ci, norm]
                whole = R.vsd_from_depths(est, gt, test, *args).cpu().numpy()
                three = R.vsd_from_depths(est[:3], gt, test, *args).cpu().numpy()
                np.testing.assert_allclose(whole, want, rtol=0, atol=1e-9, err_msg=f"{g['name']} {cost} {norm}")
                for k in range(len(est)):
                    one = R.vsd_from_depths(est[k:k + 1], gt, test, *args).cpu().numpy()
                    assert one.shape == (1, len(taus)) and one[0].tobytes() == whole[k].tobytes(), (g["name"], cost, norm, k)
                    if k < 3:
                        assert one[0].tobytes() == three[k].tobytes()
                    stub = lambda jobs, K, size, k=k: torch.stack([est[k], gt])
                    single = R.vsd(np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), test, g["K"], float(g["delta"]), taus, bool(norm),
                                   float(g["diameter"]), None, 1, cost, render=stub)
                    assert np.asarray(single, np.float64).tobytes() == one[0].tobytes()
        names = [str(n) for n in g["est_names"]]
        if "empty_union" in names:
            assert (g["errors"][names.index("empty_union")] == 1.0).all()
        if "perfect" in names:
            assert (g["errors"][names.index("perfect")] == 0.0).all()


def test_vsd_edges_equal_the_toolkit():
    g = {x["name"]: x for x in vsd_edge_groups()}
    # what was recorded is what was meant: at the principal point the step cost flips between tau = 20 and the next double
    taus = g["pixel_on_axis"]["taus"].tolist()
    at, above = taus.index(20.0), taus.index(float(np.nextafter(20.0, 100.0)))
    assert g["pixel_on_axis"]["errors"][0, 0, 0, at] == 1.0 and g["pixel_on_axis"]["errors"][0, 0, 0, above] == 0.0
    assert g["pixel_on_axis"]["errors"][0, 1, 0, at] == 1.0 and 0.3 < g["pixel_on_axis"]["errors"][0, 1, 0, -1] < 0.34   # 20 / 60
    assert (g["blob"]["errors"][2, 1, 0, 0] == 1.0) and 0 < g["blob"]["errors"][2, 1, 0, 4] < 1                # tlinear clipped / not
    check_vsd_edges("cpu")
