"""The restatements and inputs of the training-step and kNN kernel tests, without a GPU: the float32 transcription of the
loss agrees with float64 autograd where SSIM is well conditioned, the conditions the device tests rely on hold on every
case, the committed bound table is current, and the Adam / densification / kNN restatements agree with independent ones."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import train_cases as TC                 # noqa: E402
import train_reference as TR             # noqa: E402
import test_train_kernels_gpu as G       # noqa: E402

F32 = np.float32
ALL_CASES = list(G.LOSS_CASES.values()) + list(G.MASKED_CASES.values())


def _separated(d):
    return bool(((d == 0.0) | (np.abs(d) >= TC.SEPARATION)).all())


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def test_every_loss_case_keeps_its_l1_signs_decided():
    """x - y' and alpha - mask, in float64 from the float32 inputs, are exactly 0 or at least 1e-4 in magnitude: on every
    element of every case, so the device comparison leaves nothing out."""
    assert len(G.LOSS_CASES) == len(TC.loss_cases()) and len(G.MASKED_CASES) == len(TC.masked_cases())   # names are unique
    equal_regions = 0
    for case in ALL_CASES:
        inp = G.case_inputs(case)
        x, y = inp["x"].astype(np.float64), inp["y"].astype(np.float64)
        assert inp["x"].dtype == inp["y"].dtype == F32 and inp["x"].shape == inp["y"].shape == (3, case["H"], case["W"])
        if inp["mask"] is not None:
            m = inp["mask"].astype(np.float64)
            y = y * m[None] + inp["bg"].astype(np.float64)[:, None, None] * (1.0 - m[None])
            assert m.min() >= 0.0 and m.max() <= 1.0
            if case["kind"] == "binary":
                assert set(np.unique(m)) <= {0.0, 1.0}
                assert np.array_equal(TR.masked_target_f32(inp["y"], inp["mask"], inp["bg"]).astype(np.float64), y)
                assert (x == y)[:, m == 0].all()                             # converged to the background outside the mask
                if (m == 1).any():
                    assert (x != y)[:, m == 1].any()
            if inp["alpha"] is not None:
                da = inp["alpha"].astype(np.float64) - m
                assert _separated(da), case["name"]
                if case["kind"] == "binary":
                    assert (da == 0).any() and (da != 0).any()
        d = x - y
        assert _separated(d), (case["name"], float(np.abs(d[d != 0]).min()))
        equal_regions += bool((d == 0).any() and (d != 0).any())
    assert equal_regions >= 20


def test_case_lists_cover_what_they_claim():
    shapes = {(c["H"], c["W"]) for c in G.LOSS_CASES.values()}
    assert shapes == set(TC.SHAPES) and len(TC.SHAPES) == 13
    for fam in TC.FAMILIES:
        mine = [c for c in G.LOSS_CASES.values() if c["family"] == fam]
        hw = {(c["H"], c["W"]) for c in mine}
        assert len(hw) >= 4 and any(min(s) == 1 and max(s) > 1 for s in hw), fam                  # a thin shape
        assert any(s[0] % 16 and s[1] % 16 and min(s) > 16 for s in hw), fam                         # ragged in both axes
        assert sum(c["lams"] == (0.0, 0.2, 1.0) for c in mine) >= 2, fam
    assert sum(c["lams"] == (0.0, 0.2, 1.0) for c in G.LOSS_CASES.values() if c["family"] == "noise") >= 3
    consts = {TC.CONSTANTS[c["variant"]] for c in G.LOSS_CASES.values() if c["family"] == "constant"}
    assert consts == {0.25, 0.5, 1.0, 0.0}
    m = list(G.MASKED_CASES.values())
    assert {c["lam_a"] for c in m} == {0.0, 0.5} and {c["use_alpha"] for c in m} == {True, False}
    assert {c["want_grad"] for c in m} == {True, False} and {c["bg"] for c in m} == set(TC.BACKGROUNDS)
    assert {c["want_grad_alpha"] for c in m if c["use_alpha"]} == {True, False} and {c["kind"] for c in m} == {"binary", "soft"}
    assert {c["lam"] for c in m} == {0.0, 0.2, 1.0}


def test_impulses_sit_on_tile_corners_and_window_edges():
    px = TC.impulse_pixels(33, 47)
    at = {(r, q) for _, r, q in px}
    assert {(0, 0), (15, 15), (16, 16), (32, 46), (5, 5), (6, 6), (10, 10), (11, 11), (21, 21), (22, 22)} <= at
    assert {c for c, _, _ in px} == {0, 1, 2}
    assert {(r, q) for _, r, q in TC.impulse_pixels(1, 1)} == {(0, 0)}
    x, y = TC.image_pair("texture_impulses", 33, 47)
    for c, r, q in px:
        assert abs(float(x[c, r, q]) - float(y[c, r, q]) - 0.5) <= 2.0 ** -23   # (y + 0.5 rounds to float once)
    # the 21 x 21 footprint of one step reaches the neighbouring tiles and the image border
    f64 = G._f64(dict(x=x, y=y, mask=None, alpha=None, bg=None, lam_a=0.0), 1.0)
    x2 = x.copy()
    x2[0, 16, 16] = y[0, 16, 16]
    g2 = G._f64(dict(x=x2, y=y, mask=None, alpha=None, bg=None, lam_a=0.0), 1.0)
    moved = np.argwhere(np.abs(f64["grad"][0] - g2["grad"][0]) > 0)
    assert moved.min(axis=0).tolist() == [6, 6] and moved.max(axis=0).tolist() == [26, 26]


# ---- the loss restatements --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", TC.WELL_CONDITIONED)
def test_transcription_agrees_with_float64_where_ssim_is_well_conditioned(family):
    """A transcription error must not hide inside a measured bound: on noise and texture the float32 transcription is within
    1e-5 of the largest gradient element of float64 autograd, and 1e-6 in the loss terms."""
    for case in (c for c in G.LOSS_CASES.values() if c["family"] == family):
        for lam in case["lams"]:
            _, f64, f32, _ = G.reference(case, lam)
            dev = G.deviations(f64, f32)
            assert dev["grad"] <= 1e-5 * np.abs(f64["grad"]).max(), (case["name"], lam, dev)
            assert dev["loss"] <= 1e-6 and dev["ssim"] <= 1e-6 and abs(float(f32["out"][1]) - f64["l1"]) <= 1e-6


def test_committed_bound_table_is_current():
    worst = G.measure()
    assert set(worst) == set(G.MEASURED)
    for fam, w in worst.items():
        for q in G.QUANTITIES:
            have = G.MEASURED[fam][q]
            assert have / 1.5 <= w[q] <= have * 1.5, (fam, q, w[q], have)


def test_l1_terms_of_the_transcription_meet_the_fixed_bound():
    """mean |x - y'| and mean |alpha - m| are held to 2^-22 of their value on the device; float32 differences summed in
    double meet that on every case (and the exact quantities are exact)."""
    for case in ALL_CASES:
        for lam in G.case_lambdas(case):
            inp, f64, f32, bound = G.reference(case, lam)
            assert abs(float(f32["out"][1]) - f64["l1"]) <= bound["l1"], (case["name"], f32["out"][1], f64["l1"])
            assert abs(float(f32["out"][3]) - f64["al1"]) <= bound["al1"], case["name"]
            if f32["grad_alpha"] is not None and inp["lam_a"] > 0:
                assert np.allclose(f32["grad_alpha"], f64["grad_alpha"], rtol=1e-6, atol=0)
                assert (np.sign(f32["grad_alpha"]) == np.sign(f64["grad_alpha"])).all()
            assert (np.sign(f32["grad"]) == np.sign(f64["grad"])).all() or lam > 0
    # the product the device test compares grad_alpha with is exact: one float times -1, 0 or 1


def test_transcription_of_identical_images_is_exactly_zero():
    for H, W in TC.SHAPES:
        for fam in ("noise", "flat_object", "out_of_range"):
            x, _ = TC.image_pair(fam, H, W)
            for lam in (0.0, 1.0):
                r = TR.loss_f32(x, x.copy(), lam)
                assert r["out"][0] == 0.0 and r["out"][1] == 0.0 and abs(float(r["out"][2]) - 1.0) <= G.FLOOR
                assert not r["grad"].any()


def test_unit_mask_is_the_unmasked_transcription():
    x, y = TC.image_pair("noise", 21, 27)
    a = TR.loss_f32(x, y, 0.2)
    b = TR.masked_loss_f32(x, None, y, np.ones((21, 27), F32), np.array([0.3, 0.2, 0.9], F32), 0.2, 0.0)
    assert a["grad"].tobytes() == b["grad"].tobytes() and a["out"].tobytes() == b["out"].tobytes()


def test_blur_is_the_two_dimensional_window():
    rng = np.random.default_rng(0)
    v = rng.random((2, 13, 19)).astype(F32)
    w = TR.window64()
    p = np.pad(v.astype(np.float64), ((0, 0), (5, 5), (5, 5)))
    want = sum(w[i] * w[j] * p[:, i:i + 13, j:j + 19] for i in range(11) for j in range(11))
    assert np.abs(TR.blur_f32(v) - want).max() <= 4e-7
    assert abs(float(TR.window32().astype(np.float64).sum()) - 1.0) < 1e-7 and TR.SSIM_C2 == F32(0.03) * F32(0.03)


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def test_adam_transcription_against_float64_and_torch():
    import torch
    rng = np.random.default_rng(5)
    n = 4097
    for betas, eps in (((0.9, 0.999), 1e-15), ((0.8, 0.99), 1e-8)):
        for start in TC.ADAM_START_STEPS:
            for kind in ("wide", "unit", "tiny", "huge"):
                p = rng.standard_normal(n).astype(F32)
                m, v = TC.adam_history(kind, n, start, rng)
                g = TC.adam_gradient(kind, n, 0, rng)
                lr, step = 0.01, start + 1
                p32, m32, v32 = TR.adam_f32(p, g, m, v, lr, *betas, eps, step)
                p64, m64, v64 = TR.adam_f64(p, g, m, v, lr, *betas, eps, step)
                # m and v: the float weights and two roundings each (2^-24 relative of the operands); the update m / denom passes through
                # five more (sqrt, scale, + eps, divide, and the rounded step size), taken against |m| + |g| because the
                # new m may have cancelled; the final fma rounds at p's size
                e = 2.0 ** -24
                assert (np.abs(m32 - m64) <= 2 * e * (np.abs(m.astype(np.float64)) + np.abs(g.astype(np.float64)))).all()
                assert (np.abs(v32 - v64) <= 4 * e * v64).all()
                denom = np.sqrt(v64) / math.sqrt(1.0 - betas[1] ** step) + eps
                upd = (lr / (1.0 - betas[0] ** step)) * (np.abs(m.astype(np.float64)) + np.abs(g.astype(np.float64))) / denom
                assert (np.abs(p32 - p64) <= e * np.abs(p64) + 12 * e * upd).all(), (betas, start, kind)
                # torch's own CPU kernels round in the same places up to contraction: a couple of ulp
                tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
                opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps, foreach=False)
                if start:
                    opt.state[tp] = {"step": torch.tensor(float(start)), "exp_avg": torch.from_numpy(m.copy()),
                                     "exp_avg_sq": torch.from_numpy(v.copy())}
                tp.grad = torch.from_numpy(g.copy())
                opt.step()
                st = opt.state[tp]
                assert TR.ulps(m32, st["exp_avg"].numpy()).max() <= 2 and TR.ulps(v32, st["exp_avg_sq"].numpy()).max() <= 2
                assert float(st["step"]) == step


def test_adam_scalars_and_cases():
    k = TR.adam_scalars(0.01, 0.9, 0.999, 1e-15, 29999)
    assert 1.0 - math.pow(0.9, 29999.0) == 1.0 and k["neg_step_size"] == F32(-0.01)        # the late step: bc1 rounds to 1
    assert k["w1"] == F32(1.0 - 0.9) and k["w2"] == F32(1.0 - 0.999) and k["eps"] == F32(1e-15) and k["eps"] > 0
    assert TR.adam_scalars(0.01, 0.9, 0.999, 1e-15, 1)["neg_step_size"] == F32(-(0.01 / (1.0 - 0.9)))
    layouts = TC.adam_layouts()
    count = lambda groups, cond=lambda n, k: True: sum(cond(n, k) for g in groups for n, k in zip(g["sizes"], g["kinds"]))
    assert count(layouts["sixteen"]) == 16 == count(layouts["sixteen"], lambda n, k: n > 0)
    e = [n for g in layouts["sixteen_empties"] for n in g["sizes"]]
    assert e[0] == 0 and e[-1] == 0 and 0 in e[1:-1] and sum(n > 0 for n in e) == 16 and len(e) == 19
    assert count(layouts["seventeen"], lambda n, k: k != "none") == 17 and count(layouts["seventeen"], lambda n, k: k == "none") == 1
    assert any(len(g["sizes"]) == 3 for g in layouts["seventeen"])
    assert count(layouts["thirty_three"]) == 33 and len({(g["betas"], g["eps"]) for g in layouts["thirty_three"]}) == 2
    for groups in layouts.values():
        assert all(b1 > 0.5 for g in groups for b1 in g["betas"][:1])           # the kernel is at::lerp's weight < 0.5 branch
    sizes = {n for groups in layouts.values() for g in groups for n in g["sizes"]}
    assert set(TC.ADAM_EDGE_SIZES) <= sizes
    rng = np.random.default_rng(0)
    seen = set()
    for kind in TC.GRAD_KINDS:
        for k_ in range(TC.ADAM_STEPS):
            g = TC.adam_gradient(kind, 5000, k_, rng)
            assert ((g == 0) | (np.abs(g) >= F32(1e-15))).all() and np.isfinite(g).all()
            seen.add((float(np.abs(g).min()) == 0.0, bool((g > 0).any() and (g < 0).any())))
            if kind == "wide":
                assert np.abs(g).min() < 1e-10 and np.abs(g).max() > 1e5
    assert (True, False) in seen and (False, True) in seen
    assert TC.adam_gradient("none", 3, 0, rng) is None


# ---- densification statistics ---------------------------------------------------------------------------------------------
def test_densify_inputs_and_restatement():
    import torch
    for n in TC.DENSIFY_N:
        for columns in TC.DENSIFY_COLUMNS:
            d = TC.densify_inputs(n, columns)
            vis = d["radii"] > 0
            assert d["vgrad"].shape == (n, columns) and np.isfinite(d["vgrad"][vis]).all() and np.isfinite(d["accum"][vis]).all()
            if n > 1:
                assert {0, 1, 2 ** 24 + 1} <= set(d["radii"].tolist()) and (d["radii"] < 0).any()
                assert np.isnan(d["vgrad"][~vis]).any() and np.isinf(d["vgrad"][~vis]).any()
                assert np.isnan(d["accum"][~vis]).any() or n < 300
            acc, den, mr = TR.densify_f64(d["vgrad"], d["radii"], d["accum"], d["denom"], d["max_r"])
            t = {k: torch.from_numpy(v.copy()) for k, v in d.items()}
            tv = torch.from_numpy(vis)
            t["accum"][tv] += torch.norm(t["vgrad"][tv, :2], dim=-1, keepdim=True)
            assert TR.ulps(acc[vis].astype(F32), t["accum"].numpy().reshape(-1)[vis]).max(initial=0) <= 2
            assert np.array_equal(den[vis], d["denom"].reshape(-1)[vis] + 1)
            assert np.array_equal(mr[vis], np.maximum(d["max_r"][vis], d["radii"][vis].astype(F32)))
            for a, b in ((den, d["denom"]), (mr, d["max_r"])):
                assert np.array_equal(a.view(np.int32)[~vis], b.reshape(-1).view(np.int32)[~vis])
    assert F32(2 ** 24 + 1) == 2.0 ** 24
    assert (TC.densify_inputs(1, 2, 0)["radii"] > 0).all() and (TC.densify_inputs(1, 2, 1)["radii"] <= 0).all()


# ---- kNN --------------------------------------------------------------------------------------------------------------------
def test_knn_cases_and_restatement():
    assert TC.knn_grid_target(125) == 4 and TC.knn_grid_target(729) == 8            # lattice cells of exactly h
    assert TC.knn_grid_target(5000) == 14 and 14 ** 3 % 1024 != 0 and TC.knn_grid_target(150_000) == 43
    assert TC.knn_grid_target(TC.KNN_BIG_N) == 128 and TC.knn_grid_target(TC.KNN_BIG_N - 1) == 127
    for name in TC.KNN_CASES:
        p = TC.knn_points(name)
        assert p.dtype == F32 and p.ndim == 2 and p.shape[1] == 3 and np.isfinite(p).all()
        if name.startswith("lattice"):
            k = int(name[7])
            assert len(p) == k ** 3
            ext = p.max(axis=0) - p.min(axis=0)
            assert (ext == (k - 1) * TC.LATTICE_H).all() and F32(ext[0]) / F32(k - 1) == F32(TC.LATTICE_H)
            cells = (p - p.min(axis=0)) / F32(TC.LATTICE_H)
            assert (cells == np.round(cells)).all()                                  # every point on a cell boundary
            assert (TR.knn_f64(p) == TC.LATTICE_H ** 2).all()
        if name in ("identical", "two_groups"):
            assert not TR.knn_f64(p, brute=True).any()
    assert {len(TC.knn_points(n)) for n in ("n2", "n3", "n4", "n5")} == {2, 3, 4, 5}
    assert len(TC.knn_points("identical")) == 300 and len(TC.knn_points("two_groups")) == 64
    line = TC.knn_points("line_z")
    assert not line[:, :2].any() and len(np.unique(line[:, 2])) > 2900
    box = TC.knn_points("long_box")
    ext = box.max(axis=0) - box.min(axis=0)
    assert 0.99e3 < ext[0] / ext[1] < 1.01e3 and 0.99e3 < ext[1] / ext[2] < 1.01e3
    one = TC.knn_points("one_cell")
    assert len(one) == 20_001 and (np.abs(one[:-1]) <= 1e-3).all() and (one[-1] == 1e6).all()
    p = TC.knn_points("uniform5000")
    some = np.arange(0, 5000, 50)
    assert np.allclose(TR.knn_f64(p, queries=some), TR.knn_f64(p, queries=some, brute=True), rtol=1e-14, atol=0)
    d = TR.knn_f64(TC.knn_points("n5"), brute=True)
    q = TC.knn_points("n5").astype(np.float64)
    want = [np.sort(((q - q[i]) ** 2).sum(axis=1))[1:4].mean() for i in range(5)]
    assert np.allclose(d, want, rtol=1e-15)
