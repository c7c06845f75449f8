"""The C oracle against the float64 rasterizer reference (tests/raster_reference.py), on the CPU: per-element bounds, decided
sets, caps on what may stay undecided, ladders against their closed forms, and mutation checks -- the evidence, without a GPU,
that the reference and its bounds are sound (the oracle is inside them everywhere) and tight (a 0.1 % change of any constant of
the model, or a flipped strictness, is outside them).  tests/test_raster_decisions_gpu.py makes the same comparison for HIP."""
import functools
import math

import numpy as np
import pytest

import raster_cases as RC
import raster_reference as RR

from raster_cases import MAX_UNDECIDED_GAUSSIANS, MAX_UNDECIDED_PIXELS

F32 = np.float32
EPS = float(F32(1e-4))
AMIN = float(F32(1.0) / F32(255.0))
AMAX = float(F32(0.99))


@functools.lru_cache(maxsize=None)
def oracle_out(name, cull_mode):
    import oracle
    return oracle.forward(**RC.case(name)["kw"], num_threads=4, cull_mode=cull_mode)


def _report(tag, ratios):
    print(f"{tag}: " + "  ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


@pytest.mark.parametrize("cull_mode", (0, 1))
@pytest.mark.parametrize("name", RC.NAMES)
def test_oracle_within_float64_bounds(name, cull_mode):
    """Every output of the oracle against float64: continuous ones within the per-element bound, integer ones equal on decided
    Gaussians and one of the neighbouring outcomes elsewhere, lists complete (cull_mode 0) or short of skipped instances only
    (cull_mode 1) and sorted, blended sets / last blended / stop entry equal on decided pixels."""
    pre, img = RC.reference(name)
    ratios, fails = RR.compare(pre, img, oracle_out(name, cull_mode), tight=bool(cull_mode))
    _report(f"{name} cull_mode={cull_mode}", ratios)
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("name", RC.NAMES)
def test_no_case_meets_det_zero_and_decided_work_exists(name):
    pre, img = RC.reference(name)
    assert not pre["det_zero"][pre["possible"] | pre["projected"]].any()        # det == 0 cannot occur after + 0.3
    assert (pre["det"].v[pre["projected"]] >= 0.3 * 0.3 * 0.999).all()
    assert pre["projected"].any() and img["decided"].any()


@pytest.mark.parametrize("name", RC.GENERIC + RC.CONDITIONING + ("posed_two_objects",))
def test_undecided_shares_obey_the_caps(name):
    pre, img = RC.reference(name)
    shares = RR.undecided_shares(pre)
    und = float((~img["decided"]).mean())
    print(f"{name}: undecided Gaussians {shares}  undecided pixels {und:.3g} {img['und_kinds']}")
    for kind, share in shares.items():
        assert share <= MAX_UNDECIDED_GAUSSIANS, (name, kind, share)
    assert und <= MAX_UNDECIDED_PIXELS, (name, und, img["und_kinds"])
    info = RC.case(name)["info"]
    if "min_det_cond" in info:
        assert pre["det_cond"][pre["projected"]].max() > info["min_det_cond"]
    if "min_clamped" in info:
        c, r = pre["clamped"][pre["projected"]], np.stack([t.v for t in pre["txtz"]], 1)[pre["projected"]]
        assert c.any(1).sum() >= info["min_clamped"]
        assert (c[:, 0] & (r[:, 0] > 0)).any() and (c[:, 0] & (r[:, 0] < 0)).any()
        assert (c[:, 1] & (r[:, 1] > 0)).any() and (c[:, 1] & (r[:, 1] < 0)).any()


def test_deep_blending_exercises_the_accumulated_T_bound():
    pre, img = RC.reference("deep_800_faint")
    deep = img["decided"] & (img["nblend"] > 100)
    assert deep.mean() > 0.5, (deep.mean(), img["nblend"].max(), img["und_kinds"])
    T = img["final_T"]
    # the bound grows with the number of blends: a few u per blend, relative
    rel = (T.e / T.v)[deep] / RR.U
    assert (rel > 100).all() and (rel < 40 * img["nblend"][deep]).all(), (rel.min(), rel.max())


# ---- ladders: the closed form, and every rung at 8x its bound or more decided and in agreement ------------------------------
def _pix_closed(c, g):
    """Pixel position of splat g of an unrotated camera at the origin: ((p00 x / (z + 1e-7) + 1) W - 1) / 2."""
    v, m = c["view"], c["act"]["means3d"].astype(np.float64)
    pm = np.asarray(v.full_proj_transform, F32).astype(np.float64).reshape(16)
    w = m[g, 2] + float(F32(1e-7))
    return ((pm[0] * m[g, 0] / w + 1.0) * v.width - 1.0) / 2.0, ((pm[5] * m[g, 1] / w + 1.0) * v.height - 1.0) / 2.0


def _cov2_closed(c, g):
    """Sigma2D of an isotropic splat (scale s) seen by an unrotated camera: s^2 J J^T + 0.3 I with
    J = [[fx / z, 0, -fx x / z^2], [0, fy / z, -fy y / z^2]] (no clamp: |x / z| < 1.3 tanfov is asserted)."""
    v, a = c["view"], c["act"]
    x, y, z = (float(t) for t in a["means3d"][g])
    s = float(a["scales"][g, 0])
    tfx, tfy = float(F32(v.tanfovx)), float(F32(v.tanfovy))
    fx, fy = v.width / (2.0 * tfx), v.height / (2.0 * tfy)
    assert abs(x / z) < 1.3 * tfx and abs(y / z) < 1.3 * tfy
    j = ((fx / z, -fx * x / z ** 2), (fy / z, -fy * y / z ** 2))
    lp = float(F32(0.3))
    return (s * s * (j[0][0] ** 2 + j[0][1] ** 2) + lp, s * s * j[0][1] * j[1][1], s * s * (j[1][0] ** 2 + j[1][1] ** 2) + lp)


def _radius_closed(c, g):
    a, b, cc = _cov2_closed(c, g)
    mid = 0.5 * (a + cc)
    return 3.0 * math.sqrt(mid + math.sqrt(max(float(F32(0.1)), mid * mid - (a * cc - b * b))))


def test_radius_ladder():
    c = RC.case("ladder_radius")
    pre, _ = RC.reference("ladder_radius")
    o = oracle_out("ladder_radius", 0)
    n_far = n_open = 0
    for g, (R, k, sgn) in enumerate(c["info"]["rungs"]):
        closed = _radius_closed(c, g)
        assert abs(pre["rr"].v[g] - closed) <= 1e-12 * closed, (g, pre["rr"].v[g], closed)
        a, b, cc = _cov2_closed(c, g)
        assert b == 0.0 and abs(a / cc - 1.0) < 1e-6 and (0.5 * (a - cc)) ** 2 < 0.1      # isotropic: the max(0.1, .) floor holds
        assert abs(closed / R - 1.0 - sgn * 2.0 ** -k) < 4e-7                          # the rung stands where it was put
        if abs(closed - R) >= 8.0 * pre["rr"].e[g]:
            n_far += 1
            want = R + 1 if closed > R else R
            assert pre["dec"]["radius"][g] and pre["radius"][g] == want == o["radii"][g], (g, R, k, sgn)
        n_open += not pre["dec"]["radius"][g]
        if k == 30:
            assert not pre["dec"]["radius"][g]                                           # 2^-30 is inside any float32 bound
    assert n_far >= 4 * 2 * 6 and n_open >= 4 * 2 * 3, (n_far, n_open)


def test_rectangle_ladder():
    c = RC.case("ladder_rect")
    pre, _ = RC.reference("ladder_rect")
    o = oracle_out("ladder_rect", 0)
    gx, gy = pre["grid"]
    assert (pre["radius"] == c["info"]["radius"]).all() and pre["dec"]["radius"].all()
    n_far = 0
    for g, (axis, m, which, k, sgn) in enumerate(c["info"]["rungs"]):
        pix = _pix_closed(c, g)[axis]
        closed = (pix - 3.0) / 16.0 if which == "min" else (pix + 3.0 + 15.0) / 16.0
        j = axis + (0 if which == "min" else 2)
        edge = pre["edges"][j]
        assert abs(edge.v[g] - closed) <= 1e-12 * max(1.0, abs(closed)), (g, edge.v[g], closed)
        if abs(closed - m) >= 8.0 * edge.e[g]:
            n_far += 1
            want = min((gx, gy)[axis], max(0, math.floor(closed) if closed > 0 else 0))
            assert pre["rect_lo"][g, j] == pre["rect_hi"][g, j] == pre["rect"][g, j] == want, (g, axis, m, which, k, sgn)
    assert n_far >= 10 * 2 * 6, n_far
    # the oracle's tile counts on every decided rung (its rectangles are not an output)
    dm = pre["dec"]["member"]
    tt = (pre["rect"][:, 2] - pre["rect"][:, 0]) * (pre["rect"][:, 3] - pre["rect"][:, 1]) * pre["projected"]
    assert np.array_equal(o["tiles_touched"][dm], tt[dm]) and 0 < (~dm).sum() < 0.6 * dm.size


@pytest.mark.parametrize("name", ("ladder_near_exact", "ladder_near_translated"))
def test_near_plane_ladder(name):
    c = RC.case(name)
    pre, _ = RC.reference(name)
    o = oracle_out(name, 0)
    near = float(F32(0.2))
    vm14 = float(np.asarray(c["view"].world_view_transform, F32).reshape(16)[14])
    n_far = 0
    for g, rung in enumerate(c["info"]["rungs"]):
        closed = float(c["act"]["means3d"][g, 2]) + vm14
        assert abs(pre["z"].v[g] - closed) <= 1e-15
        if name == "ladder_near_exact":
            assert pre["z"].e[g] == 0 and pre["dec"]["near"][g]                          # view z IS the input: every rung decided
        if abs(closed - near) >= 8.0 * pre["z"].e[g]:
            n_far += 1
            assert pre["dec"]["near"][g] and bool(pre["culled"][g]) == (closed <= near) == (o["radii"][g] == 0), (g, rung)
    assert n_far >= (53 if name == "ladder_near_exact" else 2 * 10)
    if name == "ladder_near_exact":
        # 0.2f itself is culled, its upper neighbour is not
        assert pre["culled"][0] and not pre["culled"][1] and pre["culled"][2]
    else:
        assert not pre["dec"]["near"].all()


def _oracle_last(o, pre, y, x):
    """The Gaussian the oracle blended last at pixel (x, y)."""
    t = (y // 16) * pre["grid"][0] + x // 16
    nc = int(o["n_contrib"][y, x])
    return int(o["gauss_sorted"][int(o["ranges"][t, 0]) + nc - 1]) if nc else -1


def _probe_alpha(c, pre, g, px, py):
    """(closed form of opacity * exp(power) of splat g at its probe pixel, the reference's pair)."""
    cx, cy = _pix_closed(c, g)
    a, b, cc = _cov2_closed(c, g)
    dx, dy = cx - px, cy - py
    closed = float(c["act"]["opacities"][g]) * math.exp(-0.5 * (cc * dx * dx - 2.0 * b * dx * dy + a * dy * dy) / (a * cc - b * b))
    _, a = RR.pair_alpha(pre, g, np.float64(px), np.float64(py))
    return closed, a


@pytest.mark.parametrize("name,thr", (("ladder_alpha_min", AMIN), ("ladder_alpha_max", AMAX)))
def test_alpha_ladders(name, thr):
    c = RC.case(name)
    pre, img = RC.reference(name)
    o = oracle_out(name, 1)
    px, py = c["info"]["probe"]
    n_far = 0
    for g, rung in enumerate(c["info"]["rungs"]):
        x, y = int(px[g]), int(py[g])
        closed, a = _probe_alpha(c, pre, g, x, y)
        assert abs(float(a.v) - closed) <= 1e-10 * closed, (g, float(a.v), closed)
        if g == 0:
            assert float(a.v) == thr and float(a.e) == 0.0 and img["decided"][y, x]      # ON the threshold, bound 0
        if abs(closed - thr) >= 8.0 * float(a.e):
            n_far += 1
            assert img["decided"][y, x], (g, rung)
            if thr == AMIN:
                assert img["nblend"][y, x] == (closed >= thr) == (o["n_contrib"][y, x] > 0), (g, rung)
            else:
                T = 1.0 - min(AMAX, closed)
                assert abs(img["final_T"].v[y, x] - T) <= 1e-9 and abs(o["final_T"][y, x] - T) <= img["final_T"].e[y, x] + 1e-9
    assert n_far >= 2 * 6 and (~img["decided"]).sum() >= 4, (n_far, (~img["decided"]).sum())


@pytest.mark.parametrize("name", ("ladder_stop_3", "ladder_stop_10", "ladder_stop_900"))
def test_stop_ladders(name):
    c = RC.case(name)
    pre, img = RC.reference(name)
    o = oracle_out(name, 1)
    m = c["info"]["m"]
    px, py = c["info"]["probe"]
    n_far = 0
    for r, (k, sgn) in enumerate(c["info"]["rungs"]):
        g, x, y = r * (m + 1), int(px[r]), int(py[r])
        closed, a = _probe_alpha(c, pre, g, x, y)
        assert abs(float(a.v) - closed) <= 1e-10 * closed
        t_m = (1.0 - closed) ** m
        assert abs(t_m / EPS - 1.0 - sgn * 2.0 ** -k) < 1e-7 * m + 4e-6                  # opacity is a float32 number
        T = img["final_T"]
        bound = T.e[y, x] / T.v[y, x] * EPS * (m + 1) / m                                # the accumulated bound, one blend on
        if abs(t_m - EPS) >= 8.0 * bound:
            n_far += 1
            want = m if t_m >= EPS else m - 1
            assert img["decided"][y, x] and img["nblend"][y, x] == want, (r, k, sgn, want)
            assert img["stop_g"][y, x] == g + want and _oracle_last(o, pre, y, x) == g + want - 1
    assert n_far >= min(len(c["info"]["rungs"]), 2 * 5), n_far
    if m < 900:
        assert (~img["decided"]).any()                                                   # the fine rungs are open


def test_stop_exactly_at_t_eps():
    c = RC.case("stop_exact")
    pre, img = RC.reference("stop_exact")
    x, y = c["info"]["probe"]
    o = oracle_out("stop_exact", 0)
    # after three blends T = 55 * 2^-19; the fourth's test value is 1e-4f itself with no bound: blended, then the fifth stops
    assert img["decided"][y, x] and img["nblend"][y, x] == 4 == o["n_contrib"][y, x] and img["stop_g"][y, x] == 4
    assert _oracle_last(o, pre, y, x) == 3
    assert img["final_T"].v[y, x] == EPS and img["final_T"].e[y, x] == 0.0 and float(o["final_T"][y, x]) == EPS


def test_colour_clamp_ladder():
    c = RC.case("ladder_color")
    pre, _ = RC.reference("ladder_color")
    o = oracle_out("ladder_color", 0)
    n_far = 0
    for g, (k, sgn) in enumerate(c["info"]["rungs"]):
        closed = math.sqrt(1.0 / (4.0 * math.pi)) * float(c["act"]["shs"][g, 0, 0]) + 0.5
        raw = pre["raw_color"][g][0]
        assert abs(float(raw.v) - closed) <= 1e-15
        if abs(closed) >= 8.0 * float(raw.e):
            n_far += 1
            assert RR.decided(raw, 0.0) and (o["rgb"][g, 0] > 0) == (closed > 0)
            assert abs(o["rgb"][g, 0] - max(closed, 0.0)) <= float(raw.e)
    assert n_far >= 2 * 10 and not pre["dec"]["color"].all()


def test_single_splat_is_the_analytic_image():
    c = RC.case("single_on_axis")
    info = c["info"]
    pre, img = RC.reference("single_on_axis")
    o = oracle_out("single_on_axis", 1)
    W, H = c["view"].width, c["view"].height
    a, b, cc = _cov2_closed(c, 0)
    assert b == 0.0 and pre["radius"][0] == math.ceil(_radius_closed(c, 0)) == o["radii"][0]
    Y, X = np.mgrid[0:H, 0:W].astype(np.float64)
    alpha = info["op"] * np.exp(-0.5 * ((X - (W - 1) / 2) ** 2 / a + (Y - (H - 1) / 2) ** 2 / cc))
    alpha = np.where(alpha >= AMIN, alpha, 0.0)                                          # the rectangle is the whole image
    assert (pre["rect"][0] == (0, 0, pre["grid"][0], pre["grid"][1])).all()
    rgb = np.asarray(c["act"]["shs"][0, 0], np.float64) * math.sqrt(1.0 / (4.0 * math.pi)) + 0.5
    want = rgb[:, None, None] * alpha + np.asarray(c["bg"])[:, None, None].astype(F32).astype(np.float64) * (1.0 - alpha)
    assert img["decided"].all()
    assert np.abs(img["color"].v - want).max() <= 1e-12 and np.abs(img["depth"].v - info["z"] * alpha).max() <= 1e-12
    assert (np.abs(o["color"] - want) <= img["color"].e + 1e-12).all()
    assert img["final_T"].v[H // 2, W // 2] == 1.0 - info["op"]                          # power = 0 exactly at the centre


# ---- mutation checks: every constant of the model moved by about 0.1 %, every strictness flipped -------------------------------
MUTATIONS = (
    ("c1_33x17", dict(lowpass=0.3003)),
    ("ladder_radius", dict(radius_factor=3.003)),
    ("ladder_radius", dict(disc_floor=0.1003)),
    ("ladder_alpha_min", dict(alpha_min=1.0 / 254.0)),
    ("ladder_alpha_max", dict(alpha_max=0.989)),
    ("ladder_stop_10", dict(t_eps=1.01e-4)),
    ("ladder_near_exact", dict(near=0.2002)),
    ("ladder_near_translated", dict(near=0.2002)),
    ("clamp_1p3", dict(clamp=1.301)),
    ("c1_33x17", dict(color_offset=0.5005)),
    ("c1_33x17", dict(tile=8)),
    ("c1_33x17", dict(hom_eps=1e-4)),
    ("ladder_near_exact", dict(near_cull_inclusive=False)),
    ("single_on_axis", dict(power_skip_strict=False)),
    ("ladder_alpha_min", dict(alpha_skip_strict=False)),
    ("stop_exact", dict(stop_strict=False)),
    ("ladder_rect", dict(empty_inclusive=False)),
)


@pytest.mark.parametrize("name,change", MUTATIONS, ids=[f"{n}-{'-'.join(c)}" for n, c in MUTATIONS])
def test_a_mutated_model_disagrees_with_the_oracle(name, change):
    """The reference with one constant perturbed, or one strictness flipped, against the UNCHANGED oracle: the comparison that
    passes for the model's own values must fail.  A mutation that passed would mean its bound or its ladder is too coarse."""
    pre, img = RC.mutated(name, **change)
    _, fails = RR.compare(pre, img, oracle_out(name, 0), tight=False)
    print(f"{name} {change}: {len(fails)} failures, e.g. {fails[:2]}")
    assert fails, (name, change)
    _, base = RR.compare(*RC.reference(name), oracle_out(name, 0), tight=False)
    assert not base
