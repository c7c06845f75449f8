"""Deterministic, named inputs for pgr_bop_gt_info, shared by tests/test_gt_info_host.py and tests/test_gt_info_gpu.py.

A case is a dict: ``name``, ``why`` (the part of the launch or of the kernel it exists for), ``canvases`` float32
[S,Hc,Wc], ``margin`` (mx, my), ``scene`` float32 [F,H,W], ``slots`` and ``frames`` int32 [J] (true indirections), ``K``
float64 [J,4] = fx, fy, cx, cy per job, ``delta``, and ``check``: a function of the reference's (mask, visib, stats) that
asserts the property which makes the case discriminating (a case that lost it would pass a broken kernel).

The two shapes at which the launch changes path are read from pegasus_amd/_lib.py, which mirrors include/pegasus_raster.h
(tests/test_gt_info_host.py holds the two against each other)."""
import numpy as np

from pegasus_amd import _lib

import gt_info_reference as GR

JPL = _lib.PGR_GT_INFO_JOBS_PER_LAUNCH          # jobs per kernel launch: T.first offsets the output rows beyond
BLOCKS_X = _lib.PGR_GT_INFO_BLOCKS_X            # workgroups per job, at most
GRID = BLOCKS_X * 256                           # pixels of one grid pass: planes beyond are walked by the grid-stride loop
WAVE = 64
I32MAX, I32MIN = GR.INT32_MAX, GR.INT32_MIN
EMPTY_ROW = [0, 0, 0, I32MAX, I32MAX, I32MIN, I32MIN, I32MAX, I32MAX, I32MIN, I32MIN]
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def case(name, why, canvases, margin, scene, K, delta, slots=None, frames=None, check=None):
    canvases, scene = np.ascontiguousarray(canvases, np.float32), np.ascontiguousarray(scene, np.float32)
    J = len(K)
    slots = np.arange(J) if slots is None else slots
    frames = np.zeros(J, np.int64) if frames is None else frames
    c = dict(name=name, why=why, canvases=canvases, margin=(int(margin[0]), int(margin[1])), scene=scene,
             slots=np.asarray(slots, np.int32), frames=np.asarray(frames, np.int32), K=np.asarray(K, np.float64).reshape(J, 4),
             delta=float(delta), check=check or (lambda mask, visib, stats: None))
    Hc, Wc = canvases.shape[1:]
    H, W = scene.shape[1:]
    assert c["margin"][0] + W <= Wc and c["margin"][1] + H <= Hc and min(c["margin"]) >= 0
    assert 0 <= c["slots"].min() and c["slots"].max() < len(canvases) and 0 <= c["frames"].min() and c["frames"].max() < len(scene)
    return c


def reference(c, **replace):
    """The reference's outputs of a case (with some inputs replaced: how the checks show that an input matters)."""
    a = dict(c, **replace)
    return GR.reduce(a["canvases"], a["margin"], a["scene"], a["slots"], a["frames"], a["K"], a["delta"])


def _differs(a, b):
    """Per job: do the outputs (mask, visib, stats) of two runs differ."""
    return np.array([any(not np.array_equal(x[k], y[k]) for x, y in zip(a, b)) for k in range(len(a[0]))])


def _K(rng, n, W, H, f=(20.0, 40.0)):
    """One fx, fy, cx, cy per job, none equal to another's."""
    return np.stack([rng.uniform(*f, n), rng.uniform(*f, n), W / 2 + rng.uniform(-2, 2, n), H / 2 + rng.uniform(-2, 2, n)], 1)


def _blob(rng, Hc, Wc, lo=0.8, hi=1.6, fill=0.5):
    """A canvas with a random rectangle of depths (holes inside) and a few scattered pixels, margin included."""
    c = np.zeros((Hc, Wc), np.float32)
    x0, y0 = rng.integers(0, max(1, Wc // 2)), rng.integers(0, max(1, Hc // 2))
    x1, y1 = rng.integers(x0 + 1, Wc + 1), rng.integers(y0 + 1, Hc + 1)
    c[y0:y1, x0:x1] = np.where(rng.random((y1 - y0, x1 - x0)) < fill + 0.4, rng.uniform(lo, hi, (y1 - y0, x1 - x0)), 0)
    pts = rng.random((Hc, Wc)) < 0.03
    c[pts] = rng.uniform(lo, hi, int(pts.sum()))
    return c


def _scene(rng, H, W, lo=0.8, hi=1.6):
    """Scene depth: per pixel missing, an occluder in front of every model depth, or something among the model depths."""
    u = rng.random((H, W))
    return np.where(u < 0.2, 0, np.where(u < 0.45, 0.5 * lo, rng.uniform(lo, hi * 1.2, (H, W)))).astype(np.float32)


# ---- job counts: the chunking of the launches, T.first, slot and frame as indirections, K per job -----------------------
def job_count_case(n_jobs):
    rng = np.random.default_rng(1000 + n_jobs)
    W, H = 8, 6
    Wc, Hc = 3 * W, 3 * H
    n_slots, n_frames, dead_frame = n_jobs + 3, 6, 2
    slots = rng.permutation(n_slots)[:n_jobs]
    K = _K(rng, n_jobs, W, H)
    canvases = np.full((n_slots, Hc, Wc), NAN, np.float32)          # the 3 canvases no job names stay NaN
    for s, (fx, fy, cx, cy) in zip(slots, K):
        canvases[s] = _blob(rng, Hc, Wc)
        inside = rng.random((H, W)) < 0.6                             # never sparse inside the window: the frame matters
        canvases[s, H:2 * H, W:2 * W][inside] = rng.uniform(0.8, 1.6, int(inside.sum()))
        # image pixel (0, 0): every scene is 1 there, the model lies behind it by delta less one part in 10^4 under the job's
        # OWN K -- visible; under an fx or fy that stretches the distance by more, it is not
        stretch = np.sqrt(1.0 + ((0 - cx) / fx) ** 2 + ((0 - cy) / fy) ** 2)
        canvases[s, H, W] = 1.0 + 0.1 / stretch * (1.0 - 1e-4)
    scene = np.stack([_scene(rng, H, W) for _ in range(n_frames)])
    scene[:, 0, 0] = 1.0
    scene[dead_frame] = NAN                                          # a frame no job names
    live = np.array([f for f in range(n_frames) if f != dead_frame])
    frames = live[rng.integers(0, len(live), n_jobs)] if n_jobs > 1 else np.array([live[-1]])

    def check(mask, visib, stats):
        c = dict(canvases=canvases, margin=(W, H), scene=np.nan_to_num(scene, nan=0.7), slots=slots, frames=frames, K=K, delta=0.1)
        base = reference(c)
        assert not np.isnan(canvases[slots]).any() and np.isnan(canvases).any() and sorted(set(frames)) != list(range(n_frames))
        # a dropped T.first writes job k's rows at k - JPL: those rows must differ
        for k in range(JPL, n_jobs):
            assert not np.array_equal(stats[k], stats[k - JPL]) and not np.array_equal(mask[k], mask[k - JPL]), k
        # slot and frame are indirections: the neighbouring canvas or frame, and the job's own index, give other outputs
        for other in (np.arange(n_jobs), (slots + 1) % n_slots, (slots - 1) % n_slots):
            sel = other != slots
            alt = reference(dict(c, canvases=np.nan_to_num(canvases, nan=1.0)), slots=other)
            assert _differs(base, alt)[sel].all()
        for step in (1, 2, 3, 4, 5):
            alt = reference(c, frames=(frames + step) % n_frames)
            assert _differs(base, alt).all(), step
        # every job has its own K, and the K decides: with the neighbouring job's K, a good share of the jobs changes
        assert len({tuple(r) for r in K}) == n_jobs and visib[:, 0, 0].all()
        if n_jobs > 1:
            shared = reference(c, K=np.roll(K, 1, 0))
            assert _differs(base, shared).mean() >= 0.25 and (shared[1][:, 0, 0] == 0).mean() >= 0.25
    return case(f"jobs_{n_jobs}", f"{n_jobs} jobs around {JPL} per launch: chunking, T.first, slot/frame indirection, K per job",
                canvases, (W, H), scene, K, 0.1, slots, frames, check)


# ---- plane sizes: partial waves, partial workgroups, the grid-stride loop -----------------------------------------------
def small_plane_case(Wc, Hc, W, H, mx, my):
    rng = np.random.default_rng(2000 + 31 * Wc + Hc)
    canvases = np.stack([_blob(rng, Hc, Wc, fill=0.3) for _ in range(2)])
    canvases[0, 0, 0] = canvases[0, -1, -1] = 1.0                    # the first and the last pixel of the plane count
    canvases[1, my + H - 1, mx + W - 1] = 1.25                       # and the last pixel of the window
    scene = np.stack([_scene(rng, H, W)])
    scene[0, H - 1, W - 1] = 0.0

    def check(mask, visib, stats):
        assert Wc * Hc == canvases[0].size and stats[0, 0] >= 2 - (Wc * Hc == 1) and visib[1, H - 1, W - 1] == 1
        assert stats[0, 5] == Wc - 1 - mx and stats[0, 6] == Hc - 1 - my and stats[0, 3] == -mx and stats[0, 4] == -my
    return case(f"plane_{Wc}x{Hc}", f"a plane of {Wc * Hc} pixels: the last wave and workgroup are partial or exactly full",
                canvases, (mx, my), scene, _K(rng, 2, W, H), 0.1, check=check)


def _paint(canvas, rng, rows, cols, depth=1.0):
    y0, y1 = rows
    x0, x1 = cols
    canvas[y0:y1, x0:x1] = depth + rng.integers(0, 4, (y1 - y0, x1 - x0)) / 8.0


def grid_case(name, Wc, Hc, W, H, mx, my, why):
    """Three jobs: silhouette, visible pixels and all extremes of both boxes (a) only at plane indices >= GRID, (b) only
    below, (c) on both sides."""
    rng = np.random.default_rng(3000 + Hc)
    plane = Wc * Hc
    row_g = -(-GRID // Wc)                                           # the first canvas row wholly at indices >= GRID
    canvases = np.zeros((3, Hc, Wc), np.float32)
    beyond = plane > GRID
    if beyond:
        assert row_g < my + H, "the image window must reach beyond the first grid pass"
        top = max(row_g, my)
        _paint(canvases[0], rng, (top, my + H), (mx + 3, mx + W - 5))            # inside the window, beyond the first pass
        _paint(canvases[0], rng, (Hc - 1, Hc), (1, Wc - 2))                      # the last canvas row (the last pass)
        _paint(canvases[1], rng, (max(0, my - 2), min(row_g - 1, my + H)), (mx - 1, mx + W // 2))
        canvases[2] = np.where(rng.random((Hc, Wc)) < 0.01, 1.5, 0).astype(np.float32)
        canvases[2, 0, 0] = canvases[2, Hc - 1, Wc - 1] = 1.0
    else:
        _paint(canvases[0], rng, (Hc - 1, Hc), (0, Wc))                          # the last row of the last workgroup
        _paint(canvases[1], rng, (0, my + 2), (mx + 1, mx + 9))
        canvases[2] = np.where(rng.random((Hc, Wc)) < 0.01, 1.5, 0).astype(np.float32)
        canvases[2, 0, 0] = canvases[2, Hc - 1, Wc - 1] = 1.0
    scene = np.full((1, H, W), 3.0, np.float32)
    scene[0, :, ::7] = 0.4                                            # occluded columns
    scene[0, ::5, :] = 0.0                                            # rows of missing depth
    K = _K(rng, 3, W, H, f=(150.0, 250.0))

    def check(mask, visib, stats):
        assert (plane == GRID) if not beyond else (plane > GRID)
        if not beyond:
            return
        index = lambda x, y: (y + my) * Wc + (x + mx)
        a, b = stats[0], stats[1]
        assert a[0] > 0 and a[2] > 0 and b[0] > 0 and b[2] > 0
        # job 0: every silhouette pixel, every visible pixel, hence every extreme of both boxes, lies beyond the first pass
        assert index(a[3], a[4]) >= GRID and index(a[7], a[8]) >= GRID
        assert np.flatnonzero(canvases[0] > 0).min() >= GRID
        # job 1: the same, all below
        assert index(b[5], b[6]) < GRID and index(b[9], b[10]) < GRID
        if plane > 2 * GRID:
            assert index(a[5], a[6]) >= 2 * GRID                      # a third pass holds the box's far corner
    return case(name, why, canvases, (mx, my), scene, K, 0.1, check=check)


# ---- margins --------------------------------------------------------------------------------------------------------
def margin_case(name, Wc, Hc, W, H, mx, my, why):
    rng = np.random.default_rng(4000 + 97 * mx + my + Wc)
    canvases = np.stack([_blob(rng, Hc, Wc) for _ in range(3)])
    canvases[0, 0, 0] = canvases[0, Hc - 1, Wc - 1] = 1.0
    canvases[1, my, mx] = canvases[1, my + H - 1, mx + W - 1] = 1.0
    scene = np.stack([_scene(rng, H, W), _scene(rng, H, W)])
    scene[:, 0, 0] = scene[:, H - 1, W - 1] = 0.0

    def check(mask, visib, stats):
        assert stats[0, 3:7].tolist() == [-mx, -my, Wc - 1 - mx, Hc - 1 - my]
        assert visib[1, 0, 0] == 1 and visib[1, H - 1, W - 1] == 1
        if mx != my and my + W <= Wc and mx + H <= Hc:
            swapped = reference(dict(canvases=canvases, margin=(my, mx), scene=scene, slots=np.arange(3), frames=[0, 1, 1], K=K, delta=0.1))
            assert _differs((mask, visib, stats), swapped).all()
    K = _K(rng, 3, W, H)
    return case(name, why, canvases, (mx, my), scene, K, 0.1, frames=[0, 1, 1], check=check)


# ---- where the silhouette lies --------------------------------------------------------------------------------------------
def placement_case():
    rng = np.random.default_rng(5000)
    W, H = 8, 6
    Wc, Hc = 3 * W, 3 * H
    names = ["empty", "margin_only", "canvas_tl", "canvas_tr", "canvas_bl", "canvas_br", "image_tl", "image_tr", "image_bl",
             "image_br", "full"]
    canvases = np.zeros((len(names), Hc, Wc), np.float32)
    canvases[1, 1:4, 2:7] = 1.0
    canvases[1, Hc - 2, Wc - 3] = 1.0
    corners = [(0, 0), (Wc - 1, 0), (0, Hc - 1), (Wc - 1, Hc - 1), (W, H), (2 * W - 1, H), (W, 2 * H - 1), (2 * W - 1, 2 * H - 1)]
    for k, (x, y) in enumerate(corners):
        canvases[2 + k, y, x] = 1.0
    canvases[10] = rng.uniform(0.8, 1.6, (Hc, Wc))
    scene = np.full((1, H, W), 5.0, np.float32)

    def check(mask, visib, stats):
        assert stats[0].tolist() == EMPTY_ROW and GR.info(stats[0])[0] == dict(
            px_count_all=0, px_count_valid=0, px_count_visib=0, visib_fract=0.0, bbox_obj=[-1] * 4, bbox_visib=[-1] * 4)
        assert stats[1, 0] == 16 and not mask[1].any() and stats[1, 7:].tolist() == EMPTY_ROW[7:]
        assert stats[1, 3:7].tolist() == [2 - W, 1 - H, Wc - 3 - W, Hc - 2 - H]
        for k, (x, y) in enumerate(corners):
            row = stats[2 + k]
            assert row[0] == 1 and row[3:7].tolist() == [x - W, y - H, x - W, y - H]                # a box of width and height 0
            assert int(mask[2 + k].sum()) == (k >= 4) == int(row[2])
        assert stats[2, 3] < 0 and stats[2, 4] < 0
        assert stats[10, 0] == Wc * Hc and stats[10, 2] == W * H and stats[10, 3:].tolist() == [-W, -H, 2 * W - 1, 2 * H - 1, 0, 0, W - 1, H - 1]
    return case("placement", "empty, margin-only, single pixels at every canvas and image corner, the full canvas: sentinels, "
                "negative image coordinates, boxes of width 0", canvases, (W, H), scene, _K(rng, len(names), W, H), 0.1, check=check)


# ---- visibility -----------------------------------------------------------------------------------------------------
def visibility_cases():
    """A canvas whose rows are exactly one wave wide: what a wave sees is what a row holds."""
    W, H, my = WAVE, 4, 4
    Wc, Hc = W, H + 2 * my
    rng = np.random.default_rng(6000)
    K = _K(rng, 4, W, H, f=(60.0, 90.0))
    out = []
    # job 0: visible only where the scene has no depth; job 1: fully occluded; job 2: negative model depth over missing
    # scene depth -- dist_model > 0, so the pixel is in both masks, but it is no silhouette pixel and not valid: px_count_visib
    # is the only thing this wave holds; job 3: the same over row 1, nothing else anywhere
    canvases = np.zeros((4, Hc, Wc), np.float32)
    canvases[0, my:my + H] = 1.0
    canvases[1, my + 1:my + 3, 5:40] = 1.0
    canvases[2, my + 2, 10:20] = -1.0
    canvases[2, 1, 3:9] = 1.0                                        # its silhouette lies in another wave, in the margin
    canvases[3, my + 1, 60:64] = -2.0
    scene = np.full((3, H, W), 0.25, np.float32)
    scene[0, :, 1::2] = 0.0
    scene[2] = 0.0

    def check(mask, visib, stats):
        assert np.array_equal(visib[0], (scene[0] == 0).astype(np.uint8)) and stats[0, 1] == W * H // 2 == stats[0, 2]
        assert stats[1, 0] == 70 == stats[1, 1] and stats[1, 2] == 0 and stats[1, 7:].tolist() == EMPTY_ROW[7:]
        assert stats[2].tolist() == [6, 0, 10, 3, 1 - my, 8, 1 - my, 10, 2, 19, 2]
        assert stats[3].tolist() == [0, 0, 4, I32MAX, I32MAX, I32MIN, I32MIN, 60, 1, 63, 1]
    out.append(case("visibility_waves", "visible only through dist_test == 0; fully occluded; a wave that holds nothing but "
                    "visible pixels (the early wave exit must not drop it)", canvases, (0, my), scene, K, 0.1, frames=[0, 1, 2, 2],
                    check=check))
    # the three deltas on millimetre depths: the scene sits exactly on the model (equal distances: visible at delta = 0), one
    # float32 step nearer and farther, and in front by a float32 distance difference of exactly 15 and its two neighbours
    canv_mm = np.zeros((2, Hc, Wc), np.float32)
    canv_mm[0, my:my + H] = rng.uniform(500, 700, (H, W))
    canv_mm[1, my:my + H, ::2] = rng.uniform(500, 700, (H, W // 2))
    model = canv_mm[:, my:my + H]
    scene_mm = np.empty((2, H, W), np.float32)
    scene_mm[0] = model[0]
    scene_mm[0, 1] = np.nextafter(model[0, 1], np.float32(0))
    scene_mm[0, 2] = np.nextafter(model[0, 2], INF)
    scene_mm[1] = model[1] - rng.uniform(13.5, 16.5, (H, W)).astype(np.float32)
    Kd = _K(rng, 2, W, H, f=(600.0, 900.0))
    stretch = GR.dist_image(np.ones((H, W), np.float32), *Kd[0])
    dist_model = GR.dist_image(model[0], *Kd[0]).astype(np.float32)
    side = np.arange(W) % 3                                          # difference == 15, just above (hidden), just below
    for x in range(W):
        at = np.float32(dist_model[3, x] - np.float32(15.0))
        want = [at, np.nextafter(at, np.float32(0)), np.nextafter(at, INF)][side[x]]
        d = np.float32(np.float64(want) / stretch[3, x])
        for _ in range(64):                                           # the float32 depth whose rounded distance is `want`
            got = np.float32(np.float64(d) * stretch[3, x])
            if got == want:
                break
            d = np.nextafter(d, INF if got < want else np.float32(0))
        scene_mm[0, 3, x] = d
    dist_scene = GR.dist_image(scene_mm[0], *Kd[0]).astype(np.float32)
    exact = (dist_model[3] - dist_scene[3]) == np.float32(15.0)
    assert (exact == (side == 0)).sum() >= W - 4 and exact.sum() >= W // 4       # the search found (nearly) every target

    def check_zero(mask, visib, stats):
        assert visib[0, 0].all() and visib[0, 2].all() and 0 < stats[0, 2] < W * H
    out.append(case("delta_0", "delta = 0 with equal distances: <= must hold where the difference is exactly 0", canv_mm, (0, my),
                    scene_mm, Kd, 0.0, frames=[0, 1], check=check_zero))
    out.append(case("delta_15", "the toolkit's 15 on millimetre depths, differences on both sides of it", canv_mm, (0, my), scene_mm, Kd,
                    15.0, frames=[0, 1], check=lambda m, v, s: _assert(0 < s[1, 2] < s[1, 1] and (v[0, 3][exact] == 1).all()
                                                                       and (v[0, 3][(dist_model[3] - dist_scene[3]) > 15] == 0).all()
                                                                       and (v[0, 3] == 0).sum() >= W // 4)))
    out.append(case("delta_inf", "delta = +inf: every finite difference is visible", canv_mm, (0, my), scene_mm, Kd, np.inf,
                    frames=[0, 1], check=lambda m, v, s: _assert(np.array_equal(m, v))))
    return out


def _assert(ok):
    assert ok


# ---- hostile values -------------------------------------------------------------------------------------------------
def hostile_cases():
    rng = np.random.default_rng(7000)
    W, H = 20, 12
    Wc, Hc = 3 * W, 3 * H
    special = np.array([0.0, -1.0, -0.0, NAN, INF, 1.0, 1.5, -INF], np.float32)
    canvases = special[rng.integers(0, len(special), (4, Hc, Wc))]
    scene = special[rng.integers(0, len(special), (2, H, W))]
    K = _K(rng, 4, W, H)
    K[:, 2:] = np.round(K[:, 2:])                                    # x == cx and y == cy occur: 0 * inf

    def check(mask, visib, stats):
        assert mask.any() and visib.any() and not np.array_equal(mask, visib)
        assert (mask[canvases[:, H:2 * H, W:2 * W] == -1.0] == 1).all()          # dist_model > 0 for a negative depth
    return [case(f"hostile_delta_{d}", "negative, NaN and infinite depths in canvases and scene: the toolkit's formulas taken "
                 "literally, and no fault", canvases, (W, H), scene, K, d, frames=[0, 1, 1, 0], check=check) for d in (15.0, np.inf)]


def all_cases():
    cases = [job_count_case(n) for n in (1, JPL - 1, JPL, JPL + 1, 2 * JPL + 1)]
    cases += [small_plane_case(*s) for s in ((1, 1, 1, 1, 0, 0), (37, 1, 35, 1, 1, 0), (1, 29, 1, 27, 0, 1), (9, 7, 5, 3, 2, 2),
                                             (8, 8, 4, 4, 2, 2), (13, 5, 9, 3, 2, 1), (17, 15, 11, 9, 3, 3), (16, 16, 8, 8, 4, 4),
                                             (257, 1, 255, 1, 1, 0))]
    assert [c["canvases"][0].size for c in cases[5:]] == [1, 37, 29, 63, 64, 65, 255, 256, 257]
    Wg = 512
    assert GRID % Wg == 0 and GRID // Wg > 120
    Hg = GRID // Wg
    cases.append(grid_case("grid_exact", Wg, Hg, 200, 100, 156, (Hg - 100) // 2, f"exactly {GRID} pixels: the last pass-free plane"))
    cases.append(grid_case("grid_plus_row", Wg, Hg + 1, 200, 100, 156, Hg + 1 - 100,
                           "one canvas row beyond the grid: the window is flush with that row, which only the stride loop reaches"))
    assert 600 * 450 > 2 * GRID
    cases.append(grid_case("grid_3x_canvas", 600, 450, 200, 150, 200, 150, "the toolkit's 3x canvas of a 200x150 image: three passes"))
    cases.append(margin_case("margin_0_0", 12, 9, 12, 9, 0, 0, "no margin: the canvas is the image"))
    cases.append(margin_case("margin_x_only", 18, 7, 10, 7, 4, 0, "a margin in x only"))
    cases.append(margin_case("margin_y_only", 10, 17, 10, 7, 0, 5, "a margin in y only"))
    cases.append(margin_case("margin_off_centre", 50, 40, 20, 10, 3, 25, "a canvas wider than W + 2 mx, the window off-centre"))
    cases.append(margin_case("margin_flush", 30, 20, 12, 8, 18, 12, "the window flush with the canvas's last row and column"))
    cases.append(placement_case())
    cases += visibility_cases()
    cases += hostile_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    return cases
