"""Registration on the GPU (pegasus_amd/registration.py over pgr_nn_grid_build, pgr_nn_correspond, pgr_icp_sums and
pgr_radius_normals) against the float64 brute force of tests/registration_reference.py.  Correspondences: integer equality of
the indices and bit equality of d2, in cell order and in row order.  Sums: 1e-12 of the sum of the terms' absolute values (a
tree of depth <= 15 and a few roundings per term stay below 2e-15 of it: the factor is headroom), the count exact, equal bytes
from call to call.  Normals: |n . n_ref| >= 1 - 1e-10 where the eigen-gap ratio is above its floor, counts and signs exact.
ICP: iterations, fitness and correspondence set equal, the transformation within the reference's own error (RC.T_TOL); the
RMSE within 1e-12 relative, which is what the tolerance on the sum of d2 under it allows."""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import registration_cases as RC          # noqa: E402
import registration_reference as RR      # noqa: E402

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-12
RMSE_RTOL = 1e-12
DOT_MIN = 1 - 1e-10


def dev_t(dev, a):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)


def gpu_nearest(dev, source, target, distance, T=None, cell_order=True):
    """(index int64, d2 float64) through the package's pair object, in either lane order."""
    import torch
    from pegasus_amd import registration
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    pair = registration._Pair(dev_t(dev, source), dev_t(dev, target), distance, "test", init=T, cell_order=cell_order)
    assert (pair.order is not None) == (cell_order and len(source) > 0 and len(target) > 0)
    if pair.order is not None:
        assert np.array_equal(np.sort(pair.order.cpu().numpy()), np.arange(len(source)))          # a permutation
    pair.correspond(T)
    assert pair.index.dtype == torch.int32 and pair.d2.dtype == torch.float64
    assert tuple(pair.index.shape) == tuple(pair.d2.shape) == (len(source),)
    return pair.index.cpu().numpy().astype(np.int64), pair.d2.cpu().numpy()


def same_neighbours(got, want, what=""):
    index, d2 = got
    bad = np.nonzero(index != want.index)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), index[bad[:8]].tolist(), want.index[bad[:8]].tolist())
    assert d2.tobytes() == want.d2.tobytes(), (what, np.nonzero(d2 != want.d2)[0][:8].tolist())


# ---- correspondences
@pytest.mark.parametrize("cell_order", [True, False])
@pytest.mark.parametrize("ns,nt", [(1, 1), (1, 4099), (4099, 1), (255, 257), (257, 255), (256, 256), (256, 4099), (4099, 4099)])
def test_sizes(gpu_device, ns, nt, cell_order):
    source, target = RC.pair(ns, nt)
    want = RC.reference_pair(ns, nt)
    if min(ns, nt) >= 255:
        assert want.distance_margin > RC.DISTANCE_MARGIN_MIN and (want.index >= 0).any() and (want.index < 0).any()
    same_neighbours(gpu_nearest(gpu_device, source, target, RC.MAX_DISTANCE, RC.POSE_NEAR, cell_order), want, (ns, nt))


def test_public_function_and_empty_clouds(gpu_device):
    import torch
    from pegasus_amd.registration import evaluate_registration, nearest_neighbors
    source, target = RC.pair(257, 4099)
    index, d2 = nearest_neighbors(dev_t(gpu_device, source), dev_t(gpu_device, target), RC.MAX_DISTANCE, RC.POSE_NEAR)
    assert index.dtype == torch.int32 and d2.dtype == torch.float64
    same_neighbours((index.cpu().numpy().astype(np.int64), d2.cpu().numpy()), RC.reference_pair(257, 4099))
    none = torch.zeros((0, 3), device=gpu_device)
    index, d2 = nearest_neighbors(none, dev_t(gpu_device, target), RC.MAX_DISTANCE)
    assert tuple(index.shape) == tuple(d2.shape) == (0,)
    index, d2 = nearest_neighbors(dev_t(gpu_device, source), none, RC.MAX_DISTANCE)
    assert index.cpu().tolist() == [-1] * 257 and d2.cpu().tolist() == [0.0] * 257
    for s, t in ((none, dev_t(gpu_device, target)), (dev_t(gpu_device, source), none)):
        r = evaluate_registration(s, t, RC.MAX_DISTANCE)
        assert r.fitness == 0.0 and r.inlier_rmse == 0.0 and tuple(r.correspondence_set.shape) == (0, 2)


def test_a_point_far_from_everything_has_no_correspondent(gpu_device):
    source, target = RC.pair(257, 4099)
    source = np.vstack([source, [[100.0, -100.0, 100.0]]]).astype(np.float32)
    index, d2 = gpu_nearest(gpu_device, source, target, RC.MAX_DISTANCE, RC.POSE_NEAR)
    assert index[-1] == -1 and d2[-1] == 0.0
    same_neighbours((index[:-1], d2[:-1]), RC.reference_pair(257, 4099))


@pytest.mark.parametrize("cell_order", [True, False])
def test_equidistant_targets_give_the_lower_index(gpu_device, cell_order):
    source, target, distance = RC.equidistant()
    for rows, want in (([0, 1, 2], 0), ([1, 0, 2], 0), ([2, 1, 0], 1), ([2, 0, 1], 1)):
        index, d2 = gpu_nearest(gpu_device, source, target[rows], distance, cell_order=cell_order)
        assert index.tolist() == [want] and d2.tolist() == [2.0 ** -12], rows


def test_comparison_is_strict_and_the_distance_is_float64(gpu_device):
    source, target, distance = RC.tie_345()
    index, d2 = gpu_nearest(gpu_device, source, target, distance)
    assert index.tolist() == [-1] and d2.tolist() == [0.0]
    index, d2 = gpu_nearest(gpu_device, source, target, float(np.nextafter(distance, np.inf)))
    assert index.tolist() == [0] and d2.tolist() == [25 * 2.0 ** -14]
    assert np.float32(distance) == np.float32(np.nextafter(distance, np.inf))      # float32 cannot tell the two apart


@pytest.mark.parametrize("centre,hair", RC.lattice_centres())
def test_cell_walls(gpu_device, centre, hair):
    source, target, distance = RC.wall_lattice(centre, hair)
    want = RR.nearest(source, target, distance)
    assert (want.index >= 0).all()
    for cell_order in (True, False):
        same_neighbours(gpu_nearest(gpu_device, source, target, distance, cell_order=cell_order), want, centre)
    # the same lattices a hair too far apart: nothing corresponds
    inside = distance * (1.0 - 4 * hair)
    want = RR.nearest(source, target, inside)
    assert (want.index < 0).all()
    same_neighbours(gpu_nearest(gpu_device, source, target, inside), want, centre)
    # and posed: the source rotated by a quarter turn about z lands on lattice points again only around the origin
    T = RC.rigid((0, 0, 90), (0, 0, 0))
    same_neighbours(gpu_nearest(gpu_device, source, target, distance, T), RR.nearest(source, target, distance, T), centre)


def test_coincident_targets(gpu_device):
    target = RC.coincident(300)
    source = np.vstack([target[:3], target[:2] + np.float32(5e-4), target[:1] + np.float32(0.5)]).astype(np.float32)
    want = RR.nearest(source, target, 1e-3)
    assert want.index.tolist() == [0, 0, 0, 0, 0, -1]
    for cell_order in (True, False):
        same_neighbours(gpu_nearest(gpu_device, source, target, 1e-3, cell_order=cell_order), want)


def test_a_row_permutation_of_the_target_permutes_the_indices_and_nothing_else(gpu_device):
    source, target = RC.pair(4099, 4099)
    want = RC.reference_pair(4099, 4099)
    perm = np.random.default_rng(7).permutation(len(target))
    index, d2 = gpu_nearest(gpu_device, source, np.ascontiguousarray(target[perm]), RC.MAX_DISTANCE, RC.POSE_NEAR)
    assert np.array_equal(index < 0, want.index < 0)
    hit = index >= 0
    assert np.array_equal(perm[index[hit]], want.index[hit]) and d2.tobytes() == want.d2.tobytes()


def test_twenty_thousand_points(gpu_device):
    source, target = RC.scans("large")
    want = RC.reference_evaluation("large").neighbours
    assert want.distance_margin > RC.DISTANCE_MARGIN_MIN and want.gap_margin > RC.DISTANCE_MARGIN_MIN
    for cell_order in (True, False):
        same_neighbours(gpu_nearest(gpu_device, source, target, RC.MAX_DISTANCE, RC.POSE_NEAR, cell_order), want, cell_order)


def test_out_of_domain_and_non_finite_input_is_refused(gpu_device):
    import torch
    from pegasus_amd.registration import estimate_normals, nearest_neighbors
    source, target = (dev_t(gpu_device, a) for a in RC.pair(257, 4099))
    far = RC.rigid((0, 0, 0), (0.01 * 2.0 ** 30, 0, 0))
    with pytest.raises(ValueError, match="2\\^30"):
        nearest_neighbors(source, target, 0.01, far)
    with pytest.raises(ValueError, match="2\\^30"):
        nearest_neighbors(source, target, 0.02 / 2.0 ** 30)
    with pytest.raises(ValueError, match="2\\^30"):
        estimate_normals(target, 0.02 / 2.0 ** 30)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for which in (0, 1):
            clouds = [source.clone(), target.clone()]
            clouds[which][5, 1] = bad
            with pytest.raises(ValueError, match="finite"):
                nearest_neighbors(clouds[0], clouds[1], 0.01)
        q = target.clone()
        q[7, 2] = bad
        with pytest.raises(ValueError, match="finite"):
            estimate_normals(q, 0.01)
    with pytest.raises(ValueError):
        nearest_neighbors(source.double(), target, 0.01)
    with pytest.raises(ValueError):
        nearest_neighbors(source, target[:, :2], 0.01)


# ---- guard words
GUARD = 256
SENTINEL = 0x5A5A5A5A


def _guarded(dev, n, dtype, fill):
    import torch
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)


def _guards_ok(buf, n, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


@pytest.mark.parametrize("ns,nt", [(1, 1), (257, 255), (4099, 4099)])
def test_guards_short_workspaces_and_repeatability(gpu_device, ns, nt):
    """The entries themselves, on buffers with guard words on both sides: grid, order, correspondences and sums."""
    import ctypes as C
    import torch
    from pegasus_amd import _lib
    dev = gpu_device
    source, target = RC.pair(ns, nt)
    want = RC.reference_pair(ns, nt)
    s, t = dev_t(dev, source), dev_t(dev, target)
    T = (C.c_double * 16)(*RC.POSE_NEAR.reshape(-1))
    need = int(_lib.lib().pgr_nn_grid_build_workspace_bytes(nt))
    grid = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    g = grid[GUARD:]
    assert _lib.enqueue("pgr_nn_grid_build", dev, nt, _lib.ptr(t), RC.MAX_DISTANCE, _lib.ptr(g), need - 1) == \
        _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    torch.cuda.synchronize()
    assert bool((grid == 0xA5).all())                                              # nothing was launched
    assert _lib.enqueue("pgr_nn_grid_build", dev, nt, _lib.ptr(t), RC.MAX_DISTANCE, _lib.ptr(g), need) == _lib.PGR_OK
    need_o = int(_lib.lib().pgr_nn_source_order_workspace_bytes(ns))
    ows = torch.full((need_o + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    order = _guarded(dev, ns, torch.int32, SENTINEL)
    args = (ns, _lib.ptr(s), T, RC.MAX_DISTANCE, _lib.ptr(order[GUARD:]), _lib.ptr(ows[GUARD:]))
    assert _lib.enqueue("pgr_nn_source_order", dev, *args, need_o - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    torch.cuda.synchronize()
    assert bool((order == SENTINEL).all()) and bool((ows == 0xA5).all())
    assert _lib.enqueue("pgr_nn_source_order", dev, *args, need_o) == _lib.PGR_OK
    torch.cuda.synchronize()
    assert _guards_ok(order, ns, SENTINEL) and _guards_ok(ows, need_o, 0xA5) and _guards_ok(grid, need, 0xA5)
    assert np.array_equal(np.sort(order[GUARD:GUARD + ns].cpu().numpy()), np.arange(ns))

    def correspond(grid_bytes, with_order):
        index, d2 = _guarded(dev, ns, torch.int32, SENTINEL), _guarded(dev, ns, torch.float64, -7.0)
        status = _lib.enqueue("pgr_nn_correspond", dev, ns, _lib.ptr(s), _lib.ptr(order[GUARD:]) if with_order else None, T, nt,
                              RC.MAX_DISTANCE, _lib.ptr(g), grid_bytes, _lib.ptr(index[GUARD:]), _lib.ptr(d2[GUARD:]))
        torch.cuda.synchronize()
        assert _guards_ok(index, ns, SENTINEL) and _guards_ok(d2, ns, -7.0) and _guards_ok(grid, need, 0xA5)
        return status, index[GUARD:GUARD + ns], d2[GUARD:GUARD + ns]

    status, index, d2 = correspond(need - 1, True)
    assert status == _lib.PGR_ERR_WORKSPACE_TOO_SMALL and bool((index == SENTINEL).all()) and bool((d2 == -7.0).all())
    results = [correspond(need, with_order) for with_order in (True, False, True)]
    for status, index, d2 in results:
        assert status == _lib.PGR_OK
        same_neighbours((index.cpu().numpy().astype(np.int64), d2.cpu().numpy()), want, (ns, nt))
    index, d2 = results[0][1].contiguous(), results[0][2].contiguous()

    need_s = int(_lib.lib().pgr_icp_sums_workspace_bytes(ns))
    normals = dev_t(dev, RR.normals(target, 0.012)[0])

    def reduce(ws_bytes):
        out = _guarded(dev, RR.SUMS, torch.float64, -7.0)
        ws = torch.full((need_s + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        status = _lib.enqueue("pgr_icp_sums", dev, ns, _lib.ptr(s), T, _lib.ptr(index), _lib.ptr(d2), nt, _lib.ptr(t),
                              _lib.ptr(normals), _lib.ptr(out[GUARD:]), _lib.ptr(ws[GUARD:]), ws_bytes)
        torch.cuda.synchronize()
        assert _guards_ok(out, RR.SUMS, -7.0) and _guards_ok(ws, need_s, 0xA5)
        return status, out[GUARD:GUARD + RR.SUMS].cpu().numpy()

    status, out = reduce(need_s - 1)
    assert status == _lib.PGR_ERR_WORKSPACE_TOO_SMALL and (out == -7.0).all()
    (status_a, a), (status_b, b) = reduce(need_s), reduce(need_s)
    assert status_a == status_b == _lib.PGR_OK and a.tobytes() == b.tobytes()
    v, mag = RR.sums(source, target, normals.cpu().numpy(), RC.POSE_NEAR, want.index, want.d2)
    assert a[RR.COUNT] == v[RR.COUNT] and (np.abs(a - v) <= SUM_TOL * mag).all()


# ---- sums
def gpu_sums(dev, source, target, normals, T, distance=RC.MAX_DISTANCE):
    """The 48 sums of the GPU's own correspondences at T, twice: (first, second)."""
    from pegasus_amd import registration
    pair = registration._Pair(dev_t(dev, source), dev_t(dev, target), distance, "test", init=T,
                              target_normals=None if normals is None else dev_t(dev, normals))
    pair.correspond(T)
    out = []
    for _ in range(2):
        pair.sums.fill_(-7.0)
        pair.reduce(T)
        out.append(pair.sums.cpu().numpy())
    return out


def check_sums(got, v, mag, what):
    worst = 0.0
    for k in range(RR.SUMS):
        err = abs(got[k] - v[k])
        print(what, "sum", k, "gpu", got[k], "reference", v[k], "error / sum |terms|", err / mag[k] if mag[k] > 0 else err)
        assert err <= SUM_TOL * mag[k], (what, k, got[k], v[k], mag[k])             # (a sum of zeros is exactly 0)
        worst = max(worst, err / mag[k] if mag[k] > 0 else 0.0)
    assert got[RR.COUNT] == v[RR.COUNT] and float(got[RR.COUNT]).is_integer()
    return worst


@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("n", RC.SUM_SIZES)
def test_sums(gpu_device, n, with_normals):
    source, target = RC.pair(n, 4099)
    want = RC.reference_pair(n, 4099)
    normals = RR.normals(target, 0.012)[0] if with_normals else None
    v, mag = RR.sums(source, target, normals, RC.POSE_NEAR, want.index, want.d2)
    first, second = gpu_sums(gpu_device, source, target, normals, RC.POSE_NEAR)
    assert first.tobytes() == second.tobytes()
    check_sums(first, v, mag, (n, with_normals))
    if n >= 257:
        assert v[RR.COUNT] > 0 and (with_normals or (first[:27] == 0.0).all())
    assert (first[45:] == 0.0).all()


def test_sums_of_twenty_thousand_points(gpu_device):
    source, target = RC.scans("large")
    ev = RC.reference_evaluation("large")
    first, second = gpu_sums(gpu_device, source, target, RC.target_normals("large")[0], RC.POSE_NEAR)
    assert first.tobytes() == second.tobytes()
    check_sums(first, ev.sums, ev.abs_sums, "large")
    assert ev.sums[RR.COUNT] > 10000


def test_sums_without_correspondences_are_zero(gpu_device):
    source, target = RC.pair(4099, 4099)
    T = RC.rigid((0, 0, 0), (1.0, 0, 0))
    first, second = gpu_sums(gpu_device, source, target, RR.normals(target, 0.012)[0], T)
    assert (first == 0.0).all() and (second == 0.0).all()


# ---- normals
def check_normals(dev, pts, radius):
    import torch
    from pegasus_amd.registration import estimate_normals
    want, counts, ratio = RR.normals(pts, radius)
    got, got_counts = estimate_normals(dev_t(dev, pts), radius, return_counts=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(pts), 3) and got_counts.dtype == torch.int32
    got, got_counts = got.cpu().numpy(), got_counts.cpu().numpy().astype(np.int64)
    assert np.array_equal(got_counts, counts)
    few = counts < 3
    assert (got[few] == np.array([0.0, 0.0, 1.0])).all()
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() < 1e-14
    lead = np.abs(got).argmax(axis=1)
    assert (got[np.arange(len(got)), lead] > 0).all()                             # the sign rule, on every normal
    sure = ~few & (ratio > RC.EIGEN_GAP_MIN)
    dots = np.abs((got[sure] * want[sure]).sum(axis=1))
    if sure.any():
        print(len(pts), radius, "compared", int(sure.sum()), "least |n . n_ref| - 1 =", dots.min() - 1.0)
        assert dots.min() >= DOT_MIN
        # the same sign as the reference wherever the leading component is not contested
        mags = np.sort(np.abs(want[sure]), axis=1)
        clear = mags[:, 2] - mags[:, 1] > 1e-6
        assert ((got[sure] * want[sure]).sum(axis=1)[clear] > 0).all()
    return int(sure.sum()), int(few.sum())


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 4099])
def test_normals(gpu_device, n):
    pts = RC.pair(4099, n)[1]
    compared, few = check_normals(gpu_device, pts, 0.012 if n == 4099 else 0.03)
    if n >= 255:
        assert compared > n // 2
    if n < 3:
        assert few == n


def test_normals_of_the_icp_targets(gpu_device):
    for name in ("small",):
        want, counts, ratio = RC.target_normals(name)
        assert ratio.min() > RC.EIGEN_GAP_MIN and counts.min() >= 3
        compared, few = check_normals(gpu_device, RC.scans(name)[1], RC.ICP_CASES[name][1])
        assert compared == len(want) and few == 0


def test_normals_of_a_plane_and_of_lonely_points(gpu_device):
    from pegasus_amd.registration import estimate_normals
    pts, n = RC.planar_patch()
    lonely = np.vstack([pts, [[5.0, 5.0, 5.0]], [[-5.0, 5.0, 5.0]], [[-5.0, 5.0, 5.0]]]).astype(np.float32)
    got, counts = estimate_normals(dev_t(gpu_device, lonely), 0.01, return_counts=True)
    got, counts = got.cpu().numpy(), counts.cpu().numpy()
    assert counts[-3:].tolist() == [1, 2, 2] and (got[-3:] == np.array([0.0, 0.0, 1.0])).all()
    assert counts[:-3].min() >= 3 and (got[:-3] @ n > 1 - 1e-9).all()              # +n: its x and z lead, both positive
    check_normals(gpu_device, lonely, 0.01)
    flat = pts.copy()
    flat[:, 2] = np.float32(0.25)                                                  # exactly planar: exactly (0, 0, 1)
    got = estimate_normals(dev_t(gpu_device, flat), 0.01).cpu().numpy()
    assert (np.abs(got[:, 2]) > 1 - 1e-15).all() and np.abs(got[:, :2]).max() < 1e-12


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_normals_guards_and_short_workspace(gpu_device, n):
    import torch
    from pegasus_amd import _lib
    dev = gpu_device
    pts = RC.pair(4099, n)[1]
    want, counts, ratio = RR.normals(pts, 0.03)
    x = dev_t(dev, pts)
    need = int(_lib.lib().pgr_radius_normals_workspace_bytes(n))

    def call(ws_bytes):
        normals, got_counts = _guarded(dev, 3 * n, torch.float64, -7.0), _guarded(dev, n, torch.int32, SENTINEL)
        ws = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        status = _lib.enqueue("pgr_radius_normals", dev, n, _lib.ptr(x), 0.03, _lib.ptr(normals[GUARD:]), _lib.ptr(got_counts[GUARD:]),
                              _lib.ptr(ws[GUARD:]), ws_bytes)
        torch.cuda.synchronize()
        assert _guards_ok(normals, 3 * n, -7.0) and _guards_ok(got_counts, n, SENTINEL) and _guards_ok(ws, need, 0xA5)
        return status, normals[GUARD:GUARD + 3 * n].cpu().numpy().reshape(n, 3), got_counts[GUARD:GUARD + n].cpu().numpy()

    status, normals, got_counts = call(need - 1)
    assert status == _lib.PGR_ERR_WORKSPACE_TOO_SMALL and (normals == -7.0).all() and (got_counts == SENTINEL).all()
    status, normals, got_counts = call(need)
    assert status == _lib.PGR_OK and np.array_equal(got_counts.astype(np.int64), counts)
    sure = (counts >= 3) & (ratio > RC.EIGEN_GAP_MIN)
    assert (np.abs((normals[sure] * want[sure]).sum(axis=1)) >= DOT_MIN).all()


# ---- evaluate_registration and registration_icp
def check_result(got, want_index, fitness, rmse, what):
    index = want_index
    rows = np.nonzero(index >= 0)[0]
    pairs = got.correspondence_set.cpu().numpy()
    assert got.correspondence_set.dtype.is_floating_point is False and pairs.dtype == np.int64 and pairs.shape == (len(rows), 2)
    assert np.array_equal(pairs[:, 0], rows) and np.array_equal(pairs[:, 1], index[rows]), what
    assert got.fitness == fitness, what
    print(what, "rmse", got.inlier_rmse, "reference", rmse)
    assert abs(got.inlier_rmse - rmse) <= RMSE_RTOL * rmse, what


def test_evaluate_registration(gpu_device):
    from pegasus_amd.registration import evaluate_registration
    source, target = RC.scans("small")
    ev = RC.reference_evaluation("small")
    got = evaluate_registration(dev_t(gpu_device, source), dev_t(gpu_device, target), RC.MAX_DISTANCE, RC.POSE_NEAR)
    assert np.array_equal(got.transformation, RC.POSE_NEAR) and got.iterations == 0
    check_result(got, ev.neighbours.index, ev.fitness, ev.rmse, "evaluate")
    assert 0.5 < got.fitness < 1.0


@pytest.mark.parametrize("name,estimation", [("small", "point_to_plane"), ("small", "point_to_point"), ("large", "point_to_plane")])
def test_registration_icp(gpu_device, name, estimation):
    from pegasus_amd.registration import registration_icp
    source, target = RC.scans(name)
    want = RC.reference_icp(name, estimation)
    assert want.distance_margin > RC.DISTANCE_MARGIN_MIN and want.gap_margin > RC.DISTANCE_MARGIN_MIN
    got = registration_icp(dev_t(gpu_device, source), dev_t(gpu_device, target), RC.MAX_DISTANCE, estimation=estimation,
                           target_normals=dev_t(gpu_device, RC.target_normals(name)[0]))
    diff = float(np.abs(got.transformation - want.transformation).max())
    print(name, estimation, "iterations", got.iterations, want.iterations, "largest |T - T_ref| =", diff, "allowed", RC.T_TOL)
    assert got.iterations == want.iterations
    check_result(got, want.index, want.fitness, want.rmse, (name, estimation))
    assert diff <= RC.T_TOL


def test_registration_icp_estimates_the_normals_it_needs(gpu_device):
    from pegasus_amd.registration import registration_icp
    source, target = RC.scans("small")
    want = RC.reference_icp("small", "point_to_plane")
    got = registration_icp(dev_t(gpu_device, source), dev_t(gpu_device, target), RC.MAX_DISTANCE, normals_radius=0.012)
    # the device's normals agree with the reference's to 1e-5 rad, not to the bit: the pose to 1e-7, the decisions all the same
    assert got.iterations == want.iterations and np.abs(got.transformation - want.transformation).max() < 1e-7
    check_result(got, want.index, want.fitness, want.rmse, "estimated normals")


def test_no_iterations_is_the_evaluation_at_init(gpu_device):
    from pegasus_amd.registration import registration_icp
    source, target = RC.scans("small")
    ev = RC.reference_evaluation("small")
    for estimation in RC.ESTIMATIONS:
        got = registration_icp(dev_t(gpu_device, source), dev_t(gpu_device, target), RC.MAX_DISTANCE, RC.POSE_NEAR, estimation,
                               dev_t(gpu_device, RC.target_normals("small")[0]), max_iteration=0)
        assert got.iterations == 0 and np.array_equal(got.transformation, RC.POSE_NEAR)
        check_result(got, ev.neighbours.index, ev.fitness, ev.rmse, estimation)


def test_without_correspondences_the_pose_stays(gpu_device):
    from pegasus_amd.registration import registration_icp
    source, target = RC.scans("small")
    init = RC.rigid((5, 0, 0), (1.0, 0, 0))
    for estimation in RC.ESTIMATIONS:
        got = registration_icp(dev_t(gpu_device, source), dev_t(gpu_device, target), RC.MAX_DISTANCE, init, estimation,
                               dev_t(gpu_device, RC.target_normals("small")[0]))
        assert np.array_equal(got.transformation, init) and got.fitness == 0.0 and got.inlier_rmse == 0.0
        assert got.iterations == 1 and tuple(got.correspondence_set.shape) == (0, 2)


def test_a_singular_system_gives_the_identity_update(gpu_device):
    from pegasus_amd.registration import registration_icp
    rng = np.random.default_rng(3)
    flat = np.concatenate([rng.uniform(-0.05, 0.05, (500, 2)), np.full((500, 1), 0.02)], axis=1).astype(np.float32)
    lifted = flat + np.array([0, 0, 0.001], dtype=np.float32)
    up = np.tile([0.0, 0.0, 1.0], (500, 1))
    want = RR.icp(lifted, flat, 0.005, None, "point_to_plane", up)
    assert np.array_equal(want.transformation, np.eye(4)) and want.fitness == 1.0 and want.iterations == 1
    got = registration_icp(dev_t(gpu_device, lifted), dev_t(gpu_device, flat), 0.005, target_normals=dev_t(gpu_device, up))
    assert np.array_equal(got.transformation, np.eye(4)) and got.fitness == 1.0 and got.iterations == 1
    assert abs(got.inlier_rmse - want.rmse) <= RMSE_RTOL * want.rmse


# ---- models
def _model(dev, pts, seed=11):
    """A model over ``pts`` with random splats and SH; about a tenth of the opacities activate below 0.5."""
    from pegasus_amd.gaussian_model import GaussianModel
    n = len(pts)
    rng = np.random.default_rng(seed)
    rot = rng.normal(size=(n, 4))
    return GaussianModel.from_arrays(np.array(pts), rng.normal(size=(n, 1, 3)), rng.normal(size=(n, 15, 3)),
                                     rng.normal(1.3, 1.0, (n, 1)), rng.normal(-4.0, 0.3, (n, 3)),
                                     rot / np.linalg.norm(rot, axis=1, keepdims=True), device=dev)


ROW_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def test_merge_models_poses_about_the_origin(gpu_device):
    import torch
    from pegasus_amd import compose
    from pegasus_amd.registration import merge_models
    source, target = RC.scans("small")
    source = source + np.array([0.5, -0.3, 0.2], dtype=np.float32)                 # a mean far from the origin
    a, b = _model(gpu_device, target, 1), _model(gpu_device, source, 2)
    T = RC.rigid((20.0, -30.0, 10.0), (0.05, 0.02, -0.04))
    before = {k: getattr(b, k).clone() for k in ROW_ATTRS}
    merged = merge_models(a, b, T)
    na, nb = len(target), len(source)
    for k in ROW_ATTRS:
        assert getattr(merged, k).shape[0] == na + nb and torch.equal(getattr(merged, k)[:na], getattr(a, k)), k
        assert torch.equal(getattr(b, k), before[k]), k                            # the source model is left as it was
    for k in ("_features_dc", "_opacity", "_scaling"):
        assert torch.equal(getattr(merged, k)[na:], getattr(b, k)), k
    assert merged.active_sh_degree == a.active_sh_degree and merged.max_sh_degree == a.max_sh_degree
    x = source.astype(np.float64)
    want = x @ T[:3, :3].T + T[:3, 3]
    # float32: R rounded, three products and three sums, each within 2^-24 of sum |R_kj x_j| + |t_k| <= sqrt(3) max|x| + max|t|
    tol = 8 * 2.0 ** -24 * (np.sqrt(3.0) * np.abs(x).max() + np.abs(T[:3, 3]).max())
    got = merged._xyz[na:].cpu().numpy().astype(np.float64)
    assert np.abs(got - want).max() <= tol
    mean = x.mean(axis=0)
    about_mean = (x - mean) @ T[:3, :3].T + mean + T[:3, 3]
    assert np.abs(got - about_mean).max() > 0.1                                    # not GaussianModel.apply_transformation's
    # orientations and SH: the existing pose kernel with centre zero
    xyz, rot, rest = torch.empty_like(b._xyz), torch.empty_like(b._rotation), torch.empty_like(b._features_rest)
    compose.compose_object(b._xyz.contiguous(), b._rotation.contiguous(), b._features_rest.contiguous(),
                           compose.make_pose(T, np.zeros(3)), xyz, rot, rest)
    assert torch.equal(merged._xyz[na:], xyz) and torch.equal(merged._rotation[na:], rot)
    assert torch.equal(merged._features_rest[na:], rest)
    assert not torch.equal(rot, b._rotation) and not torch.equal(rest, b._features_rest)


def test_merge_models_drops_the_overlap(gpu_device):
    import torch
    from pegasus_amd.registration import merge_models
    source, target = RC.scans("small")
    a, b = _model(gpu_device, target, 1), _model(gpu_device, source, 2)
    full = merge_models(a, b, RC.KNOWN_POSE)
    na = len(target)
    posed = full._xyz[na:].cpu().numpy()
    for d in (0.002, 0.004):
        nb = RR.nearest(posed, target, d)
        assert nb.distance_margin > RC.DISTANCE_MARGIN_MIN
        keep = nb.index < 0
        assert 0 < keep.sum() < len(source)
        merged = merge_models(a, b, RC.KNOWN_POSE, drop_within=d)
        for k in ROW_ATTRS:
            assert getattr(merged, k).shape[0] == na + int(keep.sum()), k
            assert torch.equal(getattr(merged, k)[:na], getattr(a, k)), k
            assert torch.equal(getattr(merged, k)[na:], getattr(full, k)[na:][torch.from_numpy(keep).to(gpu_device)]), k
    with pytest.raises(ValueError):
        merge_models(a, b, RC.KNOWN_POSE, drop_within=0.0)


def test_register_models(gpu_device):
    from pegasus_amd.registration import register_models, registration_icp
    source, target = RC.scans("small")
    a, b = _model(gpu_device, target, 1), _model(gpu_device, source, 2)
    got = register_models(a, b, np.eye(4), RC.MAX_DISTANCE, estimation="point_to_point", min_opacity=0.5)
    keep_a, keep_b = (m.get_opacity[:, 0] >= 0.5 for m in (a, b))
    assert 0.8 * len(target) < int(keep_a.sum()) < len(target)
    want = registration_icp(b._xyz[keep_b].contiguous(), a._xyz[keep_a].contiguous(), RC.MAX_DISTANCE, estimation="point_to_point")
    assert np.array_equal(got.transformation, want.transformation) and got.iterations == want.iterations > 1
    assert got.fitness == want.fitness and got.correspondence_set.shape == want.correspondence_set.shape
    plane = register_models(a, b, np.eye(4), RC.MAX_DISTANCE, normals_radius=0.012)
    assert RR.rotation_angle_deg(plane.transformation[:3, :3], RC.KNOWN_POSE[:3, :3]) < RC.POSE_DEG_MAX
    assert np.linalg.norm(plane.transformation[:3, 3] - RC.KNOWN_POSE[:3, 3]) < RC.POSE_M_MAX


def test_command_line_round_trip(gpu_device, tmp_path, capsys):
    from pegasus_amd import registration
    from pegasus_amd.gaussian_model import GaussianModel
    source, target = RC.scans("small")
    a, b = _model(gpu_device, target, 1), _model(gpu_device, source, 2)
    up, down, out = tmp_path / "up.ply", tmp_path / "down.ply", tmp_path / "fused" / "fused.ply"
    a.save_ply(up)
    b.save_ply(down)
    np.savetxt(tmp_path / "T.txt", np.eye(4))
    argv = ["--target", str(up), "--source", str(down), "--max_distance", str(RC.MAX_DISTANCE), "--out", str(out)]
    assert registration.main(argv + ["--init", str(tmp_path / "T.txt"), "--estimation", "point_to_point", "--drop_within", "0.002"]) == 0
    text = capsys.readouterr().out
    assert "before: fitness" in text and "after" in text and "inlier RMSE" in text
    want = registration.register_models(a, b, np.eye(4), RC.MAX_DISTANCE, min_opacity=0.5, estimation="point_to_point")
    T = np.loadtxt(out.parent / "transformation_b2a.txt")
    assert T.shape == (4, 4) and np.array_equal(T, want.transformation)            # (point to point repeats to the bit)
    fused = GaussianModel(3, gpu_device)
    fused.load_ply(out)
    merged = registration.merge_models(a, b, want.transformation, drop_within=0.002)
    assert len(target) < fused._xyz.shape[0] == merged._xyz.shape[0] < len(target) + len(source)
    assert np.array_equal(fused._xyz.cpu().numpy(), merged._xyz.cpu().numpy())
    # picked points instead of a matrix, point to plane: the known pose, within what the reference itself reaches
    picks = np.random.default_rng(4).uniform(-0.05, 0.05, (6, 3))
    inv = np.linalg.inv(RC.KNOWN_POSE)
    np.savetxt(tmp_path / "a.txt", picks)
    np.savetxt(tmp_path / "b.txt", picks @ inv[:3, :3].T + inv[:3, 3])
    points = ["--points_target", str(tmp_path / "a.txt"), "--points_source", str(tmp_path / "b.txt")]
    assert registration.main(argv + points + ["--normals_radius", "0.012"]) == 0
    T = np.loadtxt(out.parent / "transformation_b2a.txt")
    assert RR.rotation_angle_deg(T[:3, :3], RC.KNOWN_POSE[:3, :3]) < RC.POSE_DEG_MAX
    assert np.linalg.norm(T[:3, 3] - RC.KNOWN_POSE[:3, 3]) < RC.POSE_M_MAX
    # picked points that say the scans differ in scale
    np.savetxt(tmp_path / "b.txt", 1.05 * (picks @ inv[:3, :3].T + inv[:3, 3]))
    with pytest.raises(SystemExit, match="scale of 0.952"):
        registration.main(argv + points)
