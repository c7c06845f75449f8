"""The radius-outlier filter on the GPU (pegasus_amd/outliers.py over pgr_radius_count) against the float64 brute force of
tests/outlier_reference.py: integer equality on every point, no tolerance.  Sizes around the block, strictness and the float64
radius, cell walls, table load, the cap, two sizes beyond one block of everything, guard words, and the model layer
(denoise_point_cloud, load_ply(clean_pcd=True), mask_points with an optimizer, the command line)."""
import copy
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import outlier_cases as OC               # noqa: E402
import outlier_reference as OR           # noqa: E402

pytestmark = pytest.mark.gpu


def gpu_counts(dev, pts, radius, cap=None):
    import torch
    from pegasus_amd.outliers import radius_neighbor_count
    got = radius_neighbor_count(torch.from_numpy(np.array(pts)).to(dev), radius, cap)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(pts),)
    return got.cpu().numpy().astype(np.int64)


def same(got, want, what=""):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), np.asarray(want)[bad[:8]].tolist())


@pytest.mark.parametrize("cap", [None, 17])
@pytest.mark.parametrize("n", OC.SIZES)
def test_sizes(gpu_device, n, cap):
    pts = np.ascontiguousarray(OC.random_cloud()[:n])
    want = OC.reference("random", 0.05)[0] if n == 4099 else OR.neighbor_counts(pts, 0.05)[0]
    same(gpu_counts(gpu_device, pts, 0.05, cap), want if cap is None else np.minimum(want, cap), (n, cap))


@pytest.mark.parametrize("nb_points,radius", OC.SETTINGS)
def test_random_cloud_at_the_reference_settings(gpu_device, nb_points, radius):
    import torch
    from pegasus_amd.outliers import radius_outlier_mask, remove_radius_outlier
    pts = OC.random_cloud()
    want = OC.reference("random", radius)[0]
    same(gpu_counts(gpu_device, pts, radius), want, radius)
    t = torch.from_numpy(pts.copy()).to(gpu_device)
    mask = radius_outlier_mask(t, nb_points, radius)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), want > nb_points)
    kept, ind = remove_radius_outlier(t, nb_points, radius)
    assert ind.dtype == torch.int64 and np.array_equal(ind.cpu().numpy(), np.nonzero(want > nb_points)[0])
    assert torch.equal(kept, t[ind])
    assert int(mask.sum()) == dict(zip(OC.SETTINGS, (3495, 3939, 4047)))[(nb_points, radius)]


def test_comparison_is_strict_and_the_radius_is_float64(gpu_device):
    pts, radius = OC.tie_345()
    assert gpu_counts(gpu_device, pts, radius).tolist() == [1, 1]
    assert gpu_counts(gpu_device, pts, float(np.nextafter(radius, np.inf))).tolist() == [2, 2]
    for pair, r_in, r_out in OC.knife_pairs():
        assert gpu_counts(gpu_device, pair, r_in).tolist() == [2, 2], (pair, r_in)
        assert gpu_counts(gpu_device, pair, r_out).tolist() == [1, 1], (pair, r_out)


def test_cell_walls(gpu_device):
    r = OC.R_LATTICE
    assert gpu_counts(gpu_device, OC.lattice(5, r), r).tolist() == [1] * 125
    near = gpu_counts(gpu_device, OC.lattice(5, r * (1 - 2.0 ** -20)), r)
    same(near, 1 + OC.lattice_axis_neighbours(5), "lattice just inside r")
    assert sorted(set(near.tolist())) == [4, 5, 6, 7]
    for centre in OC.constellation_centres():
        pts, want = OC.constellation(OC.RADIUS_CONSTELLATION, centre)
        got = gpu_counts(gpu_device, pts, OC.RADIUS_CONSTELLATION)
        same(got, want, centre)
        assert got[13] == 27


@pytest.mark.parametrize("cap", [None, 1, 17, 300, 301])
def test_coincident_points(gpu_device, cap):
    assert gpu_counts(gpu_device, OC.coincident(300), 1e-3, cap).tolist() == [min(300, cap or 300)] * 300


@pytest.mark.parametrize("floater", [False, True])
def test_table_load(gpu_device, floater):
    pts = OC.table_load(floater)
    assert gpu_counts(gpu_device, pts, OC.R_LATTICE).tolist() == [1] * len(pts)


def test_cap(gpu_device):
    pts = OC.random_cloud()
    assert gpu_counts(gpu_device, pts, 0.05, cap=1).tolist() == [1] * len(pts)
    for nb_points, radius in OC.SETTINGS:
        exact = gpu_counts(gpu_device, pts, radius)
        capped = gpu_counts(gpu_device, pts, radius, cap=nb_points + 1)
        same(capped, np.minimum(exact, nb_points + 1), (nb_points, radius))
        assert np.array_equal(capped > nb_points, exact > nb_points)


def test_twenty_thousand_points(gpu_device):
    want, margin = OC.reference("uniform", OC.RADIUS_UNIFORM)
    assert margin > OC.MARGIN_MIN
    same(gpu_counts(gpu_device, OC.uniform_cloud(), OC.RADIUS_UNIFORM), want)
    same(gpu_counts(gpu_device, OC.uniform_cloud(), OC.RADIUS_UNIFORM, 17), np.minimum(want, 17))


def test_two_hundred_thousand_points_and_a_permutation(gpu_device):
    pts, rows = OC.plane_cloud()
    want, margin = OC.reference("plane", OC.RADIUS_PLANE)
    assert margin > OC.MARGIN_MIN
    got = gpu_counts(gpu_device, pts, OC.RADIUS_PLANE)
    same(got[rows], want, "query rows")
    perm = np.random.default_rng(7).permutation(len(pts))
    same(gpu_counts(gpu_device, pts[perm], OC.RADIUS_PLANE), got[perm], "row permutation")
    same(gpu_counts(gpu_device, pts, OC.RADIUS_PLANE, 17), np.minimum(got, 17), "capped")


def test_out_of_domain_points_are_refused(gpu_device):
    import torch
    from pegasus_amd.outliers import radius_neighbor_count
    pts = torch.from_numpy(OC.random_cloud().copy()).to(gpu_device)
    with pytest.raises(ValueError, match="2\\^30"):
        radius_neighbor_count(pts, 1800.0 / 2.0 ** 30)
    edge = 1801.0 / 2.0 ** 30                                   # cell indices up to 2^30 / 1.0008
    same(gpu_counts(gpu_device, OC.random_cloud(), edge), OR.neighbor_counts(OC.random_cloud(), edge)[0], "domain edge")
    for bad in (float("nan"), float("inf"), -float("inf")):
        q = pts.clone()
        q[5, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            radius_neighbor_count(q, 0.05)
    with pytest.raises(ValueError):
        radius_neighbor_count(pts.double(), 0.05)
    with pytest.raises(ValueError):
        radius_neighbor_count(pts[:, :2], 0.05)


# ---- bit for bit
GUARD = 256
SENTINEL = 0x5A5A5A5A


def _guarded_call(dev, pts, radius, cap, short=0):
    """pgr_radius_count on buffers with guard words on both sides: (status, counts, counts guards ok, workspace guards ok)."""
    import torch
    from pegasus_amd import _lib
    n = len(pts)
    x = torch.from_numpy(np.array(pts)).to(dev)
    need = int(_lib.lib().pgr_radius_count_workspace_bytes(n))
    counts = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    ws = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    status = _lib.enqueue("pgr_radius_count", dev, n, _lib.ptr(x), radius, cap, _lib.ptr(counts[GUARD:]), _lib.ptr(ws[GUARD:]),
                          need - short)
    torch.cuda.synchronize()
    counts_ok = bool((counts[:GUARD] == SENTINEL).all()) and bool((counts[GUARD + n:] == SENTINEL).all())
    ws_ok = bool((ws[:GUARD] == 0xA5).all()) and bool((ws[GUARD + need:] == 0xA5).all())
    return status, counts[GUARD:GUARD + n].cpu().numpy().astype(np.int64), counts_ok, ws_ok


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_guards_and_repeatability(gpu_device, n):
    from pegasus_amd import _lib
    pts = OC.random_cloud()[:n]
    want = OR.neighbor_counts(np.ascontiguousarray(pts), 0.05)[0]
    first = _guarded_call(gpu_device, pts, 0.05, n)
    second = _guarded_call(gpu_device, pts, 0.05, n)
    for status, counts, counts_ok, ws_ok in (first, second):
        assert status == _lib.PGR_OK and counts_ok and ws_ok
        same(counts, want, n)
    assert first[1].tobytes() == second[1].tobytes()
    status, counts, counts_ok, ws_ok = _guarded_call(gpu_device, pts, 0.05, n, short=1)
    assert status == _lib.PGR_ERR_WORKSPACE_TOO_SMALL and counts_ok and ws_ok
    assert (counts == SENTINEL).all()                                              # nothing was launched


# ---- the model layer
def _model(dev, pts):
    """A model over ``pts`` whose opacity column is the row number."""
    from pegasus_amd.gaussian_model import GaussianModel
    n = len(pts)
    rng = np.random.default_rng(11)
    rot = rng.normal(size=(n, 4))
    return GaussianModel.from_arrays(np.array(pts), rng.normal(size=(n, 1, 3)), rng.normal(size=(n, 15, 3)),
                                     np.arange(n, dtype=np.float32)[:, None], rng.normal(-4.0, 0.3, (n, 3)),
                                     rot / np.linalg.norm(rot, axis=1, keepdims=True), device=dev)


def _rows(m):
    return m._opacity.detach()[:, 0].cpu().numpy().astype(np.int64)


ROW_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def test_denoise_point_cloud(gpu_device):
    m = _model(gpu_device, OC.random_cloud())
    m.denoise_point_cloud()
    want = np.nonzero(OC.reference("random", 0.05)[0] > 16)[0]
    assert np.array_equal(_rows(m), want)
    assert np.array_equal(m.get_xyz.cpu().numpy(), OC.random_cloud()[want])
    for attr in ROW_ATTRS:
        assert getattr(m, attr).shape[0] == len(want)
    m = _model(gpu_device, OC.random_cloud())
    m.denoise_point_cloud(nb_points=50, radius=0.1, debug=True)
    assert np.array_equal(_rows(m), np.nonzero(OC.reference("random", 0.1)[0] > 50)[0])


def test_denoise_point_cloud_filters_the_posed_positions(gpu_device):
    import torch
    from scipy.spatial.transform import Rotation as Rot
    T = np.eye(4)
    T[:3, :3] = Rot.from_rotvec([0.3, -0.5, 0.2]).as_matrix()
    T[:3, 3] = (0.4, -0.1, 0.25)
    T = torch.tensor(T, dtype=torch.float32, device=gpu_device)
    a, b = _model(gpu_device, OC.random_cloud()), _model(gpu_device, OC.random_cloud())
    b.apply_transformation(T)
    posed = b.get_xyz.cpu().numpy()
    assert not np.array_equal(posed, OC.random_cloud())
    mask, margin = OR.keep_mask(posed, 16, 0.05)
    assert margin > OC.MARGIN_MIN
    a.apply_transformation(T)                                   # recorded, not applied yet
    a.denoise_point_cloud()
    assert np.array_equal(_rows(a), np.nonzero(mask)[0])
    assert np.array_equal(a.get_xyz.cpu().numpy(), posed[mask])


def test_load_ply_clean_pcd(gpu_device, tmp_path):
    import torch
    from pegasus_amd.gaussian_model import GaussianModel
    path = tmp_path / "point_cloud.ply"
    _model(gpu_device, OC.random_cloud()).save_ply(path)
    cleaned, full = GaussianModel(3, gpu_device), GaussianModel(3, gpu_device)
    cleaned.load_ply(path, clean_pcd=True)
    full.load_ply(path)
    mask = OC.reference("random", 0.03)[0] > 16
    full.mask_points(torch.from_numpy(mask).to(gpu_device))
    assert np.array_equal(_rows(cleaned), np.nonzero(mask)[0])
    for attr in ROW_ATTRS:
        assert torch.equal(getattr(cleaned, attr), getattr(full, attr)), attr
    assert cleaned.active_sh_degree == full.active_sh_degree == 3


def test_denoise_with_an_optimizer_equals_prune_points(gpu_device):
    import torch
    from pegasus_amd.train import OPTIMIZATION_DEFAULTS, _Options
    m = _model(gpu_device, OC.random_cloud())
    m.spatial_lr_scale = 1.0
    m.training_setup(_Options(None, OPTIMIZATION_DEFAULTS))
    gen = torch.Generator(device="cpu").manual_seed(3)
    for attr in ROW_ATTRS:
        p = getattr(m, attr)
        p.grad = (1e-3 * torch.randn(p.shape, generator=gen)).to(gpu_device)
    m.optimizer.step()
    n = m.get_xyz.shape[0]
    m.xyz_gradient_accum = torch.rand((n, 1), generator=gen).to(gpu_device)
    m.denom = torch.randint(0, 9, (n, 1), generator=gen).float().to(gpu_device)
    m.max_radii2D = torch.rand((n,), generator=gen).to(gpu_device)
    other = copy.deepcopy(m)
    mask, margin = OR.keep_mask(m.get_xyz.detach().cpu().numpy(), 16, 0.05)      # (the step moved the positions)
    assert margin > OC.MARGIN_MIN and 0 < mask.sum() < n
    m.denoise_point_cloud()
    other.prune_points(torch.from_numpy(~mask).to(gpu_device))
    assert m.get_xyz.shape[0] == int(mask.sum())
    for (ga, gb) in zip(m.optimizer.param_groups, other.optimizer.param_groups):
        pa, pb = ga["params"][0], gb["params"][0]
        assert ga["name"] == gb["name"] and isinstance(pa, torch.nn.Parameter) and pa.requires_grad
        assert torch.equal(pa.detach(), pb.detach()), ga["name"]
        sa, sb = m.optimizer.state[pa], other.optimizer.state[pb]
        for k in ("exp_avg", "exp_avg_sq"):
            assert sa[k].shape == pa.shape and torch.equal(sa[k], sb[k]) and float(sa[k].abs().max()) > 0, (ga["name"], k)
    for name, attr in m._PARAM_NAMES:
        assert getattr(m, attr) is [g for g in m.optimizer.param_groups if g["name"] == name][0]["params"][0]
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(m, k), getattr(other, k)) and getattr(m, k).shape[0] == int(mask.sum()), k


def test_command_line_round_trip(gpu_device, tmp_path, capsys):
    from pegasus_amd import outliers
    from pegasus_amd.ply_io import read_ply_vertices
    src, dst = tmp_path / "in.ply", tmp_path / "out" / "cleaned.ply"
    _model(gpu_device, OC.random_cloud()).save_ply(src)
    assert outliers.main(["--in", str(src), "--out", str(dst)]) == 0
    want = np.nonzero(OC.reference("random", 0.03)[0] > 16)[0]
    assert f"kept {len(want)} of 4099" in capsys.readouterr().out
    before, after = read_ply_vertices(src), read_ply_vertices(dst)
    assert after.dtype == before.dtype and np.array_equal(after["opacity"].astype(np.int64), want)
    assert after.tobytes() == before[want].tobytes()
    assert outliers.main(["--in", str(src), "--out", str(dst), "--nb_points", "50", "--radius", "0.1"]) == 0
    assert len(read_ply_vertices(dst)) == int((OC.reference("random", 0.1)[0] > 50).sum())
