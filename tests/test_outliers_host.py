"""The radius-outlier filter without a device: the two entries are declared, exported and prototyped; the size function and
every argument check that pgr_radius_count decides on the host; the float64 reference (tests/outlier_reference.py) against
hand-worked answers and against scipy's exact k-d tree; and the margin census: no random fixture sits near a tie."""
import ctypes as C
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))

import outlier_cases as OC               # noqa: E402
import outlier_reference as OR           # noqa: E402
from pegasus_amd import outliers         # noqa: E402,F401  (without the feature nothing in this file runs)

NAMES = ("pgr_radius_count_workspace_bytes", "pgr_radius_count")
FAKE = 0x10000                           # a non-NULL, 16-byte aligned address that is never dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import _lib, build
    build.build()
    return _lib.lib()


def test_symbols_are_declared_exported_and_prototyped(lib):
    from pegasus_amd import _lib
    header = (ROOT / "include" / "pegasus_raster.h").read_text()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert _lib.SYMBOLS[NAMES[0]] == (C.c_size_t, [C.c_int32])
    res, args = _lib.SYMBOLS[NAMES[1]]
    assert res is C.c_int32 and args[2] is C.c_double and len(args) == 8
    assert lib.pgr_abi_version() == 4


def test_workspace_size(lib):
    size = lib.pgr_radius_count_workspace_bytes
    assert size(-1) == 0 and size(-(1 << 31)) == 0
    assert size(1) > 0
    ns = [0, 1, 2, 127, 128, 129, 255, 256, 257, 4099, 65536, 65537, 1 << 20, (1 << 20) + 1, 2_000_000, (1 << 31) - 1]
    sizes = [size(n) for n in ns]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert all(s % 256 == 0 for s in sizes)
    # storage follows the number of points: a table of at most 4 n slots of 20 bytes, 4 + 16 bytes per point
    assert size(2_000_000) <= 2_000_000 * (4 * 20 + 20) + 5 * 256


def _call(lib, n=4, xyz=FAKE, radius=0.05, cap=17, counts=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.pgr_radius_count_workspace_bytes(max(n, 0))
    return lib.pgr_radius_count(n, xyz, radius, cap, counts, ws, ws_bytes, None)


def test_invalid_arguments_are_refused_on_the_host(lib):
    from pegasus_amd import _lib
    bad = _lib.PGR_ERR_INVALID_ARGUMENT
    assert _call(lib, n=-1) == bad
    assert _call(lib, cap=0) == bad and _call(lib, cap=-5) == bad
    for radius in (0.0, -0.05, math.nan, math.inf, -math.inf):
        assert _call(lib, radius=radius) == bad, radius
        assert _call(lib, n=0, radius=radius) == bad, radius
    assert _call(lib, xyz=None) == bad
    assert _call(lib, counts=None) == bad
    assert _call(lib, ws=None) == bad
    assert _call(lib, n=0, cap=0) == bad


def test_short_workspace_is_refused_and_no_points_is_ok(lib):
    from pegasus_amd import _lib
    for n in (1, 257, 4099):
        need = lib.pgr_radius_count_workspace_bytes(n)
        assert _call(lib, n=n, ws_bytes=need - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
        assert _call(lib, n=n, ws_bytes=0) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert _call(lib, n=0) == _lib.PGR_OK
    assert _call(lib, n=0, xyz=None, counts=None, ws=None, ws_bytes=0) == _lib.PGR_OK


def test_python_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    pts = torch.zeros((4, 3))
    for fn, args in ((outliers.radius_neighbor_count, (0.05,)), (outliers.radius_outlier_mask, (16, 0.05)),
                     (outliers.remove_radius_outlier, (16, 0.05))):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            fn(pts, *args)
    with pytest.raises(ValueError):
        outliers.radius_outlier_mask(pts, 0, 0.05)
    with pytest.raises(ValueError):
        outliers.radius_outlier_mask(pts, 16, 0.0)
    with pytest.raises(ValueError):
        outliers.radius_outlier_mask(pts, 16, -1.0)


def test_model_and_mesh_cli_take_the_filter():
    import inspect
    from pegasus_amd import mesh
    from pegasus_amd.gaussian_model import GaussianModel
    sig = inspect.signature(GaussianModel.denoise_point_cloud)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [("nb_points", 16), ("radius", 0.05), ("debug", False)]
    base = ["-m", "model", "--out", "out", "--obj_id", "1"]
    assert mesh._parser().parse_args(base + ["--clean_pcd"]).clean_pcd is True
    assert mesh._parser().parse_args(base).clean_pcd is False


# ---- the reference against hand-worked answers
def test_reference_is_strict_on_the_3_4_5_tie():
    pts, radius = OC.tie_345()
    assert radius * radius == 25 * 2.0 ** -14                                      # d2 and r2 are the same float64
    assert OR.neighbor_counts(pts, radius)[0].tolist() == [1, 1]
    assert OR.neighbor_counts(pts, np.nextafter(radius, np.inf))[0].tolist() == [2, 2]
    assert OR.neighbor_counts(pts, np.nextafter(radius, 0.0))[0].tolist() == [1, 1]


def test_reference_counts_coincident_points():
    counts, margin = OR.neighbor_counts(OC.coincident(300), 1e-3)
    assert counts.tolist() == [300] * 300 and margin == np.inf
    assert OR.keep_mask(OC.coincident(300), 299, 1e-3)[0].all()
    assert not OR.keep_mask(OC.coincident(300), 300, 1e-3)[0].any()


def test_reference_on_the_constellation_and_the_lattices():
    pts, want = OC.constellation(2.0 ** -4, (0.0, 0.0, 0.0))
    assert want[13] == 27 and sorted(set(want.tolist())) == [8, 12, 18, 27]
    assert np.array_equal(OR.neighbor_counts(pts, 2.0 ** -4)[0], want)
    for centre in OC.constellation_centres():
        pts, want = OC.constellation(OC.RADIUS_CONSTELLATION, centre)
        assert np.array_equal(OR.neighbor_counts(pts, OC.RADIUS_CONSTELLATION)[0], want), centre
    r = OC.R_LATTICE
    assert OR.neighbor_counts(OC.lattice(5, r), r)[0].tolist() == [1] * 125                 # neighbours exactly r away
    near = OR.neighbor_counts(OC.lattice(5, r * (1 - 2.0 ** -20)), r)[0]
    assert np.array_equal(near, 1 + OC.lattice_axis_neighbours(5)) and sorted(set(near.tolist())) == [4, 5, 6, 7]
    assert OR.neighbor_counts(OC.table_load(True), r)[0].tolist() == [1] * 4097


def test_knife_edge_radii_decide_the_pair():
    pairs = OC.knife_pairs()
    assert len(pairs) == 16
    for pts, r_in, r_out in pairs:
        assert OR.neighbor_counts(pts, r_in)[0].tolist() == [2, 2]
        assert OR.neighbor_counts(pts, r_out)[0].tolist() == [1, 1]
        assert np.float32(r_in) == np.float32(r_out)                                # float32 cannot tell the two radii apart


def test_random_cloud_is_as_described():
    pts = OC.random_cloud()
    assert pts.shape == (4099, 3) and pts.dtype == np.float32 and pts[-1].tolist() == [900.0, -1800.0, 400.0]
    # (the issue's 3 528 / 3 956 / 4 049 are another seed of the same construction)
    kept = [int((OC.reference("random", r)[0] > nb).sum()) for nb, r in OC.SETTINGS]
    assert kept == [3495, 3939, 4047]
    assert not (OC.reference("random", 0.1)[0] > 50)[-40:].any()                  # the wide points and the floater go


@pytest.mark.parametrize("name,radius", OC.random_cases())
def test_margin_census(name, radius):
    counts, margin = OC.reference(name, radius)
    print(name, radius, "least |d2/r2 - 1| =", margin)
    assert margin > OC.MARGIN_MIN
    assert counts.min() >= 1


@pytest.mark.parametrize("name,radius", OC.random_cases())
def test_reference_equals_scipy_ball_query(name, radius):
    """cKDTree counts d <= r in float64 with sums of its own: equal wherever no pair is on a tie (the census above)."""
    from scipy.spatial import cKDTree
    if name == "plane":
        pts, rows = OC.plane_cloud()
    else:
        pts = {"random": OC.random_cloud, "uniform": OC.uniform_cloud}[name]()
        rows = np.arange(len(pts))
    p = pts.astype(np.float64)
    got = cKDTree(p).query_ball_point(p[rows], radius, return_length=True)
    assert np.array_equal(got, OC.reference(name, radius)[0])
