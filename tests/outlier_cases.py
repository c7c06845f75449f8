"""Inputs of the radius-outlier tests (tests/test_outliers_host.py, tests/test_outliers_gpu.py), all seeded, and their
reference counts, computed once per process (tests/outlier_reference.py) and handed out read-only."""
import functools

import numpy as np

import outlier_reference as OR

SETTINGS = ((16, 0.03), (16, 0.05), (50, 0.1))          # the reference's: load_ply, denoise_point_cloud, ao_test.py
SIZES = (0, 1, 2, 255, 256, 257, 4099)
MARGIN_MIN = 1e-12                                      # float64 rounds at 1e-16: no fixture may sit nearer a tie than this
R_LATTICE = 2.0 ** -5                                   # a power of two: k * R_LATTICE is exact in float32


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_cloud():
    """4 059 points N(0, 0.05^2), 39 uniform in +-3 m and one at (900, -1800, 400): 4 099 points, float32."""
    rng = np.random.default_rng(20240619)
    blob = rng.normal(0.0, 0.05, (4059, 3))
    wide = rng.uniform(-3.0, 3.0, (39, 3))
    return _frozen(np.vstack([blob, wide, [[900.0, -1800.0, 400.0]]]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def uniform_cloud():
    """20 011 points uniform in a 1 m cube (about 10 within 0.05)."""
    return _frozen(np.random.default_rng(20011).uniform(-0.5, 0.5, (20011, 3)).astype(np.float32))


RADIUS_UNIFORM = 0.05


@functools.lru_cache(maxsize=None)
def plane_cloud():
    """200 003 points in a 4 m x 4 m x 2 m box, two thirds of them on the plane z = 0 with +-1 cm of noise; and 2 000 seeded
    query rows."""
    rng = np.random.default_rng(200003)
    n, on_plane = 200003, 133335
    pts = rng.uniform((-2.0, -2.0, -1.0), (2.0, 2.0, 1.0), (n, 3))
    pts[:on_plane, 2] = rng.uniform(-0.01, 0.01, on_plane)
    pts = pts[rng.permutation(n)].astype(np.float32)
    return _frozen(pts), _frozen(np.sort(rng.choice(n, 2000, replace=False)))


RADIUS_PLANE = 0.05


@functools.lru_cache(maxsize=None)
def reference(name, radius):
    """(counts, margin) of a named random case; for the plane cloud, of its query rows only."""
    if name == "plane":
        pts, rows = plane_cloud()
        got = OR.neighbor_counts(pts, radius, rows)
    else:
        got = OR.neighbor_counts({"random": random_cloud, "uniform": uniform_cloud}[name](), radius)
    return _frozen(got[0]), got[1]


def random_cases():
    """(name, radius) of every random case: what the margin census covers."""
    out = [("random", r) for _, r in SETTINGS]
    return out + [("uniform", RADIUS_UNIFORM), ("plane", RADIUS_PLANE)]


def tie_345():
    """Two points exactly 5 * 2^-7 apart (every product and sum exact) and that radius."""
    return np.array([[0, 0, 0], [3 * 2.0 ** -7, 4 * 2.0 ** -7, 0]], dtype=np.float32), 5 * 2.0 ** -7


def knife_pairs(count=16):
    """[(points [2,3], r_in, r_out)]: random float32 pairs, with r_in a float64 a few ulps above sqrt(d2), so that
    r_in * r_in > d2 (the pair counts), and r_out a few ulps below, so that r_out * r_out <= d2 (it does not)."""
    rng = np.random.default_rng(345)
    out = []
    for _ in range(count):
        pts = (rng.normal(0.0, 1.0, (2, 3)) * 10.0 ** rng.uniform(-2, 2)).astype(np.float32)
        d = pts[1].astype(np.float64) - pts[0].astype(np.float64)
        d2 = ((d[0] * d[0]) + d[1] * d[1]) + d[2] * d[2]
        r_in = r_out = np.sqrt(d2)
        for _ in range(3):
            r_in, r_out = np.nextafter(r_in, np.inf), np.nextafter(r_out, 0.0)
        assert r_in * r_in > d2 and r_out * r_out <= d2 and d2 > 0
        out.append((pts, float(r_in), float(r_out)))
    return out


def lattice(side, spacing, lo=None):
    """side^3 points at spacing * (i, j, k), the indices starting at ``lo`` (default: centred on 0, so that negative
    coordinates and the cell walls around 0 are among them); float32."""
    lo = -(side // 2) if lo is None else lo
    k = np.arange(lo, lo + side, dtype=np.float64) * spacing
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    assert np.array_equal(g.astype(np.float32).astype(np.float64), g)          # exact in float32
    return g.astype(np.float32)


def lattice_axis_neighbours(side):
    """For lattice(side, ..): how many of a point's 6 axis neighbours exist."""
    i = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return ((i > 0).sum(axis=1) + (i < side - 1).sum(axis=1)).astype(np.int64)


def constellation(radius, centre):
    """27 points at centre + {-0.55 r, 0, +0.55 r}^3 (float32), the centre at row 13.  Two of them lie 0.55 r |D| apart with
    D in {-2..2}^3, within r iff |D|^2 <= 3 (0.3025 * 3 = 0.9075 against 0.3025 * 4 = 1.21), that is iff no component of D is
    +-2: a point counts 3 along every axis on which its own offset is 0 and 2 along the others."""
    o = np.stack(np.meshgrid(*[np.array([-1.0, 0.0, 1.0])] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = (np.asarray(centre, dtype=np.float64) + 0.55 * radius * o).astype(np.float32)
    want = np.prod(np.where(o == 0.0, 3, 2), axis=1).astype(np.int64)
    return pts, want


def constellation_centres():
    """8 random translations (negative coordinates among them) and one far from the origin."""
    rng = np.random.default_rng(27)
    c = rng.uniform(-2.0, 2.0, (8, 3))
    assert (c < 0).any() and (c > 0).any()
    return [tuple(x) for x in c] + [(1000.0, -2000.0, 500.0)]


RADIUS_CONSTELLATION = 0.05


def coincident(count=300):
    return np.tile(np.array([[0.1, -0.2, 0.3]], dtype=np.float32), (count, 1))


def table_load(floater=False):
    """4 096 points on a lattice of spacing 3 r (4 096 occupied cells, no two within r); with ``floater`` one more at 10^6 r."""
    pts = lattice(16, 3 * R_LATTICE)
    if floater:
        pts = np.vstack([pts, np.array([[1e6 * R_LATTICE, -5e5 * R_LATTICE, 1e6 * R_LATTICE]], dtype=np.float32)])
    return pts
