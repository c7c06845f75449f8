"""NumPy float64 brute force of the radius-outlier rule, shared by tests/test_outliers_host.py and
tests/test_outliers_gpu.py.  It shares nothing with pegasus_amd or its library.

count_i = #{ j, j = i included : ((dx*dx) + dy*dy) + dz*dz < radius*radius }, in float64 with every operation rounded on its
own (NumPy never fuses), dx, dy, dz the float64 differences of the float32 coordinates widened exactly, radius*radius rounded
once, the comparison strict.  A point is kept iff count_i > nb_points.

Every row is compared with every point that can count: the candidates are sorted by x and a chunk of rows meets those whose x
lies within radius * (1 + 1e-9) of the chunk's x range.  A point left out has |dx| > radius (1 + 1e-9), so its dx*dx, rounded,
exceeds radius*radius, rounded, by far more than the two roundings (2^-53 each), and so does the sum of three non-negative
terms: leaving it out changes no count."""
import numpy as np

ROWS_PER_CHUNK = 64


def neighbor_counts(points, radius, rows=None):
    """(counts int64 [len(rows)], margin): the counts of ``rows`` (all rows for None) against ALL points, and the least
    |d2 / r2 - 1| over every pair compared (inf if there was none but the pairs of a point with itself and its copies)."""
    p32 = np.asarray(points)
    assert p32.dtype == np.float32 and p32.ndim == 2 and p32.shape[1] == 3
    p = p32.astype(np.float64)
    r = np.float64(radius)
    assert np.isfinite(r) and r > 0
    r2 = r * r
    rows = np.arange(len(p)) if rows is None else np.asarray(rows, dtype=np.int64)
    counts = np.zeros(len(rows), dtype=np.int64)
    margin = np.inf
    if len(p) == 0 or len(rows) == 0:
        return counts, margin
    cand = p[np.argsort(p[:, 0], kind="stable")]
    reach = r * (1.0 + 1e-9)
    by_x = np.argsort(p[rows, 0], kind="stable")                   # positions in `rows`, in x order
    for at in range(0, len(rows), ROWS_PER_CHUNK):
        pos = by_x[at:at + ROWS_PER_CHUNK]
        q = p[rows[pos]]
        lo = np.searchsorted(cand[:, 0], q[:, 0].min() - reach, side="left")
        hi = np.searchsorted(cand[:, 0], q[:, 0].max() + reach, side="right")
        c = cand[lo:hi]
        dx = c[None, :, 0] - q[:, None, 0]
        dy = c[None, :, 1] - q[:, None, 1]
        dz = c[None, :, 2] - q[:, None, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        counts[pos] = (d2 < r2).sum(axis=1)
        apart = d2[d2 > 0.0]
        if apart.size and r2 > 0.0 and np.isfinite(r2):
            margin = min(margin, float(np.abs(apart / r2 - 1.0).min()))
    return counts, margin


def keep_mask(points, nb_points, radius):
    """(mask bool [N], margin): open3d's remove_radius_outlier as a mask."""
    assert int(nb_points) >= 1
    counts, margin = neighbor_counts(points, radius)
    return counts > int(nb_points), margin
