"""NumPy float64 restatement of the minimal-oriented-box and diameter rules, independent of the code
under test: nothing here imports pegasus_amd.  It takes exactly the float32 points the kernels get, widened to float64.

The rule.  Candidate of triangle (i0, i1, i2) over points p:  a = p[i0], u = p[i1] - a, v0 = p[i2] - a, w = u x v0, v = w x u,
each of u, v, w divided by its norm; q = ((p - a).u, (p - a).v, (p - a).w) for every point; lo, hi = per-axis min, max of q;
extent = hi - lo; volume = extent.x extent.y extent.z.  The minimal box is the candidate of smallest FINITE volume, the lowest
triangle index among equal ones, none (-1) if no volume is finite.  R = [u v w] as columns, center = a + R (lo + hi) / 2.
NumPy's min and max propagate NaN, so a degenerate triangle (NaN axes) and a NaN or Inf point give a volume that is not finite.

Tolerances.  EPS = 2^-53 is float64's unit roundoff.  Each bound is a count of rounding steps times EPS times the magnitude
the step acts on; none was read off the kernels' observed error.  The kernel and this module are two float64 evaluations of
the same real number, each off the exact value by the one-evaluation bound, so every count is doubled.

One projection q_k = d . e_k, d = p - a, D = |d.x| + |d.y| + |d.z|, |e_k| = 1, per evaluation, to first order in EPS:
    d = p - a, one rounding per component                                                1 D
    three products and two sums (fused or not), each rounding a partial sum <= D          3 D
    the axis divided by its norm: x x + y y + z z of positive terms 3 roundings, halved by the square root (1.5), the
    square root and the division each within 1 ulp = 2 EPS                                5.5 -> 6 D
    direction of u: one rounding per component, |delta u| <= EPS |u| (< the 7 below)
    direction of w = u x v0: a component u_j v0_k - u_k v0_j carries the roundings of u_j, v0_k, the product and the
    difference: 4 EPS (|u_j v0_k| + |u_k v0_j|) <= 4 EPS |u| |v0| (Cauchy-Schwarz), the vector sqrt(3) times that,
    < 7 EPS |u| |v0|; against |w| = |u| |v0| / kappa, kappa = |u| |v0| / |w| >= 1 (1 / sin of the triangle's angle at a):
    the unit axis turns by at most                                                        7 kappa D
    direction of v = w x u: w's error passes through (7 kappa), its own components as above with |v| = |w| |u| exactly
    perpendicular: 7                                                                      (7 kappa + 7) D
The worst axis is v: 1 + 3 + 6 + 7 + 7 kappa = 17 + 7 kappa per evaluation.
"""
import numpy as np

EPS = 2.0 ** -53
K_Q_FIXED = 2 * 17               # two evaluations of 17
K_Q_KAPPA = 2 * 7                # two evaluations of 7 kappa
K_EXTENT = 2                     # hi - lo: one rounding per evaluation, on |extent|
K_VOLUME = 4                     # two products per evaluation, on |volume|
K_D2 = 2 * 5                     # d2 = dx dx + dy dy + dz dz: dx one rounding (2 on its square), the square 1, two sums 2

NDDS_ORDER = (0, 2, 5, 3, 1, 7, 4, 6)


def f64(points):
    p = np.asarray(points)
    assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 3
    return p.astype(np.float64)


def frames(points, tris):
    """a [F,3], axes [F,3,3] (axes[f, k] = unit axis k: u, v, w), kappa [F] (inf for a degenerate triangle)."""
    p = f64(points)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    a = p[t[:, 0]]
    u, v0 = p[t[:, 1]] - a, p[t[:, 2]] - a
    with np.errstate(all="ignore"):
        w = np.cross(u, v0)
        v = np.cross(w, u)
        norm = lambda x: np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        nu, nv0, nw = norm(u), norm(v0), norm(w)
        axes = np.stack([u / nu[:, None], v / norm(v)[:, None], w / nw[:, None]], axis=1)
        kappa = np.where(nw > 0, nu * nv0 / nw, np.inf)
    return a, axes, kappa


def candidates(points, tris, block=64):
    """lohi [F,6], volumes [F], q_bound [F] (the bound on |q_device - q_reference| of every projection of the triangle)."""
    p = f64(points)
    a, axes, kappa = frames(points, tris)
    F = len(a)
    lohi = np.empty((F, 6))
    dmax = np.empty(F)
    with np.errstate(all="ignore"):
        for f0 in range(0, F, block):
            d = p[None, :, :] - a[f0:f0 + block, None, :]                     # [f,P,3]
            q = np.einsum("fpc,fkc->fpk", d, axes[f0:f0 + block])
            lohi[f0:f0 + block, :3] = q.min(axis=1)
            lohi[f0:f0 + block, 3:] = q.max(axis=1)
            dmax[f0:f0 + block] = np.abs(d).sum(axis=2).max(axis=1)
        extent = lohi[:, 3:] - lohi[:, :3]
        volumes = extent[:, 0] * extent[:, 1] * extent[:, 2]
        q_bound = (K_Q_FIXED + K_Q_KAPPA * kappa) * EPS * dmax
    return lohi, volumes, q_bound


def volume_bound(lohi, q_bound):
    """The bound on |volume_device - volume_reference|: each extent is within 2 q_bound + K_EXTENT EPS |extent|; the product
    of the three widened extents less the product itself, plus K_VOLUME EPS of it."""
    with np.errstate(all="ignore"):
        e = lohi[:, 3:] - lohi[:, :3]
        g = e + 2 * q_bound[:, None] + K_EXTENT * EPS * np.abs(e)
        grown = g[:, 0] * g[:, 1] * g[:, 2]
        return grown - e[:, 0] * e[:, 1] * e[:, 2] + K_VOLUME * EPS * grown


def argmin_finite(volumes):
    """The lowest index of the smallest finite volume; -1 if none is finite."""
    v = np.asarray(volumes, np.float64)
    ok = np.isfinite(v)
    if not ok.any():
        return -1
    return int(np.nonzero(ok & (v == v[ok].min()))[0][0])


def box(points, tri, lohi):
    """(center [3], R [3,3], extent [3]) of one candidate."""
    a, axes, _ = frames(points, np.asarray(tri).reshape(1, 3))
    lo, hi = lohi[:3], lohi[3:]
    R = axes[0].T
    return a[0] + R @ ((lo + hi) / 2), R, hi - lo


def minimal_box(points, tris):
    lohi, volumes, _ = candidates(points, tris)
    b = argmin_finite(volumes)
    if b < 0:
        return None
    return box(points, np.asarray(tris).reshape(-1, 3)[b], lohi[b])


def box_points(center, R, extent):
    """open3d's GetBoxPoints order."""
    x, y, z = R[:, 0] * extent[0] / 2, R[:, 1] * extent[1] / 2, R[:, 2] * extent[2] / 2
    c = np.asarray(center, np.float64)
    return np.array([c - x - y - z, c + x - y - z, c - x + y - z, c - x - y + z,
                     c + x + y + z, c - x + y + z, c + x - y + z, c + x + y - z])


def ndds_corners(center, R, extent):
    return box_points(center, R, extent)[list(NDDS_ORDER)]


def contains(center, R, extent, points, tol):
    q = (np.asarray(points, np.float64) - center) @ R
    return (np.abs(q) <= extent / 2 + tol).all(axis=1)


def far_candidates(p):
    """Indices (ascending) of the points that can belong to a farthest pair.  With c any centre, r_i = |p_i - c| and L the
    distance of some pair, a pair (i, j) with r_i + r_j < L is shorter than L by the triangle inequality, so a point with
    r_i < L - max r is in no farthest pair.  A relative margin of 1e-9 covers the rounding of r and L."""
    if len(p) < 3:
        return np.arange(len(p))
    r = np.linalg.norm(p - p.mean(0), axis=1)
    L = np.linalg.norm(p - p[np.argmax(r)], axis=1).max()
    return np.nonzero(r >= L - r.max() - 1e-9 * (L + r.max()))[0]


def diameter(points, block=256):
    """(largest squared distance over pairs i < j, the lexicographically lowest pair attaining it); (0.0, None) below two
    points.  Brute force over far_candidates, which keeps the order of the points."""
    keep = far_candidates(f64(points))
    best, pair = _diameter_brute(f64(points)[keep], block)
    return (best, None) if pair is None else (best, (int(keep[pair[0]]), int(keep[pair[1]])))


def _diameter_brute(p, block):
    best, pair = -1.0, None
    for i0 in range(0, len(p), block):
        d = p[None, :, :] - p[i0:i0 + block, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d2[np.arange(len(p))[None, :] <= (i0 + np.arange(d2.shape[0]))[:, None]] = -1.0      # only i < j
        m = d2.max() if d2.size else -1.0
        if m > best:
            i, j = np.unravel_index(np.argmax(d2), d2.shape)                                 # row-major first: lowest (i, j)
            best, pair = float(m), (int(i0 + i), int(j))
    return (best, pair) if pair is not None else (0.0, None)


def d2_of(points, i, j):
    p = f64(points)
    d = p[j] - p[i]
    return float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
