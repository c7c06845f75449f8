"""The ground-plane rule of DESIGN.md section 18 as a float64 brute force in NumPy: what tests/test_alignment_host.py and
tests/test_alignment_gpu.py hold pegasus_amd/alignment.py and the three pgr_plane_* entries against.  Nothing here is fast, and
nothing is shared with the package.

Every elementwise NumPy operation rounds on its own (no operation is fused), which is the rule's "every operation rounded on
its own".  The sums, the refit and the transformation take a dtype: float64 is the rule, numpy.longdouble is what the tolerance
on the final 4x4 is measured with (the inlier decisions stay the float64 rule's in both)."""
from types import SimpleNamespace

import numpy as np

SUMS = 12
COUNT, SUM_Q, SUM_QQ, SUM_D2 = 0, 1, 4, 10
EIGEN_GAP_MIN = 1e-12


def _p64(points):
    p32 = np.asarray(points)
    assert p32.dtype == np.float32 and p32.ndim == 2 and p32.shape[1] == 3
    return p32.astype(np.float64)


def hypotheses(points, triples):
    """(planes float64 [H,4], valid uint8 [H])."""
    p = _p64(points)
    n = len(p)
    tri = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    planes, valid = np.zeros((len(tri), 4)), np.zeros(len(tri), dtype=np.uint8)
    ok = ((tri >= 0) & (tri < n)).all(axis=1) & (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
    rows = np.nonzero(ok)[0]
    if len(rows) == 0:
        return planes, valid
    p0, p1, p2 = p[tri[rows, 0]], p[tri[rows, 1]], p[tri[rows, 2]]
    a, b = p1 - p0, p2 - p0
    cx = (a[:, 1] * b[:, 2]) - (a[:, 2] * b[:, 1])
    cy = (a[:, 2] * b[:, 0]) - (a[:, 0] * b[:, 2])
    cz = (a[:, 0] * b[:, 1]) - (a[:, 1] * b[:, 0])
    with np.errstate(all="ignore"):
        norm = np.sqrt(((cx * cx) + cy * cy) + cz * cz)
        good = (norm != 0.0) & np.isfinite(norm)
        nx, ny, nz = cx / norm, cy / norm, cz / norm
        d = -(((nx * p0[:, 0]) + ny * p0[:, 1]) + nz * p0[:, 2])
    found = np.stack([nx, ny, nz, d], axis=1)
    planes[rows[good]] = found[good]
    valid[rows[good]] = 1
    return planes, valid


def distances(points, plane):
    """float64 [N]: |((nx*x + ny*y) + nz*z) + d|."""
    p = _p64(points)
    nx, ny, nz, d = (float(v) for v in plane)
    return np.abs(((nx * p[:, 0] + ny * p[:, 1]) + nz * p[:, 2]) + d)


def scores(points, planes, threshold):
    """counts int64 [H], sumsq float64 [H] (a sum of non-negative terms: it is its own sum of absolute terms), and the
    smallest |dist - threshold| over the planes that are not four zeros."""
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    counts, sumsq, margin = np.zeros(len(planes), dtype=np.int64), np.zeros(len(planes)), np.inf
    for h, plane in enumerate(planes):
        if not plane.any() or len(points) == 0:
            continue
        dist = distances(points, plane)
        inl = dist < threshold
        counts[h], sumsq[h] = int(inl.sum()), float((dist[inl] * dist[inl]).sum())
        margin = min(margin, float(np.abs(dist - threshold).min()))
    return SimpleNamespace(counts=counts, sumsq=sumsq, margin=margin)


def choose(counts, sumsq, valid):
    """(best, second): the valid hypotheses in the rule's order -- largest count, then smallest sumsq, then lowest index; -1
    where there is none."""
    rows = np.nonzero(np.asarray(valid).astype(bool))[0]
    ranked = sorted(rows, key=lambda h: (-int(counts[h]), float(sumsq[h]), int(h)))
    return (int(ranked[0]) if ranked else -1), (int(ranked[1]) if len(ranked) > 1 else -1)


def inlier_sums(points, plane, pivot, threshold, dtype=np.float64):
    """mask uint8 [N], the 12 sums in ``dtype``, the sums of the terms' absolute values, the margin."""
    p = _p64(points)
    plane = np.asarray(plane, dtype=np.float64)
    out, mag = np.zeros(SUMS, dtype=dtype), np.zeros(SUMS, dtype=dtype)
    if len(p) == 0 or not plane.any():
        return SimpleNamespace(mask=np.zeros(len(p), dtype=np.uint8), sums=out, mag=mag, margin=np.inf)
    dist = distances(points, plane)
    inl = dist < threshold
    q = p[inl].astype(dtype) - np.asarray(pivot, dtype=np.float64).astype(dtype)
    terms = np.zeros((int(inl.sum()), SUMS), dtype=dtype)
    terms[:, COUNT] = 1
    terms[:, SUM_Q:SUM_Q + 3] = q
    at = SUM_QQ
    for a in range(3):
        for b in range(a, 3):
            terms[:, at] = q[:, a] * q[:, b]
            at += 1
    terms[:, SUM_D2] = dist[inl].astype(dtype) * dist[inl].astype(dtype)
    terms = np.ascontiguousarray(terms.T)                      # (rows of one term: NumPy adds those pairwise)
    out[:], mag[:] = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    return SimpleNamespace(mask=inl.astype(np.uint8), sums=out, mag=mag, margin=float(np.abs(dist - threshold).min()))


def _solve3(A, b):
    """Gaussian elimination with partial pivoting in the dtype of A."""
    A, b = A.copy(), b.copy()
    for k in range(3):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, piv]], b[[k, piv]] = A[[piv, k]], b[[piv, k]]
        for r in range(k + 1, 3):
            f = A[r, k] / A[k, k]
            A[r] -= f * A[k]
            b[r] -= f * b[k]
    x = np.zeros(3, dtype=A.dtype)
    for k in (2, 1, 0):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def smallest_eigenvector(cov):
    """(eigenvalues ascending in float64, the unit eigenvector of the smallest in the dtype of ``cov``).  float64: numpy's
    eigh, as the rule has it.  Any other dtype: eigh's answer refined by inverse iteration in that dtype, with a shift a
    thousandth of the gap below the smallest eigenvalue (every step gains three digits)."""
    w, v = np.linalg.eigh(cov.astype(np.float64))
    x = v[:, 0] / np.linalg.norm(v[:, 0])
    if cov.dtype == np.float64:
        return w, x
    dtype = cov.dtype.type
    x = x.astype(dtype)
    shifted = cov - np.eye(3, dtype=dtype) * dtype(w[0] - 1e-3 * (w[1] - w[0]))
    for _ in range(12):
        x = _solve3(shifted, x)
        x = x / np.sqrt((x * x).sum())
    return w, x if x @ v[:, 0].astype(dtype) >= 0 else -x


def refit(sums, pivot, hypothesis_plane, dtype=np.float64):
    """(plane in ``dtype``, the eigen-gap ratio (l1 - l0) / l2, or 0 where the hypothesis plane is kept)."""
    sums = np.asarray(sums, dtype=dtype)
    keep = np.asarray(hypothesis_plane, dtype=np.float64).astype(dtype)
    count = sums[COUNT]
    if count < 3:
        return keep, 0.0
    m = sums[SUM_Q:SUM_Q + 3] / count
    S = np.zeros((3, 3), dtype=dtype)
    S[np.triu_indices(3)] = sums[SUM_QQ:SUM_QQ + 6]
    S = S + np.triu(S, 1).T
    cov = S / count - np.outer(m, m)
    w, normal = smallest_eigenvector(cov)
    if not (w[2] > 0.0 and (w[1] - w[0]) / w[2] > EIGEN_GAP_MIN):
        return keep, 0.0
    centre = np.asarray(pivot, dtype=np.float64).astype(dtype) + m
    plane = np.array([normal[0], normal[1], normal[2], -(normal @ centre)], dtype=dtype)
    return plane, float((w[1] - w[0]) / w[2])


def orient(plane, plane_normal=None, camera_centers=None):
    plane = np.array(plane)
    n = plane[:3].astype(np.float64)
    if plane_normal is not None:
        flip = float(n @ np.asarray(plane_normal, dtype=np.float64)) < 0.0
    elif camera_centers is not None and len(camera_centers):
        c = np.asarray(camera_centers, dtype=np.float64).reshape(-1, 3)
        flip = 2 * int((c @ n + float(plane[3]) > 0.0).sum()) < len(c)
    else:
        flip = n[int(np.argmax(np.abs(n)))] < 0.0
    return -plane if flip else plane


def rotation_to_z(normal):
    """Rodrigues about normal x z in the dtype of ``normal``; the identity for +z, a half turn about x for -z."""
    n = np.asarray(normal)
    dtype = n.dtype.type
    if n[0] == 0 and n[1] == 0:
        return np.eye(3, dtype=dtype) if n[2] > 0 else np.diag([dtype(1), dtype(-1), dtype(-1)])
    zero = dtype(0)
    K = np.array([[zero, zero, -n[0]], [zero, zero, -n[1]], [n[0], n[1], zero]], dtype=dtype)       # [n x z]_x
    return np.eye(3, dtype=dtype) + K + K @ K / (dtype(1) + n[2])


def transformation(plane, centroid, scale=1.0):
    """4x4 of x' = s R x + t in the dtype of ``plane``."""
    plane = np.asarray(plane)
    dtype = plane.dtype.type
    c, n, s = np.asarray(centroid).astype(dtype), plane[:3], dtype(scale)
    origin = c - ((n @ c) + plane[3]) * n
    R = rotation_to_z(n)
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = s * R
    T[:3, 3] = -s * (R @ origin)
    return T


def fit(points, triples, threshold, plane_normal=None, camera_centers=None, scale=1.0, dtype=np.float64):
    """The whole rule.  ``margin``: the smallest |dist - threshold| over every valid hypothesis and, again, under the refitted
    plane; ``sumsq_gap``: the relative difference in sumsq between the best and the second best where their counts are equal
    (inf where they differ)."""
    p = _p64(points)
    planes, valid = hypotheses(points, triples)
    sc = scores(points, planes, threshold)
    best, second = choose(sc.counts, sc.sumsq, valid)
    if best < 0:
        raise ValueError("no valid hypothesis")
    sumsq_gap = np.inf
    if second >= 0 and sc.counts[second] == sc.counts[best]:
        sumsq_gap = abs(sc.sumsq[second] - sc.sumsq[best]) / max(sc.sumsq[best], np.finfo(np.float64).tiny)
    pivot = p[int(np.asarray(triples)[best, 0])]
    first = inlier_sums(points, planes[best], pivot, threshold, dtype)
    plane, gap = refit(first.sums, pivot, planes[best], dtype)
    after = inlier_sums(points, plane.astype(np.float64), pivot, threshold, dtype)
    count = int(after.sums[COUNT])
    centroid = pivot.astype(dtype) + after.sums[SUM_Q:SUM_Q + 3] / after.sums[COUNT] if count else pivot.astype(dtype)
    oriented = orient(plane, plane_normal, camera_centers)
    return SimpleNamespace(planes=planes, valid=valid, counts=sc.counts, sumsq=sc.sumsq, best_index=best, second_index=second,
                           sumsq_gap=float(sumsq_gap), margin=min(sc.margin, after.margin), hypothesis_plane=planes[best],
                           hypothesis_count=int(first.sums[COUNT]), plane=oriented, eigen_gap=gap, mask=after.mask,
                           inliers=np.nonzero(after.mask)[0], count=count, fitness=count / len(p),
                           inlier_rmse=float(np.sqrt(after.sums[SUM_D2] / after.sums[COUNT])) if count else 0.0,
                           centroid=centroid, transformation=transformation(oriented, centroid, scale))


def plane_angle_deg(a, b):
    c = abs(float(np.asarray(a, dtype=np.float64)[:3] @ np.asarray(b, dtype=np.float64)[:3]))
    return float(np.degrees(np.arccos(min(1.0, c))))
