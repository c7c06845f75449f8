"""NumPy brute force of the registration rules, shared by tests/test_registration_host.py and
tests/test_registration_gpu.py.  It shares nothing with pegasus_amd or its library.

Posed source point: s' = R s + t in float64, s the float32 point widened exactly, each coordinate ((r0*x + r1*y) + r2*z) + t
with every operation rounded on its own (NumPy never fuses).  Correspondent: the target of smallest d2 = ((dx*dx) + dy*dy) +
dz*dz, dx = q.x - s'.x, among equal d2 the lowest target row; accepted iff d2 < max_distance * max_distance (rounded once,
strict).  Every source row is compared with every target that can be accepted, and with more: the targets are sorted by x and
a chunk of rows meets those whose x and y lie within 2 max_distance of the chunk's ranges.  A target left out has |dx| or
|dy| > 2 max_distance: it can neither be accepted nor come nearer than max_distance to the threshold or to an accepted one.

The sums and the two updates take a dtype: float64 is the rule, numpy.longdouble is what the tolerance on the final
transformation is measured against (tests/registration_cases.py)."""
from collections import namedtuple

import numpy as np

ROWS_PER_CHUNK = 64
SINGULAR = 1e-12                     # the rule's: smallest eigen- / singular value against the largest
# where the sums lie (include/pegasus_raster.h)
JTJ, JTR, COUNT, D2, SUM_S, SUM_Q, SUM_SQ, SUM_SS, SUMS = 0, 21, 27, 28, 29, 32, 35, 44, 48

Neighbours = namedtuple("Neighbours", "index d2 distance_margin gap_margin")
Evaluation = namedtuple("Evaluation", "fitness rmse sums abs_sums neighbours")
Icp = namedtuple("Icp", "transformation fitness rmse index iterations distance_margin gap_margin")


def pose(source, T):
    """float64 [N,3]: the rule's s'."""
    s32 = np.asarray(source)
    assert s32.dtype == np.float32 and s32.ndim == 2 and s32.shape[1] == 3
    s = s32.astype(np.float64)
    T = np.asarray(T, dtype=np.float64)
    out = np.empty_like(s)
    for k in range(3):
        out[:, k] = ((T[k, 0] * s[:, 0] + T[k, 1] * s[:, 1]) + T[k, 2] * s[:, 2]) + T[k, 3]
    return out


def nearest(source, target, max_distance, T=None):
    """Neighbours(index int64 [Ns] (-1: none), d2 float64 [Ns] (0 where none), the least |d - max_distance| over all source
    rows (d: the distance to the nearest target), the least gap between the nearest and the second nearest target's distance
    over the accepted rows); a margin is inf where nothing was compared."""
    t32 = np.asarray(target)
    assert t32.dtype == np.float32 and t32.ndim == 2 and t32.shape[1] == 3
    s = pose(source, np.eye(4) if T is None else T)
    t = t32.astype(np.float64)
    r = np.float64(max_distance)
    assert np.isfinite(r) and r > 0
    r2 = r * r
    index = np.full(len(s), -1, dtype=np.int64)
    d2_out = np.zeros(len(s))
    distance_margin = gap_margin = np.inf
    if len(s) == 0 or len(t) == 0:
        return Neighbours(index, d2_out, distance_margin, gap_margin)
    by_x_t = np.argsort(t[:, 0], kind="stable")
    cand = t[by_x_t]
    reach = 2.0 * r
    # rows that share a chunk lie in one slab of x and are neighbours in y, so that few targets are within reach of any of them
    order = np.lexsort((s[:, 1], np.floor(s[:, 0] / reach)))
    for at in range(0, len(s), ROWS_PER_CHUNK):
        pos = order[at:at + ROWS_PER_CHUNK]
        q = s[pos]
        lo = np.searchsorted(cand[:, 0], q[:, 0].min() - reach, side="left")
        hi = np.searchsorted(cand[:, 0], q[:, 0].max() + reach, side="right")
        near_y = (cand[lo:hi, 1] >= q[:, 1].min() - reach) & (cand[lo:hi, 1] <= q[:, 1].max() + reach)
        if not near_y.any():
            continue
        c, rows = cand[lo:hi][near_y], by_x_t[lo:hi][near_y]
        dx = c[None, :, 0] - q[:, None, 0]
        dy = c[None, :, 1] - q[:, None, 1]
        dz = c[None, :, 2] - q[:, None, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        best = d2.min(axis=1)
        first = np.where(d2 == best[:, None], rows[None, :], np.iinfo(np.int64).max).min(axis=1)     # the lowest row among equals
        hit = best < r2
        index[pos[hit]] = first[hit]
        d2_out[pos[hit]] = best[hit]
        distance_margin = min(distance_margin, float(np.abs(np.sqrt(best) - r).min()))
        if hit.any() and d2.shape[1] > 1:
            two = np.sqrt(np.partition(d2[hit], 1, axis=1)[:, :2])
            gap_margin = min(gap_margin, float((two[:, 1] - two[:, 0]).min()))
    return Neighbours(index, d2_out, distance_margin, gap_margin)


def sums(source, target, normals, T, index, d2, dtype=np.float64):
    """(the 48 sums in ``dtype``, the sums of the terms' absolute values): over the rows with index >= 0."""
    rows = np.nonzero(index >= 0)[0]
    out, mag = np.zeros(SUMS, dtype=dtype), np.zeros(SUMS, dtype=dtype)
    if len(rows) == 0:
        return out, mag
    s = pose(source, T)[rows].astype(dtype)
    q = np.asarray(target)[index[rows]].astype(dtype)
    terms = np.zeros((len(rows), SUMS), dtype=dtype)
    terms[:, COUNT] = 1
    terms[:, D2] = np.asarray(d2)[rows]
    if normals is not None:
        n = np.asarray(normals)[index[rows]].astype(dtype)
        r = (s - q)[:, 0] * n[:, 0] + (s - q)[:, 1] * n[:, 1] + (s - q)[:, 2] * n[:, 2]
        J = np.concatenate([np.cross(s, n), n], axis=1)
        at = JTJ
        for a in range(6):
            for b in range(a, 6):
                terms[:, at] = J[:, a] * J[:, b]
                at += 1
        terms[:, JTR:JTR + 6] = J * r[:, None]
    terms[:, SUM_S:SUM_S + 3] = s
    terms[:, SUM_Q:SUM_Q + 3] = q
    terms[:, SUM_SQ:SUM_SQ + 9] = (s[:, :, None] * q[:, None, :]).reshape(len(rows), 9)
    terms[:, SUM_SS] = (s * s).sum(axis=1)
    return terms.sum(axis=0), np.abs(terms).sum(axis=0)


def evaluate(source, target, max_distance, T, normals=None, dtype=np.float64):
    nb = nearest(source, target, max_distance, T)
    v, mag = sums(source, target, normals, T, nb.index, nb.d2, dtype)
    count = float(v[COUNT])
    fitness = count / len(source) if len(source) else 0.0
    rmse = float(np.sqrt(np.float64(v[D2]) / count)) if count > 0 else 0.0
    return Evaluation(fitness, rmse, v, mag, nb)


def vec6_to_matrix(x, dtype=np.float64):
    """Rz(gamma) Ry(beta) Rx(alpha) with the translation, as three explicit matrix products."""
    x = np.asarray(x, dtype=dtype)
    one, zero = dtype(1), dtype(0)
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[one, zero, zero], [zero, ca, -sa], [zero, sa, ca]], dtype=dtype)
    Ry = np.array([[cb, zero, sb], [zero, one, zero], [-sb, zero, cb]], dtype=dtype)
    Rz = np.array([[cg, -sg, zero], [sg, cg, zero], [zero, zero, one]], dtype=dtype)
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = x[3:6]
    return T


def _solve(A, b):
    """Gaussian elimination with partial pivoting in the dtype of A."""
    A, b = A.copy(), b.copy()
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]
            b[i] -= f * b[k]
    x = np.zeros(n, dtype=A.dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def plane_update(v, dtype=np.float64):
    """The point-to-plane update from the sums; the identity with fewer than 6 correspondences or a singular system."""
    if v[COUNT] < 6:
        return np.eye(4, dtype=dtype)
    A = np.zeros((6, 6), dtype=dtype)
    A[np.triu_indices(6)] = v[JTJ:JTJ + 21]
    A = A + np.triu(A, 1).T
    w = np.linalg.eigvalsh(A.astype(np.float64))
    if not (w[-1] > 0.0 and w[0] > SINGULAR * w[-1]):
        return np.eye(4, dtype=dtype)
    return vec6_to_matrix(_solve(A, -np.asarray(v[JTR:JTR + 6], dtype=dtype)), dtype)


def _inverse3(M):
    a, b, c, d, e, f, g, h, i = M.reshape(-1)
    adj = np.array([[e * i - f * h, c * h - b * i, b * f - c * e],
                    [f * g - d * i, a * i - c * g, c * d - a * f],
                    [d * h - e * g, b * g - a * h, a * e - b * d]], dtype=M.dtype)
    return adj / (a * adj[0, 0] + b * adj[1, 0] + c * adj[2, 0])


def point_update(v, dtype=np.float64):
    """Kabsch without scale from the sums; the identity with fewer than 3 correspondences or a cross-covariance of rank < 2.
    float64: by the SVD, as the rule has it.  Any other dtype: the same rotation as the orthogonal polar factor of the
    cross-covariance, by Newton's iteration in that dtype (it must then have a positive determinant)."""
    n = v[COUNT]
    if n < 3:
        return np.eye(4, dtype=dtype)
    mu_s, mu_q = v[SUM_S:SUM_S + 3] / n, v[SUM_Q:SUM_Q + 3] / n
    H = v[SUM_SQ:SUM_SQ + 9].reshape(3, 3) / n - np.outer(mu_s, mu_q)
    U, S, Vt = np.linalg.svd(H.astype(np.float64))
    if not (S[0] > 0.0 and S[1] > SINGULAR * S[0]):
        return np.eye(4, dtype=dtype)
    if dtype == np.float64:
        D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) > 0 else -1.0])
        R = Vt.T @ D @ U.T
    else:
        assert np.linalg.det(H.astype(np.float64)) > 0
        X = H.astype(dtype) / dtype(S[0])
        for _ in range(60):
            X = (X + _inverse3(X).T) / 2
        R = X.T
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = R
    T[:3, 3] = mu_q - R @ mu_s
    return T


def icp(source, target, max_distance, init=None, estimation="point_to_plane", normals=None, max_iteration=30,
        relative_fitness=1e-6, relative_rmse=1e-6, dtype=np.float64):
    """The ICP rule.  The correspondences are always found in float64 with the transformation rounded to float64; the sums,
    the solve and the product update @ T run in ``dtype``.  The margins are the least over every evaluation."""
    plane = estimation == "point_to_plane"
    assert plane or estimation == "point_to_point"
    assert not plane or normals is not None
    T = np.eye(4, dtype=dtype) if init is None else np.asarray(init, dtype=dtype)
    update = plane_update if plane else point_update
    ev = evaluate(source, target, max_distance, T.astype(np.float64), normals if plane else None, dtype)
    dm, gm = ev.neighbours.distance_margin, ev.neighbours.gap_margin
    iterations = 0
    for _ in range(max_iteration):
        T = update(ev.sums, dtype) @ T
        before = ev
        ev = evaluate(source, target, max_distance, T.astype(np.float64), normals if plane else None, dtype)
        dm, gm = min(dm, ev.neighbours.distance_margin), min(gm, ev.neighbours.gap_margin)
        iterations += 1
        if abs(before.fitness - ev.fitness) < relative_fitness and abs(before.rmse - ev.rmse) < relative_rmse:
            break
    return Icp(T, ev.fitness, ev.rmse, ev.neighbours.index, iterations, dm, gm)


def normals(points, radius):
    """(normals float64 [N,3], counts int64 [N], gap ratio float64 [N]): the covariance of the points strictly within
    ``radius`` (the point itself included) about their mean, numpy.linalg.eigh, the eigenvector of the smallest eigenvalue with
    its component of largest magnitude positive; (0,0,1) with fewer than 3 neighbours.  Gap ratio: (l1 - l0) / l2 of the
    ascending eigenvalues (inf where l2 is 0 or the neighbours are fewer than 3)."""
    p32 = np.asarray(points)
    assert p32.dtype == np.float32 and p32.ndim == 2 and p32.shape[1] == 3
    p = p32.astype(np.float64)
    r = np.float64(radius)
    r2 = r * r
    out = np.tile(np.array([0.0, 0.0, 1.0]), (len(p), 1))
    counts = np.zeros(len(p), dtype=np.int64)
    ratio = np.full(len(p), np.inf)
    by_x = np.argsort(p[:, 0], kind="stable")
    cand = p[by_x]
    reach = r * (1.0 + 1e-9)
    for at in range(0, len(p), ROWS_PER_CHUNK):
        pos = by_x[at:at + ROWS_PER_CHUNK]
        q = p[pos]
        lo = np.searchsorted(cand[:, 0], q[:, 0].min() - reach, side="left")
        hi = np.searchsorted(cand[:, 0], q[:, 0].max() + reach, side="right")
        c = cand[lo:hi]
        dx = c[None, :, 0] - q[:, None, 0]
        dy = c[None, :, 1] - q[:, None, 1]
        dz = c[None, :, 2] - q[:, None, 2]
        within = ((dx * dx) + dy * dy) + dz * dz < r2
        counts[pos] = within.sum(axis=1)
        for k, row in enumerate(pos):
            if counts[row] < 3:
                continue
            nb = c[within[k]]
            d = nb - nb.mean(axis=0)
            w, v = np.linalg.eigh(d.T @ d / len(nb))
            n = v[:, 0]
            out[row] = n if n[np.argmax(np.abs(n))] > 0 else -n
            if w[2] > 0:
                ratio[row] = (w[1] - w[0]) / w[2]
    return out, counts, ratio


def rotation_angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, dtype=np.float64).T @ np.asarray(Rb, dtype=np.float64)) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
