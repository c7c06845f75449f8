"""Vertex clustering in NumPy float64, restated from the rule of DESIGN.md section 19 (pegasus_amd/csrc/decimate.hip.h): the
reference of tests/test_decimate_host.py and tests/test_decimate_gpu.py.  It shares no code with pegasus_amd/decimate.py.

NumPy rounds every ufunc call on its own, so writing the rule's operations one per call is the rule's "every product, quotient
and sum is rounded on its own"; the sums follow the rule's fixed order (64 partials, then a fold) literally.

``mutant`` switches ONE clause of the rule off, for the tests that show each clause is observable:
    "no_half_voxel"    lo = min, without the half voxel
    "count_once"       a face with two corners in a cluster adds to it once
    "flip_rotation"    the rotation to the smallest index reverses the orientation
    "keep_duplicates"  duplicate faces stay
    "order_xyz"        clusters numbered in ascending (cx, cy, cz)
    "no_box_test"      the quadric position is accepted on the determinant alone
"""
from dataclasses import dataclass

import numpy as np

CELL_MAX = float((1 << 20) - 1)
LANES = 64
U = 2.0 ** -53


@dataclass
class Clustered:
    vertices: np.ndarray          # float64 [K,3]
    faces: np.ndarray             # int32 [F',3]
    cluster_of_vertex: np.ndarray # int32 [V]
    used_quadric: np.ndarray      # uint8 [K]
    corner: np.ndarray            # float64 [K,3]: the cells' lower corners
    cells: np.ndarray             # int64 [K,3]: (cx, cy, cz)
    members: np.ndarray           # int64 [K]: vertices per cluster
    lo: np.ndarray
    # quadric diagnostics (None for "average"): what the tolerance of the GPU test is derived from
    terms: np.ndarray = None      # int64 [K]: corner terms per cluster
    A: np.ndarray = None          # float64 [K,6]: Axx Axy Axz Ayy Ayz Azz
    b: np.ndarray = None          # float64 [K,3]
    x: np.ndarray = None          # float64 [K,3]: -A^-1 b (nan / inf where det == 0)
    det: np.ndarray = None
    threshold: np.ndarray = None
    sum_norm_A: np.ndarray = None # sum over the terms of ||A_i||_2 = w_i
    sum_norm_b: np.ndarray = None # sum over the terms of ||b_i||_2 = w_i |d_i|
    average: np.ndarray = None    # float64 [K,3]: the average positions (what a rejected cluster takes)


def segmented_sum(values, start):
    """values [T,C] ordered by segment, start [K+1] -> [K,C]: per segment the rule's sum.  Term j of a segment goes to partial
    j mod 64, the partials add their terms in ascending j from 0.0, then p[l] += p[l + d] (l < d) for d = 32 .. 1; p[0]."""
    values = np.asarray(values, np.float64)
    start = np.asarray(start, np.int64)
    K, C = len(start) - 1, values.shape[1]
    m = np.diff(start)
    lanes = np.minimum(m, LANES)
    pstart = np.concatenate([[0], np.cumsum(lanes)])
    seg = np.repeat(np.arange(K), m)
    rank = np.arange(len(values)) - start[seg]
    pidx = pstart[seg] + rank % LANES
    rnd = rank // LANES
    p = np.zeros((int(pstart[-1]), C), np.float64)
    for r in range(int(rnd.max()) + 1 if len(rnd) else 0):
        sel = rnd == r
        p[pidx[sel]] = p[pidx[sel]] + values[sel]          # (one term per partial and round: no index repeats)
    plane = np.arange(len(p)) - np.repeat(pstart[:-1], lanes)
    d = LANES // 2
    while d >= 1:
        src = np.nonzero((plane >= d) & (plane < 2 * d))[0]
        p[src - d] = p[src - d] + p[src]
        d //= 2
    out = np.zeros((K, C), np.float64)
    has = m > 0
    out[has] = p[pstart[:-1][has]]
    return out


def cluster_reference(vertices, faces, voxel, contraction="quadric", mutant=None):
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    x = v32.astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    voxel = float(voxel)
    # 1. cells
    lo = x.min(axis=0) if mutant == "no_half_voxel" else x.min(axis=0) - voxel / 2.0
    cell = np.clip(np.floor((x - lo) / voxel), 0.0, CELL_MAX).astype(np.int64)
    if mutant == "order_xyz":
        key = (cell[:, 0] << 40) | (cell[:, 1] << 20) | cell[:, 2]
    else:
        key = (cell[:, 2] << 40) | (cell[:, 1] << 20) | cell[:, 0]
    ukey, first, cov = np.unique(key, return_index=True, return_inverse=True)
    cov = cov.reshape(-1)
    K = len(ukey)
    cells = cell[first]
    corner = lo + cells.astype(np.float64) * voxel
    members = np.bincount(cov, minlength=K)
    # 3. average: the cluster's vertices in ascending index
    order = np.argsort(cov, kind="stable")
    vstart = np.concatenate([[0], np.cumsum(members)])
    mean = segmented_sum(x[order] - corner[cov[order]], vstart) / members[:, None].astype(np.float64)
    average = corner + np.minimum(np.maximum(mean, 0.0), voxel)
    out = Clustered(average.copy(), None, cov.astype(np.int32), np.zeros(K, np.uint8), corner, cells, members, lo, average=average)
    # 5. faces
    cl = cov[f] if len(f) else np.zeros((0, 3), np.int64)
    keep = (cl[:, 0] != cl[:, 1]) & (cl[:, 1] != cl[:, 2]) & (cl[:, 0] != cl[:, 2])
    cl = cl[keep]
    if len(cl):
        s = np.argmin(cl, axis=1)
        rows = np.arange(len(cl))
        if mutant == "flip_rotation":
            cl = np.stack([cl[rows, s], cl[rows, (s + 2) % 3], cl[rows, (s + 1) % 3]], axis=1)
        else:
            cl = np.stack([cl[rows, s], cl[rows, (s + 1) % 3], cl[rows, (s + 2) % 3]], axis=1)
        cl = cl[np.lexsort((cl[:, 2], cl[:, 1], cl[:, 0]))]
        if mutant != "keep_duplicates":
            cl = cl[np.concatenate([[True], (cl[1:] != cl[:-1]).any(axis=1)])]
    out.faces = cl.astype(np.int32).reshape(-1, 3)
    if contraction == "average":
        return out
    assert contraction == "quadric"
    # 4. quadric: the corners (f, j) by cluster, in ascending 3 f + j
    tc = cov[f.reshape(-1)] if len(f) else np.zeros(0, np.int64)
    t_keep = np.ones(len(tc), bool)
    if mutant == "count_once" and len(f):
        c3 = tc.reshape(-1, 3)
        t_keep = np.stack([np.ones(len(c3), bool), c3[:, 1] != c3[:, 0], (c3[:, 2] != c3[:, 0]) & (c3[:, 2] != c3[:, 1])],
                          axis=1).reshape(-1)
    torder = np.argsort(tc, kind="stable")
    torder = torder[t_keep[torder]]
    tcl = tc[torder]
    tf = f[torder // 3]
    cor = corner[tcl]
    q0, q1, q2 = x[tf[:, 0]] - cor, x[tf[:, 1]] - cor, x[tf[:, 2]] - cor
    e1, e2 = q1 - q0, q2 - q0
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    a2 = np.sqrt((nx * nx + ny * ny) + nz * nz)
    ok = (a2 > 0.0) & (tf[:, 0] != tf[:, 1]) & (tf[:, 1] != tf[:, 2]) & (tf[:, 0] != tf[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        ux, uy, uz = nx / a2, ny / a2, nz / a2
        w = a2 / 2.0
        d = -((ux * q0[:, 0] + uy * q0[:, 1]) + uz * q0[:, 2])
        wx, wy, wz, wd = w * ux, w * uy, w * uz, w * d
        term = np.stack([wx * ux, wx * uy, wx * uz, wy * uy, wy * uz, wz * uz, wd * ux, wd * uy, wd * uz, w, w * np.abs(d)], axis=1)
    term[~ok] = 0.0
    terms = np.bincount(tcl, minlength=K)
    tstart = np.concatenate([[0], np.cumsum(terms)])
    S = segmented_sum(term, tstart)
    Axx, Axy, Axz, Ayy, Ayz, Azz, bx, by, bz = (S[:, i] for i in range(9))
    c00, c01, c02 = Ayy * Azz - Ayz * Ayz, Axz * Ayz - Axy * Azz, Axy * Ayz - Axz * Ayy
    c11, c12, c22 = Axx * Azz - Axz * Axz, Axy * Axz - Axx * Ayz, Axx * Ayy - Axy * Axy
    det = (Axx * c00 + Axy * c01) + Axz * c02
    t = ((Axx + Ayy) + Azz) / 3.0
    threshold = 1e-4 * ((t * t) * t)
    with np.errstate(divide="ignore", invalid="ignore"):
        x0 = -(((c00 * bx + c01 * by) + c02 * bz) / det)
        x1 = -(((c01 * bx + c11 * by) + c12 * bz) / det)
        x2 = -(((c02 * bx + c12 * by) + c22 * bz) / det)
    sol = np.stack([x0, x1, x2], axis=1)
    with np.errstate(invalid="ignore"):
        accept = np.abs(det) > threshold
        if mutant != "no_box_test":
            accept &= ((sol >= 0.0) & (sol <= voxel)).all(axis=1)
        else:
            accept &= np.isfinite(sol).all(axis=1)
    out.vertices[accept] = corner[accept] + sol[accept]
    out.used_quadric = accept.astype(np.uint8)
    out.terms, out.A, out.b, out.x, out.det, out.threshold = terms, S[:, :6], S[:, 6:9], sol, det, threshold
    out.sum_norm_A, out.sum_norm_b = S[:, 9], S[:, 10]
    return out


def quadric_tolerance(ref: Clustered, voxel: float):
    """(tol [K], masked bool [K]) for comparing a float64 implementation of the rule that may sum in another order.

    tol_k = 8 (m_k + 8) 2^-53 ||A^-1||_2 (sum ||b_i|| + ||x|| sum ||A_i||): with A x = -b, a perturbation (dA, db) of the sums
    moves x by at most ||A^-1|| (||db|| + ||dA|| ||x||) to first order; a sum of m non-cancelling terms (every A_i is positive
    semidefinite; b_i is bounded by its norm) carries a rounding error of at most (m - 1) u sum ||.||, each term's own few
    roundings add a handful of u more (the + 8), and the leading 8 is headroom for the norm inequalities and the 3x3 solve.

    masked: the accept / reject decision itself lies within that error -- | |det| - threshold | below the error the sums'
    bound e = 8 (m + 8) u sum ||A_i|| induces in det and threshold (|d det| <= 3 ||A||_F^2 e, |d threshold| <= 1e-4 tr^2 e / 3,
    both with a factor 2 to spare), or an x that passes the determinant test within tol of a cell wall.  Such a cluster is compared on
    neither branch."""
    K = len(ref.det)
    A = np.zeros((K, 3, 3))
    for (r, c), i in {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}.items():
        A[:, r, c] = A[:, c, r] = ref.A[:, i]
    finite = np.isfinite(ref.x).all(axis=1)
    smallest = np.abs(np.linalg.eigvalsh(A)).min(axis=1)                # A is symmetric: ||A^-1||_2 = 1 / min |eigenvalue|
    with np.errstate(divide="ignore"):
        inv_norm = np.where(finite & (smallest > 0.0), 1.0 / smallest, np.inf)
    xn = np.where(finite, np.linalg.norm(np.where(np.isfinite(ref.x), ref.x, 0.0), axis=1), 0.0)
    head = 8.0 * (ref.terms + 8.0) * U
    with np.errstate(invalid="ignore"):
        tol = head * inv_norm * (ref.sum_norm_b + xn * ref.sum_norm_A)       # (nan where inf meets 0: never accepted there)
    e = head * ref.sum_norm_A
    tr = ref.A[:, 0] + ref.A[:, 3] + ref.A[:, 5]
    det_err = 2.0 * (3.0 * (A ** 2).sum(axis=(1, 2)) + 1e-4 * tr * tr / 3.0) * e
    masked = np.abs(np.abs(ref.det) - ref.threshold) < det_err          # (strict: sums of zeros carry no error)
    finite_tol = np.where(np.isfinite(tol), tol, 0.0)[:, None]
    with np.errstate(invalid="ignore"):
        near_wall = ((np.abs(ref.x) <= finite_tol) | (np.abs(ref.x - voxel) <= finite_tol)).any(axis=1)
    return tol, masked | ((np.abs(ref.det) > ref.threshold) & near_wall)
