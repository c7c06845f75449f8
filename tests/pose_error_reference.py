"""NumPy restatements of the BOP pose errors (pegasus_amd/pose_error.py, pegasus_amd/csrc/poseerr.hip.h).

errors_f64 / adi_f64   the seven errors from their definitions in float64; checked against the toolkit's own outputs
                       (tests/golden/bop_pose_errors.npz) by tests/test_pose_error_host.py, and the reference of the GPU tests
errors_f32 / adi_f32   the kernels' stated arithmetic: transforms composed in float64 and rounded once, every per-vertex
                       operation in float32 in the kernels' order, the means from float32 lane sums added in float64
"""
import math

import numpy as np

F = np.float32
LANES = 256


# ---- float64, from the definitions ----------------------------------------------------------------------------------
def transform(pts, R, t):
    return pts.dot(R.T) + t.reshape(1, 3)


def project(pts, K, R, t):
    cam = transform(pts, R, t)
    im = cam.dot(K.T)
    return im[:, :2] / im[:, 2:3]


def re_f64(R_est, R_gt):
    trace = 0.0
    for i in range(3):
        trace += (R_est[i, 0] * R_gt[i, 0] + R_est[i, 1] * R_gt[i, 1]) + R_est[i, 2] * R_gt[i, 2]
    return 180.0 * math.acos(min(1.0, max(-1.0, 0.5 * (float(trace) - 1.0)))) / math.pi


def te_f64(t_est, t_gt):
    d = np.asarray(t_gt, np.float64).reshape(3) - np.asarray(t_est, np.float64).reshape(3)
    return math.sqrt(float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def nearest_dists(queries, points, block=512):
    out = np.empty(len(queries), queries.dtype)
    for a in range(0, len(queries), block):
        d = queries[a:a + block, None, :] - points[None, :, :]
        out[a:a + block] = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(axis=1)
    return out


def adi_f64(pts, R_est, t_est, R_gt, t_gt):
    pts = np.asarray(pts, np.float64)
    return float(np.sqrt(nearest_dists(transform(pts, R_gt, t_gt), transform(pts, R_est, t_est))).mean())


def errors_f64(pts, sym_R, sym_t, R_est, t_est, R_gt, t_gt, K=None):
    """{mssd, mspd, add, proj, re, te} of one pair; pts [n,3], sym_R [S,3,3], sym_t [S,3] (index 0 the identity).  The
    estimate and every symmetric ground truth go through the same operations, so equal transforms give equal points."""
    pts = np.asarray(pts, np.float64)
    R_est, R_gt = np.asarray(R_est, np.float64), np.asarray(R_gt, np.float64)
    t_est, t_gt = np.asarray(t_est, np.float64).reshape(3), np.asarray(t_gt, np.float64).reshape(3)
    Rs = np.stack([R_est] + [R_gt.dot(R) for R in sym_R])
    ts = np.stack([t_est] + [R_gt.dot(t) + t_gt for t in sym_t])
    cam = np.einsum("vj,sij->svi", pts, Rs) + ts[:, None, :]
    d3 = np.linalg.norm(cam[1:] - cam[0], axis=2)
    out = {"mssd": float(d3.max(axis=1).min()), "add": float(d3[0].mean()), "re": re_f64(R_est, R_gt), "te": te_f64(t_est, t_gt)}
    if K is not None:
        im = np.einsum("svi,ji->svj", cam, np.asarray(K, np.float64))
        px = im[..., :2] / im[..., 2:3]
        d2 = np.linalg.norm(px[1:] - px[0], axis=2)
        out["mspd"] = float(d2.max(axis=1).min())
        out["proj"] = float(d2[0].mean())
    return out


# ---- float32, the kernels' arithmetic -------------------------------------------------------------------------------
def compose_gt_sym(R_gt, t_gt, sym_R, sym_t):
    """R_gt R_s and R_gt t_s + t_gt in float64 in the kernel's order, rounded to float32: ([S,3,3], [S,3])."""
    R_gt, t_gt = np.asarray(R_gt, np.float64), np.asarray(t_gt, np.float64).reshape(3)
    R = np.empty(sym_R.shape, np.float64)
    t = np.empty(sym_t.shape, np.float64)
    for i in range(3):
        for j in range(3):
            R[:, i, j] = (R_gt[i, 0] * sym_R[:, 0, j] + R_gt[i, 1] * sym_R[:, 1, j]) + R_gt[i, 2] * sym_R[:, 2, j]
        t[:, i] = ((R_gt[i, 0] * sym_t[:, 0] + R_gt[i, 1] * sym_t[:, 1]) + R_gt[i, 2] * sym_t[:, 2]) + t_gt[i]
    return R.astype(F), t.astype(F)


def _apply(R, t, p):
    """((R0 x + R1 y) + R2 z) + t per row in float32; R [...,3,3], t [...,3] broadcast against p [V,3] -> three [..., V]."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return tuple(((R[..., i, 0, None] * x + R[..., i, 1, None] * y) + R[..., i, 2, None] * z) + t[..., i, None] for i in range(3))


def lane_mean(values):
    """Mean of float32 ``values`` [V] as the kernels take it: lane l adds its values l, l + 256, ... in float32, the lane sums
    are added in float64 (butterfly inside each wave of 64, then the four waves in order)."""
    n = len(values)
    padded = np.zeros(-(-n // LANES) * LANES, F)
    padded[:n] = values
    lanes = np.add.reduce(padded.reshape(-1, LANES), axis=0, dtype=F).astype(np.float64)
    waves = lanes.reshape(4, 64)
    for d in (1, 2, 4, 8, 16, 32):
        waves = waves + waves[:, np.arange(64) ^ d]
    return F((((waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0]) / np.float64(n))


def errors_f32(pts, sym_R, sym_t, R_est, t_est, R_gt, t_gt, K=None):
    p = np.asarray(pts, F)
    Re, te = np.asarray(R_est, np.float64).astype(F), np.asarray(t_est, np.float64).reshape(3).astype(F)
    Rg, tg = compose_gt_sym(R_gt, t_gt, np.asarray(sym_R, np.float64), np.asarray(sym_t, np.float64))
    if K is None:
        fx, fy, cx, cy = F(1), F(1), F(0), F(0)
    else:
        K = np.asarray(K, np.float64)
        fx, fy, cx, cy = F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])
    with np.errstate(all="ignore"):
        Xe, Ye, Ze = _apply(Re, te, p)
        X, Y, Z = _apply(Rg, tg, p)
        dx, dy, dz = Xe - X, Ye - Y, Ze - Z
        d3 = (dx * dx + dy * dy) + dz * dz
        du = ((fx * Xe) / Ze + cx) - ((fx * X) / Z + cx)
        dv = ((fy * Ye) / Ze + cy) - ((fy * Y) / Z + cy)
        d2 = du * du + dv * dv
        assert d3.dtype == F and d2.dtype == F
        out = {"mssd": np.sqrt(np.fmax.reduce(d3, axis=1)).min(), "mspd": np.sqrt(np.fmax.reduce(d2, axis=1)).min(),
               "add": lane_mean(np.sqrt(d3[0])), "proj": lane_mean(np.sqrt(d2[0]))}
    out = {k: float(v) for k, v in out.items()}
    out["re"] = re_f64(np.asarray(R_est, np.float64), np.asarray(R_gt, np.float64))
    out["te"] = te_f64(t_est, t_gt)
    return out


def adi_query_transform(R_est, t_est, R_gt, t_gt):
    """M = R_est^T R_gt and c = R_est^T (t_gt - t_est) in float64 in the library's order, rounded to float32; M is the
    identity exactly when R_est equals R_gt element for element."""
    Re, Rg = np.asarray(R_est, np.float64), np.asarray(R_gt, np.float64)
    d = np.asarray(t_gt, np.float64).reshape(3) - np.asarray(t_est, np.float64).reshape(3)
    M, c = np.empty((3, 3)), np.empty(3)
    for i in range(3):
        for j in range(3):
            M[i, j] = (Re[0, i] * Rg[0, j] + Re[1, i] * Rg[1, j]) + Re[2, i] * Rg[2, j]
        c[i] = (Re[0, i] * d[0] + Re[1, i] * d[1]) + Re[2, i] * d[2]
    if np.array_equal(Re, Rg):
        M = np.eye(3)
    return M.astype(F), c.astype(F)


def adi_f32(pts, R_est, t_est, R_gt, t_gt):
    p = np.asarray(pts, F)
    M, c = adi_query_transform(R_est, t_est, R_gt, t_gt)
    q = np.stack(_apply(M, c, p), axis=1)
    best = nearest_dists(q, p)
    assert best.dtype == F
    dist = np.sqrt(best)
    total = 0.0
    for a in range(0, len(p), LANES):              # one float64 partial per workgroup of 256 queries, added in order
        group = np.zeros(LANES, np.float64)
        group[:len(dist[a:a + LANES])] = dist[a:a + LANES]
        waves = group.reshape(4, 64)
        for d in (1, 2, 4, 8, 16, 32):
            waves = waves + waves[:, np.arange(64) ^ d]
        total += ((waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0]
    return float(F(total / np.float64(len(p))))
