"""NumPy float64 reference of object posing, independent of the code under test (pegasus_amd/csrc/compose.hip.h:
compose_object_kernel, pose_reduce_kernel, pose_prepare_kernel, pose_apply_kernel).

Every function takes exactly the float32 values the kernels get, widened to float64 (never a float64 rotation the kernel did
not see), and returns float64.  Nothing here imports pegasus_amd or oracle: the SH basis constants are written out below, the
band matrices come from a least-squares solve over this module's own seeded directions, the quaternion of R from an
eigen-decomposition (never Shepperd's branches, which are what pose_prepare_kernel uses).

Tolerances.  u = 2^-24 is float32's unit roundoff (one rounding moves a value by at most u times its magnitude).  Each bound
below is a count of rounding steps times u times the magnitude the step acts on; none was read off a kernel's observed error.
"""
import numpy as np

U = 2.0 ** -24

# ---- positions ------------------------------------------------------------------------------------------------------
# out_i = fl(fl(s_i + c32_i) + t_i),  s_i = fma(R_i2, d_2, fma(R_i1, d_1, fl(R_i0 d_0))),  d_k = fl(x_k - c32_k),  c32 = fl(c).
# With S_i = sum_k |R_ik| |x_k - c_k| and C_i = sum_k |R_ik| |c_k| (R mixes the centre's rounding error across components, so
# the issue's per-element |c| is read as |c_i| + C_i: for a cloud at (1000, -2000, 500) the z row sees the 2000 of y through
# R, which |c_z| alone would not hold), to first order in u:
#   centre rounded to float32, through R                               1 u C_i
#   centre rounded to float32, added back                              1 u |c_i|
#   the subtraction x_k - c32_k, through R                             1 u S_i
#   three fused steps, each rounding a partial sum <= S_i              3 u S_i
#   + c32_i                                                            1 u (S_i + |c_i|)
#   + t_i                                                              1 u (S_i + |c_i| + |t_i|)
# R itself is the float32 matrix the reference also takes: no term.  The largest coefficient is 6 (on S_i); the fp64 mean of
# 2 000 003 rows differs from the exact mean by 2e-10 |c| (0.004 u) and second-order terms are smaller still; 6 plus that,
# rounded up to a power of two, times the magnitude sum |x_i| + |c_i| + C_i + |t_i| + S_i:
K_XYZ = 8
# ---- SH: one band row is 7 fused steps at most (7 u), D rounded to float32 once against the exact D used here (1 u), the
# coefficients exact; 8, and one for second-order terms:
K_SH = 9
# ---- device-built pose ----------------------------------------------------------------------------------------------
# quaternion: each component is one float64 result rounded to float32, and an entry of M(q) moves by at most
# 2 (|w|+|x|+|y|+|z|) u <= 4 u for that; a float32-ROUNDED rotation is off a true one by under 1 u more; rounded up: 8 u.
K_QUAT = 8
# A matrix that is not a rotation to float32 rounding (an accumulated float32 trajectory) adds its own distance from one, which
# Shepperd's formula (linear in the entries, then normalised) and the nearest rotation (this module) resolve differently.
# With delta = max |R^T R - I|:  R = Q (I + S), max |S| <= delta / 2 to first order, E = Q S has max |E| <= 3 max |S|; a
# component of Shepperd's unnormalised vector (length 4 q_max >= 2) reads at most 3 entries, so |dq| <= sqrt(9 + 3 * 4) max |E|
# / 2 = 2.3 max |E|, and an entry of M(q) moves by at most 4 |dq|:  4 * 2.3 * 1.5 delta = 13.8 delta, rounded up to 16 delta.
# Rounding a true rotation to float32 gives delta <= 2 u, which K_QUAT already holds; only the excess counts: for the 52 cases
# that are float32-rounded rotations the bounds ARE 8 u and 2e-6; the accumulated trajectory (delta = 2.76e-6 = 46 u) alone gets
# the allowance, 16 (delta - 2 u) = 4.2e-5, a worst-case count that a small error in q could hide under on that one case.
K_QUAT_NONORTHO = 16
# band matrices: one float64 result (|D_ij| <= 1) rounded to float32 is 1 u; both constructions are exact to 1e-13; 2 u.
K_D = 2
# centre: one float64 mean rounded to float32: u |c|, plus 1e-12 absolute for a centre at zero.
CENTER_ABS = 1e-12
# the project's existing numbers (tests/test_compose.py)
ORIENT_ATOL = 2e-6
UNIT_ATOL = 1e-6
NORM_FLOOR = 1e-12                       # F.normalize's eps: q / max(|q|, 1e-12)

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)
BANDS = {1: slice(1, 4), 2: slice(4, 9), 3: slice(9, 16)}


def f64(a):
    """float32 values widened to float64; refuses anything that is not exactly representable in float32."""
    a = np.asarray(a)
    w = a.astype(np.float64)
    if a.dtype != np.float32:
        with np.errstate(over="ignore", invalid="ignore"):
            assert np.array_equal(w.astype(np.float32).astype(np.float64), w, equal_nan=True), "not float32 values"
    return w


def basis(d):
    """[M,16] values of the 3DGS real-SH basis (degree 3) at directions d [M,3] (any length: homogeneous polynomials)."""
    d = np.asarray(d, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([
        np.full_like(x, C0),
        -C1 * y, C1 * z, -C1 * x,
        C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
        C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
        C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)], axis=1)


def _own_directions(m=384, seed=20240611):
    d = np.random.default_rng(seed).normal(size=(m, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


_DIRS = _own_directions()
_BASIS = basis(_DIRS)


def band_matrices(R32):
    """(D1 [3,3], D2 [5,5], D3 [7,7]) with c'_l = D_l c_l, from f'(d) = f(R^T d).  Y_lm(R^T d) is a homogeneous polynomial of
    degree l in d, so on the sphere it lies in bands l, l-2, ...: ALL 16 functions are fitted jointly (an exact fit for any
    matrix, a rotation or not) and D_l is the fit's band-l block, the L2 projection onto the band."""
    R = f64(R32).reshape(3, 3)
    X, res, rank, _ = np.linalg.lstsq(_BASIS, basis(_DIRS @ R), rcond=None)          # (R^T d)^T = d^T R
    assert rank == 16
    return tuple(X[s, s] for s in BANDS.values())


def rotate_rest(f_rest32, R32):
    """f_rest [n, n_rest, 3] (n_rest in 0, 3, 8, 15) -> (rotated float64, per-element magnitude sum_k |D_ik| |c_k|)."""
    c = f64(f_rest32)
    n_rest = c.shape[1]
    out, mag = np.zeros_like(c), np.zeros_like(c)
    for D, lo, hi in zip(band_matrices(R32), (0, 3, 8), (3, 8, 15)):
        if n_rest >= hi:
            out[:, lo:hi] = np.einsum("ij,njc->nic", D, c[:, lo:hi])
            mag[:, lo:hi] = np.einsum("ij,njc->nic", np.abs(D), np.abs(c[:, lo:hi]))
    return out, mag


def center_of(xyz32):
    x = f64(xyz32).reshape(-1, 3)
    return x.mean(axis=0) if len(x) else np.zeros(3)


def positions(xyz32, R32=None, t32=None, about_origin=False, center=None):
    """R (x - c) + c + t and the per-element magnitude sum |x_i| + |c_i| + sum_k |R_ik| |c_k| + |t_i| + sum_k |R_ik| |x_k - c_k|
    the tolerance K_XYZ * U is scaled by (one term more than the issue's sum: the centre's rounding error reaches row i through
    R, see K_XYZ).  c: the float64 mean of the
    float32 rows; zero for about_origin; R = None is the identity about nothing (c = 0), t = None is zero.  ``center``: a centre
    handed to the kernel from outside (pgr_compose_object), as float32 values."""
    x = f64(xyz32).reshape(-1, 3)
    if R32 is None:
        R, c = np.eye(3), np.zeros(3)
    else:
        R = f64(R32).reshape(3, 3)
        c = np.zeros(3) if about_origin else (center_of(xyz32) if center is None else f64(center))
    t = np.zeros(3) if t32 is None else f64(t32).reshape(3)
    d = x - c
    out = d @ R.T + c + t
    mag = np.abs(x) + np.abs(c) + np.abs(R) @ np.abs(c) + np.abs(t) + np.abs(d) @ np.abs(R).T
    return out, mag


def quat_matrix(q):
    """[..., 4] (w,x,y,z) -> [..., 3, 3] of q AS GIVEN (no normalisation: M is quadratic in q)."""
    q = np.asarray(q, np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    n = w * w + x * x + y * y + z * z
    M = np.stack([n - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), n - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), n - 2 * (x * x + y * y)], axis=-1)
    return M.reshape(q.shape[:-1] + (3, 3))


def normalize_rule(rot32):
    """The reference's F.normalize: q / max(|q|, 1e-12), in float64 -> (rows, |q|)."""
    q = f64(rot32).reshape(-1, 4)
    norm = np.linalg.norm(q, axis=1)
    return q / np.maximum(norm, NORM_FLOOR)[:, None], norm


def orientations(rot32, R32=None):
    """R @ M(q / max(|q|, 1e-12)) [n,3,3] and the norm |q / max(|q|, 1e-12)| the output quaternion must have."""
    qn, norm = normalize_rule(rot32)
    R = np.eye(3) if R32 is None else f64(R32).reshape(3, 3)
    return R @ quat_matrix(qn), np.linalg.norm(qn, axis=1)


def non_orthonormality(R32):
    R = f64(R32).reshape(3, 3)
    return float(np.abs(R.T @ R - np.eye(3)).max())


def orient_bound(R32):
    """Bound on |M(q_out) - R M(q_in)| entries: the project's 2e-6 for a rotation; a matrix off a rotation by delta cannot be
    matched by ANY quaternion closer than that, counted as for the quaternion itself (K_QUAT_NONORTHO)."""
    return ORIENT_ATOL + K_QUAT_NONORTHO * max(0.0, non_orthonormality(R32) - 2 * U)


def quat_bound(R32):
    """Bound on |M(q_device) - M(q_reference)| entries: see K_QUAT, K_QUAT_NONORTHO above."""
    return K_QUAT * U + K_QUAT_NONORTHO * max(0.0, non_orthonormality(R32) - 2 * U)


def quat_of(R32):
    """Unit quaternion (w,x,y,z), w >= 0 where it matters not, of the rotation nearest to R: the eigenvector of the largest
    eigenvalue of Bar-Itzhack's symmetric 4x4 matrix.  No branches on the trace or the diagonal."""
    return quat_of_f64(f64(R32))


def quat_of_f64(m):
    """quat_of on float64 entries (host tests feed it true rotations; the kernels' inputs go through quat_of)."""
    m = np.asarray(m, np.float64).reshape(3, 3)
    K = np.array([[m[0, 0] - m[1, 1] - m[2, 2], m[1, 0] + m[0, 1], m[2, 0] + m[0, 2], m[2, 1] - m[1, 2]],
                  [m[1, 0] + m[0, 1], m[1, 1] - m[0, 0] - m[2, 2], m[2, 1] + m[1, 2], m[0, 2] - m[2, 0]],
                  [m[2, 0] + m[0, 2], m[2, 1] + m[1, 2], m[2, 2] - m[0, 0] - m[1, 1], m[1, 0] - m[0, 1]],
                  [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], m[0, 0] + m[1, 1] + m[2, 2]]]) / 3.0
    val, vec = np.linalg.eigh(K)
    x, y, z, w = vec[:, -1]
    q = np.array([w, x, y, z])
    return q / np.linalg.norm(q)


BRANCHES = ("trace", "x", "y", "z")
TIES = ("tr==m00", "tr==m11", "tr==m22", "m00==m11", "m00==m22", "m11==m22")


def census(R32):
    """What R presents to pose_prepare_kernel's comparisons (fp64 on the widened float32 entries, tr = m00 + m11 + m22 summed
    left to right): the set holding the branch taken and every tie between the compared quantities."""
    m = f64(R32).reshape(3, 3)
    m00, m11, m22 = m[0, 0], m[1, 1], m[2, 2]
    tr = m00 + m11 + m22
    if tr >= m00 and tr >= m11 and tr >= m22:
        keys = {"trace"}
    elif m00 >= m11 and m00 >= m22:
        keys = {"x"}
    elif m11 >= m22:
        keys = {"y"}
    else:
        keys = {"z"}
    for name, a, b in (("tr==m00", tr, m00), ("tr==m11", tr, m11), ("tr==m22", tr, m22), ("m00==m11", m00, m11),
                       ("m00==m22", m00, m22), ("m11==m22", m11, m22)):
        if a == b:
            keys.add(name)
    return keys
