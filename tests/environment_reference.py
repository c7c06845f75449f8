"""NumPy restatement of the environment field (pegasus_amd/csrc/envfield.hip.h) and of the ground in the
rigid-body rule (pegasus_amd/csrc/rigid.hip.h): what pgr_sdf_from_tsdf and the *_ground entries are held against.  It shares no
code with the package.  dist2 is brute force over all pairs of grid points; phi is stated twice, in float64 and in float32
operation by operation.

The rule.  inside(p) <=> tsdf(p) < 0 (a NaN is outside); s = -1 inside, +1 outside.  D2(p) = min |p - q|^2 over the grid points q
with inside(q) != inside(p), in voxels, NONE (-1) without one.  p is a band point if an in-grid 6-neighbour n (order -x, +x, -y,
+y, -z, +z) has the other sign; beta(p) = min_n a / (a + b), a = |tsdf(p)|, b = |tsdf(n)|, 1 for a value that is not finite.
phi = s voxel beta (band), s voxel (sqrt(D2) - 0.5) (other points with a D2), s voxel (nx + ny + nz) (NONE).

float32 (phi32).  (float) D2 is exact (D2 < 2^22).  sqrtf and the division are correctly rounded on the device (the library is
built without fast-math; HIP's default is the correctly rounded pair) as numpy's float32 sqrt and division are, the subtraction
and the products are single IEEE operations, and the minimum of numbers that are not NaN is exact: phi32 is the device's value
bit for bit, no counted bound is needed.  a + b > 0 always: one of the two values is < 0, so its magnitude is > 0 (or counts 1).

Accuracy (rule_bounds), in voxels, against the exact distance d to a surface S whose carved volume holds clip(d / truncation)
with a truncation of at least one voxel, for a solid and a free space that are, near S, more than a voxel thick along every
axis (a half space, a box wider than a voxel, a ball of a few voxels):
  other points.  Take p outside, d = d(p) > 0; the inside case mirrors it.  Every inside grid point q is at least d away (the
    segment p q crosses S), so sqrt(D2) >= d.  Let s be the point of S nearest to p and q the grid point whose coordinate on each
    axis is the first grid coordinate from s_i in the direction away from the outward normal (q_i = s_i where n_i = 0 and s_i is
    a grid coordinate): |q_i - s_i| <= 1, (q - s).n <= 0, q is inside, and |p - q| <= d + sqrt(3).  So
        d - 0.5  <=  phi  <=  d + sqrt(3) - 0.5.
  band points.  p outside with an inside neighbour n one voxel away: d is 1-Lipschitz, so d(p) + |d(n)| <= 1, both unclipped
    (truncation >= 1 voxel), and beta = d(p) / (d(p) + |d(n)|) >= d(p); beta <= 1.  So  d <= phi <= 1  and  phi - d < 1.
  Together  -0.5 <= phi - d <= sqrt(3) - 0.5 = 1.232  (LOW, HIGH).  The trial on 32^3 grids stayed inside [-0.5, +0.79].
A trilinear sample is a convex combination of the cell's corners, each within |x - c| of d(x) (d is 1-Lipschitz), and the
weighted corner distance is at most sqrt(3)/2 (collision_cases.drop_slack): a sample of the field is within
    E_g = (sqrt(3)/2 + sqrt(3) - 0.5) voxel = 2.098 voxel
above d(x), and within (sqrt(3)/2 + 0.5) voxel below it: what ground_slack returns.
"""
import contextlib

import numpy as np

import collision_reference as CR
import dynamics_reference as DR

NONE = -1
LOW, HIGH = -0.5, 3.0 ** 0.5 - 0.5
NEIGHBOURS = ((0, -1), (0, +1), (1, -1), (1, +1), (2, -1), (2, +1))      # (axis x, y, z; step) in the rule's order


def ground_slack(voxel):
    """E_g: how far above the exact distance a trilinear sample of the field can lie."""
    return (0.5 * 3.0 ** 0.5 + HIGH) * float(voxel)


def inside(tsdf):
    return np.asarray(tsdf) < 0                                          # (NaN < 0 is False)


def dist2(tsdf, block=1024):
    """int64 [nz,ny,nx]: D2 by brute force over all pairs, NONE without a point of the other sign."""
    t = np.asarray(tsdf)
    nz, ny, nx = t.shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = np.stack([i, j, k], axis=-1).reshape(-1, 3).astype(np.float64)   # small integers: every product below is exact
    cls = inside(t).reshape(-1)
    out = np.full(len(p), NONE, np.int64)
    for mine in (False, True):
        a, b = np.flatnonzero(cls == mine), np.flatnonzero(cls != mine)
        if len(a) == 0 or len(b) == 0:
            continue
        qb, qq = p[b], (p[b] ** 2).sum(1)
        for s in range(0, len(a), block):
            pa = p[a[s:s + block]]
            d2 = (pa ** 2).sum(1)[:, None] + qq[None, :] - 2.0 * (pa @ qb.T)
            out[a[s:s + block]] = np.rint(d2.min(1)).astype(np.int64)
    return out.reshape(t.shape)


def _magnitude(t, dtype):
    t = np.asarray(t, dtype)
    return np.where(np.isfinite(t), np.abs(t), dtype(1.0)).astype(dtype)


def band(tsdf, dtype=np.float64):
    """(is a band point bool [nz,ny,nx], beta [nz,ny,nx] in ``dtype``, inf where it is none): the minimum in the rule's order,
    every quotient one ``dtype`` addition and one division."""
    t = np.asarray(tsdf, np.float32)
    ins, a = inside(t), _magnitude(t, dtype)
    is_band = np.zeros(t.shape, bool)
    beta = np.full(t.shape, np.inf, dtype)
    for axis, step in NEIGHBOURS:
        ax = 2 - axis                                                    # the array is [z, y, x]
        n = t.shape[ax]
        me = [slice(None)] * 3
        nb = [slice(None)] * 3
        me[ax] = slice(1, n) if step < 0 else slice(0, n - 1)
        nb[ax] = slice(0, n - 1) if step < 0 else slice(1, n)
        me, nb = tuple(me), tuple(nb)
        other = ins[me] != ins[nb]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (a[me] / (a[me] + a[nb]).astype(dtype)).astype(dtype)
        beta[me] = np.where(other, np.minimum(beta[me], q), beta[me])
        is_band[me] |= other
    return is_band, beta


def _phi(tsdf, voxel, d2, dtype):
    t = np.asarray(tsdf, np.float32)
    nz, ny, nx = t.shape
    voxel = dtype(np.float32(voxel))
    is_band, beta = band(t, dtype)
    root = np.sqrt(np.maximum(d2, 0).astype(dtype)).astype(dtype)
    m = np.where(is_band, voxel * np.where(is_band, beta, dtype(0)),
                 np.where(d2 == NONE, voxel * dtype(nx + ny + nz), voxel * (root - dtype(0.5)).astype(dtype))).astype(dtype)
    return np.where(inside(t), -m, m).astype(dtype)


def phi64(tsdf, voxel, d2=None):
    """The field in float64 (from the float32 volume and voxel the device gets)."""
    return _phi(tsdf, voxel, dist2(tsdf) if d2 is None else d2, np.float64)


def phi32(tsdf, voxel, d2=None):
    """The field in float32, operation by operation: the device's bits (module docstring)."""
    return _phi(tsdf, voxel, dist2(tsdf) if d2 is None else d2, np.float32)


def rule_bounds():
    return LOW, HIGH


# ---- the ground in the rigid-body rule -------------------------------------------------------------------------------------
class RefGround:
    """field [nz,ny,nx] (the device's, read back, or the reference's own) on a RefGrid, and the friction."""

    def __init__(self, field, grid, friction=0.5):
        self.field = np.asarray(field, np.float64)
        self.grid = grid
        self.friction = float(np.float32(friction))


def ground_points(types, type_row, state, a, ground, idx=None):
    """dynamics_reference.pair_points against the ground: the plane branch with collision_reference.sample on the ground's field
    at the world point itself, the unit gradient as the normal (no rotation)."""
    A = types[type_row[a]]
    Ra, Ta = DR.frame(state[a], A.com)
    s = A.shell if idx is None else A.shell[np.asarray(idx, np.int64)]
    p = s @ Ra.T + Ta
    reach = max(1.0, float(np.abs(p).max()) if len(p) else 1.0, float(np.abs(state[:, :3]).max()))
    phi, grad, info = CR.sample(ground.field, ground.grid, p, True)
    gn = np.linalg.norm(grad, axis=1)
    ok = gn >= 1e-6
    normal = grad / np.where(ok, gn, 1.0)[:, None]
    return p, phi, normal, ok, CR.sweep_step_bound(reach, CR.sample_bound(ground.grid, info)) + 2.0 * DR.U * reach


def ground_in_range(types, type_row, state, a, ground, params, sphere=True):
    """(the ground's sphere test lets mover a through, how far the test is from its threshold); ``sphere`` False: no early-out."""
    if not sphere:
        return True, np.inf
    value, _, _ = CR.sample(ground.field, ground.grid, state[a:a + 1, :3])
    gap = (float(value[0]) - types[type_row[a]].radius) - 2.0 * ground.grid.voxel
    return not gap > params.margin, abs(gap - params.margin)


@contextlib.contextmanager
def ground_rule(ground, sphere=True):
    """Inside the block dynamics_reference's plane IS the ground: its pair_points and in_range take the ground for b == PLANE, so
    world_words, build_rows, step and simulate follow the ground's rule with their own code.  The caller's Params carry the
    ground's friction as plane_friction (ground_params)."""
    pair_points, in_range = DR.pair_points, DR.in_range

    def points(types, type_row, state, a, b, params, idx=None):
        if b == DR.PLANE:
            return ground_points(types, type_row, state, a, ground, idx)
        return pair_points(types, type_row, state, a, b, params, idx)

    def near(types, type_row, state, a, b, params):
        if b == DR.PLANE:
            return ground_in_range(types, type_row, state, a, ground, params, sphere)
        return in_range(types, type_row, state, a, b, params)

    DR.pair_points, DR.in_range = points, near
    try:
        yield
    finally:
        DR.pair_points, DR.in_range = pair_points, in_range
