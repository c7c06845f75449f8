"""NumPy float64 restatement of the collision geometry (pegasus_amd/csrc/meshsdf.hip.h, pegasus_amd/collision.py): what the
kernels are held against.  It shares no code with the package: the distance is Ericson's closest-point regions (the kernel takes
the minimum over segments and an interior solve), the grid, the trilinear cell, the sphere tracing and the placement loop are
written out again here.

The error bounds are counted, not fitted.  u = 2^-24 is the unit roundoff of float32; every float32 operation is rounded on its
own (the library is built without contraction).

Distance (distance_bound).  Inputs are exact: the vertices are float32, the grid point is the float32 number the kernel's own rule
gives (grid_points repeats it).  For a face with longest edge L at exact distance d from p every difference a - p, b - p, c - p and
every edge is at most M = d + L long.
  segment (u, v):  U = u - p and e = v - u carry u each, relatively.  U.e: 2u from its inputs, 3u from 3 products and 2 sums that
    matter (first order): 5u |U||e|; e.e likewise 5u e.e; the quotient t adds 1u: |dt| <= 11u |U|/|e|.  Clamping does not raise it.
    q = U + t e:  |e||dt| = 11u |U|, the product t e carries 2u |e| (its rounding and e's), the sum 1u |q|, U itself 1u |U|:
    |dq| <= 15u M.  sqrt(q.q): 3u on q.q halves to 1.5u, the root adds 1u: 2.5u d.  A point q(t) with t in [0,1] is a point of the
    segment and the distance is 1-Lipschitz in q and stationary in t at the optimum, so the segment candidate is within 18u M.
  interior:  q = (A + v e1) + w e2 with v, w >= 0, v + w <= 1 is a point of the triangle up to its own rounding (1u |A|, 2u |v e1|,
    2u |w e2|, 2u |q|, 1u L for v + w = 1 + u: 8u M), so a candidate can undercut the exact distance by 8u M + 2.5u d at most,
    however badly (v, w) are solved: a sliver or a zero-area face costs nothing on that side.  Where the closest point IS
    interior the candidate must also be close from above.  g11, g12, g22 carry 5u relatively, h1, h2 5u |A||e|; each product of two
    1u more, so det = g11 g22 - g12 g12 is off by 12u (g11 g22 + g12^2) <= 24u g11 g22 = 24u kappa det with
    kappa = g11 g22 / det (1 / sin^2 of the angle at a), and the numerators by 24u |e1||e2|^2 |A| (|e1|^2 |e2||A|); v = num / det
    then moves the point in the plane by |e1||dv| <= (24 + 24 + 2)u kappa |A|, w likewise: |delta| <= 100u kappa M in the plane.
    The candidate is sqrt(d^2 + delta^2) <= d + |delta|; if (v, w) is pushed out of the triangle the point was within |delta| of
    its boundary and the segments give the same.
  Together: |d_gpu - d_ref| <= (18 + 100 kappa) u (d + L), kappa the largest over the faces with area, L the longest edge.  The
  faces far from p cannot win: their own error is the same few u of a distance many times d.

Sample (sample_bound).  With F the largest |corner| of the cell and n the most points on an axis: each lerp a + t (b - a) is 3
  roundings of numbers <= 2F: 6u F, three levels deep: 18u F.  The fraction f = (p - o) / voxel - i is off by 2u |g| <= 2u n (the
  reference takes it in float64 from the same float32 p, o, voxel), and the value changes by at most the corner spread <= 2F per
  unit of each of the three fractions: 12u n F.  Across a cell border the trilinear value is continuous, so choosing the other cell
  costs nothing.  Outside, o = (g - gc) voxel adds 2u |g| voxel + 2u |o| per axis, and sqrt(r^2 + m^2) is 1-Lipschitz in both and adds 3u of
  itself:  16u max(|p - o|, r) on top of the field's own bound.
  Gradient: differences of corners (1u each), two lerps, a division: 12u D / voxel with D the corner spread, plus the fraction's
  2u n on a second difference <= 2D per other axis: (12 + 8n) u D / voxel; compared only away from cell borders.

Sweep (sweep_step_bound).  The point in the target's frame is three float32 affine maps of numbers <= P (the largest coordinate
  in play): 4u + 3u + 3u + 2u for s dir: 12u sqrt(3) P in position, times the trilinear cell's slope <= sqrt(3): 36u P, plus the
  sample bound.  Each step of the sphere tracing repeats it.
"""
import math

import numpy as np

U = 2.0 ** -24


# ---- grid ---------------------------------------------------------------------------------------------------------------
class RefGrid:
    """nx, ny, nz, origin [3], voxel: the float32 numbers the device gets, held as float64."""

    def __init__(self, nx, ny, nz, origin, voxel):
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.origin = np.asarray(origin, np.float32).astype(np.float64)
        self.voxel = float(np.float32(voxel))

    @property
    def shape(self):
        return (self.nz, self.ny, self.nx)

    @property
    def n(self):
        return np.array([self.nx, self.ny, self.nz])


def grid_around(lo, hi, resolution):
    """The grid over [lo, hi] with ``resolution`` points on the longest axis, centred (what Grid.around promises)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    voxel = ext.max() / (resolution - 1)
    n = [max(2, math.ceil(e / voxel - 1e-9) + 1) for e in ext]
    origin = [0.5 * (a + b) - 0.5 * voxel * (k - 1) for a, b, k in zip(lo, hi, n)]
    return RefGrid(n[0], n[1], n[2], origin, voxel)


def body_grid(vertices, resolution):
    """The grid of MeshSDF.from_mesh with its default padding of two voxels."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    pad = 2.0 * (hi - lo).max() / (resolution - 5)
    return grid_around(lo - pad, hi + pad, resolution)


def grid_points(g: RefGrid) -> np.ndarray:
    """[nz,ny,nx,3] float64 holding the float32 points of the kernel's rule: origin + voxel * (float) index, two roundings."""
    o, vx = g.origin.astype(np.float32), np.float32(g.voxel)
    axes = [o[a] + vx * np.arange(k, dtype=np.float32) for a, k in enumerate((g.nx, g.ny, g.nz))]
    assert all(a.dtype == np.float32 for a in axes)
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x, y, z], axis=-1).astype(np.float64)


# ---- exact distance and winding number ----------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def _segment_distance(p, a, b):
    e = b - a
    ee = _dot(e, e)
    t = np.clip(_dot(p - a, e) / ee, 0.0, 1.0) if ee > 0 else 0.0
    q = a + np.asarray(t)[..., None] * e
    return np.linalg.norm(p - q, axis=-1)


def point_triangle_distance(p, a, b, c):
    """[N]: the distance from every p [N,3] to the triangle (a, b, c) by closest-point regions (Ericson, Real-Time Collision
    Detection 5.1.5); a triangle without area is its longest segment."""
    ab, ac = b - a, c - a
    n = np.cross(ab, ac)
    if _dot(n, n) <= 1e-28 * max(_dot(ab, ab), _dot(ac, ac), _dot(c - b, c - b)) ** 2:
        return np.minimum(np.minimum(_segment_distance(p, a, b), _segment_distance(p, b, c)), _segment_distance(p, c, a))
    ap, bp, cp = p - a, p - b, p - c
    d1, d2 = _dot(ap, ab), _dot(ap, ac)
    d3, d4 = _dot(bp, ab), _dot(bp, ac)
    d5, d6 = _dot(cp, ab), _dot(cp, ac)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    q = np.empty_like(p)
    done = np.zeros(len(p), bool)

    def put(mask, value):
        m = mask & ~done
        q[m] = value[m] if np.ndim(value) == 2 else value
        done[m] = True

    with np.errstate(divide="ignore", invalid="ignore"):
        put((d1 <= 0) & (d2 <= 0), a)
        put((d3 >= 0) & (d4 <= d3), b)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[:, None] * ab)
        put((d6 >= 0) & (d5 <= d6), c)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[:, None] * ac)
        put((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b))
        den = va + vb + vc
        put(np.ones(len(p), bool), a + (vb / den)[:, None] * ab + (vc / den)[:, None] * ac)
    return np.linalg.norm(p - q, axis=-1)


def solid_angle(p, a, b, c):
    """[N]: the signed solid angle of (a, b, c) from every p (Van Oosterom and Strackee 1983)."""
    A, B, C = a - p, b - p, c - p
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (A, B, C))
    num = _dot(A, np.cross(B, C))
    den = la * lb * lc + _dot(A, B) * lc + _dot(A, C) * lb + _dot(B, C) * la
    return 2.0 * np.arctan2(num, den)


def mesh_distance(points, vertices, faces, want_winding=True):
    """(distance [N] >= 0, winding number [N]) of float64 points against a float32 mesh; +inf and 0 without faces.  A face with an
    index outside the vertices adds nothing."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    d = np.full(len(p), np.inf)
    w = np.zeros(len(p))
    for f in np.asarray(faces, np.int64).reshape(-1, 3):
        if f.min() < 0 or f.max() >= len(v):
            continue
        a, b, c = v[f[0]], v[f[1]], v[f[2]]
        d = np.minimum(d, point_triangle_distance(p, a, b, c))
        if want_winding:
            w += solid_angle(p, a, b, c)
    return d, w / (4.0 * np.pi)


def signed(d, w):
    return np.where(w >= 0.5, -d, d)


def mesh_shape(vertices, faces):
    """(longest edge, kappa: the largest g11 g22 / det over the faces with area, the bounding box's diagonal)."""
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    L, kappa = 0.0, 1.0
    for f in np.asarray(faces, np.int64).reshape(-1, 3):
        if f.min() < 0 or f.max() >= len(v):
            continue
        a, b, c = v[f[0]], v[f[1]], v[f[2]]
        e1, e2 = b - a, c - a
        L = max(L, np.linalg.norm(e1), np.linalg.norm(e2), np.linalg.norm(c - b))
        g11, g12, g22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
        det = g11 * g22 - g12 * g12
        if det > 1e-14 * g11 * g22:
            kappa = max(kappa, g11 * g22 / det)
    diag = float(np.linalg.norm(v.max(0) - v.min(0))) if len(v) else 0.0
    return float(L), float(kappa), diag


def distance_bound(d, L, kappa):
    """The counted bound on |d_gpu - d_ref| (module docstring)."""
    return (18.0 + 100.0 * kappa) * U * (np.asarray(d) + L)


# ---- trilinear samples ----------------------------------------------------------------------------------------------------
def _cell(g: RefGrid, p):
    p = np.asarray(p, np.float32).astype(np.float64).reshape(-1, 3)
    gc_raw = (p - g.origin) / g.voxel
    gc = np.clip(np.nan_to_num(gc_raw, nan=0.0, posinf=np.inf, neginf=-np.inf), 0.0, g.n - 1.0)
    i = np.minimum(gc.astype(np.int64), g.n - 2)
    return p, gc_raw, gc, i, gc - i


def sample(field, g: RefGrid, points, want_gradient=False):
    """(value [N], gradient [N,3] or None, info) of the trilinear rule on a field [nz,ny,nx], float64.  info holds per point the
    largest |corner| (F), the corner spread (D), the distance to the box (r) and the distance of the fractions from a cell border."""
    fld = np.asarray(field, np.float64)
    p, gr, gc, i, f = _cell(g, points)
    c = {}
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                c[dx, dy, dz] = fld[i[:, 2] + dz, i[:, 1] + dy, i[:, 0] + dx]
    lerp = lambda a, b, t: a + t * (b - a)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    x00, x10 = lerp(c[0, 0, 0], c[1, 0, 0], fx), lerp(c[0, 1, 0], c[1, 1, 0], fx)
    x01, x11 = lerp(c[0, 0, 1], c[1, 0, 1], fx), lerp(c[0, 1, 1], c[1, 1, 1], fx)
    y0, y1 = lerp(x00, x10, fy), lerp(x01, x11, fy)
    phi = lerp(y0, y1, fz)
    grad = None
    if want_gradient:
        dx = lerp(lerp(c[1, 0, 0] - c[0, 0, 0], c[1, 1, 0] - c[0, 1, 0], fy), lerp(c[1, 0, 1] - c[0, 0, 1], c[1, 1, 1] - c[0, 1, 1], fy), fz)
        grad = np.stack([dx, lerp(x10 - x00, x11 - x01, fz), y1 - y0], axis=1) / g.voxel
    o = (gr - gc) * g.voxel
    r = np.linalg.norm(o, axis=1)
    value = np.where(r > 0, np.sqrt(r * r + np.maximum(phi, 0.0) ** 2), phi)
    corners = np.stack(list(c.values()), axis=1)
    info = dict(F=np.abs(corners).max(1), D=corners.max(1) - corners.min(1), r=r, border=np.minimum(f, 1 - f).min(1),
                reach=np.abs(p - g.origin).max(1))
    return value, grad, info


def sample_bound(g: RefGrid, info):
    n = float(max(g.n))
    return (18.0 + 12.0 * n) * U * info["F"] + np.where(info["r"] > 0, 16.0 * U * np.maximum(info["reach"], info["r"]), 0.0)


def gradient_bound(g: RefGrid, info):
    n = float(max(g.n))
    return (12.0 + 8.0 * n) * U * info["D"] / g.voxel


# ---- sweeps -----------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def world_points(shell, T):
    T = np.asarray(T, np.float64)
    return f32(shell).reshape(-1, 3) @ f32(T[:3, :3]).T + f32(T[:3, 3])


def sweep_body(field, g: RefGrid, shell, Ta, Tb, direction, tol, max_travel, max_steps):
    """(phi0 [n], travel [n], steps [n], worst: per point the largest sample bound met) of shell points of a body at pose Ta
    against the field of a body at pose Tb, by the rule of pgr_sdf_sweep in float64."""
    x = world_points(shell, Ta)
    Rb, tb, d = f32(np.asarray(Tb)[:3, :3]), f32(np.asarray(Tb)[:3, 3]), f32(direction)
    tol, max_travel = float(np.float32(tol)), float(np.float32(max_travel))

    def phi_at(s, idx):
        y = ((x[idx] + s[:, None] * d) - tb) @ Rb
        value, _, info = sample(field, g, y)
        return value, sample_bound(g, info)

    every = np.arange(len(x))
    phi0, worst = phi_at(np.zeros(len(x)), every)
    s, phi, steps = np.zeros(len(x)), phi0.copy(), np.zeros(len(x), np.int64)
    for _ in range(int(max_steps)):
        go = (phi > tol) & (s < max_travel)
        if not go.any():
            break
        idx = every[go]
        s[idx] = np.minimum(s[idx] + phi[idx], max_travel)
        phi[idx], b = phi_at(s[idx], idx)
        worst[idx] = np.maximum(worst[idx], b)
        steps[idx] += 1
    return phi0, s, steps, worst


def sweep_plane(shell, Ta, plane, direction, tol, max_travel):
    x = world_points(shell, Ta)
    pl, d = f32(plane), f32(direction)
    tol, max_travel = float(np.float32(tol)), float(np.float32(max_travel))
    phi0 = x @ pl[:3] - pl[3]
    c = -float(pl[:3] @ d)
    s = np.where(phi0 <= tol, 0.0, np.minimum(phi0 / c, max_travel) if c > 0 else max_travel)
    return phi0, s


def sweep_step_bound(reach, sample_worst):
    """The counted bound on one evaluation of the field at a swept point; ``reach``: the largest coordinate in play."""
    return 36.0 * U * reach + sample_worst


def order_bits(value) -> int:
    u = int(np.float32(value).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else u ^ 0x80000000


def word(value, index) -> int:
    return (order_bits(value) << 32) | int(index)


# ---- placement ----------------------------------------------------------------------------------------------------------
class RefBody:
    """A mesh with its exact float64 field on the grid MeshSDF.from_mesh would build."""

    def __init__(self, vertices, faces, resolution):
        self.vertices = np.asarray(vertices, np.float32)
        self.faces = np.asarray(faces, np.int32)
        self.grid = body_grid(self.vertices, resolution)
        d, w = mesh_distance(grid_points(self.grid).reshape(-1, 3), self.vertices, self.faces)
        self.field = signed(d, w).reshape(self.grid.shape)
        self.size = float(np.linalg.norm(np.ptp(self.vertices.astype(np.float64), axis=0)))


def drop_reference(bodies, orientations, xy, tol=1e-4, max_rounds=8, max_steps=128):
    """The placement loop of collision.drop, transcribed on the reference's own fields for the plane z = 0 with given
    orientations and positions: (poses [B,4,4], rounds [B], settled [B])."""
    n = np.array([0.0, 0.0, 1.0])
    margin = 2.0 * max(b.grid.voxel for b in bodies) + 2.0 * tol
    poses = np.tile(np.eye(4), (len(bodies), 1, 1))
    rounds, settled, tops = [], [], []
    for k, body in enumerate(bodies):
        R = np.asarray(orientations[k], np.float64)
        v = body.vertices.astype(np.float64)
        h = max([0.0] + tops) + margin - float((v @ R.T @ n).min())
        poses[k, :3, :3] = R
        poses[k, :3, 3] = np.array([xy[k][0], xy[k][1], h])                  # the plane frame of n = +z is (x, y)
        max_travel = h + body.size + margin
        r, ok = 0, False
        while r < max_rounds:
            travels = [sweep_plane(body.vertices, poses[k], (0, 0, 1, 0), -n, tol, max_travel)[1].min()]
            for j in range(k):
                o = bodies[j]
                travels.append(sweep_body(o.field, o.grid, body.vertices, poses[k], poses[j], -n, tol, max_travel, max_steps)[1].min())
                travels.append(sweep_body(body.field, body.grid, o.vertices, poses[j], poses[k], n, tol, max_travel, max_steps)[1].min())
            travel = float(np.float32(min(travels)))
            r += 1
            if travel <= tol:
                ok = True
                break
            poses[k, :3, 3] -= travel * n
        rounds.append(r)
        settled.append(ok)
        tops.append(float((v @ poses[k, :3, :3].T + poses[k, :3, 3])[:, 2].max()))
    return poses, rounds, settled


def exact_clearances(meshes, poses):
    """[B, B+1]: the smallest exact signed distance from the vertices of mesh a (at its pose) to mesh b (at its pose), column B
    against the plane z = 0; the diagonal is +inf.  meshes: (vertices, faces) pairs."""
    B = len(meshes)
    out = np.full((B, B + 1), np.inf)
    for a in range(B):
        xa = np.asarray(meshes[a][0], np.float64) @ poses[a, :3, :3].T + poses[a, :3, 3]
        out[a, B] = xa[:, 2].min()
        for b in range(B):
            if a == b:
                continue
            local = (xa - poses[b, :3, 3]) @ poses[b, :3, :3]
            d, w = mesh_distance(local, meshes[b][0], meshes[b][1])
            out[a, b] = signed(d, w).min()
    return out
