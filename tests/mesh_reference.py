"""NumPy reference of the mesh kernels (pegasus_amd/csrc/mesh.hip.h): TSDF fusion with space carving and marching
tetrahedra.  Same rules, same float32 operations in the same order, same output order -- the GPU tests compare against it
exactly.  The tetrahedron case table is derived here on its own, from the geometry of the Kuhn split.  tsdf_oracle is
the second, independent reference of the fusion: float64, written from the header's contract, with the points where
float32 may decide otherwise marked."""
from __future__ import annotations

import itertools
from collections import Counter

import numpy as np

NEAR_Z = np.float32(0.2)                      # pgr_common.h, the renderer's near cull
# the 7 edges a grid point owns, in slot order: +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z (as corner codes: bit 0 = x)
EDGE_CODES = (1, 2, 4, 3, 5, 6, 7)
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def _code_xyz(code):
    return np.array([(code >> a) & 1 for a in range(3)], dtype=np.int64)


def _orient(P, i, j, k, l):
    return int(np.sign(round(np.linalg.det(np.stack([P[j] - P[i], P[k] - P[i], P[l] - P[i]]).astype(float)))))


def tet_table():
    """The 6 Kuhn tetrahedra of a cell and their 16-case triangle table.
    corner[t,q]: corner code of vertex q; owner[t,e] / slot[t,e]: the grid corner owning edge e and its slot;
    ntri[t,c]: triangles of sign pattern c (bit q = vertex q inside); tri[t,c,:3*ntri]: their vertices as edge ids."""
    corner = np.zeros((6, 4), np.int64)
    owner = np.zeros((6, 6), np.int64)
    slot = np.zeros((6, 6), np.int64)
    ntri = np.zeros((6, 16), np.int64)
    tri = np.zeros((6, 16, 6), np.int64)
    for t, (a, b, _c) in enumerate(itertools.permutations(range(3))):
        code = [0, 1 << a, (1 << a) | (1 << b), 7]
        corner[t] = code
        P = [_code_xyz(c) for c in code]
        for e, (u, w) in enumerate(TET_EDGES):
            owner[t, e] = code[u]
            slot[t, e] = EDGE_CODES.index(code[w] ^ code[u])

        def E(p, q):
            return TET_EDGES.index((min(p, q), max(p, q)))
        for c in range(16):
            ins = [q for q in range(4) if (c >> q) & 1]
            outs = [q for q in range(4) if not (c >> q) & 1]
            if len(ins) in (1, 3):
                x, o = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
                ccw = (_orient(P, x, *o) > 0) == (len(ins) == 1)
                tri[t, c, :3] = [E(x, o[0]), E(x, o[1] if ccw else o[2]), E(x, o[2] if ccw else o[1])]
                ntri[t, c] = 1
            elif len(ins) == 2:
                q = [E(ins[0], outs[0]), E(ins[0], outs[1]), E(ins[1], outs[1]), E(ins[1], outs[0])]
                if _orient(P, ins[0], ins[1], outs[0], outs[1]) < 0:
                    q = [q[0], q[3], q[2], q[1]]
                tri[t, c] = [q[0], q[1], q[2], q[0], q[2], q[3]]
                ntri[t, c] = 2
    return dict(corner=corner, owner=owner, slot=slot, ntri=ntri, tri=tri)


def _axes(grid):
    f32 = np.float32
    k, j, i = np.meshgrid(np.arange(grid.nz), np.arange(grid.ny), np.arange(grid.nx), indexing="ij")
    o = [f32(x) for x in grid.origin]
    vox = f32(grid.voxel)
    return i.ravel(), j.ravel(), k.ravel(), o, vox


def _coord(o, vox, idx):
    return np.float32(o) + np.float32(vox) * idx.astype(np.float32)


def tsdf_reference(grid, viewmats, tanfovx, tanfovy, depth, final_T, truncation, alpha_min, return_ambiguous=False):
    """sdf float32 [nz,ny,nx] of pgr_tsdf_integrate.  viewmats [V,16] float32 (world_view_transform, transposed storage);
    depth / final_T [V,H,W].  With return_ambiguous: also the points whose projection lies within 1e-4 px of a pixel
    boundary in some view (where the pixel a float32 rounding picks is not pinned by the rules)."""
    f32 = np.float32
    i, j, k, o, vox = _axes(grid)
    px, py, pz = _coord(o[0], vox, i), _coord(o[1], vox, j), _coord(o[2], vox, k)
    V, H, W = depth.shape
    trunc, amin = f32(truncation), f32(alpha_min)
    cx, cy = f32(W - 1) * f32(0.5), f32(H - 1) * f32(0.5)
    n = px.size
    s = np.zeros(n, f32)
    w = np.zeros(n, np.int64)
    carved = np.zeros(n, bool)
    ambiguous = np.zeros(n, bool)
    for v in range(V):
        m = np.asarray(viewmats[v], f32).reshape(16)
        x = m[0] * px + m[4] * py + m[8] * pz + m[12]
        y = m[1] * px + m[5] * py + m[9] * pz + m[13]
        z = m[2] * px + m[6] * py + m[10] * pz + m[14]
        front = z > NEAR_Z
        zs = np.where(front, z, f32(1))
        fx = f32(W / (2.0 * float(f32(tanfovx[v]))))
        fy = f32(H / (2.0 * float(f32(tanfovy[v]))))
        u = (x / zs) * fx + cx
        vv = (y / zs) * fy + cy
        hu, hv = u + f32(0.5), vv + f32(0.5)
        ambiguous |= front & ((np.abs(hu - np.round(hu)) < 1e-4) | (np.abs(hv - np.round(hv)) < 1e-4))
        fu, fv = np.floor(hu), np.floor(hv)
        ok = front & ~carved & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        iu = np.where(ok, fu, 0).astype(np.int64)
        iv = np.where(ok, fv, 0).astype(np.int64)
        T = final_T[v][iv, iu].astype(f32)
        D = depth[v][iv, iu].astype(f32)
        carve = ok & (f32(1) - T < amin)
        carved |= carve
        d = D - z
        use = ok & ~carve & ~(d < -trunc)
        s = np.where(use, s + np.fmin(d, trunc) / trunc, s).astype(f32)         # fminf: a NaN depth gives trunc
        w += use
    sdf = np.where(carved, f32(1), np.where(w == 0, f32(-1), s / np.maximum(w, 1).astype(f32))).astype(f32)
    border = (i == 0) | (j == 0) | (k == 0) | (i == grid.nx - 1) | (j == grid.ny - 1) | (k == grid.nz - 1)
    sdf[border] = f32(1)
    shape = (grid.nz, grid.ny, grid.nx)
    if return_ambiguous:
        return sdf.reshape(shape), (ambiguous & ~border).reshape(shape)
    return sdf.reshape(shape)


def _cell_cases(cin, T):
    """Sign pattern of each of the 6 tetrahedra ([C,6]) from the cells' corner inside-ness cin [C,8]."""
    case = np.zeros((cin.shape[0], 6), np.int64)
    for t_ in range(6):
        for q in range(4):
            case[:, t_] |= cin[:, T["corner"][t_, q]].astype(np.int64) << q
    return case


def _active_cells(inside):
    """Flat index of the (0,0,0) corner of every cell whose 8 corners do not all have one sign, ascending."""
    nz, ny, nx = inside.shape
    n_in = np.zeros((nz - 1, ny - 1, nx - 1), np.uint8)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        n_in += inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    kk, jj, ii = np.nonzero((n_in > 0) & (n_in < 8))
    return kk * (ny * nx) + jj * nx + ii


def _corner_offsets(nx, ny):
    return np.array([(c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny for c in range(8)])


def table_coverage(sdf, table=None):
    """The set of (tetrahedron, sign pattern) pairs with triangles (patterns 1..14) that occur in the cells of ``sdf``."""
    T = table or tet_table()
    inside = np.ascontiguousarray(sdf, np.float32) < 0
    nz, ny, nx = inside.shape
    cell = _active_cells(inside)
    case = _cell_cases(inside.ravel()[cell[:, None] + _corner_offsets(nx, ny)[None, :]], T)
    return {(t, int(c)) for t in range(6) for c in np.unique(case[:, t]) if 0 < c < 15}


_POPCOUNT7 = np.array([bin(m).count("1") for m in range(128)], np.int64)


def _march_sparse(sdf, grid, T):
    """march_reference on the active cells and the points that own a crossed edge only.  Measured on one
    CPU core: the 256^3 gyroid of the device test (1.53 M vertices, 3.05 M triangles) takes 2.8 s and stays below
    1.2 GB, the field included; the dense form's [cells,6,6] int64 arrays alone would take 4.8 GB each."""
    f32 = np.float32
    nz, ny, nx = sdf.shape
    inside = sdf < 0
    mask = np.zeros((nz, ny, nx), np.uint8)                                  # bit s: the point's edge in slot s is crossed
    for s, code in enumerate(EDGE_CODES):
        dx, dy, dz = (code & 1), (code >> 1) & 1, (code >> 2) & 1
        mask[:nz - dz, :ny - dy, :nx - dx] |= (inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]).astype(
            np.uint8) << np.uint8(s)
    mask = mask.ravel()
    owners = np.flatnonzero(mask)                                           # points that own a crossed edge
    own_mask = mask[owners]
    first = np.cumsum(_POPCOUNT7[own_mask]) - _POPCOUNT7[own_mask]            # index of each owner's first vertex
    row, s = np.nonzero((own_mask[:, None] >> np.arange(7, dtype=np.uint8)[None, :]) & 1)
    p = owners[row]
    verts = _edge_vertices(sdf, grid, p, s)
    cell = _active_cells(inside)
    off = _corner_offsets(nx, ny)
    case = _cell_cases(inside.ravel()[cell[:, None] + off[None, :]], T)
    tet = np.arange(6)[None, :]
    edges = T["tri"][tet, case]                                              # [C,6,6]
    owner = cell[:, None, None] + off[T["owner"][tet[..., None], edges]]
    slot = T["slot"][tet[..., None], edges]
    # an edge a triangle names is crossed, so its owner is in ``owners``; the padding of the table (edge 0 of an
    # untriangulated pattern) may name any point and is dropped by ``valid``
    at = np.minimum(np.searchsorted(owners, owner), max(len(owners) - 1, 0))
    ids = (first[at] + _POPCOUNT7[own_mask[at] & ((1 << slot) - 1).astype(np.uint8)]).reshape(cell.size, 6, 2, 3)
    valid = np.arange(2)[None, None, :] < T["ntri"][tet, case][..., None]    # [C,6,2]
    return verts, ids[valid].astype(np.int32).reshape(-1, 3)


def _edge_vertices(sdf, grid, p, s):
    """The vertices of the crossed edges (owner p, slot s): pa + t (pb - pa), t = fa / (fa - fb), in float32."""
    f32 = np.float32
    nz, ny, nx = sdf.shape
    i, j, k, o, vox = (p % nx), (p // nx) % ny, p // (nx * ny), [f32(x) for x in grid.origin], f32(grid.voxel)
    codes = np.asarray(EDGE_CODES)[s]
    dx, dy, dz = codes & 1, (codes >> 1) & 1, (codes >> 2) & 1
    flat = sdf.ravel()
    fa = flat[p]
    fb = flat[p + dx + dy * nx + dz * nx * ny]
    t = fa / (fa - fb)
    verts = np.empty((p.size, 3), f32)
    for ax, (a0, d) in enumerate(((i, dx), (j, dy), (k, dz))):
        pa = _coord(o[ax], vox, a0)
        pb = _coord(o[ax], vox, a0 + d)
        verts[:, ax] = pa + t * (pb - pa)
    return verts


# ---- the float64 oracle of pgr_tsdf_integrate -----------------------------------------------------------------------
# Written from the contract in include/pegasus_raster.h, not from the kernel: float64 throughout, the view transform as one
# 4x4 product on homogeneous row vectors (the storage is the transposed matrix), pixel centres at integer coordinates.
# The device decides in float32, so next to every decision stands a bound on the float32 error of the quantity it tests;
# a point with a decision inside its bound, in a view it reaches, is masked.  The bounds are first-order rounding
# analysis with u = 2^-24 and gamma(n) = n u / (1 - n u) for n roundings in a row:
#   p_a = o_a + voxel * i        two roundings, each at most u * pmax_a, pmax_a = |o_a| + voxel (n_a - 1)
#   x = c0 px + c1 py + c2 pz + c3   with B = sum |c_r| pmax_r + |c3| (the largest intermediate is at most B): the inputs
#                                carry 2 u B, the three products u B, the three additions 3 u B      -> E_lin = gamma(6) B
#   q = x / z                    (E_x + |q| E_z) / (z - E_z) from the operands, u |q| from the division  -> E_q
#   t = q * fx                   fx itself is rounded to float32 and so is the product               -> fx E_q + gamma(2) |t|
#   u = t + cx, h = u + 0.5      cx = (W-1)/2 and 0.5 are exact; each addition rounds its result     -> + u |u| + u |h|
#   a = 1 - final_T              one rounding                                                        -> u |a|
#   d = depth - z                the error of z and one rounding                                     -> E_z + u |d|
# Outside the mask every view agrees on what it does, so the sdf differs only through the values: a term
# min(d, trunc) / trunc is exactly 1 where d >= trunc beyond its bound and otherwise off by E_d / trunc + u (the
# division); adding w terms of magnitude <= 1 one after the other loses at most gamma(w - 1) * w, and the last division
# u.  tol = (sum of the term errors) / w + gamma(w): what the device may differ from the float64 value by.
_U = 2.0 ** -24


def _gamma(n):
    return n * _U / (1.0 - n * _U)


CENSUS_KEYS = ("near", "left", "right", "top", "bottom", "carved", "behind", "fused")


def tsdf_oracle(grid, viewmats, tanfovx, tanfovy, depth, final_T, truncation, alpha_min):
    """(sdf float64, masked bool, tol float64, census) of pgr_tsdf_integrate, each array [nz,ny,nx].  ``masked``: an
    interior point where some view it reaches decides within float32 rounding of a threshold.  ``census``: the share
    of (interior point, view) pairs that end in each of CENSUS_KEYS (a point outside two sides counts for both; the
    views after a carving one are not reached), and "in_image_per_view": how many points each view holds in its
    image."""
    f64 = np.float64
    o = [float(np.float32(x)) for x in grid.origin]
    vox = float(np.float32(grid.voxel))
    dims = (grid.nx, grid.ny, grid.nz)
    k, j, i = np.meshgrid(np.arange(grid.nz), np.arange(grid.ny), np.arange(grid.nx), indexing="ij")
    idx = [a.ravel() for a in (i, j, k)]
    P = np.stack([o[a] + vox * idx[a].astype(f64) for a in range(3)] + [np.ones(idx[0].size)], axis=1)     # [n,4]
    pmax = np.array([abs(o[a]) + vox * (dims[a] - 1) for a in range(3)])
    border = np.zeros(idx[0].size, bool)
    for a in range(3):
        border |= (idx[a] == 0) | (idx[a] == dims[a] - 1)
    V, H, W = depth.shape
    trunc, amin = float(np.float32(truncation)), float(np.float32(alpha_min))
    near = 0.2
    near_repr = abs(float(NEAR_Z) - near)                                   # the device holds 0.2 as a float32
    n = P.shape[0]
    s, err, w = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    done = border.copy()                                                    # carved, or not walked at all
    carved = np.zeros(n, bool)
    masked = np.zeros(n, bool)
    census = dict.fromkeys(CENSUS_KEYS, 0)
    in_image_per_view = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for v in range(V):
            M = np.asarray(viewmats[v], np.float32).astype(f64).reshape(4, 4)
            Pv = P @ M
            x, y, z = Pv[:, 0], Pv[:, 1], Pv[:, 2]
            Ex, Ey, Ez = (_gamma(6) * (np.abs(M[:3, c]) @ pmax + abs(M[3, c])) for c in range(3))
            live = ~done
            m_near = np.abs(z - near) <= Ez + near_repr
            front = z > near
            zs = np.where(front, z, 1.0)
            pix, m_pix, outside = [], np.zeros(n, bool), []
            for coord, Ec, size, tanfov in ((x, Ex, W, tanfovx[v]), (y, Ey, H, tanfovy[v])):
                f = size / (2.0 * float(np.float32(tanfov)))
                q = coord / zs
                Eq = (Ec + np.abs(q) * Ez) / (zs - Ez) + _U * np.abs(q)
                t = q * f
                Et = f * Eq + _gamma(2) * np.abs(t)
                u = t + (size - 1) / 2.0
                h = u + 0.5
                Eh = Et + _U * (np.abs(u) + Et) + _U * (np.abs(h) + Et)
                b = np.rint(h)
                # the boundaries 0 .. size separate pixels, or the image from the outside; the others separate nothing
                m_pix |= (np.abs(h - b) <= Eh) & (b >= 0) & (b <= size)
                c = np.floor(h)
                pix.append(c)
                outside.append((c < 0, c >= size))
            in_img = front & ~outside[0][0] & ~outside[0][1] & ~outside[1][0] & ~outside[1][1]
            col = np.where(in_img, pix[0], 0).astype(np.int64)
            row = np.where(in_img, pix[1], 0).astype(np.int64)
            T = np.asarray(final_T[v], np.float32).astype(f64)[row, col]
            D = np.asarray(depth[v], np.float32).astype(f64)[row, col]
            a = 1.0 - T
            carve = in_img & (a < amin)
            m_alpha = in_img & (np.abs(a - amin) <= _U * np.abs(a))
            d = D - z
            Ed = Ez + _U * np.abs(d)
            behind = in_img & ~carve & (d < -trunc)
            m_behind = in_img & ~carve & np.isfinite(d) & (np.abs(d + trunc) <= Ed)      # inf and NaN are far from it
            use = in_img & ~carve & ~behind
            masked |= live & (m_near | (front & (m_pix | m_alpha | m_behind)))
            term = np.fmin(d, trunc) / trunc                                # min(NaN, trunc) = trunc, as fminf
            term_err = np.where(d < trunc + Ed, Ed / trunc + _U, 0.0)       # false for inf and NaN: exactly 1
            add = live & use
            s = np.where(add, s + term, s)
            err = np.where(add, err + term_err, err)
            w += add
            for key, sel in (("near", ~front), ("left", front & outside[0][0]), ("right", front & outside[0][1]),
                             ("top", front & outside[1][0]), ("bottom", front & outside[1][1]), ("carved", carve),
                             ("behind", behind), ("fused", use)):
                census[key] += int((live & sel).sum())
            in_image_per_view.append(int((~border & in_img).sum()))
            carved |= live & carve
            done |= carved
    n_int = int((~border).sum())
    census = {key: c / max(n_int * V, 1) for key, c in census.items()}
    census["in_image_per_view"] = in_image_per_view
    wf = np.maximum(w, 1).astype(f64)
    sdf = np.where(border | carved, 1.0, np.where(w == 0, -1.0, s / wf))
    tol = np.where(border | carved | (w == 0), 0.0, err / wf + _gamma(1) * wf)
    shape = (grid.nz, grid.ny, grid.nx)
    return sdf.reshape(shape), (masked & ~border).reshape(shape), tol.reshape(shape), census


def interior(grid):
    """The points pgr_tsdf_integrate walks the views for: everything but the outermost layer."""
    m = np.zeros((grid.nz, grid.ny, grid.nx), bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m


def march_reference(sdf, grid, table=None, sparse=False):
    """(vertices float32 [V,3], faces int32 [F,3]) of pgr_march_count / pgr_march_emit, in the same order.  The dense
    form builds [points,7] and [cells,6,6] arrays and is the plain statement of the rules; ``sparse`` gives the same
    bytes from the active cells alone and is the one that fits a 256^3 grid."""
    f32 = np.float32
    T = table or tet_table()
    sdf = np.ascontiguousarray(sdf, f32)
    if sparse:
        return _march_sparse(sdf, grid, T)
    nz, ny, nx = sdf.shape
    inside = sdf < 0
    crossed = np.zeros((nz, ny, nx, 7), bool)
    for s, code in enumerate(EDGE_CODES):
        dx, dy, dz = (code & 1), (code >> 1) & 1, (code >> 2) & 1
        crossed[:nz - dz, :ny - dy, :nx - dx, s] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
    crossed = crossed.reshape(-1, 7)
    vid = np.full(crossed.shape, -1, np.int64)
    vid[crossed] = np.arange(int(crossed.sum()))
    # vertices, (point, slot) order
    p, s = np.nonzero(crossed)
    i, j, k, o, vox = (p % nx), (p // nx) % ny, p // (nx * ny), [f32(x) for x in grid.origin], f32(grid.voxel)
    codes = np.asarray(EDGE_CODES)[s]
    dx, dy, dz = codes & 1, (codes >> 1) & 1, (codes >> 2) & 1
    flat = sdf.ravel()
    fa = flat[p]
    fb = flat[p + dx + dy * nx + dz * nx * ny]
    t = fa / (fa - fb)
    verts = np.empty((p.size, 3), f32)
    for ax, (a0, d) in enumerate(((i, dx), (j, dy), (k, dz))):
        pa = _coord(o[ax], vox, a0)
        pb = _coord(o[ax], vox, a0 + d)
        verts[:, ax] = pa + t * (pb - pa)
    # faces, (cell, tetrahedron, triangle) order; a cell is named by its (0,0,0) corner
    kk, jj, ii = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    cell = (kk * ny * nx + jj * nx + ii).ravel()
    off = np.array([(c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny for c in range(8)])
    cin = inside.ravel()[cell[:, None] + off[None, :]]                                   # [C,8]
    case = np.zeros((cell.size, 6), np.int64)
    for t_ in range(6):
        for q in range(4):
            case[:, t_] |= cin[:, T["corner"][t_, q]].astype(np.int64) << q
    tet = np.arange(6)[None, :]
    edges = T["tri"][tet, case]                                                          # [C,6,6]
    owner = cell[:, None, None] + off[T["owner"][tet[..., None], edges]]
    ids = vid[owner, T["slot"][tet[..., None], edges]].reshape(cell.size, 6, 2, 3)
    valid = np.arange(2)[None, None, :] < T["ntri"][tet, case][..., None]                # [C,6,2]
    faces = ids[valid].astype(np.int32)
    return verts, faces.reshape(-1, 3)


# ---- properties of a mesh -----------------------------------------------------------------------------------------
def assert_watertight(faces):
    directed = Counter(map(tuple, np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).tolist()))
    assert all(n == 1 for n in directed.values()), "a directed edge appears twice"
    assert all((b, a) in directed for (a, b) in directed), "an edge without its reverse"
    return len(directed) // 2


def components(n_vertices, faces):
    parent = list(range(n_vertices))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b, c in faces.tolist():
        parent[find(a)] = find(b)
        parent[find(b)] = find(c)
    return len({find(v) for v in np.unique(faces)})
