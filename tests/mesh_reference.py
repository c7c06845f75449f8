"""NumPy reference of the mesh kernels (pegasus_amd/csrc/mesh.hip.h): TSDF fusion with space carving and marching
tetrahedra.  Same rules, same float32 operations in the same order, same output order -- the GPU tests compare against it
exactly.  The tetrahedron case table is derived here on its own, from the geometry of the Kuhn split."""
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
        s = np.where(use, s + np.minimum(d, trunc) / trunc, s).astype(f32)
        w += use
    sdf = np.where(carved, f32(1), np.where(w == 0, f32(-1), s / np.maximum(w, 1).astype(f32))).astype(f32)
    border = (i == 0) | (j == 0) | (k == 0) | (i == grid.nx - 1) | (j == grid.ny - 1) | (k == grid.nz - 1)
    sdf[border] = f32(1)
    shape = (grid.nz, grid.ny, grid.nx)
    if return_ambiguous:
        return sdf.reshape(shape), (ambiguous & ~border).reshape(shape)
    return sdf.reshape(shape)


def march_reference(sdf, grid, table=None):
    """(vertices float32 [V,3], faces int32 [F,3]) of pgr_march_count / pgr_march_emit, in the same order."""
    f32 = np.float32
    T = table or tet_table()
    sdf = np.ascontiguousarray(sdf, f32)
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
