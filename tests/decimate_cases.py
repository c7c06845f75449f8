"""The meshes of the vertex-clustering tests (tests/test_decimate_host.py, tests/test_decimate_gpu.py).  Every builder
returns (vertices float32 [V,3], faces int32 [F,3], voxel); coordinates meant to be exact are dyadic."""
import numpy as np

TILE = 2048                  # pegasus_amd/csrc/decimate.hip.h DEC_TILE: items per workgroup of the sorts and scans
PACKED_LIMIT = 1 << 21       # from this many vertices on the face sort runs in two stages


def _mesh(v, f):
    return np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)


# ---- hand-worked ------------------------------------------------------------------------------------------------------
def two_triangles_one_cell():
    """Two triangles sharing an edge, all four vertices in one cell: K = 1, no face."""
    return (*_mesh([(0, 0, 0), (0.125, 0, 0), (0, 0.125, 0), (0.125, 0.125, 0)], [(0, 1, 3), (0, 3, 2)]), 1.0)


def unit_square():
    """A unit square over 2 x 2 cells (lo = -0.5): clusters 0..3 are the vertices in (cy, cx) order; the faces are given
    rotated, (3,0,1) and (2,0,3), and come out as (0,1,3), (0,3,2)."""
    return (*_mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)], [(3, 0, 1), (2, 0, 3)]), 1.0)


def half_voxel_split():
    """A square of side 0.625 at voxel 1: with lo = min - voxel / 2 its corners fall into four cells, with lo = min into one."""
    return (*_mesh([(0, 0, 0), (0.625, 0, 0), (0, 0.625, 0), (0.625, 0.625, 0)], [(0, 1, 3), (0, 3, 2)]), 1.0)


def _three_pairs():
    # clusters 0, 1, 2 (cells x = 0, 1, 2) with two vertices each: 0/3, 1/4, 2/5
    return [(0, 0, 0), (1, 0, 0), (2, 0.25, 0), (0.125, 0.125, 0), (1.125, 0.125, 0), (2.125, 0.125, 0.125)]


def duplicate_pair():
    """Two different faces over the same three clusters, same orientation: one face (0,1,2) remains."""
    return (*_mesh(_three_pairs(), [(0, 1, 2), (4, 5, 3)]), 1.0)


def opposite_pair():
    """The same, opposite orientations: (0,1,2) and (0,2,1) both stay, in that order."""
    return (*_mesh(_three_pairs(), [(0, 1, 2), (3, 5, 4)]), 1.0)


def flat_cluster():
    """A planar 5 x 5 grid at z = 0.25 inside one cell of a 2 x 2 arrangement: every quadric has rank 1, so every cluster takes
    the average."""
    n = 9
    g = np.arange(n) / 8.0
    v = np.stack([np.tile(g, n), np.repeat(g, n), np.full(n * n, 0.25)], axis=1)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            f += [(a, a + 1, a + n + 1), (a, a + n + 1, a + n)]
    return (*_mesh(v, f), 0.75)


ANCHOR = (0.0, 0.0, 0.0)     # an unreferenced vertex that pins lo to (-0.5, -0.5, -0.5) at voxel 1
CORNER_CELL = (1, 1, 1)      # the cell [0.5, 1.5)^3 whose cluster the two cases below are about


def _three_planes(apex, in_cell, others, extra=()):
    """Three triangles in the orthogonal planes z = const, x + y = const, x - y = const through ``apex``; triangle k has
    in_cell[k] (inside CORNER_CELL) and others[k] (two vertices in cells of their own).  Vertex 0 is the anchor, vertices 1..3
    are in_cell: the cluster of CORNER_CELL holds exactly those (plus ``extra`` vertices), and its quadric's minimiser is the
    apex, which is no vertex."""
    v = [ANCHOR] + list(in_cell)
    f = []
    for k in range(3):
        v += list(others[k])
        f.append((1 + k, 4 + 2 * k, 5 + 2 * k))
    first_extra = len(v)
    v += list(extra)
    return v, f, first_extra


def corner_inside():
    """The apex (1.125, 1, 1) lies inside CORNER_CELL (corner 0.5): the quadric position is the apex, x = (0.625, 0.5, 0.5)."""
    v, f, _ = _three_planes((1.125, 1.0, 1.0),
                            [(0.625, 1.0, 1.0), (0.875, 1.25, 1.25), (0.875, 0.75, 0.875)],
                            [((1.25, 2.75, 1.0), (2.875, 2.75, 1.0)), ((0.125, 2.0, 2.75), (0.125, 2.0, 0.125)),
                             ((2.875, 2.75, 2.625), (2.875, 2.75, 0.25))])
    return (*_mesh(v, f), 1.0)


CORNER_INSIDE_APEX = (1.125, 1.0, 1.0)


def corner_in_neighbour():
    """The same three planes through (1.625, 1, 1), which lies in the NEXT cell along x: the minimiser fails the box test and
    the cluster takes the average of its three vertices."""
    v, f, _ = _three_planes((1.625, 1.0, 1.0),
                            [(0.625, 1.0, 1.0), (1.25, 1.375, 1.25), (1.375, 0.75, 0.875)],
                            [((1.25, 2.75, 1.0), (2.875, 2.75, 1.0)), ((0.125, 2.5, 2.75), (0.125, 2.5, 0.125)),
                             ((2.875, 2.25, 2.625), (2.875, 2.25, 0.25))])
    return (*_mesh(v, f), 1.0)


def two_corner_face():
    """corner_inside plus a fourth triangle in the plane z = 1.25 with TWO corners in CORNER_CELL: counted twice it pulls the
    minimiser's z further from 1 than counted once."""
    v, f, e = _three_planes((1.125, 1.0, 1.0),
                            [(0.625, 1.0, 1.0), (0.875, 1.25, 1.25), (0.875, 0.75, 0.875)],
                            [((1.25, 2.75, 1.0), (2.875, 2.75, 1.0)), ((0.125, 2.0, 2.75), (0.125, 2.0, 0.125)),
                             ((2.875, 2.75, 2.625), (2.875, 2.75, 0.25))],
                            extra=[(0.75, 0.625, 1.25), (1.0, 0.625, 1.25), (1.25, 2.75, 1.25)])
    f.append((e, e + 1, e + 2))
    return (*_mesh(v, f), 1.0)


HAND_CASES = {"two_triangles_one_cell": two_triangles_one_cell, "unit_square": unit_square, "half_voxel_split": half_voxel_split,
              "duplicate_pair": duplicate_pair, "opposite_pair": opposite_pair, "flat_cluster": flat_cluster,
              "corner_inside": corner_inside, "corner_in_neighbour": corner_in_neighbour, "two_corner_face": two_corner_face}


# ---- shapes -------------------------------------------------------------------------------------------------------------
def random_mesh(n_vertices, n_faces, seed, voxel=0.25):
    """Uniform vertices in the unit cube and uniform index triples (some with a repeated index): nothing a mesh would be, and
    every path of the kernels."""
    rng = np.random.default_rng(seed)
    v = rng.random((n_vertices, 3), dtype=np.float32)
    f = rng.integers(0, n_vertices, (n_faces, 3), dtype=np.int32)
    return v, f, voxel


def dense_cell():
    """1400 of 1500 vertices in one cell, 700 faces: that cluster sums far more than 1024 corner terms and 1024 vertices."""
    rng = np.random.default_rng(11)
    v = np.concatenate([0.2 * rng.random((1400, 3), dtype=np.float32), rng.random((100, 3), dtype=np.float32)])
    f = rng.integers(0, 1500, (700, 3), dtype=np.int32)
    return v, f, 0.5


def own_cells():
    """A 7^3 lattice of spacing 1 at voxel 0.5: every vertex in a cell of its own, K = V."""
    g = np.arange(7, dtype=np.float32)
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    f = np.random.default_rng(5).integers(0, len(v), (600, 3), dtype=np.int32)
    return v, f, 0.5


def dyadic_walls():
    """Vertices on the lattice k / 8 at voxel 1 / 4: with lo = min - 1/8 every other lattice plane IS a cell wall."""
    g = np.arange(9, dtype=np.float32) / 8.0
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    f = np.random.default_rng(6).integers(0, len(v), (900, 3), dtype=np.int32)
    return v, f, 0.25


def degenerate_faces():
    """A random mesh whose faces use only the first half of the vertices (the rest are unreferenced), plus faces with a
    repeated index, faces over coincident vertices and collinear (zero-area) faces."""
    v, f, voxel = random_mesh(400, 500, 21)
    f = f % 200
    v[210] = v[10]                                         # coincident with vertex 10, itself unreferenced by the random faces
    v[0], v[1], v[2] = (0.125, 0.125, 0.125), (0.375, 0.375, 0.375), (0.75, 0.75, 0.75)      # collinear, three cells
    extra = np.asarray([(5, 5, 9), (1, 2, 1), (7, 7, 7), (10, 210, 33), (0, 1, 2), (2, 1, 0)], np.int32)
    return v, np.concatenate([f, extra]), voxel


def thin_slab():
    """Three 9 x 9 sheets 1/64 apart at voxel 1/4, the middle one wound the other way: the sheets share cells, so the result
    holds duplicates (removed) and opposite faces (kept)."""
    n = 9
    g = np.arange(n) / 8.0
    v, f = [], []
    for s in range(3):
        base = s * n * n
        v.append(np.stack([np.tile(g, n), np.repeat(g, n), np.full(n * n, s / 64.0)], axis=1))
        for j in range(n - 1):
            for i in range(n - 1):
                a = base + j * n + i
                quad = [(a, a + 1, a + n + 1), (a, a + n + 1, a + n)]
                f += [(t[0], t[2], t[1]) for t in quad] if s == 1 else quad
    return (*_mesh(np.concatenate(v), f), 0.25)


def big_lattice():
    """129 x 128 x 128 = 2 113 536 vertices (just above 2^21) of spacing 1 at voxel 0.5, each in a cell of its own, and 1000
    faces: the face sort's two-stage path."""
    gx, gy, gz = np.arange(129, dtype=np.float32), np.arange(128, dtype=np.float32), np.arange(128, dtype=np.float32)
    v = np.stack(np.meshgrid(gz, gy, gx, indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1].copy()
    f = np.random.default_rng(7).integers(0, len(v), (1000, 3), dtype=np.int32)
    f[:8] = f[8:16][:, [1, 2, 0]]                          # rotated copies: duplicates
    f[16:24] = f[24:32][:, [0, 2, 1]]                      # flipped copies: opposites
    return v, f, 0.5


def wide_extent():
    """60 vertices spread over [0, 1] along x at a voxel with (max - min) / voxel + 1 = 2^20 - 1.25: the largest cell index is
    2^20 - 2."""
    rng = np.random.default_rng(9)
    v = rng.random((60, 3), dtype=np.float32)
    v[:, 1:] *= 1e-3
    v[0, 0], v[1, 0] = 0.0, 1.0
    f = rng.integers(0, 60, (90, 3), dtype=np.int32)
    return v, f, 1.0 / (2.0 ** 20 - 2.25)


SHAPE_CASES = {
    "v1_f1": lambda: random_mesh(1, 1, 1),
    "v255_f255": lambda: random_mesh(255, 255, 2),
    "v256_f256": lambda: random_mesh(256, 256, 3),
    "v257_f257": lambda: random_mesh(257, 257, 4),
    "beyond_a_tile": lambda: random_mesh(TILE + 1, TILE + 1, 5),
    "no_faces": lambda: random_mesh(300, 0, 6),
    "one_cluster": lambda: random_mesh(300, 500, 7, voxel=4.0),
    "own_cells": own_cells,
    "dense_cell": dense_cell,
    "degenerate_faces": degenerate_faces,
    "thin_slab": thin_slab,
    "wide_extent": wide_extent,
}
AVERAGE_ONLY = {"dyadic_walls": dyadic_walls}      # lattice-aligned: minimisers sit exactly on cell walls


# ---- the surfaces of the quadric comparison ------------------------------------------------------------------------------
def icosphere():
    from mesh_raster_cases import icosphere as ico
    return ico(5, 0.1)


def gyroid_mesh():
    from mesh_cases import gyroid
    from mesh_reference import march_reference
    from pegasus_amd.mesh import Grid
    grid = Grid(48, 48, 48, (-1.0, -1.0, -1.0), 2.0 / 47.0)
    v, f = march_reference(gyroid(grid), grid)[:2]
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def voxel_for(vertices, cells_across):
    """The voxel at which the longest axis of the bounding box spans ``cells_across`` cells."""
    ext = vertices.astype(np.float64)
    return float((ext.max(axis=0) - ext.min(axis=0)).max()) / cells_across
