"""Procedural meshes and scenes for the collision tests: no fixture files.  Every reference (tests/collision_reference.py, float64)
is computed once per process and shared, unchanged, by the tests that need it."""
import functools

import numpy as np

import collision_reference as CR

FACE_TILE = 256                      # PGR_SDF_FACE_TILE: tests/test_collision_abi.py holds it against the header
WINDING_MARGIN = 0.05                # the sign is compared where |winding - 0.5| >= this ...
SURFACE_MARGIN = 1e-5                # ... and the distance is above this fraction of the mesh diagonal
MAX_EXEMPT = 0.01                    # at most this share of a case's points may be exempt


# ---- meshes -----------------------------------------------------------------------------------------------------------------
def cube(side=1.0, center=(0.0, 0.0, 0.0)):
    """12 outward-wound faces."""
    h = 0.5 * side
    v = np.array([[x, y, z] for z in (-h, h) for y in (-h, h) for x in (-h, h)], np.float64) + np.asarray(center, np.float64)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]], np.int32)
    return v.astype(np.float32), f


def icosphere(subdivisions=2, radius=0.5, center=(0.0, 0.0, 0.0)):
    """20 * 4^subdivisions outward-wound faces: 320 at 2."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return (np.asarray(v) * radius + np.asarray(center, np.float64)).astype(np.float32), np.asarray(f, np.int32)


def l_prism(scale=0.5, height=0.6):
    """A concave L (three unit squares) extruded along z: 28 outward-wound faces, closed."""
    loop = [(0, 0), (1, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2), (0, 1)]                  # counter-clockwise
    xy = np.asarray(loop, np.float64) * scale - 0.75 * scale
    n = len(loop)
    v = np.concatenate([np.c_[xy, np.full(n, -0.5 * height)], np.c_[xy, np.full(n, 0.5 * height)]])
    squares = [(0, 1, 4, 7), (1, 2, 3, 4), (7, 4, 5, 6)]                                      # counter-clockwise from +z
    f = []
    for a, b, c, d in squares:
        f += [(a + n, b + n, c + n), (a + n, c + n, d + n), (a, c, b), (a, d, c)]
    for i in range(n):
        j = (i + 1) % n
        f += [(i, j, j + n), (i, j + n, i + n)]
    return v.astype(np.float32), np.asarray(f, np.int32)


def open_cube():
    """The cube without its +z face."""
    v, f = cube()
    return v, np.ascontiguousarray(f[[0, 1, 4, 5, 6, 7, 8, 9, 10, 11]])


def degenerate_cube():
    """The cube with a duplicated vertex and two faces without area: one through the duplicate (two equal corners), one along
    an edge (three collinear corners).  The surface and the winding numbers are the cube's."""
    v, f = cube()
    v = np.concatenate([v, v[:1], 0.5 * (v[0:1] + v[1:2])])
    return v, np.concatenate([f, np.array([[0, 8, 1], [0, 9, 1]], np.int32)])


def padded(v, f, n_faces, seed=0):
    """``f`` cut or padded to ``n_faces`` faces: the padding is small triangles far away (they change no minimum, and their solid
    angles are part of the reference like any face's)."""
    if n_faces <= len(f):
        return v, np.ascontiguousarray(f[:n_faces])
    rng = np.random.default_rng(seed)
    k = n_faces - len(f)
    base = rng.uniform(-1.0, 1.0, (k, 3)) + np.array([40.0, -30.0, 25.0])
    legs = np.eye(3)[[[0, 1], [1, 2], [2, 0], [1, 0], [2, 1], [0, 2]]][np.arange(k) % 6] * 0.05       # right angles, both windings
    tri = base[:, None, :] + np.concatenate([np.zeros((k, 1, 3)), legs], axis=1)
    extra = (len(v) + np.arange(3 * k).reshape(k, 3)).astype(np.int32)
    return np.concatenate([v, tri.reshape(-1, 3).astype(np.float32)]), np.concatenate([f, extra])


def translated(v, f, offset):
    return (v.astype(np.float64) + np.asarray(offset, np.float64)).astype(np.float32), f


OFFSET = (1000.0, -2000.0, 500.0)


def box_grid(shape, half=0.8, center=(0.0, 0.0, 0.0), shift=(0.013, -0.007, 0.021)):
    """A grid of ``shape`` = (nx, ny, nz) points over the cube of half-edge ``half``, pushed off every symmetry plane."""
    voxel = 2.0 * half / (max(shape) - 1)
    origin = np.asarray(center, np.float64) + np.asarray(shift) - 0.5 * voxel * (np.asarray(shape) - 1)
    return CR.RefGrid(shape[0], shape[1], shape[2], origin, voxel)


# name -> (mesh, grid, compare the sign); the closed ones at 24^3 must have no exempt point at all
SDF_CASES = {
    "cube_5x7x9": (cube, lambda: box_grid((5, 7, 9)), True),
    "cube_2x2x2": (cube, lambda: box_grid((2, 2, 2), half=0.3), True),
    "cube_24": (cube, lambda: box_grid((24, 24, 24)), True),
    "icosphere_24": (icosphere, lambda: box_grid((24, 24, 24)), True),
    "l_prism_33x17x3": (l_prism, lambda: box_grid((33, 17, 3)), True),
    "l_prism_24": (l_prism, lambda: box_grid((24, 24, 24)), True),
    "open_cube_5x7x9": (open_cube, lambda: box_grid((5, 7, 9)), True),
    "degenerate_5x7x9": (degenerate_cube, lambda: box_grid((5, 7, 9)), True),
    "faces_0": (lambda: padded(*cube(), 0), lambda: box_grid((5, 7, 9)), True),
    "faces_1": (lambda: padded(*cube(), 1), lambda: box_grid((5, 7, 9)), True),
    "faces_255": (lambda: padded(*cube(), FACE_TILE - 1), lambda: box_grid((5, 7, 9)), True),
    "faces_256": (lambda: padded(*cube(), FACE_TILE), lambda: box_grid((5, 7, 9)), True),
    "faces_257": (lambda: padded(*cube(), FACE_TILE + 1), lambda: box_grid((5, 7, 9)), True),
    "off_centre": (lambda: translated(*icosphere(), OFFSET), lambda: box_grid((5, 7, 9), center=OFFSET), True),
    # grid points exactly on the cube's vertices, edges and faces: magnitude only, by construction
    "on_surface": (cube, lambda: CR.RefGrid(5, 5, 5, (-1.0, -1.0, -1.0), 0.5), False),
}
CLOSED_24 = ("cube_24", "icosphere_24", "l_prism_24")


@functools.lru_cache(maxsize=None)
def sdf_case(name):
    """(vertices, faces, grid, reference): reference holds d, w [nz,ny,nx], the bound on d, the mask of the points whose sign
    is compared, and the mesh's shape numbers."""
    make_mesh, make_grid, with_sign = SDF_CASES[name]
    v, f = make_mesh()
    g = make_grid()
    d, w = CR.mesh_distance(CR.grid_points(g).reshape(-1, 3), v, f)
    L, kappa, diag = CR.mesh_shape(v, f)
    sure = (np.abs(w - 0.5) >= WINDING_MARGIN) & (d > SURFACE_MARGIN * diag) if with_sign else np.zeros(len(d), bool)
    ref = dict(d=d.reshape(g.shape), w=w.reshape(g.shape), bound=CR.distance_bound(d, L, kappa).reshape(g.shape),
               sure=sure.reshape(g.shape), with_sign=with_sign, L=L, kappa=kappa, diag=diag)
    for a in (v, f, *[x for x in ref.values() if isinstance(x, np.ndarray)]):
        a.setflags(write=False)
    return v, f, g, ref


# ---- samples ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sample_case():
    """(field [nz,ny,nx] float32, grid, points float32 [N,3]): the exact field of the icosphere on a 9x8x7 grid, points inside
    the grid away from cell borders, then points beyond each of the six sides and beyond a corner."""
    v, f = icosphere()
    g = box_grid((9, 8, 7), half=0.7)
    d, w = CR.mesh_distance(CR.grid_points(g).reshape(-1, 3), v, f)
    field = CR.signed(d, w).reshape(g.shape).astype(np.float32)
    rng = np.random.default_rng(5)
    n = 301
    cell = np.stack([rng.integers(0, k - 1, n) for k in (g.nx, g.ny, g.nz)], axis=1)
    inside = g.origin + g.voxel * (cell + rng.uniform(0.1, 0.9, (n, 3)))
    lo, hi = g.origin, g.origin + g.voxel * (g.n - 1)
    mid = 0.5 * (lo + hi) + 0.23 * g.voxel
    outside = []
    for axis in range(3):
        for side, sign in ((lo, -1.0), (hi, 1.0)):
            q = mid.copy()
            q[axis] = side[axis] + sign * 0.37
            outside.append(q)
    outside.append(hi + np.array([0.2, 0.3, 0.4]))
    outside.append(lo - np.array([0.4, 0.0, 0.0]) + np.array([0.0, 0.31, 0.27]) * g.voxel)
    points = np.concatenate([inside, np.asarray(outside)]).astype(np.float32)
    for a in (field, points):
        a.setflags(write=False)
    return field, g, points, n


# ---- drop scenes ----------------------------------------------------------------------------------------------------------------
DROP_RESOLUTION = 24
DROP_TOL = 1e-4
SPHERE_OFFSETS = ((0.0, 0.0), (0.3, 0.1), (0.7, 0.0), (0.95, 0.0), (0.99, 0.3), (1.2, 0.0))


def drop_scene(name):
    """(meshes, orientations, xy): bodies in the order they are placed."""
    if name.startswith("sphere_"):
        off = SPHERE_OFFSETS[int(name.split("_")[1])]
        return [cube(), icosphere()], [np.eye(3)] * 2, [(0.0, 0.0), off]
    if name == "three_in_a_row":
        return [cube(), icosphere(), cube(0.6)], [np.eye(3)] * 3, [(0.05, -0.02)] * 3
    raise KeyError(name)


DROP_SCENES = tuple(f"sphere_{i}" for i in range(len(SPHERE_OFFSETS))) + ("three_in_a_row",)


@functools.lru_cache(maxsize=None)
def ref_body(kind, arg=None):
    v, f = {"cube": cube, "icosphere": icosphere}[kind](*(() if arg is None else (arg,)))
    return CR.RefBody(v, f, DROP_RESOLUTION)


def drop_ref_bodies(name):
    if name.startswith("sphere_"):
        return [ref_body("cube"), ref_body("icosphere")]
    return [ref_body("cube"), ref_body("icosphere"), ref_body("cube", 0.6)]


def drop_slack(voxels):
    """E = (sqrt(3) / 2) (largest voxel): how far a trilinear sample of a 1-Lipschitz field can be from the field."""
    return 0.5 * 3.0 ** 0.5 * max(voxels)


def assert_placement(meshes, poses, orientations, xy, settled, E, tol=DROP_TOL):
    """Checks 1-3 of a placement against the exact float64 mesh distances."""
    clear = CR.exact_clearances(meshes, np.asarray(poses, np.float64))
    B = len(meshes)
    for a in range(B):
        assert all(settled), settled
        # 1: nothing deeper than E + tol in anything else (both directions of every pair are rows of `clear`)
        assert clear[a].min() >= -E - tol, (a, clear[a].tolist(), E)
        # 2: it touches something: the plane, a body below it (its shell in their field, or theirs in its own)
        nearest = min(clear[a].min(), min((clear[b, a] for b in range(B) if b != a), default=np.inf))
        assert nearest <= tol + E, (a, nearest, E)
        # 3: orientation and lateral position are what was asked for
        assert np.allclose(poses[a][:3, :3], orientations[a], atol=1e-12)
        assert np.allclose(poses[a][:2, 3], xy[a], atol=1e-12)
    return clear
