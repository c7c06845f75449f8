"""Shapes and poses shared by the mesh-rasterizer tests and the golden generator (no reference code, no GPU)."""
import numpy as np


def icosphere(subdivisions: int, radius: float = 1.0):
    """(vertices float32 [V,3], faces int32 [F,3]) of a closed icosphere, outward winding."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(np.float32), np.asarray(f, np.int32)


def box(half=(1.0, 1.0, 1.0)):
    """The 12-face box [-h, h]^3."""
    h = np.asarray(half, np.float64)
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * h
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return v.astype(np.float32), np.asarray(f, np.int32)


def job(vertices, faces, R=None, t=(0, 0, 0), fx=100.0, fy=100.0, cx=0.0, cy=0.0, slot=0):
    return dict(vertices=np.asarray(vertices, np.float32), faces=np.asarray(faces, np.int32),
                R=np.eye(3) if R is None else np.asarray(R, np.float64), t=np.asarray(t, np.float64), fx=fx, fy=fy, cx=cx, cy=cy,
                slot=slot)


def rotation(axis, angle):
    from scipy.spatial.transform import Rotation as Rot
    a = np.asarray(axis, np.float64)
    return Rot.from_rotvec(a / np.linalg.norm(a) * angle).as_matrix()


def rotated_triangle_case():
    """(job, W, H, depth float32 [H,W]) derived by hand, with nothing symmetric: the rotation is the cyclic permutation
    X = p.y, Y = p.z, Z = p.x (its transpose gives X = p.z, Y = p.x, Z = p.y), t = (-3, 5, 0.5), fx = 2, fy = 4, cx = 3, cy = 1.

    The model points a = (0.5, 3.25, -4.875), b = (1.5, 11.5, -4.75), c = (3.5, 4, 3.5) reach the camera at (0.25, 0.125, 1),
    (8.5, 0.25, 2), (1, 8.5, 4) and the image at (0.5, 0.5) + (cx, cy), (8.5, 0.5) + (cx, cy), (0.5, 8.5) + (cx, cy); every
    operation on the way is exact in float32.  Pixel (i + 3, j + 1) samples (i + 0.5, j + 0.5) + (cx, cy): it is covered for
    i >= 0, j >= 0 (the left and the top edge own their samples) and i + j < 8 (the hypotenuse is neither, its samples stay
    empty).  1/z is affine in the image: 1 at a, 1/2 at b, 1/4 at c, so 1/z = 1 - i/16 - 3j/32 and z = 32 / (32 - 2i - 3j),
    rounded once: the integer edge values times 1, 1/2 and 1/4 and their sum are exact."""
    R = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], np.float64)
    pts = np.array([[0.5, 3.25, -4.875], [1.5, 11.5, -4.75], [3.5, 4.0, 3.5]], np.float32)
    W, H = 16, 12
    want = np.zeros((H, W), np.float32)
    for j in range(8):
        for i in range(8 - j):
            want[j + 1, i + 3] = np.float32(32) / np.float32(32 - 2 * i - 3 * j)
    return job(pts, [[0, 1, 2]], R=R, t=(-3.0, 5.0, 0.5), fx=2.0, fy=4.0, cx=3.0, cy=1.0), W, H, want


def lattice_nudge(vertices, tz, fx, fy, cx, cy):
    """Moves every vertex sideways (by less than 1/1024 pixel) so that, for R = I and t = (0, 0, tz), it projects onto the
    image lattice k / 1024 + 1 / 4096 pixel: the snapped coordinate q = 256 u - 128 then sits at least 1/16 away from a
    rounding boundary, far more than float32 and float64 projections differ, so both snap alike."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    Z = (v[:, 2].astype(np.float32) + np.float32(tz)).astype(np.float64)
    out = v.copy()
    for a, (f, c) in enumerate(((fx, cx), (fy, cy))):
        u = f * v[:, a] / Z + c
        uq = np.round(u * 1024) / 1024 + 1.0 / 4096
        out[:, a] = (uq - c) * Z / f
    return out.astype(np.float32)
