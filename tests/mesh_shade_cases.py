"""The cases of pgr_mesh_visibility + pgr_mesh_shade shared by the host test (transcription against the oracle) and the GPU
test (kernels against the transcription): name -> dict(jobs, W, H, near, n_slots, opts, straddle).  No reference code, no GPU.

A job is the dict of mesh_raster_cases.job plus ``normals``, ``colors`` (per vertex) and ``surf_color``."""
import numpy as np

import mesh_raster_cases as MC


def plane_points(points_uv, z=2.0, f=2.0):
    """Model points that R = I, t = 0, fx = fy = f project to the image points ``points_uv``; ``z``: one depth or one each."""
    zs = np.broadcast_to(np.asarray(z, np.float64), (len(points_uv),))
    return np.array([[u * zz / f, v * zz / f, zz] for (u, v), zz in zip(points_uv, zs)], np.float32)


def with_attributes(job, rng, normals=None):
    """``job`` with random vertex colours in [0,1] and normals (default: random unit vectors)."""
    n = len(job["vertices"])
    job["colors"] = rng.random((n, 3)).astype(np.float32)
    if normals is None:
        normals = rng.normal(size=(n, 3))
        normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    job["normals"] = np.asarray(normals, np.float32)
    return job


def radial(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def case(jobs, W, H, near=0.25, n_slots=None, straddle=None, **opts):
    return dict(jobs=jobs, W=W, H=H, near=near, n_slots=n_slots, straddle=straddle, opts=opts)


def rotated_triangle(flipped=False):
    job, W, H, _want = MC.rotated_triangle_case()
    job = with_attributes(dict(job, faces=np.asarray([[0, 2, 1]] if flipped else [[0, 1, 2]], np.int32)), np.random.default_rng(2))
    return case([job], W, H, use_colors=True)


def sphere(smooth):
    fx = fy = 64.0
    v, f = MC.icosphere(2, 1.0)
    v = MC.lattice_nudge(v, 4.0, fx, fy, 30.0, 26.0)
    job = with_attributes(MC.job(v, f, t=(0, 0, 4.0), fx=fx, fy=fy, cx=30.0, cy=26.0), np.random.default_rng(3), radial(v))
    return case([job], 60, 52, smooth=smooth, use_colors=True, light=(1.5, -2.0, 0.5) if smooth else (0.0, 0.0, 0.0))


def threshold_boxes():
    """Two faces side by side in one canvas: a clipped box of 17 x 16 samples (just over MESHR_LARGE_BOX = 256: queued) and
    one of 16 x 16 (just under: walked by its lane), vertices at different depths."""
    pts, faces = [], []
    for x0, y0, w, h in ((3, 2, 17, 16), (24, 3, 16, 16)):
        faces.append([len(pts), len(pts) + 1, len(pts) + 2])
        pts += [(x0 + 0.25, y0 + 0.25), (x0 + w - 0.25, y0 + 0.25), (x0 + 0.25, y0 + h - 0.25)]
    P = plane_points(pts, z=[1.0, 2.0, 4.0, 2.0, 4.0, 1.0])
    job = with_attributes(MC.job(P, faces, fx=2.0, fy=2.0), np.random.default_rng(4))
    return case([job], 44, 21, smooth=True, use_colors=True)


def mirrored():
    """A negative determinant: every front face arrives with area2 < 0 and is flipped; distinct attributes per vertex."""
    v, f = MC.icosphere(1, 1.0)
    R = np.diag([-1.0, 1.0, 1.0]) @ MC.rotation((1, 2, 3), 0.7)
    job = with_attributes(MC.job(v, f, R=R, t=(0.1, -0.05, 4.0), fx=80.0, fy=80.0, cx=24.5, cy=20.25), np.random.default_rng(5), radial(v))
    return case([job], 50, 41, smooth=True, use_colors=True)


def coincident():
    """Faces 0 and 1 coincide (same points in the same order, own vertices and colours): equal keys up to the face index.
    Jobs 0 and 1 (and 2, nearer, over a part) share slot 0 at the same pose: equal depth, the lower job wins."""
    quad = plane_points([(2.5, 2.5), (20.5, 2.5), (2.5, 14.5)] * 2, z=[2.0, 2.0, 4.0] * 2)
    rng = np.random.default_rng(6)
    a = with_attributes(MC.job(quad, [[0, 1, 2], [3, 4, 5]], fx=2.0, fy=2.0), rng)
    near_tri = plane_points([(8.5, 1.5), (23.5, 1.5), (8.5, 15.5)], z=1.0)
    b = with_attributes(MC.job(near_tri, [[0, 1, 2]], fx=2.0, fy=2.0), rng)
    return case([a, dict(a), b, dict(a, slot=1)], 24, 16, n_slots=2, use_colors=True)


def surf_colours():
    """colors == NULL: two jobs of one mesh at one pose in one slot (the lower job's colour shows) and a third beside them."""
    v, f = MC.box((0.8, 0.5, 0.6))
    fx = fy = 64.0
    v = MC.lattice_nudge(v, 4.0, fx, fy, 0.0, 0.0)
    mk = lambda cx, col, tz=4.0: dict(MC.job(v, f, t=(0, 0, tz), fx=fx, fy=fy, cx=cx, cy=14.0), surf_color=col)
    return case([mk(16.0, (0.9, 0.2, 0.1)), mk(16.0, (0.1, 0.3, 0.8)), mk(30.0, (0.1, 0.3, 0.8), 4.5)], 48, 28, light=(0.5, 0.5, -1.0))


def many_jobs():
    """MESHR_JOBS_PER_LAUNCH + 1 = 33 jobs of a 12-face box into 5 slots, out of order: two raster launches, two table launches.
    Every job at a depth of its own (boxes that overlap in a slot then differ by far more than the depth bound), its vertices
    nudged onto the lattice for that depth."""
    fx = fy = 64.0
    v, f = MC.box((0.8, 0.5, 0.6))
    rng = np.random.default_rng(7)
    jobs = []
    for k in range(33):
        tz = 4.0 + 0.0625 * ((10 * k) % 33)
        jobs.append(with_attributes(MC.job(MC.lattice_nudge(v, tz, fx, fy, 0.0, 0.0), f, t=(0, 0, tz), fx=fx, fy=fy, cx=float(10 + (7 * k) % 40),
                                           cy=float(12 + (5 * k) % 30), slot=(3 * k + 1) % 5), rng, radial(v)))
    return case(jobs, 60, 52, n_slots=5, smooth=True, use_colors=True)


def thin(W, H):
    P = plane_points([(-3.0, -3.0), (80.0, -3.0), (-3.0, 70.0), (0.25, 0.25), (0.75, 0.25), (0.25, 0.75)], z=[2.0, 4.0, 1.0, 1.0, 1.0, 1.0])
    job = with_attributes(MC.job(P, [[0, 1, 2], [3, 4, 5]], fx=2.0, fy=2.0), np.random.default_rng(8))
    return case([job], W, H, smooth=True, use_colors=True)


def degenerate():
    """The mesh of the depth test: a collinear and a zero-area face, one off the canvas, a visible one, one behind the
    camera, three that straddle ``near`` (counted, no id) and two with a vertex index out of range."""
    P = plane_points([(2.5, 2.5), (9.5, 2.5), (16.5, 2.5), (2.5, 9.5), (-50.0, -50.0), (-40.0, -50.0), (-50.0, -40.0), (3.0, 12.0), (12.0, 12.0),
                      (3.0, 20.0)])
    behind = np.array([[0.1, 0.1, -1.0], [0.5, 0.1, -2.0], [0.1, 0.5, 0.1]], np.float32)
    strad = np.array([[1.0, 1.0, 2.0], [3.0, 1.0, 2.0], [1.0, 3.0, 0.125], [1.0, 3.0, -3.0]], np.float32)
    V = np.vstack([P, behind, strad])
    faces = [[0, 1, 2], [0, 0, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15], [13, 14, 16], [13, 15, 16], [7, 8, 99], [-1, 8, 9]]
    job = with_attributes(MC.job(V, faces, fx=2.0, fy=2.0), np.random.default_rng(9))
    return case([job], 32, 24, straddle=3, use_colors=True)


def zero_normal():
    """Face 0 has three zero model normals (normal 0, diffuse 0: rgb = ambient colour), face 1 one zero and two opposite
    ones (the interpolated normal passes through 0 inside the face)."""
    P = plane_points([(1.5, 1.5), (12.5, 1.5), (1.5, 10.5), (14.5, 1.5), (26.5, 1.5), (14.5, 10.5)])
    job = with_attributes(MC.job(P, [[0, 1, 2], [3, 4, 5]], fx=2.0, fy=2.0), np.random.default_rng(10))
    job["normals"] = np.array([[0, 0, 0]] * 3 + [[0, 0, 0], [0, 0, -1], [0, 0, 1]], np.float32)
    return case([job], 30, 13, smooth=True, use_colors=True)


def zero_faces():
    v, _f = MC.box()
    job = with_attributes(MC.job(v, np.zeros((0, 3), np.int32), t=(0, 0, 4.0)), np.random.default_rng(11))
    return case([job], 9, 7, use_colors=True, bg=(0.25, 0.5, 0.75))


CASES = {
    "rotated triangle": rotated_triangle, "rotated triangle, other winding": lambda: rotated_triangle(True),
    "icosphere smooth": lambda: sphere(True), "icosphere flat": lambda: sphere(False), "boxes across the large threshold": threshold_boxes,
    "mirrored": mirrored, "coincident faces and jobs": coincident, "surf colours": surf_colours, "33 jobs in 5 slots": many_jobs,
    "1x1": lambda: thin(1, 1), "1x40": lambda: thin(1, 40), "40x1": lambda: thin(40, 1), "17x13": lambda: thin(17, 13),
    "degenerate faces": degenerate, "zero normal": zero_normal, "zero faces": zero_faces,
}
