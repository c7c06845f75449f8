"""Inputs of the minimal-oriented-box and diameter tests, made in code (no hull library is needed to build them).

A case is (points float32 [P,3], triangles int32 [F,3]).  TF, TP and TD are the kernels' tiles as include/pegasus_raster.h
declares them: triangles per workgroup, points staged per LDS tile, points per diameter tile.
"""
import re
from functools import lru_cache
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
_HEADER = (ROOT / "include" / "pegasus_raster.h").read_text()


def _define(name):
    m = re.search(rf"#define {name} (\d+)", _HEADER)
    assert m, f"{name} is not defined in include/pegasus_raster.h"
    return int(m[1])


TF, TP, TD = _define("PGR_OBB_TRI_TILE"), _define("PGR_OBB_POINT_TILE"), _define("PGR_DIAMETER_TILE")
EDGE_F = (1, TF - 1, TF, TF + 1, 3 * TF + 1)
EDGE_P = (3, TP - 1, TP, TP + 1, 2 * TP + 1)
DIAMETER_P = (1, 2, TD - 1, TD, TD + 1, 2 * TD + 1, 20011)
OFFSET = np.array([1000.0, -2000.0, 500.0])
BOX_DIMS = np.array([60.0, 160.0, 210.0])                # the 6 x 16 x 21 cm box, in millimetres as BOP models are


def rotation(seed):
    """A rotation from a seeded QR decomposition."""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def tetrahedron():
    p = np.array([[0, 0, 0], [1, 0, 0], [0.2, 0.9, 0], [0.3, 0.3, 0.8]], np.float32)
    return p, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)


# corner index = 4 x + 2 y + z; every triangle starts at the right angle of its face, its two edges along box edges
BOX_TRIANGLES = np.array([[0, 2, 1], [3, 1, 2], [4, 5, 6], [7, 6, 5], [0, 1, 4], [5, 4, 1],
                          [2, 6, 3], [7, 3, 6], [0, 4, 2], [6, 2, 4], [1, 3, 5], [7, 5, 3]], np.int32)


def box_corners_exact(dims=BOX_DIMS, R=None, t=OFFSET):
    """The 8 corners in float64, before they are rounded to float32."""
    R = rotation(11) if R is None else R
    c = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)]) * dims
    return c @ R.T + t


def box_rounding_allowance(dims, exact_corners, roundings=1):
    """What rounding a box's exact corners to float32 (``roundings`` times in a row) allows its minimal box: (delta, grow, shrink).
    The float64 bounds of tests/obb_reference.py are 1e-8 of it.
    A coordinate moves by at most 2^-24 of itself per rounding, so a point moves by at most delta = roundings 2^-24
    max(|x| + |y| + |z|) along any direction.  A hull triangle's first edge u runs along a box edge or a face diagonal; one that
    runs along an edge spans the box's own frame up to a turn theta: u turns by 2 delta / L_min; w = u x v0 by
    |delta w| / |w| <= 2 delta (|u| + |v0|) / (|u| |v0| sin) <= 4 delta / (L_min sin), where sin >= L_min / (largest face
    diagonal); v = w x u by both.  Every extent of that candidate is within grow = 2 delta + theta (space diagonal) of the
    box's, so the smallest volume is at most prod(dims + grow), and a face lies within grow of the box's: a corner, where
    three meet, within 3 grow.  From below: a box that holds the rounded points, grown by delta on every side, holds the
    exact corners, whose smallest box is the box itself: prod(e + 2 delta) >= V; no extent e of a candidate exceeds the
    cloud's diameter D = space diagonal + 2 delta, so prod(e) >= V - (2 delta 3 D^2 + 4 delta^2 3 D + 8 delta^3) = V - shrink."""
    dims = np.sort(np.asarray(dims, np.float64))
    delta = roundings * 2.0 ** -24 * np.abs(exact_corners).sum(axis=1).max()
    face_diag = np.sqrt(dims[1] ** 2 + dims[2] ** 2)
    theta = 2 * delta / dims[0] + 4 * delta * face_diag / dims[0] ** 2
    grow = 2 * delta + theta * np.linalg.norm(dims)
    D = np.linalg.norm(dims) + 2 * delta
    return delta, grow, 6 * delta * D ** 2 + 12 * delta ** 2 * D + 8 * delta ** 3


def rotated_box():
    return box_corners_exact().astype(np.float32), BOX_TRIANGLES.copy()


def icosphere(level):
    """Unit icosphere: 12 / 42 / 162 / 642 points, 20 / 80 / 320 / 1280 outward triangles at levels 0..3."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, np.int32)


def affine_icosphere(level, offset=(0.0, 0.0, 0.0)):
    """The icosphere under x -> A x + offset, A = rotation . diag(0.03, 0.08, 0.10) . rotation: an affine image of a convex
    polyhedron keeps its triangulation as its hull."""
    v, f = icosphere(level)
    A = rotation(5) @ np.diag([0.03, 0.08, 0.10]) @ rotation(6)
    return (v @ A.T + np.asarray(offset)).astype(np.float32), f


def random_case(F, P, seed=None):
    """P random points and F random triangles over them with three distinct indices each."""
    rng = np.random.default_rng(1000 * F + P if seed is None else seed)
    pts = rng.uniform(-1, 1, size=(P, 3)).astype(np.float32)
    tri = np.stack([rng.permutation(P)[:3] for _ in range(F)]).astype(np.int32)
    return pts, tri


@lru_cache(maxsize=None)
def split_case():
    """12 triangles over 100 003 points (the point-split path): the rotated box's corners first, the rest inside the box
    grown by 1.5 about its centre, so that no candidate is the box itself."""
    corners, tris = rotated_box()
    rng = np.random.default_rng(42)
    inner = (rng.uniform(-0.75, 0.75, size=(100003 - 8, 3)) * BOX_DIMS) @ rotation(11).T + OFFSET
    return np.concatenate([corners, inner.astype(np.float32)]), tris


def split_case_embedded(n=5000):
    """The same points, the same 12 triangles at positions spread among ``n`` random ones.  Returns (points, triangles,
    the 12 positions)."""
    pts, tris = split_case()
    rng = np.random.default_rng(43)
    tri = np.stack([rng.choice(len(pts), 3, replace=False) for _ in range(n)]).astype(np.int32)
    where = np.sort(rng.choice(n, len(tris), replace=False))
    tri[where] = tris
    return pts, tri, where


def ball_cloud(n, seed=3, offset=(0.0, 0.0, 0.0)):
    """n points uniform in the unit ball, moved by ``offset``."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d *= (rng.uniform(size=(n, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    return (d + np.asarray(offset)).astype(np.float32)


def all_cases():
    """name -> (points, triangles): everything compared per element with the reference."""
    out = {"tetrahedron": tetrahedron(), "rotated_box": rotated_box(), "split": split_case()}
    for level in range(4):
        out[f"icosphere{level}"] = affine_icosphere(level)
    out["icosphere2_offset"] = affine_icosphere(2, OFFSET)
    for F in EDGE_F:
        for P in EDGE_P:
            out[f"random_F{F}_P{P}"] = random_case(F, P)
    return out
