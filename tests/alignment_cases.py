"""Inputs of the alignment tests (tests/test_alignment_host.py, tests/test_alignment_gpu.py), all seeded, and their reference
results, computed once per process (tests/alignment_reference.py) and handed out read-only.

The scene: a ground square of 2 x 2 m with +-4 mm of uniform height (60 % of the rows), eight blobs 0 - 0.25 m above it (35 %)
and floaters in a 3 m cube (5 %), posed by a random rotation and an offset of metres, rows shuffled, float32.  Threshold 0.01.

A case is valid only if no decision of it sits near a tie, and every function below that hands out a case asserts it:
  MARGIN_MIN     coordinates are a few metres, where a float64 ulp is 9e-16; the seven operations of a distance stay below
                 1e-14, which leaves 1000 x headroom under 1e-11 m.  Held by |dist - threshold| of every point under every
                 valid hypothesis and, again, under the refitted plane.
  SUMSQ_GAP_MIN  the best and the second-best hypothesis differ in count, or in sumsq by more than 1e-9 relative (the sums
                 themselves agree to 1e-12).
The tolerance on the 4x4, T_TOL, is the reference's own error: 100 x the largest element-wise difference between its run in
numpy.longdouble and its run in float64 over END_TO_END, floor 1e-13.  Measured: see T_TOL_MEASURED;
tests/test_alignment_host.py::test_transformation_tolerance_is_the_references_own_error measures it again."""
import functools
import re
from pathlib import Path

import numpy as np

import alignment_reference as AR

ROOT = Path(__file__).resolve().parents[1]
THRESHOLD = 0.01
MARGIN_MIN = 1e-11
SUMSQ_GAP_MIN = 1e-9
SCENE_SEED, TRIPLE_SEED = 7, 11
END_TO_END = ((4099, 257), (1025, 65))                  # (points, hypotheses)
SHAPES = END_TO_END + ((257, 64),)
# largest |T_longdouble - T_float64| per shape: see the module docstring
T_TOL_MEASURED = {(4099, 257): 5.2e-15, (1025, 65): 4.7e-16}
T_TOL = max(1e-13, 100 * max(T_TOL_MEASURED.values()))                       # 5.2e-13
PLANE_DEG_MAX, PLANE_M_MAX = 0.1, 1e-3                  # how near the refitted plane must come to the known one
SCALE = 2.5


def _constant(name):
    text = (ROOT / "pegasus_amd" / "csrc" / "plane.hip.h").read_text()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text)[1])


PLANE_BLOCK, PLANE_POINTS_PER_LANE, PLANE_HYP_BATCH = (_constant(k) for k in
                                                       ("PLANE_BLOCK", "PLANE_POINTS_PER_LANE", "PLANE_HYP_BATCH"))
PLANE_SCORE_MIN_BLOCKS = _constant("PLANE_SCORE_MIN_BLOCKS")
TILE = PLANE_BLOCK * PLANE_POINTS_PER_LANE
SCORE_NS = (1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)         # at SCORE_H hypotheses
SCORE_H = 65
BATCH_HS = (1, PLANE_HYP_BATCH - 1, PLANE_HYP_BATCH, PLANE_HYP_BATCH + 1)         # at BATCH_N points
BATCH_N = 257
FINAL_BLOCKS = (1, 2, 15, 16, 17)                                                 # workgroups, at FINAL_H hypotheses
FINAL_H = 3
HYPOTHESIS_HS = (1, 63, 64, 65, 257)


def _frozen(a):
    a.setflags(write=False)
    return a


def _rotation(rng):
    """A rotation by a random angle of 0.5 - 2.5 rad about a random axis (Rodrigues)."""
    k = rng.normal(size=3)
    k /= np.linalg.norm(k)
    angle = rng.uniform(0.5, 2.5)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


@functools.lru_cache(maxsize=None)
def scene(n, seed=SCENE_SEED):
    """(points float32 [n,3], known plane float64 [4] with the normal towards the blobs, R, offset)."""
    rng = np.random.default_rng(seed)
    n_ground, n_blobs = int(round(0.6 * n)), int(round(0.35 * n))
    n_float = n - n_ground - n_blobs
    ground = np.concatenate([rng.uniform(-1.0, 1.0, (n_ground, 2)), rng.uniform(-0.004, 0.004, (n_ground, 1))], axis=1)
    centres = rng.uniform(-0.8, 0.8, (8, 2))
    which = rng.integers(0, 8, n_blobs)
    blobs = np.concatenate([centres[which] + rng.normal(0.0, 0.05, (n_blobs, 2)), rng.uniform(0.0, 0.25, (n_blobs, 1))], axis=1)
    floaters = rng.uniform(-1.5, 1.5, (n_float, 3))
    local = np.concatenate([ground, blobs, floaters])
    R, offset = _rotation(rng), rng.uniform(-3.0, 3.0, 3)
    world = (local @ R.T + offset)[rng.permutation(n)]
    normal = R[:, 2]
    return _frozen(world.astype(np.float32)), _frozen(np.append(normal, -normal @ offset)), _frozen(R), _frozen(offset)


def triples(n, h, seed=TRIPLE_SEED):
    return _frozen(np.random.default_rng(seed).integers(0, n, size=(h, 3)).astype(np.int32))


def cameras_above(n_points, count=5):
    """Camera centres 1 - 2 m above the ground of scene(n_points), on the side of the blobs."""
    _, _, R, offset = scene(n_points)
    rng = np.random.default_rng(23)
    local = np.concatenate([rng.uniform(-1.0, 1.0, (count, 2)), rng.uniform(1.0, 2.0, (count, 1))], axis=1)
    return _frozen(local @ R.T + offset)


def _check_margin(margin, what):
    assert margin >= MARGIN_MIN, f"{what}: a distance lies {margin:.3g} from the threshold; pick another seed"


@functools.lru_cache(maxsize=None)
def reference_fit(n, h, dtype="float64", oriented_by="cameras"):
    """The reference's whole fit of scene(n) with triples(n, h), valid by both conditions."""
    points = scene(n)[0]
    kw = dict(camera_centers=cameras_above(n)) if oriented_by == "cameras" else {}
    ref = AR.fit(points, triples(n, h), THRESHOLD, scale=SCALE, dtype=getattr(np, dtype), **kw)
    _check_margin(ref.margin, f"scene({n}) with {h} hypotheses")
    assert ref.sumsq_gap > SUMSQ_GAP_MIN, f"scene({n}) with {h} hypotheses: the two best tie; pick another seed"
    return ref


@functools.lru_cache(maxsize=None)
def score_case(n_points, n_hyp, source=(2 * TILE + 1, SCORE_H)):
    """(points, planes, reference scores): the first ``n_points`` rows of scene(source[0]) (its rows are shuffled, so any prefix
    covers it) against the first ``n_hyp`` planes of triples(*source) over the WHOLE scene, so that a prefix of one, two or three
    points still meets real planes."""
    points = scene(source[0])[0]
    planes, valid = AR.hypotheses(points, triples(*source))
    assert valid.sum() >= 0.9 * len(valid)
    points, planes = _frozen(np.ascontiguousarray(points[:n_points])), _frozen(np.ascontiguousarray(planes[:n_hyp]))
    ref = AR.scores(points, planes, THRESHOLD)
    _check_margin(ref.margin, f"score_case({n_points}, {n_hyp})")
    return points, planes, ref


def final_case(blocks):
    """``blocks`` workgroups of the score kernel: (blocks - 1) * TILE + 1 points at FINAL_H hypotheses."""
    big = (max(FINAL_BLOCKS) - 1) * TILE + 1
    return score_case((blocks - 1) * TILE + 1, FINAL_H, source=(big, FINAL_H))


def score_launch(n_points, n_hyp):
    """(tiles, hypothesis batches per workgroup, groups of batches) of pgr_plane_score's launch: the arithmetic of the entry.
    A cloud of fewer than PLANE_SCORE_MIN_BLOCKS tiles spreads the batches over the grid's y axis."""
    tiles = max((n_points + TILE - 1) // TILE, 1)
    batches = max((n_hyp + PLANE_HYP_BATCH - 1) // PLANE_HYP_BATCH, 1)
    wanted = min(batches, (PLANE_SCORE_MIN_BLOCKS + tiles - 1) // tiles)
    per_group = (batches + wanted - 1) // wanted
    return tiles, per_group, (batches + per_group - 1) // per_group


def grouped_shape(tiles=max(FINAL_BLOCKS)):
    """(points, hypotheses) at which every workgroup of the score kernel walks TWO batches, the last group a full batch and
    then one of a single hypothesis: the least even number of batches above what the launch would give a group each."""
    wanted = (PLANE_SCORE_MIN_BLOCKS + tiles - 1) // tiles
    batches = wanted + 1 if (wanted + 1) % 2 == 0 else wanted + 2
    return (tiles - 1) * TILE + 1, (batches - 1) * PLANE_HYP_BATCH + 1


def grouped_case():
    """The score case of grouped_shape(): the batch loop inside a workgroup, LDS reused from batch to batch, a short batch
    behind a full one."""
    n, h = grouped_shape()
    tiles, per_group, groups = score_launch(n, h)
    assert per_group == 2 and groups * per_group * PLANE_HYP_BATCH - h == PLANE_HYP_BATCH - 1 and groups > 1
    return score_case(n, h, source=(n, h))


@functools.lru_cache(maxsize=None)
def inlier_case(n_points):
    """(points, plane, pivot, reference): the first rows of the largest score scene under its best hypothesis of SCORE_H."""
    source = (2 * TILE + 1, SCORE_H)
    whole = scene(source[0])[0]
    planes, valid = AR.hypotheses(whole, triples(*source))
    sc = AR.scores(whole, planes, THRESHOLD)
    best, _ = AR.choose(sc.counts, sc.sumsq, valid)
    pivot = whole[int(triples(*source)[best, 0])].astype(np.float64)
    points = _frozen(np.ascontiguousarray(whole[:n_points]))
    ref = AR.inlier_sums(points, planes[best], pivot, THRESHOLD)
    _check_margin(ref.margin, f"inlier_case({n_points})")
    return points, _frozen(planes[best].copy()), _frozen(pivot), ref


def degenerate_triples(n):
    """Triples that must come out invalid without a read outside the points: repeated rows, rows -1 and n, the collinear and
    the coincident rows that degenerate_points() puts in front."""
    return np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [5, 5, 5], [-1, 0, 1], [0, -1, 1], [0, 1, -1], [n, 0, 1], [0, n, 1],
                     [0, 1, n], [-2 ** 31, 0, 1], [2 ** 31 - 1, 1, 2], [0, 1, 2], [3, 5, 6], [3, 4, 0]], dtype=np.int32)


def degenerate_points(n):
    """scene(n) with rows 0, 1, 2 collinear (exactly: small dyadic coordinates) and rows 3, 4 coincident."""
    points = np.array(scene(n)[0])
    points[0], points[1], points[2] = (0.5, 0.25, -1.0), (1.0, 0.5, -0.5), (2.0, 1.0, 0.5)
    points[4] = points[3]
    return _frozen(points)


def strictness():
    """(points, plane, threshold, expected mask): the plane through (0,0,0), (1,0,0), (0,1,0), where dist = |z| exactly."""
    inside = np.nextafter(np.float32(0.25), np.float32(0))
    z = np.array([0.25, -0.25, inside, -inside, 0.0, 0.5], dtype=np.float32)
    points = np.stack([np.linspace(-1, 1, len(z), dtype=np.float32), np.ones(len(z), dtype=np.float32), z], axis=1)
    points = np.concatenate([np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32), points])
    return points, np.array([[0, 1, 2]], dtype=np.int32), 0.25, np.array([1, 1, 1, 0, 0, 1, 1, 1, 0], dtype=np.uint8)
