"""The transcription of pgr_mesh_visibility + pgr_mesh_shade (tests/mesh_shade_reference.py) against answers worked out by
hand, the mutants those answers must reject, and against the float64 oracle on every case the GPU test runs.  No GPU."""
import functools

import numpy as np
import pytest

import mesh_raster_cases as MC
import mesh_raster_reference as MR
import mesh_shade_cases as SC
import mesh_shade_reference as SR

MAX_MASKED = 0.01                # as tests/test_mesh_raster_gpu.py: a condition on the inputs
REL = 2e-6                       # hand values computed in float64 against float32 results: a few dozen roundings of 2^-24


def rgb_triangle(faces):
    """Red, green and blue vertices at the image points (0.5, 0.5), (8.5, 0.5), (0.5, 8.5), all at Z = 2 (fx = fy = 2):
    pixel (i, j) samples (i + 0.5, j + 0.5), so with equal Z the weights are the screen barycentrics (1 - (i + j) / 8, i / 8,
    j / 8), all dyadic: every operation of the rule is exact."""
    job = MC.job(SC.plane_points([(0.5, 0.5), (8.5, 0.5), (0.5, 8.5)]), faces, fx=2.0, fy=2.0)
    job["colors"] = np.eye(3, dtype=np.float32)
    return job


def check_rgb_triangle(shade):
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):
        job = rgb_triangle(faces)
        r = shade([job], 10, 10, 0.25, use_colors=True, ambient=1.0)          # light_w = min(1 + diffuse, 1) = 1: rgb = colour
        for (i, j), want in (((0, 0), (1.0, 0.0, 0.0)), ((4, 2), (0.25, 0.5, 0.25)), ((1, 6), (0.125, 0.125, 0.75))):
            assert r["rgb"][0, j, i].tolist() == list(want), (faces, i, j, r["rgb"][0, j, i])
            assert r["xyz"][0, j, i].tolist() == [i + 0.5, j + 0.5, 2.0]
        assert (r["face_id"][0] >= 0).sum() == 36 and r["face_id"][0, 0, 8] == -1 and (r["rgb"][0, 0, 8] == 0).all()
    # the points sit on the lattice lattice_nudge moves to, to within its 1/4096 pixel: the same snapped integers
    nudged = dict(job, vertices=MC.lattice_nudge(job["vertices"], 0.0, 2.0, 2.0, 0.0, 0.0))
    for a, b in zip(MR._project(job, np.float32)[3:], MR._project(nudged, np.float32)[3:]):
        assert (MR._snap(a) == MR._snap(b)).all()


def tilted_quad(faces=((0, 1, 2), (0, 2, 3)), **kw):
    """The quad A (0, 0, 2), B (1, 0, 4), C (1, 1.5, 4), D (0, 0.75, 2) in the plane z = 2 + 2 x, fx = fy = 16, cx = cy = 0.5:
    it projects to the image points (0.5, 0.5), (4.5, 0.5), (4.5, 6.5), (0.5, 6.5) exactly, covering pixels 0 <= i < 4,
    0 <= j < 6.  The ray of pixel (i, j) is s (i / 16, j / 16, 1) and meets the plane at s = 2 / (1 - i / 8).  The plane's
    unit normal towards the camera is (2, 0, -1) / sqrt(5): 63.4 degrees off the view axis."""
    pts = np.array([[0, 0, 2], [1, 0, 4], [1, 1.5, 4], [0, 0.75, 2]], np.float32)
    return MC.job(pts, np.asarray(faces, np.int32), fx=16.0, fy=16.0, cx=0.5, cy=0.5, **kw)


def quad_point(i, j):
    s = 2.0 / (1.0 - i / 8.0)
    return np.array([s * i / 16.0, s * j / 16.0, s])


def quad_light_w(i, j, light=(0.0, 0.0, 0.0), ambient=0.5):
    P = quad_point(i, j)
    L = np.asarray(light, np.float64) - P
    cos = float(L @ (np.array([2.0, 0.0, -1.0]) / np.sqrt(5.0))) / np.linalg.norm(L)
    return min(1.0, ambient + max(cos, 0.0))


def check_tilted_quad_xyz(shade):
    r = shade([tilted_quad()], 6, 8, 0.25)
    assert (r["face_id"][0, :6, :4] >= 0).all() and (r["face_id"][0] >= 0).sum() == 24
    for i, j in ((2, 3), (0, 0), (3, 5), (1, 4)):
        np.testing.assert_allclose(r["xyz"][0, j, i], quad_point(i, j), rtol=REL, atol=1e-7)      # ray-plane intersection
        np.testing.assert_allclose(r["depth"][0, j, i], quad_point(i, j)[2], rtol=REL)
    np.testing.assert_allclose(r["xyz"][0, 3, 2], [1.0 / 3.0, 0.5, 8.0 / 3.0], rtol=REL)


def check_plane_lit_from_the_camera(shade):
    r = shade([tilted_quad()], 6, 8, 0.25)                                    # grey 0.5, ambient 0.5, light at the camera
    for i, j in ((0, 0), (2, 3), (3, 5), (1, 0)):
        want = quad_light_w(i, j)
        assert want < 1.0                                                    # cos(theta') <= 1 / sqrt(5): never clamped here
        np.testing.assert_allclose(r["rgb"][0, j, i], [0.5 * want] * 3, rtol=REL)
        np.testing.assert_allclose(r["normal"][0, j, i], np.array([2.0, 0.0, -1.0]) / np.sqrt(5.0), rtol=REL, atol=1e-7)
    np.testing.assert_allclose(r["rgb"][0, 0, 0, 0], 0.5 * (0.5 + 1.0 / np.sqrt(5.0)), rtol=REL)


def check_back_face_is_lit_like_its_mirror_image(shade):
    front = shade([tilted_quad()], 6, 8, 0.25)
    back = shade([tilted_quad(faces=((0, 2, 1), (0, 3, 2)))], 6, 8, 0.25)
    assert front["normal"].tobytes() == back["normal"].tobytes()             # cross(u, v) = -cross(v, u) exactly, then the flip
    np.testing.assert_allclose(back["rgb"], front["rgb"], rtol=REL)
    for i, j in ((0, 0), (2, 3)):
        np.testing.assert_allclose(back["rgb"][0, j, i], [0.5 * quad_light_w(i, j)] * 3, rtol=REL)
        np.testing.assert_allclose(front["rgb"][0, j, i], [0.5 * quad_light_w(i, j)] * 3, rtol=REL)


def check_light_off_axis(shade):
    light = (3.0, -2.0, 1.0)
    r = shade([tilted_quad()], 6, 8, 0.25, light=light, ambient=0.25)
    seen = set()
    for i, j in ((0, 0), (2, 3), (3, 5), (3, 0)):
        want = quad_light_w(i, j, light, 0.25)
        seen.add(want < 1.0)
        np.testing.assert_allclose(r["rgb"][0, j, i], [0.5 * want] * 3, rtol=REL)
    assert True in seen                                                      # the light's cosine shows unclamped somewhere
    behind = shade([tilted_quad()], 6, 8, 0.25, light=(-4.0, 0.0, 6.0), ambient=0.25)         # behind the plane: diffuse 0
    np.testing.assert_allclose(behind["rgb"][0, 3, 2], [0.125] * 3, rtol=0, atol=0)


def check_coincident_faces(shade):
    P = SC.plane_points([(1.5, 1.5), (9.5, 1.5), (1.5, 9.5)] * 2)
    job = MC.job(P, [[0, 1, 2], [3, 4, 5]], fx=2.0, fy=2.0)
    job["colors"] = np.array([[1, 0, 0]] * 3 + [[0, 1, 0]] * 3, np.float32)
    r = shade([job], 12, 12, 0.25, use_colors=True, ambient=1.0)
    hit = r["face_id"][0] >= 0
    assert hit.sum() == 36 and (r["face_id"][0][hit] == 0).all() and (r["rgb"][0][hit] == [1.0, 0.0, 0.0]).all()


def check_jobs_in_one_slot(shade):
    far = SC.plane_points([(1.5, 1.5), (9.5, 1.5), (1.5, 9.5)], z=4.0)
    near = SC.plane_points([(1.5, 1.5), (9.5, 1.5), (1.5, 9.5)], z=2.0)
    mk = lambda P, col: dict(MC.job(P, [[0, 1, 2]], fx=2.0, fy=2.0), surf_color=col)
    red, green, blue = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    r = shade([mk(far, red), mk(near, green), mk(near, blue)], 12, 12, 0.25, ambient=1.0)
    hit = r["job_id"][0] >= 0
    assert hit.sum() == 36 and (r["job_id"][0][hit] == 1).all()              # the nearer job; of the two equal ones the lower
    assert (r["rgb"][0][hit] == green).all() and (r["depth"][0][hit] == 2.0).all()


HAND_CASES = [check_rgb_triangle, check_tilted_quad_xyz, check_plane_lit_from_the_camera, check_back_face_is_lit_like_its_mirror_image,
              check_light_off_axis, check_coincident_faces, check_jobs_in_one_slot]


@pytest.mark.parametrize("check", HAND_CASES, ids=lambda c: c.__name__[6:])
def test_hand_worked_case(check):
    check(SR.shade_f32)


@pytest.mark.parametrize("mutant", SR.MUTANTS)
def test_the_hand_cases_reject_the_mutant(mutant):
    shade = functools.partial(SR.shade_f32, mutant=mutant)
    rejected = []
    for check in HAND_CASES:
        try:
            check(shade)
        except AssertionError:
            rejected.append(check.__name__)
    print(f"{mutant}: rejected by {rejected}")
    assert rejected, f"no hand-worked case tells the mutant '{mutant}' from the rule"


def test_the_depth_of_the_transcription_is_render_f32s():
    for name in ("rotated triangle", "33 jobs in 5 slots", "degenerate faces"):
        c = SC.CASES[name]()
        r = SR.shade_f32(c["jobs"], c["W"], c["H"], c["near"], c["n_slots"], **c["opts"])
        depth, straddle = MR.render_f32(c["jobs"], c["W"], c["H"], c["near"], c["n_slots"])
        assert r["depth"].tobytes() == depth.tobytes() and r["straddle"] == straddle
        if c["straddle"] is not None:
            assert straddle == c["straddle"]
    job, W, H, want = MC.rotated_triangle_case()
    assert SR.shade_f32([job], W, H, 0.25)["depth"][0].tobytes() == want.tobytes()


@pytest.mark.parametrize("name", list(SC.CASES))
def test_transcription_against_the_float64_oracle(name):
    c = SC.CASES[name]()
    r = SR.shade_f32(c["jobs"], c["W"], c["H"], c["near"], c["n_slots"], **c["opts"])
    o = SR.shade_f64(c["jobs"], c["W"], c["H"], c["near"], r["keys"], c["n_slots"], **c["opts"])
    share = SR.compare(r, o)
    free = ~o["masked"] & (r["job_id"] >= 0)
    worst = {n: float(np.abs(r[n].astype(np.float64) - o[n]).max(-1)[free].max()) if free.any() else 0.0 for n in ("xyz", "normal", "rgb")}
    print(f"{name}: {int((r['job_id'] >= 0).sum())} covered, masked share {share:.5f}, worst errors {worst}, xyz bound {o['bounds']['xyz']:.3g}")
    assert share <= MAX_MASKED, f"oracle masks {share:.4f} of a canvas: the inputs are not fit for this check"


def test_empty_pixels_and_zero_normals():
    c = SC.CASES["zero normal"]()
    r = SR.shade_f32(c["jobs"], c["W"], c["H"], c["near"], **c["opts"])
    zero = r["face_id"][0] == 0
    assert zero.sum() > 20 and (r["normal"][0][zero] == 0).all()
    col = SR._resolve(r["job_id"], r["face_id"], c["jobs"], c["W"], c["H"], np.float32(c["near"]), np.float32,
                      dict(c["opts"], ambient=1.0, smooth=False))["rgb"]                      # light_w = 1: the colour itself
    assert (r["rgb"][0][zero] == np.float32(0.5) * col[0][zero]).all()                          # diffuse 0: ambient * colour
    c = SC.CASES["zero faces"]()
    r = SR.shade_f32(c["jobs"], c["W"], c["H"], c["near"], **c["opts"])
    assert (r["keys"] == 0).all() and (r["face_id"] == -1).all() and (r["job_id"] == -1).all() and (r["depth"] == 0).all()
    assert (r["xyz"] == 0).all() and (r["normal"] == 0).all() and (r["rgb"] == np.float32([0.25, 0.5, 0.75])).all()
