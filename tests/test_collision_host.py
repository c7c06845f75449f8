"""Host side of the collision geometry, without a device: the cases are sound by the float64 reference alone (the census of
exempt points, the trilinear slack, the placement scenes), resting orientations, the reference's file layout, the word packing."""
import json

import numpy as np
import pytest

import collision_cases as CC
import collision_reference as CR


# ---- the reference itself ---------------------------------------------------------------------------------------------------
def test_reference_distance_and_winding_on_known_shapes():
    v, f = CC.cube()
    p = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.9], [0.9, 0.9, 0.9], [0.9, 0.0, 0.9], [0.2, 0.1, 0.45]])
    d, w = CR.mesh_distance(p, v, f)
    assert np.allclose(d, [0.5, 0.4, 0.4 * 3 ** 0.5, 0.4 * 2 ** 0.5, 0.05], atol=1e-15)
    assert np.allclose(w, [1, 0, 0, 0, 1], atol=1e-14)
    # against brute-force sampling of one triangle
    rng = np.random.default_rng(0)
    a, b, c = rng.normal(size=(3, 3))
    q = rng.normal(size=(50, 3)) * 2
    uv = rng.uniform(size=(200000, 2))
    uv[uv.sum(1) > 1] = 1 - uv[uv.sum(1) > 1]
    cloud = a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a)
    brute = np.array([np.linalg.norm(cloud - x, axis=1).min() for x in q])
    exact = CR.point_triangle_distance(q, a, b, c)
    assert np.all(exact <= brute + 1e-12) and np.all(brute - exact < 2e-2)
    # a triangle without area is its segment
    assert np.allclose(CR.point_triangle_distance(np.array([[0.5, 1.0, 0.0], [3.0, 0.0, 4.0]]), np.zeros(3), np.array([1.0, 0, 0]),
                                                  np.array([2.0, 0, 0])), [1.0, 17 ** 0.5])


@pytest.mark.parametrize("name", sorted(CC.SDF_CASES))
def test_census_of_exempt_points(name):
    """From the reference alone: at most 1 % of a case's points are exempt from the sign comparison; the closed meshes at 24^3
    have none, and their winding numbers are 0 or 1."""
    v, f, g, ref = CC.sdf_case(name)
    assert ref["d"].shape == g.shape
    if not ref["with_sign"]:
        assert name == "on_surface" and (ref["d"] == 0).sum() >= 8 + 12 + 6          # vertices, edge and face centres
        return
    exempt = 1.0 - ref["sure"].mean()
    assert exempt <= CC.MAX_EXEMPT, (name, exempt)
    if name in CC.CLOSED_24:
        assert ref["sure"].all()
        assert np.abs(ref["w"] - np.round(ref["w"])).max() < 1e-12 and set(np.round(ref["w"]).ravel()) == {0.0, 1.0}
    if len(f) == 0:
        assert np.isinf(ref["d"]).all() and (ref["w"] == 0).all()
    assert np.isfinite(ref["bound"]).all() or len(f) == 0
    assert ref["kappa"] < 8                                                       # no slivers: the bound stays a few hundred u


def test_tile_edge_cases_have_the_counts_they_name():
    for n in (0, 1, CC.FACE_TILE - 1, CC.FACE_TILE, CC.FACE_TILE + 1):
        assert len(CC.sdf_case(f"faces_{n}")[1]) == n
    v, f, _, ref = CC.sdf_case("degenerate_5x7x9")
    cube_ref = CC.sdf_case("cube_5x7x9")[3]
    assert np.array_equal(ref["d"], cube_ref["d"]) and np.abs(ref["w"] - cube_ref["w"]).max() < 1e-12
    assert np.array_equal(v[8], v[0])


def test_trilinear_sample_is_within_the_lipschitz_slack_of_the_exact_distance():
    """|trilinear - exact| <= (sqrt(3) / 2) voxel: the distance is 1-Lipschitz, so a corner value differs from the value at the
    point by at most their distance, and the trilinear value is a convex combination of the corners."""
    body = CC.ref_body("icosphere")
    g = body.grid
    rng = np.random.default_rng(1)
    lo = g.origin
    p = lo + rng.uniform(0, 1, (4000, 3)) * g.voxel * (g.n - 1)
    value, _, _ = CR.sample(body.field, g, p)
    pf = p.astype(np.float32)
    d, w = CR.mesh_distance(pf, body.vertices, body.faces)
    worst = np.abs(value - CR.signed(d, w)).max()
    assert worst <= CC.drop_slack([g.voxel]), (worst, g.voxel)
    # outside the grid the rule is a lower bound of the distance (up to the same slack, which the clamped sample carries) ...
    far = lo - rng.uniform(0.1, 2.0, (200, 3))
    v_far, _, info = CR.sample(body.field, g, far)
    d_far, _ = CR.mesh_distance(far.astype(np.float32), body.vertices, body.faces)
    assert (info["r"] > 0).all() and np.all(v_far <= d_far + CC.drop_slack([g.voxel]))
    # ... which the plain sum of the box distance and the clamped field is not: it is the triangle inequality's UPPER bound
    at_box, _, _ = CR.sample(body.field, g, np.clip(far, lo, lo + g.voxel * (g.n - 1)))
    assert np.any(info["r"] + at_box > d_far + 2 * g.voxel)


def test_sample_case_covers_every_side_and_a_corner():
    field, g, points, n_inside = CC.sample_case()
    _, _, info = CR.sample(field, g, points, True)
    assert (info["r"][:n_inside] == 0).all() and (info["border"][:n_inside] > 0.05).all()
    assert (info["r"][n_inside:] > 0).all() and len(points) - n_inside == 8


@pytest.mark.parametrize("name", CC.DROP_SCENES)
def test_placement_scenes_are_sound_in_the_reference(name):
    """The reference's own transcription of the loop places every scene within the bounds the GPU test asserts."""
    meshes, orientations, xy = CC.drop_scene(name)
    bodies = CC.drop_ref_bodies(name)
    poses, rounds, settled = CR.drop_reference(bodies, orientations, xy, CC.DROP_TOL)
    E = CC.drop_slack([b.grid.voxel for b in bodies])
    clear = CC.assert_placement(meshes, poses, orientations, xy, settled, E)
    assert max(rounds) <= 4, rounds
    if name == "sphere_0":                                  # the sphere stands on the cube: centre at 1 + 0.5
        assert abs(poses[1][2, 3] - 1.5) < E and clear[1, 0] < E
    if name == "sphere_5":                                  # beside the cube: on the plane
        assert abs(poses[1][2, 3] - 0.5) < 1e-3


# ---- resting orientations -------------------------------------------------------------------------------------------------------
def _mesh(v, f):
    from pegasus_amd.mesh import Mesh
    return Mesh(np.asarray(v, np.float32), np.asarray(f, np.int32))


def _cone(n=16, radius=0.5, height=1.0):
    ring = [(radius * np.cos(2 * np.pi * k / n), radius * np.sin(2 * np.pi * k / n), 0.0) for k in range(n)]
    v = np.asarray(ring + [(0.0, 0.0, 0.0), (0.0, 0.0, height)])
    f = []
    for k in range(n):
        j = (k + 1) % n
        f += [(k, j, n + 1), (j, k, n)]
    return _mesh(v, f)


def _box(ext):
    v, f = CC.cube()
    return _mesh(v.astype(np.float64) * np.asarray(ext), f)


def _assert_stable(mesh, rotations, normals):
    """In float64: every orientation turns its face down and puts the centre of mass over the face's polygon."""
    from scipy.spatial import ConvexHull
    c = mesh.center_of_mass()
    v = mesh.vertices.astype(np.float64)
    for R, n in zip(rotations, normals):
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0.999
        assert np.allclose(R @ n, [0, 0, -1], atol=1e-12)
        w = v @ R.T
        low = w[:, 2].min()
        support = w[w[:, 2] < low + 1e-6][:, :2]
        assert len(support) >= 3
        hull = ConvexHull(support)
        com = (R @ c)[:2]
        assert np.all(hull.equations[:, :2] @ com + hull.equations[:, 2] <= 1e-9)


def test_resting_orientations_of_a_box():
    from pegasus_amd import collision as COL
    ext = np.array([1.0, 2.0, 3.0])
    box = _box(ext)
    R, w, n = COL.resting_orientations(box)
    assert len(R) == 6 and abs(w.sum() - 1) < 1e-12
    _assert_stable(box, R, n)
    for normal, weight in zip(n, w):
        axis = int(np.abs(normal).argmax())
        assert abs(abs(normal[axis]) - 1) < 1e-9
        a, b = np.delete(ext, axis) / 2
        h = ext[axis] / 2
        solid = 4 * np.arctan(a * b / (h * np.sqrt(a * a + b * b + h * h)))          # a rectangle seen from above its centre
        assert abs(weight - solid / (4 * np.pi)) < 1e-9


def test_resting_orientations_of_a_cone():
    from pegasus_amd import collision as COL
    cone = _cone()
    R, w, n = COL.resting_orientations(cone)
    _assert_stable(cone, R, n)
    base = [k for k in range(len(n)) if np.allclose(n[k], [0, 0, -1], atol=1e-9)]
    side = [k for k in range(len(n)) if k not in base]
    assert len(base) == 1 and len(side) == 16
    slope = np.arctan2(0.5 * np.cos(np.pi / 16), 1.0)                                # the side facets' normals rise by this
    assert np.allclose([n[k][2] for k in side], np.sin(slope), atol=1e-9)


def test_resting_orientations_leave_out_faces_the_centre_of_mass_is_not_over():
    from pegasus_amd import collision as COL
    # a tall wedge leaning far over: a box sheared along x
    v, f = CC.cube()
    v = v.astype(np.float64)
    v[:, 0] += 2.0 * (v[:, 2] + 0.5)
    sheared = _mesh(v, f)
    R, w, n = COL.resting_orientations(sheared)
    _assert_stable(sheared, R, n)
    assert len(R) < 6


# ---- files --------------------------------------------------------------------------------------------------------------------
def test_simulation_steps_round_trip(tmp_path):
    from scipy.spatial.transform import Rotation
    from pegasus_amd import collision as COL, trajectory as TR
    rng = np.random.default_rng(3)
    poses = np.tile(np.eye(4), (3, 1, 1))
    poses[:, :3, :3] = Rotation.random(3, random_state=4).as_matrix()
    poses[:, :3, 3] = rng.normal(size=(3, 3))
    centers = rng.normal(size=(3, 3))
    path = tmp_path / "sub" / "simulation_steps.json"
    COL.write_simulation_steps(path, ["obj_000001", "obj_000001", "obj_000005"], ["mug", "mug", "can"], [1, 1, 5], poses, centers, steps=2)
    doc = json.loads(path.read_text())
    assert set(doc) == {"asset_infos", "trajectory"}
    assert doc["asset_infos"]["object"]["obj_000001"] == {"bullet_id": [1, 2], "center_of_mass": centers[0].tolist(),
                                                          "class_name": "mug", "object_ID": 1}
    assert doc["asset_infos"]["object"]["obj_000005"]["bullet_id"] == [3]
    assert sorted(doc["trajectory"]) == ["0", "1", "2", "3"] and sorted(doc["trajectory"]["1"]) == ["0", "1"]
    # the reference's static mode: the last step of body 1's keys, q as scipy's x, y, z, w
    last = list(doc["trajectory"]["1"].keys())[-1]
    x = rng.normal(size=(20, 3))
    rows = COL.read_simulation_steps(path)
    for k in range(3):
        step = doc["trajectory"][str(k + 1)][last]
        assert np.allclose(Rotation.from_quat(step["q"]).as_matrix(), poses[k, :3, :3], atol=1e-12)
        T = TR.absolute_pose(rows[k + 1][None], 0)
        mu = centers[k]
        moved = (x - mu) @ T[:3, :3].T + mu + T[:3, 3]                           # the reference applies a pose about the mean
        assert np.allclose(moved, x @ poses[k, :3, :3].T + poses[k, :3, 3], atol=1e-12)
    with pytest.raises(ValueError):
        COL.write_simulation_steps(path, ["a"], ["a"], [1, 2], poses[:1])


def test_word_packing_orders_like_the_floats():
    from pegasus_amd import collision as COL
    values = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], np.float32)
    words = [CR.word(v, 7) for v in values]
    assert words == sorted(words) and len(set(words)) == len(words)
    assert CR.word(1.0, 3) < CR.word(1.0, 4)
    got_v, got_i = COL.decode_words(np.array(words + [2 ** 64 - 1], np.uint64))
    assert got_v[:-1].tobytes() == values.tobytes() and (got_i[:-1] == 7).all()
    assert got_v[-1] == np.inf and got_i[-1] == -1
    # as the int64 tensor holds them
    got_v2, _ = COL.decode_words(np.array(words, np.uint64).view(np.int64))
    assert got_v2.tobytes() == values.tobytes()


def test_mesh_files_finds_plys_and_collision_objs(tmp_path):
    from pegasus_amd import collision as COL, mesh as M
    v, f = CC.cube()
    (tmp_path / "urdf").mkdir()
    M.write_obj(tmp_path / "urdf" / "obj_000003_collision.obj", M.Mesh(v, f))
    assert COL.mesh_files(tmp_path) == {3: tmp_path / "urdf" / "obj_000003_collision.obj"}
    back = COL.read_obj(tmp_path / "urdf" / "obj_000003_collision.obj")
    assert np.array_equal(back.vertices, v) and np.array_equal(back.faces, f)
    M.write_ply(tmp_path / "obj_000002.ply", M.Mesh(v, f))
    assert list(COL.mesh_files(tmp_path)) == [2]
    with pytest.raises(FileNotFoundError):
        COL.mesh_files(tmp_path / "urdf" / "nothing")
