"""The vertex-attribute rules without a GPU: the NumPy transcriptions (tests/mesh_attr_reference.py) held against answers
worked out by hand, against mutants of the colour rule, against mesh_render.vertex_normals (float64) and the float64
colour oracle, on the analytic sphere, and over the cases the device tests use (each reaches the branches it names);
then the host plumbing of pegasus_amd.mesh: the Mesh fields, fill_unseen and write_ply."""
import math

import numpy as np
import pytest

import mesh_attr_cases as AC
import mesh_attr_reference as AR

f32 = np.float32


# ---- normals --------------------------------------------------------------------------------------------------------
def test_flat_fan_is_exactly_plus_z():
    v, f = AC.fan(7)
    n = AR.normals_f32(v, f)
    assert n.dtype == np.float32
    np.testing.assert_array_equal(n, np.tile(f32([0, 0, 1]), (len(v), 1)))


def test_cube_corners_for_this_triangulation():
    """The rule sums per TRIANGLE: the corners 0 and 7, where every face's diagonal starts, hold 2 + 2 + 2 triangles and get
    (1,1,1) / sqrt 3; every other corner holds 2 triangles of one face and 1 of each of the other two."""
    n = AR.normals_f32(AC.CUBE_VERTICES, AC.CUBE_FACES)
    counts = {0: (-2, -2, -2), 1: (2, -1, -1), 2: (-1, 2, -1), 3: (1, 1, -2), 4: (-1, -1, 2), 5: (1, -2, 1), 6: (-2, 1, 1),
              7: (2, 2, 2)}
    for corner, s in counts.items():
        s = np.asarray(s, np.float64)
        np.testing.assert_array_equal(n[corner], (s / np.sqrt((s * s).sum())).astype(f32), err_msg=str(corner))
    assert abs(float(n[1][0]) - 2 / math.sqrt(6)) < 1e-7 and abs(float(n[1][0]) - 1 / math.sqrt(3)) > 0.2
    sums, _ = AR.normal_sums(AC.CUBE_VERTICES, AC.CUBE_FACES)
    np.testing.assert_array_equal(sums[3], np.array([1, 1, -2], np.int64) << 30)


def test_zero_area_faces_isolated_vertices_winding_and_bad_indices():
    v, f = AC.icosphere(1, 0.5, (0.1, 0.2, -0.3))
    base = AR.normals_f32(v, f)
    # an isolated vertex gives 0 and changes nothing else
    v2 = np.concatenate([v, f32([[9, 9, 9]])])
    n2 = AR.normals_f32(v2, f)
    np.testing.assert_array_equal(n2[:-1], base)
    np.testing.assert_array_equal(n2[-1], f32([0, 0, 0]))
    # zero-area faces (a repeated index; three equal points) add nothing
    f3 = np.concatenate([f, np.array([[0, 0, 5], [4, 4, 4]], np.int32)])
    np.testing.assert_array_equal(AR.normals_f32(v, f3), base)
    # reversed winding negates, exactly (the same first corner: e2 x e1 = -(e1 x e2) term by term)
    np.testing.assert_array_equal(AR.normals_f32(v, f[:, [0, 2, 1]]), -base)
    np.testing.assert_allclose(AR.normals_f32(v, f[:, ::-1]), -base, rtol=0, atol=1e-6)
    # a face with an index of V or -1 is skipped whole
    f4 = np.concatenate([np.array([[0, 1, len(v)], [2, -1, 3]], np.int32), f])
    n4, census = AR.normals_f32(v, f4, return_census=True)
    np.testing.assert_array_equal(n4, base)
    assert census["out_of_range"] == 2 and census["used"] == len(f)
    assert np.abs(np.linalg.norm(base.astype(np.float64), axis=1) - 1).max() < 1e-7


@pytest.mark.parametrize("name", sorted(AC.NORMAL_CASES))
def test_normal_cases_agree_with_the_float64_rule(name):
    """Against mesh_render.vertex_normals.  Per face the float32 unit normal is off by at most 8 u (two edges, a cross
    product of two products and a difference each, the length, the division) and the quantisation by half of 2^-30; a vertex
    of valence deg sums deg of them, and normalising by |S| (the length of the float64 sum of unit normals) carries the error
    over: deg * (8 * 2^-24 + 2^-30) / |S|, doubled.  That count takes the cross product at face value: in a sliver the two
    products of a component cancel and their roundings grow by |e1| |e2| / |e1 x e2| = 1 / sin(angle).  The fan (5000
    triangles in a quarter circle) and the marched gyroid (marching tetrahedra cuts slivers) are such meshes: for them,
    and only for them, each face's 8 u is multiplied by its own 1 / sin.  Faces the float64 rule keeps but float32 calls
    degenerate (or the reverse) are not in these cases: the counts are compared."""
    from pegasus_amd.mesh_render import vertex_normals
    v, f = AC.normal_case(name)
    got, census = AC.normal_reference(name)
    for key in AC.NORMAL_CASES[name][1]:
        assert census[key] > 0, (key, census)
    V = len(v)
    ok = ((f >= 0) & (f < V)).all(axis=1)
    f = f[ok]
    v64 = v.astype(np.float64)
    fn = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
    length = np.linalg.norm(fn, axis=1)
    # a face whose float64 area is not 0 but tiny against its edges is where the two precisions may part: none here
    edge = np.maximum(np.linalg.norm(v64[f[:, 1]] - v64[f[:, 0]], axis=1), np.linalg.norm(v64[f[:, 2]] - v64[f[:, 0]], axis=1))
    assert int((length > 0).sum()) == census["used"]
    assert not ((length > 0) & (length < 1e-4 * edge * edge)).any()
    want = vertex_normals(v, f)
    unit = np.divide(fn, length[:, None], out=np.zeros_like(fn), where=length[:, None] > 0)
    S = np.zeros((V, 3))
    deg = np.zeros(V)
    for c in range(3):
        np.add.at(S, f[:, c], unit)
        np.add.at(deg, f[:, c], (length > 0).astype(np.float64))
    norm_S = np.linalg.norm(S, axis=1)
    seen = norm_S > 1e-6 * np.maximum(deg, 1)          # (sums that cancel to nothing have no direction to compare)
    bound = 2.0 * deg * (8 * 2.0 ** -24 + 2.0 ** -30) / np.maximum(norm_S, 1e-300) + 2.0 ** -24      # (+ the result's own rounding)
    if name in SLIVER_CASES:
        e1, e2 = np.linalg.norm(v64[f[:, 1]] - v64[f[:, 0]], axis=1), np.linalg.norm(v64[f[:, 2]] - v64[f[:, 0]], axis=1)
        amp = np.divide(e1 * e2, length, out=np.ones_like(length), where=length > 0)
        total = np.zeros(V)
        for c in range(3):
            np.add.at(total, f[:, c], np.where(length > 0, 8 * 2.0 ** -24 * amp + 2.0 ** -30, 0.0))
        bound = 2.0 * total / np.maximum(norm_S, 1e-300) + 2.0 ** -24
        print(f"{name}: largest 1 / sin of a face {float(amp.max()):.3g}")
    err = np.abs(got.astype(np.float64) - want).max(axis=1)
    print(f"{name}: worst error / bound {float((err[seen] / bound[seen]).max()) if seen.any() else 0:.3g}, "
          f"largest valence {int(deg.max()) if V else 0}")
    assert (err[seen] <= bound[seen]).all(), float((err[seen] / bound[seen]).max())
    np.testing.assert_array_equal(got[deg == 0], 0)


SLIVER_CASES = ("fan-5000-on-one-vertex", "gyroid-37x35x33")


# ---- colours: hand-worked answers -------------------------------------------------------------------------------------
IDENTITY = np.eye(4, dtype=f32).reshape(16)
FILL = (0.25, 0.5, 0.75)


def look_at_matrix(eye, target):
    """world_view_transform (transposed storage) of a camera at ``eye`` looking at ``target``: the target lands on the optical
    axis."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    M = np.eye(4)
    M[:3, :3] = R.T
    M[3, :3] = -R @ eye
    return M.astype(f32).reshape(16)


def flat_image(n_views, W, H, rgb, alpha=1.0, depth=1.0):
    """Views whose every pixel holds premultiplied ``alpha * rgb`` (one rgb per view), transmittance 1 - alpha and ``depth``."""
    rgb = np.asarray(rgb, np.float64).reshape(n_views, 3)
    color = np.broadcast_to((alpha * rgb)[:, :, None, None], (n_views, 3, H, W)).astype(f32).copy()
    return color, np.full((n_views, H, W), depth, f32), np.full((n_views, H, W), 1.0 - alpha, f32)


def scenario(name):
    """(arguments of the rule as a dict, expected colours [V,3], expected seen [V], tolerance).  A 5 x 5 image with
    tanfov = 2.5, so fx = fy = 1 and cx = cy = 2: the camera at the origin (identity transform) sees the point (a, b, 1) at
    pixel (2 + a, 2 + b)."""
    W = H = 5
    base = dict(vertices=f32([[0, 0, 1]]), normals=f32([[0, 0, -1]]), viewmats=[IDENTITY], tanfovx=[2.5], tanfovy=[2.5],
                campos=f32([[0, 0, 0]]), depth_tol=0.05, alpha_min=0.5, cos_min=0.3, fill=FILL)
    rgb = (0.2, 0.4, 0.6)
    color, depth, final_T = flat_image(1, W, H, [rgb], alpha=0.8)
    base.update(color=color, depth=depth, final_T=final_T)
    seen_fill = (np.asarray([FILL], f32), [0], 0.0)
    if name == "fronto-parallel":                  # colour = pixel / alpha
        return base, np.asarray([rgb]), [1], 1e-6
    if name == "two-views-0-and-60-degrees":       # weights cos^2 = 1 and 0.25
        eye2 = np.array([0.0, 0.0, 1.0]) + 1.5 * np.array([math.sin(math.radians(60)), 0.0, -math.cos(math.radians(60))])
        c2 = (0.8, 0.1, 0.3)
        color, depth, final_T = flat_image(2, W, H, [rgb, c2], alpha=0.8, depth=1.0)
        depth[1] = 1.5
        base.update(viewmats=[IDENTITY, look_at_matrix(eye2, (0, 0, 1))], tanfovx=[2.5, 2.5], tanfovy=[2.5, 2.5],
                    campos=f32([[0, 0, 0], eye2]), color=color, depth=depth, final_T=final_T)
        return base, (np.asarray([rgb]) + 0.25 * np.asarray([c2])) / 1.25, [2], 1e-6
    if name == "depth-nearer-by-twice-the-tolerance":      # something in front of the vertex: occluded
        base.update(depth=np.full((1, H, W), 1.0 - 2 * 0.05, f32))
        return (base,) + seen_fill
    if name == "depth-farther-by-twice-the-tolerance":     # the view's surface lies behind the vertex
        base.update(depth=np.full((1, H, W), 1.0 + 2 * 0.05, f32))
        return (base,) + seen_fill
    if name == "depth-at-the-tolerance":           # |d| == depth_tol counts: 1.0625 - 1 and 0.0625 are exact
        base.update(depth=np.full((1, H, W), 1.0625, f32), depth_tol=0.0625)
        return base, np.asarray([rgb]), [1], 1e-6
    if name == "see-through-pixel":
        color, depth, final_T = flat_image(1, W, H, [rgb], alpha=0.4)
        base.update(color=color, depth=depth, final_T=final_T)
        return (base,) + seen_fill
    if name == "back-facing":
        base.update(normals=f32([[0, 0, 1]]))
        return (base,) + seen_fill
    if name == "cosine-equal-to-cos_min":          # n . e / |e| = 0.5 exactly, and 0.5 > 0.5 is false
        base.update(normals=f32([[0, 0, -0.5]]), cos_min=0.5)
        return (base,) + seen_fill
    if name == "cosine-just-above-cos_min":
        base.update(normals=f32([[0, 0, -0.5]]), cos_min=float(np.nextafter(f32(0.5), f32(0))))
        return base, np.asarray([rgb]), [1], 1e-6
    if name == "at-the-near-plane":                # z == NEAR_Z is skipped, the next float is not
        z0 = float(AR.NEAR_Z)
        z1 = float(np.nextafter(AR.NEAR_Z, f32(1)))
        base.update(vertices=f32([[0, 0, z0], [0, 0, z1], [0, 0, -1]]), normals=f32([[0, 0, -1]] * 3),
                    depth=np.full((1, H, W), z1, f32))
        return base, np.asarray([FILL, rgb, FILL]), [0, 1, 0], 1e-6
    if name == "one-pixel-outside-each-edge":      # pixel columns -1 and 5, rows -1 and 5; 0 and 4 are inside
        pts = [[-3, 0, 1], [3, 0, 1], [0, -3, 1], [0, 3, 1], [-2, 0, 1], [2, 0, 1], [0, -2, 1], [0, 2, 1]]
        base.update(vertices=f32(pts), normals=None)
        return base, np.asarray([FILL] * 4 + [rgb] * 4), [0, 0, 0, 0, 1, 1, 1, 1], 1e-6
    if name == "nearest-pixel":                    # u = 2.6 is pixel 3, not 2: every pixel column has its own colour
        color = np.zeros((1, 3, H, W), f32)
        color[0, 0] = np.arange(W, dtype=f32)[None, :] * f32(0.125)
        color[0, 1] = np.arange(H, dtype=f32)[:, None] * f32(0.125)
        base.update(vertices=f32([[0.6, -0.6, 1]]), normals=None, color=color, final_T=np.zeros((1, H, W), f32))
        return base, np.asarray([[3 * 0.125, 1 * 0.125, 0.0]]), [1], 1e-7
    if name == "null-normals":                     # no angle test and weight 1: the back-facing vertex is coloured
        base.update(normals=None)
        return base, np.asarray([rgb]), [1], 1e-6
    if name == "clamped-above-one":
        color, depth, final_T = flat_image(1, W, H, [(1.5, 0.9, -0.5)], alpha=0.8)
        base.update(color=color, depth=depth, final_T=final_T)
        return base, np.asarray([[1.0, 0.9, 0.0]]), [1], 1e-6
    raise KeyError(name)


SCENARIOS = ("fronto-parallel", "two-views-0-and-60-degrees", "depth-nearer-by-twice-the-tolerance",
             "depth-farther-by-twice-the-tolerance", "depth-at-the-tolerance", "see-through-pixel", "back-facing",
             "cosine-equal-to-cos_min", "cosine-just-above-cos_min", "at-the-near-plane", "one-pixel-outside-each-edge",
             "nearest-pixel", "null-normals", "clamped-above-one")


def agrees(result, want, want_seen, tol):
    colors, seen = result
    return bool(np.array_equal(seen, np.asarray(want_seen)) and np.abs(colors.astype(np.float64) - want).max() <= tol)


@pytest.mark.parametrize("name", SCENARIOS)
def test_colour_rule_gives_the_hand_worked_answer(name):
    args, want, want_seen, tol = scenario(name)
    got = AR.colors_f32(**args)
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert agrees(got, want, want_seen, tol), (got, want, want_seen)
    oracle, oracle_seen, masked, _tol = AR.colors_oracle(**args)
    if not masked.any():                           # (the cases that sit exactly on a threshold are masked, as they should be)
        assert agrees((oracle, oracle_seen), want, want_seen, max(tol, 1e-12))


def scalar_rule(args, mutant=None):
    """The colour rule once more, one vertex and one view at a time in Python floats, with one deliberate mistake per
    ``mutant``.  Without a mutant it gives the hand-worked answers too."""
    a = args
    n_views, H, W = a["depth"].shape
    out, seen_all = [], []
    for i, p in enumerate(np.asarray(a["vertices"], np.float64)):
        acc, wsum, seen = np.zeros(3), 0.0, 0
        for k in range(n_views):
            M = np.asarray(a["viewmats"][k], np.float64).reshape(4, 4)
            x, y, z = (np.append(p, 1.0) @ M)[:3]
            if z <= float(AR.NEAR_Z):
                continue
            fx, fy = W / (2 * a["tanfovx"][k]), H / (2 * a["tanfovy"][k])
            u, v = x / z * fx + (W - 1) / 2, y / z * fy + (H - 1) / 2
            iu, iv = (math.floor(u), math.floor(v)) if mutant == "floor-u" else (math.floor(u + 0.5), math.floor(v + 0.5))
            if not (0 <= iu < W and 0 <= iv < H):
                continue
            alpha = 1.0 - float(a["final_T"][k, iv, iu])
            if alpha < a["alpha_min"]:
                continue
            d = float(a["depth"][k, iv, iu]) - z
            if mutant == "one-sided-occluded-only":
                if d < -a["depth_tol"]:
                    continue
            elif mutant == "one-sided-behind-only":
                if d > a["depth_tol"]:
                    continue
            elif not abs(d) <= a["depth_tol"]:
                continue
            w = 1.0
            if a["normals"] is not None and mutant != "normal-ignored":
                e = np.asarray(a["campos"][k], np.float64) - p
                cs = float(np.asarray(a["normals"][i], np.float64) @ e / np.linalg.norm(e))
                if not cs > a["cos_min"]:
                    continue
                w = cs if mutant == "weight-cs" else cs * cs
            value = a["color"][k, :, iv, iu].astype(np.float64)
            acc += w * (value if mutant == "no-division-by-alpha" else value / alpha)
            wsum += 1.0 if mutant == "wsum-unweighted" else w
            seen += 1
        out.append(np.clip(acc / wsum, 0, 1) if seen else np.asarray(a["fill"], np.float64))
        seen_all.append(seen)
    return np.asarray(out), np.asarray(seen_all)


MUTANTS = ("no-division-by-alpha", "weight-cs", "one-sided-occluded-only", "one-sided-behind-only", "normal-ignored", "floor-u",
           "wsum-unweighted")


def test_the_scalar_rule_gives_the_hand_worked_answers_too():
    for name in SCENARIOS:
        args, want, want_seen, tol = scenario(name)
        assert agrees(scalar_rule(args), want, want_seen, max(tol, 1e-6)), name


@pytest.mark.parametrize("mutant", MUTANTS)
def test_hand_worked_answers_reject_the_mutant(mutant):
    rejected = [name for name in SCENARIOS
                if not agrees(scalar_rule(scenario(name)[0], mutant), *scenario(name)[1:3], max(scenario(name)[3], 1e-6))]
    print(mutant, "rejected by", rejected)
    assert rejected, mutant


# ---- the analytic sphere ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere-162-cos0.3", "sphere-162-cos0.5", "sphere-642-cos0.3", "sphere-642-cos0.5"])
def test_analytic_sphere_on_the_host(name):
    colors, seen, _census = AC.color_reference(name)
    err, bound = AC.check_sphere(name, colors, seen)
    assert bound < 0.1 and err < 0.7 / 10


# ---- the device cases, on the host ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AC.COLOR_CASES))
def test_colour_cases_reach_their_branches_and_agree_with_the_oracle(name):
    c = AC.color_case(name)
    _colors, _seen, census = AC.color_reference(name)
    for key in c.reaches:
        assert census[key] > 0, (key, census)
    assert census["pairs"] == len(c.vertices) * len(c.raw)
    AC.check_colors_against_oracle(name)


def test_case_shapes_are_the_ones_the_kernels_change_path_at():
    assert [len(AC.color_case(n).vertices) for n in ("V255", "V256", "V257")] == [255, 256, 257]
    assert len(AC.color_case("views-255").raw) == 255 and len(AC.color_case("views-256").raw) == 256
    assert AC.color_case("views-256").depth.shape[1:] == (17, 23)
    assert [AC.color_case(n).depth.shape[1:] for n in ("image-1x1", "image-1x40", "image-40x1")] == [(1, 1), (40, 1), (1, 40)]
    assert len(AC.icosphere(2)[0]) == 162 and len(AC.icosphere(3)[0]) == 642
    v, f = AC.normal_case("fan-5000-on-one-vertex")
    assert (f == 0).any(axis=1).all() and len(f) == 5000
    assert np.isnan(AC.color_case("depth-nan").depth).any() and np.isinf(AC.color_case("depth-inf").depth).any()


# ---- host plumbing of pegasus_amd.mesh ------------------------------------------------------------------------------------
def test_mesh_carries_its_attributes():
    from pegasus_amd.mesh import Mesh
    v, f = AC.icosphere(1)
    plain = Mesh(v, f)
    assert plain.normals is None and plain.colors is None
    v2, f2 = AC.icosphere(0, 0.1, (5, 0, 0))
    both_v, both_f = np.concatenate([v, v2]), np.concatenate([f, f2 + len(v)])
    n = AR.normals_f32(both_v, both_f)
    col = np.random.default_rng(0).uniform(size=both_v.shape).astype(f32)
    m = Mesh(both_v, both_f, normals=n, colors=col)
    s = m.scaled(1000.0)
    assert s.normals is n and s.colors is col and s.faces is m.faces
    big = m.largest_component()
    assert len(big.vertices) == len(v)
    np.testing.assert_array_equal(big.normals, n[:len(v)])
    np.testing.assert_array_equal(big.colors, col[:len(v)])
    assert Mesh(both_v, both_f).largest_component().normals is None


def test_fill_unseen_spreads_from_coloured_neighbours():
    from pegasus_amd.mesh import Mesh, fill_unseen
    # a strip of triangles 0-1-2, 1-2-3, 2-3-4, 3-4-5 and an unconnected vertex 6
    v = np.zeros((7, 3), f32)
    f = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 5, 4]], np.int32)
    colors = np.zeros((7, 3), f32)
    colors[0], colors[1] = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    colors[6] = (0.5, 0.5, 0.5)
    seen = np.array([1, 2, 0, 0, 0, 0, 0])
    out = fill_unseen(Mesh(v, f), colors, seen)
    assert out.dtype == np.float32
    np.testing.assert_array_equal(out[:2], colors[:2])
    np.testing.assert_allclose(out[2], [0.5, 0.5, 0.0])              # round 1: neighbours 0 and 1 (3 and 4 are not coloured yet)
    np.testing.assert_allclose(out[3], [0.0, 1.0, 0.0])              # round 1: neighbour 1 alone
    np.testing.assert_allclose(out[4], [0.25, 0.75, 0.0])            # round 2: the mean of 2 and 3
    np.testing.assert_allclose(out[5], [0.0, 1.0, 0.0])              # round 2 as well: of 3 and 4 only 3 is coloured by then
    np.testing.assert_array_equal(out[6], colors[6])                 # unreachable: nothing changes, the loop ends
    np.testing.assert_array_equal(fill_unseen(Mesh(v, f), colors, np.zeros(7, int)), colors)
    np.testing.assert_array_equal(fill_unseen(Mesh(v, f), colors, np.ones(7, int)), colors)


def test_write_ply_with_and_without_attributes(tmp_path):
    from pegasus_amd.mesh import Mesh, write_ply
    from pegasus_amd.ply_io import read_ply_model, write_ply_mesh
    v, f = AC.icosphere(1, 0.05)
    write_ply(tmp_path / "plain.ply", Mesh(v, f), scale=1000.0)
    write_ply_mesh(tmp_path / "before.ply", (v.astype(np.float64) * 1000.0).astype(f32), f)
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "before.ply").read_bytes()
    assert b"nx" not in (tmp_path / "plain.ply").read_bytes()[:400]
    n = AR.normals_f32(v, f)
    col = np.linspace(0.0, 1.0, v.size, dtype=np.float64).reshape(v.shape).astype(f32)
    write_ply(tmp_path / "full.ply", Mesh(v, f, normals=n, colors=col), scale=1000.0)
    header = (tmp_path / "full.ply").read_bytes().split(b"end_header")[0].decode()
    names = [line.split()[-1] for line in header.splitlines() if line.startswith("property") and "list" not in line]
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert "property uchar red" in header and "property float nx" in header
    model = read_ply_model(tmp_path / "full.ply")
    np.testing.assert_array_equal(model["pts"], (v.astype(np.float64) * 1000.0).astype(f32))
    np.testing.assert_array_equal(model["normals"], n)
    assert model["colors"].dtype == np.uint8
    np.testing.assert_array_equal(model["colors"], np.rint(255.0 * col.astype(np.float64)).astype(np.uint8))
    np.testing.assert_array_equal(model["faces"], f)


def test_degree_zero_model_survives_save_and_load(tmp_path):
    """The command line reads the model from its PLY: a model without f_rest_ columns (SH degree 0) loads."""
    from pegasus_amd.gaussian_model import GaussianModel
    rng = np.random.default_rng(4)
    n = 17
    arrays = [rng.normal(size=s).astype(f32) for s in ((n, 3), (n, 1, 3), (n, 0, 3), (n, 1), (n, 3), (n, 4))]
    model = GaussianModel.from_arrays(*arrays, sh_degree=0, device="cpu")
    model.save_ply(tmp_path / "point_cloud.ply")
    back = GaussianModel(0, "cpu")
    back.load_ply(tmp_path / "point_cloud.ply")
    assert tuple(back._features_rest.shape) == (n, 0, 3) and back.active_sh_degree == 0
    np.testing.assert_array_equal(back._features_dc.numpy(), arrays[1])
    np.testing.assert_array_equal(back._xyz.numpy(), arrays[0])
