"""The environment field without a device: the reference's rule (tests/environment_reference.py) against the exact analytic
distance within the bound derived there, its zero set against mesh_reference's marching vertices, the ground's contact words of
the float64 reference alone (the exemption budget of the GPU test, checked here first), the files and the command lines."""
import json

import numpy as np
import pytest

import collision_reference as CR
import dynamics_cases as DC
import dynamics_reference as DR
import environment_cases as EC
import environment_reference as ER
import mesh_reference as MR

SHAPE = (24, 24, 24)


def _border_distance(g):
    """[nz,ny,nx]: every grid point's distance to the grid's box, in voxels."""
    k, j, i = np.meshgrid(np.arange(g.nz), np.arange(g.ny), np.arange(g.nx), indexing="ij")
    return np.minimum.reduce([i, g.nx - 1 - i, j, g.ny - 1 - j, k, g.nz - 1 - k]).astype(np.float64)


@pytest.mark.parametrize("name", EC.ANALYTIC)
def test_the_rule_stays_within_its_derived_bound_of_the_exact_distance(name):
    """-0.5 <= (|phi| - |d|) / voxel <= sqrt(3) - 0.5 (environment_reference's docstring), over every point whose nearest grid
    point of the other sign the derivation can name inside the grid: |d| + sqrt(3) voxels short of the grid's box."""
    g = EC.field_grid(SHAPE)
    d = EC.exact_distance(name, g) / g.voxel
    _, _, phi = EC.reference_field(name, SHAPE)
    err = (np.abs(phi) / g.voxel - np.abs(d))
    assert ((phi < 0) == (d < 0)).all()
    held = np.abs(d) + 3.0 ** 0.5 < _border_distance(g)
    is_band, _ = ER.band(EC.volume(name, SHAPE))
    low, high = ER.rule_bounds()
    near = held & (np.abs(d) < 2.0)
    print(f"\n[environment] {name}: phi - d in [{err[held].min():+.3f}, {err[held].max():+.3f}] voxels over {int(held.sum())} points; "
          f"|d| < 2: [{err[near].min():+.3f}, {err[near].max():+.3f}]; band points: [{err[held & is_band].min():+.3f}, "
          f"{err[held & is_band].max():+.3f}]")
    assert held.sum() >= 2000 and (held & is_band).sum() >= 100
    assert err[held].min() >= low - 1e-9 and err[held].max() <= high + 1e-9
    assert err[held & is_band].min() >= -1e-6 and err[held & is_band].max() < 1.0        # d <= phi <= 1 on the band
    # how steep the field is along an axis: recorded in DESIGN.md section 25, held here below two voxels per voxel
    slope = max(float(np.abs(np.diff(phi, axis=a)).max()) for a in range(3)) / g.voxel
    print(f"[environment] {name}: largest difference between axis neighbours {slope:.3f} voxels")
    assert slope < 2.0


@pytest.mark.parametrize("name", EC.ANALYTIC + ("random",))
def test_the_band_puts_the_zero_where_marching_puts_its_vertex(name):
    """Along the grid axis on which a band point takes its beta, the point phi away from it is the marching vertex of that edge."""
    from scipy.spatial import cKDTree
    g = EC.field_grid(SHAPE)
    t = EC.volume(name, SHAPE)
    vertices, _ = MR.march_reference(t, g, sparse=True)
    tree = cKDTree(vertices.astype(np.float64))
    is_band, beta = ER.band(t)
    points = CR.grid_points(g)
    ins = ER.inside(t)
    worst, n = 0.0, 0
    a = np.where(np.isfinite(t), np.abs(t.astype(np.float64)), 1.0)
    for axis, step in ER.NEIGHBOURS:
        ax = 2 - axis
        nb = np.roll(a, -step, axis=ax)
        other = np.roll(ins, -step, axis=ax) != ins
        idx = np.arange(t.shape[ax])
        valid = (idx + step >= 0) & (idx + step < t.shape[ax])
        shape = [1, 1, 1]
        shape[ax] = -1
        with np.errstate(divide="ignore", invalid="ignore"):
            here = is_band & other & valid.reshape(shape) & (a / (a + nb) == beta)
        e = np.zeros(3)
        e[axis] = step
        zero = points[here] + (beta[here] * g.voxel)[:, None] * e
        dist, _ = tree.query(zero)
        worst, n = max(worst, float(dist.max()) if len(dist) else 0.0), n + len(dist)
    print(f"\n[environment] {name}: {n} band edges, farthest marching vertex {worst / g.voxel:.2e} voxels")
    assert n >= int(is_band.sum()) and worst <= 1e-5 * g.voxel


def test_special_volumes_follow_the_rule():
    shape = (5, 4, 3)
    d2, phi, _ = EC.reference_field("all_inside", shape)
    assert (d2 == ER.NONE).all() and (phi == -np.float32(EC.VOXEL) * np.float32(12)).all()
    d2, phi, _ = EC.reference_field("all_outside", shape)
    assert (d2 == ER.NONE).all() and (phi == np.float32(EC.VOXEL) * np.float32(12)).all()
    d2, phi, _ = EC.reference_field("corner", shape)
    assert d2[0, 0, 0] == 1 and d2[2, 3, 4] == 16 + 9 + 4 and phi[0, 0, 0] == -np.float32(EC.VOXEL) * (np.float32(0.25) / np.float32(1.25))
    assert phi[0, 0, 1] == np.float32(EC.VOXEL) * (np.float32(1.0) / np.float32(1.25))                 # a band point
    assert phi[2, 3, 4] == np.float32(EC.VOXEL) * (np.sqrt(np.float32(29)) - np.float32(0.5))
    t = EC.volume("nan_and_zero", (17, 9, 6))
    flat = t.reshape(-1)
    k_nan, k_zero = len(flat) // 3, (2 * len(flat)) // 3
    assert np.isnan(flat[k_nan]) and flat[k_zero] == 0.0
    d2, phi, _ = EC.reference_field("nan_and_zero", (17, 9, 6))
    assert np.isfinite(phi).all() and phi.reshape(-1)[k_nan] > 0 and phi.reshape(-1)[k_zero] >= 0      # both are outside
    assert (d2 >= 1).all()
    # float32 and float64 statements agree to float32's precision
    for content, s in EC.field_cases():
        _, p32, p64 = EC.reference_field(content, s)
        assert np.abs(p32 - p64).max() <= 8 * CR.U * np.abs(p64).max(), (content, s)


def test_the_ground_words_of_the_reference_alone_stay_within_the_exemption_budget():
    """The worlds of the GPU test, on the reference's own field: few exact ties, and the sphere early-out hides no candidate."""
    types = [DC.ref_type(EC.BODY)]
    ground = EC.ground_reference()
    p = EC.ground_params(types)
    states = EC.contact_states()
    n_words = n_exempt = n_filled = 0
    for w, state in enumerate(states):
        with ER.ground_rule(ground):
            words, exempt = DC.word_exemptions(types, [0], state, p)
        with ER.ground_rule(ground, sphere=False):
            full = DR.world_words(types, [0], state, p)
        assert words == full, w                                          # every candidate found without the sphere test
        n_words += exempt.size
        n_exempt += int(exempt.sum())
        n_filled += sum(x != DR.EMPTY for x in words[0])
    print(f"\n[environment] ground words of the reference: {n_filled} filled, {n_exempt}/{n_words} exempt")
    assert n_filled >= 7 * (len(states) - 2) and n_exempt <= DC.MAX_WORD_EXEMPT * n_words
    with ER.ground_rule(ground):
        assert all(x == DR.EMPTY for x in DR.world_words(types, [0], states[0], p)[0])                 # in the air


def test_npz_round_trip_is_host_only(tmp_path):
    """save / load on the arrays alone: the file holds the float32 field, the grid and the friction."""
    field = EC.z_field()
    path = tmp_path / "sub" / "env.npz"
    g = EC.ground_grid()
    path.parent.mkdir()
    with open(path, "wb") as f:
        np.savez_compressed(f, field=field, shape=np.array([g.nx, g.ny, g.nz], np.int32), origin=g.origin, voxel=np.float64(g.voxel),
                            friction=np.float64(0.25))
    with np.load(path) as z:
        assert sorted(z.files) == ["field", "friction", "origin", "shape", "voxel"]
        assert z["field"].dtype == np.float32 and z["field"].tobytes() == field.tobytes() and tuple(z["shape"]) == (24, 24, 16)
    from pegasus_amd import environment as ENV
    with pytest.raises(RuntimeError, match="HIP device"):
        ENV.EnvironmentField.load(path, device="cpu")


def test_default_document_of_write_trajectory_is_unchanged(tmp_path):
    from pegasus_amd import dynamics as DYN
    traj = np.zeros((2, 1, 7))
    traj[:, 0, 6], traj[:, 0, 2] = 1.0, (0.5, 0.25)
    a = DYN.write_trajectory(tmp_path / "a.json", ["obj_000001"], ["Thing"], [1], traj, [[0.1, 0.0, 0.2]])
    expected = {"asset_infos": {"environment": {"plane": {"bullet_id": [0], "class_name": "plane"}},
                                "object": {"obj_000001": {"bullet_id": [1], "center_of_mass": [0.1, 0.0, 0.2], "class_name": "Thing",
                                                          "object_ID": 1}}},
                "trajectory": {"0": {"0": {"t": [0.0, 0.0, 0.0], "q": [0.0, 0.0, 0.0, 1.0]}, "1": {"t": [0.0, 0.0, 0.0], "q": [0.0, 0.0, 0.0, 1.0]}},
                               "1": {"0": {"t": [0.0, 0.0, 0.5], "q": [0.0, 0.0, 0.0, 1.0]}, "1": {"t": [0.0, 0.0, 0.25], "q": [0.0, 0.0, 0.0, 1.0]}}}}
    assert (tmp_path / "a.json").read_bytes() == json.dumps(expected).encode() and a == expected
    b = DYN.write_trajectory(tmp_path / "b.json", ["obj_000001"], ["Thing"], [1], traj, [[0.1, 0.0, 0.2]], environment="kitchen")
    assert b["asset_infos"]["environment"] == {"kitchen": {"bullet_id": [0], "class_name": "environment"}}
    assert b["trajectory"] == a["trajectory"] and b["asset_infos"]["object"] == a["asset_infos"]["object"]


def test_grids_bounds_and_subsampling():
    from pegasus_amd import environment as ENV
    lo, hi = ENV.default_bounds()
    assert lo.tolist() == [-1.0, -1.0, -0.04] and hi.tolist() == [1.0, 1.0, 1.0]
    g = ENV.bounds_grid(lo, hi, 0.01)
    assert (g.nx, g.ny, g.nz) == (201, 201, 105) and g.origin == (-1.0, -1.0, -0.04) and g.voxel == 0.01
    assert ENV.bounds_grid((0, 0, 0), (0.3, 0.1, 0.05), 0.1).shape == (2, 2, 4)
    for bad in (((0, 0, 0), (0, 1, 1), 0.1), ((0, 0, 0), (1, 1, 1), 0.0), ((0, 0, 0), (1, 1, float("nan")), 0.1), ((0, 0, 0), (11, 1, 1), 0.01)):
        with pytest.raises(ValueError):
            ENV.bounds_grid(*bad)
    assert ENV.subsample(range(10), 256) == list(range(10)) and ENV.subsample(range(1000), 256)[0] == 0
    picked = ENV.subsample(range(1000), 256)
    assert len(picked) == 256 and picked[-1] == 999 and len(set(picked)) == 256 and picked == sorted(picked)
    assert ENV.subsample(range(5), 1) == [0] and ENV.subsample(range(5), 2) == [0, 4]
    with pytest.raises(RuntimeError, match="HIP device"):
        ENV.EnvironmentField(np.zeros((2, 2, 2), np.float32), ENV.Grid(2, 2, 2, (0, 0, 0), 1.0))


def test_command_line_parsers():
    from pegasus_amd import collision as COL, dynamics as DYN, environment as ENV
    a = ENV._parser().parse_args(["-m", "model", "--out", "env.npz"])
    assert (a.model_path, a.iteration, a.out, a.bounds, a.plane_size, a.height, a.voxel, a.views, a.image_size, a.mesh) == \
        ("model", -1, "env.npz", None, 2.0, 1.0, 0.01, 128, 512, None)
    a = ENV._parser().parse_args(["-m", "model", "--iteration", "7000", "--out", "e.npz", "--bounds", "-1", "-2", "0", "1", "2", "0.5",
                                  "--voxel", "0.02", "--views", "64", "--image_size", "256", "--mesh", "env.ply"])
    assert a.bounds == [-1.0, -2.0, 0.0, 1.0, 2.0, 0.5] and (a.iteration, a.voxel, a.views, a.image_size, a.mesh) == (7000, 0.02, 64, 256, "env.ply")
    with pytest.raises(SystemExit):
        ENV._parser().parse_args(["--out", "env.npz"])                   # no model
    with pytest.raises(SystemExit):
        ENV._parser().parse_args(["-m", "model", "--out", "e.npz", "--bounds", "0", "0", "0"])
    with pytest.raises(SystemExit):
        ENV.main(["-m", "model", "--out", "e.npz", "--views", "257"])
    d = DYN._parser().parse_args(["--models", "m", "--objects", "1", "2", "--out", "o"])
    assert d.environment is None
    d = DYN._parser().parse_args(["--models", "m", "--objects", "1", "--out", "o", "--environment", "env.npz"])
    assert d.environment == "env.npz"
    c = COL._parser().parse_args(["--models", "m", "--out", "s.json"])
    assert c.environment is None
    c = COL._parser().parse_args(["--models", "m", "--check", "data", "--environment", "env.npz"])
    assert c.environment == "env.npz" and c.check == "data"


def test_engine_takes_the_environment_instance_as_its_ground():
    import types as pytypes
    from pegasus_amd import dynamics as DYN
    eng = DYN.Engine({}, "x.json")
    eng.add_object(pytypes.SimpleNamespace(TYPE="environment", urdf_file_name="plane.urdf"))
    assert eng.ground is None
    marker = object()
    eng.add_object(pytypes.SimpleNamespace(TYPE="environment", urdf_file_name="kitchen.urdf", field=marker))
    assert eng.ground is marker and eng.environment_name == "kitchen"
    lo, hi = np.array([-1.0, -1.0, 0.0]), np.array([1.0, 1.0, 2.0])
    ground = pytypes.SimpleNamespace(box=lambda: (lo, hi))
    poses = np.array([[0, 0, 1, 0, 0, 0, 1], [1.5, 0, 1, 0, 0, 0, 1], [0, 0, -0.1, 0, 0, 0, 1.0]])
    assert DYN.outside_ground(ground, poses).tolist() == [False, True, True]
