"""pgr_sdf_from_tsdf, the *_ground entries and pegasus_amd.environment on the GPU against tests/environment_reference.py: the
field per point and bit for bit, the ground's contact words and one step by the scheme and bounds of DESIGN.md section 24, drops
onto a flat field, onto a table and beside it, determinism, placement by sweeps, and the field of a rendered Gaussian scene.

One step: the asserted bounds are section 24's, unchanged: 2.96e-4 in v and omega, 4.04e-7 in x and q."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import collision_cases as CC
import collision_reference as CR
import dynamics_cases as DC
import dynamics_reference as DR
import environment_cases as EC
import environment_reference as ER
import mesh_cases as MC
import mesh_reference as MR

pytestmark = pytest.mark.gpu
STEP_VELOCITY_BOUND, STEP_POSE_BOUND = 2.96e-4, 4.04e-7


def package_grid(g):
    from pegasus_amd.mesh import Grid
    return Grid(g.nx, g.ny, g.nz, tuple(float(x) for x in g.origin), g.voxel)


# ---- 1: the field -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content,shape", EC.field_cases(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_field_equals_the_reference_bit_for_bit(gpu_device, content, shape):
    import torch
    from pegasus_amd import environment as ENV
    grid = package_grid(EC.field_grid(shape))
    t = torch.from_numpy(EC.volume(content, shape).copy()).to(gpu_device)
    sdf, dist2 = ENV.sdf_from_tsdf(t, grid, want_dist2=True)
    again, dist2_again = ENV.sdf_from_tsdf(t, grid, want_dist2=True)
    alone = ENV.sdf_from_tsdf(t, grid)
    want_d2, want_phi, _ = EC.reference_field(content, shape)
    sdf, dist2 = sdf.cpu().numpy(), dist2.cpu().numpy()
    assert dist2.dtype == np.int32 and np.array_equal(dist2.astype(np.int64), want_d2)
    assert sdf.dtype == np.float32 and sdf.tobytes() == want_phi.tobytes(), int((sdf != want_phi).sum())
    assert again.cpu().numpy().tobytes() == sdf.tobytes() and dist2_again.cpu().numpy().tobytes() == dist2.tobytes()
    assert alone.cpu().numpy().tobytes() == sdf.tobytes()
    assert np.array_equal(t.cpu().numpy(), EC.volume(content, shape), equal_nan=True)                  # the volume is read only


# ---- the worlds ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rigid(name=EC.BODY):
    from pegasus_amd import collision as COL, dynamics as DYN
    from pegasus_amd.mesh import Mesh
    m = Mesh(*DC.mesh(name))
    body = COL.CollisionBody(m, COL.MeshSDF.from_mesh(m, resolution=DC.RESOLUTION), shell=DC.shell(name))
    return DYN.RigidBody.from_collision(body, mass=1.0, friction=0.5)


@functools.lru_cache(maxsize=None)
def ref_type(name=EC.BODY):
    """The reference's type on the DEVICE's field of that body, read back."""
    b = rigid(name).body
    g = b.sdf.grid
    return DC.ref_type(name, 0.5, field=b.sdf.field.cpu().numpy().astype(np.float64), grid=CR.RefGrid(g.nx, g.ny, g.nz, g.origin, g.voxel))


@functools.lru_cache(maxsize=None)
def ground(kind="table"):
    """(the package's EnvironmentField, the reference's ground on the DEVICE's field, read back)."""
    import torch
    from pegasus_amd import environment as ENV
    grid = package_grid(EC.ground_grid())
    if kind == "z":
        env = ENV.EnvironmentField(torch.from_numpy(EC.z_field().copy()).cuda(), grid, EC.GROUND_FRICTION)
    else:
        env = ENV.EnvironmentField.from_tsdf(torch.from_numpy(EC.ground_volume(kind).copy()).cuda(), grid, EC.GROUND_FRICTION)
    return env, ER.RefGround(env.field.cpu().numpy().astype(np.float64), EC.ground_grid(), EC.GROUND_FRICTION)


def host_words(words):
    return words.cpu().numpy().view(np.uint64)


def test_ground_field_is_the_reference_and_names_the_table(gpu_device):
    env, ref = ground()
    assert env.field.cpu().numpy().tobytes() == ER.phi32(EC.ground_volume(), EC.GROUND_VOXEL).tobytes()
    s = env.struct()
    assert s.sdf == env.field.data_ptr() and abs(s.friction - 0.5) < 1e-7 and (s.grid.nx, s.grid.ny, s.grid.nz) == EC.GROUND_SHAPE
    import torch
    pts = torch.tensor([[-0.5, 0.0, 0.55], [0.8, 0.0, 0.0], [-0.5, 0.0, 0.3], [0.8, 0.0, 0.5]], device="cuda")
    phi, grad = env.signed_distance(pts, gradient=True)
    phi, grad = phi.cpu().numpy(), grad.cpu().numpy()
    assert abs(phi[0]) < 1e-6 and abs(phi[1]) < 1e-6 and phi[2] < -0.1 and phi[3] > 0.3               # the band puts the zero exactly
    assert np.allclose(grad[:2], [[0, 0, 1], [0, 0, 1]], atol=1e-5)
    assert env.top_under((-0.6, -0.1), (-0.4, 0.1)) == 0.4375 + 0.0 and env.top_under((0.7, -0.1), (0.9, 0.1)) == -0.0625


# ---- 2: contact words against the ground --------------------------------------------------------------------------------------
def test_ground_contact_words_against_the_reference_on_the_device_fields(gpu_device):
    from pegasus_amd import dynamics as DYN
    from pegasus_amd.collision import decode_words
    env, ref = ground()
    bodies, types = [rigid()], [ref_type()]
    states = EC.contact_states()
    p = EC.ground_params(types)
    S = len(states)
    words = host_words(DYN.contacts(bodies, [[0]] * S, states, DC.package_params(p), ground=env))
    assert words.shape == (S, 1, 7)
    assert words.tobytes() == host_words(DYN.contacts(bodies, [[0]] * S, states, DC.package_params(p), ground=env)).tobytes()
    value, index = decode_words(words)
    n_exempt = n_words = n_compared = 0
    worst = 0.0
    for w in range(S):
        with ER.ground_rule(ref):
            ref_words, exempt = DC.word_exemptions(types, [0], states[w], p)
            _, info = DR.world_words(types, [0], states[w], p, detail=True)
        with ER.ground_rule(ref, sphere=False):                         # the early-out switched off in the reference
            assert DR.world_words(types, [0], states[w], p) == ref_words, w
        n_words += exempt.size
        n_exempt += int(exempt.sum())
        for j in range(7):
            if exempt[0, j]:
                continue
            if ref_words[0][j] == DR.EMPTY:
                assert int(words[w, 0, j]) == DR.EMPTY, (w, j)
                continue
            i = ref_words[0][j] & 0xFFFFFFFF
            assert index[w, 0, j] == i, (w, j, int(index[w, 0, j]), i)
            err, bound = abs(float(value[w, 0, j]) - info[0]["values"][i, j]), info[0]["bound"][i] + 4 * CR.U * abs(info[0]["values"][i, j])
            assert err <= bound, (w, j, err, bound)
            worst = max(worst, err / bound)
            n_compared += 1
    print(f"\n[environment] ground words: {n_compared} compared, {n_exempt}/{n_words} exempt, max error/bound {worst:.4f}")
    assert n_exempt <= DC.MAX_WORD_EXEMPT * n_words and n_compared >= 50
    assert (words[0] == np.uint64(DR.EMPTY)).all()                      # in the air: out of sphere range
    # through the plane entry the same states see the plane z = 0, not the table
    plane_words = host_words(DYN.contacts(bodies, [[0]] * S, states, DC.package_params(p)))
    assert (plane_words[1] == np.uint64(DR.EMPTY)).all() and (words[1] != np.uint64(DR.EMPTY)).all()


# ---- 3: one step --------------------------------------------------------------------------------------------------------------
def test_one_step_on_the_table_within_the_bounds_of_the_plane(gpu_device):
    """Section 24's eight states, the column standing on the table top instead of the plane (moved by the table's place and
    height), stepped once against the reference with the device's contact list."""
    from pegasus_amd import dynamics as DYN
    env, ref = ground()
    names = DC.SCENES["column"]
    bodies, types = [rigid(n) for n in names], [ref_type(n) for n in names]
    _, states = DC.contact_states()
    states = np.array(states)
    states[:, :, 0] += -0.5
    states[:, :, 2] += EC.TABLE_HEIGHT
    states = DR.f32(states)
    p = EC.ground_params(types)
    pp = DC.package_params(p)
    S = len(states)
    words = host_words(DYN.contacts(bodies, [[0, 1, 2]] * S, states, pp, ground=env))
    traj, rest, status, after = DYN.simulate(bodies, [[0, 1, 2]] * S, steps=1, params=pp, state=states, return_state=True, ground=env)
    after = after.cpu().numpy().astype(np.float64)
    assert (status.cpu().numpy() == 0).all() and (rest.cpu().numpy() == -1).all()
    n_rows = n_near = n_ground = 0
    worst_v = worst_x = 0.0
    for w in range(S):
        contacts = DR.contact_list([[int(x) for x in row] for row in words[w]], 3)
        with ER.ground_rule(ref):
            new, rows, _ = DR.step(types, [0, 1, 2], states[w], p, contacts)
        n_rows += len(rows)
        n_ground += sum(r["b"] == DR.PLANE for r in rows)
        near = sum(r["near_clamp"] for r in rows)
        n_near += near
        if near:
            continue
        ev, ex = np.abs(after[w, :, 7:] - new[:, 7:]).max(), np.abs(after[w, :, :7] - new[:, :7]).max()
        print(f"\n[environment] one step, state {w}: {len(rows)} rows, velocity error {ev:.3g}, pose error {ex:.3g}")
        worst_v, worst_x = max(worst_v, ev), max(worst_x, ex)
    print(f"\n[environment] one step: worst velocity error {worst_v:.4g} (bound {STEP_VELOCITY_BOUND:.4g}), worst pose error "
          f"{worst_x:.4g} (bound {STEP_POSE_BOUND:.4g}); {n_near}/{n_rows} rows near a clamp, {n_ground} against the ground")
    assert n_rows >= 20 and n_ground >= 4 and n_near <= DC.MAX_ROW_EXEMPT * n_rows
    assert worst_v <= STEP_VELOCITY_BOUND and worst_x <= STEP_POSE_BOUND


# ---- 4: flat ground against the plane -------------------------------------------------------------------------------------------
def test_flat_field_rests_the_tilted_cube_where_the_plane_does(gpu_device):
    from pegasus_amd import dynamics as DYN
    env, ref = ground("z")
    bodies, types = [rigid("cube")], [ref_type("cube")]
    p = DC.scene_params("cube_tilted", types)
    pp = DC.package_params(p)
    poses0 = np.stack([DC.start_poses("cube_tilted", w) for w in range(2)])
    on_field = DYN.simulate(bodies, [[0]] * 2, poses0, DC.STEPS, pp, record_every=DC.STEPS, ground=env)
    on_plane = DYN.simulate(bodies, [[0]] * 2, poses0, DC.STEPS, pp, record_every=DC.STEPS)
    # counted: a trilinear sample of the field z (exact in exact arithmetic) carries collision_reference.sample_bound
    g = EC.ground_grid()
    bound = (18.0 + 12.0 * max(g.n)) * CR.U * float(np.abs(EC.z_field()).max()) + 36.0 * CR.U * 2.0
    for (traj, rest, status), what in ((on_field, "field"), (on_plane, "plane")):
        assert (status.cpu().numpy() == 0).all() and ((rest.cpu().numpy() >= 0) & (rest.cpu().numpy() < DC.STEPS)).all(), what
    zf, zp = on_field[0].cpu().numpy()[:, -1, 0, 2].astype(np.float64), on_plane[0].cpu().numpy()[:, -1, 0, 2].astype(np.float64)
    print(f"\n[environment] flat field: final heights {zf.tolist()} on the field, {zp.tolist()} on the plane; rest steps "
          f"{on_field[1].tolist()} and {on_plane[1].tolist()}; allowed difference {p.slop + bound:.3g}")
    assert np.abs(zf - zp).max() <= p.slop + bound and np.abs(zp - 0.5).max() <= CC.drop_slack([types[0].grid.voxel]) + p.slop


# ---- 5: the table -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_depth():
    """d: the float64 reference's own deepest steady penetration on its own table field (dynamics_cases.steady_depth)."""
    types = [DC.ref_type(EC.BODY)]
    p = EC.ground_params(types)
    with ER.ground_rule(EC.ground_reference()):
        run = DR.simulate(types, [0], DC.state_of(types, EC.cube_start(EC.ON_TABLE)), DC.STEPS, p)
    assert run["rest_step"] >= 0
    return DC.steady_depth(run, p)


def final_pose(row):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = DR.rotation(row[3:]), row[:3]
    return T


def test_cubes_rest_on_the_table_and_on_the_floor_beside_it(gpu_device):
    from pegasus_amd import dynamics as DYN
    env, ref = ground()
    bodies, types = [rigid()], [ref_type()]
    p = EC.ground_params(types)
    pp = DC.package_params(p)
    poses0 = np.stack([EC.cube_start(EC.ON_TABLE), EC.cube_start(EC.BESIDE_TABLE)])
    traj, rest, status = DYN.simulate(bodies, [[0]] * 2, poses0, DC.STEPS, pp, record_every=DC.STEPS, ground=env)
    traj, rest, status = traj.cpu().numpy().astype(np.float64)[:, -1, 0], rest.cpu().numpy(), status.cpu().numpy()
    assert (status == 0).all() and ((rest >= 0) & (rest < DC.STEPS)).all(), (status.tolist(), rest.tolist())
    E, d = ER.ground_slack(EC.GROUND_VOXEL), reference_depth()
    below = (0.5 * 3.0 ** 0.5 + 0.5) * EC.GROUND_VOXEL                   # how far BELOW the exact distance a sample can lie
    v = DC.mesh(EC.BODY)[0].astype(np.float64)
    clear = []
    for w in range(2):
        T = final_pose(traj[w])
        clear.append(float(EC.ground_distance(v @ T[:3, :3].T + T[:3, 3]).min()))
        assert clear[w] >= -(E + p.slop + d), (w, clear[w])
        assert clear[w] <= p.margin + below, (w, clear[w])               # it lies ON the ground, it does not hover
        assert not DYN.outside_ground(env, traj[w]).any()
    half = 0.3
    print(f"\n[environment] table: rest steps {rest.tolist()}, final heights {traj[:, 2].tolist()}, exact clearances {clear} "
          f"(allowed {-(E + p.slop + d):.3g} .. {p.margin + below:.3g}); d = {d:.3g}")
    assert abs(traj[0, 2] - (EC.TABLE_HEIGHT + half)) <= E + p.slop + d and abs(traj[1, 2] - half) <= E + p.slop + d
    # the same start through the existing plane entry ends a table's height lower: what the feature is for
    plane, prest, pstatus = DYN.simulate(bodies, [[0]], poses0[:1], DC.STEPS, pp, record_every=DC.STEPS)
    z_plane = float(plane.cpu().numpy()[0, -1, 0, 2])
    assert int(pstatus[0]) == 0 and int(prest[0]) >= 0
    assert abs((traj[0, 2] - z_plane) - EC.TABLE_HEIGHT) <= E + p.slop + d, (traj[0, 2], z_plane)


# ---- 6: the null ground, batches ----------------------------------------------------------------------------------------------
def _simulate_entry(entry, bodies, types, poses0, steps, pp, ground_args=()):
    import torch
    from pegasus_amd import _lib, dynamics as DYN
    t = DYN._types(types, len(bodies))
    S, B = t.shape
    device = bodies[0].body.sdf.field.device
    d_type = torch.from_numpy(t).to(device)
    d_state = torch.as_tensor(DYN.states_from_poses(bodies, t, poses0)).to(device).contiguous().clone()
    traj = torch.zeros((S, steps, B, 7), dtype=torch.float32, device=device)
    rest = torch.full((S,), -1, dtype=torch.int32, device=device)
    status = torch.zeros((S,), dtype=torch.int32, device=device)
    ws = _lib.workspace("pgr_rigid", device, S, B)
    p = pp.struct(bodies)
    _lib.call(entry, device, C.byref(p), *ground_args, len(bodies), DYN._table(bodies), S, B, _lib.ptr(d_type), _lib.ptr(d_state),
              steps, 1, _lib.ptr(traj), _lib.ptr(rest), _lib.ptr(status), _lib.ptr(ws), ws.numel())
    return [x.cpu().numpy() for x in (traj, rest, status, d_state)]


def test_null_ground_gives_the_bytes_of_the_plane_entries(gpu_device):
    from pegasus_amd import dynamics as DYN
    names = DC.SCENES["column"]
    bodies, types = [rigid(n) for n in names], [ref_type(n) for n in names]
    pp = DC.package_params(DC.params(types))
    poses0 = np.stack([DC.start_poses("column", w) for w in range(4)])
    rows = [[0, 1, 2]] * 4
    old = _simulate_entry("pgr_rigid_simulate", bodies, rows, poses0, 200, pp)
    new = _simulate_entry("pgr_rigid_simulate_ground", bodies, rows, poses0, 200, pp, (None,))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(old, new))
    assert np.abs(old[0][:, -1] - old[0][:, 0]).max() > 0.1                # they did move and touch
    through = DYN.simulate(bodies, rows, poses0, 200, pp, return_state=True)
    assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(old, through))
    _, states = DC.contact_states()
    import torch
    from pegasus_amd import _lib
    S = len(states)
    d_type = torch.from_numpy(DYN._types([[0, 1, 2]] * S, 3)).cuda()
    d_state = torch.as_tensor(np.asarray(states, np.float32)).cuda().contiguous()
    out = []
    for entry, extra in (("pgr_rigid_contacts", ()), ("pgr_rigid_contacts_ground", (None,))):
        words = torch.empty((S, 9, 7), dtype=torch.int64, device="cuda")
        ws = _lib.workspace("pgr_rigid", d_type.device, S, 3)
        p = pp.struct(bodies)
        _lib.call(entry, d_type.device, C.byref(p), *extra, 3, DYN._table(bodies), S, 3, _lib.ptr(d_type), _lib.ptr(d_state),
                  _lib.ptr(words), _lib.ptr(ws), ws.numel())
        out.append(words.cpu().numpy().tobytes())
    assert out[0] == out[1]


def test_ground_runs_repeat_and_worlds_of_a_batch_are_independent(gpu_device):
    from pegasus_amd import dynamics as DYN
    env, _ = ground()
    bodies, types = [rigid()], [ref_type()]
    pp = DC.package_params(EC.ground_params(types))
    spots = [EC.ON_TABLE, EC.BESIDE_TABLE, (-0.9, 0.3, 1.3), (0.05, 0.0, 1.3), (-0.5, -0.6, 1.3), (0.6, -0.5, 1.3), (-0.2, 0.2, 1.5),
             (0.9, 0.9, 1.2)]
    poses0 = np.stack([EC.cube_start(np.asarray(at, np.float64), w) for w, at in enumerate(spots)])
    steps = 300

    def run(q):
        return [x.cpu().numpy() for x in DYN.simulate(bodies, [[0]] * len(q), q, steps, pp, return_state=True, ground=env)]
    a, b = run(poses0), run(poses0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "two runs differ"
    assert (a[2] == 0).all() and (a[1] >= 0).any()
    for w in (0, 3, 7):
        alone = run(poses0[w:w + 1])
        assert all(x[w:w + 1].tobytes() == y.tobytes() for x, y in zip(a, alone)), f"world {w} alone differs"


# ---- 7: placement by sweeps ---------------------------------------------------------------------------------------------------
def test_drop_puts_a_box_on_the_table_top_and_distances_follow_the_reference(gpu_device):
    from pegasus_amd import collision as COL
    env, ref = ground()
    body = rigid().body
    tol = CC.DROP_TOL
    E = ER.ground_slack(EC.GROUND_VOXEL)
    poses, reports = COL.drop([body, body], orientations=[np.eye(3)] * 2, xy=[(-0.5, 0.0), (0.78, 0.0)], tol=tol, environment=env)
    assert all(r["settled"] for r in reports) and reports[0]["touches"] == ["environment"], reports
    assert abs(poses[0, 2, 3] - (EC.TABLE_HEIGHT + 0.3)) <= tol + E and abs(poses[1, 2, 3] - 0.3) <= tol + E, poses[:, 2, 3]
    plain, _ = COL.drop([body], orientations=[np.eye(3)], xy=[(-0.5, 0.0)], tol=tol)
    assert abs(plain[0, 2, 3] - 0.3) <= tol + CC.drop_slack([body.voxel])         # without the environment: down on the plane
    # min_distances: column B + 1 is the smallest sample of the ground's field over the body's shell
    D = COL.min_distances([body, body], poses, environment=env)
    assert D.shape == (2, 4) and np.isinf(D[:, 2]).all()
    for a in range(2):
        x = CR.world_points(DC.shell(EC.BODY), poses[a])
        value, _, info = CR.sample(ref.field, ref.grid, x)
        k = int(np.argmin(value))
        bound = CR.sweep_step_bound(max(1.0, float(np.abs(x).max())), CR.sample_bound(ref.grid, info)[k]) + 4 * CR.U * abs(value[k])
        assert abs(float(D[a, 3]) - value[k]) <= bound, (a, float(D[a, 3]), value[k], bound)
        assert D[a, 3] <= 2 * tol + 1e-6
    # lifted by 0.4, the sweep brings it back down; the field is not 1-Lipschitz, so a step may overshoot by the field's error
    travel = COL.sweep([body], _lifted(poses[:1], 0.4), 0, (0, 0, -1), environment=env, tol=tol)
    assert abs(travel["travel"] - 0.4) <= 2 * tol + E and travel["jobs"][-1][1] == 1


def _lifted(poses, dz):
    out = np.array(poses, np.float64)
    out[:, 2, 3] += dz
    return out


# ---- 8: from Gaussians ----------------------------------------------------------------------------------------------------------
def slab_scene():
    """A floor slab of Gaussians around z = 0 with a raised block on it, as scenes.py builds its plane and its boxes."""
    from pegasus_amd import scenes
    from pegasus_amd.gaussian_model import GaussianModel
    rng = np.random.default_rng(25)
    floor = scenes.ground_plane(rng, 30_000, 1.0, math.log(0.006), 0.3, 0.1, 0.002)
    block = scenes.rigid_transform(scenes.box_object(rng, 12_000, (0.2, 0.16, 0.08), math.log(0.004), 0.3, 0.15, object_id=0), np.eye(3),
                                   np.array([0.0, 0.0, 0.04]))
    cloud = scenes.SplatCloud.concat([floor, block])
    cloud.opacity[:] = 6.0                                              # opaque: the renders' alpha is 1 on the surfaces
    return GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling, cloud.rotation)


def test_field_of_a_rendered_scene_is_the_field_of_the_reference_volume(gpu_device):
    import torch
    from pegasus_amd import environment as ENV, mesh as M
    from test_mesh_gpu import device_specs
    model = slab_scene()
    raw = [v for v in MC.raw_views_around((0.0, 0.0, 0.03), 1.0, 48, 64, 64, math.radians(40.0), math.radians(40.0))
           if v.camera_center[2] > 0.35][:16]
    assert len(raw) == 16
    specs = device_specs(raw)
    voxel = 0.025
    lo, hi = np.array([-0.3, -0.3, -0.1]), np.array([0.275, 0.275, 0.175])
    env = ENV.EnvironmentField.from_gaussians(model, specs, (lo, hi), voxel)
    g = env.grid
    assert (g.nx, g.ny, g.nz) == (24, 24, 12) and env.tsdf is not None
    depth, final_T = M.render_views(model, specs)
    rg = CR.RefGrid(g.nx, g.ny, g.nz, g.origin, g.voxel)
    want, ambiguous = MR.tsdf_reference(g, [v.world_view_transform.reshape(16) for v in raw], [v.tanfovx for v in raw],
                                        [v.tanfovy for v in raw], depth.cpu().numpy(), final_T.cpu().numpy(), 4.0 * voxel, 0.5,
                                        return_ambiguous=True)
    got = env.tsdf.cpu().numpy()
    differs = got != want
    assert not (differs & ~ambiguous).any() and differs.mean() < 0.001
    assert env.field.cpu().numpy().tobytes() == ER.phi32(got, voxel).tobytes()
    from_reference = ENV.EnvironmentField.from_tsdf(torch.from_numpy(want).cuda(), g)
    assert from_reference.field.cpu().numpy().tobytes() == ER.phi32(want, voxel).tobytes()
    if not differs.any():
        assert from_reference.field.cpu().numpy().tobytes() == env.field.cpu().numpy().tobytes()
    # where the zero level lies over the Gaussians' plane z = 0 and over the block's top z = 0.08: measured, held to two voxels
    pts = CR.grid_points(rg)
    phi = env.field.cpu().numpy().astype(np.float64)

    def level(ix, iy):
        col, z = phi[:, iy, ix], pts[:, iy, ix, 2]
        k = int(np.flatnonzero((col[:-1] < 0) & (col[1:] >= 0))[-1])
        return z[k] + (z[k + 1] - z[k]) * (-col[k]) / (col[k + 1] - col[k])
    floor = np.array([level(ix, iy) for ix in (2, 3, 20, 21) for iy in (2, 3, 20, 21)])
    top = np.array([level(ix, iy) for ix in (11, 12, 13) for iy in (11, 12, 13)])
    print(f"\n[environment] rendered slab: zero level over the floor {floor.min() / voxel:+.3f} .. {floor.max() / voxel:+.3f} voxels from "
          f"z = 0, over the block {(top.min() - 0.08) / voxel:+.3f} .. {(top.max() - 0.08) / voxel:+.3f} voxels from its top")
    assert np.abs(floor).max() <= 2 * voxel and np.abs(top - 0.08).max() <= 2 * voxel
    mesh = env.surface_mesh()
    assert len(mesh.faces) > 100


def test_files_and_engine_with_an_environment(gpu_device, tmp_path):
    import types as pytypes
    import json
    from pegasus_amd import dynamics as DYN, environment as ENV
    env, _ = ground()
    path = env.save(tmp_path / "env" / "table.npz")
    back = ENV.EnvironmentField.load(path)
    assert back.field.cpu().numpy().tobytes() == env.field.cpu().numpy().tobytes() and back.grid == env.grid and back.friction == env.friction
    by_id = {1: rigid()}
    out = tmp_path / "sim" / "simulation_steps.json"
    eng = DYN.Engine(by_id, str(out), simulation_steps=400, seed=3, params=DC.package_params(EC.ground_params([ref_type()])))
    eng.add_object(pytypes.SimpleNamespace(TYPE="environment", urdf_file_name="table.urdf", field=back))
    eng.add_object(pytypes.SimpleNamespace(TYPE="object", ID=1, urdf_file_name="obj_000001.urdf"), start_pos=[-0.5, 0.0, 1.3])
    traj, rest, status = eng.simulate()
    doc = json.loads(out.read_text())
    assert status == 0 and doc["asset_infos"]["environment"] == {"table": {"bullet_id": [0], "class_name": "environment"}}
    assert traj[-1, 0, 2] > EC.TABLE_HEIGHT                              # on the table, not on the plane under it
    from pegasus_amd.mesh import Mesh
    box = ENV.EnvironmentField.from_mesh(Mesh(*DC.mesh("cube")), resolution=24, friction=0.25)
    import torch
    inside_outside = box.signed_distance(torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.58]], device="cuda")).cpu().numpy()     # in its grid
    assert abs(inside_outside[0] + 0.5) < 0.05 and abs(inside_outside[1] - 0.08) < 0.05 and box.struct().friction == 0.25
    poses = DYN.start_states([rigid()], [[0, 0]], seed=1, radius=0.2, ground=env)
    plain = DYN.start_states([rigid()], [[0, 0]], seed=1, radius=0.2)
    assert poses[0, 0, 2] >= plain[0, 0, 2] + 0.4 and np.array_equal(poses[..., 3:], plain[..., 3:])  # above the table top


def test_collision_command_line_places_on_and_checks_against_the_environment(gpu_device, tmp_path, capsys):
    import json
    from pegasus_amd import collision as COL, environment as ENV, mesh as M
    env, _ = ground()
    npz = env.save(tmp_path / "table.npz")
    models = tmp_path / "models"
    v, f = DC.mesh(EC.BODY)
    M.write_ply(models / "obj_000001.ply", M.Mesh(v, f), scale=1000.0)            # BOP millimetres
    out = tmp_path / "placed" / "simulation_steps.json"
    args = ["--models", str(models), "--objects", "1", "--scale", "0.001", "--resolution", "24", "--seed", "2", "--radius", "0.05"]
    assert COL.main(args + ["--environment", str(npz), "--out", str(out)]) == 0
    assert "touches ['environment']" in capsys.readouterr().out
    E = ER.ground_slack(EC.GROUND_VOXEL)
    z = COL.read_simulation_steps(out)[1][2]
    assert abs(z - (EC.TABLE_HEIGHT + 0.3)) <= CC.DROP_TOL + E, z                 # on the table top: the footprint reaches over it
    # a dataset whose camera frame is the world's: the cube 0.1 deep in the table top in one image, well above it in the other
    scene = tmp_path / "data" / "train" / "000000"
    scene.mkdir(parents=True)
    entry = lambda t: {"obj_id": 1, "cam_R_m2c": np.eye(3).ravel().tolist(), "cam_t_m2c": list(t)}
    cam = {"cam_K": [100, 0, 32, 0, 100, 32, 0, 0, 1], "cam_R_w2c": np.eye(3).ravel().tolist(), "cam_t_w2c": [0.0, 0.0, 0.0]}
    (scene / "scene_gt.json").write_text(json.dumps({"0": [entry((-0.5, 0.0, EC.TABLE_HEIGHT + 0.2))], "1": [entry((-0.5, 0.0, 1.2))]}))
    (scene / "scene_camera.json").write_text(json.dumps({"0": cam, "1": cam}))
    report = COL.check_dataset(tmp_path / "data", models, resolution=24, environment=ENV.EnvironmentField.load(npz))[str(scene)]
    assert abs(report["0"] + 0.1) <= E and report["1"] > 0.2, report
    assert COL.check_dataset(tmp_path / "data", models, resolution=24)[str(scene)]["0"] == float("inf")      # one object, no environment
    assert COL.main(["--check", str(tmp_path / "data"), "--models", str(models), "--resolution", "24", "--environment", str(npz)]) == 0
    assert "deepest interpenetration: -0." in capsys.readouterr().out
    (scene / "scene_camera.json").write_text(json.dumps({"0": {"cam_K": cam["cam_K"]}, "1": cam}))
    with pytest.raises(ValueError, match="cam_R_w2c"):
        COL.check_dataset(tmp_path / "data", models, resolution=24, environment=env)
