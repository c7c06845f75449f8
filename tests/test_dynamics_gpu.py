"""pgr_rigid_contacts, pgr_rigid_simulate and pegasus_amd.dynamics on the GPU against the float64 reference
(tests/dynamics_reference.py) evaluated on the device's own fields, read back: contact words per word, one step per state, free
flight against the closed recursion, settling, friction, determinism and the files.

Measured on the MI355X: over the eight states of dynamics_cases.contact_states the largest one-step error
against the reference stepped with the device's contact list is MEASURED_STEP_VELOCITY in v and omega and MEASURED_STEP_POSE in
x and q; the test asserts four times that (the factor covers differences in fused multiply-add contraction between machines)."""
import functools
import json
import types as pytypes

import numpy as np
import pytest

import collision_cases as CC
import collision_reference as CR
import dynamics_cases as DC
import dynamics_reference as DR

pytestmark = pytest.mark.gpu
MEASURED_STEP_VELOCITY = 7.4e-5       # state 3, 24 rows: 7.366e-05; the bias phi / h carries a field error of 1e-7 a thousandfold
MEASURED_STEP_POSE = 1.01e-7         # states 1 and 5: 1.003e-07
STEP_FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def rigid(name, friction=0.5):
    """The package's body of a case mesh: a 24^3 field, the case's shell."""
    from pegasus_amd import collision as COL, dynamics as DYN
    from pegasus_amd.mesh import Mesh
    m = Mesh(*DC.mesh(name))
    body = COL.CollisionBody(m, COL.MeshSDF.from_mesh(m, resolution=DC.RESOLUTION), shell=DC.shell(name))
    return DYN.RigidBody.from_collision(body, mass=1.0, friction=friction)


@functools.lru_cache(maxsize=None)
def ref_type(name, friction=0.5):
    """The reference's type on the DEVICE's field of that body, read back."""
    b = rigid(name, friction).body
    g = b.sdf.grid
    t = DC.ref_type(name, friction, field=b.sdf.field.cpu().numpy().astype(np.float64), grid=CR.RefGrid(g.nx, g.ny, g.nz, g.origin, g.voxel))
    r = rigid(name, friction)
    assert np.array_equal(t.com, DR.f32(r.com)) and np.array_equal(t.iinv, DR.f32(r.inv_inertia)) and t.radius == float(np.float32(r.radius))
    return t


def column():
    names = DC.SCENES["column"]
    return [rigid(n) for n in names], [ref_type(n) for n in names]


def host_words(words):
    return words.cpu().numpy().view(np.uint64)


# ---- 1: contact words ---------------------------------------------------------------------------------------------------------
def test_contact_words_against_the_reference_on_the_device_fields(gpu_device):
    from pegasus_amd import dynamics as DYN
    from pegasus_amd.collision import decode_words
    bodies, types = column()
    _, states = DC.contact_states()
    p = DC.params(types)
    S = len(states)
    words = host_words(DYN.contacts(bodies, [[0, 1, 2]] * S, states, DC.package_params(p)))
    assert words.shape == (S, 9, 7)
    assert words.tobytes() == host_words(DYN.contacts(bodies, [[0, 1, 2]] * S, states, DC.package_params(p))).tobytes()
    value, index = decode_words(words)
    n_exempt = n_words = n_compared = 0
    worst = 0.0
    for w in range(S):
        ref, exempt = DC.word_exemptions(types, [0, 1, 2], states[w], p)
        _, info = DR.world_words(types, [0, 1, 2], states[w], p, detail=True)
        n_words += exempt.size
        n_exempt += int(exempt.sum())
        for k in range(9):
            for j in range(7):
                if exempt[k, j]:
                    continue
                if ref[k][j] == DR.EMPTY:
                    assert int(words[w, k, j]) == DR.EMPTY, (w, k, j)
                    continue
                i = ref[k][j] & 0xFFFFFFFF
                assert index[w, k, j] == i, (w, k, j, int(index[w, k, j]), i)
                err, bound = abs(float(value[w, k, j]) - info[k]["values"][i, j]), info[k]["bound"][i] + 4 * CR.U * abs(info[k]["values"][i, j])
                assert err <= bound, (w, k, j, err, bound)
                worst = max(worst, err / bound)
                n_compared += 1
    print(f"\n[dynamics] contact words: {n_compared} compared, {n_exempt}/{n_words} exempt, max error/bound {worst:.4f}")
    assert n_exempt <= DC.MAX_WORD_EXEMPT * n_words and n_compared >= 100
    assert (words[0] == np.uint64(DR.EMPTY)).all() and (words[4] == np.uint64(DR.EMPTY)).all()      # mid-air: out of sphere range


def test_contact_ties_empty_slots_and_a_single_body(gpu_device):
    from pegasus_amd import dynamics as DYN
    from pegasus_amd.collision import decode_words
    bodies, types = column()
    p = DC.params(types)
    flat = DC.state_of(types, np.array([[0.0, 0.0, 0.5, 0, 0, 0, 1.0], [3.0, 0.0, 5.0, 0, 0, 0, 1.0], [0.0, 3.0, 0.31, 0, 0, 0, 1.0]]))
    # S = 1, B = 1: the cube flat on the plane; every bottom point has the same phi and the same r.z: the lowest index wins
    w1 = host_words(DYN.contacts(bodies[:1], [[0]], flat[None, :1], DC.package_params(p)))
    value, index = decode_words(w1)
    bottom = np.flatnonzero(DC.shell("cube")[:, 2] == -0.5)
    assert w1.shape == (1, 1, 7) and index[0, 0, 0] == bottom[0] and index[0, 0, 5] == bottom[0] and index[0, 0, 6] == bottom[0]
    assert value[0, 0, 0] == 0.0 and value[0, 0, 5] == np.float32(-0.5)
    ref = DR.world_words(types[:1], [0], flat[:1], p)
    assert [int(x) for x in w1[0, 0]] == ref[0]                                   # exact numbers: the words are the reference's
    # an empty slot takes part in nothing
    w3 = host_words(DYN.contacts(bodies, [[0, -1, 2]], flat[None], DC.package_params(p)))
    assert (w3[0, [1, 3, 4, 5, 7]] == np.uint64(DR.EMPTY)).all()                  # pairs with slot 1, and slot 1 on the plane
    assert w3[0, 0, 0] != np.uint64(DR.EMPTY) and w3[0, 8, 0] != np.uint64(DR.EMPTY)
    assert (w3[0, [2, 6]] == np.uint64(DR.EMPTY)).all()                           # cube and small cube: out of sphere range
    assert w3[0, 0].tobytes() == w1[0, 0].tobytes()
    traj, rest, status = DYN.simulate(bodies, [[0, -1, 2]], steps=3, params=DC.package_params(p), state=flat[None])
    assert (traj.cpu().numpy()[0, :, 1] == (0, 0, 0, 0, 0, 0, 1)).all() and int(status[0]) == 0


# ---- 2: one step --------------------------------------------------------------------------------------------------------------
def test_one_step_against_the_reference_with_the_device_contact_list(gpu_device):
    from pegasus_amd import dynamics as DYN
    bodies, types = column()
    _, states = DC.contact_states()
    p = DC.params(types)
    S = len(states)
    pp = DC.package_params(p)
    words = host_words(DYN.contacts(bodies, [[0, 1, 2]] * S, states, pp))
    traj, rest, status, after = DYN.simulate(bodies, [[0, 1, 2]] * S, steps=1, params=pp, state=states, return_state=True)
    after, traj = after.cpu().numpy().astype(np.float64), traj.cpu().numpy().astype(np.float64)
    assert (status.cpu().numpy() == 0).all() and (rest.cpu().numpy() == -1).all() and traj.shape == (S, 1, 3, 7)
    n_rows = n_near = 0
    worst_v = worst_x = 0.0
    for w in range(S):
        contacts = DR.contact_list([[int(x) for x in row] for row in words[w]], 3)
        new, rows, _ = DR.step(types, [0, 1, 2], states[w], p, contacts)
        n_rows += len(rows)
        near = sum(r["near_clamp"] for r in rows)
        n_near += near
        for a in range(3):
            assert np.abs(traj[w, 0, a] - DR.mesh_pose(after[w, a], types[a].com)).max() <= 64 * CR.U * 4.0          # the record is the state
        if near:
            continue
        ev, ex = np.abs(after[w, :, 7:] - new[:, 7:]).max(), np.abs(after[w, :, :7] - new[:, :7]).max()
        print(f"\n[dynamics] one step, state {w}: {len(rows)} rows, velocity error {ev:.3g}, pose error {ex:.3g}")
        worst_v, worst_x = max(worst_v, ev), max(worst_x, ex)
    print(f"\n[dynamics] one step: worst velocity error {worst_v:.4g} (recorded {MEASURED_STEP_VELOCITY:.4g}), worst pose error "
          f"{worst_x:.4g} (recorded {MEASURED_STEP_POSE:.4g}); {n_near}/{n_rows} rows near a clamp")
    assert n_rows >= 20 and n_near <= DC.MAX_ROW_EXEMPT * n_rows
    assert worst_v <= STEP_FACTOR * MEASURED_STEP_VELOCITY and worst_x <= STEP_FACTOR * MEASURED_STEP_POSE


# ---- 3: free fall -------------------------------------------------------------------------------------------------------------
def test_free_fall_follows_the_recursion_within_the_counted_bound(gpu_device):
    from pegasus_amd import dynamics as DYN
    types = [ref_type("cube")]
    p = DC.params(types)
    K, z0, v0, spin = 200, 50.0, (0.3, 0.0, 2.0), (1.0, -2.0, 3.0)
    state = DC.state_of(types, np.array([[0.1, -0.2, z0, 0.0, 0.0, 0.0, 1.0]]))
    state[0, 7:10], state[0, 10:13] = v0, spin
    traj, rest, status, after = DYN.simulate([rigid("cube")], [[0]], steps=K, params=DC.package_params(p), state=state[None],
                                             return_state=True)
    traj, after = traj.cpu().numpy().astype(np.float64)[0, :, 0], after.cpu().numpy().astype(np.float64)[0, 0]
    run = DR.simulate(types, [0], state, K, p)
    assert int(rest[0]) == -1 and int(status[0]) == 0 and run["contacts"].max() == 0
    # counted: v_k = (v + h g) f takes 3 roundings of |v| <= vmax per step; z_k = z + h v_k two of |z| <= z0 + 1, plus h times
    # the error of v_k; q' = q + (h/2)(..) and its normalisation take fewer than 16 roundings of numbers <= 1 per step
    u, vmax = CR.U, abs(v0[2]) + K * p.h * abs(p.gravity[2])
    v_bound = K * 3 * u * vmax
    z_bound = K * (2 * u * (z0 + 1.0) + p.h * v_bound)
    q_bound = K * 16 * u
    worst = 0.0
    for k in (1, 2, 17, 100, K):
        z, _ = DR.free_flight(state[0, 2], v0[2], p.gravity[2], p.h, p.lin_factor, k)
        assert abs(traj[k - 1, 2] - z) <= z_bound, (k, traj[k - 1, 2], z)
        worst = max(worst, abs(traj[k - 1, 2] - z) / z_bound)
    _, v = DR.free_flight(state[0, 2], v0[2], p.gravity[2], p.h, p.lin_factor, K)
    assert abs(after[9] - v) <= v_bound and abs(after[7] - v0[0] * p.lin_factor ** K) <= v_bound
    assert np.abs(after[10:13] - np.asarray(spin) * p.ang_factor ** K).max() <= K * 2 * u * 3.0
    q_err = np.abs(traj[:, 3:] - run["trajectory"][:, 0, 3:]).max()
    assert q_err <= q_bound and abs(np.linalg.norm(after[3:7]) - 1.0) <= 4 * u
    assert np.abs(run["trajectory"][-1, 0, 3:] - (0, 0, 0, 1)).max() > 0.1        # it did turn
    print(f"\n[dynamics] free fall: z error/bound {worst:.4f}, v error/bound {abs(after[9] - v) / v_bound:.4f}, q error/bound "
          f"{q_err / q_bound:.4f}")


# ---- 4: settling --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DC.SCENES))
def test_scenes_settle_without_interpenetration(gpu_device, name):
    from pegasus_amd import dynamics as DYN
    names = DC.SCENES[name]
    bodies, types = [rigid(n) for n in names], [ref_type(n) for n in names]
    p = DC.scene_params(name, types)
    B = len(names)
    poses0 = np.stack([DC.start_poses(name, w) for w in range(DC.WORLDS)])
    traj, rest, status = DYN.simulate(bodies, [list(range(B))] * DC.WORLDS, poses0, DC.STEPS, DC.package_params(p),
                                      record_every=DC.STEPS)
    traj, rest, status = traj.cpu().numpy().astype(np.float64), rest.cpu().numpy(), status.cpu().numpy()
    assert (status == 0).all() and np.isfinite(traj).all()
    assert ((rest >= 0) & (rest < DC.STEPS)).all(), rest.tolist()
    E = CC.drop_slack([t.grid.voxel for t in types])
    d = DC.steady_depth(DC.reference_run(name, 0), p)
    meshes = [DC.mesh(n) for n in names]
    deepest, farthest = 0.0, 0.0
    for w in range(DC.WORLDS):
        poses = np.tile(np.eye(4), (B, 1, 1))
        for k, row in enumerate(traj[w, -1]):
            poses[k, :3, :3], poses[k, :3, 3] = DR.rotation(row[3:]), row[:3]
        clear = CR.exact_clearances(meshes, poses)
        assert clear.min() >= -(E + p.slop + d), (w, clear.tolist())
        for a in range(B):
            nearest = min(clear[a].min(), min((clear[b, a] for b in range(B) if b != a), default=np.inf))
            assert nearest <= p.margin + E, (w, a, nearest)
            farthest = max(farthest, nearest)
        deepest = min(deepest, clear.min())
        if name == "sphere":
            assert abs(traj[w, -1, 0, 2] - 0.5) <= E + p.slop + d, (w, traj[w, -1, 0, 2])
    print(f"\n[dynamics] {name}: rest steps {rest.tolist()}, deepest exact clearance {deepest:.3g} (allowed {-(E + p.slop + d):.3g}), "
          f"farthest nearest-neighbour {farthest:.3g}")


# ---- 5: friction --------------------------------------------------------------------------------------------------------------
def test_friction_holds_above_tan_and_slides_below(gpu_device):
    from pegasus_amd import dynamics as DYN
    moved = {}
    for case, friction in DC.FRICTION_CASES.items():
        types = [ref_type("cube", friction)]
        p = DC.friction_params(types)
        traj, rest, status = DYN.simulate([rigid("cube", friction)], [[0]], DC.friction_start()[None], DC.FRICTION_STEPS,
                                          DC.package_params(p), record_every=DC.FRICTION_STEPS)
        assert int(status[0]) == 0
        moved[case] = traj.cpu().numpy().astype(np.float64)[0, -1, 0, :3] - DC.friction_start()[0, :3]
    voxel = ref_type("cube").grid.voxel
    reference = DC.friction_reference("slides")["state"][0, 0]
    print(f"\n[dynamics] friction: mu 0.5 moved {np.linalg.norm(moved['sticks']):.3g} (one voxel {voxel:.3g}); mu 0.1 slid "
          f"{moved['slides'][0]:.4g}, the reference {reference:.4g}")
    assert np.linalg.norm(moved["sticks"]) < voxel
    assert moved["slides"][0] >= 0.9 * reference


# ---- 6: determinism and independence ------------------------------------------------------------------------------------------
def test_runs_repeat_worlds_are_independent_and_records_are_strided(gpu_device):
    from pegasus_amd import dynamics as DYN
    bodies, types = column()
    p = DC.package_params(DC.params(types))
    poses0 = np.stack([DC.start_poses("column", w) for w in range(DC.WORLDS)])
    rows = [[0, 1, 2]] * DC.WORLDS
    steps = 240

    def run(t, q, every=1):
        out = DYN.simulate(bodies, t, q, steps, p, record_every=every, return_state=True)
        return [x.cpu().numpy() for x in out]
    a, b = run(rows, poses0), run(rows, poses0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "two runs differ"
    assert (a[1] >= 0).any()                                                      # the runs are long enough to come to rest
    for w in (0, 5):
        alone = run(rows[:1], poses0[w:w + 1])
        assert all(x[w:w + 1].tobytes() == y.tobytes() for x, y in zip(a, alone)), f"world {w} alone differs"
    every4 = run(rows, poses0, 4)
    assert every4[0].shape == (DC.WORLDS, steps // 4, 3, 7) and every4[0].tobytes() == np.ascontiguousarray(a[0][:, 3::4]).tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], every4[1:]))


# ---- 7: end to end ------------------------------------------------------------------------------------------------------------
def _write_models(tmp_path):
    from pegasus_amd.mesh import Mesh, write_obj
    d = tmp_path / "urdf"
    d.mkdir()
    for i, name in ((1, "cube"), (2, "small_cube")):
        v, f = DC.mesh(name)
        write_obj(d / f"obj_{i:06d}_collision.obj", Mesh((v.astype(np.float64) * 0.1).astype(np.float32), f))
    return d


def test_engine_and_command_line_write_files_the_readers_read(gpu_device, tmp_path, capsys):
    from pegasus_amd import collision as COL, dynamics as DYN, trajectory as TJ
    models = _write_models(tmp_path)
    by_id = DYN.bodies_from_dir(models, resolution=24)
    path = tmp_path / "engine" / "simulation_steps.json"
    eng = DYN.Engine(by_id, str(path), simulation_steps=300, seed=4)
    eng.add_object(pytypes.SimpleNamespace(TYPE="environment", urdf_file_name="plane.urdf"))
    eng.add_object(pytypes.SimpleNamespace(TYPE="object", ID=1, urdf_file_name="obj_000001.urdf"), start_pos=[0.0, 0.0, 0.12])
    eng.add_object(pytypes.SimpleNamespace(TYPE="object", ID=2, urdf_file_name="obj_000002.urdf"), start_pos=[0.01, 0.0, 0.3])
    traj, rest, status = eng.simulate()
    assert traj.shape == (300, 2, 7) and status == 0 and np.isfinite(traj).all()
    sim = TJ.load_simulation(path)
    last = COL.read_simulation_steps(path)
    assert sim.shape == (2, 300, 7) and sorted(last) == [0, 1, 2]
    doc = json.loads(path.read_text())
    assert doc["asset_infos"]["object"]["obj_000002"]["object_ID"] == 2
    for k in range(2):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = DR.rotation(traj[-1, k, 3:].astype(np.float64)), traj[-1, k, :3]
        center = by_id[k + 1].body.mesh.vertices.astype(np.float64).mean(0)
        assert np.allclose(last[k + 1][:3], COL.reference_translation(T, center), atol=1e-9)
        assert np.allclose(last[k + 1][3:], traj[-1, k, 3:], atol=0) and np.array_equal(last[k + 1], sim[k, -1])
    assert traj[-1, 0, 2] < 0.12 and traj[0, 1, 2] > traj[-1, 1, 2] > 0.0         # both fell, neither through the ground
    out = tmp_path / "cli"
    assert DYN.main(["--models", str(models), "--objects", "1", "2", "--scenes", "3", "--steps", "200", "--seed", "0",
                     "--resolution", "24", "--out", str(out)]) == 0
    text = capsys.readouterr().out
    for w in range(3):
        f = out / f"scene_{w:06d}" / "simulation_steps.json"
        assert str(f) in text and TJ.load_simulation(f).shape == (2, 200, 7) and sorted(COL.read_simulation_steps(f)) == [0, 1, 2]
    assert not np.array_equal(TJ.load_simulation(out / "scene_000000" / "simulation_steps.json"),
                              TJ.load_simulation(out / "scene_000001" / "simulation_steps.json"))


def test_start_states_follow_the_seed_and_clear_each_other(gpu_device):
    from pegasus_amd import dynamics as DYN
    bodies, _ = column()
    a, b = DYN.start_states(bodies, [[0, 1, 2], [2, -1, 0]], seed=5), DYN.start_states(bodies, [[0, 1, 2], [2, -1, 0]], seed=5)
    assert a.shape == (2, 3, 7) and np.array_equal(a, b) and not np.array_equal(a, DYN.start_states(bodies, [[0, 1, 2], [2, -1, 0]], seed=6))
    assert np.allclose(np.linalg.norm(a[..., 3:], axis=-1), 1.0) and (a[0, :, 3:] > 0).all()      # four draws from (0, 1)
    assert (a[1, 1] == (0, 0, 0, 0, 0, 0, 1)).all() and (np.diff(a[0, :, 2]) > 0).all()           # an empty slot; stacked heights
    words = host_words(DYN.contacts(bodies, [[0, 1, 2]], DYN.states_from_poses(bodies, [[0, 1, 2]], a[:1])))
    assert (words == np.uint64(DR.EMPTY)).all()                                   # nothing starts within a voxel of anything
