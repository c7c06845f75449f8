"""The rigid-body rule without a device: the float64 reference (tests/dynamics_reference.py) obeys the closed free-flight
recursion, exchanges momentum equally in a two-body contact, selects contacts by the word rule (ties included), settles every
scene of tests/dynamics_cases.py within its step budget and stays within the exemption caps of the GPU tests by itself; the
trajectory file round-trips; Engine and the command line reject bad arguments before they touch a device."""
import json
import types as pytypes

import numpy as np
import pytest

import collision_reference as CR
import dynamics_cases as DC
import dynamics_reference as DR


def test_free_flight_follows_the_closed_recursion():
    types = [DC.ref_type("cube")]
    p = DC.params(types)
    state = DC.state_of(types, np.array([[0.1, -0.2, 50.0, 0.0, 0.0, 0.0, 1.0]]))
    state[0, 7:10] = (0.3, 0.0, 2.0)
    run = DR.simulate(types, [0], state, 200, p)
    assert run["contacts"].max() == 0 and run["rest_step"] == -1 and run["status"] == 0
    for k in (1, 2, 17, 200):
        z, v = DR.free_flight(state[0, 2], 2.0, p.gravity[2], p.h, p.lin_factor, k)
        x, _ = DR.free_flight(state[0, 0], 0.3, 0.0, p.h, p.lin_factor, k)
        assert abs(run["trajectory"][k - 1, 0, 2] - z) <= 1e-12 * abs(z)
        assert abs(run["trajectory"][k - 1, 0, 0] - x) <= 1e-12
    # v_k in closed form: the geometric sum of the recursion
    f, hg = p.lin_factor, p.h * p.gravity[2]
    assert abs(DR.free_flight(0.0, 2.0, p.gravity[2], p.h, f, 200)[1] - (2.0 * f ** 200 + hg * f * (1 - f ** 200) / (1 - f))) <= 1e-9


def _momentum(types, state):
    lin, ang = np.zeros(3), np.zeros(3)
    for t, s in zip(types, state):
        R = DR.rotation(s[3:7])
        inertia = R @ np.linalg.inv(t.iinv) @ R.T
        lin += t.mass * s[7:10]
        ang += inertia @ s[10:13] + t.mass * np.cross(s[0:3], s[7:10])
    return lin, ang


def test_a_two_body_contact_exchanges_momentum_equally():
    types = [DC.ref_type("cube"), DC.ref_type("small_cube")]
    p = DC.params(types, plane=(0.0, 0.0, 1.0, -100.0), gravity=(0.0, 0.0, 0.0), lin_damp=0.0, ang_damp=0.0)
    state = DC.state_of(types, np.array([[0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 1.0], [0.21, 0.13, 1.29, 0.05, -0.02, 0.1, 1.0]]))
    state[0, 7:13] = (0.2, 0.0, 0.4, 0.1, -0.3, 0.2)
    state[1, 7:13] = (-0.3, 0.1, -1.5, 0.5, 0.4, -0.6)
    contacts = DR.contact_list(DR.world_words(types, [0, 1], state, p), 2)
    assert contacts and all(b != DR.PLANE for _, b, _ in contacts)
    rows = DR.build_rows(types, [0, 1], state, contacts, p)
    V = state[:, 7:13].copy()
    DR.solve(rows, V, p)
    after = state.copy()
    after[:, 7:13] = V
    assert np.abs(V - state[:, 7:13]).max() > 1e-3                               # the contact did something
    (l0, a0), (l1, a1) = _momentum(types, state), _momentum(types, after)
    # the state's quaternion is a float32 one: its norm is off by u = 2^-24, so R I R^T and R Iinv R^T are inverses to 4 u only
    assert np.abs(l1 - l0).max() <= 1e-12 and np.abs(a1 - a0).max() <= 4 * DR.U * max(1.0, np.abs(a0).max())
    assert all(r["lam"][0] >= 0 and abs(r["lam"][1]) <= r["mu"] * r["lam"][0] + 1e-15 for r in rows)


def test_words_and_contact_selection_on_hand_made_points():
    phi = np.array([0.5, -0.1, -0.1, 0.2, 0.9, 0.2])
    r = np.array([[1, 0, 0], [0, 2, 0], [0, 2, 0], [-3, 0, 1], [9, 9, 9], [1, -1, 1]], np.float64)
    cand = phi <= 0.5                                                            # point 4 is no candidate
    words = DR.words_of(phi, r, cand)
    value, index = zip(*[((w >> 32), w & 0xFFFFFFFF) for w in words])
    assert index[0] == 1                                                         # phi: -0.1 twice, the lower index wins
    assert list(index[1:]) == [3, 0, 5, 1, 0, 3]                                 # +x -x +y -y +z -z; ties to the lowest index
    assert value[0] == CR.order_bits(-0.1) and value[4] == CR.order_bits(-2.0)
    assert DR.contacts_of(words) == [0, 1, 3, 5]                                 # distinct, ascending: point 2 never wins a tie
    assert DR.words_of(phi, r, np.zeros(6, bool)) == [DR.EMPTY] * 7 and DR.contacts_of([DR.EMPTY] * 7) == []
    assert DR.contacts_of(DR.words_of(phi[:1], r[:1], np.ones(1, bool))) == [0]  # one candidate fills all seven words
    assert [(a, b) for a, b in DR.pair_order(3)] == [(0, -1), (0, 1), (0, 2), (1, -1), (1, 0), (1, 2), (2, -1), (2, 0), (2, 1)]
    assert [DR.slot(a, b, 3) for a, b in DR.pair_order(3)] == [0, 1, 2, 4, 3, 5, 8, 6, 7]


@pytest.mark.parametrize("name", sorted(DC.SCENES))
def test_the_reference_settles_every_scene_within_its_budget(name):
    run = DC.reference_run(name, 0)
    types = [DC.ref_type(n) for n in DC.SCENES[name]]
    p = DC.scene_params(name, types)
    assert run["status"] == 0 and 0 <= run["rest_step"] < DC.STEPS, run["rest_step"]
    assert np.isfinite(run["trajectory"]).all()
    assert (run["trajectory"][run["rest_step"]:] == run["trajectory"][run["rest_step"]]).all()        # poses repeat
    E = DC.CC.drop_slack([t.grid.voxel for t in types])
    d = DC.steady_depth(run, p)
    poses = np.tile(np.eye(4), (len(types), 1, 1))
    for k, row in enumerate(run["trajectory"][-1]):
        poses[k, :3, :3], poses[k, :3, 3] = DR.rotation(row[3:]), row[:3]
    clear = CR.exact_clearances([DC.mesh(n) for n in DC.SCENES[name]], poses)
    print(f"\n[dynamics] reference {name}: rest at {run['rest_step']}, deepest steady penetration beyond slop d = {d:.3g}, "
          f"smallest exact clearance {clear.min():.3g}")
    assert clear.min() >= -(E + p.slop + d)
    if name == "sphere":
        assert abs(run["state"][0, 2] - 0.5) <= E + p.slop + d


def test_friction_holds_and_lets_go_in_the_reference():
    stick, slide = DC.friction_reference("sticks"), DC.friction_reference("slides")
    voxel = DC.ref_type("cube").grid.voxel
    assert np.linalg.norm(stick["state"][0, :3] - (0.0, 0.0, 0.5)) < voxel
    g = 50.0 * DC.SIZE
    free = 0.5 * g * (np.sin(DC.TILT) - 0.1 * np.cos(DC.TILT)) * (DC.FRICTION_STEPS * 1e-3) ** 2
    assert 0.9 * free <= slide["state"][0, 0] <= 1.1 * free                      # Coulomb's a = g (sin - mu cos)


def test_the_exemption_caps_are_met_by_the_reference_alone():
    names, states = DC.contact_states()
    types = [DC.ref_type(n) for n in names]
    p = DC.params(types)
    n_words = n_exempt = n_rows = n_near = 0
    for state in states:
        _, exempt = DC.word_exemptions(types, [0, 1, 2], state, p)
        n_words += exempt.size
        n_exempt += int(exempt.sum())
        _, rows, _ = DR.step(types, [0, 1, 2], state, p)
        n_rows += len(rows)
        n_near += sum(r["near_clamp"] for r in rows)
    print(f"\n[dynamics] exempt words {n_exempt}/{n_words}, rows near a clamp {n_near}/{n_rows}")
    assert n_rows >= 20                                                          # the states do hold contacts
    assert n_exempt <= DC.MAX_WORD_EXEMPT * n_words and n_near <= DC.MAX_ROW_EXEMPT * n_rows


def test_trajectory_file_round_trip(tmp_path):
    from pegasus_amd import collision as COL, dynamics as DYN, trajectory as TJ
    rng = np.random.default_rng(3)
    traj = rng.normal(size=(5, 2, 7))
    traj[..., 3:] /= np.linalg.norm(traj[..., 3:], axis=-1, keepdims=True)
    centers = np.array([[0.1, 0.2, 0.3], [0.0, -0.5, 0.25]])
    path = tmp_path / "sub" / "simulation_steps.json"
    doc = DYN.write_trajectory(path, ["obj_000001", "obj_000002"], ["A", "B"], [1, 2], traj, centers)
    assert doc["asset_infos"]["object"]["obj_000002"] == {"bullet_id": [2], "center_of_mass": centers[1].tolist(), "class_name": "B",
                                                          "object_ID": 2}
    assert json.loads(path.read_text()) == doc and list(doc["trajectory"]) == ["0", "1", "2"]
    sim = TJ.load_simulation(path)
    assert sim.shape == (2, 5, 7) and np.array_equal(sim[..., 3:], traj.transpose(1, 0, 2)[..., 3:])
    for k in range(2):
        for s in range(5):
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = DR.rotation(traj[s, k, 3:]), traj[s, k, :3]
            assert np.allclose(sim[k, s, :3], COL.reference_translation(T, centers[k]), atol=1e-12)       # applied once
            # R (x - mu) + mu + t is the mesh-frame pose again
            x = rng.normal(size=3)
            assert np.allclose(T[:3, :3] @ (x - centers[k]) + centers[k] + sim[k, s, :3], T[:3, :3] @ x + T[:3, 3], atol=1e-12)
    last = COL.read_simulation_steps(path)
    assert sorted(last) == [0, 1, 2] and np.array_equal(last[2], sim[1, -1]) and np.array_equal(COL.read_simulation_steps(path, 0)[1], sim[0, 0])
    assert TJ.rest_index(sim) == 4 and TJ.rest_index(np.concatenate([sim, sim[:, -1:], sim[:, -1:]], axis=1)) == 4
    assert TJ.rest_index(sim[:, :1]) == 0
    tables, motions = TJ.simulation_poses(sim, [np.zeros(3), np.ones(3), np.ones(3)], 4, stride=2)
    assert tables.shape == (4, 3, 20) and np.allclose(motions[-1][1], np.eye(4)) and np.allclose(motions[-1][3], np.eye(4))
    assert not np.allclose(motions[0][1], motions[0][2])                         # every object its own body's motion
    with pytest.raises(ValueError):
        DYN.write_trajectory(path, ["a"], ["a"], [1], traj, centers)
    with pytest.raises(ValueError):
        DYN.write_trajectory(path, ["a", "b"], ["a", "b"], [1, 2], np.full((1, 2, 7), np.nan))


def test_engine_and_command_line_reject_bad_arguments(tmp_path):
    from pegasus_amd import dynamics as DYN
    with pytest.raises(ValueError):
        DYN.Engine({}, simulation_steps=0)
    with pytest.raises(ValueError):
        DYN.Engine({}, simulation_steps=10, record_every=11)
    eng = DYN.Engine({}, str(tmp_path / "s.json"), simulation_steps=10)
    eng.add_object(pytypes.SimpleNamespace(TYPE="environment"))                   # the ground: nothing to add
    with pytest.raises(ValueError, match="Wrong entity"):
        eng.add_object(pytypes.SimpleNamespace(TYPE="robot", ID=1))
    with pytest.raises(KeyError):
        eng.add_object(pytypes.SimpleNamespace(TYPE="object", ID=7))
    eng.bodies[7] = object()
    with pytest.raises(ValueError, match="start_pos"):
        eng.add_object(pytypes.SimpleNamespace(TYPE="object", ID=7), start_pos=[0.0, float("nan"), 1.0])
    with pytest.raises(ValueError, match="no object"):
        DYN.Engine({}, simulation_steps=10).simulate()
    a = DYN._parser().parse_args(["--models", "m", "--objects", "1", "2", "5", "--scenes", "10", "--steps", "4000", "--seed", "0", "--out", "o"])
    assert (a.objects, a.scenes, a.steps, a.seed, a.record_every, a.resolution) == ([1, 2, 5], 10, 4000, 0, 1, 96)
    for bad in (["--scenes", "0"], ["--steps", "0"], ["--record_every", "0"], ["--steps", "3", "--record_every", "4"]):
        with pytest.raises(SystemExit):
            DYN.main(["--models", "m", "--objects", "1", "--out", "o"] + bad)
    with pytest.raises(SystemExit):
        DYN.main(["--models", "m", "--objects"] + [str(k) for k in range(1, 10)] + ["--out", "o"])          # nine bodies
    with pytest.raises(SystemExit):
        DYN._parser().parse_args(["--models", "m", "--out", "o"])                # --objects is required
    with pytest.raises(ValueError):
        DYN.RigidBody.from_collision(None, mass=0.0)
    with pytest.raises(ValueError):
        DYN._types([[0, 3]], 2)                                                  # a type outside the table
    with pytest.raises(ValueError):
        DYN._types(np.zeros((1, 9)), 1)
