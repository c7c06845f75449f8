"""rigid_contacts_kernel and rigid_solve_kernel at the edges the other dynamics tests never reach: shells beyond one block of 256
points, world batches around the 64 lanes of a workgroup, eight slots and sixteen types, lanes of one wave on different type
rows, rest and sleeping, record strides that do not divide the steps, and the guard (rule 7).

Most checks are byte equalities with the BASE run: the eight states of dynamics_cases.contact_states as S = 8, B = 3, which
tests/test_dynamics_gpu.py ties to the float64 reference.  A world's arithmetic depends neither on its lane, nor on S, nor on the
numbers of the slots its bodies sit in while their ascending order is kept; so every such world must give base's bytes.  The
contact words of the larger shells and the crowded world's step are held against the reference itself."""
import functools

import numpy as np
import pytest

import collision_reference as CR
import dynamics_cases as DC
import dynamics_reference as DR
import environment_cases as EC
from test_dynamics_gpu import column, host_words, ref_type, rigid

pytestmark = pytest.mark.gpu
BASE_STEPS = 60
EMPTY_POSE = (0, 0, 0, 0, 0, 0, 1)


def base_of(w):
    """The contact state world w of a batch starts from: every residue in every run of eight lanes."""
    return (5 * w + 3) % 8


def simulate(bodies, types, state, steps, pp, **kw):
    """[trajectory, rest step, status, final state] on the host."""
    from pegasus_amd import dynamics as DYN
    return [x.cpu().numpy() for x in DYN.simulate(bodies, types, steps=steps, params=pp, state=state, return_state=True, **kw)]


def column_params(**kw):
    return DC.package_params(DC.params(column()[1], **kw))


@functools.lru_cache(maxsize=None)
def base(steps=BASE_STEPS, sleep_steps=DC.SLEEP_STEPS):
    """The base run (for ``steps`` steps), read-only."""
    bodies, _ = column()
    _, states = DC.contact_states()
    out = simulate(bodies, [[0, 1, 2]] * len(states), states, steps, column_params(sleep_steps=sleep_steps))
    assert out[0].shape == (8, steps, 3, 7) and np.isfinite(out[0]).all() and (out[2] == 0).all()
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def base_words():
    from pegasus_amd import dynamics as DYN
    bodies, _ = column()
    _, states = DC.contact_states()
    return host_words(DYN.contacts(bodies, [[0, 1, 2]] * len(states), states, column_params()))


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def assert_world(got, w, want, v, slots=slice(None), want_slots=slice(None), rest=True, what=""):
    """World w of ``got`` equals world v of ``want`` byte for byte: trajectory, final state, status and (``rest``) rest step."""
    assert same(got[0][w][:, slots], want[0][v][:, want_slots]), f"{what}: trajectory of world {w} differs from world {v}"
    assert same(got[3][w][slots], want[3][v][want_slots]), f"{what}: final state of world {w} differs from world {v}"
    assert got[2][w] == want[2][v], f"{what}: status of world {w}"
    if rest:
        assert got[1][w] == want[1][v], f"{what}: rest step of world {w}: {got[1][w]}, not {want[1][v]}"


@functools.lru_cache(maxsize=None)
def rigid_with_shell(name, key):
    """``rigid(name)`` -- the same mesh and the same device field -- with another shell: key (k, n) is body k of a shell case, 'tie'
    the tie shell.  Returns (the package's body, the reference's type on the device's field)."""
    from pegasus_amd import collision as COL, dynamics as DYN
    points = DC.tie_shell() if key == "tie" else DC.scattered_shell(name, key[1], key)
    r = rigid(name)
    body = DYN.RigidBody.from_collision(COL.CollisionBody(r.body.mesh, r.body.sdf, shell=np.array(points)), mass=1.0, friction=0.5)
    t = DC.with_shell(ref_type(name), points)
    assert len(body.body.shell) == len(points) and t.radius == float(np.float32(body.radius))
    return body, t


def compare_words(words, types, rows, states, p):
    """test_contact_words_against_the_reference_on_the_device_fields' comparison of words [S, B*B, 7] with the reference, word by
    word.  Returns (compared, exempt, all, compared with an index >= 256, largest error / bound)."""
    from pegasus_amd.collision import decode_words
    value, index = decode_words(words)
    n_exempt = n_words = n_compared = n_high = 0
    worst = 0.0
    for w in range(len(states)):
        ref, exempt = DC.word_exemptions(types, rows[w], states[w], p)
        _, info = DR.world_words(types, rows[w], states[w], p, detail=True)
        n_words += exempt.size
        n_exempt += int(exempt.sum())
        for k in range(exempt.shape[0]):
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
                n_high += i >= DC.POINT_BLOCK
    return n_compared, n_exempt, n_words, n_high, worst


# ---- 1: shells beyond one point block -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.SHELL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_contact_words_of_shells_beyond_one_point_block(gpu_device, case):
    """test_contact_words_against_the_reference_on_the_device_fields' comparison, bound, exemption rule and cap on scattered
    shells of up to three point blocks.  Measured on the MI355X: (257, 513, 256) compares 148 words, exempts
    6 of 504, 23 compared words name a point >= 256; (300, 700, 64) compares 147, exempts 7 of 504, 30 name a point >= 256;
    largest error/bound 0.030 in both."""
    from pegasus_amd import dynamics as DYN
    made = [rigid_with_shell(name, (k, n)) for k, (name, n) in enumerate(zip(DC.SCENES["column"], case))]
    bodies, types = [m[0] for m in made], [m[1] for m in made]
    _, states = DC.contact_states()
    p = DC.params(column()[1])
    S = len(states)
    rows = [[0, 1, 2]] * S
    words = host_words(DYN.contacts(bodies, rows, states, DC.package_params(p)))
    assert words.shape == (S, 9, 7)
    assert words.tobytes() == host_words(DYN.contacts(bodies, rows, states, DC.package_params(p))).tobytes()
    n_compared, n_exempt, n_words, n_high, worst = compare_words(words, types, rows, states, p)
    print(f"\n[dynamics edges] shells {case}: {n_compared} words compared, {n_exempt}/{n_words} exempt, {n_high} compared words with "
          f"an index >= {DC.POINT_BLOCK}, max error/bound {worst:.4f}")
    assert n_exempt <= DC.MAX_WORD_EXEMPT * n_words and n_compared >= 100
    assert n_high >= DC.MIN_HIGH_INDEX_WORDS
    assert (words[0] == np.uint64(DR.EMPTY)).all() and (words[4] == np.uint64(DR.EMPTY)).all()      # mid-air: out of sphere range


def test_a_tie_across_point_blocks_resolves_to_the_lowest_index(gpu_device):
    from pegasus_amd import dynamics as DYN
    from pegasus_amd.collision import decode_words
    body, t = rigid_with_shell("cube", "tie")
    p = DC.params(column()[1])
    flat = DC.flat_cube_state([t])
    w1 = host_words(DYN.contacts([body], [[0]], flat[None], DC.package_params(p)))
    value, index = decode_words(w1)
    bottom = np.flatnonzero(DC.tie_shell()[:, 2] == -0.5)
    assert DC.POINT_BLOCK <= bottom[0] < 2 * DC.POINT_BLOCK <= bottom[-1]         # the tie spans blocks 1 and 2; block 0 has no candidate
    assert w1.shape == (1, 1, 7) and index[0, 0, 0] == bottom[0] and index[0, 0, 5] == bottom[0] and index[0, 0, 6] == bottom[0]
    assert value[0, 0, 0] == 0.0 and value[0, 0, 5] == np.float32(-0.5)
    assert [int(x) for x in w1[0, 0]] == DR.world_words([t], [0], flat, p)[0]     # exact numbers: the words are the reference's
    assert w1.tobytes() == host_words(DYN.contacts([body], [[0]], flat[None], DC.package_params(p))).tobytes()


# ---- 2: world-batch edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (63, 64, 65, 130))
def test_every_world_of_a_batch_gives_the_bytes_of_base(gpu_device, S):
    from pegasus_amd import dynamics as DYN
    bodies, _ = column()
    _, states = DC.contact_states()
    pick = [base_of(w) for w in range(S)]
    got = simulate(bodies, [[0, 1, 2]] * S, states[pick], BASE_STEPS, column_params())
    assert got[0].shape == (S, BASE_STEPS, 3, 7)
    for w in range(S):
        assert_world(got, w, base(), pick[w], what=f"S = {S}")
    assert (base()[1] >= 0).any() and (base()[1] < 0).any()                        # worlds that sleep and worlds that do not
    if S == 130:
        words = host_words(DYN.contacts(bodies, [[0, 1, 2]] * S, states[pick], column_params()))
        assert same(words, base_words()[pick])
        # 64 is a multiple of 8: above, lane l of every workgroup holds the same state.  Once more with each workgroup shifted
        shifted = [(pick[w] + w // 64) % 8 for w in range(S)]
        got = simulate(bodies, [[0, 1, 2]] * S, states[shifted], BASE_STEPS, column_params())
        for w in range(S):
            assert_world(got, w, base(), shifted[w], what=f"S = {S}, shifted")


def test_every_world_of_a_batch_on_a_field_ground_gives_the_bytes_of_a_small_run(gpu_device):
    from test_environment_gpu import ground, ref_type as env_ref_type, rigid as env_rigid
    env, _ = ground()
    bodies = [env_rigid()]
    pp = DC.package_params(EC.ground_params([env_ref_type()]))
    states = EC.contact_states()
    n = len(states)
    small = simulate(bodies, [[0]] * n, states, BASE_STEPS, pp, ground=env)
    assert (small[2] == 0).all() and np.abs(small[0][:, -1] - small[0][:, 0]).max() > 0.01            # they do move
    S = 65
    pick = [(7 * w + 3) % n for w in range(S)]
    assert sorted(set(pick)) == list(range(n))
    got = simulate(bodies, [[0]] * S, states[pick], BASE_STEPS, pp, ground=env)
    for w in range(S):
        assert_world(got, w, small, pick[w], what="field ground")


def test_lanes_of_one_wave_on_different_type_rows(gpu_device):
    bodies, types = column()
    _, states = DC.contact_states()
    rows = [[0, 1, 2], [0, -1, 2], [-1, -1, -1], [0, 1, 2], [2, -1, -1], [0, 1, 2]]
    pick = [3, 5, 1, 7, 6, 2]
    start = np.array(states[pick])
    start[2] = DR.f32(np.arange(39).reshape(3, 13) * 0.25 - 3.0)                   # an empty world's state: any bytes
    pp = column_params()
    got = simulate(bodies, rows, start, BASE_STEPS, pp)
    for w in (0, 3, 5):
        assert_world(got, w, base(), pick[w], what="mixed rows")
    for w in (1, 4):
        alone = simulate(bodies, rows[w:w + 1], start[w:w + 1], BASE_STEPS, pp)
        assert_world(got, w, alone, 0, what="mixed rows, alone")
        assert (got[0][w][:, 1] == EMPTY_POSE).all() and same(got[3][w][1], start[w, 1].astype(np.float32))
        assert np.abs(got[0][w][-1, 0] - got[0][w][0, 0]).max() > 0 and got[2][w] == 0
    assert got[2][2] == 0 and (got[0][2] == EMPTY_POSE).all() and same(got[3][2], start[2].astype(np.float32))
    run = DR.simulate(types, rows[2], start[2], BASE_STEPS, DC.params(types))
    assert got[1][2] == DC.SLEEP_STEPS - 1 == run["rest_step"] and run["status"] == 0    # calm from the first step on


# ---- 3: slot and type-table edges ---------------------------------------------------------------------------------------------
def eight_slots(states, fill):
    """[S,8,13]: the column's states in slots 1, 4 and 7, ``fill`` {slot: [13]} in the others."""
    out = np.zeros((len(states), 8, 13))
    out[:, list(DC.COLUMN_SLOTS)] = states
    for a, s in fill.items():
        out[:, a] = s
    return out


def test_the_column_embedded_in_eight_slots(gpu_device):
    bodies, _ = column()
    _, states = DC.contact_states()
    fill = {a: DR.f32(np.arange(13) * 0.5 - a) for a in DC.FLYER_SLOTS}            # empty slots: any bytes, they must stay
    start = eight_slots(states, fill)
    got = simulate(bodies, [list(DC.EMBEDDED_ROW)] * 8, start, BASE_STEPS, column_params())
    for w in range(8):
        assert_world(got, w, base(), w, slots=list(DC.COLUMN_SLOTS), what="embedded")
        assert (got[0][w][:, list(DC.FLYER_SLOTS)] == EMPTY_POSE).all()
        assert same(got[3][w][list(DC.FLYER_SLOTS)], start[w][list(DC.FLYER_SLOTS)].astype(np.float32))


def test_eight_full_slots_whose_extra_bodies_touch_nothing(gpu_device):
    bodies, types = column()
    _, states = DC.contact_states()
    fly = DC.flyers(types)
    pp = column_params(sleep_steps=0)
    start = eight_slots(states, fly)
    got = simulate(bodies, [list(DC.FULL_ROW)] * 8, start, BASE_STEPS, pp)
    want = base(BASE_STEPS, 0)
    assert (got[1] == -1).all() and (want[1] == -1).all()
    for w in range(8):
        assert_world(got, w, want, w, slots=list(DC.COLUMN_SLOTS), rest=False, what="full")
    for a, s in fly.items():
        alone = simulate(bodies, [[DC.FULL_ROW[a]]], s[None, None], BASE_STEPS, pp)
        assert alone[0][0, -1, 0, 2] < alone[0][0, 0, 0, 2] and alone[2][0] == 0                      # it falls
        for w in (0, 7):
            assert_world(got, w, alone, 0, slots=[a], rest=False, what=f"flyer in slot {a}")


def test_type_indices_up_to_the_last_of_sixteen(gpu_device):
    from pegasus_amd import dynamics as DYN
    bodies, _ = column()
    table = [rigid("icosphere")] * DYN.MAX_TYPES
    table[15], table[7], table[3] = bodies
    _, states = DC.contact_states()
    got = simulate(table, [[15, 7, 3]] * 8, states, BASE_STEPS, column_params())
    for w in range(8):
        assert_world(got, w, base(), w, what="types 15, 7, 3")
    words = host_words(DYN.contacts(table, [[15, 7, 3]] * 8, states, column_params()))
    assert same(words, base_words())


def test_a_crowded_world_of_eight_bodies_against_the_reference(gpu_device):
    """Eight small cubes in mutual contact: 56 pair slots in use, about 200 rows.  The tolerance is not the device's: the solver
    drives each normal velocity to minus its bias phi / h, so an error of a row's phi shows as that over h in v; the velocity
    tolerance is the largest phi bound the reference states for this state's rows (pair_points' fifth value) over h, the pose
    tolerance h times that plus 64 u.  Measured on the MI355X: 392 words compared, 0 of 448 exempt, largest
    error/bound 0.019; 200 rows, none near a clamp; velocity error 1.874e-4 against the tolerance 4.869e-3, pose error 9.377e-8
    against 8.684e-6."""
    from pegasus_amd import dynamics as DYN
    body, t = rigid("small_cube"), ref_type("small_cube")
    types, row = [t], [0] * 8
    p = DC.params(types)
    pp = DC.package_params(p)
    state = DC.crowd(types)
    words = host_words(DYN.contacts([body], [row], state[None], pp))
    assert words.shape == (1, 64, 7) and same(words, host_words(DYN.contacts([body], [row], state[None], pp)))
    n_compared, n_exempt, n_words, _, worst = compare_words(words, types, [row], state[None], p)
    assert n_exempt <= DC.MAX_WORD_EXEMPT * n_words and n_compared >= 300
    got = simulate([body], [row], state[None], 1, pp)
    again = simulate([body], [row], state[None], 1, pp)
    assert all(same(a, b) for a, b in zip(got, again)), "two runs differ"
    assert got[2][0] == 0 and got[1][0] == -1
    contacts = DR.contact_list([[int(x) for x in r] for r in words[0]], 8)
    new, rows, _ = DR.step(types, row, state, p, contacts)
    near = sum(r["near_clamp"] for r in rows)
    tol_v = max(float(DR.pair_points(types, row, state, a, b, p, [i])[4][0]) for a, b, i in contacts) / p.h
    tol_x = p.h * tol_v + 64 * CR.U
    after = got[3][0].astype(np.float64)
    ev, ex = np.abs(after[:, 7:] - new[:, 7:]).max(), np.abs(after[:, :7] - new[:, :7]).max()
    print(f"\n[dynamics edges] crowd: {n_compared} words compared, {n_exempt}/{n_words} exempt, max error/bound {worst:.4f}; "
          f"{len(rows)} rows, {near} near a clamp; velocity error {ev:.4g} (tolerance {tol_v:.4g}), pose error {ex:.4g} "
          f"(tolerance {tol_x:.4g})")
    assert len(rows) >= 150 and near <= DC.MAX_ROW_EXEMPT * len(rows)
    for a in range(8):
        assert np.abs(got[0][0, 0, a] - DR.mesh_pose(after[a], t.com)).max() <= 64 * CR.U * 4.0           # the record is the state
    assert ev <= tol_v and ex <= tol_x
    # as world 64 of a batch whose first wave holds empty worlds only: rows at stride 65, in the second workgroup
    batch = np.zeros((65, 8, 13))
    batch[:, :, 6] = 1.0
    batch[64] = state
    in_batch = simulate([body], [[-1] * 8] * 64 + [row], batch, 1, pp)
    assert_world(in_batch, 64, got, 0, what="crowd in a batch")
    assert (in_batch[0][:64] == EMPTY_POSE).all() and (in_batch[2] == 0).all()


# ---- 4: rest, sleeping and records --------------------------------------------------------------------------------------------
REST_STEPS = 240


@functools.lru_cache(maxsize=None)
def drop(steps=REST_STEPS, every=1, sleep_steps=DC.SLEEP_STEPS):
    """The column's eight start worlds (dynamics_cases.start_poses), from poses."""
    from pegasus_amd import dynamics as DYN
    bodies, _ = column()
    poses0 = np.stack([DC.start_poses("column", w) for w in range(DC.WORLDS)])
    out = DYN.simulate(bodies, [[0, 1, 2]] * DC.WORLDS, poses0, steps, column_params(sleep_steps=sleep_steps), record_every=every,
                       return_state=True)
    return [x.cpu().numpy() for x in out]


def test_a_world_at_rest_repeats_its_pose_and_sleeping_changes_nothing_before(gpu_device):
    a, awake = drop(), drop(sleep_steps=0)
    assert (awake[1] == -1).all() and (awake[2] == 0).all() and (a[2] == 0).all()
    resting = np.flatnonzero(a[1] >= 0)
    assert len(resting) >= 4, a[1].tolist()
    for w in resting:
        r = int(a[1][w])
        assert DC.SLEEP_STEPS - 1 <= r < REST_STEPS - 1
        assert (a[0][w][r + 1:].view(np.uint32) == a[0][w][r].view(np.uint32)).all(), f"world {w} moves after its rest step {r}"
        assert (a[3][w][:, 7:].view(np.uint32) == 0).all(), f"world {w} sleeps with a velocity"
        assert same(a[0][w][:r + 1], awake[0][w][:r + 1]), f"world {w}: sleeping changed a record before the rest step"
    for w in np.flatnonzero(a[1] < 0):
        assert_world(a, w, awake, w, what="never at rest")


def test_record_strides_that_do_not_divide_the_steps_and_runs_without_a_record(gpu_device):
    ten, every4 = drop(10), drop(10, 4)
    assert every4[0].shape == (DC.WORLDS, 2, 3, 7) and same(every4[0], ten[0][:, [3, 7]])
    assert all(same(x, y) for x, y in zip(ten[1:], every4[1:]))
    three, none = drop(3), drop(3, 4)
    assert none[0].shape == (DC.WORLDS, 0, 3, 7) and all(same(x, y) for x, y in zip(three[1:], none[1:]))
    assert not same(three[3], ten[3]) and same(three[0], ten[0][:, :3])
    zero = drop(0)
    from pegasus_amd import dynamics as DYN
    bodies, _ = column()
    start = DYN.states_from_poses(bodies, [[0, 1, 2]] * DC.WORLDS, np.stack([DC.start_poses("column", w) for w in range(DC.WORLDS)]))
    assert zero[0].shape == (DC.WORLDS, 0, 3, 7) and same(zero[3], start) and (zero[1] == -1).all() and (zero[2] == 0).all()


# ---- 5: the guard -------------------------------------------------------------------------------------------------------------
def test_the_guard_freezes_a_world_at_its_last_finite_state(gpu_device):
    bodies, types = column()
    _, states = DC.contact_states()
    p = DC.params(types)
    S, steps = 66, 20
    trigger = {0: "A", 63: "B", 65: "A"}
    pick = [base_of(w) for w in range(S)]
    start = np.stack([DC.guard_state(states[pick[w]], trigger.get(w)) for w in range(S)])
    rows = [DC.guard_types(trigger.get(w)) for w in range(S)]
    got = simulate(bodies, rows, start, steps, DC.package_params(p))
    traj, rest, status, state = got
    assert np.isfinite(traj).all() and np.isfinite(state).all()
    assert [w for w in range(S) if status[w]] == sorted(trigger) and (status[sorted(trigger)] == 1).all()
    want = base(steps)
    for w in range(S):
        if w not in trigger:
            assert_world(got, w, want, pick[w], slots=[0, 1, 2], what="beside a guarded world")
            assert (traj[w][:, 3] == EMPTY_POSE).all() and same(state[w][3], start[w, 3].astype(np.float32))
    for w in (0, 65):                                                              # A: frozen at the input, in step 0
        assert rest[w] == -1 and same(state[w], start[w].astype(np.float32))
        assert (traj[w].view(np.uint32) == traj[w][0].view(np.uint32)).all()
        for a in (0, 2):
            assert np.abs(traj[w][0, a] - DR.mesh_pose(start[w, a], types[a].com)).max() <= 64 * CR.U * 4.0
        x, c = start[w, 1, :3].astype(np.float32), types[1].com.astype(np.float32)
        assert same(traj[w][0, 1], np.concatenate([x - c, np.zeros(4, np.float32)]))                  # R(0) = 1: T = x - c
    w, k = 63, DC.GUARD_STEP["B"]                                                  # B: frozen at the start of step 2
    two = base(k)
    assert rest[w] == -1 and same(state[w][:3], two[3][pick[w]]) and same(traj[w][:k, :3], two[0][pick[w]])
    assert (traj[w][k:].view(np.uint32) == traj[w][k - 1].view(np.uint32)).all()
    with np.errstate(all="ignore"):
        run = DR.simulate(types, rows[w], start[w], k + 1, p, snapshots=[k])
    assert run["status"] == 1
    far, ref = state[w][3].astype(np.float64), run["snapshots"][k][3]
    u = CR.U
    v_bound = k * 3 * u * DC.FAR_VZ
    z_bound = k * (2 * u * float(np.finfo(np.float32).max) + p.h * v_bound)
    assert abs(far[9] - ref[9]) <= v_bound and abs(far[2] - ref[2]) <= z_bound and far[2] > DC.FAR_Z
    assert np.array_equal(np.delete(far, [2, 9]), np.delete(ref, [2, 9]))          # everything else is 0 or 1 exactly
    assert traj[w][k - 1, 3, 2] > traj[w][0, 3, 2] > DC.FAR_Z
    print(f"\n[dynamics edges] guard: far body frozen at z = {far[2]:.6g} (reference {ref[2]:.6g}, bound {z_bound:.3g})")
