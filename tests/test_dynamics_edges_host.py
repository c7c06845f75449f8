"""The inputs of tests/test_dynamics_edges_gpu.py judged on the float64 reference alone, on its own fields: the scattered shells
stay within the exemption cap and do put winners beyond the first point block, the tie shell is ordered as the tie test needs, the
crowded world has enough clean rows, the guard's triggers fire at the steps the device test names, an empty world is calm from
the first step, and the flyers stay out of everything's range.  A later change of a seed cannot then hide a failure on the device."""
import numpy as np
import pytest

import dynamics_cases as DC
import dynamics_reference as DR


def column_types(shells=None):
    types = [DC.ref_type(n) for n in DC.SCENES["column"]]
    return types if shells is None else [DC.with_shell(t, s) for t, s in zip(types, shells)]


def test_scattered_shells_are_seeded_hold_the_vertices_and_lie_on_the_faces():
    for name, n in (("cube", 257), ("l_prism", 513), ("small_cube", 64)):
        s = DC.scattered_shell(name, n, (1, n))
        v, f = DC.mesh(name)
        assert s.shape == (n, 3) and s.dtype == np.float32 and s is DC.scattered_shell(name, n, (1, n))
        assert not np.array_equal(s, DC.scattered_shell(name, n, (2, n)))
        assert {tuple(x) for x in v} <= {tuple(x) for x in s}                     # every vertex is a shell point
        tri = v.astype(np.float64)[f]
        normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        off = np.abs(np.einsum("fk,nfk->nf", normal, s.astype(np.float64)[:, None] - tri[None, :, 0]))
        assert off.min(axis=1).max() <= 1e-6                                      # on a face's plane (and inside the hull)
        assert np.abs(s).max() <= np.abs(v).max()
        assert DC.with_shell(DC.ref_type(name), s).radius == DC.ref_type(name).radius          # the sphere tests do not change


@pytest.mark.parametrize("case", DC.SHELL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_shell_cases_meet_the_exemption_cap_and_win_beyond_the_first_block(case):
    names, states = DC.contact_states()
    types = column_types(DC.case_shells(case))
    p = DC.params(column_types())
    assert [len(t.shell) for t in types] == list(case)
    n_words = n_exempt = n_full = n_high = n_high_compared = 0
    for state in states:
        words, exempt = DC.word_exemptions(types, [0, 1, 2], state, p)
        full = np.array([[w != DR.EMPTY for w in pair] for pair in words])
        high = np.array([[w != DR.EMPTY and (w & 0xFFFFFFFF) >= DC.POINT_BLOCK for w in pair] for pair in words])
        n_words += exempt.size
        n_exempt += int(exempt.sum())
        n_full += int(full.sum())
        n_high += int(high.sum())
        n_high_compared += int((high & ~exempt).sum())
    print(f"\n[dynamics edges] shells {case}: {n_exempt}/{n_words} words exempt, {n_full} non-empty, {n_high} with an index >= 256 "
          f"({n_high_compared} of them compared)")
    assert n_exempt <= DC.MAX_WORD_EXEMPT * n_words and n_full >= 100
    assert n_high_compared >= DC.MIN_HIGH_INDEX_WORDS


def test_tie_shell_puts_the_bottom_face_into_blocks_one_and_two():
    s = DC.tie_shell()
    bottom = np.flatnonzero(s[:, 2] == -0.5)
    assert s.shape == (DC.TIE_POINTS, 3) and len(bottom) >= 20
    assert DC.POINT_BLOCK <= bottom[0] < 2 * DC.POINT_BLOCK and (bottom >= 2 * DC.POINT_BLOCK).sum() >= 5
    types = [DC.with_shell(DC.ref_type("cube"), s)]
    p = DC.params(column_types())
    assert not ((s[:, 2] > -0.5) & (s[:, 2] <= -0.5 + 2 * p.margin)).any()        # the candidates are the bottom points alone
    words = DR.world_words(types, [0], DC.flat_cube_state(types), p)
    assert [w & 0xFFFFFFFF for w in words[0]][0::5] == [bottom[0], bottom[0]] and words[0][6] & 0xFFFFFFFF == bottom[0]
    assert all(w & 0xFFFFFFFF in set(bottom.tolist()) for w in words[0])


def test_the_crowd_has_many_clean_rows_and_no_plane_contact():
    types = [DC.ref_type("small_cube")]
    p = DC.params(types)
    state = DC.crowd(types)
    row = [0] * 8
    words, exempt = DC.word_exemptions(types, row, state, p)
    contacts = DR.contact_list(words, 8)
    pairs = {(a, b) for a, b, _ in contacts}
    new, rows, calm = DR.step(types, row, state, p)
    near = sum(r["near_clamp"] for r in rows)
    bound = max(float(DR.pair_points(types, row, state, a, b, p, [i])[4][0]) for a, b, i in contacts)
    print(f"\n[dynamics edges] crowd: {len(rows)} rows over {len(pairs)} ordered pairs, {int(exempt.sum())}/{exempt.size} words "
          f"exempt, {near} rows near a clamp, largest phi bound {bound:.3g} (velocity tolerance {bound / p.h:.3g})")
    assert len(rows) >= 150 and len(pairs) == 56 and all(b != DR.PLANE for _, b in pairs)
    assert exempt.sum() <= DC.MAX_WORD_EXEMPT * exempt.size and near <= DC.MAX_ROW_EXEMPT * len(rows)
    assert np.isfinite(new).all() and not calm
    # equal masses: the contacts exchange momentum, gravity and damping act on every body alike
    want = (state[:, 7:10].sum(0) + 8 * p.h * p.gravity) * p.lin_factor
    assert np.abs(new[:, 7:10].sum(0) - want).max() <= 1e-13
    assert np.abs(new[:, 7:13] - state[:, 7:13]).max() > 0.1                      # the rows did something


def test_the_guard_triggers_fire_at_their_steps_in_the_reference():
    types = column_types()
    p = DC.params(types)
    _, states = DC.contact_states()
    for trigger, world in (("A", 3), ("B", 6), ("A", 0)):
        start = DC.guard_state(states[world], trigger)
        row = DC.guard_types(trigger)
        k = DC.GUARD_STEP[trigger]
        with np.errstate(all="ignore"):
            before = DR.simulate(types, row, start, k, p)
            after = DR.simulate(types, row, start, k + 3, p, snapshots=[k])
        assert before["status"] == 0 and np.isfinite(before["state"].astype(np.float32)).all()
        assert after["status"] == 1 and after["rest_step"] == -1
        assert np.array_equal(after["state"], after["snapshots"][k]) and np.array_equal(after["state"], before["state"])
        frozen = np.array([DR.mesh_pose(s, types[t].com) if t >= 0 else (0, 0, 0, 0, 0, 0, 1) for s, t in zip(after["state"], row)])
        assert (after["trajectory"][k:] == frozen).all() and np.isfinite(after["trajectory"]).all()
    # trigger B: the far body's height just before the step that overflows, and the step that does
    far = DC.far_body()
    z2, v2 = DR.free_flight(far[2], far[9], p.gravity[2], p.h, p.lin_factor, 2)
    z3, _ = DR.free_flight(far[2], far[9], p.gravity[2], p.h, p.lin_factor, 3)
    big = float(np.finfo(np.float32).max)
    assert z2 < big - 1e35 and z3 > big * (1 + 2.0 ** -25) + 1e34 and np.isfinite(np.float32(v2))


def test_an_empty_world_is_calm_from_the_first_step_in_the_reference():
    types = column_types()
    p = DC.params(types)
    state = np.zeros((3, 13))
    state[:, 6] = 1.0
    run = DR.simulate(types, [-1, -1, -1], state, p.sleep_steps + 5, p)
    assert run["rest_step"] == p.sleep_steps - 1 and run["status"] == 0 and np.array_equal(run["state"], state)
    assert (run["trajectory"] == (0, 0, 0, 0, 0, 0, 1)).all()


def test_the_flyers_stay_out_of_every_range():
    types = column_types()
    p = DC.params(types)
    assert [DC.FULL_ROW[a] for a in DC.COLUMN_SLOTS] == [0, 1, 2] and sorted(DC.COLUMN_SLOTS + DC.FLYER_SLOTS) == list(range(8))
    assert [DC.EMBEDDED_ROW[a] for a in DC.COLUMN_SLOTS] == [0, 1, 2] and all(DC.EMBEDDED_ROW[a] == -1 for a in DC.FLYER_SLOTS)
    fly = DC.flyers(types)
    drop = -DR.free_flight(0.0, 0.0, p.gravity[2], p.h, p.lin_factor, 60)[0]
    reach = 2 * max(t.radius for t in types) + p.margin + drop
    x = np.array([s[:3] for s in fly.values()])
    assert drop < 1.0 and (x[:, 2] - reach > 3.0).all()                           # the column stays below z = 3
    d = np.linalg.norm(x[:, None] - x[None], axis=-1) + np.diag(np.full(len(x), np.inf))
    assert d.min() > reach and np.linalg.norm(x[:, :2], axis=1).min() > reach + 1.0
