"""The posing reference (tests/pose_reference.py) against itself and against the project's float64 helpers, and the census of
the cases (tests/pose_cases.py): every branch of pose_prepare_kernel's quaternion rule and every tie between the quantities it
compares must be reached by a case, or this fails on the CPU."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import pose_cases as PC
import pose_reference as PR

CASES = PC.rotation_cases()
TIGHT = 1e-12
# matrices that are rotations to float32 rounding; the accumulated trajectory is deliberately not one
ROTATIONS = [c for c in CASES if c.name != "accumulated_1000"]


def test_cases_are_float32_and_nearly_rotations():
    for c in CASES:
        assert c.R.dtype == np.float32 and c.R.shape == (3, 3)
        d = PR.non_orthonormality(c.R)
        if c.name == "accumulated_1000":
            assert 2 * PR.U < d < 1e-4, d                 # off a rotation by more than rounding one would be, yet a pose
        else:
            assert d <= 2 * PR.U, (c.name, d)             # the premise of K_QUAT
        assert np.linalg.det(c.R.astype(np.float64)) > 0.99


def test_census_reaches_every_branch_and_tie():
    reached = {}
    for c in CASES:
        keys = PR.census(c.R)
        assert set(c.reach) <= keys, (c.name, c.reach, keys)          # each case reaches what it is listed for
        for k in keys:
            reached.setdefault(k, []).append(c.name)
    for k in PR.BRANCHES + PR.TIES:
        assert reached.get(k), f"no case reaches {k}"
    print({k: len(v) for k, v in reached.items()})
    # the seeded random rotations alone spread over all four branches
    rand = [next(iter(PR.census(c.R) & set(PR.BRANCHES))) for c in CASES if c.name.startswith("random_")]
    assert set(rand) == set(PR.BRANCHES), rand
    # the near-half-turn cases take the branch of their axis' largest component, from both distances
    for b in "xyz":
        for short in ("1e-3", "1e-6"):
            (c,) = [c for c in CASES if c.name == f"180-{short}_{b}"]
            assert b in PR.census(c.R)
            angle = np.linalg.norm(Rot.from_matrix(c.R.astype(np.float64)).as_rotvec())
            assert abs((np.pi - angle) - float(short)) < 3e-7, (c.name, np.pi - angle)


def test_band_matrices_are_orthogonal_and_compose():
    for c in ROTATIONS:
        # a float32-rounded rotation is off a true one by ~u, and so are its band matrices: orthogonal to l * few u
        for D in PR.band_matrices(c.R):
            assert np.abs(D @ D.T - np.eye(len(D))).max() < 64 * PR.U, c.name
    for seed in range(4):                                              # exact rotations: to 1e-12
        R1, R2 = Rot.random(random_state=seed).as_matrix(), Rot.random(random_state=100 + seed).as_matrix()
        for D in _bands64(R1):
            assert np.abs(D @ D.T - np.eye(len(D))).max() < TIGHT
        for A, B, Cm in zip(_bands64(R2 @ R1), _bands64(R2), _bands64(R1)):
            assert np.abs(A - B @ Cm).max() < TIGHT
    for D in PR.band_matrices(np.eye(3, dtype=np.float32)):
        assert np.abs(D - np.eye(len(D))).max() < TIGHT


def _bands64(R):
    """band_matrices on a float64 matrix (the module refuses non-float32 values on purpose: only host tests do this)."""
    X = np.linalg.lstsq(PR._BASIS, PR.basis(PR._DIRS @ R), rcond=None)[0]
    return tuple(X[s, s] for s in PR.BANDS.values())


def test_defining_property_on_fresh_directions():
    """f'(d) = f(R^T d): rotated coefficients evaluated at d equal the original ones evaluated at R^T d."""
    rng = np.random.default_rng(99)
    d = rng.normal(size=(500, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    for c in ROTATIONS[::3]:
        R = c.R.astype(np.float64)
        # nearest true rotation, so that the property holds to 1e-12 and not to the rounding of R
        Uu, _, Vt = np.linalg.svd(R); R = Uu @ Vt
        coef = rng.normal(size=(15,))
        out = np.concatenate([D @ coef[s.start - 1:s.stop - 1] for D, s in zip(_bands64(R), PR.BANDS.values())])
        lhs = PR.basis(d)[:, 1:] @ out
        rhs = PR.basis(d @ R)[:, 1:] @ coef
        assert np.abs(lhs - rhs).max() < TIGHT, c.name


def test_band1_is_the_signed_permutation_of_R():
    S = np.array([[0, -1, 0], [0, 0, 1], [-1, 0, 0]], float)          # (x,y,z) -> (-y, z, -x)
    for c in CASES:
        R = c.R.astype(np.float64)
        np.testing.assert_allclose(PR.band_matrices(c.R)[0], S @ R @ S.T, rtol=0, atol=TIGHT, err_msg=c.name)


def test_reference_equals_the_projects_float64_helpers():
    from oracle.compose_ref import compose_object_ref
    from pegasus_amd.sh_rotation import sh_rotation_matrices
    from pegasus_amd.sh_utils import sh_basis
    rng = np.random.default_rng(5)
    d = rng.normal(size=(300, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    np.testing.assert_allclose(PR.basis(d), sh_basis(3, d), rtol=0, atol=TIGHT)
    for c in ROTATIONS:
        for mine, theirs in zip(PR.band_matrices(c.R), sh_rotation_matrices(c.R.astype(np.float64))):
            # both fit exactly what a rotation gives; a float32-rounded one leaves a residual of ~u that the two sample sets
            # split differently: ~u times the sets' cross-talk between bands (a few per cent).  u / 8 is a sixteenth of what
            # K_D allows the device; true rotations, below, agree to 1e-12
            assert np.abs(mine - theirs).max() < PR.U / 8, c.name
    for seed in range(4):
        R = Rot.random(random_state=seed).as_matrix()
        for mine, theirs in zip(_bands64(R), sh_rotation_matrices(R)):
            assert np.abs(mine - theirs).max() < TIGHT
    xyz, rot = PC.cloud(257, far=True, seed=1), PC.quats(257, seed=1)
    keep = np.linalg.norm(rot.astype(np.float64), axis=1) >= 1e-9     # compose_ref divides by |q| itself
    for c in CASES[::4]:
        t = rng.normal(0, 0.2, 3).astype(np.float32)
        T = np.eye(4); T[:3, :3] = c.R; T[:3, 3] = t
        ref_xyz, ref_R = compose_object_ref(xyz, rot[keep], T)
        got_xyz, mag = PR.positions(xyz, c.R, t)
        np.testing.assert_allclose(got_xyz, ref_xyz, rtol=0, atol=1e-12 * np.abs(PC.FAR).max())
        assert (mag >= np.abs(got_xyz) * (1 - 1e-6)).all()                      # the magnitude sum bounds the result
        got_R, norm = PR.orientations(rot[keep], c.R)
        np.testing.assert_allclose(got_R, ref_R, rtol=0, atol=TIGHT)
        np.testing.assert_allclose(norm, 1.0, rtol=0, atol=TIGHT)


def test_quaternion_equals_scipy_up_to_sign():
    as_wxyz = lambda s: np.array([s[3], s[0], s[1], s[2]])
    for seed in range(16):                                             # true rotations: to 1e-12
        r = Rot.random(random_state=seed)
        q, s = PR.quat_of_f64(r.as_matrix()), as_wxyz(r.as_quat())
        assert min(np.abs(q - s).max(), np.abs(q + s).max()) < TIGHT
    for c in CASES:
        q = PR.quat_of(c.R)
        s = as_wxyz(Rot.from_matrix(c.R.astype(np.float64)).as_quat())
        # a float32 matrix is off a rotation by delta; scipy and the nearest rotation each stay within a few delta of it.
        # Compared as rotations: the quaternion of a half turn flips sign under rounding
        tol = max(TIGHT, 4 * PR.non_orthonormality(c.R))
        np.testing.assert_allclose(PR.quat_matrix(q), PR.quat_matrix(s), rtol=0, atol=tol, err_msg=c.name)
        assert abs(np.linalg.norm(q) - 1) < TIGHT
        # and it IS the nearest rotation: the polar factor of R
        Uu, _, Vt = np.linalg.svd(c.R.astype(np.float64))
        np.testing.assert_allclose(PR.quat_matrix(q), Uu @ Vt, rtol=0, atol=1e-9, err_msg=c.name)


def test_small_norm_rule_and_magnitudes():
    q = PC.quats(64, seed=3)
    M, norm = PR.orientations(q, None)
    n64 = np.linalg.norm(q.astype(np.float64), axis=1)
    for k, want in enumerate(np.array(PC.QUAT_NORMS)[(np.arange(64) + 3) % 8]):
        assert n64[k] == pytest.approx(want, rel=1e-6)
        assert norm[k] == pytest.approx(1.0 if want >= 1e-12 else want / 1e-12, rel=1e-6)
        assert np.isfinite(M[k]).all()
        if want == 0:
            assert not M[k].any()
    out, mag = PR.rotate_rest(PC.coefficients(5, 8), CASES[20].R)
    assert out.shape == (5, 8, 3) and (np.abs(out) <= mag + 1e-15).all()
    out, _ = PR.positions(PC.cloud(33), None, None)
    assert np.array_equal(out, PC.cloud(33).astype(np.float64))


def test_job_tables_hold_what_the_issue_lists():
    tables = PC.job_tables()
    assert tuple(int(k) for k in tables) == PC.JOB_COUNTS
    seen = set()
    for name, jobs in tables.items():
        assert len(jobs) == int(name)
        if len(jobs) >= 3:
            assert {j.kind for j in jobs} == {PC.XYZ, PC.ROT, PC.SH}
        for j in jobs:
            assert j.src.dtype == np.float32
            if j.kind == PC.XYZ:
                seen.add(("R" if j.R is not None else "nullR", "t" if j.t is not None else "nullt", j.about_origin))
            seen.update({("rs", j.R_row_stride), ("ts", j.t_stride), ("inplace", j.kind, j.in_place), ("n", j.n)})
            if j.kind == PC.SH:
                seen.add(("n_rest", j.n_rest))
    for want in [("nullR", "t", False), ("nullR", "nullt", False), ("R", "t", True), ("R", "nullt", True), ("R", "t", False),
                 ("rs", 0), ("rs", 3), ("rs", 4), ("ts", 0), ("ts", 1), ("ts", 4), ("n_rest", 3), ("n_rest", 8), ("n_rest", 15),
                 *[("inplace", k, True) for k in (PC.XYZ, PC.ROT, PC.SH)], *[("n", n) for n in PC.SIZES]]:
        assert want in seen, want
    assert all(j.n == 0 for j in tables["48"][16:32]) and tables["17"][0].n == 0 and tables["33"][32].n == 0
    assert tables["16"][15].n == 0 and tables["32"][8].n == 0


@pytest.mark.parametrize("K", [1, 300])
def test_posed_case_meets_its_conditions_on_the_cpu(oracle, K):
    """The POSED cases of tests/test_pose_gpu.py, with the oracle alone: at most 1 % of a view's pixels are `ambig` (excluded
    from the comparison there), at least 20 % of the values show content, the poses change the picture, ids skip values and
    id-0 rows exist, and every view's table holds half turns."""
    c = PC.posed_case(K)
    ids = np.unique(c.object_id)
    assert ids[0] == 0 and (c.object_id == 0).mean() > 0.5 and c.tables.shape == (3, K, 20)
    if K == 300:
        assert len(c.parts) == 144 and not (ids[1:] % 2 == 0).any() and ids.max() < K       # even ids, 289..300: rows, no Gaussian
    names = {n: r.R for n, r in ((x.name, x) for x in CASES)}
    for v, view in enumerate(c.views):
        used = [c.poses[v][k][0] for k in c.parts]
        assert any(np.array_equal(R, names[h]) for R in used for h in names if h.startswith("180_") or h[:4] in ("180x", "180y", "180z"))
        o = oracle.forward(**c.act, sh_degree=3, **view.raster_kwargs(), num_threads=8, cull_mode=1, object_id=c.object_id,
                           poses=c.tables[v])
        plain = oracle.forward(**c.act, sh_degree=3, **view.raster_kwargs(), num_threads=8, cull_mode=1)
        ambig, content = o["ambig"].astype(bool).mean(), (o["color"] > 0.05).mean()
        print(f"K={K} view {v}: ambig {100 * ambig:.3f} %, content {100 * content:.1f} %")
        assert ambig <= 0.01 and content >= 0.20
        assert np.abs(o["color"] - plain["color"]).max() > 0.05
