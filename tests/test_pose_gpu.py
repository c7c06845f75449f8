"""The object-posing kernels (pegasus_amd/csrc/compose.hip.h) against the float64 reference of tests/pose_reference.py, per
element, over the cases of tests/pose_cases.py: pgr_compose_object (pose built on the host) and pgr_pose_objects (pose built on
the device: cloud mean, quaternion of R by Shepperd's branches, SH band matrices).  Every tolerance is a counted multiple of
u = 2^-24 (pose_reference.py) or one of the project's existing numbers; each test prints the largest error / bound it saw."""
import ctypes as C

import numpy as np
import pytest

import pose_cases as PC
import pose_reference as PR

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5                     # a quiet NaN's bit pattern: never the result of the kernels' arithmetic
GUARD = 256                               # floats before and after every output
CASES = PC.rotation_cases()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ratio(err, bound):
    """max err / bound over the elements; an element whose bound is zero must be exact."""
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    assert not err[bound == 0].any(), "an element with nothing to round is not exact"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


class Stats(dict):
    def add(self, what, value):
        self[what] = max(self.get(what, 0.0), float(value))

    def report(self, title):
        print(f"\n[{title}] largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.items())))


def guarded(dev, n_floats, fill=None):
    """int32 buffer [GUARD | n_floats | GUARD] of sentinels (``fill``: float32 values of the middle) and the middle's address."""
    import torch
    buf = torch.full((2 * GUARD + n_floats,), SENTINEL, dtype=torch.int32, device=dev)
    if fill is not None and n_floats:
        buf[GUARD:GUARD + n_floats] = torch.from_numpy(bits(fill).view(np.int32).reshape(-1)).to(dev)
    return buf, buf.data_ptr() + 4 * GUARD


def guards_intact(buf, n_floats):
    g = buf.cpu().numpy().view(np.uint32)
    return (g[:GUARD] == SENTINEL).all() and (g[GUARD + n_floats:] == SENTINEL).all()


def run_jobs(dev, jobs, one_call=True):
    """The jobs through pgr_pose_objects, in one call or one call each -> list of float32 outputs.  Checks on the way: the
    sentinel rows around every dst and the workspace bytes beyond pgr_pose_objects_workspace_bytes are unchanged."""
    import torch
    from pegasus_amd import _lib, pose_queue
    L = _lib.lib()
    dirs, pinv = pose_queue._sh_tables(dev)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    structs, keep, bufs = [], [], []
    for j in jobs:
        nf = int(j.src.size)
        if j.in_place:
            buf, dst = guarded(dev, nf, j.src)
            src = dst
        else:
            buf, dst = guarded(dev, nf)
            s = t32(j.src.reshape(-1))
            src = s.data_ptr()
            keep.append(s)
        four = None
        if j.R_row_stride == 4 or j.t_stride == 4:
            four = torch.full((4, 4), 7.0, dtype=torch.float32, device=dev)        # what is not R or t must not matter
            keep.append(four)
        Rp = tp = None
        if j.R is not None:
            if j.R_row_stride == 4:
                four[:3, :3] = t32(j.R)
                Rp = four.data_ptr()
            else:
                r = t32(j.R.reshape(-1)); keep.append(r); Rp = r.data_ptr()
        if j.t is not None:
            if j.t_stride == 4:
                four[:3, 3] = t32(j.t)
                tp = four.data_ptr() + 4 * 3
            else:
                t = t32(j.t); keep.append(t); tp = t.data_ptr()
        structs.append(_lib.PgrPoseJob(src=src, dst=dst, R=Rp, t=tp, n=j.n, kind=j.kind, n_rest=j.n_rest,
                                       about_origin=int(j.about_origin), R_row_stride=j.R_row_stride, t_stride=j.t_stride))
        bufs.append(buf)
    calls = [structs] if one_call else [[s] for s in structs]
    for call in calls:
        need = int(L.pgr_pose_objects_workspace_bytes(len(call)))
        assert need > 0
        ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        arr = (_lib.PgrPoseJob * len(call))(*call)
        _lib.check(L.pgr_pose_objects(len(call), arr, _lib.ptr(dirs), _lib.ptr(pinv), _lib.ptr(ws), int(ws.numel()),
                                      _lib.stream_ptr(dev)), "pgr_pose_objects")
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all().item(), "bytes beyond pgr_pose_objects_workspace_bytes were written"
    outs = []
    for k, (j, buf) in enumerate(zip(jobs, bufs)):
        nf = int(j.src.size)
        assert guards_intact(buf, nf), f"job {k} ({j.note}): guard rows around dst changed"
        outs.append(buf[GUARD:GUARD + nf].cpu().numpy().view(np.float32).reshape(j.src.shape))
    return outs


def check_orientation(src, R, got, stats, what):
    want, want_norm = PR.orientations(src, R)
    g = got.astype(np.float64)
    assert np.isfinite(g).all(), what
    norm = np.linalg.norm(g, axis=1)
    zero = want_norm == 0
    assert not g[zero].any(), f"{what}: the zero quaternion must give exactly zero"
    nz = ~zero
    # unit norm within the project's 1e-6 for |q| >= 1e-12; below, the reference's q / 1e-12, scaled accordingly
    stats.add("norm", ratio(np.abs(norm[nz] - want_norm[nz]), PR.UNIT_ATOL * want_norm[nz]))
    assert (np.abs(norm[nz] - want_norm[nz]) <= PR.UNIT_ATOL * want_norm[nz]).all(), what
    M = PR.quat_matrix(g[nz] / norm[nz, None])
    err = np.abs(M - want[nz] / (want_norm[nz] ** 2)[:, None, None])
    bound = PR.ORIENT_ATOL if R is None else PR.orient_bound(R)
    stats.add("orientation", ratio(err, bound))
    assert (err <= bound).all(), (what, err.max(), bound)


def check_job(j, got, stats, what):
    if j.hostile:
        return
    what = f"{what}: {('xyz', 'rot', 'sh')[j.kind]} n={j.n} {j.note}"
    if j.kind == PC.XYZ:
        if j.R is None:
            want = j.src if j.t is None else j.src + j.t[None, :]        # float32 arithmetic: bit for bit
            assert np.array_equal(bits(got), bits(want)), what
            return
        want, mag = PR.positions(j.src, j.R, j.t, j.about_origin)
        err, bound = np.abs(got.astype(np.float64) - want), PR.K_XYZ * PR.U * mag
        stats.add("xyz", ratio(err, bound))
        assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
    elif j.kind == PC.ROT:
        check_orientation(j.src, j.R, got, stats, what)
    else:
        want, mag = PR.rotate_rest(j.src, j.R)
        err, bound = np.abs(got.astype(np.float64) - want), PR.K_SH * PR.U * mag
        stats.add("sh", ratio(err, bound))
        assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))


# ---- the device-built pose, read back through the kernel ----------------------------------------------------------------

def test_device_built_quaternion_and_band_matrices(gpu_device):
    """A ROT job on the row (1,0,0,0) returns the device's quaternion of R bit for bit; an SH job on the 15 unit rows returns
    the columns of D1, D2, D3.  Every rotation case, three row strides, in ONE call (2 x 53 jobs: seven launches)."""
    one = np.array([[1, 0, 0, 0]], np.float32)
    jobs = []
    for k, c in enumerate(CASES):
        jobs.append(PC.Job(PC.ROT, one, c.R, None, R_row_stride=(0, 3, 4)[k % 3], note=c.name))
        jobs.append(PC.Job(PC.SH, PC.unit_rows(15), c.R, None, R_row_stride=(4, 0, 3)[k % 3], note=c.name))
    outs = run_jobs(gpu_device, jobs)
    stats = Stats()
    for k, c in enumerate(CASES):
        q = outs[2 * k][0].astype(np.float64)
        stats.add("|q|-1", abs(np.linalg.norm(q) - 1) / (2 * PR.U))
        assert abs(np.linalg.norm(q) - 1) <= 2 * PR.U, c.name          # four components each rounded once: 1 u, and one spare
        err = np.abs(PR.quat_matrix(q / np.linalg.norm(q)) - PR.quat_matrix(PR.quat_of(c.R)))
        # two regimes, reported apart: 8 u for a float32-rounded rotation, the counted allowance for the accumulated trajectory
        rounded = PR.non_orthonormality(c.R) <= 2 * PR.U
        assert rounded == (c.name != "accumulated_1000") and (not rounded or PR.quat_bound(c.R) == PR.K_QUAT * PR.U)
        stats.add("quaternion" if rounded else "quaternion (accumulated)", ratio(err, PR.quat_bound(c.R)))
        assert (err <= PR.quat_bound(c.R)).all(), (c.name, sorted(PR.census(c.R)), err.max(), PR.quat_bound(c.R))
        e = outs[2 * k + 1]                                            # e[k, i, ch] = D[i, k] inside a band, 0 outside
        assert np.array_equal(bits(e[:, :, 0]), bits(e[:, :, 1])) and np.array_equal(bits(e[:, :, 0]), bits(e[:, :, 2]))
        cols = e[:, :, 0].astype(np.float64).T                         # [i, k]
        for D, (lo, hi) in zip(PR.band_matrices(c.R), ((0, 3), (3, 8), (8, 15))):
            err = np.abs(cols[lo:hi, lo:hi] - D)
            stats.add("D", ratio(err, PR.K_D * PR.U))
            assert (err <= PR.K_D * PR.U).all(), (c.name, lo, err.max())
            cols[lo:hi, lo:hi] = 0
        assert not cols.any(), f"{c.name}: a band matrix leaks into another band"
    stats.report("device-built pose")


def test_device_built_centre_at_every_size(gpu_device):
    """An XYZ job with the all-zero matrix as R and no t returns the device's cloud mean in every row: every size at a block and
    a partition edge and 2 000 003 rows, at the origin and far from it, in one call."""
    zero = np.zeros((3, 3), np.float32)
    jobs = [PC.Job(PC.XYZ, PC.cloud(n, far=far, seed=n % 97), zero, None, note=f"far={far}")
            for far in (False, True) for n in PC.SIZES + (PC.BIG,)]
    outs = run_jobs(gpu_device, jobs)
    stats = Stats()
    for j, got in zip(jobs, outs):
        if not j.n:
            continue
        assert (bits(got) == bits(got[0])[None, :]).all(), "every row holds the one centre"
        c = PR.center_of(j.src)
        err, bound = np.abs(got[0].astype(np.float64) - c), PR.U * np.abs(c) + PR.CENTER_ABS
        stats.add("centre", ratio(err, bound))
        assert (err <= bound).all(), (j.n, j.note, err, bound)
    stats.report("device-built centre")


# ---- pgr_pose_objects: the job tables ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [str(c) for c in PC.JOB_COUNTS])
def test_job_table_matches_the_reference(gpu_device, name):
    jobs = PC.job_tables()[name]
    first = run_jobs(gpu_device, jobs)
    stats = Stats()
    for k, (j, got) in enumerate(zip(jobs, first)):
        check_job(j, got, stats, f"table {name} job {k}")
    stats.report(f"pgr_pose_objects, {name} jobs")
    # the same call twice gives the same bits (the mean is summed in a fixed order)
    again = run_jobs(gpu_device, jobs)
    # src == dst equals out of place, bit for bit
    flipped = PC.job_tables()[name]
    for j in flipped:
        j.in_place = not j.in_place
    other = run_jobs(gpu_device, flipped)
    # and the jobs issued one call each: job 17 of a call is job 1 of its launch, with its own workspace segment
    alone = run_jobs(gpu_device, jobs, one_call=False) if len(jobs) > 16 else first
    for k, (a, b, c, d) in enumerate(zip(first, again, other, alone)):
        assert np.array_equal(bits(a), bits(b)), f"table {name} job {k}: a second run differs"
        assert np.array_equal(bits(a), bits(c)), f"table {name} job {k}: in place differs from out of place"
        assert np.array_equal(bits(a), bits(d)), f"table {name} job {k}: one call differs from a call of its own"


def test_null_rotation_keeps_rows_it_cannot_represent(gpu_device):
    """R = NULL is the identity, not a multiplication by one and zeros: rows holding Inf, -0.0 or denormals come back as
    x + t in float32, bit for bit, and as themselves without t."""
    x = PC.cloud(300, seed=8)
    x[5, 0], x[6, 1], x[7, 2], x[8, 0], x[9] = np.inf, -np.inf, -0.0, 1e-42, (np.inf, -np.inf, 3.0)
    t = np.array([0.25, -1.5, 0.0], np.float32)
    jobs = [PC.Job(PC.XYZ, x, None, t), PC.Job(PC.XYZ, x, None, None), PC.Job(PC.XYZ, x, None, t, in_place=True, t_stride=4)]
    with np.errstate(invalid="ignore"):
        want = x + t[None, :]
    got = run_jobs(gpu_device, jobs)
    assert np.array_equal(bits(got[0]), bits(want))
    assert np.array_equal(bits(got[1]), bits(x))
    assert np.array_equal(bits(got[2]), bits(want))


# ---- pgr_compose_object ----------------------------------------------------------------------------------------------

def compose_case(dev, n, R, t, n_rest, far, seed, in_pad=0, merged=False, in_place=False):
    """One pgr_compose_object call on guarded buffers -> (inputs, outputs, pose).  merged: out_rest points into an [n,16,3]
    buffer (stride 48, column 0 and the slots above 3 n_rest hold sentinels)."""
    import torch
    from pegasus_amd import _lib, compose
    L = _lib.lib()
    xyz, rot, rest = PC.cloud(n, far=far, seed=seed), PC.quats(n, seed=seed), PC.coefficients(n, n_rest, seed=seed)
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    pose = compose.make_pose(T, PR.center_of(xyz))
    in_stride = 3 * n_rest + in_pad
    padded = np.full((n, in_stride), np.float32(123.0), np.float32)
    padded[:, :3 * n_rest] = rest.reshape(n, 3 * n_rest)
    out_stride = 48 if merged else 3 * n_rest
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    bx, px = guarded(dev, 3 * n, xyz if in_place else None)
    bq, pq = guarded(dev, 4 * n, rot if in_place else None)
    br, pr = guarded(dev, out_stride * n, padded if in_place and not merged and not in_pad else None)
    sx, sq, sr = t32(xyz), t32(rot), t32(padded)
    src = (px, pq, pr) if in_place else (sx.data_ptr(), sq.data_ptr(), sr.data_ptr())
    v = lambda a: C.c_void_p(a)
    rest_ptr = (v(src[2]), v(pr + (12 if merged else 0))) if n_rest else (None, None)
    _lib.check(L.pgr_compose_object(n, v(src[0]), v(src[1]), rest_ptr[0], n_rest, in_stride, C.byref(pose), v(px), v(pq),
                                    rest_ptr[1], out_stride, _lib.stream_ptr(dev)), "pgr_compose_object")
    torch.cuda.synchronize()
    assert guards_intact(bx, 3 * n) and guards_intact(bq, 4 * n) and guards_intact(br, out_stride * n)
    grab = lambda b, m: b[GUARD:GUARD + m].cpu().numpy().view(np.float32)
    o_rest = grab(br, out_stride * n).reshape(n, out_stride)
    if merged:                                          # everything outside columns 1..n_rest of the [n,16,3] rows is untouched
        assert (bits(o_rest[:, :3]) == SENTINEL).all() and (bits(o_rest[:, 3 + 3 * n_rest:]) == SENTINEL).all()
        o_rest = o_rest[:, 3:3 + 3 * n_rest]
    return (xyz, rot, rest), (grab(bx, 3 * n).reshape(n, 3), grab(bq, 4 * n).reshape(n, 4), o_rest.reshape(n, n_rest, 3)), pose


def check_compose(inputs, outputs, pose, R, t, stats, what):
    xyz, rot, rest = inputs
    o_xyz, o_rot, o_rest = outputs
    want, mag = PR.positions(xyz, R, t, center=np.array(list(pose.center), np.float32))
    err, bound = np.abs(o_xyz.astype(np.float64) - want), PR.K_XYZ * PR.U * mag
    stats.add("xyz", ratio(err, bound))
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
    check_orientation(rot, R, o_rot, stats, what)
    want, mag = PR.rotate_rest(rest, R)
    err, bound = np.abs(o_rest.astype(np.float64) - want), PR.K_SH * PR.U * mag
    stats.add("sh", ratio(err, bound))
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))


def test_compose_object_every_rotation(gpu_device):
    stats = Stats()
    rng = np.random.default_rng(31)
    for k, c in enumerate(CASES):
        t = rng.normal(0, 0.2, 3).astype(np.float32)
        ins, outs, pose = compose_case(gpu_device, 257, c.R, t, 15, far=k % 2 == 1, seed=k)
        check_compose(ins, outs, pose, c.R, t, stats, c.name)
    stats.report("pgr_compose_object, every rotation")


@pytest.mark.parametrize("n_rest", PC.N_RESTS)
def test_compose_object_sizes_strides_and_containment(gpu_device, n_rest):
    from pegasus_amd import _lib
    stats = Stats()
    rng = np.random.default_rng(32)
    for k, n in enumerate(PC.SIZES):
        c = CASES[(7 * k + n_rest) % len(CASES)]
        t = rng.normal(0, 0.2, 3).astype(np.float32)
        kw = dict(n=n, R=c.R, t=t, n_rest=n_rest, far=k % 2 == 0, seed=50 + k)
        plain = compose_case(gpu_device, **kw)
        if n:
            check_compose(*plain, c.R, t, stats, f"n={n} {c.name}")
        # a padded input stride, output into the merged [n,16,3] rows, and in place: the same bits
        for other in (compose_case(gpu_device, in_pad=5, merged=True, **kw), compose_case(gpu_device, in_place=True, **kw)):
            for a, b in zip(plain[1], other[1]):
                assert np.array_equal(bits(a), bits(b)), (n, c.name)
    stats.report(f"pgr_compose_object, n_rest={n_rest}")
    assert _lib.lib().pgr_compose_object(0, None, None, None, 0, 0, C.byref(plain[2]), None, None, None, 0, None) == _lib.PGR_OK


# ---- the POSED branch of the preprocess ---------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 300])
def test_posed_preprocess_at_the_edge_rotations(oracle, gpu_device, K):
    """forward_views(..., posed=...) with half turns and the branch cases in every view's table (tests/pose_cases.py
    posed_case: K = 1 and K = 300 with ids that skip values, three views with different tables, id-0 rows): radii equal to the
    oracle's bit for bit, colour and depth within the project's 1e-4 outside the oracle's `ambig` pixels (at most 1 % of a
    view; at least 20 % of the values show content: both also asserted on the CPU, tests/test_pose_host.py).  Then the posed
    image against the unposed image of pgr_compose_object's output for the same poses, with the thresholds of
    test_compose.py::test_posed_objects_equal_composed_scene."""
    import torch
    from pegasus_amd import compose, rasterizer as RZ
    c = PC.posed_case(K)
    dev = gpu_device
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    specs = [RZ.ViewSpec(v.height, v.width, v.tanfovx, v.tanfovy, t(np.zeros(3, np.float32)), t(v.world_view_transform),
                         t(v.full_proj_transform), t(v.camera_center)) for v in c.views]
    scene = {k: t(c.act[k]) for k in ("means3d", "opacities", "shs", "scales", "rotations")}
    render = lambda s, sp, **kw: RZ.forward_views(s["means3d"], s["opacities"], sp, shs=s["shs"], scales=s["scales"],
                                                  rotations=s["rotations"], sh_degree=3, want_radii=True, want_aux=True, **kw)
    res = render(scene, specs, posed=dict(object_id=t(c.object_id, torch.int32), poses=t(c.tables)))
    torch.cuda.synchronize()
    worst = Stats()
    for v, (r, view) in enumerate(zip(res, c.views)):
        o = oracle.forward(**c.act, sh_degree=3, **view.raster_kwargs(), num_threads=8, cull_mode=1, object_id=c.object_id,
                           poses=c.tables[v])
        np.testing.assert_array_equal(r["radii"].cpu().numpy(), o["radii"])
        amb = o["ambig"].astype(bool)
        assert amb.mean() <= 0.01 and (o["color"] > 0.05).mean() >= 0.20
        dc = np.abs(r["color"].cpu().numpy() - o["color"])[:, ~amb].max()
        dd = np.abs(r["depth"].cpu().numpy() - o["out_depth"])[:, ~amb].max()
        worst.add("colour", dc / 1e-4); worst.add("depth", dd / 1e-4)
        assert dc <= 1e-4 and dd <= 1e-4, (v, dc, dd)
        # the same poses applied by pgr_compose_object, part by part, and rendered without poses
        comp = {k: a.clone() for k, a in scene.items()}
        for k, (sel, center) in c.parts.items():
            R, tr = c.poses[v][k]
            T = np.eye(4); T[:3, :3] = R; T[:3, 3] = tr
            idx = t(sel, torch.int64)
            n = len(sel)
            xyz, rot, rest = (torch.empty((n, 3), device=dev), torch.empty((n, 4), device=dev),
                              torch.empty((n, 15, 3), device=dev))
            compose.compose_object(scene["means3d"][idx].contiguous(), scene["rotations"][idx].contiguous(),
                                   scene["shs"][idx, 1:].contiguous(), compose.make_pose(T, center), xyz, rot, rest)
            comp["means3d"][idx], comp["rotations"][idx] = xyz, rot
            comp["shs"][idx, 1:] = rest
        b = render(comp, [specs[v]])[0]
        torch.cuda.synchronize()
        diff = (r["color"] - b["color"]).abs().cpu().numpy()
        assert np.percentile(diff, 99.5) < 2e-3 and (diff > 2e-2).mean() < 2e-3, (v, diff.max(), (diff > 2e-2).mean())
        assert (r["depth"] - b["depth"]).abs().mean().item() < 1e-3
        assert int((r["radii"] > 0).sum()) == pytest.approx(int((b["radii"] > 0).sum()), rel=0.01)
        worst.add("posed vs composed p99.5", np.percentile(diff, 99.5) / 2e-3)
    worst.report(f"POSED preprocess, K={K}")
