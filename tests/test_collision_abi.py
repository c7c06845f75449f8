"""pgr_mesh_sdf, pgr_sdf_sample, pgr_sdf_sweep without a device: the symbols stand in the header, the library and _lib.SYMBOLS;
every misuse is PGR_ERR_INVALID_ARGUMENT from host-side checks before any launch (fake non-NULL device pointers are never
dereferenced); empty inputs answer PGR_OK; the wrappers refuse host tensors; the command line has its flags."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("pgr_mesh_sdf", "pgr_sdf_sample", "pgr_sdf_sweep")
FAKE = C.c_void_p(0x1000)


def _lib():
    from pegasus_amd import _lib as L
    return L


def _grid(L, nx=4, ny=5, nz=6, voxel=0.1):
    return L.PgrGrid(nx=nx, ny=ny, nz=nz, origin=(C.c_float * 3)(0, 0, 0), voxel=voxel)


def test_symbols_stand_in_the_header_the_library_and_the_binding():
    L = _lib()
    header = (ROOT / "include" / "pegasus_raster.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in L.SYMBOLS and hasattr(L.lib(), name)
        assert L.SYMBOLS[name][1][-1] is C.c_void_p                                   # the stream comes last
    assert L.lib().pgr_abi_version() == 4
    assert f"#define PGR_SDF_FACE_TILE {L.PGR_SDF_FACE_TILE}" in header and f"#define PGR_SWEEP_PLANE ({L.PGR_SWEEP_PLANE})" in header
    import collision_cases as CC
    assert CC.FACE_TILE == L.PGR_SDF_FACE_TILE
    # the structs are the header's: 28-byte grid, then pointers at 8-byte alignment
    assert C.sizeof(L.PgrSdfBody) == 104 and L.PgrSdfBody.sdf.offset == 32 and L.PgrSdfBody.R.offset == 52
    assert C.sizeof(L.PgrSweepJob) == 36


def test_mesh_sdf_rejects_misuse_before_any_launch():
    L = _lib()
    lib, bad = L.lib(), L.PGR_ERR_INVALID_ARGUMENT
    g = _grid(L)
    assert lib.pgr_mesh_sdf(8, FAKE, 12, FAKE, None, FAKE, None, None) == bad                 # no grid
    assert lib.pgr_mesh_sdf(8, FAKE, 12, FAKE, C.byref(g), None, None, None) == bad           # no output
    assert lib.pgr_mesh_sdf(8, None, 12, FAKE, C.byref(g), FAKE, None, None) == bad           # faces without vertices
    assert lib.pgr_mesh_sdf(8, FAKE, 12, None, C.byref(g), FAKE, None, None) == bad           # no faces
    assert lib.pgr_mesh_sdf(-1, FAKE, 12, FAKE, C.byref(g), FAKE, None, None) == bad
    assert lib.pgr_mesh_sdf(8, FAKE, -1, FAKE, C.byref(g), FAKE, None, None) == bad
    for kw in (dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=1025), dict(voxel=0.0), dict(voxel=float("nan"))):
        assert lib.pgr_mesh_sdf(8, FAKE, 12, FAKE, C.byref(_grid(L, **kw)), FAKE, None, None) == bad, kw


def test_sdf_sample_rejects_misuse_and_takes_nothing():
    L = _lib()
    lib, bad = L.lib(), L.PGR_ERR_INVALID_ARGUMENT
    g = _grid(L)
    assert lib.pgr_sdf_sample(None, FAKE, 4, FAKE, FAKE, None, None) == bad
    assert lib.pgr_sdf_sample(C.byref(g), None, 4, FAKE, FAKE, None, None) == bad
    assert lib.pgr_sdf_sample(C.byref(g), FAKE, -1, FAKE, FAKE, None, None) == bad
    assert lib.pgr_sdf_sample(C.byref(g), FAKE, 4, None, FAKE, None, None) == bad
    assert lib.pgr_sdf_sample(C.byref(g), FAKE, 4, FAKE, None, None, None) == bad
    assert lib.pgr_sdf_sample(C.byref(_grid(L, nz=1)), FAKE, 4, FAKE, FAKE, None, None) == bad
    assert lib.pgr_sdf_sample(C.byref(g), FAKE, 0, None, None, None, None) == L.PGR_OK          # nothing to do


def _body(L, sdf=FAKE, shell=FAKE, n_shell=10, **grid):
    eye = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    return L.PgrSdfBody(grid=_grid(L, **grid), sdf=sdf, shell=shell, n_shell=n_shell, R=eye, t=(C.c_float * 3)(0, 0, 0))


def _job(L, mover=0, target=1, direction=(0, 0, -1), plane=(0, 0, 1, 0)):
    return L.PgrSweepJob(mover=mover, target=target, dir=(C.c_float * 3)(*direction), plane=(C.c_float * 4)(*plane))


def _sweep(L, bodies, jobs, tol=1e-4, max_travel=1.0, max_steps=8, out=FAKE, n_bodies=None, n_jobs=None):
    b = (L.PgrSdfBody * max(1, len(bodies)))(*bodies)
    j = (L.PgrSweepJob * max(1, len(jobs)))(*jobs)
    return L.lib().pgr_sdf_sweep(len(bodies) if n_bodies is None else n_bodies, b, len(jobs) if n_jobs is None else n_jobs, j,
                                 tol, max_travel, max_steps, out, None)


def test_sdf_sweep_rejects_misuse_before_any_launch():
    L = _lib()
    bad = L.PGR_ERR_INVALID_ARGUMENT
    two = [_body(L), _body(L)]
    assert L.lib().pgr_sdf_sweep(2, None, 1, (L.PgrSweepJob * 1)(_job(L)), 1e-4, 1.0, 8, FAKE, None) == bad      # no bodies
    assert L.lib().pgr_sdf_sweep(2, (L.PgrSdfBody * 2)(*two), 1, None, 1e-4, 1.0, 8, FAKE, None) == bad          # no jobs
    assert _sweep(L, two, [_job(L)], out=None) == bad
    assert _sweep(L, two, [_job(L)], n_bodies=-1) == bad
    assert _sweep(L, two, [_job(L)], n_jobs=-1) == bad
    assert _sweep(L, two, [_job(L)], max_steps=-1) == bad
    for tol in (float("nan"), -1.0):
        assert _sweep(L, two, [_job(L)], tol=tol) == bad
    for travel in (float("nan"), -1.0):
        assert _sweep(L, two, [_job(L)], max_travel=travel) == bad
    # a job naming a body outside the table, or itself, or a target below the plane's index
    for mover, target in ((2, 1), (-1, 1), (0, 2), (0, -2), (1, 1)):
        assert _sweep(L, two, [_job(L), _job(L, mover, target)]) == bad, (mover, target)
    # a direction that is not a unit vector
    for d in ((0, 0, 0), (0, 0, -1.01), (0, 0, -0.5), (float("nan"), 0, -1), (float("inf"), 0, 0)):
        assert _sweep(L, two, [_job(L, direction=d)]) == bad, d
    # a plane whose normal is not one, or whose offset is not finite
    for pl in ((0, 0, 0, 0), (0, 0, 2, 0), (0, 0, 1, float("nan"))):
        assert _sweep(L, two, [_job(L, target=L.PGR_SWEEP_PLANE, plane=pl)]) == bad, pl
    # a target without a field or with a grid that has an axis < 2; a shell that is missing or negative
    assert _sweep(L, [_body(L), _body(L, sdf=None)], [_job(L)]) == bad
    assert _sweep(L, [_body(L), _body(L, ny=1)], [_job(L)]) == bad
    assert _sweep(L, [_body(L, shell=None), _body(L)], [_job(L)]) == bad
    assert _sweep(L, [_body(L, n_shell=-1), _body(L)], [_job(L)]) == bad


def test_sdf_sweep_empty_inputs_are_ok():
    L = _lib()
    assert _sweep(L, [], []) == L.PGR_OK
    assert _sweep(L, [_body(L), _body(L)], [], out=None) == L.PGR_OK
    assert L.lib().pgr_sdf_sweep(0, None, 0, None, 1e-4, 1.0, 8, None, None) == L.PGR_OK
    # a body that is never a target needs no field; the unit check allows the rounding of a normalised float32 vector
    d = np.array([0.3, -0.2, -0.9], np.float64)
    d = (d / np.linalg.norm(d)).astype(np.float32)
    assert abs(math.sqrt(float((d.astype(np.float64) ** 2).sum())) - 1) < 1e-6
    assert _sweep(L, [], [_job(L, direction=tuple(d))], n_jobs=0) == L.PGR_OK


def test_wrappers_refuse_host_tensors():
    import torch
    from pegasus_amd import collision as COL
    from pegasus_amd.mesh import Grid, Mesh
    import collision_cases as CC
    v, f = CC.cube()
    grid = Grid(4, 4, 4, (0.0, 0.0, 0.0), 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        COL.mesh_sdf(torch.from_numpy(v), torch.from_numpy(f), grid)
    with pytest.raises(RuntimeError, match="no CPU path"):
        COL.sdf_sample(torch.zeros(4, 4, 4), grid, torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        COL.MeshSDF.from_mesh(Mesh(v, f), resolution=8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        COL.MeshSDF(grid, torch.zeros(4, 4, 4)).signed_distance(torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        COL.CollisionBody(Mesh(v, f), COL.MeshSDF(grid, torch.zeros(4, 4, 4)), shell=torch.zeros(3, 3))
    # the field is brute force: the wrapper says so where it refuses
    big = np.zeros((COL.MAX_FACES + 1, 3), np.int32)
    with pytest.raises(ValueError, match="brute force"):
        COL.MeshSDF.from_mesh((v, big), resolution=8, device="cuda")


def test_command_line_flags_and_defaults():
    from pegasus_amd import collision as COL
    a = COL._parser().parse_args(["--models", "m", "--objects", "1", "2", "5", "--out", "steps.json"])
    assert a.objects == [1, 2, 5] and a.count == 1 and a.seed == 0 and a.radius is None and a.out == "steps.json"
    assert a.check is None and a.scale == 1.0 and a.resolution == 96 and a.tol == 1e-4 and a.steps == 1
    b = COL._parser().parse_args(["--check", "dataset", "--models", "m", "--count", "3", "--seed", "7", "--radius", "0.25"])
    assert b.check == "dataset" and b.objects is None and (b.count, b.seed, b.radius) == (3, 7, 0.25)
    with pytest.raises(SystemExit):
        COL._parser().parse_args(["--out", "x.json"])                                # --models is required
    with pytest.raises(SystemExit):
        COL.main(["--models", "m"])                                                  # neither --out nor --check
