"""Mesh extraction on the device: pgr_tsdf_integrate and pgr_march_count / pgr_march_emit against the NumPy reference
(tests/mesh_reference.py), closed meshes from analytic images and from rendered Gaussian models, and the CLI.  The
second half pins the kernels where the first case does not reach: the scan over many tiles up to the default 256^3, a
surface through the grid's border, dense and hostile fields, the workspace contract, and the TSDF kernel's skip branches
against an independent float64 oracle (inputs from tests/mesh_cases.py, shared with the host tests)."""
import ctypes as C
import json
import math
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import mesh_cases as MC
import mesh_reference as R
from mesh_reference import assert_watertight, components

pytestmark = pytest.mark.gpu


def device_specs(raw):
    """The ViewSpecs of NumPy views, on the device."""
    import torch
    from pegasus_amd.rasterizer import ViewSpec
    dev = lambda a: torch.as_tensor(np.asarray(a, np.float32), device="cuda")
    return [ViewSpec(v.height, v.width, v.tanfovx, v.tanfovy, dev(np.zeros(3)), dev(v.world_view_transform),
                     dev(v.full_proj_transform), dev(v.camera_center), depth_mode=1) for v in raw]


def views_around(center, dist, n, width, height, fovx, fovy):
    """n look-at views on the full Fibonacci sphere of radius ``dist`` around ``center``: (ViewSpecs, numpy View)."""
    raw = MC.raw_views_around(center, dist, n, width, height, fovx, fovy)
    return device_specs(raw), raw


def synthetic_case():
    c = MC.synthetic_tsdf_case()
    return c.grid, device_specs(c.raw), c.raw, c.depth, c.final_T


def run_integrate(grid, specs, depth, final_T, trunc, amin):
    import torch
    from pegasus_amd.mesh import integrate
    return integrate(torch.as_tensor(depth, device="cuda"), torch.as_tensor(final_T, device="cuda"), specs, grid, trunc,
                     amin).cpu().numpy()


def test_tsdf_integrate_matches_the_reference():
    grid, specs, raw, depth, final_T = synthetic_case()
    trunc, amin = 3.0 * grid.voxel, 0.5
    got = run_integrate(grid, specs, depth, final_T, trunc, amin)
    want, ambiguous = R.tsdf_reference(grid, [v.world_view_transform.reshape(16) for v in raw],
                                       [v.tanfovx for v in raw], [v.tanfovy for v in raw], depth, final_T, trunc, amin,
                                       return_ambiguous=True)
    # a point is excluded only where a projection within 1e-4 px of a pixel boundary could explain a difference; with
    # 14 rounded coordinates per point about 0.3 % of the points have one, and every other point must match
    differs = np.abs(got - want) > 1e-6
    excluded = differs & ambiguous
    assert excluded.mean() < 0.001, excluded.mean()
    keep = ~excluded
    np.testing.assert_allclose(got[keep], want[keep], rtol=0, atol=1e-6)
    # the case exercises every branch: carved, fused, unseen
    assert (want == 1.0).mean() > 0.05 and (want == -1.0).mean() > 0.0 and (np.abs(want) < 1.0).mean() > 0.05


def test_march_matches_the_reference_and_repeats_bit_for_bit():
    import torch
    from pegasus_amd.mesh import march
    grid, specs, raw, depth, final_T = synthetic_case()
    sdf = run_integrate(grid, specs, depth, final_T, 3.0 * grid.voxel, 0.5)
    v_ref, f_ref = R.march_reference(sdf, grid)
    assert len(f_ref) > 1000
    dev = torch.as_tensor(sdf, device="cuda")
    a = march(dev, grid)
    b = march(dev, grid)
    np.testing.assert_array_equal(a.faces, f_ref)
    np.testing.assert_allclose(a.vertices, v_ref, rtol=0, atol=1e-6 * grid.voxel)
    assert a.vertices.tobytes() == b.vertices.tobytes() and a.faces.tobytes() == b.faces.tobytes()
    assert_watertight(a.faces)


def sphere_images(raw, c_world, r, W, H):
    """Ray-traced depth (view-space z of the first hit) and final_T (0 on the sphere, 1 off it)."""
    depth = np.zeros((len(raw), H, W), np.float32)
    final_T = np.ones((len(raw), H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for k, v in enumerate(raw):
        M = v.world_view_transform.astype(np.float64).T                 # world -> view (column vectors)
        c = M[:3, :3] @ c_world + M[:3, 3]
        fx, fy = W / (2 * v.tanfovx), H / (2 * v.tanfovy)
        d = np.stack([(xx - (W - 1) / 2) / fx, (yy - (H - 1) / 2) / fy, np.ones_like(xx)], axis=-1)     # z = 1
        a = (d * d).sum(-1)
        b = (d * c).sum(-1)
        disc = b * b - a * (c @ c - r * r)
        hit = disc > 0
        t = (b - np.sqrt(np.where(hit, disc, 0))) / a
        depth[k] = np.where(hit, t, 0)
        final_T[k] = np.where(hit, 0.0, 1.0)
    return depth, final_T


def test_analytic_sphere_end_to_end():
    from pegasus_amd.mesh import Grid, Mesh, march, integrate
    import torch
    r, c = 0.3, np.array([0.05, -0.02, 0.01])
    grid = Grid.around(c - 0.4, c + 0.4, 64)
    W = H = 256
    specs, raw = views_around(c, 1.5, 32, W, H, math.radians(40.0), math.radians(40.0))
    assert len(specs) == 32
    depth, final_T = sphere_images(raw, c, r, W, H)
    sdf = integrate(torch.as_tensor(depth, device="cuda"), torch.as_tensor(final_T, device="cuda"), specs, grid,
                    4.0 * grid.voxel, 0.5)
    m = march(sdf, grid)
    n_edges = assert_watertight(m.faces)
    assert len(m.vertices) - n_edges + len(m.faces) == 2
    assert components(len(m.vertices), m.faces) == 1
    # Carving sets +1 outside, not a distance, while a point just inside holds -depth/truncation: the crossing is
    # interpolated towards the inside point, so the surface sits up to about a voxel inside the sphere (1.19 voxel and
    # -4.2 % volume at 4 voxels of truncation, in the reference as on the device; 256^2 and 768^2 images agree).  The
    # outward error stays below a quarter voxel.
    rad = np.linalg.norm(m.vertices.astype(np.float64) - c, axis=1)
    assert (rad - r).max() < 0.5 * grid.voxel and (rad - r).min() > -1.25 * grid.voxel, (rad - r).min() / grid.voxel
    assert -0.05 < Mesh(m.vertices, m.faces).volume() / (4 / 3 * math.pi * r ** 3) - 1 < 0.0


def box_model(seed=11, n=40_000, dims=(0.06, 0.16, 0.21)):
    from pegasus_amd import scenes
    from pegasus_amd.gaussian_model import GaussianModel
    cloud = scenes.box_object(np.random.default_rng(seed), n, dims, math.log(0.002), 0.4, 0.15, object_id=1)
    return GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling,
                                     cloud.rotation), cloud


def test_box_object_through_the_renderer():
    from pegasus_amd.mesh import extract_mesh
    dims = np.array([0.06, 0.16, 0.21])
    model, cloud = box_model(dims=tuple(dims))
    resolution = 96
    m = extract_mesh(model, resolution=resolution, n_views=48, image_size=256)
    assert_watertight(m.faces)
    assert components(len(m.vertices), m.faces) == 1
    lo, hi = m.vertices.min(axis=0), m.vertices.max(axis=0)
    voxel = 1.2 * dims.max() / (resolution - 1)                         # the default bounds: +10 % of 0.21 on each side
    med_scale = float(np.median(np.exp(cloud.scaling)))
    ratio = m.volume() / np.prod(dims)
    info = dict(lo=lo, hi=hi, voxel=voxel, med_scale=med_scale, volume_ratio=ratio)
    # every face of the mesh's box lies within 2 voxels + 3 median scales of the box's face (the splats of a face reach
    # past its edges)
    assert np.all(np.abs(lo + dims / 2) < 2 * voxel + 3 * med_scale), info
    assert np.all(np.abs(hi - dims / 2) < 2 * voxel + 3 * med_scale), info
    # The fused surface is the outer envelope of the splats, which reach about two median scales past every face.  On
    # this 6 cm slab that layer alone adds ~10 % along the thin axis; the first device run measured +19.7 % in all, so
    # the bound is 25 % rather than the 10 % a mesh of the Gaussian centres would meet.
    assert abs(ratio - 1) < 0.25, info


def test_cli_writes_bop_model_and_urdf(tmp_path):
    from pegasus_amd import mesh as M
    from pegasus_amd.ply_io import read_ply_mesh
    model, _ = box_model(seed=12, n=20_000)
    model.save_ply(tmp_path / "model" / "point_cloud" / "iteration_30" / "point_cloud.ply")
    out = tmp_path / "out"
    (out / "models").mkdir(parents=True)
    (out / "models" / "models_info.json").write_text(json.dumps({"1": {"diameter": 1.0}}))
    assert M.main(["-m", str(tmp_path / "model"), "--out", str(out), "--obj_id", "3", "--scale", "1000", "--mass", "0.2",
                   "--resolution", "64", "--n_views", "32", "--image_size", "192"]) == 0
    v, f = read_ply_mesh(out / "models" / "obj_000003.ply")
    info = json.loads((out / "models" / "models_info.json").read_text())
    assert set(info) == {"1", "3"} and info["1"] == {"diameter": 1.0}
    ext = v.max(axis=0).astype(np.float64) - v.min(axis=0)
    np.testing.assert_allclose(ext, [info["3"][f"size_{a}"] for a in "xyz"], rtol=1e-6)
    lines = (out / "urdf" / "obj_000003.obj").read_text().splitlines()
    ov = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")])
    assert len(ov) == len(v)
    np.testing.assert_allclose(ext, 1000.0 * (ov.max(axis=0) - ov.min(axis=0)), rtol=1e-5)
    root = ET.parse(out / "urdf" / "obj_000003.urdf").getroot()
    assert float(root.find("link/inertial/mass").get("value")) == pytest.approx(0.2)
    I = root.find("link/inertial/inertia")
    g = lambda k: float(I.get(k))
    T = np.array([[g("ixx"), g("ixy"), g("ixz")], [g("ixy"), g("iyy"), g("iyz")], [g("ixz"), g("iyz"), g("izz")]])
    assert np.all(np.linalg.eigvalsh(T) > 0)
    assert root.find("link/collision/geometry/mesh").get("filename") == "obj_000003.obj"


# ---- marching: the scan, the border, dense fields, the workspace --------------------------------------------------------
def march_counts(dev_sdf, grid):
    """counts[2] of pgr_march_count, read straight from the entry point."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    g = grid.struct()
    ws = torch.empty(int(L.pgr_march_workspace_bytes(grid.nx, grid.ny, grid.nz)), dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    assert L.pgr_march_count(C.byref(g), _lib.ptr(dev_sdf), _lib.ptr(ws), ws.numel(), _lib.ptr(counts),
                             _lib.stream_ptr(dev_sdf.device)) == _lib.PGR_OK
    return tuple(int(x) for x in counts.cpu())


def check_march(sdf, grid):
    """Device against the sparse reference: counts and faces equal, vertices within 1e-6 voxel, two runs identical."""
    import torch
    from pegasus_amd.mesh import march
    sdf = np.ascontiguousarray(sdf, np.float32)
    assert sdf.shape == grid.shape
    v_ref, f_ref = R.march_reference(sdf, grid, sparse=True)
    dev = torch.as_tensor(sdf, device="cuda")
    assert march_counts(dev, grid) == (len(v_ref), len(f_ref))
    a = march(dev, grid)
    b = march(dev, grid)
    assert a.vertices.shape == v_ref.shape and a.faces.shape == f_ref.shape
    assert a.vertices.dtype == np.float32 and a.faces.dtype == np.int32
    np.testing.assert_array_equal(a.faces, f_ref)
    np.testing.assert_allclose(a.vertices, v_ref, rtol=0, atol=1e-6 * grid.voxel)
    assert a.vertices.tobytes() == b.vertices.tobytes() and a.faces.tobytes() == b.faces.tobytes()
    return a


# per = tiles each thread of the one-workgroup scan walks: 1 up to 1024 tiles, 2 up to 2048 (1025 and 1088 tiles leave the
# upper threads without a run), 4 at 3703 (the last run partly filled), 16 at 256^3
SCAN_GRIDS = [(2, 2, 2), (3, 3, 3), (10, 10, 10), (16, 8, 8), (17, 8, 8), (16, 16, 8), (15, 15, 13), (1024, 2, 2),
              (2, 1024, 2), (2, 2, 1024), (128, 93, 88), (127, 129, 64), (107, 99, 99), (129, 97, 89), (161, 157, 150),
              (256, 256, 256)]


@pytest.mark.parametrize("shape", SCAN_GRIDS, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}-tiles{MC.n_tiles(MC.unit_grid(*s))}")
def test_march_scan_across_tile_counts(shape):
    grid = MC.unit_grid(*shape)
    m = check_march(MC.gyroid(grid), grid)
    n = shape[0] * shape[1] * shape[2]
    assert len(m.faces) > (0 if n <= 27 else n // 20)          # the surface fills the grid: every tile has its share


def test_march_scan_ids_name_the_tile_counts_they_are_there_for():
    tiles = [MC.n_tiles(MC.unit_grid(*s)) for s in SCAN_GRIDS]
    assert {1, 2, 3, 4, 1023, 1024, 1025, 1088, 3703, 16384} <= set(tiles)
    assert 16 * 8 * 8 == 1024 and 127 * 129 * 64 % 1024 != 0 and 161 * 157 * 150 % (4 * 1024) != 0


def test_march_sphere_through_the_border():
    sdf, grid = MC.off_centre_sphere()
    m = check_march(sdf, grid)
    n_open, on_planes = MC.boundary_planes_hold_open_edges(m.vertices, m.faces, grid)
    assert n_open > 0 and on_planes
    assert_watertight(check_march(MC.force_outer_layer(sdf), grid).faces)


def test_march_all_inside_is_empty():
    grid = MC.unit_grid(37, 35, 33)
    m = check_march(-np.ones(grid.shape, np.float32), grid)
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)


@pytest.mark.parametrize("face", ["x0", "x1", "y0", "y1", "z0", "z1"])
def test_march_inside_on_one_face_of_the_grid(face):
    grid = MC.unit_grid(21, 19, 17)
    sdf = np.random.default_rng(31).uniform(0.1, 1.0, size=grid.shape).astype(np.float32)
    sel = [slice(None)] * 3
    sel[{"z": 0, "y": 1, "x": 2}[face[0]]] = 0 if face[1] == "0" else -1
    sdf[tuple(sel)] *= -1
    m = check_march(sdf, grid)
    n_open, on_planes = MC.boundary_planes_hold_open_edges(m.vertices, m.faces, grid)
    assert n_open > 0 and on_planes
    # one sheet between the face's layer and the next: two triangles per cell face it crosses, in each of the 6 tetrahedra
    assert len(m.faces) > 2 * 16 * 18


def test_march_inside_values_all_over_the_border():
    sdf, grid = MC.inside_on_border()
    m = check_march(sdf, grid)
    n_open, on_planes = MC.boundary_planes_hold_open_edges(m.vertices, m.faces, grid)
    assert n_open > 0 and on_planes


@pytest.mark.parametrize("field", ["checkerboard", "random-signs"])
def test_march_dense_fields(field):
    sdf, grid = MC.checkerboard() if field == "checkerboard" else MC.random_signs()
    assert MC.n_tiles(grid) == 42
    if field == "random-signs":
        assert R.table_coverage(sdf) == {(t, c) for t in range(6) for c in range(1, 15)}
    else:
        assert R.table_coverage(sdf) == {(t, c) for t in range(6) for c in (5, 10)}
    m = check_march(sdf, grid)
    if field == "checkerboard":                      # every cell holds 12 triangles, every point all its axis edges
        assert len(m.faces) == 12 * 36 * 34 * 32
    assert np.isfinite(m.vertices).all()
    closed = MC.force_outer_layer(sdf)
    if field == "random-signs":
        assert R.table_coverage(closed) == {(t, c) for t in range(6) for c in range(1, 15)}
    assert_watertight(check_march(closed, grid).faces)


def test_march_workspace_contract():
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    grid = MC.unit_grid(15, 15, 13)
    assert MC.n_tiles(grid) == 3
    sdf = MC.gyroid(grid)
    v_ref, f_ref = R.march_reference(sdf, grid, sparse=True)
    dev = torch.as_tensor(sdf, device="cuda")
    g = grid.struct()
    stream = _lib.stream_ptr(dev.device)
    nbytes = int(L.pgr_march_workspace_bytes(grid.nx, grid.ny, grid.nz))
    GUARD = 4096
    ws = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((2 + GUARD // 8,), -7, dtype=torch.int64, device="cuda")
    vertices = torch.full((3 * len(v_ref) + GUARD // 4,), -12345.0, dtype=torch.float32, device="cuda")
    faces = torch.full((3 * len(f_ref) + GUARD // 4,), -777, dtype=torch.int32, device="cuda")
    untouched = [t.clone() for t in (ws, counts, vertices, faces)]

    def same(t, ref):
        return bool(torch.equal(t, ref))
    # one byte short: refused, nothing written
    assert L.pgr_march_count(C.byref(g), _lib.ptr(dev), _lib.ptr(ws), nbytes - 1, _lib.ptr(counts), stream) \
        == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert L.pgr_march_emit(C.byref(g), _lib.ptr(dev), _lib.ptr(ws), nbytes - 1, _lib.ptr(vertices), _lib.ptr(faces), stream) \
        == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    torch.cuda.synchronize()
    assert all(same(t, r) for t, r in zip((ws, counts, vertices, faces), untouched))
    # exactly the size: the guards behind the workspace, the counts, the vertices and the faces stay as they were
    assert L.pgr_march_count(C.byref(g), _lib.ptr(dev), _lib.ptr(ws), nbytes, _lib.ptr(counts), stream) == _lib.PGR_OK
    assert tuple(int(x) for x in counts[:2].cpu()) == (len(v_ref), len(f_ref))
    assert L.pgr_march_emit(C.byref(g), _lib.ptr(dev), _lib.ptr(ws), nbytes, _lib.ptr(vertices), _lib.ptr(faces), stream) \
        == _lib.PGR_OK
    torch.cuda.synchronize()
    assert same(ws[nbytes:], untouched[0][nbytes:]) and same(counts[2:], untouched[1][2:])
    assert same(vertices[3 * len(v_ref):], untouched[2][3 * len(v_ref):])
    assert same(faces[3 * len(f_ref):], untouched[3][3 * len(f_ref):])
    np.testing.assert_array_equal(faces[:3 * len(f_ref)].cpu().numpy().reshape(-1, 3), f_ref)
    np.testing.assert_allclose(vertices[:3 * len(v_ref)].cpu().numpy().reshape(-1, 3), v_ref, rtol=0, atol=1e-6 * grid.voxel)


# ---- TSDF: every case against the transcription, the float64 oracle and the census ------------------------------------
def run_case(case):
    return run_integrate(case.grid, device_specs(case.raw), case.depth, case.final_T, case.truncation, case.alpha_min)


def check_against_transcription(case, got):
    """The rule of test_tsdf_integrate_matches_the_reference: a difference is excused only within 1e-4 px of a pixel
    boundary, and on less than 0.1 % of the points."""
    want, ambiguous = R.tsdf_reference(*case.reference_args(), return_ambiguous=True)
    differs = ~(np.abs(got - want) <= 1e-6)
    excluded = differs & ambiguous
    print(f"differs {int(differs.sum())}, excluded {int(excluded.sum())} of {got.size}")
    assert excluded.mean() < 0.001, excluded.mean()
    keep = ~excluded
    np.testing.assert_allclose(got[keep], want[keep], rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", list(MC.TSDF_CASES))
def test_tsdf_case_matches_both_references_and_reaches_its_branches(name):
    case = MC.TSDF_CASES[name]()
    got = run_case(case)
    assert got.shape == case.grid.shape and got.dtype == np.float32
    inside = R.interior(case.grid)
    assert (got[~inside] == 1.0).all()
    check_against_transcription(case, got)
    MC.check_against_oracle(case, got)


def test_tsdf_carved_points_do_not_depend_on_the_order_of_the_views():
    a, b = MC.TSDF_CASES["carve-after-fusing"](), MC.TSDF_CASES["carve-before-fusing"]()
    sa, sb = run_case(a), run_case(b)
    inside = R.interior(a.grid)
    np.testing.assert_array_equal((sa == 1.0) & inside, (sb == 1.0) & inside)
    assert ((sa == 1.0) & inside).mean() > 0.05


def test_tsdf_nan_depth_is_a_full_truncation_observation():
    """NaN < -truncation is false and fminf(NaN, truncation) is truncation: a NaN depth counts like +inf (the header says so)."""
    nan, inf = MC.TSDF_CASES["depth-nan"](), MC.TSDF_CASES["depth-inf"]()
    assert np.isnan(nan.depth).sum() == np.isinf(inf.depth).sum() > 100
    got = run_case(nan)
    assert np.isfinite(got).all()
    assert got.tobytes() == run_case(inf).tobytes()
    assert got.tobytes() != run_case(MC.TSDF_CASES["synthetic-41x33x29-7views"]()).tobytes()


# ---- end to end at the default size -------------------------------------------------------------------------------------
def test_box_object_at_the_default_resolution(monkeypatch):
    """extract_mesh with its default resolution (256), n_views (96) and image_size (512): the bounds of
    test_box_object_through_the_renderer in this run's voxel, and march of the run's own sdf against the reference."""
    import inspect
    from pegasus_amd import mesh as M
    defaults = {k: p.default for k, p in inspect.signature(M.extract_mesh).parameters.items()}
    assert (defaults["resolution"], defaults["n_views"], defaults["image_size"]) == (256, 96, 512)
    seen = {}
    real_march = M.march

    def recording_march(sdf, grid, stage_ms=None):
        seen["sdf"], seen["grid"] = sdf.cpu().numpy(), grid
        seen["mesh"] = real_march(sdf, grid, stage_ms)
        return seen["mesh"]
    monkeypatch.setattr(M, "march", recording_march)
    dims = np.array([0.06, 0.16, 0.21])
    model, cloud = box_model(dims=tuple(dims))
    m = M.extract_mesh(model)
    grid = seen["grid"]
    assert max(grid.nx, grid.ny, grid.nz) == 256 and MC.n_tiles(grid) > 2048
    assert_watertight(m.faces)
    assert components(len(m.vertices), m.faces) == 1
    lo, hi = m.vertices.min(axis=0), m.vertices.max(axis=0)
    voxel = 1.2 * dims.max() / (256 - 1)
    assert abs(grid.voxel / voxel - 1) < 0.02
    med_scale = float(np.median(np.exp(cloud.scaling)))
    ratio = m.volume() / np.prod(dims)
    info = dict(lo=lo, hi=hi, voxel=voxel, med_scale=med_scale, volume_ratio=ratio)
    print(info)
    assert np.all(np.abs(lo + dims / 2) < 2 * voxel + 3 * med_scale), info
    assert np.all(np.abs(hi - dims / 2) < 2 * voxel + 3 * med_scale), info
    assert abs(ratio - 1) < 0.25, info
    # the marcher on this run's sdf, before largest_component
    v_ref, f_ref = R.march_reference(seen["sdf"], grid, sparse=True)
    assert len(f_ref) > 100_000
    np.testing.assert_array_equal(seen["mesh"].faces, f_ref)
    np.testing.assert_allclose(seen["mesh"].vertices, v_ref, rtol=0, atol=1e-6 * grid.voxel)
    assert_watertight(f_ref)
