"""Mesh extraction on the device: pgr_tsdf_integrate and pgr_march_count / pgr_march_emit against the NumPy reference
(tests/mesh_reference.py), closed meshes from analytic images and from rendered Gaussian models, and the CLI."""
import json
import math
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import mesh_reference as R
from mesh_reference import assert_watertight, components

pytestmark = pytest.mark.gpu


def views_around(center, dist, n, width, height, fovx, fovy):
    """n look-at views on the full Fibonacci sphere of radius ``dist`` around ``center``: (ViewSpecs, numpy View)."""
    import torch
    from pegasus_amd import graphics as G
    from pegasus_amd.rasterizer import ViewSpec
    from pegasus_amd.scenes import make_view
    specs, raw = [], []
    for Rm, t in G.hemisphere_views(n, dist, elev_range=(-0.5 * math.pi, 0.5 * math.pi))[:n]:
        eye = -Rm.T @ t + np.asarray(center, np.float64)
        v = make_view(Rm, -Rm @ eye, width, height, fovx=fovx, fovy=fovy)
        dev = lambda a: torch.as_tensor(np.asarray(a, np.float32), device="cuda")
        specs.append(ViewSpec(height, width, v.tanfovx, v.tanfovy, dev(np.zeros(3)), dev(v.world_view_transform),
                              dev(v.full_proj_transform), dev(v.camera_center), depth_mode=1))
        raw.append(v)
    return specs, raw


def synthetic_case():
    from pegasus_amd.mesh import Grid
    rng = np.random.default_rng(7)
    grid = Grid(41, 33, 29, (-0.41, -0.3, -0.27), 0.02)
    center = np.array([grid.origin[a] + 0.5 * grid.voxel * (n - 1) for a, n in enumerate((41, 33, 29))])
    W, H = 37, 29
    specs, raw = views_around(center, 1.6, 7, W, H, math.radians(50.0), math.radians(40.0))
    V = len(specs)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.empty((V, H, W), np.float32)
    final_T = np.empty((V, H, W), np.float32)
    for v in range(V):
        depth[v] = 1.6 - 0.25 + 0.1 * np.sin(0.3 * xx + v) * np.cos(0.2 * yy) + 0.02 * rng.standard_normal((H, W))
        final_T[v] = np.where(rng.uniform(size=(H, W)) < 0.08, 0.9, 0.3 * rng.uniform(size=(H, W)))
    return grid, specs, raw, depth, final_T


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
