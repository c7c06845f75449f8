"""pgr_mesh_depth and pgr_bop_gt_info on the GPU: bytes against the float32 transcription, the float64 oracle outside its
mask (masked share at most 1 % per case: a condition on the inputs), the toolkit's recorded results, and the writer hook."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import mesh_raster_cases as MC
import mesh_raster_reference as MR

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
GUARD = 4096
MAX_MASKED = 0.01


def run_kernel(jobs, W, H, near, n_slots=None):
    """pgr_mesh_depth over concatenated meshes with guard regions around the output and the workspace; returns (depth
    [n_slots,H,W], straddle count).  Jobs sharing a vertex array object share its range."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    n_slots = max(j["slot"] for j in jobs) + 1 if n_slots is None else n_slots
    ranges, vs, fs, v0, f0 = {}, [], [], 0, 0
    for j in jobs:
        key = id(j["vertices"])
        if key not in ranges:
            ranges[key] = (v0, len(j["vertices"]), f0, len(j["faces"]))
            vs.append(j["vertices"]); fs.append(j["faces"])
            v0 += len(j["vertices"]); f0 += len(j["faces"])
    vert = torch.from_numpy(np.concatenate(vs).astype(np.float32)).cuda()
    face = torch.from_numpy(np.concatenate(fs).astype(np.int32).reshape(-1, 3)).cuda()
    arr = (_lib.PgrMeshJob * len(jobs))()
    for k, j in enumerate(jobs):
        r = ranges[id(j["vertices"])]
        f32 = lambda x: np.asarray(x, np.float64).astype(np.float32).reshape(-1).tolist()
        arr[k] = _lib.PgrMeshJob(vertex_first=r[0], vertex_count=r[1], face_first=r[2], face_count=r[3], R=(C.c_float * 9)(*f32(j["R"])),
                                 t=(C.c_float * 3)(*f32(j["t"])), fx=f32(j["fx"])[0], fy=f32(j["fy"])[0], cx=f32(j["cx"])[0],
                                 cy=f32(j["cy"])[0], slot=j["slot"])
    nbytes = int(L.pgr_mesh_depth_workspace_bytes(len(jobs), arr))
    assert nbytes > 0
    n = n_slots * H * W
    out = torch.full((n + 2 * GUARD,), 12345.0, dtype=torch.float32, device="cuda")
    ws = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    rc = L.pgr_mesh_depth(_lib.ptr(vert), vert.shape[0], _lib.ptr(face), face.shape[0], len(jobs), arr, W, H, float(near),
                          _lib.ptr(out[GUARD:]), n_slots, _lib.ptr(cnt[1:]), _lib.ptr(ws[GUARD:]), nbytes, _lib.stream_ptr(out.device))
    _lib.check(rc, "pgr_mesh_depth")
    torch.cuda.synchronize()
    assert (out[:GUARD] == 12345.0).all() and (out[GUARD + n:] == 12345.0).all(), "output guard overwritten"
    assert (ws[:GUARD] == 0xA5).all() and (ws[GUARD + nbytes:] == 0xA5).all(), "workspace guard overwritten"
    assert int(cnt[0]) == -7 and int(cnt[2]) == -7
    return out[GUARD:GUARD + n].reshape(n_slots, H, W).cpu().numpy(), int(cnt[1])


def check_case(name, jobs, W, H, near=0.25, n_slots=None, want_straddle=None):
    got, straddle = run_kernel(jobs, W, H, near, n_slots)
    again, straddle2 = run_kernel(jobs, W, H, near, n_slots)
    assert got.tobytes() == again.tobytes() and straddle == straddle2, "two runs differ"
    ref, ref_straddle = MR.render_f32(jobs, W, H, near, n_slots)
    diff = got.view(np.uint32) != ref.view(np.uint32)
    print(f"{name}: {int((ref > 0).sum())} covered samples, {int(diff.sum())} differ from the transcription, straddle "
          f"{straddle} (reference {ref_straddle})")
    assert straddle == ref_straddle
    if want_straddle is not None:
        assert straddle == want_straddle
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the float32 transcription"
    oracle, masked, bound = MR.render_f64(jobs, W, H, near, n_slots)
    share = max(float(m.mean()) for m in masked)
    print(f"{name}: masked share {share:.5f}, rel bound {bound:.3g}")
    assert share <= MAX_MASKED, f"oracle masks {share:.4f} of a canvas: the inputs are not fit for this check"
    MR.compare(got, oracle, masked, bound)
    return got


def plane_points(points_uv, z=2.0, f=2.0):
    return np.array([[u * z / f, v * z / f, z] for u, v in points_uv], np.float32)


def test_gyroid_of_a_256_grid_subpixel_faces():
    import torch
    from pegasus_amd import mesh
    n = 256
    ax = torch.linspace(-1, 1, n, device="cuda")
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    grid = mesh.Grid(n, n, n, (-1.0, -1.0, -1.0), 2.0 / (n - 1))
    m = None
    for periods in (2.0, 3.0, 1.5, 4.0):
        k = periods * np.pi
        sdf = torch.sin(k * x) * torch.cos(k * y) + torch.sin(k * y) * torch.cos(k * z) + torch.sin(k * z) * torch.cos(k * x)
        m = mesh.march(sdf.contiguous(), grid)
        if 2 ** 20 <= len(m.faces) <= 2 ** 22:
            break
    assert 2 ** 20 <= len(m.faces) <= 2 ** 22, len(m.faces)
    W = H = 128                                                  # 256 grid cells over ~100 pixels: every face is sub-pixel
    fx = fy = 256.0
    v = MC.lattice_nudge(m.vertices, 5.0, fx, fy, W / 2, H / 2)
    check_case(f"gyroid {len(m.faces)} faces", [MC.job(v, m.faces, t=(0, 0, 5.0), fx=fx, fy=fy, cx=W / 2, cy=H / 2)], W, H)


def test_single_triangle_over_a_2400_canvas():
    pts = plane_points([(-100.0, -50.0), (5000.0, -50.0), (-100.0, 5200.0)])
    got = check_case("one triangle, 2400^2", [MC.job(pts, [[0, 1, 2]], fx=2.0, fy=2.0)], 2400, 2400)
    assert (got > 0).mean() > 0.85


def test_mix_across_the_large_threshold():
    # boxes of 15x17 = 255, 16x16 = 256 (small path) and 257x1, 16x17 = 272, 300x200 (queued) samples, plus a cloud of
    # random faces from sub-pixel to 60 pixels on dyadic image points
    rng = np.random.default_rng(5)
    pts, faces = [], []

    def tri(a, b, c):
        faces.append([len(pts), len(pts) + 1, len(pts) + 2]); pts.extend([a, b, c])
    for x0, y0, w, h in ((10, 10, 15, 17), (40, 10, 16, 16), (70, 10, 16, 17), (10, 40, 257, 1), (10, 60, 300, 200)):
        tri((x0 + 0.25, y0 + 0.25), (x0 + w - 0.25, y0 + 0.25), (x0 + 0.25, y0 + h - 0.25))
    for _ in range(3000):
        c = rng.integers(0, 400 * 8, 2) / 8.0
        s = float(rng.choice([0.5, 2, 8, 30, 60]))
        tri(*[(c + rng.integers(-8, 9, 2) / 8.0 * s).tolist() for _ in range(3)])
    z = rng.choice([1.0, 2.0, 4.0], len(pts))
    P = np.array([[u * zz / 2.0, v * zz / 2.0, zz] for (u, v), zz in zip(pts, z)], np.float32)
    check_case("mixed sizes", [MC.job(P, faces, fx=2.0, fy=2.0)], 400, 300)


def test_degenerate_offscreen_behind_and_straddling_faces():
    P = plane_points([(2.5, 2.5), (9.5, 2.5), (16.5, 2.5), (2.5, 9.5),              # 0-3: collinear 0,1,2; zero-area 0,0,3
                      (-50.0, -50.0), (-40.0, -50.0), (-50.0, -40.0),                # 4-6: wholly off canvas
                      (3.0, 12.0), (12.0, 12.0), (3.0, 20.0)])                       # 7-9: a visible face
    behind = np.array([[0.1, 0.1, -1.0], [0.5, 0.1, -2.0], [0.1, 0.5, 0.1]], np.float32)        # all three nearer than near
    strad = np.array([[1.0, 1.0, 2.0], [3.0, 1.0, 2.0], [1.0, 3.0, 0.125], [1.0, 3.0, -3.0]], np.float32)
    V = np.vstack([P, behind, strad])
    faces = [[0, 1, 2], [0, 0, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15], [13, 14, 16], [13, 15, 16], [7, 8, 99], [-1, 8, 9]]
    got = check_case("degenerate", [MC.job(V, faces, fx=2.0, fy=2.0)], 32, 24, near=0.25, want_straddle=3)
    assert (got > 0).sum() > 10


def test_equal_depth_faces_and_saturating_vertices():
    quad = plane_points([(2.5, 2.5), (20.5, 2.5), (20.5, 14.5), (2.5, 14.5)])
    jobs = [MC.job(quad, [[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3]], fx=2.0, fy=2.0)]          # two coplanar pairs: equal depth
    got = check_case("equal depth", jobs, 24, 16)
    assert set(np.unique(got)) == {0.0, 2.0}
    # image coordinates beyond +-2^30 / 256 pixels saturate the snap; the face still covers the canvas it spans
    far = np.array([[-1e9, -1e9, 1.0], [1e9, -1e9, 1.0], [0.0, 3e9, 1.0], [5.0, 5.0, 1.0], [3e38, 5.0, 1.0], [5.0, 3e38, 1.0]], np.float32)
    got = check_case("saturating", [MC.job(far, [[0, 1, 2], [3, 4, 5]], fx=8.0, fy=8.0, cx=8.0, cy=8.0)], 16, 16)
    assert (got > 0).all()


@pytest.mark.parametrize("W,H", [(1, 1), (37, 1), (1, 29)])
def test_thin_canvases(W, H):
    P = plane_points([(-3.0, -3.0), (80.0, -3.0), (-3.0, 70.0), (0.25, 0.25), (0.75, 0.25), (0.25, 0.75)])
    got = check_case(f"{W}x{H}", [MC.job(P, [[0, 1, 2], [3, 4, 5]], fx=2.0, fy=2.0)], W, H)
    assert (got > 0).any()


@pytest.mark.parametrize("n_jobs", [1, 64])
def test_jobs_over_three_meshes_with_out_of_order_slots(n_jobs):
    fx = fy = 64.0
    shapes = [MC.icosphere(2, 1.0), MC.box((0.8, 0.5, 0.6)), MC.icosphere(1, 0.7)]
    shapes = [(MC.lattice_nudge(v, 4.0, fx, fy, 0.0, 0.0), f) for v, f in shapes]
    rng = np.random.default_rng(9)
    slots = rng.permutation(n_jobs)
    jobs = [MC.job(*shapes[k % 3], t=(0, 0, 4.0), fx=fx, fy=fy, cx=float(10 + (7 * k) % 40), cy=float(12 + (5 * k) % 30), slot=int(slots[k]))
            for k in range(n_jobs)]
    got = check_case(f"{n_jobs} jobs", jobs, 60, 52)
    assert all((g > 0).any() for g in got)


def test_gt_info_kernel_equals_the_toolkit():
    import torch
    from pegasus_amd import mesh_render as R
    g = np.load(GOLDEN / "mesh_gt_info.npz")
    W, H = (int(x) for x in g["size"])
    n = len(g["canvases"])
    canv, scene = torch.from_numpy(g["canvases"]).cuda(), torch.from_numpy(g["scene_depth"]).cuda()
    Ks = np.stack([g["K"]] * n)
    mask, visib, stats = R.reduce_gt_info(canv, (W, H), scene, np.arange(n), Ks, float(g["delta"]))
    np.testing.assert_array_equal(mask.cpu().numpy(), np.unpackbits(g["mask"], axis=-1)[..., :W])
    np.testing.assert_array_equal(visib.cpu().numpy(), np.unpackbits(g["mask_visib"], axis=-1)[..., :W])
    info = R.info_from_stats(stats)
    for k in ("px_count_all", "px_count_valid", "px_count_visib", "bbox_obj", "bbox_visib"):
        np.testing.assert_array_equal(info[k], g[k], err_msg=k)
    np.testing.assert_allclose(info["visib_fract"], g["visib_fract"], rtol=0, atol=1e-12)
    t_mask, t_visib, t_stats = R.reduce_gt_info_torch(canv, (W, H), scene, np.arange(n), Ks, float(g["delta"]))
    assert torch.equal(t_stats, stats) and torch.equal(t_mask, mask) and torch.equal(t_visib, visib)
    # the renderer reproduces the recorded canvases from the recorded poses: render_depth with the toolkit's margins
    ms = R.MeshSet({1: type("M", (), dict(vertices=g["vertices"], faces=g["faces"]))()})
    jobs = [(1, MC.rotation((1, 2, 3), 0.7), t) for t in g["t"]]
    depth, straddle = R.render_depth(ms, jobs, g["K"], (W, H), margin=(W, H), near=1.0, return_straddle=True, budget_bytes=3 * 4 * 9 * W * H)
    np.testing.assert_array_equal(depth.cpu().numpy(), g["canvases"])
    assert int(straddle) == 0


def test_vsd_on_the_device_equals_the_toolkit():
    from pegasus_amd import mesh_render as R
    g = np.load(GOLDEN / "mesh_vsd.npz")
    ms = R.MeshSet({1: type("M", (), dict(vertices=g["vertices"], faces=g["faces"]))()}, diameters={1: float(g["diameter"])})
    taus = [float(t) for t in g["taus"]]
    for k in (0, 1, 2, 5, 9):
        got = R.vsd(g["R_est"][k], g["t_est"][k], g["R_gt"][k], g["t_gt"][k], g["depth_test"][k], g["K"], float(g["delta"]), taus, True,
                    float(g["diameter"]), ms, 1, "tlinear", near=1.0)
        np.testing.assert_allclose(got, g["errors_tlinear_1"][k], rtol=0, atol=1e-9)
    batch = R.vsd(g["R_est"][3:7], g["t_est"][3:7], g["R_gt"][3], g["t_gt"][3], g["depth_test"][3], g["K"], float(g["delta"]), taus, False,
                  float(g["diameter"]), ms, 1, "step", near=1.0)
    np.testing.assert_allclose(batch[0].cpu().numpy(), g["errors_step_0"][3], rtol=0, atol=1e-9)
    assert tuple(batch.shape) == (4, len(taus))


def _box_scene():
    """The synthetic Gaussian box of the mesh tests, as a GaussianModel-like object, and its extracted mesh."""
    import math
    from pegasus_amd import mesh, scenes
    from pegasus_amd.gaussian_model import GaussianModel
    cloud = scenes.box_object(np.random.default_rng(11), 40_000, (0.06, 0.16, 0.21), math.log(0.002), 0.4, 0.15, object_id=1)
    model = GaussianModel.from_arrays(cloud.xyz, cloud.features_dc, cloud.features_rest, cloud.opacity, cloud.scaling, cloud.rotation)
    return model, mesh.extract_mesh(model, resolution=64, n_views=32, image_size=192)


def test_writer_takes_ground_truth_from_meshes(tmp_path):
    import torch
    from pegasus_amd import bop_pose, dataset_writer as DW, mesh_render as R
    model, m = _box_scene()
    ms = R.MeshSet({1: m})
    W = H = 96
    K = np.array([[120.0, 0, 48.0], [0, 120.0, 48.0], [0, 0, 1.0]])
    poses = [(0.0, 0.0, 0.6), (0.22, 0.0, 0.6), (0.0, -0.05, 0.5)]                 # centred, truncated by the right border, nearer
    B = len(poses)
    gt = {str(i): [{"cam_R_m2c": MC.rotation((0, 1, 0), 0.3 * i).reshape(-1).tolist(), "cam_t_m2c": list(p), "obj_id": 1}]
          for i, p in enumerate(poses)}
    cam = {str(i): {"cam_K": K.reshape(-1).tolist(), "depth_scale": 1.0} for i in range(B)}
    jobs = [(1, np.asarray(gt[str(i)][0]["cam_R_m2c"]).reshape(3, 3), np.asarray(poses[i])) for i in range(B)]
    own = R.render_depth(ms, jobs, K, (W, H))
    depth_m = torch.where(own > 0, own, torch.full_like(own, 6.0))
    depth_m[0, :, : W // 2] = 0.2                                                # an occluder over the left half of frame 0
    frames = {"color": torch.zeros((B, 3, H, W), device="cuda"), "depth": depth_m[:, None].contiguous()}
    w = DW.BopSceneWriter(tmp_path / "mesh", workers=1)
    w.add_batch(frames, gt, cam, meshes=ms, delta=15.0, translation_scale=1.0)
    scene = w.close()
    info = json.loads((scene / "scene_gt_info.json").read_text())
    for i in range(B):
        e = info[str(i)][0]
        mask = DW.decode_png((scene / "mask" / f"{i:06d}_000000.png").read_bytes())
        visib = DW.decode_png((scene / "mask_visib" / f"{i:06d}_000000.png").read_bytes())
        assert mask.shape == (H, W) and set(np.unique(mask)) <= {0, 255} and set(np.unique(visib)) <= {0, 255}
        assert e["px_count_visib"] == int((visib > 0).sum()) <= e["px_count_all"] and e["px_count_visib"] > 0
        assert not (visib & ~mask).any()
        bo, bv = e["bbox_obj"], e["bbox_visib"]
        assert bo[0] <= bv[0] and bo[1] <= bv[1] and bv[0] + bv[2] <= bo[0] + bo[2] and bv[1] + bv[3] <= bo[1] + bo[3]
    assert info["1"][0]["px_count_all"] > int((DW.decode_png((scene / "mask" / "000001_000000.png").read_bytes()) > 0).sum())
    assert info["0"][0]["px_count_visib"] < info["0"][0]["px_count_all"]         # the occluder hides a part


def test_writer_without_meshes_writes_the_independently_packed_files(tmp_path):
    """The default path of add_batch (no meshes=, and meshes=None) against bytes that no code of the writer or of
    mesh_render produced: every file is encode_png of an array quantised here in NumPy by the writer's documented casts
    (uint8(v * 255) and uint16(d * 1000), float32 product, truncation), or the JSON of records counted here."""
    import torch
    from pegasus_amd import dataset_writer as DW
    B, K, H, W = 3, 2, 40, 56
    rng = np.random.default_rng(21)
    color = rng.random((B, 3, H, W), dtype=np.float32)
    depth = rng.uniform(0.3, 5.0, (B, 1, H, W)).astype(np.float32)
    depth[1, 0, :5] = 0.0                                                        # missing depth: px_count_valid < px_count_all
    sil = np.zeros((B, K, H, W), np.uint8)
    sil[:, 0, 0:20, 10:30] = 1
    sil[:, 1, 12:33, 25:50] = 1
    vis = sil.copy()
    vis[:, 1, 12:20, 25:30] = 0                                                  # object 1 hides a corner of object 2
    vis[2, 0] = 0                                                                # frame 2: object 1 is not visible at all
    gt = {str(i): [{"cam_R_m2c": np.eye(3).reshape(-1).tolist(), "cam_t_m2c": [0.0, 0.0, 1.0 + i], "obj_id": k + 1} for k in range(K)]
          for i in range(B)}
    cam = {str(i): {"cam_K": [100.0, 0, 28.0, 0, 100.0, 20.0, 0, 0, 1.0], "depth_scale": 1.0} for i in range(B)}
    rgb8 = ((color * np.float32(255)).astype(np.int64) & 0xFF).astype(np.uint8).transpose(0, 2, 3, 1)
    mm = ((depth[:, 0] * np.float32(1000)).astype(np.int64) & 0xFFFF).astype(np.uint16)

    def box(m):
        ys, xs = np.nonzero(m)
        return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]
    info = {}
    for i in range(B):
        info[str(i)] = []
        for k in range(K):
            n_all, n_vis = int(sil[i, k].sum()), int(vis[i, k].sum())
            info[str(i)].append({"px_count_all": n_all, "px_count_valid": int((sil[i, k].astype(bool) & (mm[i] != 0)).sum()),
                                 "px_count_visib": n_vis, "visib_fract": n_vis / n_all,
                                 "bbox_obj": box(sil[i, k]) if n_vis else [-1] * 4, "bbox_visib": box(vis[i, k]) if n_vis else [-1] * 4})
    want = {"scene_gt.json": json.dumps(gt).encode(), "scene_camera.json": json.dumps(cam).encode(),
            "scene_gt_info.json": json.dumps(info).encode()}
    for i in range(B):
        want[f"rgb/{i:06d}.png"] = DW.encode_png(rgb8[i])
        want[f"depth/{i:06d}.png"] = DW.encode_png(mm[i])
        for k in range(K):
            want[f"mask_visib/{i:06d}_{k:06d}.png"] = DW.encode_png(vis[i, k] * 255)
            want[f"mask/{i:06d}_{k:06d}.png"] = DW.encode_png(sil[i, k] * 255)
    assert len(want) == 2 * B + 2 * B * K + 3
    dev = lambda a: torch.from_numpy(a).cuda()
    for name, kw in (("default", {}), ("none", dict(meshes=None))):
        w = DW.BopSceneWriter(tmp_path / name, workers=1)
        w.add_batch(dict(color=dev(color), depth=dev(depth), masks=dev(vis)), gt, cam, silhouettes=dev(sil), **kw)
        scene = w.close()
        files = sorted(p.relative_to(scene).as_posix() for p in scene.rglob("*") if p.is_file())
        assert files == sorted(want), name
        for f in files:
            assert (scene / f).read_bytes() == want[f], (name, f)


def test_rotated_off_centre_triangle_on_the_device():
    job, W, H, want = MC.rotated_triangle_case()
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):
        got = check_case("rotated triangle", [dict(job, faces=np.asarray(faces, np.int32))], W, H)
        assert got[0].tobytes() == want.tobytes()


def test_march_sphere_silhouette_has_no_holes():
    import torch
    from scipy import ndimage
    from pegasus_amd import mesh, mesh_render as R
    n = 64
    ax = torch.linspace(-1, 1, n, device="cuda")
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    sdf = torch.sqrt((x - 0.1) ** 2 + y * y + (z + 0.05) ** 2) - 0.7
    m = mesh.march(sdf.contiguous(), mesh.Grid(n, n, n, (-1.0, -1.0, -1.0), 2.0 / (n - 1)))
    ms = R.MeshSet({7: m})
    K = np.array([[300.0, 0, 100.0], [0, 300.0, 90.0], [0, 0, 1.0]])
    depth = R.render_depth(ms, [(7, MC.rotation((1, 2, 0), 0.8), (0.0, 0.0, 4.0))], K, (200, 180))[0].cpu().numpy()
    sil = depth > 0
    assert sil.sum() > 5000 and 3.15 < depth[sil].min() < 3.45
    np.testing.assert_array_equal(ndimage.binary_fill_holes(sil), sil)
