"""pgr_bop_gt_info and the host code around it on the GPU, against the NumPy reference (tests/gt_info_reference.py), exactly:
every case of tests/gt_info_cases.py through the C entry point between guard regions, gt_from_meshes and recompute_dataset
against the whole NumPy pipeline (tests/mesh_raster_reference.render_f32 on the 3x canvas, then the reference), and VSD at
its edges."""
import json
import shutil

import numpy as np
import pytest

import gt_info_reference as GR
import mesh_raster_cases as MC
import mesh_raster_reference as MR
from test_gt_info_host import CASES, K33, check_vsd_edges, ref

pytestmark = pytest.mark.gpu
GUARD = 4096                                     # bytes on either side of every output


def run_kernel(c):
    """pgr_bop_gt_info by ctypes: mask, mask_visib and stats lie between guard regions pre-filled with a pattern, the outputs
    themselves with bytes that are neither 0 nor 1.  Returns (mask, visib, stats) as host arrays."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    canv, scene = torch.from_numpy(c["canvases"]).cuda(), torch.from_numpy(c["scene"]).cuda()
    (S, Hc, Wc), (F, H, W), J = canv.shape, scene.shape, len(c["K"])
    arr = (_lib.PgrGtInfoJob * J)(*[_lib.PgrGtInfoJob(slot=int(s), frame=int(f), fx=k[0], fy=k[1], cx=k[2], cy=k[3])
                                    for s, f, k in zip(c["slots"], c["frames"], c["K"].tolist())])
    n = J * H * W
    mask = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    visib = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    stats = torch.full((J * GR.STATS + 2 * GUARD // 4,), -7777, dtype=torch.int32, device="cuda")
    rc = L.pgr_bop_gt_info(_lib.ptr(canv), S, Wc, Hc, c["margin"][0], c["margin"][1], _lib.ptr(scene), F, W, H, J, arr, c["delta"],
                           _lib.ptr(mask[GUARD:]), _lib.ptr(visib[GUARD:]), _lib.ptr(stats[GUARD // 4:]), _lib.stream_ptr(canv.device))
    _lib.check(rc, "pgr_bop_gt_info")
    torch.cuda.synchronize()
    assert (mask[:GUARD] == 0xA5).all() and (mask[GUARD + n:] == 0xA5).all(), "mask guard overwritten"
    assert (visib[:GUARD] == 0x5A).all() and (visib[GUARD + n:] == 0x5A).all(), "mask_visib guard overwritten"
    assert (stats[:GUARD // 4] == -7777).all() and (stats[GUARD // 4 + J * GR.STATS:] == -7777).all(), "stats guard overwritten"
    assert canv.cpu().numpy().tobytes() == c["canvases"].tobytes() and scene.cpu().numpy().tobytes() == c["scene"].tobytes(), "inputs changed"
    return (mask[GUARD:GUARD + n].reshape(J, H, W).cpu().numpy(), visib[GUARD:GUARD + n].reshape(J, H, W).cpu().numpy(),
            stats[GUARD // 4:GUARD // 4 + J * GR.STATS].reshape(J, GR.STATS).cpu().numpy())


def assert_equals_reference(got, want, what):
    for name, a, b in zip(("mask", "mask_visib", "stats"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        bad = np.argwhere(a != b)
        assert not len(bad), f"{what}: {name} differs from the reference at {len(bad)} places, first {bad[0].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}"


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_kernel_equals_the_reference(c):
    import torch
    from pegasus_amd import mesh_render as R
    got = run_kernel(c)
    again = run_kernel(c)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), "two runs differ"
    assert set(np.unique(got[0])) <= {0, 1} and set(np.unique(got[1])) <= {0, 1}, "an output byte was left unwritten"
    want = ref(c)
    print(f"{c['name']}: {len(c['K'])} jobs, canvas {c['canvases'].shape[2]}x{c['canvases'].shape[1]}, "
          f"{int(want[0].sum())} mask and {int(want[1].sum())} visible pixels")
    assert_equals_reference(got, want, c["name"])
    # the Python entry has one canvas per job: the slots are gathered first, everything else it can express
    canv = torch.from_numpy(c["canvases"]).cuda()[torch.from_numpy(c["slots"]).long().cuda()]
    m, v, s = R.reduce_gt_info(canv, c["margin"], torch.from_numpy(c["scene"]).cuda(), c["frames"], K33(c["K"]), c["delta"])
    assert_equals_reference((m.cpu().numpy(), v.cpu().numpy(), s.cpu().numpy()), want, c["name"] + " through reduce_gt_info")


# ---- the whole pipeline ----------------------------------------------------------------------------------------------------
class Mesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces = np.asarray(vertices, np.float32), np.asarray(faces, np.int32)


def numpy_pipeline(models, scene_gt, scene_camera, depth, delta, translation_scale, near=1e-3):
    """gt_from_meshes in NumPy: every object rendered by the float32 transcription on the 3x canvas (margin = image size, the
    principal point moved by it), the depth images brought to the poses' unit (float32 image times the float32 of
    depth_scale * unit), the reference on top.  ``models``: {obj_id: (vertices in the poses' unit, faces)}; scene_gt and
    scene_camera are lists per frame.  Returns (masks, visibs, info) per frame."""
    B, H, W = depth.shape
    unit = float(translation_scale) / 1000.0
    scene = np.stack([np.asarray(depth[i], np.float32) * np.float32(float(scene_camera[i].get("depth_scale", 1.0)) * unit) for i in range(B)])
    jobs, frames, Ks = [], [], []
    for i in range(B):
        K = np.asarray(scene_camera[i]["cam_K"], np.float64).reshape(3, 3)
        for e in scene_gt[i]:
            v, f = models[int(e["obj_id"])]
            jobs.append(MC.job(v, f, np.asarray(e["cam_R_m2c"], np.float64).reshape(3, 3), e["cam_t_m2c"], K[0, 0], K[1, 1], K[0, 2] + W,
                               K[1, 2] + H, slot=len(jobs)))
            frames.append(i); Ks.append([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    if jobs:
        canvases, _ = MR.render_f32(jobs, 3 * W, 3 * H, near)
        mask, visib, stats = GR.reduce(canvases, (W, H), scene, np.arange(len(jobs)), frames, np.asarray(Ks), delta * unit)
    else:
        mask = visib = np.zeros((0, H, W), np.uint8); stats = np.zeros((0, GR.STATS), np.int32)
    frames = np.asarray(frames, np.int64)
    return ([mask[frames == i] for i in range(B)], [visib[frames == i] for i in range(B)], [GR.info(stats[frames == i]) for i in range(B)])


def two_meshes():
    """An icosphere and a box, in metres."""
    v, f = MC.icosphere(2, 0.06)
    b, bf = MC.box((0.05, 0.035, 0.07))
    return {1: (v, f), 4: (b, bf)}


def frames_of(W, H, counts, seed):
    """scene_gt, scene_camera (lists per frame, poses in metres, each frame its own K and depth_scale) and depth images [B,H,W]
    as written (uint16 values) for frames with ``counts`` objects each: objects in the open, truncated by the border, wholly
    in the canvas's margin, behind one another; an occluder and holes of missing depth in the scene."""
    rng = np.random.default_rng(seed)
    models = two_meshes()
    scales = [1.0, 0.5, 2.0, 0.1]
    places = [(0.0, 0.0, 0.5), (0.16, 0.03, 0.5), (0.03, -0.02, 0.62), (0.42, 0.0, 0.55), (-0.05, 0.06, 0.45)]
    gt, cam, depth, at = [], [], [], 0
    for i, n in enumerate(counts):
        K = np.array([[60.0 + 3 * i, 0, W / 2 - 0.5 + i], [0, 58.0 - 2 * i, H / 2 + 0.25 * i], [0, 0, 1.0]])
        entries = []
        for _ in range(n):
            t = places[at % len(places)]
            entries.append({"cam_R_m2c": MC.rotation(rng.normal(size=3), rng.uniform(0, 3)).reshape(-1).tolist(), "cam_t_m2c": list(t),
                            "obj_id": [1, 4][at % 2]})
            at += 1
        gt.append(entries)
        cam.append({"cam_K": K.reshape(-1).tolist(), "depth_scale": scales[i % len(scales)]})
        mm = np.full((H, W), 2000.0)
        for e in entries:
            v, f = models[e["obj_id"]]
            d = MR.render_f32([MC.job(v, f, np.asarray(e["cam_R_m2c"]).reshape(3, 3), e["cam_t_m2c"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])], W, H, 1e-3)[0][0]
            mm = np.where(d > 0, np.minimum(mm, d.astype(np.float64) * 1000.0), mm)
        mm[: H // 2, : W // 2 + 4] = 200.0                            # an occluder over the upper left
        mm[rng.random((H, W)) < 0.08] = 0.0                           # missing depth
        depth.append(np.rint(mm / cam[-1]["depth_scale"]).astype(np.uint16))
    return models, gt, cam, np.stack(depth)


def in_millimetres(models, gt):
    models = {k: ((v.astype(np.float64) * 1000.0).astype(np.float32), f) for k, (v, f) in models.items()}
    gt = [[dict(e, cam_t_m2c=[1000.0 * x for x in e["cam_t_m2c"]]) for e in frame] for frame in gt]
    return models, gt


@pytest.mark.parametrize("translation_scale", [1, 1000])
def test_gt_from_meshes_equals_the_numpy_pipeline(translation_scale):
    import torch
    from pegasus_amd import mesh_render as R
    W, H = 40, 30
    models, gt, cam, depth = frames_of(W, H, (2, 0, 3), seed=31)
    if translation_scale == 1000:
        models, gt = in_millimetres(models, gt)
    want = numpy_pipeline(models, gt, cam, depth.astype(np.float32), 15.0, translation_scale)
    n_all = [e["px_count_all"] for f in want[2] for e in f]
    n_vis = [e["px_count_visib"] for f in want[2] for e in f]
    n_mask = [int(m.sum()) for f in want[0] for m in f]
    print(f"translation_scale {translation_scale}: px_count_all {n_all}, mask {n_mask}, visible {n_vis}")
    # the inputs are fit for the check: truncation, an object wholly in the margin, occlusion
    assert len(n_all) == 5 and any(a > m > 0 for a, m in zip(n_all, n_mask)) and any(a > 0 and m == 0 for a, m in zip(n_all, n_mask))
    assert any(0 < v < m for v, m in zip(n_vis, n_mask)) and want[2][1] == []
    ms = R.MeshSet({k: Mesh(v, f) for k, (v, f) in models.items()})
    scene_gt = {str(i): g for i, g in enumerate(gt)}
    scene_camera = {str(i): c for i, c in enumerate(cam)}
    canvas_bytes = 4 * 9 * W * H
    for budget in (canvas_bytes, 2 * canvas_bytes, R.DEFAULT_BUDGET):                 # one, two and all jobs per call
        masks, visibs, info = R.gt_from_meshes(ms, scene_gt, scene_camera, torch.from_numpy(depth.astype(np.float32)), delta=15.0,
                                               translation_scale=translation_scale, budget_bytes=budget)
        assert len(masks) == len(visibs) == len(info) == 3
        for i in range(3):
            for name, got, ref_ in (("mask", masks[i], want[0][i]), ("mask_visib", visibs[i], want[1][i])):
                assert got.dtype == torch.uint8 and tuple(got.shape) == ref_.shape, (budget, i, name)
                np.testing.assert_array_equal(got.cpu().numpy(), ref_, err_msg=f"budget {budget}, frame {i}: {name}")
            assert info[i] == want[2][i], (budget, i)


def test_render_depth_in_chunks_equals_the_single_call():
    from pegasus_amd import mesh_render as R
    W, H = 40, 30
    models, gt, cam, _ = frames_of(W, H, (2, 0, 3), seed=31)
    ms = R.MeshSet({k: Mesh(v, f) for k, (v, f) in models.items()})
    jobs = [(e["obj_id"], np.asarray(e["cam_R_m2c"]).reshape(3, 3), np.asarray(e["cam_t_m2c"])) for frame in gt for e in frame]
    Ks = np.stack([np.asarray(cam[i]["cam_K"]).reshape(3, 3) for i, frame in enumerate(gt) for _ in frame])
    near = 0.5                                                        # through the objects: faces straddle it in every job
    whole, n_whole = R.render_depth(ms, jobs, Ks, (W, H), margin=(W, H), near=near, return_straddle=True)
    parts, n_parts = R.render_depth(ms, jobs, Ks, (W, H), margin=(W, H), near=near, return_straddle=True, budget_bytes=4 * 9 * W * H)
    assert whole.cpu().numpy().tobytes() == parts.cpu().numpy().tobytes()
    want = [MR.render_f32([MC.job(*models[o], R_, t, K[0, 0], K[1, 1], K[0, 2] + W, K[1, 2] + H)], 3 * W, 3 * H, near) for (o, R_, t), K in zip(jobs, Ks)]
    counts = [s for _, s in want]
    print("straddle counts per job", counts)
    assert sum(c > 0 for c in counts) >= 2 and int(n_whole) == int(n_parts) == sum(counts)
    np.testing.assert_array_equal(whole.cpu().numpy(), np.stack([d[0] for d, _ in want]))


def write_dataset(root, translation_scale):
    """A two-scene BOP dataset written by hand: depth PNGs, models, scene_gt.json and scene_camera.json, no masks.  Returns
    what the NumPy pipeline makes of it, from the depth PNGs as decoded: {scene dir: (image ids, masks, visibs, info)}."""
    from pegasus_amd import dataset_writer as DW, mesh
    W, H = 40, 30
    models = two_meshes()
    models_mm = {k: ((v.astype(np.float64) * 1000.0).astype(np.float32), f) for k, (v, f) in models.items()}
    for k, (v, f) in models_mm.items():
        mesh.write_ply(root / "models" / f"obj_{k:06d}.ply", mesh.Mesh(v, f))
    # what MeshSet.from_dir makes of the millimetre files: float64 product with translation_scale / 1000, rounded once
    loaded = {k: ((v.astype(np.float64) * (translation_scale / 1000.0)).astype(np.float32), f) for k, (v, f) in models_mm.items()}
    want = {}
    for s, (ids, counts) in enumerate(((["0", "1", "7"], (1, 3, 0)), (["3", "12"], (2, 2)))):
        _, gt, cam, depth = frames_of(W, H, counts, seed=40 + s)
        if translation_scale == 1000:
            _, gt = in_millimetres(models, gt)
        scene = root / "ds" / "train" / f"{s:06d}"
        (scene / "depth").mkdir(parents=True)
        for i, d in zip(ids, depth):
            (scene / "depth" / f"{int(i):06d}.png").write_bytes(DW.encode_png(d))
        (scene / "scene_gt.json").write_text(json.dumps({i: g for i, g in zip(reversed(ids), reversed(gt))}))     # not in order
        (scene / "scene_camera.json").write_text(json.dumps({i: c for i, c in zip(ids, cam)}))
        decoded = np.stack([DW.decode_png((scene / "depth" / f"{int(i):06d}.png").read_bytes()) for i in ids]).astype(np.float32)
        want[scene] = (ids,) + numpy_pipeline(loaded, gt, cam, decoded, 15.0, translation_scale)
    return want


def check_dataset(want):
    from pegasus_amd import dataset_writer as DW
    for scene, (ids, masks, visibs, info) in want.items():
        text = (scene / "scene_gt_info.json").read_text()
        assert json.loads(text) == {i: e for i, e in zip(ids, info)} and list(json.loads(text)) == ids
        files = {}
        for i, m, v in zip(ids, masks, visibs):
            for o in range(len(m)):
                files[f"mask/{int(i):06d}_{o:06d}.png"] = m[o] * 255
                files[f"mask_visib/{int(i):06d}_{o:06d}.png"] = v[o] * 255
        found = sorted(p.relative_to(scene).as_posix() for d in ("mask", "mask_visib") for p in (scene / d).iterdir())
        assert found == sorted(files)
        for name, image in files.items():
            data = (scene / name).read_bytes()
            np.testing.assert_array_equal(DW.decode_png(data), image, err_msg=f"{scene.name}/{name}")
            assert data == DW.encode_png(image)
        assert sum(int(m.sum()) for m in visibs) > 0


def test_recompute_dataset_equals_the_numpy_pipeline(tmp_path):
    from pegasus_amd import mesh_render as R
    want = write_dataset(tmp_path, 1)
    scenes = R.recompute_dataset(tmp_path / "ds", tmp_path / "models", delta=15.0, translation_scale=1.0, batch=2)
    assert sorted(scenes) == sorted(want)
    check_dataset(want)


def test_command_line_recomputes_a_millimetre_dataset(tmp_path, capsys):
    from pegasus_amd import mesh_render as R
    want = write_dataset(tmp_path, 1000)
    assert R.main(["--dataset", str(tmp_path / "ds"), "--models", str(tmp_path / "models"), "--translation_scale", "1000"]) == 0
    assert "2 scene(s)" in capsys.readouterr().out
    check_dataset(want)
    for scene in want:                                                # a second run, frame by frame, over the files of the first
        shutil.rmtree(scene / "mask_visib")
    assert R.main(["--dataset", str(tmp_path / "ds"), "--models", str(tmp_path / "models"), "--translation_scale", "1000", "--batch", "1",
                   "--delta", "15"]) == 0
    check_dataset(want)


def test_vsd_edges_on_the_device_equal_the_toolkit():
    check_vsd_edges("cuda")
