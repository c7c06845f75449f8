"""The JPEG encoder on the device (pegasus_amd.jpeg) against the NumPy restatement of its rule
(tests/jpeg_reference.py): equal bytes, files the strict reader takes, no store outside a file's window."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_reference as JR

pytestmark = pytest.mark.gpu


def dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.mark.parametrize("mode", list(JC.MODES))
def test_bytes_equal_the_restatement(gpu_device, mode):
    """Every shape, content and quality of jpeg_cases.equality_images in ONE batch; every file is the restatement's, the strict
    reader takes it, PIL opens it and it keeps below the bound."""
    from PIL import Image
    from pegasus_amd import jpeg
    kind, sub = JC.MODES[mode]
    images, want = JC.equality_images(mode), JC.reference_files(mode)
    keys = list(want)
    got = jpeg.encode_batch_bytes([dev(images[name], gpu_device) for name, _ in keys], quality=[q for _, q in keys],
                                  subsampling=sub)
    wrong = [(key, len(g), len(want[key])) for key, g in zip(keys, got) if g != want[key]]
    assert not wrong, f"{len(wrong)} of {len(keys)} files differ: {wrong[:8]}"
    stuffed = {}
    for (name, q), data in zip(keys, got):
        h, w = images[name].shape[:2]
        info = JR.read_jpeg(data, q)
        assert (info["width"], info["height"], info["kind"], info["sub"]) == (w, h, kind, sub), (name, q)
        assert len(data) <= jpeg.max_bytes(w, h, kind, sub) == JR.max_bytes(w, h, kind, sub), (name, q)
        with Image.open(io.BytesIO(data)) as im:
            assert im.size == (w, h) and im.mode == ("L" if kind == JR.GRAY8 else "RGB")
        stuffed[name, q] = info["stuffed"]
    # random noise at quality 100 exercises the stuffing
    assert stuffed["noise 40x24", 100] >= 1 and stuffed[f"ramp+noise {8 * JC.R + 1} MCUs", 100] >= 1, stuffed
    # and the wide case wraps the RST index
    assert JR.read_jpeg(got[keys.index((f"ramp+noise {8 * JC.R + 1} MCUs", 50))], 50)["n_intervals"] == 9


@pytest.mark.parametrize("group", ["tokens and tables", "past one pass"])
def test_edge_cases_equal_the_restatement(gpu_device, group):
    """jpeg_cases.edge_cases in one batch a group: blocks that code one, two and three ZRLs and end without an EOB, DC
    differences of category 11, a table whose unlimited code is 17 deep (limit 16 on the device, in a file of 264
    intervals); and files of 256, 257, 513 and 260 intervals, where the finish kernel takes more than one pass.  Every file is
    the restatement's (tests/test_jpeg_host.py judges those alone) and the strict reader reports the intervals."""
    from pegasus_amd import jpeg
    cases, want = JC.edge_cases(), JC.edge_reference_files()
    past = set(JC.past_one_pass_shapes())
    names = [n for n in cases if (n in past) == (group == "past one pass")]
    assert len(names) == (4 if group == "past one pass" else 5)
    got = jpeg.encode_batch_bytes([dev(cases[n][1], gpu_device) for n in names], quality=[cases[n][2] for n in names],
                                  subsampling=[JC.MODES[cases[n][0]][1] for n in names])
    wrong = [(n, len(g), len(want[n])) for n, g in zip(names, got) if g != want[n]]
    assert not wrong, wrong
    for n, data in zip(names, got):
        mode, image, q = cases[n]
        info = JR.read_jpeg(data, q)
        assert (info["width"], info["height"]) == image.shape[1::-1]
        assert info["n_intervals"] == -(-np.prod(JR.shape(image.shape[1], image.shape[0], *JC.MODES[mode])[:2]) // JC.R)
        if n in past or n == "fibonacci":
            assert info["n_intervals"] >= 256
            assert n == "fibonacci" or info["n_intervals"] == int(n.split()[0])


def test_one_batch_mixes_kinds_sizes_qualities_and_subsamplings(gpu_device):
    from pegasus_amd import jpeg
    jobs = [("gray", "noise 17x17", 95), ("420", "rendered-like", 50), ("444", "ramp", 100), ("gray", "ramp", 1),
            ("420", f"ramp+noise {JC.R + 1} MCUs", 95), ("444", "noise 1x1", 50), ("420", "flat", 100)]
    images = [dev(JC.equality_images(m)[name], gpu_device) for m, name, _ in jobs]
    got = jpeg.encode_batch_bytes(images, quality=[q for _, _, q in jobs], subsampling=[JC.MODES[m][1] for m, _, _ in jobs])
    for (m, name, q), data in zip(jobs, got):
        assert data == JC.reference_files(m)[name, q], (m, name, q)
    again = jpeg.encode_batch_bytes(images, quality=[q for _, _, q in jobs], subsampling=[JC.MODES[m][1] for m, _, _ in jobs])
    assert again == got                                               # two runs give equal bytes


def test_views_are_read_where_they_lie(gpu_device):
    """A crop, a plane of a stack, a pixel-strided view and an RGB view into RGBA storage give the bytes of their packed copies."""
    import torch
    from pegasus_amd import jpeg
    rng = np.random.default_rng(5)
    big = dev(rng.integers(0, 256, (60, 70, 3), dtype=np.uint8), gpu_device)
    stack = dev(rng.integers(0, 256, (3, 33, 41), dtype=np.uint8), gpu_device)
    rgba = dev(rng.integers(0, 256, (25, 31, 4), dtype=np.uint8), gpu_device)
    views = [big[7:40, 5:52], stack[1], stack[2][:, ::2], big[:, :, 1], rgba[:, :, :3], big[::2, ::3]]
    assert [v.is_contiguous() for v in views] == [False, True, False, False, False, False]
    for sub in ("4:4:4", "4:2:0"):
        assert jpeg.encode_batch_bytes(views, 90, sub) == jpeg.encode_batch_bytes([v.contiguous() for v in views], 90, sub)
    want = JR.encode(big[7:40, 5:52].cpu().numpy(), 90, JR.S420)
    assert jpeg.encode_batch_bytes(views[:1], 90, "4:2:0")[0] == want
    with pytest.raises(ValueError, match="RGBA"):
        jpeg.encode_batch([rgba])
    with pytest.raises(ValueError, match="16-bit"):
        jpeg.encode_batch([torch.zeros(4, 4, dtype=torch.int16, device=gpu_device)])


def test_emit_keeps_inside_the_files_whatever_the_offsets_hold(gpu_device):
    """Device-side offsets that lie: negative, descending, beyond total.  Nothing outside [offsets[k], min(offsets[k+1], total))
    is stored: the guards and every byte no file may own stay as they were.  A short capacity is the host's refusal."""
    import torch
    from pegasus_amd import _lib, jpeg
    image = JC.rendered_like(60, 70, True)
    images = [dev(image, gpu_device) for _ in range(3)]
    n = len(images)
    jobs = (_lib.PgrJpegJob * n)(*[jpeg._job(t, 95, _lib.PGR_JPEG_420) for t in images])
    ws = _lib.workspace("pgr_jpeg", gpu_device, n, jobs)
    sizes = torch.empty(n, dtype=torch.int64, device=gpu_device)
    _lib.call("pgr_jpeg_encode", gpu_device, jobs, n, _lib.ptr(sizes), _lib.ptr(ws), ws.numel())
    size = int(sizes[0])
    total = 3 * size
    # file 0: a negative start; file 1: room for 10 bytes; file 2: cut at total, 10 bytes short
    lies = torch.tensor([-5, 2 * size, 2 * size + 10, 1 << 40], dtype=torch.int64, device=gpu_device)
    guarded = torch.full((total + 128,), 0xA5, dtype=torch.uint8, device=gpu_device)
    _lib.call("pgr_jpeg_emit", gpu_device, jobs, n, _lib.ptr(lies), total, C.c_void_p(guarded.data_ptr() + 64), total, _lib.ptr(ws),
              ws.numel())
    host = guarded.cpu().numpy()
    assert (host[:64 + 2 * size] == 0xA5).all() and (host[-64:] == 0xA5).all()
    good = JR.encode(image, 95, JR.S420)
    assert len(good) == size
    assert bytes(host[64 + 2 * size:64 + 2 * size + 10]) == good[:10]
    assert bytes(host[64 + 2 * size + 10:64 + total]) == good[:size - 10]
    before = guarded.clone()
    status = _lib.enqueue("pgr_jpeg_emit", gpu_device, jobs, n, _lib.ptr(lies), total, C.c_void_p(guarded.data_ptr() + 64), total - 1,
                          _lib.ptr(ws), ws.numel())
    assert status == _lib.PGR_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.equal(before, guarded)


def test_writer_writes_rgb_as_jpeg(tmp_path, gpu_device):
    """BopSceneWriter(rgb_format="jpg") on 2 frames of 64 x 48: rgb/*.jpg within the recorded margin of what PIL makes of the PNG
    path's pixels, depth and masks byte-equal to the PNG run, COCO names ending in .jpg; the records path writes the same."""
    import json
    import torch
    from pegasus_amd import bop_dataset as BD, dataset_writer as DW, masks as M
    B, K, H, W = 2, 2, 48, 64
    color = np.stack([JC.rendered_like(H, W, True, seed=s) for s in range(B)]).transpose(0, 3, 1, 2).astype(np.float32) / 255.0
    depth = np.random.default_rng(2).uniform(0.3, 5.0, (B, 1, H, W)).astype(np.float32)
    sil = np.zeros((B, K, H, W), np.uint8)
    sil[:, 0, 0:20, 10:30] = 1
    sil[:, 1, 12:33, 25:46] = 1
    vis = sil.copy()
    vis[:, 1, 12:20, 25:30] = 0
    gt = {str(i): [{"cam_R_m2c": np.eye(3).reshape(-1).tolist(), "cam_t_m2c": [0.0, 0.0, 1.0 + i], "obj_id": k + 3} for k in range(K)]
          for i in range(B)}
    cam = {str(i): {"cam_K": [100.0, 0, 32.0, 0, 100.0, 24.0, 0, 0, 1.0], "depth_scale": 1.0} for i in range(B)}
    images = dict(color=dev(color, gpu_device), depth=dev(depth, gpu_device), masks=dev(vis, gpu_device))
    records = dict(records=M.pack_records(images["color"], images["depth"], images["masks"]))
    scenes = {}
    for name, frames, kw in (("png", images, {}), ("jpg", images, dict(rgb_format="jpg")),
                             ("jpg_records", records, dict(rgb_format="jpg", encoder="gpu")),
                             ("jpg_420", images, dict(rgb_format="jpg", jpeg_quality=80, jpeg_subsampling="4:2:0"))):
        w = DW.BopSceneWriter(tmp_path / name / "ds", workers=2, **kw)
        w.add_batch(frames, gt, cam, n=B, silhouettes=dev(sil, gpu_device), record_shape=(H, W, K), coco=True)
        scenes[name] = w.close()
    png = scenes["png"]
    for name in ("jpg", "jpg_records", "jpg_420"):
        s = scenes[name]
        assert sorted(p.name for p in (s / "rgb").iterdir()) == ["000000.jpg", "000001.jpg"]
        q, sub = (80, JR.S420) if name == "jpg_420" else (95, JR.S444)
        for i in range(B):
            pixels = BD.decode_png((png / "rgb" / BD.image_name(i)).read_bytes())
            data = (s / "rgb" / f"{i:06d}.jpg").read_bytes()
            assert data == JR.encode(pixels, q, sub)
            JR.read_jpeg(data, q)
            ours, pil = JR.psnr(JC.pil_decode(data), pixels), JR.psnr(JC.pil_decode(JC.pil_file(pixels, q, sub)), pixels)
            assert ours >= pil - JC.PSNR_MARGIN_DB, (name, i, ours, pil)
            assert (BD.BopScene(s).read_image("rgb", i).shape, BD.BopScene(s).image_size(i)) == ((H, W, 3), (W, H))
        for kind in ("depth", "mask", "mask_visib"):
            files = sorted(p.name for p in (png / kind).iterdir())
            assert files and files == sorted(p.name for p in (s / kind).iterdir())
            for f in files:
                a, b = (png / kind / f).read_bytes(), (s / kind / f).read_bytes()
                # (the device PNG encoder frames the same pixels differently)
                assert a == b if name != "jpg_records" else np.array_equal(BD.decode_png(a), BD.decode_png(b)), (name, kind, f)
        doc = json.loads((s / "scene_gt_coco.json").read_text())
        assert [im["file_name"] for im in doc["images"]] == ["rgb/000000.jpg", "rgb/000001.jpg"]
    assert [im["file_name"] for im in json.loads((png / "scene_gt_coco.json").read_text())["images"]] == ["rgb/000000.png", "rgb/000001.png"]
    with pytest.raises(ValueError, match="'png' or 'jpg'"):
        DW.BopSceneWriter(tmp_path / "bad" / "ds", workers=1, rgb_format="webp")


def test_undistort_project_writes_jpeg_on_the_device(tmp_path, gpu_device):
    """Two 40 x 24 JPEG inputs (one RGB, one gray) with jpeg="gpu": JPEGs of the rule at quality 95, 4:2:0, that PIL opens at
    the undistorted size and that show what the host path shows."""
    from PIL import Image
    from pegasus_amd import colmap_io, undistort
    from pegasus_amd.colmap_io import ColmapCamera, ColmapImage
    c = ColmapCamera(1, "OPENCV", 40, 24, np.array([33.0, 34.0, 20.5, 11.5, -0.08, 0.0, 0.003, -0.002]))
    imgs = {}
    for root in (tmp_path / "gpu", tmp_path / "host"):
        (root / "input").mkdir(parents=True)
        for i, colour in enumerate((True, False)):
            name = f"frame_{i}.jpg"
            Image.fromarray(JC.rendered_like(24, 40, colour, seed=i)).save(root / "input" / name, quality=98)
            imgs[i + 1] = ColmapImage(i + 1, np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.1 * i, 0.0, 2.0]), 1, name,
                                      xys=np.zeros((0, 2)), point3D_ids=np.zeros(0, np.int64))
        colmap_io.write_colmap_model(root / "distorted" / "sparse" / "0", {1: c}, imgs, np.zeros((0, 3)), np.zeros((0, 3), np.uint8),
                                     binary=True)
    out = {}
    for where in ("gpu", "host"):
        root = tmp_path / where
        out[where] = undistort.undistort_project(root / "input", root / "distorted" / "sparse" / "0", root, jpeg=where)
    cam = out["gpu"]["cameras"][1]
    for i, mode in enumerate(("RGB", "L")):
        data = (tmp_path / "gpu" / "images" / f"frame_{i}.jpg").read_bytes()
        info = JR.read_jpeg(data, 95)
        assert (info["width"], info["height"]) == (cam.width, cam.height)
        assert info["sub"] == (JR.S420 if mode == "RGB" else JR.S444)
        with Image.open(io.BytesIO(data)) as im:
            assert im.size == (cam.width, cam.height) and im.mode == mode
            ours = np.asarray(im).astype(np.float64)
        host = np.asarray(Image.open(tmp_path / "host" / "images" / f"frame_{i}.jpg")).astype(np.float64)
        # two encoders of the same pixels at quality 95: each within 36 dB of them, so (the errors add at worst) within 30 dB
        assert JR.psnr(ours, host) > 30.0
    with pytest.raises(ValueError, match="jpeg is 'host' or 'gpu'"):
        undistort.undistort_project(tmp_path / "gpu" / "input", tmp_path / "gpu" / "distorted" / "sparse" / "0", tmp_path / "x", jpeg="fpga")
