"""pgr_mask_rle_count / _emit / _decode and pgr_mask_overlap on the GPU, through the C ABI with guard regions around every
buffer the kernels write, for equality with the NumPy restatement (tests/coco_reference.py) and the BOP toolkit's recorded
outputs; the Python wrappers; and the writer hook.  Everything is an integer: no tolerance anywhere."""
import functools
import json
import types
from pathlib import Path

import numpy as np
import pytest

import coco_cases as CC
import coco_reference as CR

golden_cases, undated = CC.golden_cases, CC.undated

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
GUARD = 4096                                   # elements in front of and behind every buffer; a multiple of 16 bytes
CASES = {name: stack for name, stack, _ in CC.cases()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(per-mask counts, stats) of a case, computed once."""
    stack = CASES[name]
    return [CR.rle_counts(m) for m in stack], CR.mask_stats(stack)


def guarded(n, dtype, fill):
    import torch
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")


def intact(buf, n, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


def device_masks(stack, shift=0):
    """The stack's bytes in a buffer of 0xEE (set pixels, were they read), ``shift`` bytes off the aligned start."""
    import torch
    buf = guarded(stack.size, torch.uint8, 0xEE)
    view = buf[GUARD + shift:GUARD + shift + stack.size]
    view.copy_(torch.from_numpy(stack.reshape(-1)).cuda())
    return buf, view


def run_encode(stack, shift=0, slack=0):
    """Both passes over the C ABI.  Returns (per-mask counts, stats [n,6], the raw counts buffer's bytes).  ``slack``: extra
    room per slot (offsets = exclusive sum of n_counts + slack): what the kernel does not write stays at the fill value."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    n, H, W = stack.shape
    keep, masks = device_masks(stack, shift)
    nbytes = int(L.pgr_mask_rle_workspace_bytes(n, W, H))
    assert nbytes > 0
    ws = guarded(nbytes, torch.uint8, 0xA5)
    stats = guarded(6 * n, torch.int32, -7)
    stream = _lib.stream_ptr(masks.device)
    _lib.check(L.pgr_mask_rle_count(_lib.ptr(masks), n, W, H, _lib.ptr(stats[GUARD:]), _lib.ptr(ws[GUARD:]), nbytes, stream),
               "pgr_mask_rle_count")
    torch.cuda.synchronize()
    assert intact(stats, 6 * n, -7), "stats guard overwritten"
    assert intact(ws, nbytes, 0xA5), "workspace guard overwritten by the count pass"
    st = stats[GUARD:GUARD + 6 * n].reshape(n, 6).cpu().numpy()
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(st[:, 0].astype(np.int64) + slack, out=offsets[1:])
    total = int(offsets[-1])
    counts = guarded(total, torch.int32, -9)
    off_dev = torch.from_numpy(offsets).cuda()
    _lib.check(L.pgr_mask_rle_emit(_lib.ptr(masks), n, W, H, _lib.ptr(off_dev), total, _lib.ptr(counts[GUARD:]), total,
                                   _lib.ptr(ws[GUARD:]), nbytes, stream), "pgr_mask_rle_emit")
    torch.cuda.synchronize()
    assert intact(counts, total, -9), "counts guard overwritten"
    assert intact(ws, nbytes, 0xA5), "workspace guard overwritten by the emit pass"
    assert bool((keep[:GUARD + shift] == 0xEE).all()) and bool((keep[GUARD + shift + stack.size:] == 0xEE).all())
    raw = counts[GUARD:GUARD + total].cpu().numpy()
    per = [raw[offsets[k]:offsets[k] + st[k, 0]] for k in range(n)]
    for k in range(n):                                                      # the slack behind a slot's counts is untouched
        assert (raw[offsets[k] + st[k, 0]:offsets[k + 1]] == -9).all()
    return per, st, raw.tobytes()


def check_encode(name, shift=0):
    stack = CASES[name]
    per, st, raw = run_encode(stack, shift)
    per2, st2, raw2 = run_encode(stack, shift)
    assert raw == raw2 and st.tobytes() == st2.tobytes(), "two runs differ"
    want, want_stats = reference(name)
    np.testing.assert_array_equal(st, want_stats, err_msg=name)
    for k in range(len(stack)):
        np.testing.assert_array_equal(per[k], want[k], err_msg=f"{name} mask {k}")
    return per, st


@pytest.mark.parametrize("name", list(CASES))
def test_encode_equals_the_reference(name):
    per, st = check_encode(name)
    H, W = CASES[name].shape[1:]
    assert all(int(c.sum()) == H * W for c in per)


def test_encode_equals_the_toolkit():
    golden = np.load(GOLDEN / "coco_rle.npz")
    for name, stack, counts, boxes, _ in golden_cases(golden):
        per, st, _ = run_encode(stack)
        from pegasus_amd import coco as CO
        for k in range(len(stack)):
            np.testing.assert_array_equal(per[k], counts[k], err_msg=name)
            if stack[k].any():
                assert CO.bbox_from_stats(st[k]).tolist() == boxes[k].tolist(), name


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_masks_that_start_on_any_byte(shift):
    """The stack itself 1, 2, 3 bytes off a dword: every row's dwords are assembled from two aligned ones, and the bytes
    around the stack (0xEE, which would read as set pixels) stay out of the result."""
    for name in ("odd 5x7", "odd 17x33", f"tile cols W={CC.TILE_COLS + 1}", "1x1 set", "row strip W=300"):
        check_encode(name, shift)


def test_checkerboard_has_the_most_runs_a_mask_can_have():
    per, st = check_encode("checkerboard 17x33")
    assert [len(c) for c in per] == [561, 562, 561] and st[:, 0].tolist() == [561, 562, 561]
    assert per[0].tolist() == [1] * 561 and per[1].tolist() == [0] + [1] * 561


def test_special_masks_have_the_documented_counts():
    per, st = check_encode("all zero 17x33")
    assert [c.tolist() for c in per] == [[561]] * 3 and (st[:, 2:4] == 2 ** 31 - 1).all() and (st[:, 4:6] == -2 ** 31).all()
    per, _ = check_encode("all set 17x33")
    assert [c.tolist() for c in per] == [[0, 561]] * 3
    per, _ = check_encode("pixel 0 / last pixel / column seam")
    assert [c.tolist() for c in per] == [[0, 1, 560], [560, 1], [32, 2, 527]]
    per, _ = check_encode("full columns")
    assert per[0].tolist() == [3 * 33, 4 * 33, 10 * 33]
    per, _ = check_encode("runs at a column end")
    assert per[0].tolist() == [4 * 33 + 20, 13 + 6, 561 - 5 * 33 - 6]
    per, _ = check_encode("300x300 all zero")
    assert per[0].tolist() == [90_000]
    per, st = check_encode("empty, dense, empty, sparse")
    assert [c.tolist() for c in per] == [[960], [0, 960], [960], [7 * 24 + 5, 1, 33 * 24 + 20 - (7 * 24 + 6), 2, 960 - (33 * 24 + 22)]]
    assert st[:, 0].tolist() == [1, 2, 1, 5] and st[3, 1:].tolist() == [3, 7, 5, 33, 21]


def test_emit_stays_inside_each_masks_slot():
    """Slots larger than needed keep their tail; a slot SMALLER than a mask's counts (offsets that do not belong to the
    masks) cuts that mask's counts and leaves the neighbours' slots alone."""
    import torch
    from pegasus_amd import _lib
    stack = CASES["empty, sparse, blobs"]
    per, st, _ = run_encode(stack, slack=3)
    want, _ = reference("empty, sparse, blobs")
    for k in range(3):
        np.testing.assert_array_equal(per[k], want[k])
    L = _lib.lib()
    n, H, W = stack.shape
    _, masks = device_masks(stack)
    nbytes = int(L.pgr_mask_rle_workspace_bytes(n, W, H))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stats = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    stream = _lib.stream_ptr(masks.device)
    _lib.check(L.pgr_mask_rle_count(_lib.ptr(masks), n, W, H, _lib.ptr(stats), _lib.ptr(ws), nbytes, stream), "count")
    offsets = np.array([0, 1, 3, 3 + len(want[2])], np.int64)              # mask 1 has 5 counts and a slot of 2
    total = int(offsets[-1])
    counts = guarded(total, torch.int32, -9)
    _lib.check(L.pgr_mask_rle_emit(_lib.ptr(masks), n, W, H, _lib.ptr(torch.from_numpy(offsets).cuda()), total,
                                   _lib.ptr(counts[GUARD:]), total, _lib.ptr(ws), nbytes, stream), "emit")
    torch.cuda.synchronize()
    assert intact(counts, total, -9)
    raw = counts[GUARD:GUARD + total].cpu().numpy()
    np.testing.assert_array_equal(raw[0:1], want[0])
    np.testing.assert_array_equal(raw[1:3], want[1][:2])
    np.testing.assert_array_equal(raw[3:], want[2])


# ---- decode ------------------------------------------------------------------------------------------------------------
def run_decode(per_counts, H, W):
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    n = len(per_counts)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum([len(c) for c in per_counts], out=offsets[1:])
    flat = np.concatenate(per_counts).astype(np.int32)
    counts = torch.from_numpy(flat).cuda()
    out = guarded(n * H * W, torch.uint8, 0x5A)
    _lib.check(L.pgr_mask_rle_decode(_lib.ptr(counts), _lib.ptr(torch.from_numpy(offsets).cuda()), n, W, H, _lib.ptr(out[GUARD:]),
                                     _lib.stream_ptr(out.device)), "pgr_mask_rle_decode")
    torch.cuda.synchronize()
    assert intact(out, n * H * W, 0x5A), "mask guard overwritten"
    return out[GUARD:GUARD + n * H * W].reshape(n, H, W).cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_decode_inverts_encode(name):
    stack = CASES[name]
    want, _ = reference(name)
    got = run_decode(want, *stack.shape[1:])
    np.testing.assert_array_equal(got, (stack != 0).astype(np.uint8))


def test_decode_equals_the_toolkit_with_zero_length_runs():
    golden = np.load(GOLDEN / "coco_rle.npz")
    H, W = (int(v) for v in golden["zero_size"])
    lists = np.split(golden["zero_counts"], np.cumsum(golden["zero_lengths"])[:-1])
    np.testing.assert_array_equal(run_decode(lists, H, W), golden["zero_decoded"])
    for name, stack, counts, _, decoded in golden_cases(golden):
        if stack.shape[1] * stack.shape[2] <= 20_000:
            np.testing.assert_array_equal(run_decode(counts, *stack.shape[1:]), decoded, err_msg=name)
    # zero-length runs between real ones, across a chunk of runs and in a mask of more than one slice
    H, W = 200, 150
    base = CR.rle_counts(CC.blobs(np.random.default_rng(3), H, W))
    padded = np.concatenate([[c, 0, 0] for c in base] + [[0, 0]]).astype(np.int64)
    np.testing.assert_array_equal(run_decode([padded], H, W), CR.decode(base, (H, W))[None])


# ---- overlap -----------------------------------------------------------------------------------------------------------
def run_overlap(a, b, shift=0):
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    (n_a, H, W), n_b = a.shape, b.shape[0]
    _, da = device_masks(a, shift)
    _, db = device_masks(b, (2 * shift) % 4)
    inter, aa, ab = guarded(n_a * n_b, torch.int32, -7), guarded(n_a, torch.int32, -7), guarded(n_b, torch.int32, -7)
    _lib.check(L.pgr_mask_overlap(_lib.ptr(da), n_a, _lib.ptr(db), n_b, W, H, _lib.ptr(inter[GUARD:]), _lib.ptr(aa[GUARD:]),
                                  _lib.ptr(ab[GUARD:]), _lib.stream_ptr(da.device)), "pgr_mask_overlap")
    torch.cuda.synchronize()
    assert intact(inter, n_a * n_b, -7) and intact(aa, n_a, -7) and intact(ab, n_b, -7), "overlap guard overwritten"
    return (inter[GUARD:GUARD + n_a * n_b].reshape(n_a, n_b).cpu().numpy(), aa[GUARD:GUARD + n_a].cpu().numpy(),
            ab[GUARD:GUARD + n_b].cpu().numpy())


def check_overlap(a, b, shift=0):
    got = run_overlap(a, b, shift)
    for g, w in zip(got, CR.overlap(a, b)):
        np.testing.assert_array_equal(g.astype(np.int64), w)
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_overlap_equals_numpy(name):
    stack = CASES[name]
    check_overlap(stack, np.ascontiguousarray(stack[::-1, :, ::-1]))          # against the mirrored stack: as a and as b
    check_overlap(np.ascontiguousarray(stack[:, ::-1]), stack)


def test_overlap_shapes_and_special_pairs():
    stack = CASES["odd 17x33"]
    for n_a, n_b in ((1, 1), (1, 3), (3, 1), (3, 3)):
        for shift in (0, 1, 3):
            check_overlap(stack[:n_a], np.ascontiguousarray(stack[:n_b, ::-1]), shift)
    H, W = 33, 17
    outer = np.zeros((H, W), np.uint8); outer[4:30, 2:15] = 255
    inner = np.zeros((H, W), np.uint8); inner[10:20, 5:9] = 1
    apart = np.zeros((H, W), np.uint8); apart[:4] = 2
    inter, aa, ab = check_overlap(np.stack([outer, inner, apart]), np.stack([outer, inner, apart]))
    assert np.diag(inter).tolist() == aa.tolist() == ab.tolist()              # identical
    assert inter[0, 1] == inter[1, 0] == aa[1] == 40                          # nested
    assert inter[0, 2] == inter[2, 0] == inter[1, 2] == 0                     # disjoint


# ---- the Python wrappers -------------------------------------------------------------------------------------------------
def test_wrappers_encode_decode_and_iou():
    import torch
    from pegasus_amd import coco as CO
    stack = CASES["640x480 blobs"]
    dev = torch.from_numpy(stack).cuda()
    counts, offsets, stats = CO.rle_encode(dev)
    want, want_stats = reference("640x480 blobs")
    assert counts.dtype == torch.int32 and counts.is_cuda and isinstance(offsets, np.ndarray) and offsets.dtype == np.int64
    np.testing.assert_array_equal(counts.cpu().numpy(), np.concatenate(want))
    np.testing.assert_array_equal(offsets, np.concatenate([[0], np.cumsum([len(c) for c in want])]))
    np.testing.assert_array_equal(stats.cpu().numpy(), want_stats)
    np.testing.assert_array_equal(CO.mask_stats(dev != 0).cpu().numpy(), want_stats)      # bool tensors are their bytes
    binary = (stack != 0).astype(np.uint8)
    np.testing.assert_array_equal(CO.rle_decode((counts, offsets), size=(480, 640)).cpu().numpy(), binary)
    rles = [{"counts": c.tolist(), "size": [480, 640]} for c in want]
    np.testing.assert_array_equal(CO.rle_decode(rles).cpu().numpy(), binary)
    np.testing.assert_array_equal(CO.rle_decode([c.tolist() for c in want], size=(480, 640)).cpu().numpy(), binary)
    with pytest.raises(ValueError, match="sum to"):
        CO.rle_decode((counts[:-1], np.array([0, len(counts) - 1])), size=(480, 640))
    other = torch.from_numpy(np.ascontiguousarray(stack[:2, ::-1])).cuda()
    ious = CO.mask_ious(other, dev)
    assert ious.dtype == torch.float64 and tuple(ious.shape) == (2, 3)
    np.testing.assert_array_equal(ious.cpu().numpy(), CR.ious(stack[:2, ::-1], stack))
    empty = torch.zeros((1, 480, 640), dtype=torch.uint8, device="cuda")
    assert CO.mask_ious(empty, empty).item() == 0.0                                          # an empty union is 0, not NaN
    golden = np.load(GOLDEN / "coco_rle.npz")
    small = CASES["odd 17x33"]
    inter, a_dt, a_gt = (t.cpu().numpy().astype(np.int64) for t in
                         CO.mask_overlap(torch.from_numpy(np.ascontiguousarray(small[:, ::-1])).cuda(), torch.from_numpy(small).cuda()))
    np.testing.assert_array_equal(a_dt[:, None] + a_gt[None, :] - inter, CC.toolkit_unions(golden["ious_toolkit"]))
    np.testing.assert_array_equal(inter > 0, golden["ious_toolkit"] > 0)


def test_annotations_on_the_device_equal_the_toolkits_scene():
    import torch
    from pegasus_amd import coco as CO
    want = json.loads((GOLDEN / "coco_scene.json").read_text())
    for bbox_type in ("amodal", "modal"):
        images, per = [], {}
        for im_id, inst in CC.scene().items():
            images.append((im_id, f"rgb/{im_id:06d}.png", [CC.SCENE_W, CC.SCENE_H]))
            visib = torch.from_numpy(np.stack([v for _, v, _, _ in inst])).cuda()
            full = torch.from_numpy(np.stack([f for _, _, f, _ in inst])).cuda()
            per[im_id] = CO.annotations(visib, full, [o for o, _, _, _ in inst], [f for _, _, _, f in inst], im_id, bbox_type)
        doc = CO.scene_coco(images, per, [2, 5, 7, 9], want["dataset"])
        assert undated(doc) == undated(want["scene"][bbox_type])


# ---- the writer hook -----------------------------------------------------------------------------------------------------
def check_scene_against_its_pngs(scene, bbox_type, n_expected=None):
    from pegasus_amd import coco as CO, dataset_writer as DW
    name = "scene_gt_coco.json" if bbox_type == "amodal" else "scene_gt_coco_modal.json"
    doc = json.loads((scene / name).read_text())
    gt = json.loads((scene / "scene_gt.json").read_text())
    anns = doc["annotations"]
    assert [a["id"] for a in anns] == list(range(1, len(anns) + 1))
    assert [a["image_id"] for a in anns] == sorted(a["image_id"] for a in anns)                # frame order
    assert [i["id"] for i in doc["images"]] == sorted(int(k) for k in gt)
    want = []
    for i in sorted(gt, key=int):
        for k, e in enumerate(gt[i]):
            visib = DW.decode_png((scene / "mask_visib" / f"{int(i):06d}_{k:06d}.png").read_bytes())
            full = DW.decode_png((scene / "mask" / f"{int(i):06d}_{k:06d}.png").read_bytes()) if bbox_type == "amodal" else visib
            if not visib.any() or not full.any():
                continue
            want.append((int(i), int(e["obj_id"]), visib, CR.bbox(full)))
    assert len(anns) == len(want) and (n_expected is None or len(anns) == n_expected)
    decoded = CO.rle_decode([a["segmentation"] for a in anns]).cpu().numpy()
    for a, (i, obj, visib, box), d in zip(anns, want, decoded):
        assert (a["image_id"], a["category_id"]) == (i, obj)
        np.testing.assert_array_equal(d * 255, visib)
        assert a["area"] == int((visib > 0).sum()) and a["bbox"] == box
        assert a["segmentation"]["size"] == list(visib.shape) and (a["width"], a["height"]) == visib.shape[::-1]
        assert type(a["ignore"]) is bool
    return doc


def test_writer_hook_from_splat_masks_and_a_two_writer_merge(tmp_path):
    import torch
    from pegasus_amd import dataset_writer as DW
    B, K, H, W = 4, 2, 40, 56
    rng = np.random.default_rng(21)
    color = rng.random((B, 3, H, W), dtype=np.float32)
    depth = rng.uniform(0.3, 5.0, (B, 1, H, W)).astype(np.float32)
    sil = np.zeros((B, K, H, W), np.uint8)
    sil[:, 0, 0:20, 10:30] = 1
    sil[:, 1, 12:33, 25:50] = 1
    vis = sil.copy()
    vis[:, 1, 12:20, 25:30] = 0
    vis[2, 0] = 0                                                                # frame 2: object 1 is not visible: skipped, no id
    vis[3, 1] = 0; vis[3, 1, 30, 40] = 1                                         # frame 3: one pixel of 525 visible: ignore
    gt = {str(i): [{"cam_R_m2c": np.eye(3).reshape(-1).tolist(), "cam_t_m2c": [0.0, 0.0, 1.0 + i], "obj_id": k + 3} for k in range(K)]
          for i in range(B)}
    cam = {str(i): {"cam_K": [100.0, 0, 28.0, 0, 100.0, 20.0, 0, 0, 1.0], "depth_scale": 1.0} for i in range(B)}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    writers = []
    for rank in range(2):                                                        # frames 0, 2 and 1, 3: a view-sharded run
        ids = list(range(rank, B, 2))
        w = DW.BopSceneWriter(tmp_path / "ds", workers=1)
        w.add_batch(dict(color=dev(color[ids]), depth=dev(depth[ids]), masks=dev(vis[ids])), {str(j): gt[str(i)] for j, i in enumerate(ids)},
                    {str(j): cam[str(i)] for j, i in enumerate(ids)}, silhouettes=dev(sil[ids]), frame_ids=ids, coco=True)
        w.close(write_json=False)
        assert all("id" not in a for anns in w.scene_gt_coco.values() for a in anns)
        writers.append(w)
    writers[0].merge_records([(writers[1].scene_gt, writers[1].scene_camera, writers[1].scene_gt_info, writers[1].coco_records())])
    writers[0].write_records()
    doc = check_scene_against_its_pngs(writers[0].scene, "amodal", n_expected=B * K - 1)
    assert [a["ignore"] for a in doc["annotations"]] == [False] * 6 + [True]
    assert doc["info"]["description"] == "ds_train" and [c["id"] for c in doc["categories"]] == [3, 4]
    # modal boxes need no silhouettes; amodal ones say that they do
    w = DW.BopSceneWriter(tmp_path / "modal", workers=1)
    w.add_batch(dict(color=dev(color), depth=dev(depth), masks=dev(vis)), gt, cam, coco="modal")
    check_scene_against_its_pngs(w.close(), "modal", n_expected=B * K - 1)
    w = DW.BopSceneWriter(tmp_path / "refused", workers=1)
    with pytest.raises(ValueError, match="coco='modal' only"):
        w.add_batch(dict(color=dev(color), depth=dev(depth), masks=dev(vis)), gt, cam, coco=True)
    w.close(write_json=False)


def test_writer_hook_from_meshes(tmp_path):
    import torch
    import mesh_raster_cases as MC
    from pegasus_amd import dataset_writer as DW, mesh_render as R
    v, f = MC.icosphere(2, 0.06)
    ms = R.MeshSet({1: types.SimpleNamespace(vertices=v, faces=f)})
    W = H = 96
    K = np.array([[120.0, 0, 48.0], [0, 120.0, 48.0], [0, 0, 1.0]])
    poses = [(0.0, 0.0, 0.6), (0.22, 0.0, 0.6), (0.0, -0.05, 0.5), (3.0, 0.0, 0.6)]      # centred, truncated, nearer, outside
    B = len(poses)
    gt = {str(i): [{"cam_R_m2c": np.eye(3).reshape(-1).tolist(), "cam_t_m2c": list(p), "obj_id": 1}] for i, p in enumerate(poses)}
    cam = {str(i): {"cam_K": K.reshape(-1).tolist(), "depth_scale": 1.0} for i in range(B)}
    own = R.render_depth(ms, [(1, np.eye(3), np.asarray(p)) for p in poses], K, (W, H))
    depth_m = torch.where(own > 0, own, torch.full_like(own, 6.0))
    depth_m[0, :, : W // 2] = 0.2                                                # an occluder over the left half of frame 0
    frames = {"color": torch.zeros((B, 3, H, W), device="cuda"), "depth": depth_m[:, None].contiguous()}
    w = DW.BopSceneWriter(tmp_path / "mesh", workers=1)
    w.add_batch(frames, gt, cam, meshes=ms, delta=15.0, translation_scale=1.0, coco="amodal")
    doc = check_scene_against_its_pngs(w.close(), "amodal", n_expected=3)        # the object outside the image has no annotation
    info = json.loads((w.scene / "scene_gt_info.json").read_text())
    for a in doc["annotations"]:
        assert a["ignore"] == (info[str(a["image_id"])][0]["visib_fract"] < 0.1)
