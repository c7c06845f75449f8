"""COCO annotations without a device: the NumPy restatement against the BOP toolkit's recorded outputs, scene_coco's
numbering, skips and ignore flags, recompute_dataset over a written dataset through the NumPy backend, and the argument
checks of every new entry point (host-side, before any launch)."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import coco_cases as CC
import coco_reference as CR

GOLDEN = Path(__file__).resolve().parent / "golden"
DATES = CC.DATES
undated, golden_cases = CC.undated, CC.golden_cases


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "coco_rle.npz")


@pytest.fixture(scope="module")
def golden_json():
    return json.loads((GOLDEN / "coco_scene.json").read_text())


def test_cases_cover_what_the_kernels_can_get_wrong():
    names = [n for n, _, _ in CC.cases()]
    assert len(names) == len(set(names))
    shapes = {s.shape[1:] for _, s, _ in CC.cases()}
    for W in (CC.TILE_COLS - 1, CC.TILE_COLS, CC.TILE_COLS + 1):
        assert any(s[1] == W for s in shapes)
    for H in (CC.WORD_ROWS - 1, CC.WORD_ROWS, CC.WORD_ROWS + 1, CC.BLOCK_ROWS - 1, CC.BLOCK_ROWS, CC.BLOCK_ROWS + 1):
        assert any(s[0] == H for s in shapes)
    for unit in {CC.DECODE_MIN_SLICE, CC.OVERLAP_CHUNK}:
        for px in (unit - 1, unit, unit + 1):
            assert any(s[0] * s[1] == px for s in shapes)
    most = CC.DECODE_MAX_SLICES * CC.DECODE_MIN_SLICE
    pixels = sorted(s[0] * s[1] for s in shapes)
    assert most in pixels and most - 1 in pixels and any(most < px <= most + 64 for px in pixels)
    lengths = {len(CR.rle_counts(m)) for _, s, _ in CC.cases() if s.shape[1] * s.shape[2] < 1000 for m in s}
    assert {CC.DECODE_CHUNK - 1, CC.DECODE_CHUNK, CC.DECODE_CHUNK + 1} <= lengths


def test_reference_equals_the_toolkit_on_every_case(golden):
    n = 0
    for name, stack, counts, boxes, decoded in golden_cases(golden):
        for k, m in enumerate(stack):
            np.testing.assert_array_equal(CR.rle_counts(m), counts[k], err_msg=name)
            assert int(counts[k].sum()) == m.size
            np.testing.assert_array_equal(CR.decode(counts[k], m.shape), decoded[k], err_msg=name)
            np.testing.assert_array_equal(decoded[k], (m != 0).astype(np.uint8), err_msg=name)
            if m.any():
                assert CR.bbox(m) == boxes[k].tolist(), name
            n += 1
    assert n >= 60
    H, W = (int(v) for v in golden["zero_size"])
    ends = np.cumsum(golden["zero_lengths"])
    for c, want in zip(np.split(golden["zero_counts"], ends[:-1]), golden["zero_decoded"]):
        np.testing.assert_array_equal(CR.decode(c, (H, W)), want)


def test_reference_overlap_against_the_toolkits_unions(golden):
    """compute_ious: only its unions and `intersection > 0` are comparable -- its einsum over booleans yields any-overlap,
    so what it returns is 1 / union where two masks overlap and 0 elsewhere.  Every pair of this case overlaps, so the
    toolkit's unions are the rounded reciprocals of what it returned."""
    stack = dict((n, s) for n, s, _ in CC.cases())["odd 17x33"]
    other = stack[:, ::-1].copy()
    inter, a_dt, a_gt = CR.overlap(other, stack)
    unions = a_dt[:, None] + a_gt[None, :] - inter
    assert (golden["ious_toolkit"] > 0).all()
    np.testing.assert_array_equal(unions, CC.toolkit_unions(golden["ious_toolkit"]))
    np.testing.assert_array_equal(inter > 0, golden["ious_toolkit"] > 0)
    np.testing.assert_allclose(golden["ious_toolkit"], (inter > 0) / unions, rtol=1e-15)
    assert (CR.ious(other, stack) > golden["ious_toolkit"]).all()          # the true IoU is not what the toolkit returns


def test_annotation_dicts_equal_the_toolkits(golden_json):
    from pegasus_amd import coco as CO
    stacks = {name: stack for name, stack, _ in CC.cases()}
    seen = 0
    for key, want in golden_json["annotation_info"].items():
        name, k = key.rsplit("/", 1)
        m = stacks[name][int(k)][None]
        got = CO.annotations(m, m, [11], [0.05 if int(k) % 2 else 0.9], 3, "amodal", backend=CR)
        if want is None:
            assert got == []
            continue
        assert len(got) == 1 and {"id": 7, **got[0]} == want, key
        assert type(got[0]["ignore"]) is bool and list(got[0]) == [k for k in want if k != "id"]
        seen += 1
    assert seen >= 30


def scene_inputs():
    images, per = [], {}
    from pegasus_amd import coco as CO
    for im_id, inst in CC.scene().items():
        images.append((im_id, f"rgb/{im_id:06d}.png", [CC.SCENE_W, CC.SCENE_H]))
        visib = np.stack([v for _, v, _, _ in inst])
        full = np.stack([f for _, _, f, _ in inst])
        per[im_id] = {bt: CO.annotations(visib, full, [o for o, _, _, _ in inst], [f for _, _, _, f in inst], im_id, bt, backend=CR)
                      for bt in ("amodal", "modal")}
    return images, per


@pytest.mark.parametrize("bbox_type", ["amodal", "modal"])
def test_scene_coco_numbering_skips_and_ignore(golden_json, bbox_type):
    from pegasus_amd import coco as CO
    images, per = scene_inputs()
    doc = CO.scene_coco(list(reversed(images)), {k: v[bbox_type] for k, v in per.items()}, [2, 5, 7, 9], golden_json["dataset"])
    want = golden_json["scene"][bbox_type]
    assert undated(doc) == undated(want)
    assert [a["id"] for a in doc["annotations"]] == list(range(1, len(want["annotations"]) + 1))
    assert len(want["annotations"]) == (4 if bbox_type == "amodal" else 5)       # one skip always, one more with amodal boxes
    assert [a["ignore"] for a in doc["annotations"]].count(True) == 1
    assert set(doc["info"]) >= set(DATES[:1]) | {"year"} and "date_captured" in doc["images"][0]
    json.dumps(doc)                                                              # plain JSON types throughout


@pytest.mark.parametrize("bbox_type", ["amodal", "modal"])
def test_recompute_dataset_reads_a_written_directory(tmp_path, golden_json, bbox_type):
    from pegasus_amd import coco as CO, dataset_writer as DW
    root = tmp_path / golden_json["dataset"]
    scene = root / "train" / "000000"
    for d in ("rgb", "mask", "mask_visib"):
        (scene / d).mkdir(parents=True)
    gt, info = {}, {}
    for im_id, inst in CC.scene().items():
        (scene / "rgb" / f"{im_id:06d}.png").write_bytes(DW.encode_png(np.zeros((CC.SCENE_H, CC.SCENE_W, 3), np.uint8)))
        gt[str(im_id)] = [{"cam_R_m2c": np.eye(3).reshape(-1).tolist(), "cam_t_m2c": [0, 0, 1.0], "obj_id": o} for o, _, _, _ in inst]
        info[str(im_id)] = [{"visib_fract": f} for _, _, _, f in inst]
        for k, (_, visib, full, _) in enumerate(inst):
            (scene / "mask_visib" / f"{im_id:06d}_{k:06d}.png").write_bytes(DW.encode_png((visib != 0).astype(np.uint8) * 255))
            (scene / "mask" / f"{im_id:06d}_{k:06d}.png").write_bytes(DW.encode_png((full != 0).astype(np.uint8) * 255))
    (scene / "scene_gt.json").write_text(json.dumps({k: gt[k] for k in sorted(gt, reverse=True)}))      # file order is not id order
    (scene / "scene_gt_info.json").write_text(json.dumps(info))
    scenes = CO.recompute_dataset(root, bbox_type, backend=CR, batch=1 if bbox_type == "modal" else 8)
    assert scenes == [scene]
    name = "scene_gt_coco.json" if bbox_type == "amodal" else "scene_gt_coco_modal.json"
    got = json.loads((scene / name).read_text())
    assert undated(got) == undated(golden_json["scene"][bbox_type])


def test_recompute_dataset_takes_the_image_size_from_rgb_then_the_first_mask_then_zero(tmp_path):
    """Image 0 has an rgb PNG 7 wide and 2 high beside a 5 x 3 mask, image 1 only masks (the first one's header counts),
    image 2 neither."""
    from pegasus_amd import coco as CO, dataset_writer as DW
    scene = tmp_path / "ds" / "train" / "000004"
    for d in ("rgb", "mask_visib"):
        (scene / d).mkdir(parents=True)
    mask = np.zeros((3, 5), np.uint8)
    mask[1, 1:4] = 255
    (scene / "rgb" / "000000.png").write_bytes(DW.encode_png(np.zeros((2, 7, 3), np.uint8)))
    for name in ("000000_000000.png", "000001_000000.png", "000001_000001.png"):
        (scene / "mask_visib" / name).write_bytes(DW.encode_png(mask))
    gt = {"0": [{"obj_id": 3}], "1": [{"obj_id": 3}, {"obj_id": 5}], "2": []}
    (scene / "scene_gt.json").write_text(json.dumps(gt))
    assert CO.recompute_dataset(tmp_path / "ds", "modal", backend=CR, batch=1) == [scene]
    doc = json.loads((scene / "scene_gt_coco_modal.json").read_text())
    assert [(i["id"], i["file_name"], i["width"], i["height"]) for i in doc["images"]] == [
        (0, "rgb/000000.png", 7, 2), (1, "rgb/000001.png", 5, 3), (2, "rgb/000002.png", 0, 0)]
    assert [(a["image_id"], a["category_id"], a["bbox"]) for a in doc["annotations"]] == [(0, 3, [1, 1, 3, 1]), (1, 3, [1, 1, 3, 1]),
                                                                                           (1, 5, [1, 1, 3, 1])]


def test_writer_merges_annotations_and_numbers_after_the_merge(tmp_path, golden_json):
    """Two writers of one scene (a view-sharded run): each keeps its frames' annotations WITHOUT ids; the merged writer
    numbers them in frame order -- also one that added no frame of its own and has box type and size from the others."""
    from pegasus_amd import dataset_writer as DW
    images, per = scene_inputs()
    writers = []
    for rank, im_id in enumerate(sorted(per)):
        w = DW.BopSceneWriter(tmp_path / golden_json["dataset"], workers=1)
        w.scene_gt[str(im_id)] = [{"obj_id": o} for o, _, _, _ in CC.scene()[im_id]]
        w.scene_camera[str(im_id)] = {}
        w.scene_gt_coco[str(im_id)] = per[im_id]["amodal"]
        w.coco_bbox_type, w.coco_size = "amodal", (CC.SCENE_W, CC.SCENE_H)
        assert all("id" not in a for a in w.scene_gt_coco[str(im_id)])
        writers.append(w)
    record = lambda w: (w.scene_gt, w.scene_camera, w.scene_gt_info, w.coco_records())
    empty = DW.BopSceneWriter(tmp_path / golden_json["dataset"], workers=1)
    assert empty.coco_records() is None
    for root, others in ((writers[1], [writers[0]]), (empty, [writers[1], writers[0]])):      # the LATER frame merges; no frame at all
        root.merge_records([record(w) for w in others])
        root.merge_records([({}, {}), ({}, {}, {}), ({}, {}, {}, None)])         # shorter tuples, and ranks without annotations
        scene = root.close()
        got = json.loads((scene / "scene_gt_coco.json").read_text())
        assert undated(got) == undated(golden_json["scene"]["amodal"])
        (scene / "scene_gt_coco.json").unlink()
    modal = DW.BopSceneWriter(tmp_path / golden_json["dataset"], workers=1)
    modal.coco_bbox_type, modal.coco_size = "modal", (CC.SCENE_W, CC.SCENE_H)
    with pytest.raises(ValueError, match="do not go with"):
        modal.merge_records([record(writers[0])])
    modal.close(write_json=False)


def test_default_writer_writes_no_coco_file(tmp_path):
    from pegasus_amd import dataset_writer as DW
    w = DW.BopSceneWriter(tmp_path / "ds", workers=1)
    w.scene_gt["0"], w.scene_camera["0"] = [], {}
    scene = w.close()
    assert not list(scene.glob("scene_gt_coco*"))


def test_mirrored_tile_sizes_are_the_headers():
    """The shapes the cases are built around are the #defines of include/pegasus_raster.h, not retyped values."""
    import re
    from pegasus_amd import _lib
    text = (Path(__file__).resolve().parents[1] / "include" / "pegasus_raster.h").read_text()
    defines = {k: int(v) for k, v in re.findall(r"^#define (PGR_(?:RLE|MASK)_[A-Z_]+)\s+(\d+)", text, flags=re.M)}
    assert set(defines) == {"PGR_RLE_WORD_ROWS", "PGR_RLE_TILE_COLS", "PGR_RLE_BLOCK_ROWS", "PGR_RLE_DECODE_CHUNK",
                            "PGR_RLE_DECODE_MIN_SLICE", "PGR_RLE_DECODE_MAX_SLICES", "PGR_MASK_OVERLAP_CHUNK"}
    for name, value in defines.items():
        assert getattr(_lib, name) == value, name
    assert (CC.WORD_ROWS, CC.TILE_COLS, CC.BLOCK_ROWS, CC.DECODE_CHUNK, CC.DECODE_MIN_SLICE, CC.DECODE_MAX_SLICES, CC.OVERLAP_CHUNK) == tuple(
        defines[k] for k in ("PGR_RLE_WORD_ROWS", "PGR_RLE_TILE_COLS", "PGR_RLE_BLOCK_ROWS", "PGR_RLE_DECODE_CHUNK",
                             "PGR_RLE_DECODE_MIN_SLICE", "PGR_RLE_DECODE_MAX_SLICES", "PGR_MASK_OVERLAP_CHUNK"))


def test_recompute_refuses_a_batch_below_one(tmp_path):
    from pegasus_amd import coco as CO
    (tmp_path / "train").mkdir()
    for batch in (0, -3):
        with pytest.raises(ValueError, match="at least one image"):
            CO.recompute_dataset(tmp_path, backend=CR, batch=batch)


# ---- argument checks: host-side, no device is touched ------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import _lib, build
    build.build()
    return _lib.lib()


FAKE = C.c_void_p(0x10000)
INVALID, TOO_SMALL = -1, -2


def test_workspace_size_is_host_only(lib):
    assert lib.pgr_mask_rle_workspace_bytes(1, 1, 1) > 0
    one, eight = lib.pgr_mask_rle_workspace_bytes(1, 800, 800), lib.pgr_mask_rle_workspace_bytes(8, 800, 800)
    assert 800 * 800 // 8 + 16 * 800 <= one <= 800 * 800 // 4 and 7 * one <= eight <= 8 * one
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8193, 8), (1, 8, 8193), (1, -5, 8)):
        assert lib.pgr_mask_rle_workspace_bytes(*bad) == 0
    assert lib.pgr_mask_rle_workspace_bytes(1, 8192, 8192) > 0


def test_count_refuses_bad_arguments(lib):
    need = lib.pgr_mask_rle_workspace_bytes(2, 17, 33)
    ok = dict(masks=FAKE, n=2, w=17, h=33, stats=FAKE, ws=FAKE, nbytes=need)

    def rc(**kw):
        a = {**ok, **kw}
        return lib.pgr_mask_rle_count(a["masks"], a["n"], a["w"], a["h"], a["stats"], a["ws"], a["nbytes"], None)
    for kw in (dict(masks=None), dict(stats=None), dict(ws=None), dict(n=0), dict(n=-3), dict(w=0), dict(h=0), dict(w=8193),
               dict(h=8193), dict(ws=C.c_void_p(0x10004))):
        assert rc(**kw) == INVALID, kw
    assert rc(nbytes=need - 1) == TOO_SMALL and rc(nbytes=0) == TOO_SMALL


def test_emit_refuses_bad_arguments(lib):
    need = lib.pgr_mask_rle_workspace_bytes(2, 17, 33)
    ok = dict(masks=FAKE, n=2, w=17, h=33, offsets=FAKE, total=10, counts=FAKE, cap=10, ws=FAKE, nbytes=need)

    def rc(**kw):
        a = {**ok, **kw}
        return lib.pgr_mask_rle_emit(a["masks"], a["n"], a["w"], a["h"], a["offsets"], a["total"], a["counts"], a["cap"], a["ws"],
                                     a["nbytes"], None)
    for kw in (dict(masks=None), dict(offsets=None), dict(counts=None), dict(ws=None), dict(n=0), dict(n=-1), dict(w=0), dict(h=0),
               dict(w=8193), dict(h=8193), dict(cap=9), dict(cap=0), dict(total=1), dict(total=2 * (17 * 33 + 1) + 1, cap=1 << 20)):
        assert rc(**kw) == INVALID, kw
    assert rc(nbytes=need - 1) == TOO_SMALL


def test_decode_and_overlap_refuse_bad_arguments(lib):
    def dec(counts=FAKE, offsets=FAKE, n=2, w=17, h=33, masks=FAKE):
        return lib.pgr_mask_rle_decode(counts, offsets, n, w, h, masks, None)
    for kw in (dict(counts=None), dict(offsets=None), dict(masks=None), dict(n=0), dict(n=-1), dict(w=0), dict(h=0), dict(w=8193),
               dict(h=8193)):
        assert dec(**kw) == INVALID, kw

    def ov(a=FAKE, n_a=1, b=FAKE, n_b=3, w=17, h=33, inter=FAKE, area_a=FAKE, area_b=FAKE):
        return lib.pgr_mask_overlap(a, n_a, b, n_b, w, h, inter, area_a, area_b, None)
    for kw in (dict(a=None), dict(b=None), dict(inter=None), dict(area_a=None), dict(area_b=None), dict(n_a=0), dict(n_b=0),
               dict(n_a=-1), dict(w=0), dict(h=0), dict(w=8193), dict(h=8193)):
        assert ov(**kw) == INVALID, kw


def test_decode_wrapper_refuses_bad_lists_before_any_call():
    from pegasus_amd import coco as CO
    with pytest.raises(ValueError, match="sum to 19, not to H\\*W = 20"):
        CO.rle_decode([[3, 2, 15], [4, 15]], size=(5, 4), device="cpu")
    with pytest.raises(ValueError, match="sum to 21"):
        CO.rle_decode([{"counts": [0, 21], "size": [5, 4]}], device="cpu")
    with pytest.raises(ValueError, match="negative"):
        CO.rle_decode([[25, -5]], size=(5, 4), device="cpu")
    with pytest.raises(ValueError, match="compressed RLE.*pycocotools"):
        CO.rle_decode([{"counts": "PPYo1", "size": [5, 4]}], device="cpu")
    with pytest.raises(ValueError, match="share one size"):
        CO.rle_decode([{"counts": [20], "size": [5, 4]}, {"counts": [20], "size": [4, 5]}], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        CO.rle_decode([[20]], size=(5, 4), device="cpu")


def test_device_wrappers_refuse_host_tensors_and_bad_box_types():
    import torch
    from pegasus_amd import coco as CO
    m = torch.zeros((1, 4, 4), dtype=torch.uint8)
    for fn in (CO.rle_encode, CO.mask_stats):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        CO.mask_ious(m, m)
    with pytest.raises(ValueError, match="not a valid bounding box type"):
        CO.annotations(m.numpy(), m.numpy(), [1], [1.0], 0, "tight", backend=CR)
    with pytest.raises(ValueError, match="only bbox_type='modal'"):
        CO.annotations(m.numpy(), None, [1], [1.0], 0, "amodal", backend=CR)
    assert CO.bbox_from_stats(np.array([[3, 6, 2, 5, 4, 9]])).tolist() == [[2, 5, 3, 5]]
