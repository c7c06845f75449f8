"""The COCO score rule without a GPU: the string codec, hand-worked answers asserted on the NumPy restatement
(tests/coco_eval_reference.py) so that the rule is pinned before any kernel is, a census of the random cases, the host side
of pegasus_amd.coco_eval (grouping, loaders, file names, the time rule) and the entry points' argument checks."""
import ctypes as C
import json

import numpy as np
import pytest

import coco_eval_cases as CC
import coco_eval_reference as CR

AP51, AP_TFT = 51 / 101, (51 + 50 * (2 / 3)) / 101
ONE_OF_ONE = 1.0 / (1.0 + 2.0 ** -52)                # pr of a lone true positive: tp / (fp + tp + np.spacing(1))


def box_gt(boxes, areas=None, crowd=None, ignore=None, cats=None, images=None, n_images=1, n_cats=1):
    n = len(boxes)
    return {"images": [{"id": i + 1, "width": 640, "height": 480} for i in range(n_images)],
            "categories": [{"id": c + 1} for c in range(n_cats)],
            "annotations": [{"id": k + 1, "image_id": images[k] if images else 1, "category_id": cats[k] if cats else 1,
                             "bbox": list(boxes[k]), "area": areas[k] if areas else boxes[k][2] * boxes[k][3],
                             "iscrowd": crowd[k] if crowd else 0, "ignore": ignore[k] if ignore else False} for k in range(n)]}


def box_dt(boxes, scores, cats=None, images=None):
    return [{"image_id": images[k] if images else 1, "category_id": cats[k] if cats else 1, "bbox": list(b), "score": scores[k]}
            for k, b in enumerate(boxes)]


def stats(gt, dt, iou_type="bbox", **params):
    return dict(zip(CR.STAT_NAMES, CR.evaluate(gt, dt, iou_type, CR.default_params(**params))["stats"]))


# ---- the string codec -------------------------------------------------------------------------------------------------
def test_hand_derived_strings():
    """[5, 3, 40]: 5 -> group 5, nothing left, no bit 0x10: '5' (53).  3 -> '3'.  40 -> group 40 & 31 = 8, x = 1 left and bit
    0x10 clear, so more follow: 8 | 0x20 = 40 -> chr(88) = 'X'; then group 1, x = 0: chr(49) = '1'.  "53X1".
    [0, 17, 4, 2]: 0 -> '0'.  17 -> group 17 has bit 0x10 and x = 0 != -1, so more follow: 17 | 0x20 = 49 -> chr(97) = 'a';
    then group 0, x = 0, bit 0x10 clear: '0'.  4 -> '4'.  The fourth count is written as 2 - counts[1] = -15: group -15 & 31 =
    17, x = -15 >> 5 = -1, bit 0x10 set and x == -1: the last group, chr(65) = 'A'.  "0a04A"."""
    from pegasus_amd.coco_eval import rle_string_decode, rle_string_encode
    assert rle_string_encode([5, 3, 40]) == "53X1" and rle_string_decode("53X1") == [5, 3, 40]
    assert rle_string_encode([0, 17, 4, 2]) == "0a04A" and rle_string_decode("0a04A") == [0, 17, 4, 2]
    assert CR.string_decode("53X1") == [5, 3, 40] and CR.string_decode("0a04A") == [0, 17, 4, 2]
    assert rle_string_decode(b"0a04A") == [0, 17, 4, 2]
    with pytest.raises(ValueError, match="ends inside"):
        rle_string_decode("0a")[0]
    with pytest.raises(ValueError, match="not part of"):
        rle_string_decode("0 ")


def test_string_round_trip():
    from pegasus_amd.coco_eval import rle_string_decode, rle_string_encode
    rng = np.random.default_rng(5)
    lists = [c for size in (CC.SMALL, CC.LARGE) for c in CC.family(size, rng).values()]
    lists += [[1 << 20, 5, (1 << 20) + 3, 2, 1 << 27, 0, 0, 31, 32, 15, 16, 1023, 1024, 2 ** 31 - 1], [10, 20, 30, 5], [0], [7],
              [16, 16, 16, 0, 0, 48], [100, 1, 1, 100, 100, 1]]
    for c in lists:
        s = rle_string_encode(c)
        assert all(48 <= ord(ch) < 112 for ch in s)
        assert rle_string_decode(s) == list(c) and CR.string_decode(s) == list(c)


# ---- hand-worked answers, on the reference ----------------------------------------------------------------------------------
def test_perfect_detections_score_one_where_there_is_ground_truth():
    """Six GT, two per range (areas 100 and 400 small, 2000 and 2500 medium, 10000 and 14400 large), each detected exactly
    with a distinct score: every detection is a TP at every threshold.  In every range tp reaches 2, and 2 / (0 + 2 + 2^-52)
    is exactly 1 (the sum rounds to 2), which the running maximum from the right carries to the front: pr = 1 everywhere,
    rc reaches 1, and every AP / AR is exactly 1 -- but AR1 = 1/6: one detection per image is kept and the image has six GT.
    A range with ONE counted GT stops at tp = 1, and 1 / (0 + 1 + 2^-52) = 0.9999999999999998: 1 + 2^-52 is a float64.
    That is COCOeval's own answer for a perfectly detected single instance, and it is kept.  With the large GT removed
    their range holds no GT: npig = 0 and AP_large = AR_large = -1."""
    boxes = [[0, 0, 10, 10], [20, 0, 20, 20], [100, 0, 50, 40], [100, 100, 50, 50], [200, 200, 100, 100], [400, 0, 120, 120]]
    s = stats(box_gt(boxes), box_dt(boxes, [0.9, 0.85, 0.8, 0.75, 0.7, 0.65]))
    assert {k: v for k, v in s.items() if k != "AR1"} == dict(AP=1.0, AP50=1.0, AP75=1.0, AP_small=1.0, AP_medium=1.0, AP_large=1.0,
                                                              AR10=1.0, AR100=1.0, AR_small=1.0, AR_medium=1.0, AR_large=1.0)
    assert s["AR1"] == pytest.approx(1 / 6, abs=1e-15)
    s = stats(box_gt(boxes[:4:2]), box_dt(boxes[:4:2], [0.9, 0.8]))
    assert s["AP"] == 1.0 and s["AP_large"] == -1.0 and s["AR_large"] == -1.0 and s["AR1"] == 0.5 and s["AR100"] == 1.0
    assert s["AP_small"] == pytest.approx(ONE_OF_ONE, abs=1e-16) and s["AP_medium"] == pytest.approx(ONE_OF_ONE, abs=1e-16)
    assert ONE_OF_ONE == 0.9999999999999998


def test_no_detections_score_zero():
    """npig > 0 and no detection: recall is 0 and every precision cell is 0 (searchsorted runs off the empty list)."""
    s = stats(box_gt([[0, 0, 50, 40]]), [])
    assert s["AP"] == 0.0 and s["AP50"] == 0.0 and s["AR100"] == 0.0 and s["AP_medium"] == 0.0 and s["AP_small"] == -1.0


def three_detections():
    gt = box_gt([[0, 0, 50, 40], [100, 0, 50, 40]])
    dt = box_dt([[0, 0, 50, 40], [0, 0, 50, 24], [100, 0, 50, 30.8]], [0.9, 0.8, 0.7])
    return gt, dt


def test_three_detections_worked_by_hand():
    """Two medium GT of area 2000.  d1 = g1: IoU 1.  d2 = [0,0,50,24]: inter 1200, union 2000, IoU 0.6 with g1, 0 with g2.
    d3 = [100,0,50,30.8]: IoU 0.77 with g2.  d1 takes g1 at every threshold, so d2 finds g1 matched and g2 at IoU 0: FP
    everywhere.  d3 is a TP while t <= 0.75 and an FP from 0.8 on.
    t in .5 .. .75 (six thresholds): tp = 1,1,2  fp = 0,1,1  rc = .5,.5,1  pr = 1,.5,2/3 -> from the right 1, 2/3, 2/3
      (the leading 1 is 1 / (1 + 2^-52), one ulp below: the comparisons here allow 1e-15).
      The 51 recall thresholds 0 .. .5 land on index 0 (pr 1), the 50 above on index 2 (pr 2/3): AP_t = (51 + 50 * 2/3) / 101.
    t in .8 .. .95 (four): tp = 1,1,1  fp = 0,1,2  rc = .5,.5,.5  pr = 1,.5,1/3; thresholds above .5 find nothing (0):
      AP_t = 51 / 101.
    AP = (6 (51 + 100/3) / 101 + 4 * 51 / 101) / 10; AP50 = AP75 = (51 + 100/3) / 101; recall 1 six times and .5 four times:
    AR100 = AR10 = 0.8; AR1 keeps d1 alone: 0.5.  Both GT are medium: small and large are -1."""
    gt, dt = three_detections()
    out = CR.evaluate(gt, dt, "bbox")
    ap_t = out["precision"][:, :, 0, 0, 2].mean(1)
    np.testing.assert_allclose(ap_t[:6], AP_TFT, rtol=0, atol=1e-15)
    np.testing.assert_allclose(ap_t[6:], AP51, rtol=0, atol=1e-15)
    s = dict(zip(CR.STAT_NAMES, out["stats"]))
    assert s["AP"] == pytest.approx((6 * AP_TFT + 4 * AP51) / 10, abs=1e-15)
    assert s["AP50"] == pytest.approx(AP_TFT, abs=1e-15) and s["AP75"] == pytest.approx(AP_TFT, abs=1e-15)
    assert s["AP_medium"] == s["AP"] and s["AP_small"] == -1.0 and s["AP_large"] == -1.0
    assert s["AR1"] == 0.5 and s["AR10"] == pytest.approx(0.8) and s["AR100"] == pytest.approx(0.8) and s["AR_medium"] == s["AR100"]
    g = out["groups"][1, 1]
    assert g["ious"][0, 0] == 1.0 and g["ious"][1, 0] == 0.6 and g["ious"][1, 1] == 0.0 and abs(g["ious"][2, 1] - 0.77) < 1e-12
    assert g["per"][0][0][:, 1].tolist() == [-1] * 10 and g["per"][0][0][:, 2].tolist() == [1] * 6 + [-1] * 4


def test_a_detection_matched_to_an_ignored_gt_is_neither_tp_nor_fp():
    """One counted GT g1 (detected exactly, score .9) and one crowd GT g2 detected exactly with score .8.  d2 matches g2
    and takes its ignore flag: tp = 1, fp = 0 at both positions, AP = 1 / (1 + 2^-52) (a lone TP).  Were it an FP, pr would be 1, .5."""
    boxes = [[0, 0, 50, 40], [100, 0, 50, 40]]
    gt, dt = box_gt(boxes, crowd=[0, 1]), box_dt(boxes, [0.9, 0.8])
    out = CR.evaluate(gt, dt, "bbox")
    assert dict(zip(CR.STAT_NAMES, out["stats"]))["AP"] == pytest.approx(ONE_OF_ONE, abs=1e-16)       # (one counted GT)
    dtm, dt_ig, _, gt_ig = out["groups"][1, 1]["per"][0]
    assert gt_ig.tolist() == [False, True] and dtm[0].tolist() == [0, 1] and dt_ig[0].tolist() == [False, True]


def test_a_second_detection_on_a_crowd_is_not_a_false_positive():
    """g1 counted and detected; g2 a crowd; d2 and d3 both lie inside g2 (IoU against a crowd = inter / area_d = 1).  A
    matched crowd stays open, so d3 matches it too and is ignored like d2: AP = 1 / (1 + 2^-52).  With g2 not a crowd but ignored by
    its area instead, d3 finds it taken: unmatched, inside the range, an FP: pr = 1, 1, 1/2 after the ignored d2."""
    gt = box_gt([[0, 0, 50, 40], [100, 0, 200, 200]], crowd=[0, 1])
    dt = box_dt([[0, 0, 50, 40], [110, 10, 50, 40], [150, 100, 50, 40]], [0.9, 0.8, 0.7])
    out = CR.evaluate(gt, dt, "bbox")
    dtm, dt_ig, _, _ = out["groups"][1, 1]["per"][0]
    assert dtm[0].tolist() == [0, 1, 1] and dt_ig[0].tolist() == [False, True, True]
    assert dict(zip(CR.STAT_NAMES, out["stats"]))["AP"] == pytest.approx(ONE_OF_ONE, abs=1e-16)


def test_the_break_prefers_a_counted_match():
    """One detection d = [0,0,50,40].  g1 (file order first) is a crowd that contains it: IoU 1.  g2 is counted and overlaps d
    with IoU 5/6 ([0,0,50,48]: inter 2000, union 2400).  The walk starts with the counted GT (sorted first): at t <= .8 d
    matches g2, and the walk breaks at the ignored g1 although its IoU is higher: a TP.  At t >= .85 g2 fails the threshold,
    m stays -1, no break: d matches the crowd and is ignored.  Recall is 1 for seven thresholds and 0 for three."""
    gt = box_gt([[0, 0, 100, 100], [0, 0, 50, 48]], crowd=[1, 0], areas=[10000, 2400])
    dt = box_dt([[0, 0, 50, 40]], [0.9])
    out = CR.evaluate(gt, dt, "bbox")
    dtm, dt_ig, gtm, gt_ig = out["groups"][1, 1]["per"][0]
    assert out["groups"][1, 1]["ious"].tolist() == [[1.0, 2000 / 2400]]
    assert dtm[:, 0].tolist() == [1] * 7 + [0] * 3 and dt_ig[:, 0].tolist() == [False] * 7 + [True] * 3
    assert gtm[:, 0].tolist() == [-1] * 7 + [0] * 3 and gt_ig.tolist() == [True, False]
    assert out["recall"][:, 0, 0, 2].tolist() == [1.0] * 7 + [0.0] * 3


def ignore_field_case():
    """g1 detected exactly; g2 carries ignore = True and is not detected."""
    gt = box_gt([[0, 0, 50, 40], [100, 0, 50, 40]], ignore=[False, True])
    return gt, box_dt([[0, 0, 50, 40]], [0.9])


def test_use_ignore_field_changes_ap_and_the_default_does_not_read_ignore():
    """By default (COCOeval) g2 counts: npig = 2, rc = .5, the 51 thresholds up to .5 get pr 1: AP = 51/101.  With
    use_ignore_field g2 is ignored: npig = 1, rc = 1: AP = 1 / (1 + 2^-52), a lone true positive.  The default equals the same set with the field removed."""
    gt, dt = ignore_field_case()
    assert stats(gt, dt)["AP"] == pytest.approx(AP51, abs=1e-15)
    assert stats(gt, dt, use_ignore_field=True)["AP"] == pytest.approx(ONE_OF_ONE, abs=1e-16)
    bare = json.loads(json.dumps(gt))
    for a in bare["annotations"]:
        del a["ignore"]
    assert stats(bare, dt) == stats(gt, dt)


# ---- the random cases hold what they are meant to hold --------------------------------------------------------------------
def test_census_of_the_cases():
    found = dict(matched_to_ignored=0, crowd_rematch=0, tie_across_images=0, unmatched_ignored_by_area=0, npig_zero=0, over_100=0,
                 gt_counts=set(), dt_counts=set(), empty_images=0, idle_categories=0)
    for name, (gt, dt) in CC.evaluation_sets().items():
        for iou_type in ("segm", "bbox"):
            out = CR.evaluate(gt, dt, iou_type)
            raw = {}
            for r in dt:
                raw[r["image_id"], r["category_id"]] = raw.get((r["image_id"], r["category_id"]), 0) + 1
            found["over_100"] += sum(v > 100 for v in raw.values())
            found["dt_counts"] |= set(raw.values()) | ({0} if any((i, c) not in raw for (i, c) in out["groups"]) else set())
            found["npig_zero"] += int((out["recall"] == -1).any())
            with_anything = {i for (i, c) in out["groups"]}
            found["empty_images"] += sum(i not in with_anything for i in out["img_ids"])
            found["idle_categories"] += sum(all(c != r["category_id"] for r in dt) and any(a["category_id"] == c for a in gt["annotations"])
                                            for c in out["cat_ids"])
            by_score = {}
            for (i, c), g in out["groups"].items():
                found["gt_counts"].add(len(g["g"]))
                for s in g["scores"]:
                    by_score.setdefault((c, s), set()).add(i)
                for dtm, dt_ig, gtm, gt_ig in g["per"]:
                    matched = dtm > -1
                    found["matched_to_ignored"] += int((matched & dt_ig).sum())
                    found["unmatched_ignored_by_area"] += int((~matched & dt_ig).sum())
                    for t in range(dtm.shape[0]):
                        hit = dtm[t][matched[t]]
                        found["crowd_rematch"] += len(hit) - len(set(hit.tolist()))
            found["tie_across_images"] += sum(len(v) > 1 for v in by_score.values())
    assert found["matched_to_ignored"] > 0 and found["crowd_rematch"] > 0 and found["tie_across_images"] > 0
    assert found["unmatched_ignored_by_area"] > 0 and found["npig_zero"] > 0 and found["over_100"] > 0
    assert {0, 1, 2, 63, 64, 65} <= found["gt_counts"] and {0, 1, 100, 101, 130} <= found["dt_counts"]
    assert found["empty_images"] > 0 and found["idle_categories"] > 0
    gt, _ = CC.edges()
    areas = {a["area"] for a in gt["annotations"]}
    assert 32 ** 2 in areas and 96 ** 2 in areas
    out = CR.evaluate(gt, CC.edges()[1], "segm")
    assert (out["recall"][:, out["cat_ids"].index(5), 1, :] == -1).all() and (out["recall"][:, out["cat_ids"].index(5), 0, :] > -1).all()


# ---- the host side of pegasus_amd.coco_eval ------------------------------------------------------------------------------------
@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
@pytest.mark.parametrize("name", list(CC.evaluation_sets()))
def test_prepare_lays_the_groups_out_as_the_rule_orders_them(name, iou_type):
    from pegasus_amd import coco_eval as CE
    gt, dt = CC.evaluation_sets()[name]
    prob = CE.prepare(gt, dt, iou_type)
    ref = CR.evaluate(gt, dt, iou_type)
    assert prob.img_ids == ref["img_ids"] and prob.cat_ids == ref["cat_ids"] and len(prob.groups) == len(ref["groups"])
    at = 0
    for G, ((i, c), g) in zip(prob.groups, ref["groups"].items()):
        assert (G["dt_count"], G["gt_count"], G["iou_offset"]) == (len(g["d"]), len(g["g"]), at)
        at += len(g["d"]) * len(g["g"])
        d0, g0 = G["dt_begin"], G["gt_begin"]
        assert prob.dt_score[d0:d0 + len(g["d"])].tolist() == g["scores"] and prob.dt_rank[d0:d0 + len(g["d"])].tolist() == list(range(len(g["d"])))
        shapes = [dt[k]["bbox"] if iou_type == "bbox" else CR.counts_of(dt[k]["segmentation"]) for k in g["d"]]
        assert [np.asarray(v).tolist() for v in prob.dt_shapes[d0:d0 + len(g["d"])]] == shapes
        assert prob.gt_area[g0:g0 + len(g["g"])].tolist() == g["gt_area"] and prob.gt_flag[g0:g0 + len(g["g"])].tolist() == g["flag"]
        assert (prob.dt_cat[d0:d0 + len(g["d"])] == prob.cat_ids.index(c)).all()
    assert prob.iou_total == at
    want = np.zeros((len(ref["cat_ids"]), 4), np.int64)
    for (i, c), g in ref["groups"].items():
        for a in range(4):
            want[ref["cat_ids"].index(c), a] += int((~g["per"][a][3]).sum())
    np.testing.assert_array_equal(CE.npig(prob), want)
    np.testing.assert_array_equal(CE.summarize(ref["precision"], ref["recall"], prob.params), ref["stats"])


def test_evaluate_names_what_it_rejects():
    from pegasus_amd import coco_eval as CE
    gt, dt = CC.random_set(0)
    one = dict(dt[0])
    with pytest.raises(ValueError, match="image_id 999 is not in the ground truth"):
        CE.evaluate(gt, [dict(one, image_id=999)], "segm")
    with pytest.raises(ValueError, match="category_id 77 is not in the ground truth"):
        CE.evaluate(gt, [dict(one, category_id=77)], "bbox")
    size = one["segmentation"]["size"]
    with pytest.raises(ValueError, match="differs from its image's"):
        CE.evaluate(gt, [dict(one, segmentation={"counts": [size[0] * size[1] + size[1]], "size": [size[0] + 1, size[1]]})], "segm")
    with pytest.raises(ValueError, match="not to H\\*W"):
        CE.evaluate(gt, [dict(one, segmentation={"counts": [3, 4], "size": size})], "segm")
    with pytest.raises(ValueError, match="'segm' or 'bbox'"):
        CE.evaluate(gt, dt, "keypoints")


def scene_doc(image_ids, first_ann_id=1, cats=(1,)):
    return {"images": [{"id": i, "width": 33, "height": 17} for i in image_ids], "categories": [{"id": c} for c in cats],
            "annotations": [{"id": first_ann_id + k, "image_id": i, "category_id": cats[0], "bbox": [0, 0, 5, 5], "area": 25, "iscrowd": 0}
                            for k, i in enumerate(image_ids)]}


def test_scene_merge_offsets_follow_the_toolkit():
    """merge_coco_annotations: a later scene's image ids are shifted by max id + 1 of what is merged so far."""
    from pegasus_amd import coco_eval as CE
    res = lambda sid, ims: [{"scene_id": sid, "image_id": i, "category_id": 1, "score": 0.5} for i in ims]
    gt, dt, offsets = CE.merge_scenes([(scene_doc([0, 3, 7]), res(1, [3])), (scene_doc([0, 2], cats=(1, 2)), res(2, [0, 2])),
                                       (scene_doc([5]), res(3, [5]))])
    assert offsets == [0, 8, 11]
    assert [i["id"] for i in gt["images"]] == [0, 3, 7, 8, 10, 16] and [a["image_id"] for a in gt["annotations"]] == [0, 3, 7, 8, 10, 16]
    assert [a["id"] for a in gt["annotations"]] == [1, 2, 3, 5, 6, 8] and [r["image_id"] for r in dt] == [3, 8, 10, 16]
    assert gt["categories"] == [{"id": 1}, {"id": 2}]


def write_dataset(root, scenes, name="scene_gt_coco.json"):
    for sid, doc in scenes.items():
        d = root / "train" / f"{sid:06d}"
        d.mkdir(parents=True, exist_ok=True)
        (d / name).write_text(json.dumps(doc))


def test_targets_filter_and_the_modal_file(tmp_path):
    from pegasus_amd import coco_eval as CE
    write_dataset(tmp_path, {1: scene_doc([0, 1, 2]), 2: scene_doc([0, 1])})
    write_dataset(tmp_path, {1: scene_doc([0, 1, 2], cats=(9,)), 2: scene_doc([0, 1], cats=(9,))}, "scene_gt_coco_modal.json")
    results = [{"scene_id": s, "image_id": i, "category_id": 1, "score": 0.5, "bbox": [0, 0, 5, 5], "segmentation": {}, "time": 0.1}
               for s, i in ((1, 0), (1, 1), (1, 2), (2, 0), (2, 1))]
    gt, dt = CE.load_dataset(results, tmp_path, "bbox")
    assert [i["id"] for i in gt["images"]] == [0, 1, 2, 3, 4] and [r["image_id"] for r in dt] == [0, 1, 2, 3, 4]
    targets = [{"scene_id": 2, "im_id": 1, "obj_id": 1, "inst_count": 1}, {"scene_id": 1, "im_id": 2, "obj_id": 1, "inst_count": 1},
               {"scene_id": 1, "im_id": 0, "obj_id": 1, "inst_count": 1}]
    gt, dt = CE.load_dataset(results, tmp_path, "bbox", targets=targets)             # scenes in the order the targets name them
    assert [i["id"] for i in gt["images"]] == [1, 2, 4] and [r["image_id"] for r in dt] == [1, 2, 4]
    assert CE.load_dataset(results, tmp_path, "segm")[1] == []                      # empty segmentations are filtered out
    assert CE.load_dataset(results, tmp_path, "bbox", "modal")[0]["categories"] == [{"id": 9}]
    assert CE.load_dataset(results, tmp_path, "segm", "modal")[0]["categories"] == [{"id": 1}]   # modal is a matter of boxes
    assert CE.scores_file_name("bbox", "modal") == "scores_bop22_coco_bbox_modal.json"
    assert CE.scores_file_name("bbox") == "scores_bop22_coco_bbox.json" and CE.scores_file_name("segm", "modal") == "scores_bop22_coco_segm.json"


def test_the_time_rule():
    from pegasus_amd import coco_eval as CE
    r = lambda s, i, t: {"scene_id": s, "image_id": i, "time": t}
    assert CE.average_time_per_image([r(1, 0, 0.2), r(1, 0, 0.2005), r(1, 1, 0.4), r(2, 0, 0.6)]) == pytest.approx(0.4)
    assert CE.average_time_per_image([r(1, 0, 0.2), r(1, 1, -1), r(1, 0, 5.0)]) == -1.0
    with pytest.raises(ValueError, match="scene 1 and image 0 is not the same"):
        CE.average_time_per_image([r(1, 0, 0.2), r(1, 0, 0.202)])


def test_write_results_is_the_bop22_layout(tmp_path):
    from pegasus_amd import coco_eval as CE
    CE.write_results(tmp_path / "r.json", [{"scene_id": 1, "im_id": 2, "obj_id": 3, "score": 1, "bbox": (1, 2, 3, 4)},
                                           {"scene_id": 1, "im_id": 2, "obj_id": 3, "score": 0.5, "segmentation": {"counts": [4], "size": [2, 2]},
                                            "run_time": 0.25}])
    assert json.loads((tmp_path / "r.json").read_text()) == [
        {"scene_id": 1, "image_id": 2, "category_id": 3, "score": 1.0, "bbox": [1, 2, 3, 4], "segmentation": {}, "time": -1},
        {"scene_id": 1, "image_id": 2, "category_id": 3, "score": 0.5, "bbox": [], "segmentation": {"counts": [4], "size": [2, 2]}, "time": 0.25}]


# ---- the entry points check their arguments on the host -------------------------------------------------------------------
def test_entry_points_validate_before_any_launch():
    from pegasus_amd import _lib
    L = _lib.lib()
    bad, small, fake = _lib.PGR_ERR_INVALID_ARGUMENT, _lib.PGR_ERR_WORKSPACE_TOO_SMALL, C.c_void_p(0x1000)
    Group = _lib.PgrCocoGroup

    def table(*rows):
        return (Group * len(rows))(*[Group(*r) for r in rows]), len(rows)
    good, n = table((0, 2, 0, 3, 0), (2, 1, 3, 0, 6), (3, 2, 3, 1, 6))
    bad_tables = [table((0, -1, 0, 3, 0)), table((0, 2, 0, 5, 0)), table((4, 2, 0, 3, 0)), table((0, 2, 0, 3, 3)),
                  table((0, 2, 0, 3, 0), (1, 1, 3, 1, 6)), table((0, 2, 0, 3, 0), (2, 1, 2, 1, 6)), table((0, 2, 0, 3, 0), (2, 1, 3, 1, 5)),
                  table((0, 2, 0, 3, -1))]

    def rle(groups=good, n_groups=n, w=33, h=17, ws=fake, iou_total=8, n_dt=5, n_gt=4, ws_bytes=16, inter=fake):
        return L.pgr_rle_iou(fake, fake, n_dt, 40, fake, fake, n_gt, 40, fake, w, h, groups, n_groups, iou_total, inter, fake, fake, fake,
                             ws, ws_bytes, None)
    assert rle() == small                                                   # control: every argument check passed
    for g, k in bad_tables:
        assert rle(g, k) == bad
    assert rle(w=0) == bad and rle(h=8193) == bad and rle(ws=None) == bad and rle(ws=C.c_void_p(0x1004)) == bad
    assert rle(iou_total=7) == bad and rle(n_dt=4) == bad and rle(n_gt=3) == bad and rle(inter=None) == bad and rle(None, 3) == bad

    def box(groups=good, n_groups=n, iou=fake, ws=fake, ws_bytes=16, iou_total=8):
        return L.pgr_box_iou(fake, 5, fake, 4, fake, groups, n_groups, iou_total, iou, ws, ws_bytes, None)
    assert box() == small
    assert box(iou=None) == bad and box(ws=None) == bad and box(iou_total=7) == bad and all(box(g, k) == bad for g, k in bad_tables)
    assert box(None, 0, ws_bytes=1 << 20) == 0                              # nothing to do

    thr, rng = (C.c_double * 10)(*np.linspace(.5, .95, 10)), (C.c_double * 8)(0, 1e10, 0, 1024, 1024, 9216, 9216, 1e10)

    def match(groups=good, n_groups=n, n_thr=10, n_area=4, thr=thr, rng=rng, dt_match=fake, ws=fake, ws_bytes=16):
        return L.pgr_coco_match(groups, n_groups, 8, fake, fake, 5, fake, fake, fake, 4, thr, n_thr, rng, n_area, dt_match, fake, fake,
                                fake, ws, ws_bytes, None)
    assert match() == small
    assert match(n_thr=0) == bad and match(n_area=0) == bad and match(thr=None) == bad and match(rng=None) == bad
    assert match(n_thr=17, thr=(C.c_double * 17)(*([0.5] * 17))) == bad      # 68 lanes
    assert match(rng=(C.c_double * 8)(0, 1e10, 5, 1, 0, 1, 0, 1)) == bad    # lo > hi
    assert match(dt_match=None) == bad and match(ws=None) == bad and all(match(g, k) == bad for g, k in bad_tables)

    dets = (C.c_int32 * 3)(1, 10, 100)

    def acc(n_cat=2, n_dt=5, dets=dets, n_dets=3, n_rec=101, n_thr=10, n_area=4, perm=fake, out=fake, ws=fake, ws_bytes=16):
        return L.pgr_coco_accumulate(perm, fake, n_cat, fake, fake, fake, fake, n_dt, fake, dets, n_dets, fake, n_rec, n_thr, n_area, out,
                                     fake, fake, ws, ws_bytes, None)
    assert acc() == small
    assert acc(n_cat=-1) == bad and acc(n_dt=-1) == bad and acc(dets=None) == bad and acc(n_dets=0) == bad and acc(n_dets=9) == bad
    assert acc(n_rec=0) == bad and acc(n_thr=0) == bad and acc(n_thr=17) == bad and acc(perm=None) == bad and acc(out=None) == bad
    assert acc(ws=None) == bad and acc(dets=(C.c_int32 * 3)(1, -10, 100)) == bad
    assert acc(n_cat=0, ws_bytes=1 << 20) == 0


def test_workspace_sizes_are_host_only_and_zero_for_invalid_arguments():
    from pegasus_amd import _lib
    L = _lib.lib()
    assert L.pgr_rle_iou_workspace_bytes(10, 1000, 2000) >= 10 * 24 + 4 * (2 * 1000 + 2 * 2000)
    assert L.pgr_rle_iou_workspace_bytes(0, 0, 0) > 0
    assert L.pgr_rle_iou_workspace_bytes(-1, 0, 0) == 0 and L.pgr_rle_iou_workspace_bytes(1, -1, 0) == 0 and L.pgr_rle_iou_workspace_bytes(1, 0, -1) == 0
    assert L.pgr_box_iou_workspace_bytes(10) >= 240 and L.pgr_box_iou_workspace_bytes(0) > 0 and L.pgr_box_iou_workspace_bytes(-1) == 0
    assert L.pgr_coco_match_workspace_bytes(10, 100, 4) >= 240 + 1600
    assert L.pgr_coco_match_workspace_bytes(-1, 100, 4) == 0 and L.pgr_coco_match_workspace_bytes(1, -1, 4) == 0
    assert L.pgr_coco_match_workspace_bytes(1, 1, 0) == 0 and L.pgr_coco_match_workspace_bytes(1, 1, 65) == 0
    assert L.pgr_coco_accumulate_workspace_bytes(1000, 4, 3) >= 16 * 12 * 1000 and L.pgr_coco_accumulate_workspace_bytes(0, 4, 3) > 0
    assert L.pgr_coco_accumulate_workspace_bytes(-1, 4, 3) == 0 and L.pgr_coco_accumulate_workspace_bytes(10, 0, 3) == 0
    assert L.pgr_coco_accumulate_workspace_bytes(10, 4, 0) == 0 and L.pgr_coco_accumulate_workspace_bytes(10, 4, 9) == 0
    assert (_lib.PGR_COCO_CHUNK, _lib.PGR_COCO_LDS_RUNS) == (CC.CHUNK, CC.LDS_RUNS)
    header = (__import__("pathlib").Path(__file__).resolve().parents[1] / "include" / "pegasus_raster.h").read_text()
    for name in ("PGR_COCO_CHUNK", "PGR_COCO_LDS_RUNS", "PGR_COCO_MAX_LANES", "PGR_COCO_MAX_MAXDETS"):
        assert f"#define {name} {getattr(_lib, name)} " in header
