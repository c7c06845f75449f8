"""pgr_rle_iou, pgr_box_iou, pgr_coco_match and pgr_coco_accumulate on the GPU, through the C ABI with guard regions around
every buffer the kernels write and around the workspace, against the NumPy restatement (tests/coco_eval_reference.py); then
pegasus_amd.coco_eval end to end.  Everything is an integer or a float64 from a fixed sequence of IEEE operations: every
comparison is for equality, floats bit for bit."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import coco_eval_cases as CC
import coco_eval_reference as CR

pytestmark = pytest.mark.gpu
GUARD = 4096                                   # elements in front of and behind every buffer; a multiple of 16 bytes


def guarded(n, dtype, fill):
    import torch
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")


def intact(buf, n, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


def inner(buf, n):
    return buf[GUARD:GUARD + n]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def group_table(rows):
    from pegasus_amd import _lib
    return (_lib.PgrCocoGroup * max(len(rows), 1))(*[_lib.PgrCocoGroup(*[int(v) for v in r]) for r in rows])


def with_offsets(rows, gap=0):
    """(dt_begin, dt_count, gt_begin, gt_count) rows -> five-column rows, ``gap`` unused cells in front of every matrix."""
    out, at = [], 0
    for r in rows:
        at += gap
        out.append((*r, at))
        at += r[1] * r[3]
    return out, at + gap


def flat(lists):
    offsets = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(c) for c in lists], out=offsets[1:])
    return np.concatenate([np.asarray(c, np.int32) for c in lists]), offsets


# ---- pgr_rle_iou --------------------------------------------------------------------------------------------------------
def run_rle_iou(case, gap=3):
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    H, W = case["size"]
    rows, total = with_offsets(case["groups"], gap)
    dc, do = flat(case["dt"])
    gc, go = flat(case["gt"])
    n_dt, n_gt = len(case["dt"]), len(case["gt"])
    nbytes = int(L.pgr_rle_iou_workspace_bytes(len(rows), len(dc), len(gc)))
    assert nbytes > 0
    ws, inter, iou = guarded(nbytes, torch.uint8, 0xA5), guarded(total, torch.int64, -7), guarded(total, torch.float64, float("nan"))
    dt_area, gt_area = guarded(n_dt, torch.int64, -7), guarded(n_gt, torch.int64, -7)
    keep = [dev(dc), dev(do), dev(gc), dev(go), dev(np.asarray(case["crowd"], np.uint8))]
    table = group_table(rows)
    _lib.check(L.pgr_rle_iou(_lib.ptr(keep[0]), _lib.ptr(keep[1]), n_dt, len(dc), _lib.ptr(keep[2]), _lib.ptr(keep[3]), n_gt, len(gc),
                             _lib.ptr(keep[4]), W, H, table, len(rows), total, _lib.ptr(inter[GUARD:]), _lib.ptr(iou[GUARD:]),
                             _lib.ptr(dt_area[GUARD:]), _lib.ptr(gt_area[GUARD:]), _lib.ptr(ws[GUARD:]), nbytes,
                             _lib.stream_ptr(ws.device)), "pgr_rle_iou")
    torch.cuda.synchronize()
    assert intact(ws, nbytes, 0xA5) and intact(inter, total, -7) and intact(dt_area, n_dt, -7) and intact(gt_area, n_gt, -7)
    assert bool(torch.isnan(iou[:GUARD]).all()) and bool(torch.isnan(iou[GUARD + total:]).all())
    return rows, tuple(inner(b, n).cpu().numpy() for b, n in ((inter, total), (iou, total), (dt_area, n_dt), (gt_area, n_gt)))


@pytest.mark.parametrize("name", list(CC.iou_cases()))
def test_rle_iou_equals_the_pixel_counts(name):
    case = CC.iou_cases()[name]
    n_pix = case["size"][0] * case["size"][1]
    rows, (inter, iou, dt_area, gt_area) = run_rle_iou(case)
    _, again = run_rle_iou(case)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((inter, iou, dt_area, gt_area), again)), "two runs differ"
    d_pix, g_pix = [CR.pixels(c, n_pix) for c in case["dt"]], [CR.pixels(c, n_pix) for c in case["gt"]]
    assert dt_area.tolist() == [int(p.sum()) for p in d_pix] and gt_area.tolist() == [int(p.sum()) for p in g_pix]
    want_inter, want_iou = np.full(len(inter), -7, np.int64), np.full(len(iou), np.nan)
    for d0, nd, g0, ng, at in rows:
        for d in range(nd):
            for g in range(ng):
                want_inter[at + d * ng + g], want_iou[at + d * ng + g] = CR.mask_iou(d_pix[d0 + d], g_pix[g0 + g], case["crowd"][g0 + g])
    np.testing.assert_array_equal(inter, want_inter)                         # cells of no group keep their fill
    np.testing.assert_array_equal(bits(iou), bits(want_iou))


# ---- pgr_box_iou --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.box_cases()))
def test_box_iou_is_the_rules_sequence_of_operations(name):
    """Bit for bit: a product contracted into the subtraction that follows it (an FMA) changes the last bit of the union."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    case = CC.box_cases()[name]
    rows, total = with_offsets(case["groups"], 3)
    nbytes = int(L.pgr_box_iou_workspace_bytes(len(rows)))
    ws, iou = guarded(nbytes, torch.uint8, 0xA5), guarded(total, torch.float64, float("nan"))
    d, g, crowd, table = dev(case["dt"]), dev(case["gt"]), dev(case["crowd"]), group_table(rows)
    outs = []
    for _ in range(2):
        _lib.check(L.pgr_box_iou(_lib.ptr(d), len(d), _lib.ptr(g), len(g), _lib.ptr(crowd), table, len(rows), total,
                                 _lib.ptr(iou[GUARD:]), _lib.ptr(ws[GUARD:]), nbytes, _lib.stream_ptr(ws.device)), "pgr_box_iou")
        torch.cuda.synchronize()
        assert intact(ws, nbytes, 0xA5) and bool(torch.isnan(iou[:GUARD]).all()) and bool(torch.isnan(iou[GUARD + total:]).all())
        outs.append(inner(iou, total).cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    want = np.full(total, np.nan)
    for d0, nd, g0, ng, at in rows:
        for a in range(nd):
            for b in range(ng):
                want[at + a * ng + b] = CR.box_iou(case["dt"][d0 + a], case["gt"][g0 + b], case["crowd"][g0 + b])
    np.testing.assert_array_equal(bits(outs[0]), bits(want))
    assert (want == 1.0).any() and (want == 0.0).sum() > 3            # the cases hold an exact match and disjoint pairs


# ---- the reference's groups as flat arrays ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flattened(name, iou_type, pad=2, use_ignore_field=False):
    """The reference's evaluation of a set, and its groups laid out flat with ``pad`` sentinel rows in front of every
    group's detections and GT and ``pad`` unused cells in front of every IoU matrix."""
    gt, dt = CC.evaluation_sets()[name]
    ref = CR.evaluate(gt, dt, iou_type, CR.default_params(use_ignore_field=use_ignore_field))
    A, T = 4, 10
    rows, n_dt, n_gt, cells = [], 0, 0, 0
    for g in ref["groups"].values():
        n_dt, n_gt, cells = n_dt + pad, n_gt + pad, cells + pad
        rows.append((n_dt, len(g["d"]), n_gt, len(g["g"]), cells))
        n_dt, n_gt, cells = n_dt + len(g["d"]), n_gt + len(g["g"]), cells + len(g["d"]) * len(g["g"])
    n_dt, n_gt, cells = n_dt + pad, n_gt + pad, cells + pad
    F = dict(rows=rows, n_dt=n_dt, n_gt=n_gt, cells=cells, iou=np.full(cells, np.nan), dt_area=np.full(n_dt, np.nan),
             gt_area=np.full(n_gt, np.nan), gt_flag=np.full(n_gt, 1, np.uint8), gt_crowd=np.full(n_gt, 1, np.uint8),
             dt_score=np.zeros(n_dt), dt_cat=np.full(n_dt, -1, np.int64), dt_rank=np.zeros(n_dt, np.int32),
             dt_match=np.full((A, T, n_dt), -9, np.int32), dt_ignore=np.full((A, T, n_dt), 9, np.uint8),
             gt_match=np.full((A, T, n_gt), -9, np.int32), gt_ignore=np.full((A, n_gt), 9, np.uint8),
             npig=np.zeros((len(ref["cat_ids"]), A), np.int32))
    for (d0, nd, g0, ng, at), ((i, c), g) in zip(rows, ref["groups"].items()):
        k = ref["cat_ids"].index(c)
        F["iou"][at:at + nd * ng] = g["ious"].reshape(-1)
        F["dt_area"][d0:d0 + nd], F["gt_area"][g0:g0 + ng] = g["dt_area"], g["gt_area"]
        F["gt_flag"][g0:g0 + ng], F["gt_crowd"][g0:g0 + ng] = g["flag"], g["crowd"]
        F["dt_score"][d0:d0 + nd], F["dt_cat"][d0:d0 + nd], F["dt_rank"][d0:d0 + nd] = g["scores"], k, np.arange(nd)
        for a, (dtm, dt_ig, gtm, gt_ig) in enumerate(g["per"]):
            F["dt_match"][a, :, d0:d0 + nd] = np.where(dtm > -1, dtm + g0, -1)
            F["dt_ignore"][a, :, d0:d0 + nd] = dt_ig
            F["gt_match"][a, :, g0:g0 + ng] = np.where(gtm > -1, gtm + d0, -1)
            F["gt_ignore"][a, g0:g0 + ng] = gt_ig
            F["npig"][k, a] += int((~gt_ig).sum())
    return ref, F


def run_match(F, rows):
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    p = CR.default_params()
    A, T, n_dt, n_gt = 4, 10, F["n_dt"], F["n_gt"]
    thr = (C.c_double * T)(*p["iou_thrs"])
    rng = (C.c_double * (2 * A))(*np.asarray(p["area_rng"], np.float64).reshape(-1))
    nbytes = int(L.pgr_coco_match_workspace_bytes(len(rows), n_gt, A))
    assert nbytes > 0
    ws = guarded(nbytes, torch.uint8, 0xA5)
    dt_match, dt_ignore = guarded(A * T * n_dt, torch.int32, -9), guarded(A * T * n_dt, torch.uint8, 9)
    gt_match, gt_ignore = guarded(A * T * n_gt, torch.int32, -9), guarded(A * n_gt, torch.uint8, 9)
    keep = [dev(F[k]) for k in ("iou", "dt_area", "gt_area", "gt_flag", "gt_crowd")]
    table = group_table(rows)
    _lib.check(L.pgr_coco_match(table, len(rows), F["cells"], _lib.ptr(keep[0]), _lib.ptr(keep[1]), n_dt, _lib.ptr(keep[2]),
                                _lib.ptr(keep[3]), _lib.ptr(keep[4]), n_gt, thr, T, rng, A, _lib.ptr(dt_match[GUARD:]),
                                _lib.ptr(dt_ignore[GUARD:]), _lib.ptr(gt_match[GUARD:]), _lib.ptr(gt_ignore[GUARD:]), _lib.ptr(ws[GUARD:]),
                                nbytes, _lib.stream_ptr(ws.device)), "pgr_coco_match")
    torch.cuda.synchronize()
    assert intact(ws, nbytes, 0xA5) and intact(dt_match, A * T * n_dt, -9) and intact(dt_ignore, A * T * n_dt, 9)
    assert intact(gt_match, A * T * n_gt, -9) and intact(gt_ignore, A * n_gt, 9)
    return (inner(dt_match, A * T * n_dt).cpu().numpy().reshape(A, T, n_dt), inner(dt_ignore, A * T * n_dt).cpu().numpy().reshape(A, T, n_dt),
            inner(gt_match, A * T * n_gt).cpu().numpy().reshape(A, T, n_gt), inner(gt_ignore, A * n_gt).cpu().numpy().reshape(A, n_gt))


SETS = [(name, iou_type) for name in CC.evaluation_sets() for iou_type in ("segm", "bbox")]


@pytest.mark.parametrize("name,iou_type", SETS)
def test_match_equals_the_reference(name, iou_type):
    """All four outputs for every group, area range and threshold; the sentinel rows in front of and behind every group's
    slices (detections and GT that belong to no group) keep their bytes; two runs give equal bytes."""
    for use_ignore in (False, True):
        _, F = flattened(name, iou_type, 2, use_ignore)
        got = run_match(F, F["rows"])
        for out, key in zip(got, ("dt_match", "dt_ignore", "gt_match", "gt_ignore")):
            np.testing.assert_array_equal(out, F[key], err_msg=f"{key} use_ignore_field={use_ignore}")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, run_match(F, F["rows"])))


def test_a_group_alone_equals_the_group_inside_a_table():
    _, F = flattened("edges", "segm")
    sizes = [r[1] * r[3] for r in F["rows"]]
    for k in sorted({int(np.argmax(sizes)), 0, len(sizes) - 1, int(np.argmin(sizes))}):
        d0, nd, g0, ng, at = F["rows"][k]
        got = run_match(F, [F["rows"][k]])
        for out, key, lo, n in zip(got, ("dt_match", "dt_ignore", "gt_match", "gt_ignore"), (d0, d0, g0, g0), (nd, nd, ng, ng)):
            want = np.full_like(F[key], -9 if out.dtype == np.int32 else 9)
            want[..., lo:lo + n] = F[key][..., lo:lo + n]
            np.testing.assert_array_equal(out, want, err_msg=f"group {k} {key}")


# ---- pgr_coco_accumulate --------------------------------------------------------------------------------------------------
def run_accumulate(perm, seg, rank, dt_match, dt_ignore, scores, npig, n_dt, max_dets=(1, 10, 100), rec_thrs=None):
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    rec_thrs = CR.default_params()["rec_thrs"] if rec_thrs is None else rec_thrs
    A, T = dt_match.shape[:2]
    K, M, R = len(seg) - 1, len(max_dets), len(rec_thrs)
    nbytes = int(L.pgr_coco_accumulate_workspace_bytes(n_dt, A, M))
    assert nbytes > 0
    ws = guarded(nbytes, torch.uint8, 0xA5)
    n_pr, n_rc = T * R * K * A * M, T * K * A * M
    precision, sc, recall = (guarded(n, torch.float64, float("nan")) for n in (n_pr, n_pr, n_rc))
    keep = [dev(np.asarray(perm, np.int64)), dev(np.asarray(seg, np.int64)), dev(np.asarray(rank, np.int32)), dev(np.asarray(dt_match, np.int32)),
            dev(np.asarray(dt_ignore, np.uint8)), dev(np.asarray(scores, np.float64)), dev(np.asarray(npig, np.int32)),
            dev(np.asarray(rec_thrs, np.float64))]
    outs = []
    for _ in range(2):
        _lib.check(L.pgr_coco_accumulate(_lib.ptr(keep[0]), _lib.ptr(keep[1]), K, _lib.ptr(keep[2]), _lib.ptr(keep[3]), _lib.ptr(keep[4]),
                                         _lib.ptr(keep[5]), n_dt, _lib.ptr(keep[6]), (C.c_int32 * M)(*max_dets), M, _lib.ptr(keep[7]), R, T, A,
                                         _lib.ptr(precision[GUARD:]), _lib.ptr(sc[GUARD:]), _lib.ptr(recall[GUARD:]), _lib.ptr(ws[GUARD:]),
                                         nbytes, _lib.stream_ptr(ws.device)), "pgr_coco_accumulate")
        torch.cuda.synchronize()
        assert intact(ws, nbytes, 0xA5)
        for buf, n in ((precision, n_pr), (sc, n_pr), (recall, n_rc)):
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())
        outs.append((inner(precision, n_pr).cpu().numpy().reshape(T, R, K, A, M), inner(sc, n_pr).cpu().numpy().reshape(T, R, K, A, M),
                     inner(recall, n_rc).cpu().numpy().reshape(T, K, A, M)))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs)), "two runs differ"
    return outs[0]


def accumulate_flat(perm, seg, rank, dt_match, dt_ignore, scores, npig, max_dets=(1, 10, 100), rec_thrs=None):
    """The rule's accumulation over flat arrays, in NumPy."""
    rec_thrs = CR.default_params()["rec_thrs"] if rec_thrs is None else rec_thrs
    A, T = dt_match.shape[:2]
    K, M, R = len(seg) - 1, len(max_dets), len(rec_thrs)
    precision, sc, recall = -np.ones((T, R, K, A, M)), -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                if npig[k, a] == 0:
                    continue
                sel = perm[seg[k]:seg[k + 1]]
                sel = sel[rank[sel] < max_det]
                for t in range(T):
                    ig = dt_ignore[a, t, sel] != 0
                    tp = np.cumsum((dt_match[a, t, sel] > -1) & ~ig).astype(np.float64)
                    fp = np.cumsum((dt_match[a, t, sel] == -1) & ~ig).astype(np.float64)
                    rc, pr = tp / npig[k, a], tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if len(sel) else 0
                    for i in range(len(sel) - 1, 0, -1):
                        pr[i - 1] = max(pr[i - 1], pr[i])
                    at = np.searchsorted(rc, rec_thrs, side="left")
                    precision[t, :, k, a, m] = [pr[i] if i < len(sel) else 0.0 for i in at]
                    sc[t, :, k, a, m] = [scores[sel[i]] if i < len(sel) else 0.0 for i in at]
    return precision, sc, recall


def order_of(F):
    """perm and segment starts of a flattened set, formed here in NumPy (np.lexsort is stable)."""
    rows = np.flatnonzero(F["dt_cat"] >= 0)
    perm = rows[np.lexsort((-F["dt_score"][rows], F["dt_cat"][rows]))]
    seg = np.zeros(F["npig"].shape[0] + 1, np.int64)
    np.cumsum(np.bincount(F["dt_cat"][rows], minlength=len(seg) - 1), out=seg[1:])
    return perm, seg


@pytest.mark.parametrize("name,iou_type", SETS)
def test_accumulate_equals_the_reference(name, iou_type):
    """precision, recall and scores bit for bit, from the reference's own matching: every element is copied or is one IEEE
    division of exact operands.  The sentinel rows are in no segment and are never read into a result."""
    ref, F = flattened(name, iou_type)
    perm, seg = order_of(F)
    got = run_accumulate(perm, seg, F["dt_rank"], F["dt_match"], F["dt_ignore"], F["dt_score"], F["npig"], F["n_dt"])
    for out, key in zip(got, ("precision", "scores", "recall")):
        np.testing.assert_array_equal(bits(out), bits(ref[key]), err_msg=key)
    for out, want in zip(accumulate_flat(perm, seg, F["dt_rank"], F["dt_match"], F["dt_ignore"], F["dt_score"], F["npig"]),
                         (ref["precision"], ref["scores"], ref["recall"])):
        np.testing.assert_array_equal(bits(out), bits(want))                # the flat restatement used below is the rule too


def test_accumulate_at_the_segment_edges():
    """Categories with 0, 1, chunk - 1, chunk, chunk + 1 and several chunks of detections, ranks on both sides of every
    maxDet, tied scores, a category without counted GT, entries of perm outside the detections (skipped) and recall
    thresholds that are not the default."""
    rng = np.random.default_rng(3)
    sizes = [0, 1, CC.CHUNK - 1, CC.CHUNK, CC.CHUNK + 1, 3 * CC.CHUNK + 17, 5, 0]
    A, T, K, n = 4, 10, len(sizes), sum(sizes)
    cat = np.repeat(np.arange(K), sizes)
    scores = rng.integers(1, 21, n) / 20.0
    rank = rng.choice([0, 0, 1, 5, 9, 10, 11, 50, 99, 100, 101, 120], n).astype(np.int32)
    dt_match = np.where(rng.random((A, T, n)) < 0.5, rng.integers(0, 1000, (A, T, n)), -1).astype(np.int32)
    dt_ignore = (rng.random((A, T, n)) < 0.2).astype(np.uint8)
    shuffle = rng.permutation(n)
    cat, scores, rank, dt_match, dt_ignore = cat[shuffle], scores[shuffle], rank[shuffle], dt_match[:, :, shuffle], dt_ignore[:, :, shuffle]
    perm = np.lexsort((-scores, cat))
    seg = np.zeros(K + 1, np.int64)
    np.cumsum(sizes, out=seg[1:])
    npig = rng.integers(1, 60, (K, A)).astype(np.int32)
    npig[6, 1], npig[2, 3], npig[7, :] = 0, 0, 0
    rec = np.r_[np.linspace(0, 1, 37), 0.5, 1.5, -0.25]
    for max_dets, rec_thrs in (((1, 10, 100), None), ((0, 7, 100, 1000), rec)):
        want = accumulate_flat(perm, seg, rank, dt_match, dt_ignore, scores, npig, max_dets, rec_thrs)
        got = run_accumulate(perm, seg, rank, dt_match, dt_ignore, scores, npig, n, max_dets, rec_thrs)
        for out, w, key in zip(got, want, ("precision", "scores", "recall")):
            np.testing.assert_array_equal(bits(out), bits(w), err_msg=f"{key} {max_dets}")
    bad = perm.copy()
    bad[::7] = np.where(np.arange(len(bad[::7])) % 2 == 0, -1, n + 5)
    keep = np.ones(n, bool)
    keep[perm[::7]] = False
    want = accumulate_flat(perm, seg, np.where(keep, rank, 10 ** 6).astype(np.int32), dt_match, dt_ignore, scores, npig)
    got = run_accumulate(bad, seg, rank, dt_match, dt_ignore, scores, npig, n)
    for out, w in zip(got, want):
        np.testing.assert_array_equal(bits(out), bits(w))


# ---- pegasus_amd.coco_eval end to end --------------------------------------------------------------------------------------
@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
@pytest.mark.parametrize("name", list(CC.evaluation_sets()))
def test_evaluate_equals_the_reference(name, iou_type):
    from pegasus_amd import coco_eval as CE
    gt, dt = CC.evaluation_sets()[name]
    for use_ignore in (False, True):
        ref = CR.evaluate(gt, dt, iou_type, CR.default_params(use_ignore_field=use_ignore))
        got = CE.evaluate(gt, dt, iou_type, CE.Params(use_ignore_field=use_ignore))
        for key in ("precision", "recall", "scores", "stats"):
            np.testing.assert_array_equal(bits(getattr(got, key)), bits(ref[key]), err_msg=f"{key} use_ignore_field={use_ignore}")
        assert list(got.as_dict()) == list(CR.STAT_NAMES) and list(got.as_dict().values()) == ref["stats"].tolist()
        again = CE.evaluate(gt, dt, iou_type, CE.Params(use_ignore_field=use_ignore))
        assert all(getattr(got, k).tobytes() == getattr(again, k).tobytes() for k in ("precision", "recall", "scores", "stats"))


def test_string_counts_score_like_list_counts():
    from pegasus_amd import coco_eval as CE
    for lists, strings in ((CC.edges(), CC.edges(True)), (CC.random_set(1), CC.random_set(1, True))):
        assert all(isinstance(r["segmentation"]["counts"], str) for r in strings[1])
        a, b = CE.evaluate(*lists, "segm"), CE.evaluate(*strings, "segm")
        assert a.precision.tobytes() == b.precision.tobytes() and a.scores.tobytes() == b.scores.tobytes() and a.stats.tobytes() == b.stats.tobytes()
        np.testing.assert_array_equal(bits(b.stats), bits(CR.evaluate(*strings, "segm")["stats"]))


def test_the_hand_worked_cases_on_the_device():
    """The worked three-detection case and the ignore-field pair of tests/test_coco_eval_host.py, through the kernels."""
    import test_coco_eval_host as TH
    from pegasus_amd import coco_eval as CE
    s = CE.evaluate(*TH.three_detections(), "bbox").as_dict()
    assert s["AP"] == pytest.approx((6 * TH.AP_TFT + 4 * TH.AP51) / 10, abs=1e-15) and s["AP50"] == pytest.approx(TH.AP_TFT, abs=1e-15)
    assert s["AR1"] == 0.5 and s["AR100"] == pytest.approx(0.8) and s["AP_small"] == -1.0 and s["AP_large"] == -1.0
    gt, dt = TH.ignore_field_case()
    assert CE.evaluate(gt, dt, "bbox").as_dict()["AP"] == pytest.approx(TH.AP51, abs=1e-15)
    assert CE.evaluate(gt, dt, "bbox", CE.Params(use_ignore_field=True)).as_dict()["AP"] == pytest.approx(TH.ONE_OF_ONE, abs=1e-16)
    assert CE.evaluate(gt, [], "bbox").as_dict()["AP"] == 0.0


def test_public_iou_wrappers():
    from pegasus_amd import coco_eval as CE
    case = CC.iou_cases()["split 17x33"]
    seg = lambda c: {"counts": c, "size": list(case["size"])}
    iou, inter, dt_area, gt_area = CE.rle_ious([seg(c) for c in case["dt"]], [CE.rle_string_encode(c) for c in case["gt"]], case["groups"],
                                               case["crowd"], size=case["size"])
    rows, (want_inter, want_iou, want_d, want_g) = run_rle_iou(case, gap=0)
    assert inter.cpu().numpy().tolist() == want_inter.tolist() and iou.cpu().numpy().tobytes() == want_iou.tobytes()
    assert dt_area.cpu().numpy().tolist() == want_d.tolist() and gt_area.cpu().numpy().tolist() == want_g.tolist()
    box = CC.box_cases()["several groups"]
    got = CE.box_ious(box["dt"], box["gt"], box["groups"], box["crowd"]).cpu().numpy()
    rows, _ = with_offsets(box["groups"])
    want = [CR.box_iou(box["dt"][d0 + a], box["gt"][g0 + b], box["crowd"][g0 + b]) for d0, nd, g0, ng, at in rows for a in range(nd) for b in range(ng)]
    np.testing.assert_array_equal(bits(got), bits(want))
    with pytest.raises(ValueError, match="sum to H\\*W"):
        CE.rle_ious([[5, 5]], [[561]], [(0, 1, 0, 1)], size=case["size"])


def test_a_dataset_directory_scored_by_the_cli(tmp_path, capsys):
    """Two scenes written as mask PNGs, their scene_gt_coco files by pegasus_amd.coco, the ground truth written back as
    detections with score 1 by write_results: AP = 1 for both types (to the one ulp of a lone true positive)."""
    from pegasus_amd import coco as CO, coco_eval as CE, dataset_writer as DW
    rng = np.random.default_rng(9)
    H, W = CC.LARGE
    for sid, n_images in ((1, 2), (2, 3)):
        scene = tmp_path / "ds" / "train" / f"{sid:06d}"
        (scene / "mask").mkdir(parents=True)
        (scene / "mask_visib").mkdir()
        gt, info = {}, {}
        for im in range(n_images):
            gt[str(im)], info[str(im)] = [], []
            for k, obj in enumerate((3, 3, 5)):
                full = CC.ellipse((H, W), rng.uniform(10, H - 10), 8 + 16 * k, rng.uniform(5, 12), rng.uniform(4, 7))
                visib = full & CC.rect((H, W), 0, 0, int(rng.integers(H // 2, H + 1)), W)
                (scene / "mask" / f"{im:06d}_{k:06d}.png").write_bytes(DW.encode_png(full.astype(np.uint8) * 255))
                (scene / "mask_visib" / f"{im:06d}_{k:06d}.png").write_bytes(DW.encode_png(visib.astype(np.uint8) * 255))
                gt[str(im)].append({"obj_id": obj, "cam_R_m2c": [1, 0, 0, 0, 1, 0, 0, 0, 1], "cam_t_m2c": [0, 0, 1]})
                info[str(im)].append({"visib_fract": float(visib.sum() / max(full.sum(), 1))})
        (scene / "scene_gt.json").write_text(json.dumps(gt))
        (scene / "scene_gt_info.json").write_text(json.dumps(info))
    for bbox_type in ("amodal", "modal"):
        CO.recompute_dataset(tmp_path / "ds", bbox_type)
    for bbox_type in ("amodal", "modal"):                                   # (a detection's box is the box of that file)
        results = CE.results_from_gt(tmp_path / "ds", bbox_type=bbox_type)
        assert len(results) == 15 and {r["scene_id"] for r in results} == {1, 2}
        CE.write_results(tmp_path / f"results_{bbox_type}.json", results)
    targets = [{"scene_id": 2, "im_id": 1}, {"scene_id": 1, "im_id": 0}, {"scene_id": 2, "im_id": 2}]
    (tmp_path / "targets.json").write_text(json.dumps(targets))
    for args, name in ((["--ann_type", "segm"], "scores_bop22_coco_segm.json"), (["--ann_type", "bbox"], "scores_bop22_coco_bbox.json"),
                       (["--ann_type", "bbox", "--bbox_type", "modal", "--use_ignore_field", "--targets", str(tmp_path / "targets.json")],
                        "scores_bop22_coco_bbox_modal.json")):
        capsys.readouterr()
        results_path = tmp_path / ("results_modal.json" if "modal" in args else "results_amodal.json")
        assert CE.main(["--results", str(results_path), "--dataset", str(tmp_path / "ds"), "--out", str(tmp_path / "eval"), *args]) == 0
        printed = capsys.readouterr().out
        scores = json.loads((tmp_path / "eval" / name).read_text())
        assert list(scores) == [*CR.STAT_NAMES, "average_time_per_image"] and scores["average_time_per_image"] == 0.0
        assert "AP: 1.0000" in printed and "AR100: 1.0000" in printed
        assert abs(scores["AP"] - 1.0) < 1e-15 and abs(scores["AP50"] - 1.0) < 1e-15 and scores["AR100"] == 1.0
    gt_doc, dt = CE.load_dataset(json.loads((tmp_path / "results_amodal.json").read_text()), tmp_path / "ds", "segm")
    ref = CR.evaluate(gt_doc, dt, "segm")
    np.testing.assert_array_equal(bits(CE.evaluate(gt_doc, dt, "segm").stats), bits(ref["stats"]))
