"""COCOeval (pycocotools, as the BOP toolkit's scripts/eval_bop22_coco.py runs it) restated in NumPy / Python float64 from
the written rule of DESIGN.md section 14.  It shares nothing with pegasus_amd.coco_eval: masks are decoded to pixels and
counted, and the loops read the way the rule reads (np.argsort(kind='mergesort'), np.cumsum, np.searchsorted).

pycocotools cannot be run where this project is developed: this file and the hand-worked answers of
tests/test_coco_eval_host.py are what pins the rule, not recorded outputs."""
import numpy as np

STAT_NAMES = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "AR100", "AR_small", "AR_medium",
              "AR_large")


def default_params(**over):
    p = dict(iou_thrs=np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1),
             rec_thrs=np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1), max_dets=[1, 10, 100],
             area_rng=[[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]],
             area_rng_lbl=["all", "small", "medium", "large"], use_ignore_field=False)
    p.update(over)
    return p


# ---- compressed counts ------------------------------------------------------------------------------------------------
def string_decode(s):
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = (c & 0x20) != 0
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[len(counts) - 2]
        counts.append(x)
    return counts


def counts_of(seg):
    c = seg["counts"]
    return string_decode(c) if isinstance(c, str) else [int(v) for v in c]


# ---- pixels -----------------------------------------------------------------------------------------------------------
def pixels(counts, n_pixels):
    """The mask as a flat bool vector in the order the runs are in (the order does not matter for counting)."""
    out = np.zeros(n_pixels, bool)
    at, value = 0, False
    for c in counts:
        c = max(int(c), 0)
        if value:
            out[at:at + c] = True
        at += c
        value = not value
    return out


def mask_iou(d, g, crowd):
    inter = int(np.count_nonzero(d & g))
    if inter == 0:
        return 0, 0.0
    union = int(np.count_nonzero(d)) if crowd else int(np.count_nonzero(d)) + int(np.count_nonzero(g)) - inter
    return inter, float(np.float64(inter) / np.float64(union))


def box_iou(d, g, crowd):
    dx, dy, dw, dh = (np.float64(v) for v in d)
    gx, gy, gw, gh = (np.float64(v) for v in g)
    iw = min(dx + dw, gx + gw) - max(dx, gx)
    ih = min(dy + dh, gy + gh) - max(dy, gy)
    inter = iw * ih if (iw > 0 and ih > 0) else np.float64(0.0)
    if inter == 0:
        return 0.0
    a = dw * dh
    b = gw * gh
    union = a if crowd else (a + b) - inter
    return float(inter / union)


# ---- evaluateImg ------------------------------------------------------------------------------------------------------
def match(ious, gt_area, gt_flag, gt_crowd, dt_area, lo, hi, iou_thrs):
    """One group, one area range.  ``ious`` [D,G] with the GT in FILE order.  Returns (dtm [T,D]: GT index in file order or
    -1, dt_ig [T,D], gtm [T,G]: detection index or -1 (file order), gt_ig [G] (file order))."""
    D, G, T = len(dt_area), len(gt_area), len(iou_thrs)
    ig = np.array([bool(gt_flag[g]) or gt_area[g] < lo or gt_area[g] > hi for g in range(G)], bool)
    order = np.argsort(ig.astype(np.uint8), kind="mergesort") if G else np.zeros(0, np.int64)
    s_ig = ig[order]
    dtm = -np.ones((T, D), np.int64)
    gtm = -np.ones((T, G), np.int64)                   # in sorted order
    dt_ig = np.zeros((T, D), bool)
    for ti, t in enumerate(iou_thrs):
        for d in range(D):
            best = min([t, 1 - 1e-10])
            m = -1
            for gi in range(G):
                if gtm[ti, gi] > -1 and not gt_crowd[order[gi]]:
                    continue
                if m > -1 and not s_ig[m] and s_ig[gi]:
                    break
                if ious[d, order[gi]] < best:
                    continue
                best = ious[d, order[gi]]
                m = gi
            if m == -1:
                continue
            dt_ig[ti, d] = s_ig[m]
            dtm[ti, d] = order[m]
            gtm[ti, m] = d
    outside = np.array([a < lo or a > hi for a in dt_area], bool).reshape(1, D)
    dt_ig = dt_ig | ((dtm == -1) & np.repeat(outside, T, 0))
    gtm_file = -np.ones((T, G), np.int64)
    if G:
        gtm_file[:, order] = gtm
    return dtm, dt_ig, gtm_file, ig


# ---- the whole evaluation -------------------------------------------------------------------------------------------------
def evaluate(gt, dt, iou_type, params=None):
    """Returns a dict: precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M], stats [12], and ``groups``: one entry per
    (image, category) with a GT or a detection, images and categories ascending -- dict(image, cat, d: indices into ``dt``
    in score order cut to maxDets[-1], g: indices into gt['annotations'] in file order, ious [D,G], inter [D,G] (segm),
    dt_area, gt_area (the field), per: [A] results of ``match``)."""
    p = params or default_params()
    iou_thrs, rec_thrs, max_dets = np.asarray(p["iou_thrs"], np.float64), np.asarray(p["rec_thrs"], np.float64), list(p["max_dets"])
    area_rng = [[float(a), float(b)] for a, b in p["area_rng"]]
    img_ids = sorted(int(i["id"]) for i in gt["images"])
    cat_ids = sorted(int(c["id"]) for c in gt["categories"])
    size = {int(i["id"]): (int(i["height"]), int(i["width"])) for i in gt["images"]}
    anns = gt["annotations"]
    by_gt, by_dt = {}, {}
    for k, a in enumerate(anns):
        by_gt.setdefault((int(a["image_id"]), int(a["category_id"])), []).append(k)
    for k, r in enumerate(dt):
        by_dt.setdefault((int(r["image_id"]), int(r["category_id"])), []).append(k)
    cache = {}

    def mask_of(kind, k, entry, image):
        if (kind, k) not in cache:
            cache[kind, k] = pixels(counts_of(entry["segmentation"]), size[image][0] * size[image][1])
        return cache[kind, k]

    groups = {}
    for i in img_ids:
        cache.clear()                                  # decoded masks are kept for one image at a time
        for c in cat_ids:
            g, d = by_gt.get((i, c), []), by_dt.get((i, c), [])
            if not g and not d:
                continue
            order = np.argsort([-dt[k]["score"] for k in d], kind="mergesort")
            d = [d[o] for o in order][:max_dets[-1]]
            crowd = [int(anns[k].get("iscrowd", 0)) != 0 for k in g]
            flag = [crowd[n] or (bool(p["use_ignore_field"]) and bool(anns[k].get("ignore", 0))) for n, k in enumerate(g)]
            ious = np.zeros((len(d), len(g)), np.float64)
            inter = np.zeros((len(d), len(g)), np.int64)
            for a, kd in enumerate(d):
                for b, kg in enumerate(g):
                    if iou_type == "segm":
                        inter[a, b], ious[a, b] = mask_iou(mask_of("d", kd, dt[kd], i), mask_of("g", kg, anns[kg], i), crowd[b])
                    else:
                        ious[a, b] = box_iou(dt[kd]["bbox"], anns[kg]["bbox"], crowd[b])
            if iou_type == "segm":
                dt_area = [float(np.count_nonzero(mask_of("d", kd, dt[kd], i))) for kd in d]
            else:
                dt_area = [float(np.float64(dt[kd]["bbox"][2]) * np.float64(dt[kd]["bbox"][3])) for kd in d]
            gt_area = [float(anns[k]["area"]) for k in g]
            per = [match(ious, gt_area, flag, crowd, dt_area, lo, hi, iou_thrs) for lo, hi in area_rng]
            groups[i, c] = dict(image=i, cat=c, d=d, g=g, ious=ious, inter=inter, dt_area=dt_area, gt_area=gt_area, flag=flag,
                                crowd=crowd, scores=[float(dt[k]["score"]) for k in d], per=per)
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(cat_ids), len(area_rng), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k, c in enumerate(cat_ids):
        E = [groups[i, c] for i in img_ids if (i, c) in groups]
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                if not E:
                    continue
                dt_scores = np.concatenate([np.asarray(e["scores"][:max_det], np.float64) for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                sorted_scores = dt_scores[inds]
                dtm = np.concatenate([e["per"][a][0][:, :max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["per"][a][1][:, :max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["per"][a][3] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm > -1, np.logical_not(dt_ig))
                fps = np.logical_and(dtm == -1, np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    at = np.searchsorted(rc, rec_thrs, side="left")
                    try:
                        for ri, pi in enumerate(at):
                            q[ri] = pr[pi]
                            ss[ri] = sorted_scores[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return dict(precision=precision, recall=recall, scores=scores, stats=summarize(precision, recall, p), groups=groups,
                img_ids=img_ids, cat_ids=cat_ids)


def summarize(precision, recall, p):
    iou_thrs, lbl, dets = np.asarray(p["iou_thrs"], np.float64), list(p["area_rng_lbl"]), list(p["max_dets"])

    def one(ap=1, iou_thr=None, area="all", max_det=100):
        a = [i for i, v in enumerate(lbl) if v == area]
        m = [i for i, v in enumerate(dets) if v == max_det]
        s = precision[:, :, :, a, m] if ap == 1 else recall[:, :, a, m]
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    return np.array([one(1, max_det=dets[2]), one(1, .5, max_det=dets[2]), one(1, .75, max_det=dets[2]),
                     one(1, area="small", max_det=dets[2]), one(1, area="medium", max_det=dets[2]),
                     one(1, area="large", max_det=dets[2]), one(0, max_det=dets[0]), one(0, max_det=dets[1]),
                     one(0, max_det=dets[2]), one(0, area="small", max_det=dets[2]), one(0, area="medium", max_det=dets[2]),
                     one(0, area="large", max_det=dets[2])])
