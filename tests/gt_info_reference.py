"""A NumPy float64 restatement of the BOP toolkit's scripts/calc_gt_info.py:117-177 per (job, pixel), written from the
rules in the header comment of gt_info_kernel (pegasus_amd/csrc/meshraster.hip.h); it shares no code with
pegasus_amd.mesh_render.  tests/test_gt_info_host.py pins it on the toolkit's recorded outputs (tests/golden/mesh_gt_info.npz).

  silhouette   canvas > 0 over the WHOLE canvas: px_count_all and the object box, in image coordinates (canvas - margin)
  distances    inside the image window, dist = sqrt((X X + Y Y) + d d) with X = (x - cx) / fx d and Y = (y - cy) / fy d in
               float64, the pixel taken at its integer index (misc.depth_im_to_dist_im_fast), for the canvas and for the
               scene depth of the job's frame
  visibility   both distances rounded to float32, their difference taken in float32 (visibility.py, mode bop19):
               visib = (dist_model - dist_test <= delta or dist_test == 0) and dist_model > 0, delta a float32
  mask         dist_model > 0
  stats        px_count_all, px_count_valid = #(mask and dist_test > 0), px_count_visib, then min x, min y, max x, max y of
               the silhouette and of the visible mask (INT32_MAX / INT32_MIN when empty)

Every output is an integer or a boolean of correctly rounded float64 + * / sqrt and one float32 subtraction, so a correct
implementation equals this one exactly; the formulas are followed literally for negative, NaN and infinite depths too."""
import numpy as np

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
STATS = 11


def dist_image(depth, fx, fy, cx, cy):
    """float64 [H,W] distances from the camera centre of a float32 depth image [H,W]."""
    d = np.asarray(depth, np.float32).astype(np.float64)
    H, W = d.shape
    with np.errstate(all="ignore"):
        X = ((np.arange(W, dtype=np.float64)[None, :] - np.float64(cx)) / np.float64(fx)) * d
        Y = ((np.arange(H, dtype=np.float64)[:, None] - np.float64(cy)) / np.float64(fy)) * d
        return np.sqrt((X * X + Y * Y) + d * d)


def _extent(m, ox, oy):
    ys, xs = np.nonzero(m)
    if not len(xs):
        return [INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN]
    return [int(xs.min()) - ox, int(ys.min()) - oy, int(xs.max()) - ox, int(ys.max()) - oy]


def reduce_job(canvas, margin, scene, fx, fy, cx, cy, delta):
    """One (object, image) pair: canvas float32 [Hc,Wc], scene float32 [H,W] -> (mask bool [H,W], visib bool [H,W],
    stats list of 11)."""
    mx, my = int(margin[0]), int(margin[1])
    H, W = scene.shape
    canvas = np.asarray(canvas, np.float32)
    with np.errstate(all="ignore"):
        large = canvas > 0
        dist_model = dist_image(canvas[my:my + H, mx:mx + W], fx, fy, cx, cy)
        dist_test = dist_image(scene, fx, fy, cx, cy)
        model32, test32 = dist_model.astype(np.float32), dist_test.astype(np.float32)
        diff = model32 - test32                                               # float32 - float32 -> float32
        assert diff.dtype == np.float32
        mask = model32 > 0
        visib = ((diff <= np.float32(delta)) | (test32 == 0)) & mask
        valid = mask & (test32 > 0)
    stats = [int(large.sum()), int(valid.sum()), int(visib.sum())] + _extent(large, mx, my) + _extent(visib, 0, 0)
    return mask, visib, stats


def reduce(canvases, margin, scene_depth, slots, frames, K, delta):
    """All jobs: canvases float32 [S,Hc,Wc], scene_depth float32 [F,H,W], slots and frames int [J] (true indirections),
    K float64 [J,4] = fx, fy, cx, cy of each job.  Returns (mask uint8 [J,H,W], mask_visib uint8 [J,H,W], stats int32 [J,11])."""
    slots, frames = np.asarray(slots, np.int64), np.asarray(frames, np.int64)
    K = np.asarray(K, np.float64).reshape(len(slots), 4)
    H, W = scene_depth.shape[-2:]
    mask = np.zeros((len(slots), H, W), np.uint8)
    visib = np.zeros_like(mask)
    stats = np.zeros((len(slots), STATS), np.int32)
    for k, (s, f) in enumerate(zip(slots, frames)):
        m, v, row = reduce_job(canvases[s], margin, scene_depth[f], *K[k], delta)
        mask[k], visib[k], stats[k] = m, v, row
    return mask, visib, stats


def info(stats):
    """The scene_gt_info fields calc_gt_info.py derives from a stats row, as plain Python: visib_fract = visible / all (0
    without a silhouette), boxes (x, y, x_max - x_min, y_max - y_min) as misc.calc_2d_bbox, both [-1] * 4 unless something
    is visible."""
    out = []
    for s in np.asarray(stats, np.int64).reshape(-1, STATS).tolist():
        box = lambda c: [s[c], s[c + 1], s[c + 2] - s[c], s[c + 3] - s[c + 1]]
        seen = s[2] > 0
        out.append(dict(px_count_all=s[0], px_count_valid=s[1], px_count_visib=s[2], visib_fract=s[2] / float(s[0]) if s[0] > 0 else 0.0,
                        bbox_obj=box(3) if seen else [-1] * 4, bbox_visib=box(7) if seen else [-1] * 4))
    return out
