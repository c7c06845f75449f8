"""Generates tests/golden/coco_rle.npz and tests/golden/coco_scene.json from the BOP toolkit of the reference checkout.

Run on the build machine only (``python tests/golden/make_golden_coco.py``); nothing at test time reads the reference.  Only
the toolkit's OUTPUTS are stored, no reference source text; the inputs are the deterministic masks of tests/coco_cases.py.
The functions of bop_toolkit_lib/pycoco_utils.py are called as scripts/calc_gt_coco.py calls them:
  coco_rle.npz      per case mask up to coco_cases.GOLDEN_MAX_PIXELS pixels: binary_mask_to_rle's counts and size,
                    bbox_from_binary_mask (non-empty masks), rle_to_binary_mask of those counts (bit-packed), and of lists
                    with zero-length runs in the middle; what compute_ious returns for a pair of stacks in which
                    every mask overlaps every other (so its unions can be read off as reciprocals)
  coco_scene.json   create_annotation_info's dicts for the case masks, and a scene file for the two images of
                    coco_cases.scene(), with amodal and with modal boxes.  The scene file is NOT recorded from the
                    toolkit's script, which only runs over a dataset on disk: its rules -- which instances are left out,
                    that a left-out instance takes no id, ids from 1 in image and instance order -- are restated below in
                    this project's terms, and only the dicts inside (create_annotation_info, create_image_info,
                    bbox_from_binary_mask) are the toolkit's outputs
skimage (polygon segmentations only) is not installed: a stub module stands in for it.
"""
import json
import sys
import types
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
sys.path.insert(0, str(OUT.parents[1]))

import coco_cases as CC          # noqa: E402

DATASET = "tiny"
ANNOTATION_MAX_PIXELS = 1200       # create_annotation_info is recorded for the small cases: its counts are in the npz


def toolkit():
    assert REF.exists(), "reference checkout not present"
    sys.path.insert(0, str(REF))
    sys.path.insert(0, str(REF / "submodules" / "bop_toolkit"))
    if "skimage" not in sys.modules:
        try:
            __import__("skimage")
        except Exception:
            sk = types.ModuleType("skimage")
            sk.measure = types.ModuleType("skimage.measure")
            sys.modules["skimage"], sys.modules["skimage.measure"] = sk, sk.measure
    for name in ("imageio", "png", "cv2"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
    from bop_toolkit_lib import pycoco_utils
    return pycoco_utils


def plain(o):
    """JSON types only (the toolkit leaves numpy integers and numpy bools in its dicts)."""
    if isinstance(o, dict):
        return {k: plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [plain(v) for v in o]
    if isinstance(o, (np.bool_, bool)):
        return bool(o)
    if isinstance(o, np.integer):
        return int(o)
    if isinstance(o, np.floating):
        return float(o)
    return o


def rle_golden(pc):
    out, annots = {}, {}
    names = []
    for name, stack, _ in CC.cases():
        if stack.shape[1] * stack.shape[2] > CC.GOLDEN_MAX_PIXELS:
            continue
        names.append(name)
        key = f"case{len(names) - 1}"
        counts, boxes, decoded = [], [], []
        for k, m in enumerate(stack):
            b = m.astype(bool)
            rle = pc.binary_mask_to_rle(b)
            assert rle["size"] == list(m.shape)
            counts.append(np.asarray(rle["counts"], np.int64))
            boxes.append(pc.bbox_from_binary_mask(b) if b.any() else [-1, -1, -1, -1])
            decoded.append(np.asarray(pc.rle_to_binary_mask(rle), bool))
            if m.size <= ANNOTATION_MAX_PIXELS:
                ann = pc.create_annotation_info(7, 3, 11, b, boxes[-1], ignore=bool(k % 2))
                annots[f"{name}/{k}"] = plain(ann)
        out[f"{key}_counts"] = np.concatenate(counts)
        out[f"{key}_lengths"] = np.asarray([len(c) for c in counts], np.int64)
        out[f"{key}_bbox"] = np.asarray(boxes, np.int64)
        out[f"{key}_decoded"] = np.packbits(np.stack(decoded), axis=-1)
        print(name, stack.shape, [len(c) for c in counts])
    out["names"] = np.asarray(names)
    # zero-length runs in the middle of a list (and at its ends), 5 x 4 = [H, W]
    zero_lists = [[0, 3, 0, 0, 2, 0, 15], [4, 0, 0, 6, 0, 10, 0], [0, 0, 0, 20], [20, 0, 0]]
    out["zero_counts"] = np.concatenate([np.asarray(c, np.int64) for c in zero_lists])
    out["zero_lengths"] = np.asarray([len(c) for c in zero_lists], np.int64)
    out["zero_size"] = np.asarray([5, 4], np.int64)
    out["zero_decoded"] = np.stack([np.asarray(pc.rle_to_binary_mask({"counts": c, "size": [5, 4]}), np.uint8) for c in zero_lists])
    # compute_ious as it is: any-overlap over union.  Every pair of these stacks overlaps, so no entry is 0.
    stack = dict((n, s) for n, s, _ in CC.cases())["odd 17x33"]
    mirrored = stack[:, ::-1].copy()
    as_annotations = lambda masks: [{"segmentation": pc.binary_mask_to_rle(m.astype(bool))} for m in masks]
    ious = pc.compute_ious(as_annotations(stack), as_annotations(mirrored), "segm")
    out["ious_toolkit"] = np.asarray(ious, np.float64)
    assert (out["ious_toolkit"] > 0).all()
    print("compute_ious", ious.dtype, np.round(ious, 5).tolist())
    np.savez_compressed(OUT / "coco_rle.npz", **out)
    return annots


def scene_golden(pc):
    """A scene file for coco_cases.scene() per box type, numbered by this project's restatement of the rules (see the module
    docstring); the image and annotation dicts are what the toolkit's functions return."""
    docs = {}
    for bbox_type in ("amodal", "modal"):
        images, annotations, categories = [], [], set()
        for image_id, instances in sorted(CC.scene().items()):
            images.append(pc.create_image_info(image_id, f"rgb/{image_id:06d}.png", [CC.SCENE_W, CC.SCENE_H]))
            for obj_id, visible, full, visib_fract in instances:
                categories.add(obj_id)
                visible, full = visible != 0, full != 0
                boxed = full if bbox_type == "amodal" else visible
                if not visible.any() or not boxed.any():
                    continue                                                   # left out, and takes no id
                annotations.append(pc.create_annotation_info(len(annotations) + 1, image_id, obj_id, visible,
                                                             pc.bbox_from_binary_mask(boxed), ignore=visib_fract < 0.1))
        assert all(a is not None for a in annotations)
        docs[bbox_type] = plain({"info": {"description": DATASET + "_train", "url": "https://github.com/thodan/bop_toolkit",
                                          "version": "0.1.0", "contributor": ""},
                                 "licenses": [], "categories": [{"id": o, "name": str(o), "supercategory": DATASET} for o in sorted(categories)],
                                 "images": images, "annotations": annotations})
        print(bbox_type, [(a["id"], a["image_id"], a["category_id"], a["ignore"]) for a in annotations])
    return docs


if __name__ == "__main__":
    pc = toolkit()
    annots = rle_golden(pc)
    docs = scene_golden(pc)
    (OUT / "coco_scene.json").write_text(json.dumps({"dataset": DATASET, "annotation_info": annots, "scene": docs},
                                                    separators=(",", ":")) + "\n")
    for p in ("coco_rle.npz", "coco_scene.json"):
        print(p, (OUT / p).stat().st_size, "bytes")
