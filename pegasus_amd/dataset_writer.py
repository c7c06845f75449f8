"""BOP-layout writer for the batch path ("mask/depth writers").

The directory layout, the file names, the record files and the PNG codec are ``pegasus_amd.bop_dataset``'s; this module
fills them from the renderer's frames: the five image kinds of the reference's write_training_data
(src/tools/pegasus_working.py:412-439) for the data points ['rgb','depth','seg_vis','seg_sil','sem_seg'], scene_gt_info.json
when a batch brings both visible masks and silhouettes (or meshes), scene_gt_coco.json for batches added with ``coco=``.
Quantisation runs on the GPU (pgr_quantize_frame); only the 8/16-bit images cross PCIe.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from . import bop_dataset as BD
from .bop_dataset import decode_png, encode_png  # noqa: F401  (importable from here too)


class BopSceneWriter:
    """Collects the frames of one scene; `add_batch` takes FrameRenderer output (device tensors) + pose records.

    PNG encoding is the only per-frame host work of the batch path and, on one thread, 100x slower than rendering
    (2.9 s for 64 frames that render in 26 ms).  Like the reference, which starts a thread per frame for its writers
    (/root/reference/pegasus.py:346-358), the encoder runs beside the renderer: `add_batch` quantises on the GPU, copies
    the 8/16-bit images to the host once per batch and hands one task per PNG to a thread pool (zlib releases the GIL);
    `close()` waits for them.  At most `max_pending` batches are in flight (bounded host memory).

    ``encoder="gpu"`` encodes on the device instead (pegasus_amd.png): `add_batch` lists every image of
    the batch where it lies -- rgb, depth, visible masks, silhouettes, the semantic image, with ``meshes=`` the mesh masks --
    makes ONE ``png.encode_batch`` call, and the thread pool only writes slices of the one buffer that came back to their
    paths.  Same directory, same file names, files that decode to the same arrays; the JSON records, scene_gt_info and the
    COCO annotations do not depend on the encoder.  The default stays the host encoder.

    ``rgb_format="jpg"`` writes the colour images as ``rgb/<id>.jpg``, as BOP's own train_pbr splits store them: ONE
    ``jpeg.encode_batch`` call per batch on the device (pegasus_amd.jpeg) at ``jpeg_quality`` and
    ``jpeg_subsampling`` ('4:4:4' or '4:2:0'), whatever ``encoder`` is; every other kind follows ``encoder`` as before and
    scene_gt_coco.json names the .jpg.  The default stays "png"."""

    def __init__(self, out_dir, scene_id: int = 0, png_level: int = 1, workers: int = None, max_pending: int = 4,
                 encoder: str = "host", rgb_format: str = "png", jpeg_quality: int = 95, jpeg_subsampling: str = "4:4:4"):
        import os
        from concurrent.futures import ThreadPoolExecutor
        self.scene = BD.scene_dir(out_dir, "train", scene_id)
        self.files = BD.BopScene(self.scene)
        self.files.make_dirs()
        self.scene_gt, self.scene_camera, self.scene_gt_info = {}, {}, {}
        self.scene_gt_coco, self.coco_bbox_type, self.coco_size = {}, None, None      # per frame: annotations without ids
        self.dataset_name = Path(out_dir).resolve().name
        self.n_frames, self.level = 0, png_level
        if encoder not in ("host", "gpu"):
            raise ValueError(f"encoder={encoder!r}: 'host' or 'gpu'")
        self.encoder = encoder
        if rgb_format not in ("png", "jpg"):
            raise ValueError(f"rgb_format={rgb_format!r}: 'png' or 'jpg'")
        if rgb_format == "jpg":
            from . import jpeg
            jpeg.subsampling_code(jpeg_subsampling)          # raises on anything but 4:4:4 / 4:2:0
            if not 1 <= int(jpeg_quality) <= 100:
                raise ValueError(f"jpeg_quality={jpeg_quality!r}: 1..100")
        self.rgb_format, self.jpeg_quality, self.jpeg_subsampling = rgb_format, int(jpeg_quality), jpeg_subsampling
        self._jpeg_jobs = []                                 # rgb_format="jpg": (device image, path) of the batch being added
        self._gpu_jobs = []                                  # encoder="gpu": (device image, scale, path) of the batch being added
        self.workers = max(1, min(32, os.cpu_count() or 1) if workers is None else int(workers))
        self._pool = ThreadPoolExecutor(max_workers=self.workers) if self.workers > 1 else None
        self._pending, self._max_pending = [], max(1, int(max_pending))

    def _write(self, path, image):
        path.write_bytes(encode_png(image, self.level))

    def _submit(self, batch_futures, image, kind, i, k=None, scale=1):
        """``image``: a host array (encoder="host"), or a device tensor whose samples times ``scale`` are what is written."""
        path = self.files.image_path(kind, i, k)
        if self.encoder == "gpu":
            self._gpu_jobs.append((image, scale, path))
        elif self._pool is None:
            self._write(path, image)
        else:
            batch_futures.append(self._pool.submit(self._write, path, image))

    def _encode_gpu_jobs(self, batch_futures):
        """One device encode for everything `_submit` listed; the pool (or this thread) writes the slices."""
        from . import png
        jobs, self._gpu_jobs = self._gpu_jobs, []
        if not jobs:
            return
        files, offsets = png.encode_batch([j[0] for j in jobs], level=1 if self.level else 0, scale=[j[1] for j in jobs])
        for k, (_, _, path) in enumerate(jobs):
            data = files[offsets[k]:offsets[k + 1]]
            if self._pool is None:
                path.write_bytes(data)
            else:
                batch_futures.append(self._pool.submit(path.write_bytes, data))

    def _encode_jpeg_jobs(self, batch_futures):
        """One device encode for the batch's colour images; the pool (or this thread) writes the slices."""
        from . import jpeg
        jobs, self._jpeg_jobs = self._jpeg_jobs, []
        if not jobs:
            return
        files, offsets = jpeg.encode_batch([j[0] for j in jobs], self.jpeg_quality, self.jpeg_subsampling)
        for k, (_, path) in enumerate(jobs):
            data = files[offsets[k]:offsets[k + 1]]
            if self._pool is None:
                path.write_bytes(data)
            else:
                batch_futures.append(self._pool.submit(path.write_bytes, data))

    def add_batch(self, frames: dict, scene_gt: dict, scene_camera: dict, n: int = None, silhouettes=None, frame_ids=None,
                  record_shape=None, meshes=None, delta: float = 15.0, translation_scale: float = 1.0, coco=False):
        """``frames``: FrameRenderer output (color, depth, and with masks: seg, masks); ``silhouettes``: uint8 [B,K,H,W]
        of FrameRenderer.render_silhouettes (or frames["sil"]) -> the mask/ directory.  ``frame_ids``: the frames' numbers in
        the dataset (default: consecutive) -- a view-sharded run gives every rank's writer the GLOBAL ids of its frames.
        ``meshes``: a mesh_render.MeshSet in scene_gt's unit (``translation_scale``: 1 = metres, 1000 = millimetres) -> mask/,
        mask_visib/ and scene_gt_info.json come from the meshes' depth renders tested against the written depth image with
        tolerance ``delta`` millimetres (mesh_render.gt_from_meshes: the toolkit's calc_gt_info.py and calc_gt_masks.py),
        not from the splat masks.  ``coco``: True or 'amodal' / 'modal' -> the batch's COCO annotations (pegasus_amd.coco:
        run-length masks of the visible masks, boxes of the full masks or, modal, of the visible ones) are encoded on the
        device from the masks the PNGs are written from -- the meshes' when ``meshes`` is given, else the splat masks and
        silhouettes -- and kept per frame like scene_gt_info; ``write_records`` numbers them into scene_gt_coco.json."""
        from . import masks as M
        bbox_type = None
        if coco:
            from . import coco as CO
            bbox_type = "amodal" if coco is True else str(coco)
            if bbox_type not in ("amodal", "modal"):
                raise ValueError(f"coco={coco!r}: True, 'amodal' or 'modal'")
            if self.coco_bbox_type not in (None, bbox_type):
                raise ValueError(f"this scene's annotations are {self.coco_bbox_type}; one file holds one box type")
        masks_dev = frames.get("masks")
        gpu = self.encoder == "gpu"
        jpg = self.rgb_format == "jpg"
        if "color" in frames:
            n = frames["color"].shape[0] if n is None else n
            # GPU: uint8 HWC / uint16 millimetres for the whole batch in one launch (pgr_pack_frames), then ONE
            # device->host copy per kind and batch
            packed = M.pack_frames(color=frames["color"][:n], depth=frames["depth"][:n])
            depth_mm_dev = packed["depth_mm"]
            rgb8 = packed["rgb"] if gpu or jpg else packed["rgb"].cpu().numpy()
            mm = depth_mm_dev if gpu else depth_mm_dev.cpu().numpy().view(np.uint16)
        else:
            # a records-only frame set (FrameRenderer.alloc_frames(images=False | "seg")): the compositor's epilogue wrote the
            # casts already -- the record IS what the writers take
            if record_shape is None:
                raise ValueError("a frame set without images needs record_shape=(H, W, K)")
            n = frames["records"].shape[0] if n is None else n
            H, W, K = (int(v) for v in record_shape)
            rv = M.record_views(frames["records"][:n], H, W, K)
            depth_mm_dev = rv["depth_mm"]
            # encoder="gpu": the record's own RGB and depth planes are the encoder's input, read where they lie
            rgb8 = rv["rgb"] if gpu or jpg else rv["rgb"].cpu().numpy()
            mm = depth_mm_dev if gpu else depth_mm_dev.cpu().numpy().view(np.uint16)
            masks_dev = M.unpack_mask_bits(rv["mask_bits"], K) if K else None
        if silhouettes is None:
            silhouettes = frames.get("sil")
        coco_enc = None
        if bbox_type is not None and meshes is None:
            # encoded on the device before the masks are fetched: a few hundred run lengths per mask beside its 640 kB
            n_entries = sum(len(scene_gt[str(i)]) for i in range(n))
            if masks_dev is None and n_entries:
                raise ValueError("coco= needs the batch's visible masks (or meshes=)")
            if bbox_type == "amodal" and silhouettes is None:
                raise ValueError("a batch without silhouettes and without meshes supports coco='modal' only: amodal boxes "
                                 "are those of the full masks")
            if n_entries:
                coco_enc = CO.encode_stack(masks_dev[:n].flatten(0, 1),
                                           silhouettes[:n].flatten(0, 1) if bbox_type == "amodal" else None)
        if gpu:
            # 0 / 1 planes as they lie: the encoder writes them as 0 / 255 (scale)
            mk = masks_dev[:n] if masks_dev is not None else None
            sem8 = M.pack_frames(color=frames["seg"][:n])["rgb"] if "seg" in frames else None
            sil = silhouettes[:n] if silhouettes is not None else None
        else:
            mk = (masks_dev[:n] * 255).cpu().numpy() if masks_dev is not None else None
            sem8 = M.pack_frames(color=frames["seg"][:n])["rgb"].cpu().numpy() if "seg" in frames else None
            sil = (silhouettes[:n] * 255).cpu().numpy() if silhouettes is not None else None
        mask_scale = 255 if gpu else 1
        info = None
        if silhouettes is not None and masks_dev is not None:
            # BOP's scene_gt_info from the masks the batch already holds, counted on the GPU (a few hundred numbers per batch)
            from . import bop_pose
            info = bop_pose.gt_info_from_masks(masks_dev[:n], silhouettes[:n], depth_mm_dev != 0)
        mesh_gt = None
        if meshes is not None:
            import torch
            from . import mesh_render
            mm_dev = depth_mm_dev.to(torch.int32) & 0xFFFF                   # int16 storage of uint16 millimetres
            mesh_gt = mesh_render.gt_from_meshes(meshes, {str(i): scene_gt[str(i)] for i in range(n)},
                                                 {str(i): scene_camera[str(i)] for i in range(n)}, mm_dev, delta=delta,
                                                 translation_scale=translation_scale)
            mk = sil = info = None
            if bbox_type is not None and sum(len(v) for v in mesh_gt[1]):
                coco_enc = CO.encode_stack(torch.cat(mesh_gt[1]), torch.cat(mesh_gt[0]) if bbox_type == "amodal" else None)
        futures = []
        coco_at = 0
        for i in range(n):
            fid = self.n_frames if frame_ids is None else int(frame_ids[i])
            if bbox_type is not None:
                entries = scene_gt[str(i)]
                if mesh_gt is not None:
                    fract = [e["visib_fract"] for e in mesh_gt[2][i]]
                    H, W = mesh_gt[1][i].shape[-2:]
                else:
                    n_masks = masks_dev.shape[1] if masks_dev is not None else 0
                    if len(entries) != n_masks:
                        raise ValueError(f"frame {i}: {len(entries)} scene_gt entries for {n_masks} masks")
                    fract = [float(f) for f in info["visib_fract"][i]] if info is not None else None
                    H, W = masks_dev.shape[-2:] if masks_dev is not None else mm.shape[-2:]
                self.scene_gt_coco[str(fid)] = [] if coco_enc is None else CO.annotations_from_encoded(
                    *coco_enc, (H, W), [int(e["obj_id"]) for e in entries], fract, fid, bbox_type, coco_at)
                coco_at += len(entries)
                self.coco_bbox_type, self.coco_size = bbox_type, (int(W), int(H))
            if mesh_gt is not None:
                for name, stack in (("mask", mesh_gt[0][i]), ("mask_visib", mesh_gt[1][i])):
                    for k, image in enumerate(stack if gpu else (stack * 255).cpu().numpy()):
                        self._submit(futures, image, name, fid, k, mask_scale)
                self.scene_gt_info[str(fid)] = mesh_gt[2][i]
            if jpg:
                self._jpeg_jobs.append((rgb8[i], self.files.path / "rgb" / BD.image_name(fid, ext="jpg")))
            else:
                self._submit(futures, rgb8[i], "rgb", fid)
            self._submit(futures, mm[i], "depth", fid)
            if mk is not None:
                for k in range(mk.shape[1]):
                    self._submit(futures, mk[i, k], "mask_visib", fid, k, mask_scale)
            if sem8 is not None:
                self._submit(futures, sem8[i], "sem_mask", fid)
            if sil is not None:
                for k in range(sil.shape[1]):
                    self._submit(futures, sil[i, k], "mask", fid, k, mask_scale)
            self.scene_gt[str(fid)] = scene_gt[str(i)]
            self.scene_camera[str(fid)] = scene_camera[str(i)]
            if info is not None:
                from . import bop_pose
                self.scene_gt_info[str(fid)] = bop_pose.scene_gt_info_entry(info, i)
            self.n_frames += 1
        if gpu:
            self._encode_gpu_jobs(futures)
        if jpg:
            self._encode_jpeg_jobs(futures)
        if futures:
            self._pending.append(futures)
            while len(self._pending) > self._max_pending:
                for f in self._pending.pop(0):
                    f.result()                       # re-raises a writer's exception here

    def close(self, write_json: bool = True):
        """Waits for the PNG tasks; writes scene_gt.json / scene_camera.json unless ``write_json`` is False (a view-sharded
        run merges the ranks' records first: ``merge_records``)."""
        for batch in self._pending:
            for f in batch:
                f.result()
        self._pending = []
        if self._pool is not None:
            self._pool.shutdown(wait=True)
        if write_json:
            self.write_records()
        return self.scene

    def merge_records(self, others):
        """Adds the (scene_gt, scene_camera[, scene_gt_info[, coco_records()]]) tuples of other ranks' writers (disjoint
        frame ids).  The COCO annotations travel without ids: they are global to the scene, so only ``write_records`` of
        the merged writer numbers them.  They bring their box type and image size along, so a writer that added no batch
        of its own still writes the file."""
        for rec in others:
            self.scene_gt.update(rec[0])
            self.scene_camera.update(rec[1])
            if len(rec) > 2:
                self.scene_gt_info.update(rec[2])
            if len(rec) > 3 and rec[3]:
                bbox_type, size = rec[3]["bbox_type"], tuple(rec[3]["size"])
                if self.coco_bbox_type not in (None, bbox_type) or self.coco_size not in (None, size):
                    raise ValueError(f"annotations with {bbox_type} boxes of {size} images do not go with this writer's "
                                     f"{self.coco_bbox_type} boxes of {self.coco_size} images")
                self.coco_bbox_type, self.coco_size = bbox_type, size
                self.scene_gt_coco.update(rec[3]["frames"])

    def coco_records(self):
        """What ``merge_records`` takes as a tuple's fourth element: the per-frame annotations (without ids) with their box
        type and image size (W, H); None when no batch was added with ``coco=``."""
        if self.coco_bbox_type is None:
            return None
        return {"bbox_type": self.coco_bbox_type, "size": list(self.coco_size), "frames": self.scene_gt_coco}

    def write_records(self):
        self.files.write_json(BD.SCENE_GT, BD.by_frame(self.scene_gt))
        self.files.write_json(BD.SCENE_CAMERA, BD.by_frame(self.scene_camera))
        if self.scene_gt_info:
            self.files.write_json(BD.SCENE_GT_INFO, BD.by_frame(self.scene_gt_info))
        if self.coco_bbox_type is not None:
            from . import coco as CO
            images = [(int(k), f"rgb/{BD.image_name(k, ext=self.rgb_format)}", list(self.coco_size)) for k in self.scene_gt_coco]
            doc = CO.scene_coco(images, self.scene_gt_coco, CO.scene_obj_ids(self.scene_gt), self.dataset_name)
            self.files.write_json(CO.coco_file_name(self.coco_bbox_type), doc)
