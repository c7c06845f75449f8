"""The device PNG encoder on the images of a rendered batch (DESIGN.md section 23 "Measured").

    python scripts/png_bench.py [--workload c3 --scale 0.1 --frames 32 --size 800 --repeats 5 --zlib-frames 4] [--out FILE.json]

Renders one batch of the scene as `pegasus_amd.generate` does (records-only frames, the semantic image, silhouettes), then
  (a) times pgr_png_encode + pgr_png_emit with HIP events, per image kind and for the batch's whole job list (the writer's one
      call), best of --repeats: milliseconds and GB/s of raw samples;
  (b) prints the bytes of the files per kind beside zlib.compress(raw stream, 1) + the 57 framing bytes, which are the host
      encoder's files, for the first --zlib-frames frames.
One JSON document on stdout."""
from __future__ import annotations

import argparse
import json
import sys
import zlib
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def timed_encode(images, scales, level, repeats):
    """(best milliseconds of encode + emit by HIP events, file sizes int64 [n])."""
    import torch
    from pegasus_amd import _lib, png
    dev, n = images[0].device, len(images)
    jobs = (_lib.PgrPngJob * n)(*[png._job(t, s) for t, s in zip(images, scales)])
    ws = _lib.workspace("pgr_png", dev, n, jobs)
    sizes = torch.empty(n, dtype=torch.int64, device=dev)
    best = float("inf")
    for _ in range(repeats + 1):                             # the first pass warms up
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        _lib.call("pgr_png_encode", dev, jobs, n, level, _lib.ptr(sizes), _lib.ptr(ws), ws.numel())
        ev[1].record()
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(sizes, 0, out=offsets[1:])
        total = int(offsets[-1])
        files = torch.empty(total, dtype=torch.uint8, device=dev)
        ev[2].record()
        _lib.call("pgr_png_emit", dev, jobs, n, _lib.ptr(offsets), total, _lib.ptr(files), total, _lib.ptr(ws), ws.numel())
        ev[3].record()
        torch.cuda.synchronize(dev)
        best = min(best, ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3]))
    return best, sizes.cpu().numpy()


def raw_stream(image, scale):
    """The filtered raw stream of one image as the encoder reads it (host, numpy)."""
    a = image.cpu().numpy()
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    rows = (a.astype(">u2").view(np.uint8) if a.dtype == np.uint16 else a * np.uint8(scale)).reshape(a.shape[0], -1)
    return np.concatenate([np.zeros((a.shape[0], 1), np.uint8), rows], axis=1).tobytes()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3", choices=["c2", "c3", "c5"])
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--zlib-frames", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from pegasus_amd import masks as M, scenes
    from pegasus_amd.frames import FrameRenderer
    if not torch.cuda.is_available():
        raise SystemExit("png_bench needs a HIP device")
    maker = dict(c2=lambda: scenes.scene_c2(n=int(150_000 * args.scale), n_views=args.frames, width=args.size, height=args.size),
                 c3=lambda: scenes.scene_c3(scale=args.scale, n_views=args.frames, width=args.size, height=args.size),
                 c5=lambda: scenes.scene_c5(scale=args.scale, n_views=args.frames, width=args.size, height=args.size))
    cloud, views = maker[args.workload]()
    act = cloud.activated()
    fr = FrameRenderer(act["means3d"], act["opacities"], act["scales"], act["rotations"], act["shs"], cloud.object_id, device="cuda:0")
    specs = [fr.view_spec(v) for v in views[:args.frames]]
    H, W, B, K = int(specs[0].image_height), int(specs[0].image_width), len(specs), fr.K
    frames = fr.render_frames(specs, frames=fr.alloc_frames(B, H, W, records=True, images="seg"))
    sil = fr.render_silhouettes(specs) if K else None
    torch.cuda.synchronize()
    rv = M.record_views(frames["records"][:B], H, W, K)
    vis = M.unpack_mask_bits(rv["mask_bits"], K) if K else None
    sem = M.pack_frames(color=frames["seg"][:B])["rgb"]
    kinds = {"rgb": ([rv["rgb"][i] for i in range(B)], 1), "depth": ([rv["depth_mm"][i] for i in range(B)], 1),
             "sem_mask": ([sem[i] for i in range(B)], 1)}
    if K:
        kinds["mask_visib"] = ([vis[i, k] for i in range(B) for k in range(K)], 255)
        kinds["mask"] = ([sil[i, k] for i in range(B) for k in range(K)], 255)
    doc = {"workload": args.workload, "scale": args.scale, "frames": B, "size": [W, H], "objects": K, "level": args.level,
           "device": torch.cuda.get_device_name(0), "kinds": {}}
    every, every_scales = [], []
    for name, (images, scale) in kinds.items():
        ms, sizes = timed_encode(images, [scale] * len(images), args.level, args.repeats)
        raw = sum(int(t.shape[0]) * (1 + int(t.shape[1]) * (t.element_size() if t.dim() == 2 else 3)) for t in images)
        per_frame = len(images) // B
        n_z = min(args.zlib_frames, B) * per_frame
        host = sum(len(zlib.compress(raw_stream(t, scale), 1)) + 57 for t in images[:n_z])
        doc["kinds"][name] = {"files": len(images), "raw_bytes": raw, "ms": round(ms, 3), "raw_GB_per_s": round(raw / ms / 1e6, 1),
                              "file_bytes": int(sizes.sum()), "compared_files": n_z, "gpu_bytes_compared": int(sizes[:n_z].sum()),
                              "zlib1_bytes_compared": host, "gpu_over_zlib1": round(float(sizes[:n_z].sum()) / host, 3)}
        every += images
        every_scales += [scale] * len(images)
    ms, sizes = timed_encode(every, every_scales, args.level, args.repeats)
    raw = sum(k["raw_bytes"] for k in doc["kinds"].values())
    doc["batch"] = {"files": len(every), "raw_bytes": raw, "ms": round(ms, 3), "raw_GB_per_s": round(raw / ms / 1e6, 1),
                    "file_bytes": int(sizes.sum()), "frames_per_s": round(B / ms * 1e3, 1)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
