"""The measurements of DESIGN.md section 27 on one device: the JPEG encoder on 32 rendered frames of 800 x 800 (quality 95,
both subsamplings) beside the PNG encoder and PIL on 16 threads, 32 images of 4000 x 3000, file size and PSNR against PIL at
equal settings, the workspace, and end to end `generate` and the `undistort` command line with and without the device encoder.

    python scripts/jpeg_bench.py [--out profiles/jpeg_bench.json] [--skip-end-to-end]

HIP events, median of --repeats after a warm-up pass.  One JSON document."""
from __future__ import annotations

import argparse
import io
import json
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timed_jpeg(images, quality, sub, repeats):
    """(median ms of the encode pass, of the emit pass, file sizes, workspace bytes)."""
    import torch
    from pegasus_amd import _lib, jpeg
    dev, n = images[0].device, len(images)
    jobs = (_lib.PgrJpegJob * n)(*[jpeg._job(t, quality, jpeg.subsampling_code(sub)) for t in images])
    ws = _lib.workspace("pgr_jpeg", dev, n, jobs)
    sizes = torch.empty(n, dtype=torch.int64, device=dev)
    enc, emit = [], []
    for _ in range(repeats + 1):                             # the first pass warms up
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        _lib.call("pgr_jpeg_encode", dev, jobs, n, _lib.ptr(sizes), _lib.ptr(ws), ws.numel())
        ev[1].record()
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(sizes, 0, out=offsets[1:])
        total = int(offsets[-1])
        files = torch.empty(total, dtype=torch.uint8, device=dev)
        ev[2].record()
        _lib.call("pgr_jpeg_emit", dev, jobs, n, _lib.ptr(offsets), total, _lib.ptr(files), total, _lib.ptr(ws), ws.numel())
        ev[3].record()
        torch.cuda.synchronize(dev)
        enc.append(ev[0].elapsed_time(ev[1]))
        emit.append(ev[2].elapsed_time(ev[3]))
    return float(np.median(enc[1:])), float(np.median(emit[1:])), sizes.cpu().numpy(), int(ws.numel())


def jpeg_entry(images, quality, sub, repeats):
    enc, emit, sizes, ws = timed_jpeg(images, quality, sub, repeats)
    samples = sum(int(t.numel()) for t in images)
    return {"files": len(images), "quality": quality, "subsampling": sub, "sample_bytes": samples, "encode_ms": round(enc, 3),
            "emit_ms": round(emit, 3), "ms": round(enc + emit, 3), "sample_GB_per_s": round(samples / (enc + emit) / 1e6, 1),
            "file_bytes": int(sizes.sum()), "workspace_bytes": ws}


def timed_png(images, repeats):
    import torch
    from pegasus_amd import _lib, png
    dev, n = images[0].device, len(images)
    jobs = (_lib.PgrPngJob * n)(*[png._job(t, 1) for t in images])
    ws = _lib.workspace("pgr_png", dev, n, jobs)
    sizes = torch.empty(n, dtype=torch.int64, device=dev)
    ms = []
    for _ in range(repeats + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        _lib.call("pgr_png_encode", dev, jobs, n, 1, _lib.ptr(sizes), _lib.ptr(ws), ws.numel())
        ev[1].record()
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(sizes, 0, out=offsets[1:])
        total = int(offsets[-1])
        files = torch.empty(total, dtype=torch.uint8, device=dev)
        ev[2].record()
        _lib.call("pgr_png_emit", dev, jobs, n, _lib.ptr(offsets), total, _lib.ptr(files), total, _lib.ptr(ws), ws.numel())
        ev[3].record()
        torch.cuda.synchronize(dev)
        ms.append(ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3]))
    return {"files": n, "ms": round(float(np.median(ms[1:])), 3), "file_bytes": int(sizes.sum().item()), "workspace_bytes": int(ws.numel())}


def pil_bytes(a, quality, sub, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=sub, **kw)
    return b.getvalue()


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def rendered_frames(n, size):
    """The RGB planes of n rendered frames of the c3 workload at scale 0.1, uint8 [n] x [H,W,3] views of the records."""
    import torch
    from pegasus_amd import masks as M, scenes
    from pegasus_amd.frames import FrameRenderer
    cloud, views = scenes.scene_c3(scale=0.1, n_views=n, width=size, height=size)
    act = cloud.activated()
    fr = FrameRenderer(act["means3d"], act["opacities"], act["scales"], act["rotations"], act["shs"], cloud.object_id, device="cuda:0")
    specs = [fr.view_spec(v) for v in views[:n]]
    H, W = int(specs[0].image_height), int(specs[0].image_width)
    frames = fr.render_frames(specs, frames=fr.alloc_frames(n, H, W, records=True, images=False))
    torch.cuda.synchronize()
    rv = M.record_views(frames["records"][:n], H, W, fr.K)
    return [rv["rgb"][i] for i in range(n)], frames


def photo_like(n, h, w):
    """Smooth colour fields with edges and sensor noise, not zeros: uint8 [h,w,3] device tensors."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    out = []
    for _ in range(n):
        low = torch.rand((1, 3, h // 64 + 2, w // 64 + 2), device="cuda", generator=g)
        im = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0]
        im = (im * 255 + torch.randn((3, h, w), device="cuda", generator=g) * 2.0).clamp_(0, 255)
        out.append(im.permute(1, 2, 0).to(torch.uint8).contiguous())
    return out


def dir_bytes(path):
    return sum(p.stat().st_size for p in Path(path).rglob("*") if p.is_file())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "jpeg_bench.json"))
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--kernels-only", action="store_true",
                    help="only the two 800 x 800 encodes: what to run under rocprofv3 --kernel-trace --stats for each kernel's share")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench needs a HIP device")
    doc = {"device": torch.cuda.get_device_name(0)}

    rgb, keep = rendered_frames(32, 800)
    for sub in ("4:4:4", "4:2:0"):
        doc[f"frames_800_q95_{sub.replace(':', '')}"] = jpeg_entry(rgb, 95, sub, args.repeats)
    if args.kernels_only:
        print(json.dumps(doc, indent=1))
        return
    doc["frames_800_png"] = timed_png(rgb, args.repeats)
    host = [t.cpu().numpy() for t in rgb]
    with ThreadPoolExecutor(16) as pool:
        for sub in ("4:4:4", "4:2:0"):
            list(pool.map(lambda a: pil_bytes(a, 95, sub), host[:16]))
            t0 = time.perf_counter()
            sizes = list(pool.map(lambda a: len(pil_bytes(a, 95, sub)), host))
            doc[f"frames_800_pil16_{sub.replace(':', '')}"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "file_bytes": int(sum(sizes))}
    # size and PSNR against PIL at equal settings (its own optimised tables, the same restart interval), PIL decoding both
    from PIL import Image
    from pegasus_amd import jpeg
    for sub in ("4:4:4", "4:2:0"):
        ours = jpeg.encode_batch_bytes(rgb[:4], 95, sub)
        theirs = [pil_bytes(a, 95, sub, optimize=True, restart_marker_blocks=jpeg.RESTART_MCUS) for a in host[:4]]
        doc[f"against_pil_{sub.replace(':', '')}"] = {
            "bytes": sum(map(len, ours)), "pil_bytes": sum(map(len, theirs)),
            "psnr_db": round(float(np.mean([psnr(np.asarray(Image.open(io.BytesIO(d))), a) for d, a in zip(ours, host)])), 3),
            "pil_psnr_db": round(float(np.mean([psnr(np.asarray(Image.open(io.BytesIO(d))), a) for d, a in zip(theirs, host)])), 3)}
    print(json.dumps(doc, indent=1), flush=True)
    del rgb, keep, host
    torch.cuda.empty_cache()

    big = photo_like(32, 3000, 4000)
    doc["photos_4000x3000_q95_420"] = jpeg_entry(big, 95, "4:2:0", max(2, args.repeats // 2))
    print(json.dumps(doc["photos_4000x3000_q95_420"]), flush=True)
    del big
    torch.cuda.empty_cache()

    if not args.skip_end_to_end:
        tmp = Path(tempfile.mkdtemp(prefix="jpeg_bench_"))
        try:
            for name, extra in (("generate_png", []), ("generate_rgb_jpg", ["--rgb", "jpg"])):
                cmd = [sys.executable, "-m", "pegasus_amd.generate", "--out", str(tmp / name), "--frames", "256", "--workload", "c3",
                       "--scale", "0.1", "--writers", "16", "--png", "gpu"] + extra
                t0 = time.perf_counter()
                done = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=600)
                doc[name] = {"wall_s": round(time.perf_counter() - t0, 2), "rc": done.returncode, "dataset_bytes": dir_bytes(tmp / name),
                             "rgb_bytes": dir_bytes(tmp / name / "train" / "000000" / "rgb"), "said": done.stdout.strip().splitlines()[-3:]}
                print(json.dumps(doc[name]), flush=True)
                shutil.rmtree(tmp / name, ignore_errors=True)
            # the undistort command line on 32 JPEG files of 4000 x 3000
            from pegasus_amd import colmap_io, undistort
            from pegasus_amd.colmap_io import ColmapCamera, ColmapImage
            W, H, N = 4000, 3000, 32
            cam = ColmapCamera(1, "OPENCV", W, H, np.array([3100.0, 3120.0, 2010.0, 1490.0, -0.12, 0.03, 0.0008, -0.0005]))
            (tmp / "input").mkdir()
            yy, xx = np.mgrid[0:H, 0:W]
            base = np.stack([(xx * 255 // W), (yy * 255 // H), ((xx + yy) * 255 // (W + H))], 2).astype(np.uint8)

            def write(i):
                a = base.copy()
                a[::8, ::8] = (37 * i) % 256
                Image.fromarray(a).save(tmp / "input" / f"img_{i:03d}.jpg", quality=90)
            with ThreadPoolExecutor(16) as pool:
                list(pool.map(write, range(N)))
            imgs = {i + 1: ColmapImage(i + 1, np.array([1.0, 0, 0, 0]), np.zeros(3), 1, f"img_{i:03d}.jpg", xys=np.zeros((0, 2)),
                                       point3D_ids=np.zeros(0, np.int64)) for i in range(N)}
            colmap_io.write_colmap_model(tmp / "distorted" / "sparse" / "0", {1: cam}, imgs, np.zeros((4, 3)), np.zeros((4, 3), np.uint8))
            undistort.undistort_project(tmp / "input", tmp / "distorted" / "sparse" / "0", tmp / "warm", jpeg="gpu", batch=8)
            shutil.rmtree(tmp / "warm", ignore_errors=True)
            for where in ("host", "gpu", "host", "gpu"):
                t0 = time.perf_counter()
                res = undistort.undistort_project(tmp / "input", tmp / "distorted" / "sparse" / "0", tmp / f"out_{where}", jpeg=where)
                doc.setdefault(f"undistort_jpeg_{where}", []).append(
                    {"wall_s": round(time.perf_counter() - t0, 3), "seconds": {k: round(v, 3) for k, v in res["seconds"].items()},
                     "image_bytes": dir_bytes(tmp / f"out_{where}" / "images")})
                shutil.rmtree(tmp / f"out_{where}", ignore_errors=True)
            print(json.dumps({k: v for k, v in doc.items() if k.startswith("undistort")}), flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(doc, indent=1)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
