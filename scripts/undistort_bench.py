"""The measurements of DESIGN.md section 26 on one device: the remap of 32 RGB images of 4000 x 3000 (OPENCV, the pinhole
kernel, the fisheye), a plain copy of the same bytes, the box pyramid, 1e6 observations through pgr_undistort_points, the NumPy
reference on one image, and the command line on 32 JPEG files with its decode / device / encode split.

    python scripts/undistort_bench.py [--out profiles/undistort_bench.json]
"""
import argparse
import json
import shutil
import sys
import tempfile
import time
from pathlib import Path
from concurrent.futures import ThreadPoolExecutor
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch
import undistort_reference as ref
from pegasus_amd import undistort, colmap_io
from pegasus_amd.colmap_io import ColmapCamera, ColmapImage

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "undistort_bench.json"))
args = ap.parse_args()
out = {}
W, H, N = 4000, 3000, 32
cam = ColmapCamera(1, "OPENCV", W, H, np.array([3100.0, 3120.0, 2010.0, 1490.0, -0.12, 0.03, 0.0008, -0.0005]))
t0 = time.perf_counter()
ocam = undistort.undistort_camera(cam)
torch.cuda.synchronize()
out["camera"] = dict(width=ocam.width, height=ocam.height, params=ocam.params.tolist(), seconds_first_call=time.perf_counter() - t0)
print(out["camera"], flush=True)
g = torch.Generator(device="cuda"); g.manual_seed(1)
srcs = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(N)]
dsts = [torch.empty((ocam.height, ocam.width, 3), dtype=torch.uint8, device="cuda") for _ in range(N)]
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)
ts = timed(lambda: undistort.undistort_images(srcs, cam, ocam, out=dsts))
moved = N * (H * W * 3 + ocam.height * ocam.width * 3)
out["remap_opencv_rgb"] = dict(ms=ts, median_ms=ts[len(ts) // 2], bytes=moved, gb_per_s=moved / (ts[len(ts) // 2] * 1e-3) / 1e9,
                               mpix_per_s=N * ocam.height * ocam.width / (ts[len(ts) // 2] * 1e-3) / 1e6)
print(out["remap_opencv_rgb"], flush=True)
# the same images through the pinhole kernel (no distortion arithmetic) and as gray: what the arithmetic costs
pin = ColmapCamera(1, "PINHOLE", W, H, np.array([3100.0, 3120.0, 2010.0, 1490.0]))
ts = timed(lambda: undistort.undistort_images(srcs, pin, ocam, out=dsts))
out["remap_pinhole_rgb"] = dict(ms=ts, median_ms=ts[len(ts) // 2], gb_per_s=moved / (ts[len(ts) // 2] * 1e-3) / 1e9)
print(out["remap_pinhole_rgb"], flush=True)
fish = ColmapCamera(1, "OPENCV_FISHEYE", W, H, np.array([3100.0, 3120.0, 2010.0, 1490.0, -0.02, 0.004, 0.0, 0.0]))
ts = timed(lambda: undistort.undistort_images(srcs, fish, ocam, out=dsts), reps=3)
out["remap_fisheye_rgb"] = dict(ms=ts, median_ms=ts[len(ts) // 2])
print(out["remap_fisheye_rgb"], flush=True)
# a plain device copy of the same bytes: the memory bound
flat_s, flat_d = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
ts = timed(lambda: flat_d.copy_(flat_s))
out["copy_same_bytes"] = dict(median_ms=ts[len(ts) // 2], gb_per_s=moved / (ts[len(ts) // 2] * 1e-3) / 1e9)
print(out["copy_same_bytes"], flush=True)
del flat_s, flat_d
for f in (2, 4, 8):
    ts = timed(lambda: undistort.box_downscale(dsts, f), reps=3)
    out[f"box_{f}"] = dict(median_ms=ts[len(ts) // 2])
print({k: v for k, v in out.items() if k.startswith("box")}, flush=True)
# observations
rng = np.random.default_rng(0)
pts = torch.from_numpy(rng.uniform([0, 0], [W, H], (1_000_000, 2))).cuda()
ts = timed(lambda: undistort.undistort_points(cam, pts))
uv, ok = undistort.undistort_points(cam, pts)
out["points_1e6"] = dict(ms=ts, median_ms=ts[len(ts) // 2], ok=int(ok.sum()))
print(out["points_1e6"], flush=True)
# the numpy reference on one image
one = srcs[0].cpu().numpy()
t0 = time.perf_counter()
want = ref.remap(one, cam.model, cam.params, ocam.params, ocam.width, ocam.height)
out["numpy_reference_one_image_s"] = time.perf_counter() - t0
got = dsts[0]
undistort.undistort_images(srcs[:1], cam, ocam, out=[got])
out["full_size_equal"] = bool((got.cpu().numpy() == want).all())
print(out["numpy_reference_one_image_s"], out["full_size_equal"], flush=True)
del srcs, dsts, want
torch.cuda.empty_cache()
# the CLI on 32 JPEG images
tmp = Path(tempfile.mkdtemp(prefix="und_"))
try:
    from PIL import Image
    (tmp / "input").mkdir()
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 255 // W), (yy * 255 // H), ((xx + yy) * 255 // (W + H))], 2).astype(np.uint8)
    def write(i):
        a = base.copy(); a[::8, ::8] = (37 * i) % 256
        Image.fromarray(a).save(tmp / "input" / f"img_{i:03d}.jpg", quality=90)
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(write, range(N)))
    imgs = {i + 1: ColmapImage(i + 1, np.array([1.0, 0, 0, 0]), np.zeros(3), 1, f"img_{i:03d}.jpg",
                               xys=rng.uniform([0, 0], [W, H], (30000, 2)), point3D_ids=np.arange(30000, dtype=np.int64)) for i in range(N)}
    colmap_io.write_colmap_model(tmp / "distorted" / "sparse" / "0", {1: cam}, imgs, np.zeros((4, 3)), np.zeros((4, 3), np.uint8))
    t0 = time.perf_counter()
    rc = undistort.main(["-s", str(tmp)])
    out["cli_jpeg"] = dict(wall_s=time.perf_counter() - t0, rc=rc)
    res = undistort.undistort_project(tmp / "input", tmp / "distorted" / "sparse" / "0", tmp / "again")
    out["cli_jpeg"]["seconds"] = res["seconds"]
    print(out["cli_jpeg"], flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
print("wrote", args.out)
