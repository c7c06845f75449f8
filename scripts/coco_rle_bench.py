"""Times the mask run-length encoder against the path it replaces.

    python scripts/coco_rle_bench.py [--frames 32] [--objects 8] [--size 800] [--repeats 5]

Both paths start from the same uint8 masks on the device (what pgr_bop_gt_info or the compositor leave there):
  device   pegasus_amd.coco.rle_encode: both passes, the copy of n_counts between them, and the copy of the counts to the
           host (what an annotation needs), until everything has arrived
  host     the masks copied to the host, then a vectorised NumPy encoder per mask (column-major ravel, diff, flatnonzero)
Warm, the median of --repeats runs each; prints one JSON line.  The two results are compared for equality first."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def numpy_rle(mask):
    flat = (mask != 0).ravel(order="F")
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    if flat[0]:
        change = np.concatenate(([0], change))
    return np.diff(np.concatenate(([0], change, [flat.size])))


def object_masks(n, size, device, seed=3):
    """Filled ellipses, a few per mask: compact regions with curved borders, 3 to 30 % of the image each."""
    import torch
    g = torch.Generator().manual_seed(seed)
    ax = torch.arange(size, device=device, dtype=torch.float32)
    y, x = ax[:, None], ax[None, :]
    out = torch.zeros((n, size, size), dtype=torch.uint8, device=device)
    for k in range(n):
        for _ in range(3):
            cx, cy, rx, ry = (float(v) for v in torch.rand(4, generator=g))
            out[k] |= ((((x - cx * size) / (0.05 * size + 0.2 * rx * size)) ** 2 +
                        ((y - cy * size) / (0.05 * size + 0.2 * ry * size)) ** 2) <= 1.0).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    from pegasus_amd import coco
    n = a.frames * a.objects
    masks = object_masks(n, a.size, "cuda")
    torch.cuda.synchronize()

    def device_path():
        counts, offsets, stats = coco.rle_encode(masks)
        return counts.cpu().numpy(), offsets, stats.cpu().numpy()

    def host_path():
        host = masks.cpu().numpy()
        return [numpy_rle(m) for m in host]

    def timed(fn):
        fn()                                                       # warm
        times = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return out, times
    (counts, offsets, stats), t_dev = timed(device_path)
    per_mask, t_host = timed(host_path)
    assert all(np.array_equal(counts[offsets[k]:offsets[k + 1]], per_mask[k]) for k in range(n)), "the two encoders differ"
    # the kernels alone, by events
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernel_ms = []
    for _ in range(a.repeats):
        start.record()
        coco.rle_encode(masks)
        stop.record()
        stop.synchronize()
        kernel_ms.append(start.elapsed_time(stop))
    print(json.dumps({"masks": n, "size": a.size, "mask_bytes": int(masks.numel()), "counts": int(offsets[-1]),
                      "mean_area_fraction": float(stats[:, 1].mean() / (a.size * a.size)),
                      "device_encode_ms_median": 1e3 * statistics.median(t_dev), "device_encode_ms_all": [1e3 * t for t in t_dev],
                      "device_encode_events_ms_median": statistics.median(kernel_ms),
                      "host_copy_and_numpy_ms_median": 1e3 * statistics.median(t_host), "host_ms_all": [1e3 * t for t in t_host],
                      "repeats": a.repeats}))


if __name__ == "__main__":
    main()
