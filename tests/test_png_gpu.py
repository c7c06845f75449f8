"""The device PNG encoder (pegasus_amd/png.py, csrc/png.hip.h) where it runs: every file is read back by the strict reader
of tests/png_reference.py (chunk CRCs by zlib.crc32, one IDAT, zlib's own inflate and Adler check, filter 0) and by
bop_dataset.decode_png, and must be the input exactly.  Shapes are built from S = PGR_PNG_SEGMENT_BYTES as the header exports
it: around one segment, across a segment edge, three segments.  The bounds are those of the rule of the file (no file above
63 + raw + 5 per segment) and two that follow from fixed-Huffman costs (a literal is at most 9 bits, a distance-1 match at
most 18), so they hold whichever of the three block forms the encoder picks."""
import ctypes as C
import heapq

import numpy as np
import pytest

import png_cases as PC
import png_reference as PR

pytestmark = pytest.mark.gpu

S, BPP, KIND_NAMES = PC.S, PC.BPP, PC.KIND_NAMES
shape_with_raw, sizes_of, ellipse, contents_of, place = PC.shape_with_raw, PC.sizes_of, PC.ellipse, PC.contents_of, PC.place


def check_file(data, expected, kind):
    from pegasus_amd import bop_dataset as BD
    data = bytes(data)
    h, w = expected.shape[:2]
    assert len(data) <= PR.max_bytes(w, h, kind), (len(data), PR.max_bytes(w, h, kind))
    got = PR.read_png(data)
    assert got.dtype == expected.dtype and got.shape == expected.shape
    np.testing.assert_array_equal(got, expected)
    np.testing.assert_array_equal(BD.decode_png(data), expected)


@pytest.fixture(scope="module")
def round_trip(gpu_device):
    """Everything of the round-trip grid in ONE encode call per level: {level: {(kind, size, content): (file, expected)}}."""
    from pegasus_amd import png
    rng = np.random.default_rng(5)
    cases = []
    for kind in range(3):
        for size, (w, h) in sizes_of(kind).items():
            for content, (stored, scale, expected) in contents_of(kind, w, h, rng).items():
                cases.append(((kind, size, content), stored, scale, expected))
    out = {}
    for level in (0, 1):
        tensors = [place(stored, i % 3, gpu_device) for i, (_, stored, _, _) in enumerate(cases)]
        files = png.encode_batch_bytes(tensors, level=level, scale=[c[2] for c in cases])
        out[level] = {c[0]: (f, c[3]) for c, f in zip(cases, files)}
    return out


@pytest.mark.parametrize("kind", range(3), ids=KIND_NAMES)
@pytest.mark.parametrize("level", (0, 1))
def test_round_trip(round_trip, level, kind):
    mine = {k: v for k, v in round_trip[level].items() if k[0] == kind}
    sizes = {k[1] for k in mine}
    assert {"1x1", "row", "column", "S-1", "S+1", "straddle", "3 segments"} <= sizes and (("S" in sizes) == (kind != PR.GRAY16))
    assert {k[2] for k in mine} >= {"zero", "all ones", "random", ("ellipse mask", "semantic", "depth ramp")[kind]}
    for key, (data, expected) in mine.items():
        print(level, KIND_NAMES[kind], key[1:], expected.shape, len(data), "of", PR.max_bytes(*expected.shape[1::-1], kind))
        check_file(data, expected, kind)


@pytest.mark.parametrize("level", (0, 1))
def test_random_bytes_come_out_as_stored_blocks(round_trip, level):
    """Nothing to gain in uniform random bytes: a segment of them is a stored block, its raw bytes + 5 (a Huffman block is only
    taken when it is smaller), so the file is exactly at its bound and holds the raw stream verbatim.  Asked where the raw
    stream IS random: rows of 64 bytes or more (a column's raw stream is half filter bytes) and, for the exact size, a last
    segment of 64 bytes or more (a last segment of one byte is cheaper under the fixed code)."""
    seen = 0
    for (kind, size, content), (data, expected) in round_trip[level].items():
        h, w = expected.shape[:2]
        raw = PR.raw_bytes(w, h, kind)
        if content != "random" or w * BPP[kind] < 64:
            continue
        seen += 1
        n_segments = -(-raw // S)
        first = min(raw, S)
        rows = (expected.astype(">u2").view(np.uint8) if kind == PR.GRAY16 else expected).reshape(h, -1)
        stream = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()
        head = bytes([1 if n_segments == 1 else 0, first & 255, first >> 8, ~first & 255, (~first >> 8) & 255])
        assert bytes(data)[43:43 + 5 + first] == head + stream[:first], (KIND_NAMES[kind], size)
        if raw - (n_segments - 1) * S >= 64:
            assert len(data) == PR.max_bytes(w, h, kind), (KIND_NAMES[kind], size, len(data))
    assert seen >= 12


def test_uniform_images_take_a_sixteenth_of_a_byte_per_raw_byte(round_trip):
    """An all-equal segment is a literal and distance-1 matches of 258 bytes, at most 18 bits each under the fixed code: at
    most S / 128 bytes with the block's header, end and the join.  (The first byte of a row is the filter's 0: with a
    sample of 255 the rows are matched from the row above.)"""
    for (kind, size, content), (data, expected) in round_trip[1].items():
        if content in ("zero", "all ones"):
            h, w = expected.shape[:2]
            n_segments = -(-PR.raw_bytes(w, h, kind) // S)
            assert len(data) <= 63 + n_segments * S // 128, (KIND_NAMES[kind], size, content, len(data))


def test_ellipse_mask_of_200_by_400_takes_an_eighth_at_most(gpu_device):
    """400 rows of 201 bytes with at most 4 runs each: 4 literals and 4 distance-1 matches are at most 108 bits a row under the
    fixed code, raw / 8 leaves a margin of 1.8 (zlib level 1 takes 2153 bytes of the 80400)."""
    import torch
    from pegasus_amd import png
    mask = ellipse(400, 200)
    assert max(int((np.diff(np.concatenate([[0], row])) != 0).sum()) + 1 for row in mask) <= 4
    data, = png.encode_batch_bytes([torch.from_numpy(mask).to(gpu_device)], level=1, scale=255)
    print("ellipse 200 x 400:", len(data), "bytes of", 400 * 201)
    check_file(data, mask * np.uint8(255), PR.GRAY8)
    assert len(data) <= 400 * 201 // 8


def fibonacci_image(first: int):
    """gray8, one row, one segment: value 0 only in the filter byte, the other values' counts the Fibonacci numbers from
    F(first) on (F(2) = 1, F(3) = 2), as many as fit S, shuffled.  With the filter byte's 0 (one row: F(1) of them) and the
    end-of-block symbol the counts of a literal-only block are 1, 1, F(first), F(first + 1), ..."""
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    counts = []
    for f in fib[first - 1:]:
        if 1 + sum(counts) + f > S:
            break
        counts.append(f)
    values = np.repeat(np.arange(1, len(counts) + 1, dtype=np.uint8) * 9, counts)
    np.random.default_rng(11).shuffle(values)
    return values.reshape(1, -1), counts


def shallowest_huffman_depth(counts):
    """Depth of a Huffman code of ``counts`` when every tie goes to the shallower subtree: no tie-break gives a shallower one
    for the Fibonacci-like counts here, whose only ties are between a leaf and a subtree of the same weight."""
    heap = [(f, 0) for f in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


@pytest.mark.parametrize("first", (2, 3), ids=("counts 1 1 1 2 3 5", "counts 1 1 2 3 5"))
def test_code_limiting_on_the_device(gpu_device, first):
    """Level 0 codes literals only, so the block's histogram IS the counts.  first = 2 is the case this test was first specified with (17
    values for S = 8192, 20 values and 28 655 bytes for S = 32768): with the three counts of 1 (one value, the filter byte,
    the end of block) a Huffman code of them may tie its way to half the depth of the chain, so whether the limit bites
    depends on the builder's tie-break.  first = 3 leaves 1, 1, 2, 3, 5, ...: the sum of all counts in front of F(k) is
    F(k + 1) - 1 < F(k + 1), every merge takes the accumulated subtree and the next leaf whatever the tie-break, and the
    unlimited code is one bit short of the number of symbols deep -- deeper than 15.  That file inflates only if the builder
    limited the lengths on the device and kept the code complete."""
    import torch
    from pegasus_amd import png
    image, counts = fibonacci_image(first)
    h, w = image.shape
    raw = h * (1 + w)
    assert raw <= S and (first, len(counts)) in {8192: ((2, 17), (3, 16)), 16384: ((2, 18), (3, 17)), 32768: ((2, 20), (3, 19))}[S]
    depth = shallowest_huffman_depth(counts + [h, 1])
    data, = png.encode_batch_bytes([torch.from_numpy(image).to(gpu_device)], level=0)
    print("fibonacci from F(%d):" % first, len(counts), "values,", raw, "raw bytes, shallowest unlimited code", depth, "deep, file", len(data))
    if first == 3:
        assert depth == len(counts) + 1 > 15
    check_file(data, image, PR.GRAY8)
    assert len(data) < 63 + raw + 5                                              # smaller than the stored form
    assert len(data) < 63 + raw // 2                                             # Fibonacci counts: under 4 bits a symbol


def batch_of_forty(device):
    import torch
    rng = np.random.default_rng(3)
    arrays, tensors, scales = [], [], []
    shared = torch.from_numpy(rng.integers(0, 4, (90, 120), dtype=np.uint8) * 60).to(device)
    for k in range(40):
        kind = k % 3
        w, h = int(rng.integers(1, 180)), int(rng.integers(1, 140))
        if k == 7:
            w, h = 100, -(-(2 * S + 1) // 101)
        content = contents_of(kind, w, h, rng)
        name = sorted(content)[k % len(content)]
        stored, scale, expected = content[name]
        if k in (11, 12):                                                      # two views into one tensor
            view = shared[5:75, 10:90] if k == 11 else shared[40:90:1, 0:120:2]
            tensors.append(view); scales.append(1); arrays.append((view.cpu().numpy(), PR.GRAY8))
            continue
        tensors.append(place(stored, k % 3, device)); scales.append(scale); arrays.append((expected, kind))
    return tensors, scales, arrays


def test_one_batch_of_forty_jobs(gpu_device):
    import torch
    from pegasus_amd import _lib, png
    tensors, scales, arrays = batch_of_forty(gpu_device)
    files, offsets = png.encode_batch(tensors, level=1, scale=scales)
    assert offsets[0] == 0 and offsets[-1] == len(files) and files.dtype == np.uint8
    for k, (expected, kind) in enumerate(arrays):
        check_file(files[offsets[k]:offsets[k + 1]], expected, kind)             # gap-free: every slice is one whole file
    again, offsets2 = png.encode_batch(tensors, level=1, scale=scales)
    assert np.array_equal(offsets, offsets2) and np.array_equal(files, again)
    # the two passes by hand, into a buffer with 64 guard bytes in front and behind
    n = len(tensors)
    jobs = (_lib.PgrPngJob * n)(*[png._job(t, s) for t, s in zip(tensors, scales)])
    ws = _lib.workspace("pgr_png", gpu_device, n, jobs)
    sizes = torch.empty(n, dtype=torch.int64, device=gpu_device)
    _lib.call("pgr_png_encode", gpu_device, jobs, n, 1, _lib.ptr(sizes), _lib.ptr(ws), ws.numel())
    assert sizes.cpu().tolist() == np.diff(offsets).tolist()
    total = int(offsets[-1])
    guarded = torch.full((total + 128,), 0xA5, dtype=torch.uint8, device=gpu_device)
    off_dev = torch.from_numpy(offsets).to(gpu_device)
    _lib.call("pgr_png_emit", gpu_device, jobs, n, _lib.ptr(off_dev), total, C.c_void_p(guarded.data_ptr() + 64), total,
              _lib.ptr(ws), ws.numel())
    host = guarded.cpu().numpy()
    assert (host[:64] == 0xA5).all() and (host[-64:] == 0xA5).all()
    assert np.array_equal(host[64:-64], files)


def test_emit_keeps_inside_the_files_whatever_the_offsets_hold(gpu_device):
    """Device-side offsets that lie: negative, descending, beyond total.  Nothing outside [offsets[k], min(offsets[k+1], total))
    is stored: the guards and every byte no file may own stay as they were."""
    import torch
    from pegasus_amd import _lib, png
    images = [torch.from_numpy(ellipse(60, 70)).to(gpu_device) for _ in range(3)]
    n = len(images)
    jobs = (_lib.PgrPngJob * n)(*[png._job(t, 255) for t in images])
    ws = _lib.workspace("pgr_png", gpu_device, n, jobs)
    sizes = torch.empty(n, dtype=torch.int64, device=gpu_device)
    _lib.call("pgr_png_encode", gpu_device, jobs, n, 1, _lib.ptr(sizes), _lib.ptr(ws), ws.numel())
    size = int(sizes[0])
    total = 3 * size
    # file 0: a negative start; file 1: room for 10 bytes; file 2: cut at total, 10 bytes short
    lies = torch.tensor([-5, 2 * size, 2 * size + 10, 1 << 40], dtype=torch.int64, device=gpu_device)
    guarded = torch.full((total + 128,), 0xA5, dtype=torch.uint8, device=gpu_device)
    _lib.call("pgr_png_emit", gpu_device, jobs, n, _lib.ptr(lies), total, C.c_void_p(guarded.data_ptr() + 64), total, _lib.ptr(ws),
              ws.numel())
    host = guarded.cpu().numpy()
    assert (host[:64 + 2 * size] == 0xA5).all() and (host[-64:] == 0xA5).all()
    good = png.encode_batch_bytes(images[:1], level=1, scale=255)[0]
    assert len(good) == size
    assert bytes(host[64 + 2 * size:64 + 2 * size + 10]) == good[:10]
    assert bytes(host[64 + 2 * size + 10:64 + total]) == good[:size - 10]


def test_writer_gpu_and_host_write_the_same_dataset(tmp_path, gpu_device):
    import torch
    from pegasus_amd import bop_dataset as BD, dataset_writer as DW, masks as M
    B, K, H, W = 2, 2, 40, 48
    rng = np.random.default_rng(21)
    color = rng.random((B, 3, H, W), dtype=np.float32)
    depth = rng.uniform(0.3, 5.0, (B, 1, H, W)).astype(np.float32)
    seg = np.zeros((B, 3, H, W), np.float32)
    sil = np.zeros((B, K, H, W), np.uint8)
    sil[:, 0, 0:20, 10:30] = 1
    sil[:, 1, 12:33, 25:46] = 1
    vis = sil.copy()
    vis[:, 1, 12:20, 25:30] = 0
    seg[:, 0][vis[:, 0] > 0] = 0.84
    seg[:, 1][vis[:, 1] > 0] = 0.36
    gt = {str(i): [{"cam_R_m2c": np.eye(3).reshape(-1).tolist(), "cam_t_m2c": [0.0, 0.0, 1.0 + i], "obj_id": k + 3} for k in range(K)]
          for i in range(B)}
    cam = {str(i): {"cam_K": [100.0, 0, 24.0, 0, 100.0, 20.0, 0, 0, 1.0], "depth_scale": 1.0} for i in range(B)}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    images = dict(color=dev(color), depth=dev(depth), masks=dev(vis), seg=dev(seg))
    records = dict(records=M.pack_records(images["color"], images["depth"], images["masks"]), seg=images["seg"])
    scenes = {}
    for source, frames in (("images", images), ("records", records)):
        for encoder in ("gpu", "host"):
            w = DW.BopSceneWriter(tmp_path / f"{source}_{encoder}" / "ds", workers=2, encoder=encoder)
            # (without coco=: scene_gt_coco.json carries the time it was written)
            w.add_batch(frames, gt, cam, n=B, silhouettes=dev(sil), record_shape=(H, W, K))
            scenes[source, encoder] = w.close()
    for source in ("images", "records"):
        a, b = scenes[source, "gpu"], scenes[source, "host"]
        listing = sorted(p.relative_to(a).as_posix() for p in a.rglob("*") if p.is_file())
        assert listing == sorted(p.relative_to(b).as_posix() for p in b.rglob("*") if p.is_file())
        pngs = [p for p in listing if p.endswith(".png")]
        assert len(pngs) == B * (3 + 2 * K) and {p.split("/")[0] for p in pngs} == {"rgb", "depth", "mask", "mask_visib", "sem_mask"}
        for rel in listing:
            if rel.endswith(".png"):
                data = (a / rel).read_bytes()
                np.testing.assert_array_equal(PR.read_png(data), BD.decode_png((b / rel).read_bytes()), err_msg=rel)
                np.testing.assert_array_equal(BD.decode_png(data), BD.decode_png((b / rel).read_bytes()), err_msg=rel)
            else:
                assert (a / rel).read_bytes() == (b / rel).read_bytes(), rel
        assert {"scene_gt.json", "scene_camera.json", "scene_gt_info.json"} <= set(listing)
    # and the records path wrote what the image path wrote
    for rel in sorted(p.relative_to(scenes["images", "gpu"]).as_posix() for p in scenes["images", "gpu"].rglob("*.png")):
        np.testing.assert_array_equal(BD.decode_png((scenes["images", "gpu"] / rel).read_bytes()),
                                      BD.decode_png((scenes["records", "gpu"] / rel).read_bytes()), err_msg=rel)
