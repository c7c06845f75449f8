"""The device PNG encoder (pegasus_amd/csrc/png.hip.h) byte for byte against the restatement of its rule (tests/png_reference.py),
on the cases of tests/png_cases.py: the round-trip grid in its packed and strided placements, the cases that steer the matcher
(hash candidates from earlier sub-blocks only, runs around 258 and around the 16 positions of a thread, ties, the row above, a
hash collision, a length that must not be carried over a skipped distance), the zero runs of the dynamic header, and files of
more than 256 segments, where the finish kernel takes more than one pass.  tests/test_png_rule_host.py judges the restatement
alone and checks that the cases reach what they are meant to reach.  No case is exempt."""
import numpy as np
import pytest

import png_cases as PC
import png_reference as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_files(gpu_device):
    """{level: {name: file}}: every case of a level in ONE encode call."""
    from pegasus_amd import png
    cases = PC.all_cases()
    tensors = [PC.place(c.stored, c.placement, gpu_device) for c in cases]
    return {level: dict(zip((c.name for c in cases), png.encode_batch_bytes(tensors, level=level, scale=[c.scale for c in cases])))
            for level in (0, 1)}


def first_difference(a: bytes, b: bytes) -> int:
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


@pytest.mark.parametrize("group", ("grid", "matcher", "header"))
@pytest.mark.parametrize("level", (0, 1))
def test_bytes_equal_the_restatement(device_files, level, group):
    names = [c.name for c in {"grid": PC.grid_cases, "matcher": PC.matcher_cases, "header": PC.header_cases}[group]()]
    assert names and set(names) <= set(device_files[level])
    want = PC.reference(level)
    wrong = []
    for name in names:
        got, (ref, plans) = device_files[level][name], want[name]
        if got != ref:
            at = first_difference(got, ref)
            wrong.append((name, len(got), len(ref), "first difference at byte", at, "forms", [p["form"] for p in plans]))
    assert not wrong, f"{len(wrong)} of {len(names)} files differ: {wrong[:6]}"


def test_the_cases_are_placed_packed_cropped_and_pixel_strided():
    assert {c.placement for c in PC.grid_cases()} == {0, 1, 2}
    for kind in range(3):
        assert {c.placement for c in PC.grid_cases() if c.kind == kind and len(PC.reference(1)[c.name][1]) > 1} == {0, 1, 2}


def test_files_past_one_pass_of_the_finish_kernel(gpu_device):
    """256, 257 and 513 segments of gray8 and 264 of a 16-bit ramp, one batch at level 1: the size pgr_png_encode reports is the
    file's length, the strict reader (zlib's inflate and Adler check, the CRC of every chunk) gives back the input, the file
    keeps to its bound -- and it is the restatement's file byte for byte (the restatement takes 0.7 to 1.6 s a case)."""
    import torch
    from pegasus_amd import _lib, bop_dataset as BD, png
    cases = PC.big_cases()
    segments = [-(-PR.raw_bytes(c.stored.shape[1], c.stored.shape[0], c.kind) // PC.S) for c in cases]
    if PC.S == 8192:
        assert segments == [256, 257, 513, 264]
    assert segments[0] == 256 and segments[1] == 257 and segments[2] == 513 and segments[3] > 256
    tensors = [PC.place(c.stored, 0, gpu_device) for c in cases]
    files, offsets = png.encode_batch(tensors, level=1)
    n = len(cases)
    jobs = (_lib.PgrPngJob * n)(*[png._job(t, 1) for t in tensors])
    ws = _lib.workspace("pgr_png", gpu_device, n, jobs)
    sizes = torch.empty(n, dtype=torch.int64, device=gpu_device)
    _lib.call("pgr_png_encode", gpu_device, jobs, n, 1, _lib.ptr(sizes), _lib.ptr(ws), ws.numel())
    assert sizes.cpu().tolist() == np.diff(offsets).tolist() and offsets[-1] == len(files)
    want = PC.big_reference()
    for k, c in enumerate(cases):
        data = files[offsets[k]:offsets[k + 1]].tobytes()
        h, w = c.stored.shape[:2]
        print(c.name, segments[k], "segments,", len(data), "bytes of", PR.max_bytes(w, h, c.kind))
        assert len(data) <= PR.max_bytes(w, h, c.kind)
        got = PR.read_png(data)
        assert got.dtype == c.expected.dtype
        np.testing.assert_array_equal(got, c.expected)
        np.testing.assert_array_equal(BD.decode_png(data), c.expected)
        assert len(data) == len(want[c.name]), (c.name, len(data), len(want[c.name]))
        assert data == want[c.name], (c.name, "first difference at byte", first_difference(data, want[c.name]))
