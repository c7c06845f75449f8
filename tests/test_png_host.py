"""The host side of the PNG encoder (include/pegasus_raster.h "PNG files of device images"): the code builder that the
kernels run, on host arrays, and the argument checks of the entries.  No GPU: fake device pointers are never dereferenced."""
import ctypes as C
import heapq
from fractions import Fraction

import numpy as np
import pytest

import png_reference as PR


@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import _lib, build
    build.build()
    return _lib.lib()


def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def huffman_cost_and_depth(freq):
    """Cost and depth of an unlimited Huffman code of the non-zero counts (heapq; the tie-break does not change the cost)."""
    heap = [(f, i, 0) for i, f in enumerate(freq) if f]
    heapq.heapify(heap)
    cost, tick = 0, len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return cost, heap[0][2]


SPARSE = [0] * 286
for _s, _f in ((0, 4000), (255, 900), (256, 1), (257, 30), (285, 7), (100, 1), (17, 1)):
    SPARSE[_s] = _f

CODE_CASES = {
    "fibonacci 21, limit 15": (fibonacci(21), 15),
    "fibonacci 19, limit 7": (fibonacci(19), 7),
    "one used symbol": ([0] * 29 + [12], 15),
    "two used symbols": ([0, 5, 0, 0, 1000] + [0] * 14, 7),
    "all 286 equal": ([3] * 286, 15),
    "zero-frequency majority": (SPARSE, 15),
}


@pytest.mark.parametrize("name", list(CODE_CASES))
def test_code_lengths(name):
    from pegasus_amd import png
    freq, limit = CODE_CASES[name]
    lengths = png.code_lengths(freq, limit).tolist()
    used = [s for s, f in enumerate(freq) if f]
    assert all(1 <= lengths[s] <= limit for s in used), lengths
    assert all(lengths[s] == 0 for s in range(len(freq)) if s not in used)
    kraft = sum(Fraction(1, 2 ** lengths[s]) for s in used)
    if len(used) >= 2:
        assert kraft == 1, kraft
    else:
        assert [lengths[s] for s in used] == [1]
    cost = sum(freq[s] * lengths[s] for s in used)
    flat = max(1, (len(used) - 1).bit_length())                # ceil(log2(used)), one bit for a single symbol
    assert cost <= flat * sum(freq), (cost, flat * sum(freq))
    best, depth = huffman_cost_and_depth(freq)
    if depth <= limit and len(used) >= 2:
        assert cost == best                                    # nothing to limit: Huffman's own cost
    else:
        assert cost >= best


def test_the_fibonacci_cases_need_the_limit():
    """What the two cases are for: an unlimited code of 21 Fibonacci counts is 20 deep, of 19 counts 18 deep."""
    assert huffman_cost_and_depth(fibonacci(21))[1] == 20 and huffman_cost_and_depth(fibonacci(19))[1] == 18


def test_code_lengths_on_random_counts_are_complete_and_within_the_limit():
    from pegasus_amd import png
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(2, 287))
        limit = int(rng.choice([7, 9, 15]))
        if n > 2 ** limit:
            n = 2 ** limit
        freq = (rng.integers(0, 2, n) * rng.geometric(1.0 / rng.choice([2, 40, 3000]), n)).astype(np.uint32)
        lengths = png.code_lengths(freq, limit)
        used = np.flatnonzero(freq)
        assert not lengths[freq == 0].any() and (lengths[used] >= 1).all() and (lengths[used] <= limit).all()
        if len(used) >= 2:
            assert sum(Fraction(1, 2 ** int(l)) for l in lengths[used]) == 1
            best, depth = huffman_cost_and_depth(freq.tolist())
            cost = int((freq.astype(np.int64) * lengths).sum())
            assert cost == best if depth <= limit else cost >= best
            assert cost <= max(1, (len(used) - 1).bit_length()) * int(freq.sum())


def test_code_lengths_refuses_what_the_builder_does_not_take(lib):
    from pegasus_amd import _lib
    f = (C.c_uint32 * 300)(*([1] * 300))
    out = (C.c_uint8 * 300)()
    bad = _lib.PGR_ERR_INVALID_ARGUMENT
    assert lib.pgr_png_code_lengths(None, 4, 7, out) == bad and lib.pgr_png_code_lengths(f, 4, 7, None) == bad
    assert lib.pgr_png_code_lengths(f, 0, 7, out) == bad and lib.pgr_png_code_lengths(f, 289, 15, out) == bad
    assert lib.pgr_png_code_lengths(f, 4, 0, out) == bad and lib.pgr_png_code_lengths(f, 4, 16, out) == bad
    assert lib.pgr_png_code_lengths(f, 129, 7, out) == bad                     # more symbols than codes of 7 bits
    f[2] = (1 << 22) + 1
    assert lib.pgr_png_code_lengths(f, 4, 7, out) == bad
    f[2] = 1 << 22
    assert lib.pgr_png_code_lengths(f, 4, 7, out) == 0


def test_segment_size_is_the_headers(lib):
    from pegasus_amd import _lib
    S = PR.segment_bytes()
    assert S == _lib.PGR_PNG_SEGMENT_BYTES and 8192 <= S <= 32768 and S & (S - 1) == 0


def test_max_bytes_is_the_formula(lib):
    from pegasus_amd import png
    S = PR.segment_bytes()
    for kind in (PR.GRAY8, PR.RGB8, PR.GRAY16):
        for w, h in ((1, 1), (800, 800), (S - 1, 1), (S, 1), (S + 1, 3), (16384, 16384), (37, 5000)):
            raw = h * (1 + w * (1, 3, 2)[kind])
            assert png.max_bytes(w, h, kind) == 63 + raw + 5 * -(-raw // S) == PR.max_bytes(w, h, kind)
    for bad in ((0, 4, 0), (4, 0, 0), (16385, 4, 0), (4, 16385, 1), (4, 4, 3), (4, 4, -1)):
        assert png.max_bytes(*bad) == 0


def _job(_lib, **kw):
    fields = dict(pixels=0x1000, width=48, height=40, kind=0, row_stride=48, pixel_stride=1, scale=1)
    fields.update(kw)
    return _lib.PgrPngJob(**fields)


def test_workspace_query_refuses_what_is_outside_the_domain(lib):
    from pegasus_amd import _lib
    good = (_lib.PgrPngJob * 2)(_job(_lib), _job(_lib, kind=1, row_stride=144, pixel_stride=3))
    need = lib.pgr_png_workspace_bytes(2, good)
    S = PR.segment_bytes()
    assert need >= 40 * 49 + 40 * 145 and need >= 2 * S                        # a slot per segment, at least
    assert lib.pgr_png_workspace_bytes(0, good) == 0 and lib.pgr_png_workspace_bytes(-1, good) == 0
    assert lib.pgr_png_workspace_bytes(2, None) == 0
    for bad in (dict(width=0), dict(height=0), dict(width=16385, row_stride=16385), dict(height=16385), dict(kind=3),
                dict(kind=-1), dict(scale=0), dict(scale=2), dict(scale=254), dict(kind=2, row_stride=96, pixel_stride=2, scale=255),
                dict(pixel_stride=0), dict(row_stride=47), dict(kind=1, row_stride=144, pixel_stride=2)):
        assert lib.pgr_png_workspace_bytes(1, (_lib.PgrPngJob * 1)(_job(_lib, **bad))) == 0, bad
    for ok in (dict(scale=255), dict(width=16384, height=16384, row_stride=16384), dict(kind=2, row_stride=200, pixel_stride=4),
               dict(width=1, height=1, row_stride=1)):
        assert lib.pgr_png_workspace_bytes(1, (_lib.PgrPngJob * 1)(_job(_lib, **ok))) > 0, ok


def test_encode_and_emit_refuse_before_any_launch(lib):
    """Null tables, an unknown level, capacity < total, a total no batch of these jobs can have, a short or misaligned workspace:
    integer statuses from host-side checks, with fake device pointers and no device."""
    from pegasus_amd import _lib
    bad, small, fake = _lib.PGR_ERR_INVALID_ARGUMENT, _lib.PGR_ERR_WORKSPACE_TOO_SMALL, C.c_void_p(0x1000)
    jobs = (_lib.PgrPngJob * 2)(_job(_lib), _job(_lib, kind=2, row_stride=96, pixel_stride=2))
    need = lib.pgr_png_workspace_bytes(2, jobs)
    assert lib.pgr_png_encode(None, 2, 1, fake, fake, need, None) == bad
    assert lib.pgr_png_encode(jobs, -1, 1, fake, fake, need, None) == bad
    assert lib.pgr_png_encode(jobs, 2, 2, fake, fake, need, None) == bad and lib.pgr_png_encode(jobs, 2, -1, fake, fake, need, None) == bad
    assert lib.pgr_png_encode(jobs, 2, 1, None, fake, need, None) == bad
    assert lib.pgr_png_encode(jobs, 2, 1, fake, None, need, None) == bad
    assert lib.pgr_png_encode(jobs, 2, 1, fake, C.c_void_p(0x1008), need, None) == bad
    assert lib.pgr_png_encode(jobs, 2, 1, fake, fake, need - 1, None) == small
    no_pixels = (_lib.PgrPngJob * 2)(_job(_lib), _job(_lib, pixels=None))
    assert lib.pgr_png_encode(no_pixels, 2, 1, fake, fake, need, None) == bad
    assert lib.pgr_png_encode(jobs, 0, 1, None, None, 0, None) == 0                # nothing to do
    total = 2 * 63 + 200
    most = sum(PR.max_bytes(48, 40, k) for k in (0, 2))
    assert lib.pgr_png_emit(None, 2, fake, total, fake, total, fake, need, None) == bad
    assert lib.pgr_png_emit(jobs, 2, None, total, fake, total, fake, need, None) == bad
    assert lib.pgr_png_emit(jobs, 2, fake, total, None, total, fake, need, None) == bad
    assert lib.pgr_png_emit(jobs, 2, fake, total, fake, total, None, need, None) == bad
    assert lib.pgr_png_emit(jobs, 2, fake, total, fake, total - 1, fake, need, None) == bad          # capacity < total
    assert lib.pgr_png_emit(jobs, 2, fake, 2 * 63, fake, total, fake, need, None) == bad             # files without data
    assert lib.pgr_png_emit(jobs, 2, fake, most + 1, fake, most + 1, fake, need, None) == bad        # beyond the bound
    assert lib.pgr_png_emit(jobs, 2, fake, total, fake, total, fake, need - 1, None) == small
    assert lib.pgr_png_emit(jobs, 2, fake, most, fake, most, fake, need - 1, None) == small          # the bound itself passes the checks
    assert lib.pgr_png_emit(jobs, 0, None, 0, None, 0, None, 0, None) == 0


def test_python_entry_refuses_host_tensors_and_other_types():
    import torch
    from pegasus_amd import png
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.encode_batch([torch.zeros(4, 4, dtype=torch.uint8)])
    assert png.encode_batch([])[1].tolist() == [0]


def test_writer_and_cli_know_the_switch(tmp_path):
    from pegasus_amd import dataset_writer as DW
    with pytest.raises(ValueError, match="'host' or 'gpu'"):
        DW.BopSceneWriter(tmp_path / "ds", workers=1, encoder="cpu")
    assert DW.BopSceneWriter(tmp_path / "ds", workers=1).encoder == "host"
    from pegasus_amd import generate
    with pytest.raises(SystemExit):
        generate.main(["--out", str(tmp_path / "x"), "--png", "fpga"])
