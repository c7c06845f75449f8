"""What the PNG tests share: the shapes and contents of the round-trip grid, the cases that pin the encoder's bytes against the
restatement of its rule (tests/png_reference.py) and the limit against zlib.

The limit was measured on the RESTATEMENT, never on the encoder, with

    python tests/png_cases.py

which prints, over ZLIB_CASES (an ellipse mask, a semantic palette image, a 16-bit depth ramp and a rendered-like RGB image at
2 to 3 segments each), the largest ratio of the restatement's IDAT payload to ``zlib.compress(raw, 1)`` of the same raw
stream.  Recorded with its excess over 1 doubled:

    measured: ratio 1.090 (the depth ramp; mask 0.852, semantic 0.718, rendered-like 1.004)   ->   ZLIB_RATIO = 1.180
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import png_reference as PR

S = PR.segment_bytes()
SUB = PR.subblock()
BPP = (1, 3, 2)
KIND_NAMES = ("gray8", "rgb8", "gray16")
ZLIB_RATIO = 1.180
OTHER_BYTES = 57                       # of a file, outside the IDAT's payload: signature 8, IHDR 25, IDAT 12, IEND 12

# stored: the array as the encoder is given it; expected: the array the file must hold; placement: how tests put it on the
# device (place() of this module: 0 packed, 1 a crop, 2 pixel-strided)
Case = namedtuple("Case", "name stored kind scale expected placement")


# ---- the round-trip grid ---------------------------------------------------------------------------------------------------
def shape_with_raw(target: int, kind: int):
    """(W, H) whose raw stream, H rows of 1 + W * bpp bytes, has exactly ``target`` bytes; None when no shape has."""
    bpp = BPP[kind]
    for h in range(1, target + 1):
        if target % h == 0 and (target // h - 1) >= bpp and (target // h - 1) % bpp == 0:
            return (target // h - 1) // bpp, h
    return None


def sizes_of(kind: int):
    """name -> (W, H): 1 x 1, one row, one column, a raw stream of S - 1, S, S + 1 bytes where the kind's row length allows
    it (a 16-bit row has an odd length, so no 16-bit image has a power of two of raw bytes), a row across a segment edge,
    three segments."""
    bpp = BPP[kind]
    out = {"1x1": (1, 1), "row": (37, 1), "column": (1, 53)}
    for name, target in (("S-1", S - 1), ("S", S), ("S+1", S + 1)):
        shape = shape_with_raw(target, kind)
        if shape is not None:
            out[name] = shape
    w = (S // 3 - 50) // bpp                                   # row 3 starts in front of byte S and ends behind it
    assert 3 * (1 + w * bpp) < S < 4 * (1 + w * bpp)
    out["straddle"] = (w, 7)
    out["3 segments"] = (100, -(-(2 * S + 1) // (1 + 100 * bpp)))
    assert 2 * S < PR.raw_bytes(*out["3 segments"], kind) <= 3 * S
    return out


def ellipse(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return ((((x - (w - 1) / 2) / max(w * 0.37, 0.6)) ** 2 + ((y - (h - 1) / 2) / max(h * 0.41, 0.6)) ** 2) <= 1).astype(np.uint8)


def depth_ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return (700.0 + 3.25 * x + 11.5 * y + 40.0 * np.sin(x / 9.0)).astype(np.uint16)             # millimetres of a tilted plane


def semantic(h, w):
    y, x = np.mgrid[0:h, 0:w]
    palette = np.array([[0, 0, 0], [214, 92, 92], [92, 214, 133], [92, 133, 214]], np.uint8)
    return palette[((x // 11 + y // 5) % 4) * (ellipse(h, w) > 0)]


def contents_of(kind: int, w: int, h: int, rng):
    """name -> (array as stored, scale, array the file must hold)."""
    dtype = np.uint16 if kind == PR.GRAY16 else np.uint8
    shape = (h, w, 3) if kind == PR.RGB8 else (h, w)
    top = np.iinfo(dtype).max
    out = {"zero": np.zeros(shape, dtype), "all ones": np.full(shape, top, dtype),
           "random": rng.integers(0, int(top) + 1, shape, dtype=dtype)}
    out = {k: (v, 1, v) for k, v in out.items()}
    if kind == PR.GRAY8:
        m = ellipse(h, w)
        out["ellipse mask"] = (m, 255, m * np.uint8(255))
    if kind == PR.GRAY16:
        ramp = depth_ramp(h, w)
        out["depth ramp"] = (ramp, 1, ramp)
    if kind == PR.RGB8:
        sem = semantic(h, w)
        out["semantic"] = (sem, 1, sem)
    return out


def place(array, mode: int, device):
    """The array on the device: packed (0), as a crop of a wider tensor (1: the row stride differs), or with a pixel stride of
    its own (2: every other gray sample, the first three of four channels)."""
    import torch
    a = np.ascontiguousarray(array)
    store = a.view(np.int16) if a.dtype == np.uint16 else a                    # int16 storage of uint16, as pack_frames has it
    t = torch.from_numpy(store.copy())
    if mode == 1:
        wide = torch.full((t.shape[0], t.shape[1] + 5) + tuple(t.shape[2:]), 77, dtype=t.dtype)
        wide[:, 2:2 + t.shape[1]] = t
        return wide.to(device)[:, 2:2 + t.shape[1]]
    if mode == 2 and t.dim() == 2:
        wide = torch.full((t.shape[0], t.shape[1], 2), 77, dtype=t.dtype)
        wide[:, :, 1] = t
        return wide.to(device)[:, :, 1]
    if mode == 2:
        wide = torch.full((t.shape[0], t.shape[1], 4), 77, dtype=t.dtype)
        wide[:, :, 1:] = t
        return wide.to(device)[:, :, 1:]
    return t.to(device)


def grid_cases():
    """The sizes_of x contents_of grid of tests/test_png_gpu.py, with its placements."""
    rng = np.random.default_rng(5)
    out = []
    for kind in range(3):
        for size, (w, h) in sizes_of(kind).items():
            for content, (stored, scale, expected) in contents_of(kind, w, h, rng).items():
                out.append(Case(f"grid {KIND_NAMES[kind]} {size} {content}", stored, kind, scale, expected, len(out) % 3))
    return out


# ---- the matcher ---------------------------------------------------------------------------------------------------------------
# One row of gray8 puts byte i of the row at position i + 1 of the raw stream (position 0 is the filter byte), and its row
# distance is never a candidate.  Filler bytes are below 64 -- three of them rarely repeat, and their code is short enough for
# a Huffman form to win, so a match the encoder finds or misses changes the file -- phrases and runs are above.
def _filler(rng, n):
    return rng.integers(0, 64, n, dtype=np.uint8)


def _one_row(name, raw_tail):
    a = np.asarray(raw_tail, np.uint8).reshape(1, -1)
    return Case(name, a, PR.GRAY8, 1, a, 0)


def _phrases(period, first, seed):
    rng = np.random.default_rng(seed)
    raw = np.concatenate([[0], _filler(rng, S - 1)]).astype(np.uint8)
    phrase = rng.integers(64, 256, 40, dtype=np.uint8)
    for at in range(first, S - 40, period):
        raw[at:at + 40] = phrase
    return raw[1:]


def _runs():
    """Runs of 257, 258, 259, 260 and 600 equal bytes starting at positions = 14, 15, 0 and 1 mod 16 (so their distance-1
    matches start at 15, 0, 1 and 2), three or more filler bytes between them."""
    rng = np.random.default_rng(31)
    raw = [0]
    for i, (length, residue) in enumerate((l, r) for l in (257, 258, 259, 260, 600) for r in (14, 15, 0, 1)):
        gap = 3 + (residue - (len(raw) + 3)) % 16
        raw += _filler(rng, gap).tolist() + [200 + i] * length
        assert (len(raw) - length) % 16 == residue
    raw += _filler(rng, 5).tolist()
    assert len(raw) <= S
    return raw[1:]


def hash_collision():
    """Two three-byte strings that differ in every byte and fall into one hash bucket: the first two of 400 random ones."""
    strings = np.random.default_rng(9).integers(64, 256, (400, 3), dtype=np.uint8)
    bucket = [int(PR.hash_of(s)[0]) for s in strings]
    for i, h in enumerate(bucket):
        for j in range(i):
            if bucket[j] == h and (strings[j] != strings[i]).all():
                return strings[j], strings[i]
    raise AssertionError("no collision")


def _collision():
    """X at position 300; Y, which collides with X, twice six bytes apart at 594 and 600 (distance 6 wins at 600, where X is
    the candidate and agrees in no byte) and alone at 700 (X is the candidate again: a literal).  The filler's seed is the
    first that leaves X the highest position of its bucket in the first sub-block."""
    x, y = hash_collision()
    for seed in range(100):
        rng = np.random.default_rng(seed)
        raw = np.concatenate([[0], _filler(rng, 1023)]).astype(np.uint8)
        six = np.concatenate([y, rng.integers(64, 256, 3, dtype=np.uint8)])
        raw[300:303] = x
        raw[594:600] = six
        raw[600:606] = six
        raw[700:703] = y
        cand = PR.candidates(raw)
        if cand[600] == 300 and cand[700] == 300:
            return raw[1:]
    raise AssertionError("no seed")


def _stale_carry():
    """Three rows of 561 bytes.  Row 1 is row 0 but for one byte, 257 positions in front of row 2's first sample, so a
    row-above match of 258 ends two bytes into row 2.  Row 2 starts with a run of 259; the row above has another byte at
    column 200 of that run and agrees again behind it.  The thread of row 2's first sample finds 200 bytes at the row
    distance there, skips that distance at the next position (distance 1 reaches 258) and tries it again at the one after,
    the reached one, where 198 bytes agree: a length carried over the skipped position would jump the difference and find 258."""
    rng = np.random.default_rng(7)
    tail = _filler(rng, 300)
    row1 = np.concatenate([[200] * 200, [201], [200] * 58, [202], tail]).astype(np.uint8)
    row0 = row1.copy()
    row0[304] ^= 1
    row2 = row1.copy()
    row2[200] = 200
    a = np.stack([row0, row1, row2])
    return Case("stale carry", a, PR.GRAY8, 1, a, 0)


def _copied_chunks():
    """700 random bytes, then chunks of 3 to 258 bytes copied from them: matches of many lengths and distances, each used
    once or twice, which the fixed code serves better than a code that has to be described -- in a segment that is not the last."""
    rng = np.random.default_rng(2)
    out = list(rng.integers(0, 256, 700))
    while len(out) < S:
        n = int(rng.integers(3, 259))
        at = int(rng.integers(0, 700 - n))
        out += out[at:at + n]
    return out[:S - 1] + _filler(rng, 300).tolist()


def matcher_cases():
    rng = np.random.default_rng(17)
    out = [_one_row("phrase period 700", _phrases(700, 100, 1)), _one_row("phrase period 100", _phrases(100, 20, 2)),
           _one_row("runs", _runs()),
           _one_row("run to the segment's end", np.concatenate([_filler(rng, 2699), [222] * 300])),
           _one_row("run across S", np.concatenate([_filler(rng, S - 101), [223] * 200, _filler(rng, 200)])),
           _one_row("period 1", [7] * 600), _one_row("period 2", [7, 9] * 300), _one_row("period 3", [7, 9, 11] * 200),
           _one_row("collision", _collision()), _stale_carry(), _one_row("copied chunks", _copied_chunks())]
    rgb = np.tile(np.array([[1, 2, 3], [4, 5, 6]], np.uint8), (100, 1)).reshape(1, 200, 3)
    out.append(Case("period 6 rgb", rgb, PR.RGB8, 1, rgb, 1))
    g16 = np.full((1, 300), 0x1234, np.uint16)
    out.append(Case("period 2 gray16", g16, PR.GRAY16, 1, g16, 2))
    # rows that repeat the row above: row lengths 38, 40 and 41
    for kind, w in ((PR.GRAY8, 37), (PR.RGB8, 13), (PR.GRAY16, 20)):
        if kind == PR.GRAY16:
            row = rng.integers(0, 65536, (1, w), dtype=np.uint16)
        else:
            row = rng.integers(0, 256, (1, w, 3) if kind == PR.RGB8 else (1, w), dtype=np.uint8)
        a = np.repeat(row, 40, axis=0)
        out.append(Case(f"rows repeat {KIND_NAMES[kind]}", a, kind, 1, a, kind))
    return out


# ---- the dynamic header ----------------------------------------------------------------------------------------------------
# Level 0 codes literals only: the used values ARE the non-zero code lengths, and the gaps between them the zero runs of the
# sequence.  Value 0 is always used (the filter byte), entry 256 always (the end of the block), and at level 0 the sequence
# ends with the one zero length of the distance part, entry 257.
HEADER_VALUES = {
    # gaps of 1, 2, 3, 10, 11 and 29 zeros, 3 zeros across entry 64, 138 zeros, 49 zeros
    "header gaps": (0, 2, 5, 9, 20, 32, 62, 66, 205, 255),
    "header 139": (0, 140), "header 140": (0, 141), "header 141": (0, 142), "header 148": (0, 149), "header 149": (0, 150),
    "header 255": (0,),
}


def header_cases():
    out = []
    for i, (name, values) in enumerate(HEADER_VALUES.items()):
        rng = np.random.default_rng(40 + i)
        counts = [max(1, 1500 >> k) for k in range(len(values))]                  # skewed: short codes, and far from 8 bits
        row = np.repeat(np.array(values, np.uint8), counts)
        rng.shuffle(row)
        out.append(_one_row(name, row))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = grid_cases() + matcher_cases() + header_cases()
    assert len({c.name for c in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def reference(level: int):
    """{name: (the restatement's file, the plans of its segments)}, computed once."""
    return {c.name: PR.encode_planned(c.stored, c.kind, level, c.scale) for c in all_cases()}


# ---- files past one pass of the finish kernel ------------------------------------------------------------------------------
def ramp_with_noise(h, w, kind, seed):
    """The depth ramp plus two bits of noise; gray8 takes bits 3..10 of it.  Not periodic: no two segments are alike."""
    y, x = np.mgrid[0:h, 0:w]
    ramp = (700.0 + 3.25 * x + 11.5 * y + 40.0 * np.sin(x / 9.0)).astype(np.int64)
    noise = np.random.default_rng(seed).integers(0, 4, (h, w))
    return ((ramp + noise) & 0xFFFF).astype(np.uint16) if kind == PR.GRAY16 else (((ramp >> 3) + noise) & 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def big_cases():
    """Rows of 1024 bytes: 256, 257 and 513 segments for S = 8192; and a 16-bit ramp of 1200 x 900."""
    rows = S // 1024
    out = []
    for i, (w, h, kind) in enumerate(((1023, 256 * rows, PR.GRAY8), (1023, 256 * rows + 1, PR.GRAY8), (1023, 512 * rows + 1, PR.GRAY8),
                                      (1200, 900, PR.GRAY16))):
        a = ramp_with_noise(h, w, kind, seed=60 + i)
        out.append(Case(f"big {KIND_NAMES[kind]} {w}x{h}", a, kind, 1, a, 0))
    return out


@functools.lru_cache(maxsize=None)
def big_reference():
    return {c.name: PR.encode(c.stored, c.kind, 1, c.scale) for c in big_cases()}


# ---- against zlib ----------------------------------------------------------------------------------------------------------------
def zlib_cases():
    from jpeg_cases import rendered_like
    return {"ellipse mask": (ellipse(140, 150), PR.GRAY8, 255), "semantic": (semantic(90, 80), PR.RGB8, 1),
            "depth ramp": (depth_ramp(100, 100), PR.GRAY16, 1), "rendered-like": (rendered_like(90, 80, True), PR.RGB8, 1)}


def zlib_ratio(array, kind, scale):
    """(bytes of the restatement's IDAT payload, bytes of zlib.compress(raw, 1), segments)."""
    raw, _ = PR.raw_stream(array, kind, scale)
    return len(PR.encode(array, kind, 1, scale)) - OTHER_BYTES, len(zlib.compress(raw.tobytes(), 1)), -(-len(raw) // S)


if __name__ == "__main__":
    worst = 0.0
    for name, case in zlib_cases().items():
        ours, theirs, segments = zlib_ratio(*case)
        print(f"{name}: {segments} segments, {ours} bytes against {theirs}, ratio {ours / theirs:.4f}")
        worst = max(worst, ours / theirs)
    print(f"largest ratio {worst:.3f}")
