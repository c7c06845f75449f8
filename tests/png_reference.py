"""A strict PNG reader for the files of pegasus_amd.png, and what the tests of those files share.  It shares nothing with
the encoder (pegasus_amd/csrc/png.hip.h): chunk CRCs are zlib.crc32's, the stream is inflated by zlib, which checks the
Adler-32 itself.  Stricter than bop_dataset.decode_png: exactly signature / IHDR / one IDAT / IEND and nothing behind it,
every chunk CRC, the end of the zlib stream at the end of the IDAT, every filter byte 0."""
import re
import struct
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
SIGNATURE = b"\x89PNG\r\n\x1a\n"
FRAMING_BYTES = 63      # signature 8, IHDR 25, IDAT length/tag/CRC 12, zlib header 2, Adler-32 4, IEND 12
GRAY8, RGB8, GRAY16 = 0, 1, 2


def segment_bytes() -> int:
    """PGR_PNG_SEGMENT_BYTES as include/pegasus_raster.h exports it."""
    text = (ROOT / "include" / "pegasus_raster.h").read_text()
    return int(re.search(r"^#define PGR_PNG_SEGMENT_BYTES\s+(\d+)", text, flags=re.M)[1])


def read_png(data: bytes) -> np.ndarray:
    """uint8 [H,W], uint8 [H,W,3] or uint16 [H,W]; raises AssertionError on anything the rule of the file does not allow."""
    data = bytes(data)
    assert data[:8] == SIGNATURE, "signature"
    pos, chunks = 8, []
    while pos < len(data):
        assert pos + 12 <= len(data), "a chunk header runs past the file"
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        assert pos + 12 + n <= len(data), f"chunk {tag!r} runs past the file"
        body = data[pos + 8:pos + 8 + n]
        crc = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, f"CRC of chunk {tag!r}"
        chunks.append((tag, body))
        pos += 12 + n
        if tag == b"IEND":
            break
    assert pos == len(data), "bytes behind IEND"
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"], [t for t, _ in chunks]
    assert len(chunks[0][1]) == 13 and len(chunks[2][1]) == 0
    w, h, depth, ctype, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (ctype, depth) in ((0, 8), (2, 8), (0, 16)) and (compression, filt, interlace) == (0, 0, 0)
    idat = chunks[1][1]
    assert idat[:2] == b"\x78\x01", "zlib header"
    inflater = zlib.decompressobj()
    raw = inflater.decompress(idat)
    assert inflater.eof and inflater.unused_data == b"" and inflater.unconsumed_tail == b"", "the zlib stream ends with the IDAT"
    row_bytes = w * (3 if ctype == 2 else 1) * depth // 8
    assert len(raw) == h * (1 + row_bytes), "raw stream length"
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + row_bytes)
    assert not rows[:, 0].any(), "filter type other than 0"
    body = rows[:, 1:]
    if depth == 16:
        return body.reshape(h, w, 2).copy().view(">u2").reshape(h, w).astype(np.uint16)
    return body.reshape(h, w, 3).copy() if ctype == 2 else body.copy()


def raw_bytes(width: int, height: int, kind: int) -> int:
    return height * (1 + width * (1, 3, 2)[kind])


def max_bytes(width: int, height: int, kind: int) -> int:
    """The bound of the rule: 63 + raw bytes + 5 per segment."""
    raw, S = raw_bytes(width, height, kind), segment_bytes()
    return FRAMING_BYTES + raw + 5 * ((raw + S - 1) // S)


# ---- the rule of the encoder, restated ----------------------------------------------------------------------------------------
# pegasus_amd/csrc/png.hip.h states the rule at its top and DESIGN.md section 23 in prose; this is that rule again, written
# for whole arrays in NumPy and shared with nothing of the encoder but the code-length builder's port (jpeg_reference.
# code_lengths, which tests/test_jpeg_host.py holds against the library's own).  encode() gives the file; plan_segment() gives
# what was decided on the way, which tests/test_png_rule_host.py asks for its coverage.
HASH_BITS = 11
MIN_MATCH, MAX_MATCH = 3, 258
# RFC 1951 3.2.5: base values and extra bits of the length symbols 257.. and of the distance symbols
LENGTH_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
                        227, 258], np.int64)
LENGTH_EXTRA = np.array([0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0], np.int64)
DIST_BASE = np.array([1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                      6145, 8193, 12289, 16385, 24577], np.int64)
DIST_EXTRA = np.array([0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)], np.int64)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8      # 3.2.6
FIXED_DIST = [5] * 30
STORED, FIXED, DYNAMIC = 0, 1, 2


def subblock() -> int:
    """PGR_PNG_SUBBLOCK as include/pegasus_raster.h exports it."""
    text = (ROOT / "include" / "pegasus_raster.h").read_text()
    return int(re.search(r"^#define PGR_PNG_SUBBLOCK\s+(\d+)", text, flags=re.M)[1])


def kind_of(array: np.ndarray) -> int:
    array = np.asarray(array)
    if array.dtype == np.uint8:
        return RGB8 if array.ndim == 3 else GRAY8
    assert array.dtype in (np.uint16, np.int16) and array.ndim == 2
    return GRAY16


def raw_stream(array: np.ndarray, kind: int, scale: int = 1):
    """(the filtered raw stream as uint8 [H * row_len], row_len): filter byte 0 in front of every row, gray8 samples times
    ``scale`` mod 256, 16-bit samples big-endian."""
    array = np.asarray(array)
    h = array.shape[0]
    if kind == GRAY8:
        assert array.dtype == np.uint8 and array.ndim == 2
        rows = ((array.astype(np.int64) * scale) & 255).astype(np.uint8)
    elif kind == RGB8:
        assert array.dtype == np.uint8 and array.ndim == 3 and array.shape[2] == 3 and scale == 1
        rows = array.reshape(h, -1)
    else:
        assert array.dtype in (np.uint16, np.int16) and array.ndim == 2 and scale == 1
        rows = array.astype(np.uint16).astype(">u2").view(np.uint8).reshape(h, -1)
    stream = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1)
    return stream.reshape(-1), stream.shape[1]


def hash_of(raw: np.ndarray) -> np.ndarray:
    """The bucket of every position p with p + 3 <= n."""
    b = raw.astype(np.uint64)
    word = b[:-2] | (b[1:-1] << np.uint64(8)) | (b[2:] << np.uint64(16))
    return (((word * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)).astype(np.int64)


def candidates(raw: np.ndarray) -> np.ndarray:
    """int64 [n]: the highest hashed position of p's bucket in a sub-block in front of p's own, -1 where there is none."""
    n, sub = len(raw), subblock()
    cand = np.full(n, -1, np.int64)
    if n < MIN_MATCH:
        return cand
    h = hash_of(raw)
    highest = np.full(1 << HASH_BITS, -1, np.int64)            # over the sub-blocks in front
    for first in range(0, len(h), sub):
        mine = h[first:first + sub]
        cand[first:first + len(mine)] = highest[mine]
        np.maximum.at(highest, mine, np.arange(first, first + len(mine)))
    return cand


def _lengths_at_distance(raw: np.ndarray, d: int) -> np.ndarray:
    """int64 [n]: bytes that agree at p and p - d from p on, inside the stream, at most 258; 0 where d > p."""
    n = len(raw)
    if d > n - 1:
        return np.zeros(n, np.int64)
    at = np.arange(n)
    differs = np.ones(n, bool)
    differs[d:] = raw[d:] != raw[:-d]
    stop = np.minimum.accumulate(np.where(differs, at, n)[::-1])[::-1]      # the first position from p on that differs
    return np.minimum(stop - at, MAX_MATCH)


def _lengths_at_candidates(raw: np.ndarray, cand: np.ndarray) -> np.ndarray:
    n = len(raw)
    out = np.zeros(n, np.int64)
    p = np.flatnonzero(cand >= 0)
    q = cand[p]
    for k in range(MAX_MATCH):
        keep = p + k < n
        p, q = p[keep], q[keep]
        keep = raw[p + k] == raw[q + k]
        p, q = p[keep], q[keep]
        if len(p) == 0:
            break
        out[p] = k + 1
    return out


def matches(raw: np.ndarray, row_len: int):
    """(length, distance, candidate) per position: the longest of the distances 1, 2, 3, 6, row_len and the candidate's with
    3 bytes or more, ties to the smaller distance; length 0 where there is none."""
    n = len(raw)
    cand = candidates(raw)
    at = np.arange(n)
    lengths = [_lengths_at_distance(raw, d) for d in (1, 2, 3, 6, row_len)] + [_lengths_at_candidates(raw, cand)]
    dists = [np.full(n, d, np.int64) for d in (1, 2, 3, 6, row_len)] + [np.where(cand >= 0, at - cand, 1 << 15)]
    lengths, dists = np.stack(lengths), np.stack(dists)
    lengths[lengths < MIN_MATCH] = 0
    best = np.argmax(lengths * (1 << 16) + ((1 << 16) - 1 - dists), axis=0)          # longest, then nearest
    length = lengths[best, at]
    return length, np.where(length > 0, dists[best, at], 0), cand


def greedy_parse(length: np.ndarray) -> np.ndarray:
    """Positions of the tokens: from byte 0, a match at a reached position is taken whole."""
    n = len(length)
    has = np.flatnonzero(length)
    token = np.zeros(n, bool)
    p, k = 0, 0
    while p < n:
        k = np.searchsorted(has, p)
        m = int(has[k]) if k < len(has) else n                 # literals up to the next position with a match
        token[p:m + 1 if m < n else n] = True
        p = m + int(length[m]) if m < n else n
    return np.flatnonzero(token)


def canonical_codes(lengths):
    """{symbol: (code as it is sent, LSB first; length)} of RFC 1951 3.2.2."""
    codes, code = {}, 0
    for l in range(1, 16):
        for s, ls in enumerate(lengths):
            if ls == l:
                codes[s] = (int(format(code, f"0{l}b")[::-1], 2), l)
                code += 1
        code <<= 1
    return codes


def code_length_sequence(lengths):
    """The hlit + hdist code lengths as symbols of the code-length alphabet: [(symbol, extra bits, extra value)] and the zero
    runs [(first entry, entries)].  Symbol 16 is not used."""
    seq, runs, i = [], [], 0
    while i < len(lengths):
        if lengths[i]:
            seq.append((lengths[i], 0, 0))
            i += 1
            continue
        j = i
        while j < len(lengths) and lengths[j] == 0:
            j += 1
        r = j - i
        runs.append((i, r))
        seq += [(18, 7, 138 - 11)] * (r // 138)
        rest = r % 138
        if rest >= 11:
            seq.append((18, 7, rest - 11))
        elif rest >= 3:
            seq.append((17, 3, rest - 3))
        else:
            seq += [(0, 0, 0)] * rest
        i = j
    return seq, runs


def _pack(values, bits) -> bytes:
    """Fields of ``bits`` bits each, the first in the lowest bits of the first byte (RFC 1951 3.1.1)."""
    values, bits = np.asarray(values, np.int64), np.asarray(bits, np.int64)
    field = np.repeat(np.arange(len(bits)), bits)
    within = np.arange(int(bits.sum())) - np.repeat(np.cumsum(bits) - bits, bits)
    return np.packbits(((values[field] >> within) & 1).astype(np.uint8), bitorder="little").tobytes()


def plan_segment(raw: np.ndarray, row_len: int, level: int, last: bool) -> dict:
    """One segment on its own: what the rule decides, and its bytes.  Keys: n, last, raw, row_len, length / distance / candidate
    per position (level 1), tokens (positions), sizes (bytes as stored, fixed, dynamic), form, bytes, and what the dynamic
    form would send: hlit, hdist, hclen, sequence, zero_runs [(first entry, entries)] and the three alphabets' code lengths."""
    from jpeg_reference import code_lengths
    n = len(raw)
    if level > 0:
        length, distance, cand = matches(raw, row_len)
        tokens = greedy_parse(length)
    else:
        length = distance = np.zeros(n, np.int64)
        cand = np.full(n, -1, np.int64)
        tokens = np.arange(n)
    t_len, t_dist = length[tokens], distance[tokens]
    is_match = t_len > 0
    len_sym = np.searchsorted(LENGTH_BASE, t_len[is_match], side="right") - 1
    dist_sym = np.searchsorted(DIST_BASE, t_dist[is_match], side="right") - 1
    litlen_hist = np.bincount(raw[tokens[~is_match]], minlength=288) + np.bincount(257 + len_sym, minlength=288)
    litlen_hist[256] = 1
    dist_hist = np.bincount(dist_sym, minlength=30)
    extra_bits = int(LENGTH_EXTRA[len_sym].sum() + DIST_EXTRA[dist_sym].sum())

    litlen_lengths = code_lengths(litlen_hist[:286].tolist(), 15)
    dist_lengths = code_lengths(dist_hist.tolist(), 15)
    hlit, hdist = 286, 30
    while hlit > 257 and litlen_lengths[hlit - 1] == 0:
        hlit -= 1
    while hdist > 1 and dist_lengths[hdist - 1] == 0:
        hdist -= 1
    sequence, zero_runs = code_length_sequence(litlen_lengths[:hlit] + dist_lengths[:hdist])
    cl_hist = np.bincount([s for s, _, _ in sequence], minlength=19)
    cl_lengths = code_lengths(cl_hist.tolist(), 7)
    hclen = 19
    while hclen > 4 and cl_lengths[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    header_bits = sum(cl_lengths[s] + e for s, e, _ in sequence)

    cost_fix = int((litlen_hist * np.array(FIXED_LITLEN)).sum() + 5 * dist_hist.sum())
    cost_dyn = int((litlen_hist[:286] * np.array(litlen_lengths)).sum() + (dist_hist * np.array(dist_lengths)).sum())
    bits_fix = 3 + cost_fix + extra_bits
    bits_dyn = 3 + 14 + 3 * hclen + header_bits + cost_dyn + extra_bits
    size = (lambda bits: (bits + 7) // 8) if last else (lambda bits: (bits + 3 + 7) // 8 + 4)
    form, nbytes = STORED, n + 5
    if size(bits_fix) < nbytes:
        form, nbytes = FIXED, size(bits_fix)
    if size(bits_dyn) < nbytes:
        form, nbytes = DYNAMIC, size(bits_dyn)

    plan = dict(n=n, last=last, raw=raw, row_len=row_len, sizes=(n + 5, size(bits_fix), size(bits_dyn)), length=length, distance=distance, candidate=cand, tokens=tokens, form=form, hlit=hlit, hdist=hdist,
                hclen=hclen, sequence=sequence, zero_runs=zero_runs, litlen_lengths=litlen_lengths, dist_lengths=dist_lengths,
                cl_lengths=cl_lengths)
    if form == STORED:
        plan["bytes"] = bytes([1 if last else 0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + raw.tobytes()
        return plan
    values, bits = [(1 if last else 0) | (form << 1)], [3]
    if form == DYNAMIC:
        values += [hlit - 257, hdist - 1, hclen - 4] + [cl_lengths[s] for s in CL_ORDER[:hclen]]
        bits += [5, 5, 4] + [3] * hclen
        cl_codes = canonical_codes(cl_lengths)
        for s, e, v in sequence:
            values += [cl_codes[s][0], v]
            bits += [cl_codes[s][1], e]
        litlen_codes, dist_codes = canonical_codes(litlen_lengths), canonical_codes(dist_lengths)
    else:
        litlen_codes, dist_codes = canonical_codes(FIXED_LITLEN), canonical_codes(FIXED_DIST + [5, 5])
    # a token is four fields: literal or length code, length extra, distance code, distance extra (the last three empty for a literal)
    code = np.zeros((2, 288), np.int64)
    for s, (c, l) in litlen_codes.items():
        code[:, s] = c, l
    dcode = np.zeros((2, 32), np.int64)
    for s, (c, l) in dist_codes.items():
        dcode[:, s] = c, l
    first_sym = raw[tokens].astype(np.int64)
    first_sym[is_match] = 257 + len_sym
    t_values, t_bits = np.zeros((len(tokens), 4), np.int64), np.zeros((len(tokens), 4), np.int64)
    t_values[:, 0], t_bits[:, 0] = code[0, first_sym], code[1, first_sym]
    t_values[is_match, 1], t_bits[is_match, 1] = t_len[is_match] - LENGTH_BASE[len_sym], LENGTH_EXTRA[len_sym]
    t_values[is_match, 2], t_bits[is_match, 2] = dcode[0, dist_sym], dcode[1, dist_sym]
    t_values[is_match, 3], t_bits[is_match, 3] = t_dist[is_match] - DIST_BASE[dist_sym], DIST_EXTRA[dist_sym]
    values = np.concatenate([np.array(values, np.int64), t_values.reshape(-1), [litlen_codes[256][0]]])
    bits = np.concatenate([np.array(bits, np.int64), t_bits.reshape(-1), [litlen_codes[256][1]]])
    assert int(bits.sum()) == (bits_dyn if form == DYNAMIC else bits_fix), "the cost that chose the form is the block's length"
    data = _pack(values, bits) if last else _pack(np.concatenate([values, [0]]), np.concatenate([bits, [3]])) + b"\x00\x00\xff\xff"
    assert len(data) == nbytes
    plan["bytes"] = data
    return plan


def plan(array: np.ndarray, kind: int, level: int = 1, scale: int = 1):
    """The plans of all segments of an image, in order."""
    raw, row_len = raw_stream(array, kind, scale)
    S = segment_bytes()
    return [plan_segment(raw[at:at + S], row_len, level, at + S >= len(raw)) for at in range(0, len(raw), S)]


def frame(width: int, height: int, kind: int, raw: np.ndarray, segments) -> bytes:
    """Signature, IHDR, one IDAT (78 01, the segments, the Adler-32 of the raw stream), IEND."""
    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    ihdr = struct.pack(">IIBBBBB", width, height, 16 if kind == GRAY16 else 8, 2 if kind == RGB8 else 0, 0, 0, 0)
    idat = b"\x78\x01" + b"".join(segments) + struct.pack(">I", zlib.adler32(raw.tobytes()) & 0xFFFFFFFF)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def encode_planned(array: np.ndarray, kind: int, level: int = 1, scale: int = 1):
    """(the file the rule gives for an image, the plans of its segments)."""
    array = np.asarray(array)
    raw, _ = raw_stream(array, kind, scale)
    plans = plan(array, kind, level, scale)
    return frame(array.shape[1], array.shape[0], kind, raw, [p["bytes"] for p in plans]), plans


def encode(array: np.ndarray, kind: int, level: int = 1, scale: int = 1) -> bytes:
    """The file the rule gives for an image: uint8 [H,W], uint8 [H,W,3] or uint16 / int16 [H,W]."""
    return encode_planned(array, kind, level, scale)[0]
