"""The rule of the JPEG files of pegasus_amd.jpeg restated in NumPy, and a strict reader for such
files.  It shares nothing with the encoder (pegasus_amd/csrc/jpeg.hip.h, csrc/io.hip): the tables, the DCT integers, the code
builder and the bit packing are written out again here, slowly.

THE RULE, as the restatement applies it
  samples   the image is extended to whole MCUs (8x8, or 16x16 at 4:2:0) by repeating its last column and row; RGB becomes
            Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16,
            Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16; 4:2:0 chroma is (a + b + c + d + 2) >> 2; s -= 128
  DCT       C[u][x] = round(2^19 c_u cos((2x + 1) u pi / 16)), c_0 = 1 / sqrt 2, c_u = 1;  T = s C^T (int32 range), F = C T
            (int64), f = (F + 2^27) >> 28: the coefficient at scale 2^12
  quantise  q = sign(f) ((|f| + Q 2^11) // (Q 2^12)); AC clamped to +-1023, the DC difference to +-2047
  MARGIN    |f / 2^12 - c64| <= DCT_MARGIN = 0.003 for the float64 DCT c64 of the same samples:
              first pass   8 terms, each C off by <= 0.5, |s| <= 128:  8 * 0.5 * 128 / 2^20 = 2^-11 on T; the second pass
                           multiplies it by at most sum_y |c_v(y)| <= 8 / (2 sqrt 2) = 2.83           -> 0.00138
              second pass  8 terms, each C off by <= 0.5, |T| <= 128 * 2.83 = 362.04: 8 * 0.5 * 362.04 / 2^20 -> 0.00138
              the shift    half a unit of 2^-12                                                    -> 0.00012
            so q = round(c64 / Q) wherever c64 / Q is further than DCT_MARGIN / Q from a rounding tie
  codes     per file and table; counts scaled to <= 2^22, pseudo-symbol 256 with count 1, the length-limited builder (limit
            16), the pseudo-symbol swapped to the longest length, canonical codes by (length, symbol)
  scan      intervals of RESTART_MCUS MCUs, DC predictor 0 at each start, 1-bit padding, FF -> FF 00, RST(i mod 8) between
"""
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
GRAY8, RGB8 = 0, 1
S444, S420 = 0, 1
DCT_MARGIN = 0.003
HEAD_MAX = {GRAY8: 330, RGB8: 613}          # the longest header: 12 DC and 162 AC symbols a table
BLOCK_BITS = 27 + 63 * 26                   # the longest code and the most extra bits for every coefficient
CODE_MAX_FREQ = 1 << 22

# ITU-T T.81 Annex K.1 / K.2 in natural order
BASE_LUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
# natural index of zigzag position k: diagonals of x + y, even ones walked with x ascending, odd ones with y ascending
NAT_OF_ZZ = np.array(sorted(range(64), key=lambda n: (n // 8 + n % 8, n % 8 if (n // 8 + n % 8) % 2 == 0 else n // 8)))
assert NAT_OF_ZZ[:10].tolist() == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and NAT_OF_ZZ[-3:].tolist() == [55, 62, 63]


def restart_mcus() -> int:
    """PGR_JPEG_RESTART_MCUS as include/pegasus_raster.h exports it."""
    text = (ROOT / "include" / "pegasus_raster.h").read_text()
    return int(re.search(r"^#define PGR_JPEG_RESTART_MCUS\s+(\d+)", text, flags=re.M)[1])


def quant_tables(quality: int):
    """The IJG rule: int64 [64] luminance and chrominance in natural order."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE_LUM * s + 50) // 100, 1, 255), np.clip((BASE_CHROMA * s + 50) // 100, 1, 255)


def dct_matrix() -> np.ndarray:
    """int64 [u][x]."""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(u == 0, 1.0 / np.sqrt(2.0), 1.0)
    return np.rint(2.0 ** 19 * c * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


def dct_float(samples: np.ndarray) -> np.ndarray:
    """The orthonormal 8x8 DCT-II in float64 of [..., 8, 8] samples (y, x) -> (v, u)."""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(u == 0, np.sqrt(1.0 / 8.0), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)
    return np.einsum("vy,...yx,ux->...vu", c, samples.astype(np.float64), c)


def shape(width, height, kind, sub):
    """MCUs a row, MCUs a column, blocks an MCU, Y blocks an MCU."""
    side = 16 if sub == S420 else 8
    n_y = 4 if sub == S420 else 1
    return -(-width // side), -(-height // side), (1 if kind == GRAY8 else n_y + 2), n_y


def component_blocks(image: np.ndarray, sub: int):
    """The level-shifted samples of every component as int64 [blocks down, blocks across, 8, 8]."""
    image = np.asarray(image)
    assert image.dtype == np.uint8
    gray = image.ndim == 2
    assert gray or (image.ndim == 3 and image.shape[2] == 3)
    assert not (gray and sub != S444)
    side = 16 if sub == S420 else 8
    H, W = image.shape[:2]
    pad = [(0, -H % side), (0, -W % side)] + ([] if gray else [(0, 0)])
    p = np.pad(image, pad, mode="edge").astype(np.int64)
    if gray:
        planes = [p]
    else:
        R, G, B = p[..., 0], p[..., 1], p[..., 2]
        planes = [(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
                  (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16,
                  (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16]
        if sub == S420:
            planes[1:] = [(c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2 for c in planes[1:]]
    return [(c - 128).reshape(c.shape[0] // 8, 8, c.shape[1] // 8, 8).transpose(0, 2, 1, 3) for c in planes]


def quantise(samples: np.ndarray, Q: np.ndarray) -> np.ndarray:
    """int64 [..., 64] quantised coefficients in NATURAL order (v * 8 + u) of [..., 8, 8] samples; the DC is not yet a difference."""
    C = dct_matrix()
    T = np.einsum("ux,...yx->...yu", C, samples)
    F = np.einsum("vy,...yu->...vu", C, T)
    f = ((F + (1 << 27)) >> 28).reshape(*F.shape[:-2], 64)
    q = np.sign(f) * ((np.abs(f) + (Q << 11)) // (Q << 12))
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    return q


def scan_blocks(image: np.ndarray, quality: int, sub: int):
    """The blocks in the order of the scan: (component, int64 [64] in zigzag order) -- and blocks an MCU."""
    ql, qc = quant_tables(quality)
    comps = [quantise(s, ql if i == 0 else qc)[..., NAT_OF_ZZ] for i, s in enumerate(component_blocks(image, sub))]
    kind = GRAY8 if len(comps) == 1 else RGB8
    mw, mh, bpm, n_y = shape(image.shape[1], image.shape[0], kind, sub)
    out = []
    for my in range(mh):
        for mx in range(mw):
            if sub == S420:
                out += [(0, comps[0][2 * my + (j >> 1), 2 * mx + (j & 1)]) for j in range(4)]
            else:
                out.append((0, comps[0][my, mx]))
            out += [(c, comps[c][my, mx]) for c in range(1, len(comps))]
    return out, bpm


def code_lengths(freq, limit):
    """The encoder's length-limited code builder, step for step: Huffman by Moffat and Katajainen's in-place construction on
    the counts sorted by (count, symbol); lengths beyond the limit cut to it and the Kraft sum repaired a unit at a time;
    lengths handed out again in order of the counts; the flat complete code if that is cheaper."""
    n = len(freq)
    lengths = [0] * n
    keys = sorted((int(f) << 9) | s for s, f in enumerate(freq) if f)
    m = len(keys)
    if m == 0:
        return lengths
    if m == 1:
        lengths[keys[0] & 511] = 1
        return lengths
    sym = [k & 511 for k in keys]
    w = [k >> 9 for k in keys]
    w[0] += w[1]
    root, leaf = 0, 2
    for nxt in range(1, m - 1):
        if leaf >= m or w[root] < w[leaf]:
            w[nxt] = w[root]; w[root] = nxt; root += 1
        else:
            w[nxt] = w[leaf]; leaf += 1
        if leaf >= m or (root < nxt and w[root] < w[leaf]):
            w[nxt] += w[root]; w[root] = nxt; root += 1
        else:
            w[nxt] += w[leaf]; leaf += 1
    w[m - 2] = 0
    for nxt in range(m - 3, -1, -1):
        w[nxt] = w[w[nxt]] + 1
    avail, used, depth, root, nxt = 1, 0, 0, m - 2, m - 1
    while avail > 0:
        while root >= 0 and w[root] == depth:
            used += 1; root -= 1
        while avail > used:
            w[nxt] = depth; nxt -= 1; avail -= 1
        avail = 2 * used
        depth += 1
        used = 0
    num = [0] * 17
    for i in range(m):
        num[min(w[i], limit)] += 1
    kraft = sum(num[l] << (limit - l) for l in range(1, limit + 1))
    while kraft > (1 << limit) and num[limit] > 0:
        num[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if num[l]:
                num[l] -= 1; num[l + 1] += 2
                break
        kraft -= 1
    cost, i = 0, 0
    for l in range(limit, 0, -1):
        for _ in range(num[l]):
            lengths[sym[i]] = l
            cost += int(freq[sym[i]]) * l
            i += 1
    L = 1
    while (1 << L) < m:
        L += 1
    n_short = (1 << L) - m
    flat = sum(int(freq[sym[i]]) * (L - 1 if i >= m - n_short else L) for i in range(m))
    if flat < cost:
        for i in range(m):
            lengths[sym[i]] = L - 1 if i >= m - n_short else L
    return lengths


def huffman_table(counts):
    """counts: 256 symbol counts of one table -> (bits[1..16] as a list of 17, the DHT's symbols, {symbol: (code, length)})."""
    most = max(counts)
    k = 0
    while (most + (1 << k) - 1) >> k > CODE_MAX_FREQ:
        k += 1
    freq = [(int(c) + (1 << k) - 1) >> k for c in counts] + [1]
    lengths = code_lengths(freq, 16)
    longest = max(lengths)
    if lengths[256] < longest:
        s = max(s for s in range(256) if lengths[s] == longest)
        lengths[s], lengths[256] = lengths[256], longest
    order = sorted((l, s) for s, l in enumerate(lengths) if l)
    assert order[-1][1] == 256
    codes, code, prev = {}, 0, order[0][0]
    for l, s in order:
        code <<= l - prev
        prev = l
        codes[s] = (code, l)
        code += 1
    assert codes[256][0] == (1 << codes[256][1]) - 1, "the pseudo-symbol holds the code of all ones"
    del codes[256]
    bits = [0] * 17
    for l, s in order[:-1]:
        bits[l] += 1
    return bits, [s for _, s in order[:-1]], codes


def block_tokens(zz, pred):
    """(table offset 0 DC / 1 AC, symbol, size, extra) of one block whose DC predictor is `pred`."""
    def mag(v):
        size = int(abs(v)).bit_length()
        return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)
    diff = max(-2047, min(2047, int(zz[0]) - pred))
    size, extra = mag(diff)
    out = [(0, size, size, extra)]
    last = 0
    for k in np.flatnonzero(zz[1:]) + 1:
        run = int(k) - last - 1
        out += [(1, 0xF0, 0, 0)] * (run >> 4)
        size, extra = mag(int(zz[k]))
        out.append((1, ((run & 15) << 4) | size, size, extra))
        last = int(k)
    if last < 63:
        out.append((1, 0x00, 0, 0))
    return out


def encode(image: np.ndarray, quality: int, sub: int = S444) -> bytes:
    """The whole file."""
    image = np.asarray(image)
    R = restart_mcus()
    blocks, bpm = scan_blocks(image, quality, sub)
    colour = image.ndim == 3
    nc = 3 if colour else 1
    n_tab = 4 if colour else 2
    intervals = []
    for first in range(0, len(blocks), R * bpm):
        pred = [0, 0, 0]
        tokens = []
        for comp, zz in blocks[first:first + R * bpm]:
            tokens += [(2 * min(comp, 1) + t, s, size, extra) for t, s, size, extra in block_tokens(zz, pred[comp])]
            pred[comp] = int(zz[0])
        intervals.append(tokens)
    counts = [[0] * 256 for _ in range(n_tab)]
    for tokens in intervals:
        for t, s, _, _ in tokens:
            counts[t][s] += 1
    tables = [huffman_table(c) for c in counts]
    ql, qc = quant_tables(quality)
    H, W = image.shape[:2]
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += b"\xff\xdb" + (2 + 65 * (2 if colour else 1)).to_bytes(2, "big")
    for t, q in enumerate([ql, qc][:2 if colour else 1]):
        out += bytes([t]) + bytes(q[NAT_OF_ZZ].astype(np.uint8).tolist())
    out += b"\xff\xc0" + (8 + 3 * nc).to_bytes(2, "big") + b"\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc])
    out += bytes([1, 0x22 if sub == S420 else 0x11, 0])
    if colour:
        out += bytes([2, 0x11, 1, 3, 0x11, 1])
    out += b"\xff\xc4" + (2 + sum(17 + len(v) for _, v, _ in tables)).to_bytes(2, "big")
    for t, (bits, vals, _) in enumerate(tables):
        out += bytes([((t & 1) << 4) | (t >> 1)]) + bytes(bits[1:]) + bytes(vals)
    out += b"\xff\xdd\x00\x04" + R.to_bytes(2, "big")
    out += b"\xff\xda" + (6 + 2 * nc).to_bytes(2, "big") + bytes([nc, 1, 0x00]) + (bytes([2, 0x11, 3, 0x11]) if colour else b"")
    out += bytes([0, 63, 0])
    for i, tokens in enumerate(intervals):
        acc, n = 0, 0
        for t, s, size, extra in tokens:
            code, length = tables[t][2][s]
            acc = (((acc << length) | code) << size) | extra
            n += length + size
        pad = -n % 8
        acc = (acc << pad) | ((1 << pad) - 1)
        out += acc.to_bytes((n + pad) // 8, "big").replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD0 + i % 8]) if i + 1 < len(intervals) else b"\xff\xd9"
    return bytes(out)


def max_bytes(width, height, kind, sub) -> int:
    """What no file exceeds: the longest header, every block at BLOCK_BITS with every byte stuffed, two bytes an interval."""
    mw, mh, bpm, _ = shape(width, height, kind, sub)
    return HEAD_MAX[kind] + 2 * (-(-BLOCK_BITS // 8)) * mw * mh * bpm + 2 * (-(-(mw * mh) // restart_mcus()))


def flat_bound(width, height, kind, sub) -> int:
    """What the file of a UNIFORM image cannot exceed if the code builder does its work.  Every AC is zero, so the AC tables
    hold EOB and the pseudo-symbol: EOB is one bit.  A DC table holds category 0, the categories of the interval-first blocks
    (one for Y, at most two for Cb and Cr together) and the pseudo-symbol: at most four codes, none longer than 3 bits; where
    category 0 is counted at least as often as all the others together -- asserted here -- it gets one bit.  So a first block
    of a component costs at most 3 + 11 + 1 = 15 bits and every other block 2.  Only bytes that hold bits of the first MCU
    or padding can be FF: ceil(first MCU bits / 8) + 1 stuffed bytes at most.  Per interval: those, the padding byte and
    the marker."""
    R = restart_mcus()
    mw, mh, bpm, n_y = shape(width, height, kind, sub)
    n_mcu = mw * mh
    n_iv = -(-n_mcu // R)
    nc = 1 if kind == GRAY8 else 3
    for blocks_mcu, comps in ((n_y, 1),) + (((2, 2),) if nc == 3 else ()):
        assert n_mcu * blocks_mcu - n_iv * comps >= n_iv * comps + 1, "category 0 must be the table's most frequent symbol"
    first_mcu_bits = 15 * nc + 2 * (bpm - nc)
    total = HEAD_MAX[kind]
    for i in range(n_iv):
        blocks = min(R, n_mcu - i * R) * bpm
        total += -(-(15 * nc + 2 * (blocks - nc)) // 8) + (-(-first_mcu_bits // 8) + 1) + 2
    return total


# ---- the strict reader ---------------------------------------------------------------------------------------------------------
def _segment(data, pos, marker):
    assert data[pos] == 0xFF and data[pos + 1] == marker, f"marker {marker:02X} expected at {pos}, found {data[pos]:02X} {data[pos + 1]:02X}"
    n = int.from_bytes(data[pos + 2:pos + 4], "big")
    assert n >= 2 and pos + 2 + n <= len(data), "a segment runs past the file"
    return data[pos + 4:pos + 2 + n], pos + 2 + n


def read_jpeg(data: bytes, quality=None) -> dict:
    """Reads a file of the rule and nothing else; AssertionError on any departure.  Returns width, height, kind, sub, quality,
    qtables, restart, n_intervals, stuffed (FF 00 pairs in the entropy data) and coefficients: per component int64
    [blocks down, blocks across, 64] in zigzag order, DC undone to its value."""
    data = bytes(data)
    R = restart_mcus()
    assert data[:2] == b"\xff\xd8", "SOI"
    body, pos = _segment(data, 2, 0xE0)
    assert body == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00", "APP0: JFIF 1.01, density 1:1, no thumbnail"
    body, pos = _segment(data, pos, 0xDB)
    assert len(body) in (65, 130), "DQT: one or two 8-bit tables"
    qt = []
    for t in range(len(body) // 65):
        assert body[65 * t] == t, "DQT: 8-bit precision, tables 0, 1 in order"
        q = np.zeros(64, np.int64)
        q[NAT_OF_ZZ] = np.frombuffer(body[65 * t + 1:65 * t + 65], np.uint8)
        qt.append(q)
    matches = [v for v in ([quality] if quality is not None else range(1, 101))
               if all((q == r).all() for q, r in zip(qt, quant_tables(v)))]
    assert matches, "DQT: not the IJG rule's tables" + ("" if quality is None else f" of quality {quality}")
    nc = 3 if len(qt) == 2 else 1
    body, pos = _segment(data, pos, 0xC0)
    assert len(body) == 6 + 3 * nc and body[0] == 8 and body[5] == nc, "SOF0: 8 bits, the components of the DQT"
    height, width = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
    assert width >= 1 and height >= 1
    comps = [tuple(body[6 + 3 * c:9 + 3 * c]) for c in range(nc)]
    assert comps[0] in ((1, 0x11, 0), (1, 0x22, 0)) and not (nc == 1 and comps[0][1] != 0x11)
    assert comps[1:] == [(2, 0x11, 1), (3, 0x11, 1)][:nc - 1], "SOF0: Cb and Cr at 1x1 on table 1"
    sub = S420 if comps[0][1] == 0x22 else S444
    body, pos = _segment(data, pos, 0xC4)
    tables, at = [], 0
    for t in range(2 * len(qt)):
        assert at + 17 <= len(body) and body[at] == (((t & 1) << 4) | (t >> 1)), "DHT: DC0, AC0, DC1, AC1 in order"
        bits = [0] + list(body[at + 1:at + 17])
        n = sum(bits)
        vals = list(body[at + 17:at + 17 + n])
        assert len(vals) == n and n >= 1 and len(set(vals)) == n, "DHT: symbols"
        assert all(v <= 11 for v in vals) if t % 2 == 0 else all((v & 15) <= 10 and ((v & 15) or v in (0, 0xF0)) for v in vals)
        lookup, code, k = {}, 0, 0
        for l in range(1, 17):
            for _ in range(bits[l]):
                assert code < (1 << l) - 1, "DHT: a code of all ones, or more codes than the length holds"
                lookup[(l, code)] = vals[k]
                code += 1
                k += 1
            code <<= 1
        # canonical codes of ascending length below 2^l - 1 are prefix-free: a later code is larger than every earlier one
        # extended, and the Kraft sum stays below 1
        assert sum(b * 2 ** (16 - l) for l, b in enumerate(bits)) < 2 ** 16
        tables.append(lookup)
        at += 17 + n
    assert at == len(body), "DHT: length"
    body, pos = _segment(data, pos, 0xDD)
    assert len(body) == 2 and int.from_bytes(body, "big") == R, "DRI"
    body, pos = _segment(data, pos, 0xDA)
    assert body == bytes([nc, 1, 0x00]) + (bytes([2, 0x11, 3, 0x11]) if nc == 3 else b"") + bytes([0, 63, 0]), "SOS"

    # entropy data: stuffing, markers
    kind = RGB8 if nc == 3 else GRAY8
    mw, mh, bpm, n_y = shape(width, height, kind, sub)
    n_mcu = mw * mh
    intervals, cur, stuffed, i = [], bytearray(), 0, pos
    while True:
        assert i < len(data), "no EOI"
        b = data[i]
        if b != 0xFF:
            cur.append(b); i += 1
            continue
        assert i + 1 < len(data), "FF at the end"
        m = data[i + 1]
        if m == 0x00:
            cur.append(0xFF); stuffed += 1; i += 2
        elif 0xD0 <= m <= 0xD7:
            assert m - 0xD0 == len(intervals) % 8, "RST out of sequence"
            intervals.append(bytes(cur)); cur = bytearray(); i += 2
        else:
            assert m == 0xD9, f"FF {m:02X} in the entropy data"
            intervals.append(bytes(cur)); i += 2
            break
    assert i == len(data), "bytes after EOI"
    assert len(intervals) == -(-n_mcu // R), "intervals: one per RESTART_MCUS MCUs, no RST after the last"

    grids = [np.zeros((mh * (2 if sub == S420 else 1), mw * (2 if sub == S420 else 1), 64), np.int64)] + \
            [np.zeros((mh, mw, 64), np.int64) for _ in range(nc - 1)]
    for iv, raw in enumerate(intervals):
        nbits = 8 * len(raw)
        val = int.from_bytes(raw, "big") if raw else 0
        at = 0

        def take(n):
            nonlocal at
            assert at + n <= nbits, "the interval's bits run out"
            v = (val >> (nbits - at - n)) & ((1 << n) - 1)
            at += n
            return v

        def symbol(lookup):
            nonlocal at
            for l in range(1, 17):
                if at + l <= nbits:
                    s = lookup.get((l, (val >> (nbits - at - l)) & ((1 << l) - 1)))
                    if s is not None:
                        at += l
                        return s
            raise AssertionError("no code matches")

        def value(size):
            v = take(size) if size else 0
            return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1

        pred = [0] * nc
        for mcu in range(iv * R, min(n_mcu, (iv + 1) * R)):
            my, mx = divmod(mcu, mw)
            for j in range(bpm):
                comp = 0 if j < n_y else j - n_y + 1
                zz = np.zeros(64, np.int64)
                pred[comp] += value(symbol(tables[2 * min(comp, 1)]))
                zz[0] = pred[comp]
                k = 1
                while k < 64:
                    s = symbol(tables[2 * min(comp, 1) + 1])
                    if s == 0:
                        break
                    k += s >> 4
                    if s != 0xF0:
                        assert k < 64, "a run past the block"
                        zz[k] = value(s & 15)
                    k += 1
                assert k <= 64, "a run past the block"
                if comp == 0 and sub == S420:
                    grids[0][2 * my + (j >> 1), 2 * mx + (j & 1)] = zz
                else:
                    grids[comp][my, mx] = zz
        rest = nbits - at
        assert rest < 8 and (rest == 0 or take(rest) == (1 << rest) - 1), "padding: fewer than 8 bits, all 1"
    return dict(width=width, height=height, kind=kind, sub=sub, quality=matches[0], qtables=qt, restart=R,
                n_intervals=len(intervals), stuffed=stuffed, coefficients=grids)


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)
