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

