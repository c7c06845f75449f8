"""What the JPEG tests share: the images, the cases of the byte-equality test and the limits against PIL.

The limits were measured on the RESTATEMENT (tests/jpeg_reference.py), never on the encoder, with

    python tests/jpeg_cases.py

which prints, over COMPARE_CASES, the largest shortfall of the restatement's PSNR to the source below that of PIL's own file
(same quality, subsampling, optimize=True, restart_marker_blocks = PGR_JPEG_RESTART_MCUS) and the largest ratio of the file
sizes.  Recorded doubled (the ratio: its excess over 1 doubled):

    measured: shortfall 0.034 dB, ratio 1.008   ->   PSNR_MARGIN_DB = 0.068, SIZE_RATIO = 1.016
"""
import functools
import io

import numpy as np

import jpeg_reference as JR

R = JR.restart_mcus()
QUALITIES = (1, 50, 95, 100)
MODES = {"gray": (JR.GRAY8, JR.S444), "444": (JR.RGB8, JR.S444), "420": (JR.RGB8, JR.S420)}
PSNR_MARGIN_DB = 0.068
SIZE_RATIO = 1.016


def noise(h, w, colour, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3) if colour else (h, w), dtype=np.uint8)


def ramp(h, w, colour):
    y, x = np.mgrid[0:h, 0:w]
    g = ((3 * x + 5 * y) % 256).astype(np.uint8)
    return np.stack([g, 255 - g, (g.astype(np.int64) * 7 % 256).astype(np.uint8)], -1) if colour else g


def flat(h, w, colour, value=(201, 33, 90)):
    return np.broadcast_to(np.array(value, np.uint8), (h, w, 3)).copy() if colour else np.full((h, w), value[0], np.uint8)


def rendered_like(h, w, colour, seed=3):
    """Smooth shading, a few hard edges and sensor-like noise: what a rendered frame looks like to a DCT."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for k in range(3 if colour else 1):
        p = 120 + 70 * np.sin(x / (11.0 + 3 * k) + k) * np.cos(y / (7.0 + 2 * k)) + 40 * ((x - w / 2) ** 2 + (y - h / 2) ** 2 < (min(h, w) / 3) ** 2)
        p[(x > w * 0.6) & (y > h * 0.55)] = 30 + 60 * k
        planes.append(p + rng.normal(0, 2.0, (h, w)))
    im = np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)
    return im if colour else im[..., 0]


def equality_images(mode: str):
    """name -> image for one mode: the small shapes, the widths around the restart interval and the contents."""
    kind, sub = MODES[mode]
    colour = kind == JR.RGB8
    side = 16 if sub == JR.S420 else 8
    images = {f"noise {w}x{h}": noise(h, w, colour, seed=w * 31 + h)
              for w, h in ((1, 1), (7, 9), (8, 8), (9, 8), (16, 16), (17, 17), (37, 1), (1, 37), (40, 24))}
    # one row of MCUs: R - 1, R, R + 1 MCUs and 8 R + 1 (the RST index wraps around), the last MCU cut
    for mcus in (R - 1, R, R + 1, 8 * R + 1):
        images[f"ramp+noise {mcus} MCUs"] = ramp(side - 3, mcus * side - 3, colour) ^ (noise(side - 3, mcus * side - 3, colour, seed=mcus) >> 5)
    images["zeros"] = flat(17, 33, colour, (0, 0, 0))
    images["all 255"] = flat(17, 33, colour, (255, 255, 255))
    images["flat"] = flat(17, 33, colour)
    images["ramp"] = ramp(24, 40, colour)
    images["rendered-like"] = rendered_like(40, 56, colour)
    return images


@functools.lru_cache(maxsize=None)
def reference_files(mode: str):
    """{(name, quality): bytes} of the restatement, computed once."""
    _, sub = MODES[mode]
    return {(name, q): JR.encode(im, q, sub) for name, im in equality_images(mode).items() for q in QUALITIES}


# ---- edges: tokens no ordinary image codes, the code-length limit, files past one pass of the finish kernel -----------------------
def single_coefficient_block(k: int, v: int, Q) -> np.ndarray:
    """uint8 [8,8]: the float inverse DCT of v * Q[k] at zigzag position k, plus 128, rounded.  At quality 50 the restatement
    quantises it back to exactly that coefficient (tests/test_jpeg_host.py asserts it for every block used here)."""
    X = np.zeros(64)
    X[JR.NAT_OF_ZZ[k]] = v * int(Q[JR.NAT_OF_ZZ[k]])
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(u == 0, np.sqrt(1.0 / 8.0), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)
    return np.rint(128.0 + c.T @ X.reshape(8, 8) @ c).astype(np.uint8)


TOKEN_KS = (17, 33, 49, 62, 63)            # one, two, three ZRLs; three and a run of 13; three, a run of 14 and no EOB


def grid_of_blocks(blocks, across: int) -> np.ndarray:
    blocks = np.asarray(blocks)
    return blocks.reshape(-1, across, *blocks.shape[1:]).transpose(0, 2, 1, 3).reshape(-1, across * blocks.shape[2])


def token_image(mode: str) -> np.ndarray:
    """Single-coefficient blocks of TOKEN_KS with v = 1 and -2 and a flat block: gray; or, at 4:2:0, as luminance (a gray RGB
    image: Y is the sample, the chroma 128) next to a half that carries them in Cb and Cr at constant luminance."""
    ql, qc = JR.quant_tables(50)
    luma = grid_of_blocks([single_coefficient_block(k, v, ql) for v in (1, -2) for k in TOKEN_KS] + [np.full((8, 8), 128, np.uint8)] * 2, 6)
    if mode == "gray":
        return luma
    y = np.concatenate([luma, np.full_like(luma, 128)], axis=1).astype(np.float64)
    chroma = grid_of_blocks([single_coefficient_block(k, v, qc) for v in (1, -2) for k in TOKEN_KS] + [np.full((8, 8), 128, np.uint8)] * 2, 6)
    chroma = np.kron(chroma.astype(np.float64) - 128.0, np.ones((2, 2)))                       # a chroma sample covers 2 x 2 pixels
    y = np.concatenate([y, np.full((chroma.shape[0] - y.shape[0], y.shape[1]), 128.0)], axis=0)
    y = np.concatenate([y, np.full((y.shape[0], 2 * chroma.shape[1] - y.shape[1]), 128.0)], axis=1)
    cb = np.concatenate([np.zeros_like(chroma), chroma], axis=1)
    cr = np.concatenate([np.zeros_like(chroma), np.roll(chroma, 16, axis=0)], axis=1)              # the two rows of blocks swapped
    rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], -1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def dc11_image(mode: str) -> np.ndarray:
    """Black and white blocks in both orders: at quality 100 the DC difference is +-2040, category 11."""
    side = 16 if mode == "420" else 8
    g = np.kron(np.array([[0, 255, 255, 0, 255], [255, 0, 0, 255, 0]], np.uint8), np.ones((side, side), np.uint8))
    return g if mode == "gray" else np.stack([g, g, g], -1)


FIBONACCI_COUNTS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597)        # F(2) .. F(17): 4179 blocks


def fibonacci_image() -> np.ndarray:
    """Gray, 528 x 512 = 66 x 64 blocks = 264 intervals: FIBONACCI_COUNTS[k - 1] blocks whose one coefficient is a 1 at zigzag
    position k (symbol (k - 1) << 4 | 1), shuffled, and 45 flat blocks.  With the end-of-block symbol of every block and the
    pseudo-symbol the AC table's counts are 1, 1, 2, 3, 5, ..., 1597, 4224: every merge of a Huffman code of them takes the
    accumulated subtree and the next count, whatever the tie-break, so the unlimited code is 17 deep."""
    ql, _ = JR.quant_tables(50)
    kinds = [single_coefficient_block(k, 1, ql) for k in range(1, 17)] + [np.full((8, 8), 128, np.uint8)]
    which = np.repeat(np.arange(17), FIBONACCI_COUNTS + (66 * 64 - sum(FIBONACCI_COUNTS),))
    np.random.default_rng(23).shuffle(which)
    return grid_of_blocks(np.array(kinds)[which], 66)


def shallowest_huffman_depth(counts) -> int:
    """Depth of a Huffman code of ``counts`` when every tie goes to the shallower subtree."""
    import heapq
    heap = [(int(f), 0) for f in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def past_one_pass_shapes():
    """name -> (mode, MCUs across, MCUs down): 256, 257 and 513 intervals of gray, 260 of 4:2:0.  One row of 256 R MCUs would be
    32768 pixels wide, outside the encoder's domain (sides to 16384) and, at 512 R + 1, outside what a JPEG header can say
    (65535): the same MCU counts are laid out in rows instead, intervals being counted in raster order whatever the width --
    256 R = 64 x 64, 256 R + 1 = 4097 = 241 x 17 (a last interval of one MCU), and, 512 R + 1 = 8193 = 3 x 2731 having no
    shape inside the domain, 512 R + 2 = 8194 = 241 x 34 (a last interval of two)."""
    assert R == 16
    return {"256 intervals": ("gray", 64, 64), "257 intervals": ("gray", 241, 17), "513 intervals": ("gray", 241, 34),
            "260 intervals 420": ("420", 64, 65)}


def past_one_pass_image(name: str) -> np.ndarray:
    mode, across, down = past_one_pass_shapes()[name]
    side = 16 if mode == "420" else 8
    h, w = down * side, across * side
    return ramp(h, w, mode != "gray") ^ (noise(h, w, mode != "gray", seed=across + down) >> 5)


def edge_cases():
    """name -> (mode, image, quality)."""
    out = {}
    for mode in ("gray", "420"):
        out[f"tokens {mode}"] = (mode, token_image(mode), 50)
        out[f"dc 11 {mode}"] = (mode, dc11_image(mode), 100)
    out["fibonacci"] = ("gray", fibonacci_image(), 50)
    for name, (mode, _, _) in past_one_pass_shapes().items():
        out[name] = (mode, past_one_pass_image(name), 50)
    return out


@functools.lru_cache(maxsize=None)
def edge_reference_files():
    """{name: bytes} of the restatement, computed once."""
    return {name: JR.encode(im, q, MODES[mode][1]) for name, (mode, im, q) in edge_cases().items()}


COMPARE_CASES = [(mode, q, h, w) for mode in MODES for q in (50, 75, 95) for h, w in ((48, 64), (64, 48), (90, 120))]


def pil_file(image, quality, sub):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(image).save(b, "JPEG", quality=quality, subsampling="4:2:0" if sub == JR.S420 else "4:4:4", optimize=True,
                                restart_marker_blocks=R)
    return b.getvalue()


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def compare_with_pil(mode, quality, h, w):
    """(PSNR of the restatement's file, PSNR of PIL's, bytes of the restatement's, bytes of PIL's), both decoded by PIL."""
    kind, sub = MODES[mode]
    im = rendered_like(h, w, kind == JR.RGB8)
    ours, theirs = JR.encode(im, quality, sub), pil_file(im, quality, sub)
    return JR.psnr(pil_decode(ours), im), JR.psnr(pil_decode(theirs), im), len(ours), len(theirs)


if __name__ == "__main__":
    worst_db, worst_ratio = 0.0, 0.0
    for case in COMPARE_CASES:
        a, b, na, nb = compare_with_pil(*case)
        print(case, f"psnr {a:.3f} vs {b:.3f}  bytes {na} vs {nb}  ratio {na / nb:.4f}")
        worst_db, worst_ratio = max(worst_db, b - a), max(worst_ratio, na / nb)
    print(f"largest shortfall {worst_db:.3f} dB, largest ratio {worst_ratio:.3f}")
