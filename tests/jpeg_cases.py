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
