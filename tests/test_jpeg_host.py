"""The NumPy restatement of the JPEG rule (tests/jpeg_reference.py) judged on its own -- by its strict reader, by PIL's decoder,
by a float64 DCT and against PIL's own files -- and the JPEG side of pegasus_amd.bop_dataset.  No GPU."""
import io

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_reference as JR


@pytest.mark.parametrize("mode", list(JC.MODES))
def test_the_restatements_files_pass_the_strict_reader_and_pil(mode):
    from PIL import Image
    kind, sub = JC.MODES[mode]
    images = JC.equality_images(mode)
    for (name, q), data in JC.reference_files(mode).items():
        h, w = images[name].shape[:2]
        info = JR.read_jpeg(data, q)
        assert (info["width"], info["height"], info["kind"], info["sub"], info["restart"]) == (w, h, kind, sub, JC.R), (name, q)
        assert len(data) <= JR.max_bytes(w, h, kind, sub)
        with Image.open(io.BytesIO(data)) as im:
            assert im.size == (w, h) and im.mode == ("L" if kind == JR.GRAY8 else "RGB"), (name, q)
            im.load()
    assert JR.read_jpeg(JC.reference_files(mode)["noise 40x24", 100], 100)["stuffed"] >= 1


def test_the_reader_gives_back_the_coefficients_that_were_coded():
    im = JC.rendered_like(40, 56, True)
    for sub in (JR.S444, JR.S420):
        ql, qc = JR.quant_tables(75)
        want = [JR.quantise(s, ql if i == 0 else qc)[..., JR.NAT_OF_ZZ] for i, s in enumerate(JR.component_blocks(im, sub))]
        got = JR.read_jpeg(JR.encode(im, 75, sub), 75)["coefficients"]
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b)


def test_the_strict_reader_refuses_what_the_rule_does_not_allow():
    data = bytearray(JR.encode(JC.rendered_like(24, 8 * (JC.R + 2), False), 75))
    JR.read_jpeg(bytes(data), 75)
    with pytest.raises(AssertionError, match="after EOI"):
        JR.read_jpeg(bytes(data) + b"\x00", 75)
    with pytest.raises(AssertionError, match="DQT"):
        JR.read_jpeg(bytes(data), 74)
    first_rst = data.index(b"\xff\xd0", 300)
    for at, byte, what in ((first_rst + 1, 0xD1, "RST out of sequence"), (first_rst - 1, data[first_rst - 1] ^ 1, "padding"),
                           (data.index(b"\xff\xdd") + 5, JC.R + 1, "DRI")):
        broken = bytearray(data)
        broken[at] = byte
        with pytest.raises(AssertionError, match=what):
            JR.read_jpeg(bytes(broken), 75)


@pytest.mark.parametrize("mode", list(JC.MODES))
@pytest.mark.parametrize("quality", [25, 50])           # Q >= 10: the margin is at most 0.0003 of a step
def test_quantised_coefficients_are_the_rounded_float64_dct(mode, quality):
    """q == round(c64 / Q) wherever c64 / Q is further than DCT_MARGIN / Q from a rounding tie (the margin is derived next to the
    rule in jpeg_reference.py), and the margin leaves out at most 0.1 % of the coefficients of these images."""
    kind, sub = JC.MODES[mode]
    ql, qc = JR.quant_tables(quality)
    left_out = total = 0
    for seed in range(3):
        image = JC.rendered_like(64, 96, kind == JR.RGB8, seed=seed)
        for i, samples in enumerate(JR.component_blocks(image, sub)):
            Q = (ql if i == 0 else qc).astype(np.float64)
            ratio = JR.dct_float(samples).reshape(*samples.shape[:2], 64) / Q
            q = JR.quantise(samples, ql if i == 0 else qc)
            assert np.abs(q[..., 1:]).max() < 1023                             # (the AC clamp does not bind on these images)
            to_tie = np.abs(np.abs(ratio) - np.floor(np.abs(ratio)) - 0.5)
            sure = to_tie > JR.DCT_MARGIN / Q
            want = np.sign(ratio) * np.floor(np.abs(ratio) + 0.5)
            assert (q[sure] == want[sure]).all()
            # inside the margin the two neighbours of the tie are the only values
            assert (np.abs(q - ratio) <= 0.5 + JR.DCT_MARGIN / Q).all()
            left_out += int((~sure).sum())
            total += sure.size
    assert left_out <= 0.001 * total, (left_out, total)


def test_the_integer_dct_keeps_its_margin_on_extreme_blocks():
    rng = np.random.default_rng(0)
    blocks = np.concatenate([rng.integers(-128, 128, (500, 8, 8)), rng.choice([-128, 127], (500, 8, 8)),
                             np.full((1, 8, 8), -128), np.full((1, 8, 8), 127)]).astype(np.int64)
    C = JR.dct_matrix()
    f = (np.einsum("vy,nyu->nvu", C, np.einsum("ux,nyx->nyu", C, blocks)) + (1 << 27)) >> 28
    assert np.abs(f / 4096.0 - JR.dct_float(blocks)).max() <= JR.DCT_MARGIN
    assert np.abs(np.einsum("ux,nyx->nyu", C, blocks)).max() < 2 ** 29           # the first pass fits int32


@pytest.mark.parametrize("case", JC.COMPARE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_quality_and_size_against_pil_at_equal_settings(case):
    ours, pil, n_ours, n_pil = JC.compare_with_pil(*case)
    assert ours >= pil - JC.PSNR_MARGIN_DB, (ours, pil)
    assert n_ours <= JC.SIZE_RATIO * n_pil, (n_ours, n_pil)


@pytest.mark.parametrize("mode", list(JC.MODES))
def test_a_uniform_image_costs_two_bits_a_block(mode):
    """The derived bound of jpeg_reference.flat_bound: it fails if the code builder gives EOB or the DC category 0 more than
    one bit where they dominate their tables."""
    kind, sub = JC.MODES[mode]
    for w, h, value in ((256, 64, (201, 33, 90)), (250, 100, (0, 0, 0)), (8 * JC.R + 3, 50, (255, 255, 255))):
        data = JR.encode(JC.flat(h, w, kind == JR.RGB8, value), 95, sub)
        JR.read_jpeg(data, 95)
        assert len(data) <= JR.flat_bound(w, h, kind, sub), (w, h, value, len(data), JR.flat_bound(w, h, kind, sub))


def test_code_lengths_of_the_restatement_are_complete_and_limited():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    cases = [fib[:30] + [0] * 227, [1] * 257, [0] * 200 + [5] + [0] * 55 + [1]] + \
            [(rng.integers(0, 2, 257) * rng.geometric(1.0 / rng.choice([2, 40, 3000]), 257)).tolist() for _ in range(30)]
    for freq in cases:
        freq = list(freq)
        freq[256] = 1
        lengths = JR.code_lengths(freq, 16)
        used = [s for s, f in enumerate(freq) if f]
        assert all(1 <= lengths[s] <= 16 for s in used) and all(lengths[s] == 0 for s in range(257) if not freq[s])
        if len(used) >= 2:
            assert sum(Fraction(1, 2 ** lengths[s]) for s in used) == 1
    # Fibonacci counts need the limit: an unlimited code of 30 of them is 29 deep
    assert max(JR.code_lengths(fib[:30] + [0] * 226 + [1], 16)) == 16


def test_the_device_builder_and_the_restatement_build_the_same_lengths():
    """The restatement's port of the code builder against the library's own (pgr_png_code_lengths takes limits to 15)."""
    from pegasus_amd import png
    rng = np.random.default_rng(11)
    for _ in range(40):
        n = int(rng.integers(2, 258))
        freq = (rng.integers(0, 2, n) * rng.geometric(1.0 / rng.choice([2, 40, 3000]), n)).astype(np.uint32)
        assert png.code_lengths(freq, 15).tolist() == JR.code_lengths(freq.tolist(), 15)


# ---- the edge cases of jpeg_cases.edge_cases, judged on the restatement alone ------------------------------------------------------
def _tokens_of(name):
    """[(component, [(table offset, symbol, size, extra)])] of every block of an edge case, DC predictors as the scan has them."""
    mode, image, q = JC.edge_cases()[name]
    blocks, bpm = JR.scan_blocks(image, q, JC.MODES[mode][1])
    out = []
    for first in range(0, len(blocks), JC.R * bpm):
        pred = [0, 0, 0]
        for comp, zz in blocks[first:first + JC.R * bpm]:
            out.append((comp, JR.block_tokens(zz, pred[comp])))
            pred[comp] = int(zz[0])
    return out


def _reader_gives_back_the_coefficients(name):
    mode, image, q = JC.edge_cases()[name]
    sub = JC.MODES[mode][1]
    ql, qc = JR.quant_tables(q)
    want = [JR.quantise(s, ql if i == 0 else qc)[..., JR.NAT_OF_ZZ] for i, s in enumerate(JR.component_blocks(image, sub))]
    info = JR.read_jpeg(JC.edge_reference_files()[name], q)
    for a, b in zip(want, info["coefficients"]):
        np.testing.assert_array_equal(a, b)
    return info


def _dht_bits(data):
    """bits[1..16] of every table of a file's DHT, as lists of 17."""
    at = data.index(b"\xff\xc4")
    body = data[at + 4:at + 2 + int.from_bytes(data[at + 2:at + 4], "big")]
    out, pos = [], 0
    while pos < len(body):
        bits = [0] + list(body[pos + 1:pos + 17])
        out.append(bits)
        pos += 17 + sum(bits)
    return out


@pytest.mark.parametrize("mode", ["gray", "420"])
def test_single_coefficient_blocks_code_up_to_three_zrls_and_no_eob(mode):
    """Every block of the token image quantises to the one coefficient it was built from (or to none), in luminance and, at
    4:2:0, in both chroma components; one, two and three ZRLs in a row are coded in each AC table, and the blocks whose
    coefficient 63 is not zero end without an EOB."""
    name = f"tokens {mode}"
    _, image, q = JC.edge_cases()[name]
    info = _reader_gives_back_the_coefficients(name)
    for comp, grid in enumerate(info["coefficients"]):
        found = sorted((int(k), int(zz[k])) for zz in grid.reshape(-1, 64) for k in np.flatnonzero(zz))
        assert (grid.reshape(-1, 64) != 0).sum(axis=1).max() == 1 and not grid[..., 0].any()
        assert found == sorted((k, v) for k in JC.TOKEN_KS for v in (1, -2)), (comp, found)
    for table in ((1,) if mode == "gray" else (1, 3)):
        zrls, no_eob = set(), 0
        for comp, tokens in _tokens_of(name):
            ac = [s for t, s, _, _ in tokens if t == 1]
            if 2 * min(comp, 1) + 1 != table or ac == [0x00]:
                continue
            zrls.add(ac.count(0xF0))
            assert ac[:ac.count(0xF0)] == [0xF0] * ac.count(0xF0)                 # in a row, in front of the coefficient's symbol
            no_eob += ac[-1] != 0x00
        assert zrls == {1, 2, 3} and no_eob == 2 * (1 if mode == "gray" or table == 1 else 2), (table, zrls, no_eob)
    from PIL import Image
    with Image.open(io.BytesIO(JC.edge_reference_files()[name])) as im:
        assert im.size == image.shape[1::-1]
        im.load()


@pytest.mark.parametrize("mode", ["gray", "420"])
def test_black_and_white_blocks_code_dc_category_11(mode):
    name = f"dc 11 {mode}"
    _reader_gives_back_the_coefficients(name)
    dc = [(size, extra) for comp, tokens in _tokens_of(name) for t, s, size, extra in tokens if t == 0 and comp == 0]
    assert {s for s, _ in dc} >= {11} and max(s for s, _ in dc) == 11
    # both signs: +2040 is 11111111000, -2040 its complement (a first block of black codes -1024: 01111111111)
    assert {e for s, e in dc if s == 11} >= {2040, 2047 - 2040}


def test_the_fibonacci_blocks_need_the_limit_of_16():
    """On the restatement alone: the counts are what the case promises, their unlimited code is deeper than 16, the limited
    table has a 16-bit code in the DHT, the file has 264 intervals, the reader gives back the coefficients and PIL decodes it."""
    from PIL import Image
    _, image, q = JC.edge_cases()["fibonacci"]
    counts = [0] * 256
    for comp, tokens in _tokens_of("fibonacci"):
        for t, s, _, _ in tokens:
            if t == 1:
                counts[s] += 1
    assert [counts[((k - 1) << 4) | 1] for k in range(1, 17)] == list(JC.FIBONACCI_COUNTS) and counts[0] == 66 * 64
    assert sum(1 for c in counts if c) == 17
    depth = JC.shallowest_huffman_depth([c for c in counts if c] + [1])
    bits = _dht_bits(JC.edge_reference_files()["fibonacci"])[1]
    print("fibonacci: shallowest unlimited depth", depth, "AC bits", bits[1:])
    assert depth == 17 > 16
    assert bits[16] >= 1 and sum(bits) == 17
    assert bits[1:] == JR.huffman_table(counts)[0][1:]
    info = _reader_gives_back_the_coefficients("fibonacci")
    assert info["n_intervals"] == 264 > 256
    with Image.open(io.BytesIO(JC.edge_reference_files()["fibonacci"])) as im:
        decoded = np.asarray(im).astype(np.int64)
    print("fibonacci: PIL's decode is within", int(np.abs(decoded - image).max()), "of the source")
    assert decoded.shape == image.shape


def test_files_past_one_pass_have_the_intervals_they_are_named_for():
    for name, (mode, across, down) in JC.past_one_pass_shapes().items():
        _, image, q = JC.edge_cases()[name]
        info = JR.read_jpeg(JC.edge_reference_files()[name], q)
        assert info["n_intervals"] == int(name.split()[0]) == -(-across * down // JC.R) and max(image.shape[:2]) <= 16384


# ---- bop_dataset -------------------------------------------------------------------------------------------------------------
def _scene(root, ext, gray=False):
    from PIL import Image
    from pegasus_amd import bop_dataset as BD
    scene = BD.BopScene(BD.scene_dir(root, "train", 3))
    scene.make_dirs()
    pixels = {}
    for i in (0, 7):
        pixels[i] = JC.rendered_like(30, 44, not gray, seed=i)
        if ext == ".png":
            scene.image_path("rgb", i).write_bytes(BD.encode_png(pixels[i]))
        else:
            Image.fromarray(pixels[i]).save(scene.path / "rgb" / f"{i:06d}{ext}", quality=97, progressive=(i == 7))
    scene.write_json(BD.SCENE_GT, {str(i): [] for i in pixels})
    return scene, pixels


@pytest.mark.parametrize("ext", [".jpg", ".jpeg"])
def test_bop_scene_reads_jpeg_rgb(tmp_path, ext):
    from pegasus_amd import bop_dataset as BD
    scene, pixels = _scene(tmp_path / "ds", ext)
    for i in (0, 7):
        path = scene.image_path("rgb", i)
        assert path.name == f"{i:06d}{ext}" and path.exists()
        assert BD.jpeg_size(path) == (44, 30)                                  # frame 7 is progressive: SOF2
        assert scene.image_size(i) == (44, 30)
        got = scene.read_image("rgb", i)
        assert got.dtype == np.uint8 and got.shape == (30, 44, 3) and JR.psnr(got, pixels[i]) > 35.0
        np.testing.assert_array_equal(got, BD.read_image(path))
    assert scene.first_image_size() == (44, 30)
    assert scene.image_path("rgb", 5).name == "000005.png"                     # neither exists: the PNG path as before
    assert scene.image_path("depth", 0).name == "000000.png" and scene.image_path("mask", 0, 1).name == "000000_000001.png"
    # a PNG beside the JPEG wins
    scene.image_path("rgb", 5).parent.joinpath("000000.png").write_bytes(BD.encode_png(pixels[0]))
    assert scene.image_path("rgb", 0).name == "000000.png"
    np.testing.assert_array_equal(scene.read_image("rgb", 0), pixels[0])


def test_bop_scene_with_png_rgb_behaves_as_before(tmp_path):
    from pegasus_amd import bop_dataset as BD
    scene, pixels = _scene(tmp_path / "ds", ".png")
    for i in (0, 7):
        assert scene.image_path("rgb", i).name == BD.image_name(i) == f"{i:06d}.png"
        np.testing.assert_array_equal(scene.read_image("rgb", i), pixels[i])
        np.testing.assert_array_equal(scene.read_png("rgb", i), pixels[i])
        assert scene.image_size(i) == (44, 30)
    assert scene.first_image_size() == (44, 30) and scene.image_size(3) == (0, 0)
    assert BD.image_name(4, ext="jpg") == "000004.jpg"


def test_jpeg_size_of_gray_files_and_of_what_is_no_jpeg(tmp_path):
    from pegasus_amd import bop_dataset as BD
    p = tmp_path / "g.jpg"
    p.write_bytes(JR.encode(JC.rendered_like(21, 35, False), 80))
    assert BD.jpeg_size(p) == (35, 21) and BD.read_image(p).shape == (21, 35)
    q = tmp_path / "not.jpg"
    q.write_bytes(BD.encode_png(np.zeros((4, 4), np.uint8)))
    assert BD.jpeg_size(q) is None


def test_coco_names_the_jpeg_of_a_jpeg_scene(tmp_path):
    from pegasus_amd import bop_dataset as BD
    scene, _ = _scene(tmp_path / "ds", ".jpg")
    assert f"rgb/{scene.image_path('rgb', 7).name}" == "rgb/000007.jpg"
