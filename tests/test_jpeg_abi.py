"""The host side of the JPEG entries (include/pegasus_raster.h "JPEG files of device images"): the quantisation tables, the
bounds, the struct layout and the argument checks.  No GPU: fake device pointers are never dereferenced."""
import ctypes as C
import io
import re
from pathlib import Path

import numpy as np
import pytest

import jpeg_reference as JR

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import _lib, build
    build.build()
    return _lib.lib()


def _job(_lib, **kw):
    fields = dict(pixels=0x1000, width=48, height=40, kind=0, row_stride=48, pixel_stride=1, quality=95, subsampling=0)
    fields.update(kw)
    return _lib.PgrJpegJob(**fields)


RGB = dict(kind=1, row_stride=144, pixel_stride=3)


@pytest.mark.parametrize("quality", [1, 25, 50, 75, 90, 95, 100])
def test_quant_tables_are_what_pil_writes(lib, quality):
    from PIL import Image
    from pegasus_amd import jpeg
    b = io.BytesIO()
    Image.new("RGB", (8, 8)).save(b, "JPEG", quality=quality)
    q = Image.open(io.BytesIO(b.getvalue())).quantization
    lum, chroma = jpeg.quant_tables(quality)
    assert lum.tolist() == list(q[0]) and chroma.tolist() == list(q[1])
    ref = JR.quant_tables(quality)
    assert lum.tolist() == ref[0].tolist() and chroma.tolist() == ref[1].tolist()


def test_quant_tables_refuse_what_is_no_quality(lib):
    from pegasus_amd import _lib
    out = (C.c_uint8 * 64)()
    bad = _lib.PGR_ERR_INVALID_ARGUMENT
    assert lib.pgr_jpeg_quant_tables(0, out, out) == bad and lib.pgr_jpeg_quant_tables(101, out, out) == bad
    assert lib.pgr_jpeg_quant_tables(50, None, out) == bad and lib.pgr_jpeg_quant_tables(50, out, None) == bad
    assert lib.pgr_jpeg_quant_tables(50, out, out) == 0


def test_the_header_and_ctypes_agree(lib):
    from pegasus_amd import _lib
    text = (ROOT / "include" / "pegasus_raster.h").read_text()
    for name in ("PGR_JPEG_RESTART_MCUS", "PGR_JPEG_GRAY8", "PGR_JPEG_RGB8", "PGR_JPEG_444", "PGR_JPEG_420"):
        assert int(re.search(rf"^#define {name}\s+(\d+)", text, flags=re.M)[1]) == getattr(_lib, name), name
    assert JR.restart_mcus() == _lib.PGR_JPEG_RESTART_MCUS
    body = re.search(r"typedef struct PgrJpegJob \{(.*?)\} PgrJpegJob;", text, flags=re.S)[1]
    declared = re.findall(r"(\w+)\s*[,;]", body)
    assert declared == [f[0] for f in _lib.PgrJpegJob._fields_] == ["pixels", "width", "height", "kind", "row_stride",
                                                                   "pixel_stride", "quality", "subsampling"]
    J = _lib.PgrJpegJob
    assert [getattr(J, f).offset for f, _ in J._fields_] == [0, 8, 12, 16, 24, 32, 36, 40] and C.sizeof(J) == 48
    for name in ("pgr_jpeg_workspace_bytes", "pgr_jpeg_encode", "pgr_jpeg_emit", "pgr_jpeg_max_bytes", "pgr_jpeg_quant_tables"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.pgr_abi_version() == 4


def test_max_bytes_is_the_formula(lib):
    from pegasus_amd import jpeg
    R = JR.restart_mcus()
    for kind, sub in ((JR.GRAY8, JR.S444), (JR.RGB8, JR.S444), (JR.RGB8, JR.S420)):
        for w, h in ((1, 1), (800, 800), (8 * R, 8), (8 * R + 1, 9), (16384, 16384), (37, 5000)):
            side = 16 if sub == JR.S420 else 8
            mcus = -(-w // side) * -(-h // side)
            blocks = mcus * (1 if kind == JR.GRAY8 else 6 if sub == JR.S420 else 3)
            want = (330 if kind == JR.GRAY8 else 613) + 418 * blocks + 2 * -(-mcus // R)
            assert jpeg.max_bytes(w, h, kind, sub) == want == JR.max_bytes(w, h, kind, sub)
    for bad in ((0, 4, 0, 0), (4, 0, 0, 0), (16385, 4, 0, 0), (4, 16385, 1, 0), (4, 4, 2, 0), (4, 4, -1, 0), (4, 4, 1, 2), (4, 4, 0, 1)):
        assert lib.pgr_jpeg_max_bytes(*bad) == 0, bad


def test_workspace_query_refuses_what_is_outside_the_domain(lib):
    from pegasus_amd import _lib
    good = (_lib.PgrJpegJob * 2)(_job(_lib), _job(_lib, subsampling=1, **RGB))
    need = lib.pgr_jpeg_workspace_bytes(2, good)
    assert need >= 2 * (48 * 40 + 48 * 48 * 3 // 2)                            # two bytes a coefficient, at least
    assert lib.pgr_jpeg_workspace_bytes(0, good) == 0 and lib.pgr_jpeg_workspace_bytes(-1, good) == 0
    assert lib.pgr_jpeg_workspace_bytes(2, None) == 0
    for bad in (dict(width=0), dict(height=0), dict(width=-3), dict(width=16385, row_stride=16385), dict(height=16385), dict(kind=2),
                dict(kind=-1), dict(quality=0), dict(quality=101), dict(quality=-5), dict(subsampling=2), dict(subsampling=-1),
                dict(subsampling=1),                                           # a gray job has no chroma to subsample
                dict(pixel_stride=0), dict(row_stride=47), dict(kind=1, row_stride=144, pixel_stride=2), dict(kind=1, row_stride=143, pixel_stride=3)):
        assert lib.pgr_jpeg_workspace_bytes(1, (_lib.PgrJpegJob * 1)(_job(_lib, **bad))) == 0, bad
    for ok in (dict(quality=1), dict(quality=100), dict(width=16384, height=16384, row_stride=16384), dict(subsampling=1, **RGB),
               dict(kind=1, row_stride=400, pixel_stride=4), dict(width=1, height=1, row_stride=1)):
        assert lib.pgr_jpeg_workspace_bytes(1, (_lib.PgrJpegJob * 1)(_job(_lib, **ok))) > 0, ok


def test_encode_and_emit_refuse_before_any_launch(lib):
    """Null tables, jobs outside the domain, capacity < total, a total no batch of these jobs can have, a short or misaligned
    workspace: integer statuses from host-side checks, with fake device pointers and no device."""
    from pegasus_amd import _lib
    bad, small, fake = _lib.PGR_ERR_INVALID_ARGUMENT, _lib.PGR_ERR_WORKSPACE_TOO_SMALL, C.c_void_p(0x1000)
    jobs = (_lib.PgrJpegJob * 2)(_job(_lib), _job(_lib, subsampling=1, **RGB))
    need = lib.pgr_jpeg_workspace_bytes(2, jobs)
    assert lib.pgr_jpeg_encode(None, 2, fake, fake, need, None) == bad
    assert lib.pgr_jpeg_encode(jobs, -1, fake, fake, need, None) == bad
    assert lib.pgr_jpeg_encode(jobs, 2, None, fake, need, None) == bad
    assert lib.pgr_jpeg_encode(jobs, 2, fake, None, need, None) == bad
    assert lib.pgr_jpeg_encode(jobs, 2, fake, C.c_void_p(0x1008), need, None) == bad
    assert lib.pgr_jpeg_encode(jobs, 2, fake, fake, need - 1, None) == small
    for wrong in (dict(pixels=None), dict(quality=0), dict(quality=101), dict(kind=3), dict(subsampling=3), dict(subsampling=1),
                  dict(width=0), dict(height=-1)):
        table = (_lib.PgrJpegJob * 2)(_job(_lib), _job(_lib, **wrong))
        assert lib.pgr_jpeg_encode(table, 2, fake, fake, need, None) == bad, wrong
    assert lib.pgr_jpeg_encode(jobs, 0, None, None, 0, None) == 0                   # nothing to do
    total = 2 * 700
    most = JR.max_bytes(48, 40, JR.GRAY8, JR.S444) + JR.max_bytes(48, 40, JR.RGB8, JR.S420)
    assert lib.pgr_jpeg_emit(None, 2, fake, total, fake, total, fake, need, None) == bad
    assert lib.pgr_jpeg_emit(jobs, 2, None, total, fake, total, fake, need, None) == bad
    assert lib.pgr_jpeg_emit(jobs, 2, fake, total, None, total, fake, need, None) == bad
    assert lib.pgr_jpeg_emit(jobs, 2, fake, total, fake, total, None, need, None) == bad
    assert lib.pgr_jpeg_emit(jobs, 2, fake, total, fake, total - 1, fake, need, None) == bad          # capacity < total
    assert lib.pgr_jpeg_emit(jobs, 2, fake, 2 * 120, fake, total, fake, need, None) == bad            # files without data
    assert lib.pgr_jpeg_emit(jobs, 2, fake, most + 1, fake, most + 1, fake, need, None) == bad        # beyond the bound
    assert lib.pgr_jpeg_emit(jobs, 2, fake, total, fake, total, fake, need - 1, None) == small
    assert lib.pgr_jpeg_emit(jobs, 2, fake, most, fake, most, fake, need - 1, None) == small          # the bound itself passes the checks
    assert lib.pgr_jpeg_emit(jobs, 0, None, 0, None, 0, None, 0, None) == 0


def test_python_entry_refuses_host_tensors_and_other_types(tmp_path):
    import torch
    from pegasus_amd import jpeg
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.encode_batch([torch.zeros(4, 4, dtype=torch.uint8)])
    assert jpeg.encode_batch([])[1].tolist() == [0]
    with pytest.raises(ValueError, match="4:4:4"):
        jpeg.subsampling_code("4:2:2")
    assert jpeg.subsampling_code("420") == jpeg.subsampling_code("4:2:0") == 1 and jpeg.subsampling_code("4:4:4") == 0


def test_writer_and_clis_know_the_switch(tmp_path):
    from pegasus_amd import dataset_writer as DW, generate, undistort
    with pytest.raises(ValueError, match="'png' or 'jpg'"):
        DW.BopSceneWriter(tmp_path / "ds", workers=1, rgb_format="jpeg2000")
    with pytest.raises(ValueError, match="4:4:4"):
        DW.BopSceneWriter(tmp_path / "ds", workers=1, rgb_format="jpg", jpeg_subsampling="4:2:2")
    with pytest.raises(ValueError, match="1..100"):
        DW.BopSceneWriter(tmp_path / "ds", workers=1, rgb_format="jpg", jpeg_quality=0)
    w = DW.BopSceneWriter(tmp_path / "ds", workers=1)
    assert (w.rgb_format, w.jpeg_quality, w.jpeg_subsampling) == ("png", 95, "4:4:4")
    for argv in (["--rgb", "webp"], ["--rgb", "jpg", "--jpeg-subsampling", "422"], ["--rgb", "jpg", "--jpeg-quality", "0"]):
        with pytest.raises(SystemExit):
            generate.main(["--out", str(tmp_path / "x")] + argv)
    with pytest.raises(SystemExit):
        undistort.main(["-s", str(tmp_path), "--jpeg", "fpga"])
    with pytest.raises(ValueError, match="jpeg is 'host' or 'gpu'"):
        undistort.undistort_project(tmp_path, tmp_path, tmp_path / "out", jpeg="fpga")
