"""pgr_mesh_vertex_normals and pgr_mesh_vertex_colors at the C ABI, without a GPU: the symbols stand in the header, the library
and _lib.SYMBOLS; the size function is host-only; argument misuse is an integer status from host-side checks (fake non-NULL
device pointers are never dereferenced and no device is touched); the Python wrappers refuse host tensors."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("pgr_mesh_vertex_normals_workspace_bytes", "pgr_mesh_vertex_normals", "pgr_mesh_vertex_colors")
FAKE = C.c_void_p(0x10000)


@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import _lib, build
    build.build()
    return _lib.lib()


def test_symbols_stand_in_the_header_the_library_and_the_prototypes(lib):
    from pegasus_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pegasus_raster.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(pgr_[a-z_0-9]+)\s*\(", text))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.SYMBOLS["pgr_mesh_vertex_normals"][1][-1] is C.c_void_p          # the stream comes last
    assert _lib.SYMBOLS["pgr_mesh_vertex_colors"][1][-1] is C.c_void_p
    assert lib.pgr_abi_version() == 4
    # the kernel header is compiled into the library: exactly one of the translation units that build.py compiles includes it
    from pegasus_amd import build
    including = [src.name for src in build.sources()[0] if '#include "meshattr.hip.h"' in src.read_text()]
    assert len(including) == 1, including


def test_workspace_size_is_host_only(lib):
    size = lib.pgr_mesh_vertex_normals_workspace_bytes
    assert [size(n) for n in (1, 2, 1000, 900_000)] == [24, 48, 24_000, 21_600_000]
    assert size(2 ** 31 - 1) == 24 * (2 ** 31 - 1)
    assert size(0) == 0 and size(-1) == 0 and size(-2 ** 31) == 0


def normals_rc(lib, V=10, vertices=FAKE, F=5, faces=FAKE, normals=FAKE, ws=FAKE, ws_bytes=240):
    return lib.pgr_mesh_vertex_normals(V, vertices, F, faces, normals, ws, ws_bytes, None)


def test_vertex_normals_rejects_misuse_before_any_launch(lib):
    from pegasus_amd import _lib
    bad = _lib.PGR_ERR_INVALID_ARGUMENT
    assert normals_rc(lib, vertices=None) == bad
    assert normals_rc(lib, normals=None) == bad
    assert normals_rc(lib, faces=None) == bad
    assert normals_rc(lib, ws=None) == bad
    assert normals_rc(lib, ws_bytes=239) == bad                      # a short workspace
    assert normals_rc(lib, ws_bytes=0) == bad
    assert normals_rc(lib, ws=C.c_void_p(0x10004)) == bad            # the sums are int64
    assert normals_rc(lib, V=-1) == bad
    assert normals_rc(lib, F=-1) == bad
    # no vertices: a successful no-op (nothing to zero-fill), whatever else is passed
    assert normals_rc(lib, V=0, vertices=None, F=0, faces=None, normals=None, ws=None, ws_bytes=0) == _lib.PGR_OK
    assert normals_rc(lib, V=0, F=5) == _lib.PGR_OK
    with pytest.raises(ValueError):
        _lib.check(bad, "pgr_mesh_vertex_normals")


def cameras(n, W=8, H=6, **override):
    from pegasus_amd import _lib
    arr = (_lib.PgrCamera * max(n, 1))()
    for k in range(max(n, 1)):
        kw = dict(image_width=W, image_height=H, tanfovx=0.5, tanfovy=0.4, viewmatrix=FAKE, projmatrix=None, campos=FAKE, bg=None,
                  depth_mode=1)
        kw.update(override)
        arr[k] = _lib.PgrCamera(**kw)
    return arr


def colors_rc(lib, V=10, vertices=FAKE, normals=FAKE, n_views=2, cams="default", color=FAKE, depth=FAKE, final_T=FAKE,
              depth_tol=0.01, alpha_min=0.5, cos_min=0.3, fill="default", colors=FAKE, seen=FAKE):
    cams = cameras(n_views) if cams == "default" else cams
    fill = (C.c_float * 3)(0.5, 0.5, 0.5) if fill == "default" else fill
    return lib.pgr_mesh_vertex_colors(V, vertices, normals, n_views, cams, color, depth, final_T, depth_tol, alpha_min, cos_min,
                                      fill, colors, seen, None)


def test_vertex_colors_rejects_misuse_before_any_launch(lib):
    from pegasus_amd import _lib
    bad = _lib.PGR_ERR_INVALID_ARGUMENT
    for name in ("vertices", "colors", "color", "depth", "final_T", "cams", "fill"):
        assert colors_rc(lib, **{name: None}) == bad, name
    assert colors_rc(lib, n_views=0) == bad
    assert colors_rc(lib, n_views=257, cams=cameras(257)) == bad
    assert colors_rc(lib, n_views=-1) == bad
    assert colors_rc(lib, V=-1) == bad
    for alpha_min in (0.0, -0.5, float("nan")):
        assert colors_rc(lib, alpha_min=alpha_min) == bad, alpha_min
    for depth_tol in (-1e-6, float("-inf"), float("nan")):
        assert colors_rc(lib, depth_tol=depth_tol) == bad, depth_tol
    assert colors_rc(lib, cos_min=float("nan")) == bad
    mixed = cameras(3)
    mixed[2].image_width = 9
    assert colors_rc(lib, n_views=3, cams=mixed) == bad
    mixed = cameras(3)
    mixed[1].image_height = 5
    assert colors_rc(lib, n_views=3, cams=mixed) == bad
    assert colors_rc(lib, cams=cameras(2, viewmatrix=None)) == bad
    assert colors_rc(lib, cams=cameras(2, campos=None)) == bad
    assert colors_rc(lib, cams=cameras(2, tanfovx=0.0)) == bad
    assert colors_rc(lib, cams=cameras(2, W=0)) == bad
    # no vertices: a successful no-op once everything else is in order (NULL normals and NULL seen are allowed)
    assert colors_rc(lib, V=0, vertices=None, normals=None, colors=None, seen=None) == _lib.PGR_OK
    assert colors_rc(lib, V=0, n_views=256, cams=cameras(256)) == _lib.PGR_OK
    assert colors_rc(lib, V=0, alpha_min=0.0) == bad


def test_python_wrappers_refuse_host_tensors():
    import torch
    from pegasus_amd import mesh as M
    v = np.zeros((3, 3), np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.vertex_normals((torch.from_numpy(v), torch.from_numpy(f)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.vertex_normals(M.Mesh(v, f), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.vertex_normals_device(torch.from_numpy(v), torch.from_numpy(f))

    class View:
        image_height, image_width = 4, 5
    images = dict(color=torch.zeros(1, 3, 4, 5), depth=torch.zeros(1, 4, 5), final_T=torch.zeros(1, 4, 5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.vertex_colors(M.Mesh(v, f), images["color"], images["depth"], images["final_T"], [View()], depth_tol=0.01)
    with pytest.raises(ValueError):
        M.vertex_colors(M.Mesh(v, f), images["color"], images["depth"], images["final_T"], [], depth_tol=0.01)


def test_flags_exist_and_default_off():
    from pegasus_amd import mesh as M
    a = M._parser().parse_args(["-m", "x", "--out", "y", "--obj_id", "1"])
    assert a.vertex_colors is False
    assert M._parser().parse_args(["-m", "x", "--out", "y", "--obj_id", "1", "--vertex_colors"]).vertex_colors is True
    import inspect
    sig = inspect.signature(M.extract_mesh).parameters
    assert sig["colors"].default is False and sig["depth_tol_voxels"].default == 2.0 and sig["cos_min"].default == 0.3
    assert inspect.signature(M.render_views).parameters["want_color"].default is False
    from pegasus_amd import decimate as D
    assert inspect.signature(D.write_models_eval).parameters["normals"].default is False
