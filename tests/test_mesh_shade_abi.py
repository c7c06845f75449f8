"""pgr_mesh_visibility / pgr_mesh_shade: the workspace sizes are host-only functions and the argument checks come before any
launch, so they run without a device (the pointers handed in are never dereferenced)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from pegasus_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
FAKE = C.c_void_p(4096)          # non-NULL and aligned; a call that got as far as using it would fault
NEW = ("pgr_mesh_visibility_workspace_bytes", "pgr_mesh_visibility", "pgr_mesh_shade_workspace_bytes", "pgr_mesh_shade")


@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import build
    build.build()
    return _lib.lib()


def jobs(n, faces=12, slot=0):
    arr = (_lib.PgrMeshJob * max(n, 1))()
    for k in range(n):
        arr[k] = _lib.PgrMeshJob(vertex_first=0, vertex_count=8, face_first=0, face_count=faces, R=(C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1),
                                 t=(C.c_float * 3)(0, 0, 4), fx=100.0, fy=100.0, cx=8.0, cy=8.0, slot=slot)
    return arr


def visibility(lib, n=2, arr=None, nv=8, nf=1 << 22, W=16, H=16, near=0.25, keys=FAKE, n_slots=1, cnt=FAKE, ws=FAKE, ws_bytes=None, v=FAKE, f=FAKE):
    arr = jobs(n) if arr is None else arr
    if ws_bytes is None:
        ws_bytes = lib.pgr_mesh_visibility_workspace_bytes(n, arr)
    return lib.pgr_mesh_visibility(v, nv, f, nf, n, arr, W, H, near, keys, n_slots, cnt, ws, ws_bytes, None)


def shade(lib, n=2, arr=None, nv=8, nf=1 << 22, W=16, H=16, near=0.25, keys=FAKE, n_slots=1, params="default", ws=FAKE, ws_bytes=None, v=FAKE,
          f=FAKE):
    arr = jobs(n) if arr is None else arr
    if ws_bytes is None:
        ws_bytes = lib.pgr_mesh_shade_workspace_bytes(n, arr)
    if params == "default":
        params = _lib.PgrMeshShade(ambient=0.5, rgb=FAKE)
    return lib.pgr_mesh_shade(v, nv, f, nf, n, arr, W, H, near, keys, n_slots, None if params is None else C.byref(params), ws, ws_bytes, None)


def test_the_new_symbols_are_in_the_header_and_in_the_library(lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pegasus_raster.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(pgr_[a-z_0-9]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "#define PGR_MESH_VISIBILITY_MAX_JOBS 1024" in text and _lib.PGR_MESH_VISIBILITY_MAX_JOBS == 1024
    assert "typedef struct PgrMeshShade" in text
    fields = re.search(r"typedef struct PgrMeshShade \{(.*?)\} PgrMeshShade;", text, flags=re.S).group(1)
    assert re.findall(r"\*?(\w+)(?:\[3\])?;", fields) == [n for n, _ in _lib.PgrMeshShade._fields_]


@pytest.mark.parametrize("size", ["pgr_mesh_visibility_workspace_bytes", "pgr_mesh_shade_workspace_bytes"])
def test_workspace_sizes_are_host_only_and_refuse_what_the_key_cannot_hold(lib, size):
    fn = getattr(lib, size)
    assert fn(1, jobs(1)) > 0 and fn(1024, jobs(1024)) > 0
    assert fn(1025, jobs(1025)) == 0                                             # 10 bits of the key name the job
    assert fn(1, jobs(1, faces=1 << 22)) > 0 and fn(1, jobs(1, faces=(1 << 22) + 1)) == 0       # 22 bits name the face
    assert fn(0, jobs(1)) == 0 and fn(-1, jobs(1)) == 0 and fn(1, None) == 0
    assert fn(1, jobs(1, faces=-1)) == 0


def test_workspaces_hold_what_they_are_for(lib):
    assert lib.pgr_mesh_visibility_workspace_bytes(3, jobs(3)) == lib.pgr_mesh_depth_workspace_bytes(3, jobs(3))       # the same queue
    assert lib.pgr_mesh_shade_workspace_bytes(1024, jobs(1024)) >= 1024 * (4 * 4 + 16 * 4 + 3 * 4)                     # the job table


def test_entries_refuse_too_many_jobs_with_invalid_argument(lib):
    arr = jobs(1025)
    assert visibility(lib, n=1025, arr=arr, ws_bytes=1 << 20) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert shade(lib, n=1025, arr=arr, ws_bytes=1 << 20) == _lib.PGR_ERR_INVALID_ARGUMENT
    big = jobs(1, faces=(1 << 22) + 1)
    assert visibility(lib, n=1, arr=big, nf=1 << 23, ws_bytes=1 << 20) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert shade(lib, n=1, arr=big, nf=1 << 23, ws_bytes=1 << 20) == _lib.PGR_ERR_INVALID_ARGUMENT


def test_visibility_refuses_bad_arguments_before_any_launch(lib):
    for kw in (dict(keys=None), dict(cnt=None), dict(v=None), dict(f=None), dict(n_slots=0), dict(W=0), dict(H=8193), dict(near=0.0),
               dict(near=float("nan")), dict(nv=4), dict(nf=3), dict(keys=C.c_void_p(4100)), dict(arr=jobs(2, slot=1))):
        assert visibility(lib, **kw) == _lib.PGR_ERR_INVALID_ARGUMENT, kw
    need = lib.pgr_mesh_visibility_workspace_bytes(2, jobs(2))
    assert visibility(lib, ws_bytes=need - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert visibility(lib, ws=None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL


def test_shade_refuses_bad_arguments_before_any_launch(lib):
    for kw in (dict(keys=None), dict(params=None), dict(v=None), dict(f=None), dict(n_slots=0), dict(W=0), dict(H=8193), dict(near=-1.0),
               dict(nv=4), dict(nf=3), dict(keys=C.c_void_p(4100)), dict(arr=jobs(2, slot=1)), dict(ws=C.c_void_p(4098)),
               dict(params=_lib.PgrMeshShade(ambient=float("nan"), rgb=FAKE))):
        assert shade(lib, **kw) == _lib.PGR_ERR_INVALID_ARGUMENT, kw
    need = lib.pgr_mesh_shade_workspace_bytes(2, jobs(2))
    assert shade(lib, ws_bytes=need - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert shade(lib, ws=None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL


def test_python_refuses_what_it_can_see_without_a_device():
    import numpy as np
    from pegasus_amd import mesh_render as R
    ms = R.MeshSet({1: type("M", (), dict(vertices=np.zeros((3, 3), np.float32), faces=np.array([[0, 1, 2]], np.int32)))()}, device="cpu")
    assert ms.normals is None and ms.colors is None
    K = np.eye(3)
    with pytest.raises(ValueError, match="phong"):
        R.render(ms, [(1, np.eye(3), np.zeros(3))], K, (8, 8))
    with pytest.raises(ValueError, match="outputs"):
        R.render(ms, [(1, np.eye(3), np.zeros(3))], K, (8, 8), outputs=("colour",), shading="flat")
    with pytest.raises(ValueError, match="shading"):
        R.render(ms, [(1, np.eye(3), np.zeros(3))], K, (8, 8), shading="gouraud")
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.render(ms, [(1, np.eye(3), np.zeros(3))], K, (8, 8), shading="flat")
    with pytest.raises(ValueError, match="at most 1024"):
        list(R._slot_chunks([0] * 1025, 4))
    assert list(R._slot_chunks([0, 1, 0, 2, 1], 2)) == [([0, 1, 2, 4], [0, 1]), ([3], [2])]
    assert [len(k) for k, _ in R._slot_chunks(list(range(2500)), 10 ** 6)] == [1024, 1024, 452]
