"""pgr_mesh_cluster_*: the argument checks come before any launch, so they run without a device (the pointers handed in
are never dereferenced), and the workspace size is a host-only function."""
import ctypes as C

import pytest

from pegasus_amd import _lib

FAKE = C.c_void_p(4096)          # non-NULL and 16-byte aligned; a call that got as far as using it would fault
GRID = (0.5, -0.25, -0.25, -0.25)


@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import build
    build.build()
    return _lib.lib()


def count(lib, nv=8, v=FAKE, nf=4, f=FAKE, grid=GRID, ws=FAKE, ws_bytes=None, counts=FAKE):
    if ws_bytes is None:
        ws_bytes = lib.pgr_mesh_cluster_workspace_bytes(max(nv, 0), max(nf, 0))
    return lib.pgr_mesh_cluster_count(nv, v, nf, f, *grid, ws, ws_bytes, counts, None)


def emit(lib, nv=8, v=FAKE, nf=4, f=FAKE, grid=GRID, contraction=1, ws=FAKE, ws_bytes=None, k=3, nfo=2, ov=FAKE, of=FAKE,
         cov=FAKE, used=FAKE):
    if ws_bytes is None:
        ws_bytes = lib.pgr_mesh_cluster_workspace_bytes(max(nv, 0), max(nf, 0))
    return lib.pgr_mesh_cluster_emit(nv, v, nf, f, *grid, contraction, ws, ws_bytes, k, nfo, ov, of, cov, used, None)


def test_workspace_size_is_host_only_and_grows_with_both_counts(lib):
    size = lib.pgr_mesh_cluster_workspace_bytes
    assert size(1, 0) > 0 and size(0, 0) > 0
    assert size(1000, 2000) > size(1000, 1000) > size(500, 1000)
    assert size(1000, 2000) >= 2 * 8 * 6000 + 2 * 4 * 6000                      # two key and two value buffers of 3 F corners
    assert size(-1, 0) == 0 and size(0, -1) == 0
    assert size((1 << 30) + 1, 0) == 0 and size(8, (2 ** 31 - 1) // 3 + 1) == 0  # 3 F must stay below 2^31


def test_count_refuses_null_pointers(lib):
    for kw in (dict(v=None), dict(f=None), dict(ws=None), dict(counts=None)):
        assert count(lib, **kw) == _lib.PGR_ERR_INVALID_ARGUMENT, kw
    assert count(lib, ws=C.c_void_p(4104)) == _lib.PGR_ERR_INVALID_ARGUMENT      # not 16-byte aligned
    assert count(lib, nv=-1) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert count(lib, nf=-1) == _lib.PGR_ERR_INVALID_ARGUMENT


def test_emit_refuses_null_pointers_and_bad_counts(lib):
    for kw in (dict(v=None), dict(f=None), dict(ws=None), dict(ov=None), dict(of=None), dict(cov=None), dict(used=None)):
        assert emit(lib, **kw) == _lib.PGR_ERR_INVALID_ARGUMENT, kw
    assert emit(lib, contraction=2) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert emit(lib, contraction=-1) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert emit(lib, k=9) == _lib.PGR_ERR_INVALID_ARGUMENT                       # more clusters than vertices
    assert emit(lib, nfo=5) == _lib.PGR_ERR_INVALID_ARGUMENT                     # more faces out than in
    assert emit(lib, k=-1) == _lib.PGR_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("voxel", [0.0, -1.0, float("nan"), float("inf")])
def test_a_voxel_that_is_not_finite_and_positive_is_refused(lib, voxel):
    grid = (voxel,) + GRID[1:]
    assert count(lib, grid=grid) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert emit(lib, grid=grid) == _lib.PGR_ERR_INVALID_ARGUMENT


def test_an_origin_that_is_not_finite_is_refused(lib):
    assert count(lib, grid=(0.5, float("nan"), 0.0, 0.0)) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert emit(lib, grid=(0.5, 0.0, float("-inf"), 0.0)) == _lib.PGR_ERR_INVALID_ARGUMENT


def test_a_short_workspace_is_refused(lib):
    need = lib.pgr_mesh_cluster_workspace_bytes(8, 4)
    assert count(lib, ws_bytes=need - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert emit(lib, ws_bytes=need - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert count(lib, ws_bytes=0) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL


def test_python_refuses_what_the_library_cannot_see():
    """The domain and the face indices are the caller's contract: pegasus_amd.decimate checks them with one reduction each.
    Without a device the device check comes first, so this only pins the order of the host-side checks."""
    import torch
    from pegasus_amd import decimate as D
    with pytest.raises(ValueError, match=r"\[V,3\]"):
        D.cluster_vertices(torch.zeros((4, 2)), torch.zeros((1, 3), dtype=torch.int32), 1.0)
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        D.cluster_vertices(torch.zeros((4, 3)), torch.zeros((1, 4), dtype=torch.int32), 1.0)
