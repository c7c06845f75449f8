"""The host side of the C ABI, without a device: every size function returns what tests/golden/abi_sizes.json recorded from
the library before its layout code was gathered into one function per buffer -- except the three rasterizer workspaces,
which lost the two per-view slots nothing ever read (a 256-byte camera and a 64-byte counter block aligned up to 256);
invalid arguments still size to 0; and the package reaches the current stream through pegasus_amd/_lib.py only."""
import ast
import ctypes as C
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "abi_sizes.json"

NS = (0, 1, 63, 64, 65, 4096, 4097, 100000)
IMAGES = ((1, 1), (16, 16), (17, 33), (800, 800))                  # width, height
MAX_INSTANCES = (0, 1, 1 << 20)
N_VIEWS = (1, 2, 3, 16, 17, 33)
LAYERS = (1, 8)
KS = (0, 1, 8, 9)
GRIDS = ((2, 2, 2), (3, 5, 7), (64, 64, 64), (65, 33, 17), (256, 256, 256))     # nx, ny, nz
DEAD_SLOT_BYTES = 512                                              # per view: align_up(256) + align_up(64)
SHRUNK = ("pgr_workspace_bytes", "pgr_batch_workspace_bytes", "pgr_layers_workspace_bytes")


def cases() -> dict:
    """name -> argument tuples, in the order the golden file lists the results."""
    scenes = [(n, w, h, mi) for n in NS for w, h in IMAGES for mi in MAX_INSTANCES]
    n_nv = [(n, nv) for n in NS for nv in N_VIEWS]
    return {
        "pgr_workspace_bytes": scenes,
        "pgr_batch_workspace_bytes": [s + (nv,) for s in scenes for nv in N_VIEWS],
        "pgr_layers_workspace_bytes": [s + (nv, ly) for s in scenes for nv in N_VIEWS for ly in LAYERS],
        "pgr_host_scratch_bytes": [(nv,) for nv in N_VIEWS],
        "pgr_scene_cache_bytes": [(n,) for n in NS],
        "pgr_backward_batch_scratch_bytes": n_nv,
        "pgr_camera_grad_scratch_bytes": n_nv,
        "pgr_pose_objects_workspace_bytes": [(j,) for j in N_VIEWS],
        "pgr_block_visibility_workspace_bytes": n_nv,
        "pgr_knn_workspace_bytes": [(n,) for n in NS],
        "pgr_march_workspace_bytes": list(GRIDS),
        "pgr_image_loss_workspace_bytes": [(h, w) for w, h in IMAGES],
        "pgr_image_loss_masked_workspace_bytes": [(h, w) for w, h in IMAGES],
        "pgr_frame_record_layout": [(w, h, k) for w, h in IMAGES for k in KS],
    }


def evaluate(lib) -> dict:
    """name -> results of cases() from ``lib``; a record layout is its four fields."""
    out = {}
    for name, arg_list in cases().items():
        if name == "pgr_frame_record_layout":
            rows = []
            for args in arg_list:
                lay = _record_layout_struct()
                assert lib.pgr_frame_record_layout(*args, C.byref(lay)) == 0
                rows.append([int(lay.off_rgb), int(lay.off_depth), int(lay.off_masks), int(lay.bytes)])
            out[name] = rows
        else:
            out[name] = [int(getattr(lib, name)(*args)) for args in arg_list]
    return out


def _record_layout_struct():
    from pegasus_amd import _lib
    return _lib.PgrRecordLayout()


@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import _lib, build
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def sizes(lib):
    return evaluate(lib)


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_golden_covers_the_grid(golden):
    assert set(golden) == set(cases())
    for name, arg_list in cases().items():
        assert len(golden[name]) == len(arg_list), name


@pytest.mark.parametrize("name", sorted(cases()))
def test_sizes_match_the_recorded_ones(sizes, golden, name):
    if name not in SHRUNK:
        assert sizes[name] == golden[name]
        return
    for args, was, now in zip(cases()[name], golden[name], sizes[name]):
        n_views = 1 if name == "pgr_workspace_bytes" else args[4]
        assert now == was - DEAD_SLOT_BYTES * n_views, (name, args, was, now)


def test_invalid_arguments_still_size_to_zero(lib):
    assert lib.pgr_workspace_bytes(-1, 16, 16, 1) == 0
    assert lib.pgr_workspace_bytes(1, 0, 16, 1) == 0 and lib.pgr_workspace_bytes(1, 16, 0, 1) == 0
    for nv in (0, -1):
        assert lib.pgr_batch_workspace_bytes(1, 16, 16, 1, nv) == 0
        assert lib.pgr_layers_workspace_bytes(1, 16, 16, 1, nv, 1) == 0
        assert lib.pgr_host_scratch_bytes(nv) == 0
        assert lib.pgr_backward_batch_scratch_bytes(1, nv) == 0
        assert lib.pgr_camera_grad_scratch_bytes(1, nv) == 0
        assert lib.pgr_block_visibility_workspace_bytes(1, nv) == 0
        assert lib.pgr_pose_objects_workspace_bytes(nv) == 0
    assert lib.pgr_batch_workspace_bytes(-1, 16, 16, 1, 1) == 0
    assert lib.pgr_batch_workspace_bytes(1, 0, 16, 1, 1) == 0 and lib.pgr_batch_workspace_bytes(1, 16, 0, 1, 1) == 0
    assert lib.pgr_layers_workspace_bytes(-1, 16, 16, 1, 1, 1) == 0
    assert lib.pgr_layers_workspace_bytes(1, 0, 16, 1, 1, 1) == 0 and lib.pgr_layers_workspace_bytes(1, 16, 0, 1, 1, 1) == 0
    assert lib.pgr_layers_workspace_bytes(1, 16, 16, 1, 1, 4097) == 0
    assert lib.pgr_layers_workspace_bytes(1, 16, 16, 1, 1, 4096) != 0
    for fn in ("pgr_scene_cache_bytes", "pgr_knn_workspace_bytes"):
        assert getattr(lib, fn)(-1) == 0
    for fn in ("pgr_backward_batch_scratch_bytes", "pgr_camera_grad_scratch_bytes", "pgr_block_visibility_workspace_bytes"):
        assert getattr(lib, fn)(-1, 1) == 0
    for fn in ("pgr_image_loss_workspace_bytes", "pgr_image_loss_masked_workspace_bytes"):
        assert getattr(lib, fn)(0, 16) == 0 and getattr(lib, fn)(16, 0) == 0
    assert lib.pgr_march_workspace_bytes(1, 2, 2) == 0
    lay = _record_layout_struct()
    for bad in ((0, 16, 1), (16, 0, 1), (16, 16, -1)):
        assert lib.pgr_frame_record_layout(*bad, C.byref(lay)) == -1


def test_the_current_stream_is_asked_for_in_one_place():
    """Which stream and device an entry point runs on is decided by _lib.enqueue alone: no other module of the package names
    stream_ptr, as a variable, an attribute or an import."""
    users = set()
    for path in sorted((ROOT / "pegasus_amd").rglob("*.py")):
        for node in ast.walk(ast.parse(path.read_text(), filename=str(path))):
            names = {ast.Name: lambda n: [n.id], ast.Attribute: lambda n: [n.attr], ast.FunctionDef: lambda n: [n.name],
                     ast.ImportFrom: lambda n: [a.name for a in n.names]}.get(type(node), lambda n: [])(node)
            if "stream_ptr" in names:
                users.add(path.relative_to(ROOT).as_posix())
    assert users == {"pegasus_amd/_lib.py"}


if __name__ == "__main__":
    # records the golden file: run with PGR_LIB pointing at a build of the library as it was BEFORE the layouts moved
    import sys
    sys.path.insert(0, str(ROOT))
    from pegasus_amd import _lib
    GOLDEN.write_text(json.dumps(evaluate(_lib.lib()), separators=(",", ":")) + "\n")
