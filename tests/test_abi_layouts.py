"""The host side of the C ABI, without a device: every size function returns what tests/golden/abi_sizes.json recorded from
the library before its layout code was gathered into one function per buffer -- except the three rasterizer workspaces,
which lost the two per-view slots nothing ever read (a 256-byte camera and a 64-byte counter block aligned up to 256);
invalid arguments still size to 0; and the package reaches the current stream through pegasus_amd/_lib.py only.  The size
functions of the evaluation entries (mesh depth, ADI, masks, COCO scores) were recorded just before THEIR layouts were gathered
and compare for equality; workspaces are sized through _lib.workspace except where a module keeps a policy of its own."""
import ast
import ctypes as C
import json
import re
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
# the evaluation entries: counts on either side of every max(.., 1) floor and of the first 256-byte unit (10 and 11 groups of 24
# bytes), limits and one past
COUNTS = (-1, 0, 1, 2, 10, 11, 1000)
N_AREA = (0, 1, 64, 65)                                            # PGR_COCO_MAX_LANES and one past
N_MAX_DETS = (0, 1, 8, 9)                                          # PGR_COCO_MAX_MAXDETS and one past
RLE_TOTALS = (-1, 0, 1, 1000, 1 << 40, (1 << 40) + 1)
MASK_SIDES = (1, 31, 33, 255, 257, 8192, 8193)                       # see test_golden_covers_the_grid
MESH_FACE_COUNTS = ((0,), (1,), (256, 257), tuple(1000 * (k + 1) for k in range(40)), (1 << 22,), ((1 << 22) + 1,))
JOB_FIELD = {"pgr_mesh_depth_workspace_bytes": ("PgrMeshJob", "face_count"),
             "pgr_pose_adi_workspace_bytes": ("PgrPoseErrorJob", "vertex_count")}


def adi_vertex_counts():
    """One job at and around the tile of pose_adi_kernel (one partial sum per tile), a large one, and all of them in one call."""
    tile = int(re.search(r"constexpr int ADI_TILE = (\d+);", (ROOT / "pegasus_amd" / "csrc" / "poseerr.hip.h").read_text())[1])
    single = (1, tile - 1, tile, tile + 1, 100000)
    return tuple((v,) for v in single) + (single,)


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
        # the two that take jobs: one tuple of face / vertex counts per call (evaluate() makes the job array)
        "pgr_mesh_depth_workspace_bytes": list(MESH_FACE_COUNTS),
        "pgr_pose_adi_workspace_bytes": list(adi_vertex_counts()),
        "pgr_mask_rle_workspace_bytes": [(n, w, h) for n in (0, 1, 2) for w in MASK_SIDES for h in MASK_SIDES],
        "pgr_rle_iou_workspace_bytes": [(g, d, t) for g in COUNTS for d in RLE_TOTALS for t in RLE_TOTALS],
        "pgr_box_iou_workspace_bytes": [(g,) for g in COUNTS],
        "pgr_coco_match_workspace_bytes": [(g, n, a) for g in COUNTS for n in COUNTS for a in N_AREA],
        "pgr_coco_accumulate_workspace_bytes": [(n, a, m) for n in COUNTS for a in N_AREA for m in N_MAX_DETS],
    }


def evaluate(lib, skip=()) -> dict:
    """name -> results of cases() from ``lib`` (without the names in ``skip``); a record layout is its four fields."""
    from pegasus_amd import _lib
    out = {}
    for name, arg_list in cases().items():
        if name in skip:
            continue
        if name in JOB_FIELD:
            struct, fld = (getattr(_lib, JOB_FIELD[name][0]), JOB_FIELD[name][1])
            out[name] = [int(getattr(lib, name)(len(counts), (struct * len(counts))(*[struct(**{fld: c}) for c in counts])))
                         for counts in arg_list]
        elif name == "pgr_frame_record_layout":
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
    from pegasus_amd import _lib
    # the mask sides lie around the shapes at which the mask kernels change path, and around the largest side
    assert MASK_SIDES == (1, _lib.PGR_RLE_WORD_ROWS - 1, _lib.PGR_RLE_WORD_ROWS + 1, _lib.PGR_RLE_TILE_COLS - 1,
                          _lib.PGR_RLE_TILE_COLS + 1, 8192, 8193)
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


# modules that size a workspace themselves because they do more than allocate it: a cached buffer that grows, slack bytes, a
# memory estimate
OWN_WORKSPACE_POLICY = {"pegasus_amd/rasterizer.py", "pegasus_amd/pose_queue.py", "pegasus_amd/mesh.py",
                        "pegasus_amd/diff_gaussian_rasterization/__init__.py"}


def test_workspaces_are_sized_in_one_place():
    """Asking a size function, refusing 0 and allocating the bytes is _lib.workspace: no other module of the package names
    an attribute that ends in _workspace_bytes, except those with a policy of their own."""
    users = set()
    for path in sorted((ROOT / "pegasus_amd").rglob("*.py")):
        for node in ast.walk(ast.parse(path.read_text(), filename=str(path))):
            if isinstance(node, ast.Attribute) and node.attr.endswith("_workspace_bytes"):
                users.add(path.relative_to(ROOT).as_posix())
    assert users <= OWN_WORKSPACE_POLICY | {"pegasus_amd/_lib.py"}


if __name__ == "__main__":
    # records what the golden file lacks, and never touches what it holds: run with PGR_LIB pointing at a build of the library
    # as it was BEFORE the layouts of the missing functions moved
    import sys
    sys.path.insert(0, str(ROOT))
    from pegasus_amd import _lib
    recorded = json.loads(GOLDEN.read_text())
    recorded.update(evaluate(_lib.lib(), skip=set(recorded)))
    GOLDEN.write_text(json.dumps(recorded, separators=(",", ":")) + "\n")
