"""pegasus_amd.bop_dataset without a device: scene discovery, the record files byte for byte, the record fields, the PNG
header and codec, the models directory, and bop_pose.broadcast_K that mesh_render and pose_error share."""
import json
from pathlib import Path

import numpy as np
import pytest

from pegasus_amd import bop_dataset as BD
from pegasus_amd import dataset_writer as DW

COCO = "scene_gt_coco.json"


def test_the_module_is_host_only():
    """Its module-level imports are the standard library and NumPy: no torch, no library."""
    import ast
    tree = ast.parse(Path(BD.__file__).read_text())
    names = {a.name.split(".")[0] for n in tree.body if isinstance(n, ast.Import) for a in n.names}
    names |= {"." * n.level + (n.module or "") for n in tree.body if isinstance(n, ast.ImportFrom)}
    assert names <= {"__future__", "json", "re", "struct", "zlib", "functools", "pathlib", "numpy"}, names


# ---- discovery ------------------------------------------------------------------------------------------------------
@pytest.fixture()
def dataset(tmp_path):
    """train/ with 000000 and 000002 (scene_gt.json), 000001 (without), notes/ (with) and a plain file 000003; the COCO file
    in 000000 and notes only."""
    train = tmp_path / "ds" / "train"
    for name, files in (("000000", ("scene_gt.json", COCO)), ("000002", ("scene_gt.json",)), ("000001", ()),
                        ("notes", ("scene_gt.json", COCO))):
        (train / name).mkdir(parents=True)
        for f in files:
            doc = {"images": [{"id": 7 if name == "notes" else 0}], "annotations": [], "categories": [{"id": 1}]} if f == COCO else {}
            (train / name / f).write_text(json.dumps(doc))
    (train / "000003").write_text("a file, not a scene")
    return tmp_path / "ds"


def test_scene_dirs_are_sorted_and_filtered_by_the_file_only(dataset):
    assert [p.name for p in BD.scene_dirs(dataset)] == ["000000", "000002", "notes"]
    assert BD.scene_dirs(dataset, "train", "scene_gt.json") == BD.scene_dirs(dataset)
    assert [p.name for p in BD.scene_dirs(dataset, having=COCO)] == ["000000", "notes"]
    assert BD.scene_dirs(dataset)[0] == dataset / "train" / "000000" == BD.scene_dir(dataset, "train", 0)
    assert BD.scene_dir(dataset, "test", 12).parts[-2:] == ("test", "000012")
    with pytest.raises(FileNotFoundError):
        BD.scene_dirs(dataset, "test")


def test_load_dataset_keeps_its_numeric_filter(dataset):
    from pegasus_amd import coco_eval as CE
    gt, dt = CE.load_dataset([], dataset, "bbox", targets=None)
    assert [i["id"] for i in gt["images"]] == [0] and dt == []                   # notes/ (image 7) is left out


def test_names():
    assert BD.image_name(7) == BD.image_name("7") == "000007.png" and BD.image_name(7, 12) == "000007_000012.png"
    assert BD.scene_name(3) == "000003" and BD.model_stem(21) == "obj_000021"
    assert (BD.SCENE_GT, BD.SCENE_CAMERA, BD.SCENE_GT_INFO, BD.MODELS_INFO) == (
        "scene_gt.json", "scene_camera.json", "scene_gt_info.json", "models_info.json")
    scene = BD.BopScene("/x/train/000001")
    assert str(scene.image_path("depth", "10")) == "/x/train/000001/depth/000010.png"
    assert str(scene.image_path("mask_visib", 10, 2)) == "/x/train/000001/mask_visib/000010_000002.png"


# ---- records --------------------------------------------------------------------------------------------------------
def test_record_files_are_json_dumps_byte_for_byte(tmp_path):
    scene = BD.BopScene(tmp_path)
    docs = {BD.SCENE_GT: {"10": [], "9": [{"obj_id": 3, "cam_t_m2c": [0.1, -2.0, 1e-7]}], "0": []},
            BD.SCENE_CAMERA: {"0": {"cam_K": [1.5, 0, 2, 0, 1.5, 1, 0, 0, 1], "depth_scale": 0.1}},
            BD.SCENE_GT_INFO: {"0": [{"visib_fract": 1 / 3, "bbox_obj": [-1, -1, -1, -1]}]}}
    assert scene.gt_info is None
    for name, doc in docs.items():
        scene.write_json(name, doc)
        assert (tmp_path / name).read_bytes() == json.dumps(doc).encode()         # compact, no trailing newline
    fresh = BD.BopScene(tmp_path)
    assert (fresh.gt, fresh.camera, fresh.gt_info) == tuple(docs.values())
    assert scene.gt_info is None                                                   # read once: the old object keeps its answer
    assert fresh.image_ids == ["0", "9", "10"] and list(fresh.gt) == ["10", "9", "0"]
    assert list(BD.by_frame(docs[BD.SCENE_GT])) == ["0", "9", "10"] and BD.by_frame(docs[BD.SCENE_GT]) == docs[BD.SCENE_GT]


# ---- fields ---------------------------------------------------------------------------------------------------------
def test_record_fields():
    K = BD.cam_K({"cam_K": [1, 2, 3, 4, 5, 6, 7, 8, 9]})
    assert K.dtype == np.float64 and K.shape == (3, 3) and K[0].tolist() == [1.0, 2.0, 3.0] and K[2, 0] == 7.0
    R, t = BD.pose_of({"cam_R_m2c": [0, 1, 0, 1, 0, 0, 0, 0, -1], "cam_t_m2c": [1, 2, 3]})
    assert (R.dtype, R.shape, t.dtype, t.shape) == (np.float64, (3, 3), np.float64, (3,))
    assert R[0].tolist() == [0.0, 1.0, 0.0] and t.tolist() == [1.0, 2.0, 3.0]
    assert BD.depth_unit({}, 0.001) == 0.001 and BD.depth_unit({"depth_scale": 1}, 2.5) == 2.5
    d = BD.depth_unit({"depth_scale": 0.1}, 0.001)
    assert type(d) is float and d == 0.1 * 0.001
    assert BD.unit_of(1) == 0.001 and BD.unit_of(1000.0) == 1.0 and type(BD.unit_of(np.float32(1))) is float


# ---- PNG ------------------------------------------------------------------------------------------------------------
def png_images():
    rng = np.random.default_rng(5)
    return {"grey": rng.integers(0, 256, (3, 5), dtype=np.uint8),                 # H x W: 5 wide, 3 high
            "rgb": rng.integers(0, 256, (2, 7, 3), dtype=np.uint8),
            "depth": rng.integers(0, 65536, (9, 4), dtype=np.uint16)}


def test_png_size_is_width_then_height(tmp_path):
    for name, a in png_images().items():
        (tmp_path / name).write_bytes(BD.encode_png(a))
        assert BD.png_size(tmp_path / name) == (a.shape[1], a.shape[0]), name
    assert {n: BD.png_size(tmp_path / n) for n in png_images()} == {"grey": (5, 3), "rgb": (7, 2), "depth": (4, 9)}
    (tmp_path / "zeros").write_bytes(bytes(30))
    assert BD.png_size(tmp_path / "zeros") is None


def test_png_codec_round_trips_and_stays_importable_from_the_writer():
    assert DW.encode_png is BD.encode_png and DW.decode_png is BD.decode_png
    for name, a in png_images().items():
        back = BD.decode_png(BD.encode_png(a))
        assert back.dtype == a.dtype and back.shape == a.shape and np.array_equal(back, a), name
    with pytest.raises(ValueError, match="encode_png takes"):
        BD.encode_png(np.zeros((2, 2), np.float32))


def test_scene_image_sizes(tmp_path):
    scene = BD.BopScene(tmp_path)
    assert scene.first_image_size() is None and scene.image_size(0) == (0, 0)      # no directories at all
    scene.make_dirs()
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(BD.IMAGE_KINDS)
    scene.image_path("depth", 4).write_bytes(BD.encode_png(np.zeros((9, 4), np.uint16)))
    assert scene.first_image_size() == (4, 9) and np.array_equal(scene.read_png("depth", 4), np.zeros((9, 4), np.uint16))
    scene.image_path("rgb", 2).write_bytes(bytes(30))                             # no PNG: passed over
    assert scene.first_image_size() == (4, 9)
    scene.image_path("rgb", 3).write_bytes(BD.encode_png(np.zeros((2, 7, 3), np.uint8)))
    assert scene.first_image_size() == (7, 2) and scene.image_size(3) == (7, 2) and scene.image_size(4) == (0, 0)


# ---- models ---------------------------------------------------------------------------------------------------------
def test_models_directory(tmp_path):
    with pytest.raises(FileNotFoundError, match=f"no obj_NNNNNN.ply under {tmp_path}"):
        BD.model_files(tmp_path)
    assert BD.read_models_info(tmp_path) == {}
    for name in ("obj_000002.ply", "obj_000010.ply", "obj_abc.ply", "obj_000003.ply.bak"):
        (tmp_path / name).write_text("ply")
    files = BD.model_files(str(tmp_path))
    assert files == {2: tmp_path / "obj_000002.ply", 10: tmp_path / "obj_000010.ply"} and list(files) == [2, 10]
    info = {"10": {"diameter": 2.5}, "2": {"diameter": 1.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}
    (tmp_path / "models_info.json").write_text(json.dumps(info, indent=2) + "\n")
    assert BD.read_models_info(tmp_path) == info and list(BD.read_models_info(tmp_path)) == ["10", "2"]


# ---- K --------------------------------------------------------------------------------------------------------------
def test_broadcast_K():
    from pegasus_amd.bop_pose import broadcast_K
    K = [[500, 0, 320], [0, 510, 240], [0, 0, 1]]
    out = broadcast_K(K, 4)
    assert out.dtype == np.float64 and out.shape == (4, 3, 3) and all(np.array_equal(k, np.asarray(K, np.float64)) for k in out)
    assert broadcast_K(K, 0).shape == (0, 3, 3)
    each = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    out = broadcast_K(each, 2)
    assert out.dtype == np.float64 and np.array_equal(out, each)
    for bad, n in ((np.zeros((3, 3, 3)), 2), (np.zeros((2, 3, 3)), 3), (np.zeros(9), 1)):
        with pytest.raises(ValueError, match=rf"K must be \[3,3\] or \[{n},3,3\]"):
            broadcast_K(bad, n)


def test_intrinsics_still_refuses_shape_and_skew():
    """What tests/test_pose_error_host.py asserts of PE.intrinsics, on top of the shared broadcast."""
    from pegasus_amd import pose_error as PE
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    assert PE.intrinsics(K, 2).tolist() == [[572.4114, 573.57043, 325.2611, 242.04899]] * 2
    with pytest.raises(ValueError, match=r"K must be \[3,3\] or \[2,3,3\]"):
        PE.intrinsics(np.zeros((3, 3, 3)), 2)
    skew = K.copy()
    skew[0, 1] = 0.5
    with pytest.raises(ValueError, match="skew"):
        PE.intrinsics(skew, 2)
    assert not hasattr(PE, "_K_list")
