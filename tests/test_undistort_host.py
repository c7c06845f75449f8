"""The undistortion rule and its files without a device: the camera rule on hand-worked numbers, the models
that are refused, colmap_io's observations and tracks, and the share of near-tie pixels in the fixtures of the GPU tests.  The
NumPy reference (tests/undistort_reference.py) stands in for the device through the ``backend`` argument."""
import ctypes as C
import json
import struct

import numpy as np
import pytest

import undistort_reference as ref
from pegasus_amd import colmap_io, undistort
from pegasus_amd.colmap_io import ColmapCamera, ColmapImage, UnsupportedCameraModel

BACKEND = ref.Backend()


def cam(model, w, h, fx, fy, cx, cy, coeffs=None, cid=7):
    return ColmapCamera(cid, model, w, h, ref.camera_params(model, fx, fy, cx, cy, coeffs))


def rule(camera, **kw):
    return undistort.undistort_camera(camera, backend=BACKEND, **kw)


def radial_root(k, rd):
    """The undistorted radius of the distorted radius rd under r (1 + k r^2) = rd, by the cubic's roots (independent of the
    Newton iteration): the smallest positive real root is the one on the sheet through the origin."""
    roots = np.roots([k, 0.0, 1.0, -rd])
    real = roots[np.abs(roots.imag) < 1e-12].real
    return real[real > 0].min()


# ---- the camera rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sorted(set(ref.SHAPES) - {"OPENCV_FISHEYE"}))
def test_zero_distortion_is_the_identity_camera(model):
    """Every coefficient 0: the border stays where it is, the scale is exactly 1 and the size is the source's, for focal
    lengths and principal points that are no round numbers.  (OPENCV_FISHEYE has no zero distortion: with every coefficient 0
    it is the equidistant projection, the next test.)"""
    zeros = [0.0] * ref.SHAPES[model][1]
    c = cam(model, 41, 23, 37.3, 37.3 if ref.SHAPES[model][0] == 1 else 35.9, 19.7, 12.1, zeros)
    fx, fy = c.distorted_focal
    keep = rule(c, principal_point="keep")
    assert (keep.model, keep.width, keep.height) == ("PINHOLE", 41, 23)
    assert keep.params.tolist() == [fx, fy, 19.7, 12.1]                       # unchanged, to the bit
    centred = cam(model, 41, 23, 37.3, 37.3 if ref.SHAPES[model][0] == 1 else 35.9, 20.5, 11.5, zeros)
    for mode in ("center", "keep"):
        out = rule(centred, principal_point=mode, blank_pixels=1.0)
        assert (out.width, out.height) == (41, 23) and out.params.tolist() == [fx, fy, 20.5, 11.5]


def test_fisheye_without_coefficients_is_the_equidistant_projection():
    """theta_d = theta: a distorted radius r_d comes from r = tan(r_d).  The left border's middle, x_d = -a with a = 20.5 / 37.3,
    goes to u = -tan(a): the innermost point of the undistorted border, so scale_x = tan(a) / a."""
    c = cam("OPENCV_FISHEYE", 41, 23, 37.3, 37.3, 20.5, 11.5, [0.0] * 4)
    out = rule(c, principal_point="keep")
    a, b = 20.5 / 37.3, 11.5 / 37.3
    assert out.width == int(np.floor(np.tan(a) / a * 41)) > 41 and out.height == int(np.floor(np.tan(b) / b * 23))


def test_center_mode_moves_the_principal_point_to_the_centre():
    c = cam("SIMPLE_RADIAL", 40, 30, 50.0, 50.0, 22.0, 13.0, [-0.05])
    out = rule(c)                                                              # "center" is the default
    assert out.params[2] == out.width / 2.0 and out.params[3] == out.height / 2.0
    assert out.params[0] == 50.0 and out.params[1] == 50.0


# w = 41, h = 21, f = 20.5, principal point (20.5, 10.5): the left border's middle sample (0, 10.5) is x_d = (-1, 0).
W0, H0, F0 = 41, 21, 20.5


def test_barrel_simple_radial_by_hand():
    """k < 0.  Choose the undistorted middle of the left border, u0 = -1.125: u0 (1 + k u0^2) = -1 gives
    k = (1 / 1.125 - 1) / 1.125^2 = -0.0877914951989026.  Barrel distortion pulled the corners in further than the middle, so
    undistorted the middle is the border's innermost point: left_max = 20.5 (-1.125) + 20.5 = -2.5625, and by symmetry
    right_min = 41 + 2.5625.  max_scale_x = 20.5 / (20.5 + 2.5625) = 1 / 1.125, so with blank_pixels = 0
    scale_x = 1.125 and W' = floor(1.125 * 41) = floor(46.125) = 46.
    left_min is at the corners (0, 0), (0, 21): x_d = (-1, -10.5 / 20.5), r_d = 1.12354..; the cubic k r^3 + r - r_d = 0 gives r
    and the corner goes to x_d r / r_d; with blank_pixels = 1 scale_x = (20.5 - left_min) / 20.5."""
    k = (1.0 / 1.125 - 1.0) / 1.125 ** 2
    c = cam("SIMPLE_RADIAL", W0, H0, F0, F0, 20.5, 10.5, [k])
    uv, ok = ref.undistort_points(c.model, c.params, [[0.0, 10.5], [0.0, 0.0]])
    assert ok.all() and abs(uv[0, 0] + 1.125) < 1e-12 and abs(uv[0, 1]) < 1e-15
    tight = rule(c, principal_point="keep")
    assert tight.width == 46
    # y: the top border's middle (20.5, 0) is y_d = -10.5 / 20.5; its root by the cubic
    yd = 10.5 / F0
    scale_y = radial_root(k, yd) / yd                                          # (10.5 + 20.5 v) / 10.5 with top_max = cy - f v
    assert tight.height == int(np.floor(scale_y * H0))
    assert tight.params.tolist() == [F0, F0, 20.5 * 46 / 41, 10.5 * tight.height / 21]
    # blank_pixels = 1: the enclosing size, from the corners
    rd = np.hypot(1.0, yd)
    r = radial_root(k, rd)
    left_min = F0 * (-1.0 * r / rd) + 20.5
    assert abs(uv[1, 0] - (-r / rd)) < 1e-12
    wide = rule(c, principal_point="keep", blank_pixels=1.0)
    assert wide.width == int(np.floor((20.5 - left_min) / 20.5 * W0)) and wide.width > tight.width
    assert wide.height == int(np.floor(r / rd * H0)) and wide.height > tight.height     # top_min = cy - f (yd r / rd)
    # between: the harmonic blend of the rule
    half = rule(c, principal_point="keep", blank_pixels=0.5)
    s = 1.0 / ((20.5 / (20.5 - left_min)) * 0.5 + (1.0 / 1.125) * 0.5)
    assert half.width == int(np.floor(s * W0))


def test_pincushion_simple_radial_by_hand():
    """k > 0.  u0 = -0.875 for the middle of the left border: k = (1 / 0.875 - 1) / 0.875^2 = 0.18658892128279883.  Pincushion
    distortion pushed the corners out further, so undistorted the middle is the border's OUTERMOST point:
    left_min = 20.5 (-0.875) + 20.5 = 2.5625, min_scale_x = 20.5 / (20.5 - 2.5625) = 1 / 0.875; with blank_pixels = 1
    scale_x = 0.875 and W' = floor(0.875 * 41) = floor(35.875) = 35.  left_max is at the corners, by the cubic."""
    k = (1.0 / 0.875 - 1.0) / 0.875 ** 2
    c = cam("SIMPLE_RADIAL", W0, H0, F0, F0, 20.5, 10.5, [k])
    wide = rule(c, principal_point="keep", blank_pixels=1.0)
    assert wide.width == 35
    yd = 10.5 / F0
    rd = np.hypot(1.0, yd)
    r = radial_root(k, rd)
    left_max = F0 * (-r / rd) + 20.5
    tight = rule(c, principal_point="keep")
    assert tight.width == int(np.floor((20.5 - left_max) / 20.5 * W0)) and tight.width < wide.width


def test_scale_clamps_are_reached():
    """2.0: on its sheet r (1 + k r^2) stretches a radius by less than 1.5 (the ratio at the fold), so the upper clamp takes
    another model: OPENCV_FISHEYE without coefficients is r = tan(r_d).  With f = 20.5 / 1.2 the left middle is x_d = -1.2 and
    goes to -tan(1.2) = -2.5722: the scale tan(1.2) / 1.2 = 2.1435 is clamped to 2, W' = 82; with max_scale = 3 it is
    floor(2.1435 * 41) = 87.  (The corner's r_d = hypot(1.2, 0.6146) = 1.348 is below pi / 2.)
    0.2: f = 20.5, u0 = -0.1 gives k = (10 - 1) / 0.01 = 900 and left_min = 18.45: the scale 2.05 / 20.5 = 0.1 with
    blank_pixels = 1 is clamped to 0.2, W' = floor(8.2) = 8."""
    fish = cam("OPENCV_FISHEYE", W0, H0, 20.5 / 1.2, 20.5 / 1.2, 20.5, 10.5, [0.0] * 4)
    assert rule(fish, principal_point="keep").width == 82
    assert rule(fish, principal_point="keep", max_scale=3.0).width == 87 == int(np.floor(np.tan(1.2) / 1.2 * 41))
    down = rule(cam("SIMPLE_RADIAL", W0, H0, F0, F0, 20.5, 10.5, [900.0]), principal_point="keep", blank_pixels=1.0)
    assert down.width == 8
    assert rule(cam("SIMPLE_RADIAL", W0, H0, F0, F0, 20.5, 10.5, [900.0]), principal_point="keep", blank_pixels=1.0,
                min_scale=0.05).width == 4                                     # floor(4.1)


def test_max_image_size_and_multiple_of():
    k = (1.0 / 1.125 - 1.0) / 1.125 ** 2
    c = cam("SIMPLE_RADIAL", W0, H0, F0, F0, 20.5, 10.5, [k])
    full = rule(c, principal_point="keep")                                     # 46 x H
    small = rule(c, principal_point="keep", max_image_size=20)
    # both sizes times 20 / 46, floored; the focal lengths by the exact size ratios; the principal point by the final size
    assert small.width == 20 and small.height == int(np.floor(full.height * (20 / 46)))
    assert small.params.tolist() == [F0 * (20 / 46), F0 * (small.height / full.height), 20.5 * 20 / 41,
                                     10.5 * small.height / 21]
    assert rule(c, principal_point="keep", max_image_size=46).params.tolist() == full.params.tolist()
    # multiple_of: the crop is right and bottom in keep mode, symmetric in center mode
    keep8 = rule(c, principal_point="keep", multiple_of=8)
    assert (keep8.width, keep8.height) == (40, full.height - full.height % 8)
    assert keep8.params.tolist() == full.params.tolist()
    off = cam("SIMPLE_RADIAL", W0, H0, F0, F0, 19.0, 11.0, [k])
    centre8 = rule(off, multiple_of=8)
    assert centre8.width % 8 == 0 and centre8.height % 8 == 0
    assert centre8.params.tolist() == [F0, F0, centre8.width / 2.0, centre8.height / 2.0]
    with pytest.raises(ValueError, match="multiple of 64"):
        rule(c, multiple_of=64)


@pytest.mark.parametrize("model", ["FOV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"])
def test_unsupported_models_are_refused_by_name(model):
    n = colmap_io.CAMERA_MODELS[undistort.MODEL_IDS[model]][1]
    c = ColmapCamera(3, model, 40, 30, np.r_[[30.0] * (n - 2), [20.0, 15.0]][:n])
    with pytest.raises(UnsupportedCameraModel, match=model):
        rule(c)


def test_a_distortion_that_folds_inside_the_image_names_the_camera():
    """k = -1 at f = 20.5: r (1 - r^2) peaks at r_d = 0.385, the left border is at 1."""
    with pytest.raises(ValueError, match=r"camera 7 \(SIMPLE_RADIAL\).*not invertible"):
        rule(cam("SIMPLE_RADIAL", W0, H0, F0, F0, 20.5, 10.5, [-1.0]))


def test_the_inverse_never_returns_the_root_beyond_the_fold():
    """Every distorted point of r (1 + k r^2), k < 0, has a second preimage on the far side of the origin; the rule's sheet test
    keeps the iteration from landing there."""
    k = -0.5
    rd_max = (2.0 / 3.0) * np.sqrt(-1.0 / (3.0 * k))
    ang = np.linspace(0.0, 2 * np.pi, 97)
    for rd in (1.001 * rd_max, 1.5 * rd_max, 4.0, 50.0):
        uv, ok = ref.undistort_points("SIMPLE_RADIAL", [1.0, 0.0, 0.0, k], np.stack([rd * np.cos(ang), rd * np.sin(ang)], 1))
        assert not ok.any() and np.isnan(uv).all()
    inside = 0.95 * rd_max * np.stack([np.cos(ang), np.sin(ang)], 1)
    uv, ok = ref.undistort_points("SIMPLE_RADIAL", [1.0, 0.0, 0.0, k], inside)
    assert ok.all()
    np.testing.assert_allclose(np.hypot(uv[:, 0], uv[:, 1]), radial_root(k, 0.95 * rd_max), rtol=0, atol=1e-11)


# ---- colmap_io ------------------------------------------------------------------------------------------------------------
def model_with_observations():
    rng = np.random.default_rng(5)
    cams = {1: cam("OPENCV", 40, 30, 31.0, 32.0, 20.5, 14.5, cid=1), 2: cam("SIMPLE_RADIAL", 40, 30, 30.0, 30.0, 20.0, 15.0, cid=2)}
    imgs, tracks = {}, [[] for _ in range(6)]
    for i in range(3):
        n = 4 + i
        ids = rng.integers(1, 7, n).astype(np.int64)
        ids[0] = -1
        imgs[i + 1] = ColmapImage(i + 1, np.array([1.0, 0.0, 0.0, 0.0]), rng.normal(size=3), 1 + i % 2, f"im {i}.png",
                                  xys=rng.uniform(0, 30, (n, 2)), point3D_ids=ids)
        for j, p in enumerate(ids):
            if p > 0:
                tracks[p - 1].append((i + 1, j))
    xyz, rgb = rng.normal(size=(6, 3)), rng.integers(0, 256, (6, 3), dtype=np.uint8)
    return cams, imgs, xyz, rgb, rng.uniform(0, 2, 6), [np.array(t, np.int32).reshape(-1, 2) for t in tracks], [3, 4, 9, 10, 11, 40]


@pytest.mark.parametrize("binary", [True, False])
def test_observations_and_tracks_round_trip_bit_for_bit(tmp_path, binary):
    cams, imgs, xyz, rgb, err, tracks, ids = model_with_observations()
    a, b, ext = tmp_path / "a", tmp_path / "b", ".bin" if binary else ".txt"
    colmap_io.write_colmap_model(a, cams, imgs, xyz, rgb, binary=binary, errors=err, tracks=tracks, point_ids=ids)
    suffix = "binary" if binary else "text"
    rc = getattr(colmap_io, f"read_cameras_{suffix}")(a / f"cameras{ext}", distorted=True)
    ri = getattr(colmap_io, f"read_images_{suffix}")(a / f"images{ext}", points2D=True)
    x2, c2, e2, t2, i2 = getattr(colmap_io, f"read_points3D_{suffix}")(a / f"points3D{ext}", tracks=True)
    for k in imgs:
        assert ri[k].xys.tobytes() == imgs[k].xys.tobytes() and ri[k].point3D_ids.tolist() == imgs[k].point3D_ids.tolist()
    assert i2.tolist() == ids and e2.tobytes() == err.tobytes() and all((p == q).all() for p, q in zip(t2, tracks))
    colmap_io.write_colmap_model(b, rc, ri, x2, c2, binary=binary, errors=e2, tracks=t2, point_ids=i2)
    for name in ("cameras", "images", "points3D"):
        assert (a / f"{name}{ext}").read_bytes() == (b / f"{name}{ext}").read_bytes(), name
    # the old readers skip what they skipped, and refuse what they refused
    plain = getattr(colmap_io, f"read_images_{suffix}")(a / f"images{ext}")
    assert all(im.xys is None and im.point3D_ids is None for im in plain.values()) and sorted(plain) == sorted(imgs)
    assert [im.name for im in plain.values()] == [im.name for im in imgs.values()]
    xyz_only = getattr(colmap_io, f"read_points3D_{suffix}")(a / f"points3D{ext}")
    assert len(xyz_only) == 2 and xyz_only[0].tobytes() == xyz.tobytes() and (xyz_only[1] == rgb).all()
    with pytest.raises(UnsupportedCameraModel, match="undistort the images first"):
        getattr(colmap_io, f"read_cameras_{suffix}")(a / f"cameras{ext}")


def old_write(d, cameras, images, xyz, rgb, binary):
    """write_colmap_model as it was before it learnt observations and tracks"""
    ids = {name: mid for mid, (name, _) in colmap_io.CAMERA_MODELS.items()}
    d.mkdir(parents=True)
    if binary:
        b = struct.pack("<Q", len(cameras))
        for c in cameras.values():
            b += struct.pack("<iiQQ", c.id, ids[c.model], c.width, c.height) + struct.pack("<" + "d" * len(c.params), *map(float, c.params))
        (d / "cameras.bin").write_bytes(b)
        b = struct.pack("<Q", len(images))
        for im in images.values():
            b += struct.pack("<idddddddi", im.id, *map(float, im.qvec), *map(float, im.tvec), im.camera_id)
            b += im.name.encode("utf-8") + b"\x00" + struct.pack("<Q", 0)
        (d / "images.bin").write_bytes(b)
        b = struct.pack("<Q", len(xyz))
        for i, (p, c) in enumerate(zip(xyz, rgb)):
            b += struct.pack("<QdddBBBdQ", i + 1, *map(float, p), *map(int, c), 0.0, 0)
        (d / "points3D.bin").write_bytes(b)
    else:
        (d / "cameras.txt").write_text("# Camera list\n" + "".join(
            f"{c.id} {c.model} {c.width} {c.height} {' '.join(repr(float(v)) for v in c.params)}\n" for c in cameras.values()))
        (d / "images.txt").write_text("# Image list\n" + "".join(
            f"{im.id} {' '.join(repr(float(v)) for v in im.qvec)} {' '.join(repr(float(v)) for v in im.tvec)} "
            f"{im.camera_id} {im.name}\n\n" for im in images.values()))
        (d / "points3D.txt").write_text("# 3D point list\n" + "".join(
            f"{i + 1} {' '.join(repr(float(v)) for v in p)} {' '.join(str(int(v)) for v in c)} 0.0\n"
            for i, (p, c) in enumerate(zip(xyz, rgb))))


@pytest.mark.parametrize("binary", [True, False])
def test_without_the_new_arguments_the_writer_writes_the_old_bytes(tmp_path, binary):
    cams, imgs, xyz, rgb, *_ = model_with_observations()
    for im in imgs.values():
        im.xys = im.point3D_ids = None
    colmap_io.write_colmap_model(tmp_path / "new", cams, imgs, xyz, rgb, binary=binary)
    old_write(tmp_path / "old", cams, imgs, xyz, rgb, binary)
    for f in sorted((tmp_path / "old").iterdir()):
        assert f.read_bytes() == (tmp_path / "new" / f.name).read_bytes(), f.name


def test_camera_infos_still_raises_on_a_distorted_model(tmp_path):
    cams, imgs, xyz, rgb, *_ = model_with_observations()
    colmap_io.write_colmap_model(tmp_path / "sparse" / "0", cams, imgs, xyz, rgb)
    with pytest.raises(UnsupportedCameraModel, match="undistort the images first"):
        colmap_io.camera_infos(str(tmp_path))
    cams, _ = colmap_io.read_model(str(tmp_path), distorted=True)
    assert cams[1].distorted_focal == (31.0, 32.0) and cams[2].distorted_focal == (30.0, 30.0)
    assert cams[1].principal_point == (20.5, 14.5) and cams[2].principal_point == (20.0, 15.0)
    with pytest.raises(UnsupportedCameraModel):
        cams[1].focal


# ---- the whole job, with the reference as the device ------------------------------------------------------------------------
def make_project(root, binary=True, masks=False):
    """A 40 x 30 OPENCV project of three PNG images with observations: <root>/input, <root>/distorted/sparse/0"""
    from PIL import Image
    rng = np.random.default_rng(11)
    c = cam("OPENCV", 40, 30, 33.0, 34.0, 20.5, 14.5, [-0.08, 0.0, 0.003, -0.002], cid=1)
    imgs, pixels = {}, {}
    (root / "input").mkdir(parents=True)
    for i in range(3):
        name = f"frame_{i}.png"
        pixels[name] = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
        Image.fromarray(pixels[name]).save(root / "input" / name)
        n = 5 + i
        xys = rng.uniform([0, 0], [40, 30], (n, 2))
        xys[0] = [1e4, 1e4]                                          # beyond the fold of k1 < 0, k2 = 0: no undistorted position
        ids = np.arange(1, n + 1, dtype=np.int64)
        imgs[i + 1] = ColmapImage(i + 1, np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.1 * i, 0.0, 2.0]), 1, name, xys=xys,
                                  point3D_ids=ids)
        if masks:
            (root / "masks_in").mkdir(exist_ok=True)
            Image.fromarray(rng.integers(0, 2, (30, 40), dtype=np.uint8) * 255).save(root / "masks_in" / name)
    xyz, rgb = rng.normal(size=(8, 3)), rng.integers(0, 256, (8, 3), dtype=np.uint8)
    tracks = [np.array([[1, j]], np.int32) for j in range(8)]
    colmap_io.write_colmap_model(root / "distorted" / "sparse" / "0", {1: c}, imgs, xyz, rgb, binary=binary,
                                 errors=rng.uniform(0, 1, 8), tracks=tracks)
    return c, imgs, pixels


def check_project(root, c, imgs, pixels, binary, resize):
    """<root>/images, <root>/sparse/0 and undistort.json against the reference"""
    from PIL import Image
    out_cam = rule(c, multiple_of=8 if resize else 1)
    ext = ".bin" if binary else ".txt"
    infos = colmap_io.camera_infos(str(root))                        # the trainer's reader takes it
    assert [i.image_name for i in infos] == ["frame_0", "frame_1", "frame_2"] and infos[0].width == out_cam.width
    cams, read = colmap_io.read_model(str(root), points2D=True)
    assert cams[1].model == "PINHOLE" and cams[1].params.tolist() == out_cam.params.tolist()
    assert (cams[1].width, cams[1].height) == (out_cam.width, out_cam.height)
    for k, im in imgs.items():
        want = ref.remap(pixels[im.name], c.model, c.params, out_cam.params, out_cam.width, out_cam.height)
        got = np.asarray(Image.open(root / "images" / im.name))
        assert (got == want).all(), im.name
        uv, ok = ref.undistort_points(c.model, c.params, im.xys)
        assert ok[0] == 0 and ok[1:].all()
        xy = np.stack([out_cam.params[0] * uv[:, 0] + out_cam.params[2], out_cam.params[1] * uv[:, 1] + out_cam.params[3]], 1)
        assert np.isnan(read[k].xys[0]).all() and read[k].point3D_ids[0] == -1
        assert read[k].xys[1:].tobytes() == xy[1:].tobytes() and read[k].point3D_ids[1:].tolist() == im.point3D_ids[1:].tolist()
        if resize:
            for f in (2, 4, 8):
                level = np.asarray(Image.open(root / f"images_{f}" / im.name))
                assert level.shape[:2] == (out_cam.height // f, out_cam.width // f) and (level == ref.box_downscale(want, f)).all()
    assert (root / "sparse" / "0" / f"points3D{ext}").read_bytes() == (root / "distorted" / "sparse" / "0" / f"points3D{ext}").read_bytes()
    meta = json.loads((root / "undistort.json").read_text())
    assert meta["cameras"]["1"]["source"]["model"] == "OPENCV" and meta["cameras"]["1"]["undistorted"]["width"] == out_cam.width
    assert meta["options"]["principal_point"] == "center" and meta["options"]["resize"] is resize


@pytest.mark.parametrize("binary", [True, False])
def test_project_with_the_reference_as_the_device(tmp_path, binary):
    c, imgs, pixels = make_project(tmp_path, binary, masks=True)
    res = undistort.undistort_project(tmp_path / "input", tmp_path / "distorted" / "sparse" / "0", tmp_path, resize=True,
                                      masks=tmp_path / "masks_in", backend=BACKEND, batch=2)
    check_project(tmp_path, c, imgs, pixels, binary, resize=True)
    from PIL import Image
    out_cam = res["cameras"][1]
    mask = np.asarray(Image.open(tmp_path / "masks" / "frame_1.png"))
    src = np.asarray(Image.open(tmp_path / "masks_in" / "frame_1.png"))
    assert mask.ndim == 2 and (mask == ref.remap(src, c.model, c.params, out_cam.params, out_cam.width, out_cam.height)).all()
    assert (tmp_path / "masks_8" / "frame_1.png").exists()


def test_entries_validate_before_any_launch():
    """Bad arguments are statuses from host-side checks (fake device pointers are never dereferenced); nothing to do is PGR_OK."""
    from pegasus_amd import _lib
    lib, bad, fake = _lib.lib(), _lib.PGR_ERR_INVALID_ARGUMENT, C.c_void_p(0x1000)
    p = (C.c_double * 12)(30.0, 20.0, 15.0, -0.1)
    assert lib.pgr_undistort_points(2, p, 0, None, None, None, None) == 0
    assert lib.pgr_distort_points(2, p, 0, None, None, None) == 0
    assert lib.pgr_undistort_points(2, p, -1, fake, fake, None, None) == bad
    assert lib.pgr_undistort_points(2, p, 5, None, fake, None, None) == bad
    assert lib.pgr_undistort_points(2, None, 5, fake, fake, None, None) == bad
    for model in (7, 8, 9, 10, 11, -1):
        assert lib.pgr_undistort_points(model, p, 5, fake, fake, None, None) == bad
        assert lib.pgr_distort_points(model, p, 5, fake, fake, None) == bad
    assert lib.pgr_undistort_points(2, (C.c_double * 12)(0.0, 20.0, 15.0, -0.1), 5, fake, fake, None, None) == bad
    assert lib.pgr_undistort_points(2, (C.c_double * 12)(30.0, 20.0, 15.0, float("nan")), 5, fake, fake, None, None) == bad
    assert lib.pgr_undistort_images(None, 0, None) == 0 and lib.pgr_image_box_downscale(None, 0, 2, None) == 0
    assert lib.pgr_undistort_images(None, 1, None) == bad and lib.pgr_undistort_images(None, -1, None) == bad

    def job(**kw):
        j = dict(src=fake, src_width=8, src_height=8, channels=3, model=2, src_stride=24, dst=fake, dst_width=4, dst_height=4,
                 dst_stride=12, params=p, pinhole=(C.c_double * 4)(30.0, 30.0, 2.0, 2.0))
        j.update(kw)
        return (_lib.PgrUndistortJob * 1)(_lib.PgrUndistortJob(**j))
    for kw in (dict(src=None), dict(dst=None), dict(channels=2), dict(channels=0), dict(src_width=0), dict(dst_height=0),
               dict(src_stride=23), dict(dst_stride=11), dict(src_width=32769, src_stride=1 << 20)):
        assert lib.pgr_undistort_images(job(**kw), 1, None) == bad, kw
        assert lib.pgr_image_box_downscale(job(**kw), 1, 2, None) == bad, kw
    for kw in (dict(model=7), dict(pinhole=(C.c_double * 4)(0.0, 30.0, 2.0, 2.0)),
               dict(pinhole=(C.c_double * 4)(30.0, 30.0, float("inf"), 2.0))):
        assert lib.pgr_undistort_images(job(**kw), 1, None) == bad, kw
    for factor in (0, 1, 3, 16):
        assert lib.pgr_image_box_downscale(job(), 1, factor, None) == bad
    assert lib.pgr_image_box_downscale(job(dst_width=5, dst_stride=15), 1, 2, None) == bad       # 5 * 2 > 8
    assert lib.pgr_image_box_downscale(job(), 1, 4, None) == bad                                 # 4 * 4 > 8


# ---- the GPU tests' fixtures ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ref.DISTORTED)
def test_fixtures_hold_few_near_ties(model):
    """The GPU test lets OPENCV_FISHEYE differ by 1 at pixels whose value before rounding lies within 1e-6 of a tie, and caps
    their share at 1e-3: the seeded sources meet the cap by themselves (for every model, though only the fisheye uses it)."""
    marked = total = outside = 0
    for case in ref.remap_cases(model):
        out, ties = ref.remap(case["src"], case["model"], case["params"], case["pinhole"], case["out_w"], case["out_h"], with_ties=True)
        marked += int(ties.sum())
        total += ties.size
        outside += int((out.reshape(ties.shape + (-1,)) == 0).all(axis=2).sum())
    print(f"{model}: {marked} of {total} pixels marked, {outside} blank")
    assert marked < 1e-3 * total
    assert 0 < outside < 0.5 * total                                 # the fixtures meet both sides of the inside rule
