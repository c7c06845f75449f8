"""The undistortion kernels (pegasus_amd/undistort.py, csrc/undistort.hip.h) where they run, against the NumPy float64
restatement of tests/undistort_reference.py.

Bounds.  The four polynomial models are +, -, *, / and floor of float64 in one fixed order with contraction off, so the remap must
equal the reference byte for byte.  OPENCV_FISHEYE calls atan, which the device and NumPy need not round alike: a byte may differ
by 1 where the value before rounding lies within 1e-6 of a tie (an atan off by a few ulp moves a value of at most 255 by about
1e-10), and tests/test_undistort_host.py holds the share of such pixels in these fixtures under 1e-3.  The inverse is iterative:
ok points equal the reference to 1e-10 (the issue's bound; Newton's last step is below 1e-10 and both sides stop by the same
test) and meet the rule's own residual bound when distorted again in float64 on the host.

The inside rule is the closed one of DESIGN.md section 26, 0 <= sx <= w - 1 (a second tap at x1 = w only ever meets weight 0):
with x1 >= w counted as outside, the identity test below could not hold in the last row and column."""
import numpy as np
import pytest
import torch

import undistort_reference as ref
from pegasus_amd import colmap_io, undistort
from pegasus_amd.colmap_io import ColmapCamera

pytestmark = pytest.mark.gpu

# coefficients with a fold: the radial term turns back beyond the image (f = 80 puts the 64 x 48 image's corner at r_d = 0.5)
FOLDING = {"SIMPLE_PINHOLE": [], "PINHOLE": [], "SIMPLE_RADIAL": [-0.3], "RADIAL": [-0.3, -0.02],
           "OPENCV": [-0.3, -0.02, 0.002, -0.001], "FULL_OPENCV": [-0.3, -0.02, 0.002, -0.001, 0.0, 0.01, 0.0, 0.0],
           "OPENCV_FISHEYE": [-0.3, -0.02, 0.0, 0.0]}
PW, PH, PF = 64, 48, 80.0


def cam(model, w, h, fx, fy, cx, cy, coeffs=None, cid=1):
    return ColmapCamera(cid, model, w, h, ref.camera_params(model, fx, fy, cx, cy, coeffs))


def point_set(model, n, rng):
    """n image points: most inside the image, for the models with a fold one in four beyond it (r_d 0.75 .. 30: the band
    between the largest distorted radius, about 0.7, and the fold, and far outside), and one NaN when there is room"""
    pts = rng.uniform([0.0, 0.0], [PW, PH], (n, 2))
    outside = np.zeros(n, bool)
    if FOLDING[model]:
        outside = np.arange(n) % 4 == 3
        m = int(outside.sum())
        rd, ang = np.exp(rng.uniform(np.log(0.75), np.log(30.0), m)), rng.uniform(0, 2 * np.pi, m)
        pts[outside] = np.stack([PW / 2 + 0.3 + PF * rd * np.cos(ang), PH / 2 - 0.2 + 1.03 * PF * rd * np.sin(ang)], 1)
    if n >= 63:
        pts[5] = np.nan
        outside[5] = True
    return pts, outside


@pytest.mark.parametrize("model", sorted(ref.SHAPES))
def test_points_against_the_reference(model):
    c = cam(model, PW, PH, PF, 1.03 * PF, PW / 2 + 0.3, PH / 2 - 0.2, FOLDING[model])
    rng = np.random.default_rng(3 + sorted(ref.SHAPES).index(model))
    slack = 1e-15 if model == "OPENCV_FISHEYE" else 0.0            # the device's atan against NumPy's, a few ulp of |x_d| <= 1
    for n in (0, 1, 63, 64, 65, 1000):
        pts, outside = point_set(model, n, rng)
        want, want_ok = ref.undistort_points(c.model, c.params, pts)
        assert not want_ok[outside].any() and want_ok[~outside].all()          # the fixture is what it says
        uv, ok = undistort.undistort_points(c, pts)
        assert uv.shape == (n, 2) and uv.dtype == torch.float64 and ok.shape == (n,) and ok.dtype == torch.uint8
        uv, ok = uv.cpu().numpy(), ok.cpu().numpy()
        assert (ok == want_ok).all()
        assert np.isnan(uv[ok == 0]).all()                                     # never a finite value without the flag
        good = ok == 1
        err = np.abs(uv[good] - want[good])
        res, bound = ref.residual(c.model, c.params, uv[good], pts[good])
        print(f"{model} n={n}: max |uv - ref| {err.max() if good.any() else 0:.3g}, max residual / bound "
              f"{(res / bound).max() if good.any() else 0:.3g}")
        assert (err <= 1e-10).all()
        assert (res <= bound + slack).all()
        if model in ("PINHOLE", "SIMPLE_PINHOLE"):
            fx, fy, cx, cy, _ = ref.split(c.model, c.params)
            assert (uv[good] == np.stack([(pts[good, 0] - cx) / fx, (pts[good, 1] - cy) / fy], 1)).all()     # exactly
        # the forward direction brings the ok points back
        back = undistort.distort(c, uv[good]).cpu().numpy()
        assert back.shape == (int(good.sum()), 2)
        np.testing.assert_allclose(back, pts[good], rtol=0, atol=1e-9)          # 1e-12 max(1, |x_d|) times f = 80
        if model not in ("OPENCV_FISHEYE",) and good.any():
            assert (back == ref.distort(c.model, c.params, uv[good])).all()


# ---- remap ----------------------------------------------------------------------------------------------------------------
def padded(array, pad, fill=0xAB):
    """A device view of ``array`` ([h,w] or [h,w,c]) whose rows lie ``pad`` bytes apart beyond their own, and its buffer"""
    a = np.asarray(array)
    h, w = a.shape[:2]
    c = 1 if a.ndim == 2 else a.shape[2]
    buf = torch.full((h, w * c + pad), fill, dtype=torch.uint8, device="cuda")
    view = buf[:, :w * c] if a.ndim == 2 else buf[:, :w * c].unflatten(1, (w, c))
    view.copy_(torch.from_numpy(a).cuda())
    return view, buf


def run_cases(cases):
    """One pgr_undistort_images call over the cases, sources and destinations padded as the cases say: (outputs, ok) where ok
    says that no padding byte was written"""
    srcs, dsts, cams, ocams = [], [], [], []
    for case in cases:
        src = case["src"]
        h, w = src.shape[:2]
        srcs.append(padded(src, case["pad_src"])[0])
        dsts.append(padded(np.zeros((case["out_h"], case["out_w"]) + src.shape[2:], np.uint8) + 7, case["pad_dst"]))
        cams.append(ColmapCamera(1, case["model"], w, h, case["params"]))
        ocams.append(ColmapCamera(1, "PINHOLE", case["out_w"], case["out_h"], case["pinhole"]))
    got = undistort.undistort_images(srcs, cams, ocams, out=[d[0] for d in dsts])
    torch.cuda.synchronize()
    clean = all(bool((buf[:, buf.shape[1] - case["pad_dst"]:] == 0xAB).all()) for case, (_, buf) in zip(cases, dsts))
    return [g.cpu().numpy() for g in got], clean


def compare(model, got, want, ties):
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16)).reshape(ties.shape + (-1,)).max(axis=2)
    if model == "OPENCV_FISHEYE":
        assert (diff[~ties] == 0).all() and (diff <= 1).all()
    else:
        assert (diff == 0).all()


@pytest.mark.parametrize("model", ref.DISTORTED + ("PINHOLE",))
def test_remap_against_the_reference(model):
    """Every output width 1, 3, 4, 5, 255, 256, 257 x height 1, 7 x 1, 3, 4 channels in ONE call (three launches: the jobs of a
    channel count go together), padded rows on both sides."""
    cases = ref.remap_cases(model)
    assert {(c["out_w"], c["out_h"], 1 if c["src"].ndim == 2 else c["src"].shape[2]) for c in cases} == {
        (W, H, ch) for W in ref.REMAP_WIDTHS for H in ref.REMAP_HEIGHTS for ch in ref.REMAP_CHANNELS}
    got, clean = run_cases(cases)
    assert clean
    marked = total = 0
    for case, g in zip(cases, got):
        want, ties = ref.remap(case["src"], case["model"], case["params"], case["pinhole"], case["out_w"], case["out_h"], with_ties=True)
        assert g.shape == want.shape
        compare(model, g, want, ties)
        marked, total = marked + int(ties.sum()), total + ties.size
    if model == "OPENCV_FISHEYE":                                              # the one model whose comparison uses the marks
        assert marked <= 1e-3 * total


def small_case(model, src, out_w, out_h, pinhole, f=3.0, cx=None, cy=None):
    h, w = src.shape[:2]
    params = ref.camera_params(model, f, f, w / 2.0 if cx is None else cx, h / 2.0 if cy is None else cy)
    return dict(model=model, params=params, src=src, pinhole=np.asarray(pinhole, dtype=np.float64), out_w=out_w, out_h=out_h,
                pad_src=0, pad_dst=0)


def test_remap_batches_and_small_sources():
    rng = np.random.default_rng(8)
    assert undistort.undistort_images([], [], []) == []                        # zero jobs: no launch
    # five jobs of mixed sizes, channel counts and two models in one call; the last lies wholly outside its source
    five = [small_case("OPENCV", rng.integers(1, 256, (9, 13, 3), dtype=np.uint8), 11, 6, [9.0, 9.0, 5.5, 3.0], f=9.0),
            small_case("SIMPLE_RADIAL", rng.integers(1, 256, (2, 2), dtype=np.uint8), 5, 5, [3.0, 3.0, 2.5, 2.5]),
            small_case("OPENCV", rng.integers(1, 256, (300, 7, 4), dtype=np.uint8), 6, 290, [200.0, 200.0, 3.0, 145.0], f=200.0),
            small_case("SIMPLE_RADIAL", rng.integers(1, 256, (2, 2, 3), dtype=np.uint8), 4, 4, [4.0, 4.0, 2.0, 2.0], f=4.0),
            small_case("OPENCV", rng.integers(1, 256, (8, 8, 3), dtype=np.uint8), 9, 5, [8.0, 8.0, 100.0, 2.5], f=8.0)]
    got, _ = run_cases(five)
    for case, g in zip(five, got):
        want = ref.remap(case["src"], case["model"], case["params"], case["pinhole"], case["out_w"], case["out_h"])
        assert (g == want).all()
    assert (got[4] == 0).all()                                                 # outside: 0 in every channel
    assert got[1].any() and got[3].any()                                       # a 2 x 2 source has an interior
    one, _ = run_cases(five[:1])                                               # one job
    assert (one[0] == got[0]).all()
    # a 1 x 1 source has no interior: only a pixel that lands exactly on its centre would find its taps, and the centres of
    # an even output straddle it
    single = small_case("PINHOLE", np.full((1, 1, 3), 255, np.uint8), 4, 4, [3.0, 3.0, 2.0, 2.0])
    got, _ = run_cases([single])
    assert (got[0] == 0).all() and (ref.remap(single["src"], "PINHOLE", single["params"], single["pinhole"], 4, 4) == 0).all()


@pytest.mark.parametrize("model", ["SIMPLE_RADIAL", "OPENCV", "FULL_OPENCV", "PINHOLE"])
def test_zero_distortion_is_the_identity(model):
    """center mode, the principal point at the centre, f = 32: (x + 0.5 - cx) / f f + cx is exact for a power of two, so every
    output pixel lands on its source pixel's centre with weights 1, 0, 0, 0 -- the last row and column included, whose second
    taps lie outside and carry no weight."""
    rng = np.random.default_rng(2)
    c = cam(model, 48, 20, 32.0, 32.0, 24.0, 10.0, [0.0] * ref.SHAPES[model][1])
    out_cam = undistort.undistort_camera(c)                                    # the border scan on the device
    assert (out_cam.width, out_cam.height, out_cam.params.tolist()) == (48, 20, [32.0, 32.0, 24.0, 10.0])
    for shape in ((20, 48), (20, 48, 3), (20, 48, 4)):
        src = rng.integers(0, 256, shape, dtype=np.uint8)
        out = undistort.undistort_images([torch.from_numpy(src).cuda()], c, out_cam)[0]
        assert (out.cpu().numpy() == src).all()


def test_direction_of_the_warp():
    """A barrel camera (k = -0.1 at f = 64 on 65 x 49, the principal point on the centre of pixel (32, 24)), keep mode.
    blank_pixels = 0: the source around the principal point lands on the output's principal point, and no pixel is blank.  (The
    rule promises that every output pixel's CENTRE maps inside the image; its taps also need the outer half pixel, which here
    the floor of the size leaves: 66 x 49 of 66.6 x 49.3.  At k = -0.2 the reference blanks 28 pixels of the first and last
    column.)  blank_pixels = 1: the blank pixels are a frame around the image, and the corners are blank."""
    rng = np.random.default_rng(4)
    c = cam("SIMPLE_RADIAL", 65, 49, 64.0, 64.0, 32.5, 24.5, [-0.1])
    src = rng.integers(1, 100, (49, 65), dtype=np.uint8)
    src[22:27, 30:35] = 200                                                    # 5 x 5 around the principal point's pixel
    tight = undistort.undistort_camera(c, principal_point="keep")
    assert (tight.width, tight.height) == (66, 49)
    out = undistort.undistort_images([torch.from_numpy(src).cuda()], c, tight)[0].cpu().numpy()
    assert (out == ref.remap(src, c.model, c.params, tight.params, 66, 49)).all()
    assert out[int(tight.params[3]), int(tight.params[2])] == 200
    assert (out > 0).all()
    wide = undistort.undistort_camera(c, principal_point="keep", blank_pixels=1.0)
    assert wide.width > tight.width and wide.height > tight.height
    out = undistort.undistort_images([torch.from_numpy(src).cuda()], c, wide)[0].cpu().numpy()
    assert (out == ref.remap(src, c.model, c.params, wide.params, wide.width, wide.height)).all()
    blank = out == 0
    assert blank[0, 0] and blank[0, -1] and blank[-1, 0] and blank[-1, -1]
    # a frame: undistorted, the barrel image is a cushion whose tips reach for the corners, so the blank pixels are crescents
    # along the middle of every side, joined through the corner pixels, and nothing further inside than the size grew
    h, w = blank.shape
    assert blank[0, w // 2] and blank[-1, w // 2] and blank[h // 2, 0] and blank[h // 2, -1]
    m = max(wide.width - tight.width, wide.height - tight.height)
    assert blank.any() and not blank[m:-m, m:-m].any()


# ---- box means ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [2, 4, 8])
def test_box_downscale_is_the_integer_rule(factor):
    rng = np.random.default_rng(factor)
    images = []
    for h, w in ((factor, factor), (8, 8), (24, 40)):
        yy, xx = np.mgrid[0:h, 0:w]
        for c in (1, 3, 4):
            shape = (h, w) if c == 1 else (h, w, c)
            board = (((yy + xx) % 2) * 255).astype(np.uint8)                   # sums of 255 f f / 2: the rounding
            images += [np.full(shape, 255, np.uint8), board if c == 1 else np.repeat(board[:, :, None], c, 2),
                       (((yy * w + xx) % 3 == 0) * 255).astype(np.uint8) if c == 1 else rng.integers(0, 256, shape, dtype=np.uint8),
                       rng.integers(0, 256, shape, dtype=np.uint8)]
    views = [padded(a, (0, 1, 6)[i % 3])[0] for i, a in enumerate(images)]
    got = undistort.box_downscale(views, factor)                               # one call, three launches
    assert undistort.box_downscale([], factor) == []
    for a, g in zip(images, got):
        want = ref.box_downscale(a, factor)
        assert g.shape == want.shape and (g.cpu().numpy() == want).all()
        if (a == 255).all():
            assert (want == 255).all()                                         # no overflow


# ---- the whole job --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("png", ["host", "gpu"])
def test_project_end_to_end(tmp_path, png):
    """A 40 x 30 OPENCV project of three PNG images with observations through undistort_project on the device: what
    tests/test_undistort_host.py checks of the same job run on the reference (the trainer's reader loads it, images,
    observations, points3D, undistort.json, the pyramid)."""
    from PIL import Image

    import test_undistort_host as host
    c, imgs, pixels = host.make_project(tmp_path)
    res = undistort.undistort_project(tmp_path / "input", tmp_path / "distorted" / "sparse" / "0", tmp_path, resize=True, png=png)
    out_cam = res["cameras"][1]
    want_cam = undistort.undistort_camera(c, multiple_of=8, backend=ref.Backend())
    assert (out_cam.width, out_cam.height, out_cam.params.tolist()) == (want_cam.width, want_cam.height, want_cam.params.tolist())
    assert out_cam.width % 8 == 0 and out_cam.height % 8 == 0
    infos = colmap_io.camera_infos(str(tmp_path))
    assert len(infos) == 3 and (infos[0].width, infos[0].height) == (out_cam.width, out_cam.height)
    _, read = colmap_io.read_model(str(tmp_path), points2D=True)
    for k, im in imgs.items():
        want = ref.remap(pixels[im.name], c.model, c.params, out_cam.params, out_cam.width, out_cam.height)
        assert (np.asarray(Image.open(tmp_path / "images" / im.name)) == want).all()
        for f in (2, 4, 8):
            level = np.asarray(Image.open(tmp_path / f"images_{f}" / im.name))
            assert level.shape == (out_cam.height // f, out_cam.width // f, 3) and (level == ref.box_downscale(want, f)).all()
        uv, ok = ref.undistort_points(c.model, c.params, im.xys)
        xy = np.stack([out_cam.params[0] * uv[:, 0] + out_cam.params[2], out_cam.params[1] * uv[:, 1] + out_cam.params[3]], 1)
        assert ok[0] == 0 and np.isnan(read[k].xys[0]).all() and read[k].point3D_ids[0] == -1
        assert read[k].point3D_ids[1:].tolist() == im.point3D_ids[1:].tolist()
        # 1e-10 in normalised units times the focal length of 34
        np.testing.assert_allclose(read[k].xys[1:], xy[1:], rtol=0, atol=34 * 1e-10)
    sparse, src = tmp_path / "sparse" / "0", tmp_path / "distorted" / "sparse" / "0"
    assert (sparse / "points3D.bin").read_bytes() == (src / "points3D.bin").read_bytes()
    assert (tmp_path / "undistort.json").exists()
