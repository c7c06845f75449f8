"""Training from object masks, host side: mask loading (stem matching, resizing, the RGBA alpha source, the error for a
missing mask, no compositing with masks on, unchanged loading with them off), the --masks / --lambda_alpha options and
their compat fields, the new C entries' argument checks before any launch, and the alpha-gradient reference pinned to
finite differences of the dense float64 forward."""
import ctypes as C

import numpy as np
import pytest

FAKE = 0x1000          # a non-NULL device address; the calls below must return before anything could read it


def _info(path, name, w, h):
    from pegasus_amd.colmap_io import CameraInfo
    return CameraInfo(uid=1, R=np.eye(3), T=np.array([0.0, 0.0, 3.0]), FoVx=0.8, FoVy=0.8, image_path=str(path),
                      image_name=name, width=w, height=h)


def _rgba(tmp_path, name="img_007.png", w=40, h=30):
    from PIL import Image
    rng = np.random.default_rng(1)
    arr = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    (tmp_path / "images").mkdir(exist_ok=True)
    p = tmp_path / "images" / name
    Image.fromarray(arr, "RGBA").save(p)
    return p, arr


def test_mask_directory_matches_stem_and_resizes(tmp_path):
    from PIL import Image
    from pegasus_amd.colmap_io import load_camera
    p, arr = _rgba(tmp_path)
    (tmp_path / "masks").mkdir()
    m = np.zeros((60, 80), np.uint8)        # twice the image size: resized (bilinear) to the training size
    m[10:40, 20:60] = 255
    Image.fromarray(m, "L").save(tmp_path / "masks" / "img_007.jpg".replace(".jpg", ".png"))
    Image.fromarray(np.full((5, 5), 255, np.uint8), "L").save(tmp_path / "masks" / "img_008.png")   # another image's
    cam = load_camera(_info(p, "img_007", 40, 30), data_device="cpu", masks=str(tmp_path / "masks"))
    assert tuple(cam.gt_mask.shape) == (1, 30, 40)
    ref = np.asarray(Image.fromarray(m, "L").resize((40, 30), Image.BILINEAR), np.float32) / 255.0
    np.testing.assert_allclose(cam.gt_mask[0].numpy(), ref, atol=1e-6)
    assert float(cam.gt_mask.min()) >= 0.0 and float(cam.gt_mask.max()) <= 1.0
    # the RGB is not composited with masks on
    np.testing.assert_allclose(cam.original_image.numpy(), arr[..., :3].transpose(2, 0, 1) / 255.0, atol=1e-6)
    # resolution 2: the image and its mask both come down to 20 x 15
    cam2 = load_camera(_info(p, "img_007", 40, 30), resolution=2, data_device="cpu", masks=str(tmp_path / "masks"))
    assert tuple(cam2.gt_mask.shape) == (1, 15, 20) and tuple(cam2.original_image.shape) == (3, 15, 20)


def test_alpha_source_and_masks_off(tmp_path):
    from pegasus_amd.colmap_io import load_camera
    p, arr = _rgba(tmp_path)
    cam = load_camera(_info(p, "img_007", 40, 30), data_device="cpu", masks="alpha")
    np.testing.assert_allclose(cam.gt_mask[0].numpy(), arr[..., 3] / 255.0, atol=1e-6)
    np.testing.assert_allclose(cam.original_image.numpy(), arr[..., :3].transpose(2, 0, 1) / 255.0, atol=1e-6)
    off = load_camera(_info(p, "img_007", 40, 30), data_device="cpu")
    a = arr[..., 3:4] / 255.0
    np.testing.assert_allclose(off.original_image.numpy(), (arr[..., :3] / 255.0 * a).transpose(2, 0, 1), atol=1e-6)
    assert off.gt_mask is None
    white = load_camera(_info(p, "img_007", 40, 30), white_background=True, data_device="cpu")
    np.testing.assert_allclose(white.original_image.numpy(), (arr[..., :3] / 255.0 * a + 1 - a).transpose(2, 0, 1),
                               atol=1e-6)


def test_missing_mask_names_the_image(tmp_path):
    from PIL import Image
    from pegasus_amd.colmap_io import load_camera
    p, _ = _rgba(tmp_path)
    (tmp_path / "masks").mkdir()
    with pytest.raises(FileNotFoundError, match="img_007"):
        load_camera(_info(p, "img_007", 40, 30), data_device="cpu", masks=str(tmp_path / "masks"))
    q = tmp_path / "images" / "rgb_only.png"
    Image.fromarray(np.zeros((8, 8, 3), np.uint8), "RGB").save(q)
    with pytest.raises(ValueError, match="rgb_only"):
        load_camera(_info(q, "rgb_only", 8, 8), data_device="cpu", masks="alpha")


def test_cli_and_compat_options():
    from argparse import ArgumentParser
    from pegasus_amd.train import MASK_DEFAULTS, MODEL_DEFAULTS, OPTIMIZATION_DEFAULTS, _parser
    assert MASK_DEFAULTS == dict(masks="", lambda_alpha=0.5)
    assert "masks" not in MODEL_DEFAULTS and "lambda_alpha" not in OPTIMIZATION_DEFAULTS
    a = _parser().parse_args(["-s", "x", "-m", "y"])
    assert a.masks == "" and a.lambda_alpha == 0.5
    a = _parser().parse_args(["-s", "x", "-m", "y", "--masks", "/data/masks", "--lambda_alpha", "0.25"])
    assert a.masks == "/data/masks" and a.lambda_alpha == 0.25
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "compat"))
    try:
        from arguments import ModelParams, OptimizationParams
        p = ArgumentParser()
        mp, op = ModelParams(p), OptimizationParams(p)
        args = p.parse_args(["--masks", "alpha", "--lambda_alpha", "0.1"])
        assert mp.extract(args).masks == "alpha" and op.extract(args).lambda_alpha == 0.1
        d = p.parse_args([])
        assert mp.extract(d).masks == "" and op.extract(d).lambda_alpha == 0.5
    finally:
        sys.path.pop(0)
        for k in [k for k in sys.modules if k == "arguments"]:
            del sys.modules[k]


def _load():
    from pegasus_amd import _lib, build
    build.build()
    return _lib, _lib.lib()


def test_new_entries_are_declared_exported_and_prototyped():
    from test_abi_symbols import declared_symbols
    _lib, lib = _load()
    for name in ("pgr_backward", "pgr_image_loss_masked",
                 "pgr_image_loss_masked_workspace_bytes"):
        assert name in declared_symbols() and name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.pgr_abi_version() == 4
    assert "grad_alpha" in [f[0] for f in _lib.PgrBackwardCall._fields_]
    assert lib.pgr_image_loss_masked_workspace_bytes(37, 53) > lib.pgr_image_loss_workspace_bytes(37, 53) > 0
    assert lib.pgr_image_loss_masked_workspace_bytes(0, 5) == 0


def test_masked_loss_rejects_bad_arguments_before_any_launch():
    _, lib = _load()
    L = _lib_mod()
    ws = lib.pgr_image_loss_masked_workspace_bytes(16, 16)

    def call(mask=FAKE, bg=FAKE, alpha=FAKE, lam=0.2, lam_a=0.5, grad_alpha=FAKE, wsb=ws, x=FAKE):
        v = lambda a: None if a is None else C.c_void_p(a)
        return lib.pgr_image_loss_masked(v(x), v(FAKE), v(mask), v(bg), v(alpha), 16, 16, lam, lam_a, v(FAKE), v(FAKE),
                                         v(grad_alpha), v(FAKE), wsb, None)
    bad = L.PGR_ERR_INVALID_ARGUMENT
    assert call(bg=None) == bad                                  # a mask without bg
    assert call(mask=None, bg=None) == bad                       # alpha without a mask
    assert call(alpha=None, grad_alpha=None) == bad              # lambda_alpha > 0 without alpha
    assert call(lam_a=-0.1) == bad                               # negative lambda_alpha
    assert call(alpha=None, lam_a=0.0) == bad                    # grad_alpha without alpha
    assert call(lam=1.5) == bad and call(x=None) == bad
    assert call(wsb=ws - 1) == L.PGR_ERR_WORKSPACE_TOO_SMALL


def _lib_mod():
    from pegasus_amd import _lib
    return _lib


def test_backward_ex_entries_reject_bad_arguments_before_any_launch():
    _lib, lib = _load()
    n = 10
    scene = _lib.PgrScene(n=n, means3d=FAKE, opacities=FAKE, scales=FAKE, rotations=FAKE, shs=FAKE, sh_degree=0,
                          sh_stride=1, scale_modifier=1.0)
    cam = _lib.PgrCamera(image_width=64, image_height=48, tanfovx=0.5, tanfovy=0.5)
    g = _lib.PgrGradOutputs(means3d=FAKE)
    bad = _lib.PGR_ERR_INVALID_ARGUMENT

    def rc(n_views, cams, views, ga, scratch_bytes):
        call = _lib.PgrBackwardCall(scene=C.pointer(scene), n_views=n_views, cameras=cams, views=views, grad_alpha=ga,
                                    workspace=FAKE, workspace_bytes=1 << 40, max_instances_per_view=1000, grads=C.pointer(g),
                                    scratch=FAKE, scratch_bytes=scratch_bytes)
        return lib.pgr_backward(call, None)
    # one view with a grad_alpha
    one = lambda **kw: C.pointer(_lib.PgrBackwardView(**{**dict(grad_color=FAKE, final_T=FAKE, n_contrib=FAKE, radii=FAKE), **kw}))
    ga1, sb1 = (C.c_void_p * 1)(FAKE), lib.pgr_backward_batch_scratch_bytes(n, 1)
    assert rc(1, C.pointer(cam), one(grad_color=None), ga1, sb1) == bad      # no grad_color
    assert rc(1, C.pointer(cam), one(radii=None), ga1, sb1) == bad           # no radii
    assert rc(1, None, one(), ga1, sb1) == bad                               # no camera
    cams = (_lib.PgrCamera * 2)(cam, _lib.PgrCamera(image_width=32, image_height=48))
    views = (_lib.PgrBackwardView * 2)(*[_lib.PgrBackwardView(grad_color=FAKE, final_T=FAKE, n_contrib=FAKE, radii=FAKE)
                                         for _ in range(2)])
    ga = (C.c_void_p * 2)(FAKE, None)
    sb = lib.pgr_backward_batch_scratch_bytes(n, 2)
    assert rc(2, cams, views, ga, sb) == bad                                 # mixed image sizes
    cams[1] = cam
    assert rc(2, cams, views, ga, sb - 1) == bad                             # scratch too small
    assert rc(0, cams, views, None, sb) == bad                               # no views


# ---- the alpha-gradient reference against finite differences --------------------------------------------------------------
@pytest.mark.parametrize("case", ["deg0", "colors", "opaque"])
def test_alpha_gradient_reference_matches_fd(oracle, case):
    """alpha = 1 - (dense(bg=1) - dense(bg=0)) from the unchanged dense forward; the gradient of sum G image + sum g_a alpha
    with g_a = G[red] is the oracle's colour-only backward with background bg - (1, 0, 0)."""
    from oracle.dense_ref import dense_forward, same_decisions
    from test_backward import loss_weights, tiny_scene
    P, v = tiny_scene(2 if case != "opaque" else 21, n=14 if case != "opaque" else 30)
    deg = 0 if case == "deg0" else 3
    if case == "colors":
        rng = np.random.default_rng(3)
        P["colors_precomp"] = rng.uniform(0.05, 1.0, size=(P["means3d"].shape[0], 3))
        del P["shs"]
    if case == "opaque":
        P["opacities"] = np.random.default_rng(21).uniform(0.85, 0.99, size=P["means3d"].shape[0])
        P["scales"] = P["scales"] * 1.6
    P = {k: np.asarray(np.asarray(a, np.float32), np.float64) for k, a in P.items()}
    gC, _ = loss_weights(5, v.width, v.height)
    gA = gC[0].copy()
    bg = np.array([0.2, 0.4, 0.1])

    def run(Pm):
        c, _, dec = dense_forward(sh_degree=deg, **Pm, **v.raster_kwargs(bg), return_decisions=True)
        one, _ = dense_forward(sh_degree=deg, **Pm, **v.raster_kwargs(np.ones(3)))
        zero, _ = dense_forward(sh_degree=deg, **Pm, **v.raster_kwargs(np.zeros(3)))
        alpha = 1.0 - (one[0] - zero[0])
        return float((c * gC).sum() + (alpha * gA).sum()), dec

    P32 = {k: np.asarray(a, np.float32) for k, a in P.items()}
    o = oracle.forward(**P32, sh_degree=deg, **v.raster_kwargs(bg))
    g = oracle.backward(**P32, sh_degree=deg, grad_color=gC.astype(np.float32),
                        grad_depth=np.zeros((v.height, v.width), np.float32), **v.raster_kwargs(bg - [1.0, 0.0, 0.0]))
    live = np.flatnonzero(o["radii"] > 0)
    rng = np.random.default_rng(7)
    key = dict(means3d="means3d", opacities="opacities", scales="scales", rotations="rotations", shs="shs",
               colors_precomp="colors")
    eps, discarded, total = 1e-6, 0, 0
    for name, A in P.items():
        cand = [(i,) + tuple(j) for i in live for j in np.ndindex(A.shape[1:])]
        if name == "shs":
            cand = [c for c in cand if c[1] < (deg + 1) ** 2]
        num, ana = [], []
        for pi in rng.choice(len(cand), size=min(12, len(cand)), replace=False):
            idx = cand[pi]
            Pp = {k: a.copy() for k, a in P.items()}
            Pm = {k: a.copy() for k, a in P.items()}
            Pp[name][idx] += eps
            Pm[name][idx] -= eps
            (lp, dp), (lm, dm) = run(Pp), run(Pm)
            total += 1
            if not same_decisions(dp, dm):
                discarded += 1
                continue
            num.append((lp - lm) / (2 * eps))
            ana.append(float(g[key[name]][idx]))
        num, ana = np.asarray(num), np.asarray(ana)
        assert num.size, name
        ratio = np.abs(ana - num) / np.maximum(1e-3 * np.abs(num) + 1e-5 * np.abs(num).max(), 1e-300)
        assert ratio.max() <= 1.0, (case, name, ratio.max())
    assert discarded <= 0.1 * total
