"""Multi-view training, host side: the batch backward's C ABI (declared, exported, prototyped, validated before any
launch), its scratch size, and the trainer's batch_size option (CLI flag, rejection before any GPU work)."""
import ctypes as C
from types import SimpleNamespace

import pytest

FAKE = 0x1000          # a non-NULL device address; the calls below must return before anything could read it


def _load():
    from pegasus_amd import _lib, build
    build.build()
    return _lib, _lib.lib()


def test_batch_backward_symbols_are_declared_exported_and_prototyped():
    from test_abi_symbols import declared_symbols
    _lib, lib = _load()
    for name in ("pgr_backward", "pgr_backward_batch_scratch_bytes"):
        assert name in declared_symbols()
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
    assert [f[0] for f in _lib.PgrBackwardView._fields_] == ["grad_color", "grad_depth", "final_T", "n_contrib", "radii"]


def test_scratch_bytes_grow_with_gaussians_and_views():
    _, lib = _load()
    one = lib.pgr_backward_batch_scratch_bytes(100_000, 1)
    assert one >= 100_000 * 48
    assert lib.pgr_backward_batch_scratch_bytes(200_000, 1) > one
    assert lib.pgr_backward_batch_scratch_bytes(100_000, 4) >= 4 * 100_000 * 48 > one
    assert lib.pgr_backward_batch_scratch_bytes(2_000_000, 8) >= 768_000_000
    assert lib.pgr_backward_batch_scratch_bytes(-1, 2) == 0
    assert lib.pgr_backward_batch_scratch_bytes(10, 0) == 0


def _call(lib, _lib, *, scene=None, n_views=2, cams=True, views=None, grads=True, scratch=FAKE, scratch_bytes=None,
          view_kw=None, sizes=None):
    n = 10
    if scene is None:
        scene = _lib.PgrScene(n=n, means3d=FAKE, opacities=FAKE, scales=FAKE, rotations=FAKE, shs=FAKE, sh_degree=0,
                              sh_stride=1, scale_modifier=1.0)
    sizes = sizes or [(64, 48)] * max(n_views, 1)
    cam_arr = (_lib.PgrCamera * len(sizes))(*[_lib.PgrCamera(image_width=w, image_height=h, tanfovx=0.5, tanfovy=0.5)
                                              for w, h in sizes]) if cams else None
    kw = dict(grad_color=FAKE, final_T=FAKE, n_contrib=FAKE, radii=FAKE)
    kw.update(view_kw or {})
    view_arr = views if views is not None else (_lib.PgrBackwardView * len(sizes))(
        *[_lib.PgrBackwardView(**kw) for _ in sizes])
    g = _lib.PgrGradOutputs(means3d=FAKE) if grads else None
    if scratch_bytes is None:
        scratch_bytes = lib.pgr_backward_batch_scratch_bytes(n, max(n_views, 1))
    call = _lib.PgrBackwardCall(scene=C.pointer(scene), n_views=n_views, cameras=cam_arr, views=view_arr, workspace=FAKE,
                                workspace_bytes=1 << 40, max_instances_per_view=1000,
                                grads=C.pointer(g) if g is not None else None, scratch=scratch, scratch_bytes=scratch_bytes)
    return lib.pgr_backward(call, None)


def test_backward_batch_rejects_bad_arguments_before_any_launch():
    _lib, lib = _load()
    bad = _lib.PGR_ERR_INVALID_ARGUMENT
    split = _lib.PgrScene(n=10, means3d=FAKE, opacities=FAKE, scales=FAKE, rotations=FAKE, shs=FAKE, shs_rest=FAKE,
                          sh_degree=1, sh_stride=4, scale_modifier=1.0)
    assert _call(lib, _lib, scene=split) == bad                                  # the split SH layout
    assert _call(lib, _lib, scene=_lib.PgrScene(n=10)) == bad                    # a scene without arrays
    assert _call(lib, _lib, n_views=0) == bad
    assert _call(lib, _lib, n_views=-3) == bad
    assert _call(lib, _lib, cams=False) == bad                                   # NULL tables
    assert _call(lib, _lib, views=C.POINTER(_lib.PgrBackwardView)()) == bad
    assert _call(lib, _lib, grads=False) == bad
    assert _call(lib, _lib, view_kw=dict(radii=None)) == bad                     # radii are required
    assert _call(lib, _lib, view_kw=dict(grad_color=None)) == bad
    assert _call(lib, _lib, view_kw=dict(final_T=None)) == bad
    assert _call(lib, _lib, view_kw=dict(n_contrib=None)) == bad
    assert _call(lib, _lib, sizes=[(64, 48), (64, 32)]) == bad                   # mixed image sizes
    assert _call(lib, _lib, scratch=None) == bad
    assert _call(lib, _lib, scratch_bytes=lib.pgr_backward_batch_scratch_bytes(10, 2) - 1) == bad    # scratch too small
    # one view is a batch of one: the same rules
    assert _call(lib, _lib, n_views=1, scratch=None) == bad
    assert _call(lib, _lib, n_views=1, scratch_bytes=lib.pgr_backward_batch_scratch_bytes(10, 1) - 1) == bad
    assert _call(lib, _lib, n_views=1, view_kw=dict(radii=None)) == bad
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, n_views=0), "pgr_backward")


def test_cli_accepts_batch_size():
    from pegasus_amd.train import OPTIMIZATION_DEFAULTS, _parser
    args = _parser().parse_args(["-s", "src", "-m", "out", "--batch_size", "4", "--seed", "3"])
    assert args.batch_size == 4 and args.seed == 3
    assert _parser().parse_args([]).batch_size == 1
    assert "batch_size" not in OPTIMIZATION_DEFAULTS


@pytest.mark.parametrize("how", ["keyword", "options"])
def test_training_rejects_batch_size_below_one_before_any_work(tmp_path, how):
    from pegasus_amd.train import training
    out = tmp_path / "model"
    dataset = SimpleNamespace(source_path=str(tmp_path / "missing"), model_path=str(out))
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    opt = SimpleNamespace(iterations=10, batch_size=0 if how == "options" else 2)
    kw = dict(batch_size=0) if how == "keyword" else {}
    with pytest.raises(ValueError, match="batch_size"):
        training(dataset, opt, pipe, [], [], [], None, -1, quiet=True, **kw)
    assert not out.exists()


def test_training_rejects_python_sh_with_a_batch(tmp_path):
    from pegasus_amd.train import training
    out = tmp_path / "model"
    dataset = SimpleNamespace(source_path=str(tmp_path / "missing"), model_path=str(out))
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    with pytest.raises(ValueError, match="convert_SHs_python"):
        training(dataset, SimpleNamespace(), pipe, [], [], [], None, -1, quiet=True, batch_size=4)
    assert not out.exists()


def test_camera_picks_are_distinct_and_refill_a_short_stack():
    import random
    from pegasus_amd.train import _pick_cameras
    random.seed(0)
    cams = [object() for _ in range(5)]
    seen, stack = [], None
    for _ in range(20):
        got, stack = _pick_cameras(stack or [], cams, 4)
        assert len(got) == 4 and len({id(c) for c in got}) == 4
        seen.extend(got)
    assert {id(c) for c in seen} == {id(c) for c in cams}
    with pytest.raises(ValueError, match="larger than"):
        _pick_cameras([], cams, 6)
