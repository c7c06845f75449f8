"""The block cull (pegasus_amd/csrc/blockcull.hip.h) at the edges of its bound, where it runs: inside a batch call.

Contract, for every fixture of tests/block_cull_cases.py: a CLEAR visibility bit implies radius 0 for all 64 Gaussians of
the block -- against the HIP exact path with the test switched off (the authority), against the C oracle's radii, and
against the float64 restatement of the listing rule wherever that one's margin lets it bind fp32 code -- for both bit
sources: the stand-alone pgr_block_visibility and the words the batch call itself computed and left in its workspace
(rasterizer.last_block_visibility()).  Radii, n_contrib, colour and one view's per-tile lists are bit-identical with the
test on and off.  Every comparison is on integers or bits.

Printed per case (pytest -s): the smallest float64 slack over all culled blocks -- how far outside the image a Gaussian
of a culled block sits, minus its true radius."""
import numpy as np
import pytest

import block_cull_cases as cases
import block_cull_reference as ref
from helpers import fetch_workspace
from test_block_cull import _specs, _with_cull
from test_block_cull_host import smallest_culling_n

pytestmark = pytest.mark.gpu


def _tensors(case, dev):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kw = dict(means3D=t(case.means), opacities=t(case.opacities()), colors_precomp=t(case.colors()),
              scale_modifier=case.scale_modifier)
    if case.cov6 is not None:
        kw["cov3D_precomp"] = t(case.cov6)
    else:
        kw.update(scales=t(case.scales), rotations=t(case.rotations))
    if case.posed_id is not None:
        kw["posed"] = dict(object_id=t(case.posed_id), poses=t(case.poses))
    return kw


def _forward(kw, specs, cull, list_views, n):
    """One batch call with the block test on or off: (results, in-call bits or None, {view: lists})."""
    import torch
    from pegasus_amd import rasterizer as R

    def run():
        res = R.forward_views(kw["means3D"], kw["opacities"], specs, want_radii=True, want_aux=True,
                              **{k: v for k, v in kw.items() if k not in ("means3D", "opacities")})
        torch.cuda.synchronize()
        bits = R.last_block_visibility()
        lists = {v: fetch_workspace(v, n, int(specs[0].image_width), int(specs[0].image_height)) for v in list_views}
        return res, bits, lists
    return _with_cull(cull, run)


def _same_images(on, off, tag):
    import torch
    for v in range(len(on)):
        assert torch.equal(on[v]["radii"], off[v]["radii"]), (tag, v, "radii")
        assert torch.equal(on[v]["n_contrib"], off[v]["n_contrib"]), (tag, v, "n_contrib")
        a, b = on[v]["color"], off[v]["color"]
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), (tag, v)


def _same_lists(a, b, tag):
    for v in a:
        np.testing.assert_array_equal(a[v]["ranges"], b[v]["ranges"], err_msg=f"{tag} view {v} ranges")
        np.testing.assert_array_equal(a[v]["gauss_sorted"], b[v]["gauss_sorted"], err_msg=f"{tag} view {v} lists")


def _see_all_specs(case, dev):
    """Cameras of the case's shape, pulled so far back that every Gaussian is on screen (every crect is then non-empty)."""
    v0 = case.views[0]
    lo, hi = np.nanmin(case.means, 0).astype(np.float64), np.nanmax(case.means, 0).astype(np.float64)
    span = float((hi - lo).max())
    back = 0.5 * span / min(v0.tanfovx, v0.tanfovy) * 1.5 + 1.0
    mid = 0.5 * (lo + hi)
    views = [cases.camera(np.eye(3), [-mid[0] + 0.01 * k, -mid[1], back - lo[2]], v0.width, v0.height, v0.fovx, v0.fovy)
             for k in range(len(case.views))]
    return _specs(views, dev)


@pytest.mark.parametrize("name", cases.NAMES)
def test_a_clear_bit_means_radius_zero_for_the_whole_block(gpu_device, oracle, name):
    import torch
    from pegasus_amd import rasterizer as R
    case = cases.get(name)
    n, nv, groups = case.n, len(case.views), case.groups
    kw = _tensors(case, gpu_device)
    specs = _specs(case.views, gpu_device)
    scene_kw = {k: kw.get(k) for k in ("scales", "rotations", "cov3D_precomp")}
    alone = R.block_visibility(kw["means3D"], specs, scale_modifier=case.scale_modifier, **scene_kw).cpu().numpy()
    assert alone.shape == (groups, nv)
    stale = name == "c1-400x304-iso-x"
    if stale:
        # a culled block's crects are not written: leave non-empty ones from another call of the same shape in the
        # pooled workspace first -- the binning walks must skip those blocks by their bit
        far_specs = _see_all_specs(case, gpu_device)
        res, bits, _ = _forward(kw, far_specs, True, [], n)
        assert all(bool((r["radii"] > 0).all()) for r in res), "the far cameras do not see every Gaussian"
        assert bits is not None and bool(bits.all())
    off, none_bits, lists_off = _forward(kw, specs, False, [case.list_view], n)
    assert none_bits is None, "PGR_BLOCK_CULL=0, yet the call reports visibility words"
    if stale:
        _forward(kw, far_specs, True, [], n)
    on, in_call, lists_on = _forward(kw, specs, True, [case.list_view], n)
    assert in_call is not None, "this call did not run the block test: the comparison below would be vacuous"
    in_call = in_call.cpu().numpy()
    _same_images(on, off, name)
    _same_lists(lists_on, lists_off, name)

    posed_blocks = np.zeros(groups, bool) if case.posed_id is None else cases.blocks_any(case.posed_id > 0, n)
    np.testing.assert_array_equal(in_call, alone | posed_blocks[:, None], err_msg="in-call bits != stand-alone bits")
    assert in_call[posed_blocks].all(), "a posed object's block was culled"
    for blk, v in case.must_see:
        assert in_call[blk, v] and (alone[blk, v] or posed_blocks[blk]), (name, blk, v)
        assert bool((off[v]["radii"][64 * blk:64 * blk + 64] > 0).any()), (name, blk, v, "fixture: meant to be listed")

    # the three radius sources
    hip = [r["radii"].cpu().numpy() for r in off]
    orc = cases.oracle_radii(case, oracle)
    f64 = cases.reference_listing(case)
    sources = {"in-call": in_call} if case.posed_id is not None else {"stand-alone": alone, "in-call": in_call}
    slack = np.inf
    for v in range(nv):
        seen = {"hip": cases.blocks_any(hip[v] != 0, n), "oracle": cases.blocks_any(orc[v] != 0, n)}
        if f64 is not None:
            seen["float64"] = cases.blocks_any(f64[v]["listed"] & ref.claims(f64[v]), n)
        for src, bits in sources.items():
            for what, s in seen.items():
                wrong = np.flatnonzero(s & ~bits[:, v])
                assert wrong.size == 0, f"{name} view {v}: {src} bit clear, {what} radius non-zero in blocks {wrong[:8]}"
        if f64 is not None:
            with np.errstate(invalid="ignore"):
                need = ref.outside_distance(f64[v], case.views[v]) - f64[v]["radius"]      # NaN: behind the near plane
            per_block = cases.blocks_min(np.where(np.isnan(need), np.inf, need), n)
            culled = ~in_call[:, v]
            if culled.any():
                slack = min(slack, float(per_block[culled].min()))
    print(f"\n[block-cull slack] {name}: smallest float64 slack over culled blocks {slack:.3f} px; "
          f"culled {1.0 - in_call.mean():.3f} of {groups} x {nv}")

    # non-vacuity, on the device
    for src, bits in sources.items():
        assert not bits[case.controls].any(), f"{name}: a control block is not culled ({src})"
        if case.non_vacuous:
            for label, blocks in case.sweeps.items():
                assert bits[blocks].any() and not bits[blocks].all(), f"{name} sweep {label}: {src} bits all alike"


# ------------------------------------------------------------------------------------------ more than 64 views
_BIG = {}


def _clumps(dev):
    """The smallest scene at which a 70-view call culls, rounded up to a partial last block: Morton-ordered clumps of 64 on a
    wide plane, so that most blocks are culled in most of the 48x32 views."""
    import torch
    if "scene" in _BIG:
        return _BIG["scene"]
    n = smallest_culling_n(70)
    if n % 64 == 0:
        n += 1
    groups = (n + 63) // 64
    rng = np.random.default_rng(70)
    side = int(np.ceil(np.sqrt(groups)))
    gy, gx = np.divmod(np.arange(side * side), side)

    def spread(v):                    # Morton order of the grid cells
        v = v.astype(np.uint64)
        out = np.zeros_like(v)
        for b in range(16):
            out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(2 * b)
        return out
    order = np.argsort(spread(gx) | (spread(gy) << np.uint64(1)), kind="stable")[:groups]
    centres = np.stack([gx[order] - 0.5 * side, gy[order] - 0.5 * side, np.zeros(groups)], 1) * 0.5
    means = (np.repeat(centres, 64, 0)[:n] + rng.uniform(-0.1, 0.1, size=(n, 3))).astype(np.float32)
    scales = np.exp(rng.normal(np.log(0.03), 0.5, size=(n, 3))).astype(np.float32)
    q = rng.normal(size=(n, 4))
    rots = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kw = dict(means3D=t(means), opacities=t(np.full(n, 0.8, np.float32)),
              colors_precomp=t(rng.uniform(0.1, 1.0, size=(n, 3)).astype(np.float32)), scales=t(scales), rotations=t(rots),
              scale_modifier=1.0)
    views, far = [], []
    from pegasus_amd import graphics as G, scenes
    half = 0.25 * side
    for k in range(70):
        a = 2.0 * np.pi * k / 70.0 + 0.03 * (k % 7)
        eye = np.array([0.8 * half * np.cos(a), 0.8 * half * np.sin(a), 1.5 + 0.1 * (k % 5)])
        at = np.array([0.3 * half * np.cos(2.3 * a + 1.0), 0.3 * half * np.sin(1.7 * a), 0.0])
        Rm, tt = G.look_at_opencv(tuple(eye), tuple(at), up=(0.0, 0.0, 1.0))
        views.append(scenes.make_view(Rm, tt, 48, 32, fovx=np.radians(50.0), fovy=np.radians(35.0)))
        Rf, tf = G.look_at_opencv((0.1 * k, 0.0, 4.0 * half), (0.1 * k, 0.0, 0.0), up=(0.0, 1.0, 0.0))
        far.append(scenes.make_view(Rf, tf, 48, 32, fovx=np.radians(50.0), fovy=np.radians(35.0)))
    _BIG["scene"] = (n, kw, _specs(views, dev), _specs(far, dev))
    return _BIG["scene"]


@pytest.mark.parametrize("nv", [33, 64, 65, 70])
def test_more_than_64_views_where_the_call_culls(gpu_device, nv):
    """The batch path builds its words 64 views per ballot and stores two words per ballot: 33, 64, 65 and 70 views sit on
    the word and ballot boundaries.  At 70 views the workspace first holds a call that saw everything (stale crects)."""
    import torch
    from pegasus_amd import rasterizer as R
    n, kw, specs, far = _clumps(gpu_device)
    specs, far = specs[70 - nv:], far[70 - nv:]          # (the last views in every count: view 64 + k is never view k's twin)
    groups = (n + 63) // 64
    assert n % 64 != 0
    alone = R.block_visibility(kw["means3D"], specs, scales=kw["scales"], rotations=kw["rotations"])
    pick = sorted({v for v in (0, 31, 32, 63, 64, nv - 1) if v < nv})
    off, none_bits, lists_off = _forward(kw, specs, False, pick, n)
    assert none_bits is None
    if nv == 70:
        res, bits, _ = _forward(kw, far, True, [], n)
        assert bits is not None and bool(bits.all()) and all(bool((r["radii"] > 0).all()) for r in res)
        del res
    on, in_call, lists_on = _forward(kw, specs, True, pick, n)
    assert in_call is not None, ("a %d-view call of %d Gaussians does not run the block test: the threshold moved and "
                                 "smallest_culling_n no longer finds it" % (nv, n))
    assert in_call.shape == (groups, nv)
    assert torch.equal(in_call, alone), "in-call bits != stand-alone bits"
    pad = (-n) % 64
    for v in range(nv):
        seen = torch.nn.functional.pad(off[v]["radii"] != 0, (0, pad)).reshape(-1, 64).any(dim=1)
        assert not bool((seen & ~in_call[:, v]).any()), f"view {v}: a listed Gaussian sits in a culled block"
    _same_images(on, off, f"{nv} views")
    _same_lists(lists_on, lists_off, f"{nv} views")
    culled = 1.0 - float(in_call.float().mean())
    assert culled > 0.5, culled                           # most blocks culled in most views
    assert float(in_call[:, nv - 1].float().mean()) > 0.0
    if nv > 64:
        hi, lo = in_call[:, 64:], in_call[:, :nv - 64]
        assert bool((~hi & lo).any()) and bool((hi & ~lo).any()), "views v and v - 64 never disagree: nothing crosses a word"
