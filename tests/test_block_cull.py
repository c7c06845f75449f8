"""Hierarchical culling (pegasus_amd/csrc/blockcull.hip.h): a 64-Gaussian block is skipped in a view only if every
one of its Gaussians would be culled by the exact per-Gaussian code.  Checked directly (no visible Gaussian ever sits
in a block declared invisible -- on coherent, incoherent and hostile scenes) and end to end (radii, per-tile lists and
images bit-identical with the test switched off).

Every cull-on call asserts that it DID run the block test (rasterizer.last_block_visibility() is not None) and that the
bits it computed inside its preprocess waves equal pgr_block_visibility's; every cull-off call asserts that it did not.
Without that, a call shape that switches the test off by itself would make "on equals off" hold trivially."""
import os

import numpy as np
import pytest

from pegasus_amd import scenes

pytestmark = pytest.mark.gpu


def _specs(views, dev):
    import torch
    from pegasus_amd import rasterizer as R
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return [R.ViewSpec(v.height, v.width, v.tanfovx, v.tanfovy, t(np.zeros(3)), t(v.world_view_transform),
                       t(v.full_proj_transform), t(v.camera_center)) for v in views]


def _render(act_t, specs, **kw):
    import torch
    from pegasus_amd import rasterizer as R
    res = R.forward_views(act_t["means3d"], act_t["opacities"], specs, shs=act_t["shs"], scales=act_t["scales"],
                          rotations=act_t["rotations"], sh_degree=3, want_radii=True, want_aux=True, **kw)
    torch.cuda.synchronize()
    return res


MAX_CULLING_BATCH = 15      # a small scene's call of more views spreads them over the grid and runs no block test


def _render_checked(act_t, specs, cull, vis=None, **kw):
    """_render with the block test on or off, and the proof that the call did what the switch says: off -> no visibility
    words; on -> the call's own bits, equal to ``vis`` (block_visibility of the same scene and views), bit for bit."""
    import torch
    from pegasus_amd import rasterizer as R

    def run():
        res = _render(act_t, specs, **kw)
        return res, R.last_block_visibility()
    res, bits = _with_cull(cull, run)
    if not cull:
        assert bits is None, "PGR_BLOCK_CULL=0, yet the call reports visibility words"
        return res
    assert bits is not None, f"a {len(specs)}-view call of this scene runs no block test: nothing is compared"
    if vis is None:
        vis = R.block_visibility(act_t["means3d"], specs, scales=act_t["scales"], rotations=act_t["rotations"])
    assert torch.equal(bits, vis), "the batch call's in-preprocess bits differ from pgr_block_visibility's"
    return res


def _render_in_batches(act_t, specs, cull, vis):
    """All views, rendered as batches of at most MAX_CULLING_BATCH (each batch checked like _render_checked)."""
    out = []
    for a in range(0, len(specs), MAX_CULLING_BATCH):
        b = min(a + MAX_CULLING_BATCH, len(specs))
        out += _render_checked(act_t, specs[a:b], cull, vis[:, a:b])
    return out


def _with_cull(flag, fn):
    old = os.environ.get("PGR_BLOCK_CULL")
    os.environ["PGR_BLOCK_CULL"] = "1" if flag else "0"
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("PGR_BLOCK_CULL", None)
        else:
            os.environ["PGR_BLOCK_CULL"] = old


@pytest.mark.parametrize("layout", ["morton", "input", "shuffled"])
def test_no_visible_gaussian_in_an_invisible_block(gpu_device, layout):
    """C3 at 5 % scale, 40 cameras: radii from the exact path (test off) against pgr_block_visibility's bits."""
    import torch
    from pegasus_amd import rasterizer as R
    from pegasus_amd.scene_order import spatial_order
    cloud, views = scenes.scene_c3(scale=0.05, n_views=40, width=400, height=304)
    act = cloud.activated()
    n = cloud.n
    if layout == "morton":
        perm = spatial_order(act["means3d"], cloud.object_id)
    elif layout == "shuffled":
        perm = np.random.default_rng(0).permutation(n)
    else:
        perm = np.arange(n)
    act_t = {k: torch.from_numpy(np.ascontiguousarray(a[perm])).to(gpu_device) for k, a in act.items()}
    specs = _specs(views, gpu_device)
    vis = R.block_visibility(act_t["means3d"], specs, scales=act_t["scales"], rotations=act_t["rotations"])
    assert vis.shape == ((n + 63) // 64, len(specs))
    res = _render_in_batches(act_t, specs, False, vis)
    on = _render_in_batches(act_t, specs, True, vis)
    pad = (-n) % 64
    for v, r in enumerate(res):
        seen = torch.nn.functional.pad(r["radii"] > 0, (0, pad)).reshape(-1, 64).any(dim=1)
        assert not bool((seen & ~vis[:, v]).any()), f"view {v}: a listed Gaussian sits in a culled block"
        assert torch.equal(on[v]["radii"], r["radii"]), v
    culled = 1.0 - float(vis.float().mean())
    if layout == "morton":
        assert culled > 0.25, culled          # the point of the exercise: a good share of the plane is off-screen
    if layout == "shuffled":
        assert culled < 0.05, culled          # incoherent order: boxes span the scene, nothing to cull, nothing wrong


@pytest.mark.parametrize("seed", [0, 1])
def test_hostile_blocks_are_never_culled_wrongly(gpu_device, seed):
    """NaN / Inf positions, huge, vanishing and zero scales, unnormalised and zero quaternions, cameras inside the
    cloud and looking away from it."""
    import torch
    from pegasus_amd import graphics as G, rasterizer as R
    rng = np.random.default_rng(50 + seed)
    n = 20000
    cloud, views = scenes.scene_c1(seed=60 + seed, n=n)
    act = cloud.activated()
    act["means3d"] = (act["means3d"] * rng.choice([0.2, 1.0, 30.0], size=(n, 1))).astype(np.float32)
    order = np.argsort(act["means3d"][:, 0] + 10 * np.round(act["means3d"][:, 1]))    # some coherence, some not
    act = {k: a[order] for k, a in act.items()}
    pick = lambda frac: rng.random(n) < frac
    act["means3d"][pick(0.002)] = np.nan
    act["means3d"][pick(0.002), 1] = np.inf
    act["scales"][pick(0.01)] = np.float32(1e3)
    act["scales"][pick(0.01)] = np.float32(1e-8)
    act["scales"][pick(0.01), 2] = 0.0
    act["rotations"][pick(0.01)] = 0.0
    act["rotations"][pick(0.03)] *= np.float32(37.0)
    act_t = {k: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device) for k, a in act.items()}
    cams = []
    for k in range(24):
        eye = rng.normal(0, [3.0, 3.0, 3.0][k % 3], size=3)
        at = rng.normal(0, 2.0, size=3) if k % 4 else eye + rng.normal(0, 1.0, size=3)      # some look away
        Rm, t = G.look_at_opencv(tuple(eye), tuple(at), up=(0, -1, 0))
        cams.append(scenes.make_view(Rm, t, 320, 208, fovx=np.radians(60), fovy=np.radians(41)))
    specs = _specs(cams, gpu_device)
    vis = R.block_visibility(act_t["means3d"], specs, scales=act_t["scales"], rotations=act_t["rotations"])
    off = _render_in_batches(act_t, specs, False, vis)
    on = _render_in_batches(act_t, specs, True, vis)
    pad = (-n) % 64
    for v in range(len(specs)):
        seen = torch.nn.functional.pad(off[v]["radii"] > 0, (0, pad)).reshape(-1, 64).any(dim=1)
        assert not bool((seen & ~vis[:, v]).any()), v
        assert torch.equal(on[v]["radii"], off[v]["radii"])
        assert torch.equal(on[v]["n_contrib"], off[v]["n_contrib"])
        a, b = on[v]["color"], off[v]["color"]
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    assert 0.02 < 1.0 - float(vis.float().mean()) < 0.98


def test_frames_are_bit_identical_with_and_without_block_culling(gpu_device):
    """FrameRenderer (Morton layout, fused semantic image, masks) and the posed path: same bits either way; posed
    objects' blocks are never culled."""
    import torch
    from pegasus_amd import frames as F
    from pegasus_amd.compose import pose_table
    cloud, views = scenes.scene_c3(scale=0.04, n_views=6, width=480, height=352)
    act = cloud.activated()
    fr = F.FrameRenderer(act["means3d"], act["opacities"], act["scales"], act["rotations"], act["shs"], cloud.object_id,
                         sh_degree=3, device=gpu_device)
    specs = [fr.view_spec(v) for v in views]
    keys = ("color", "depth", "seg", "seg_depth", "masks")
    snap = lambda f: {k: f[k].clone() for k in keys}
    from pegasus_amd import rasterizer as R
    vis = R.block_visibility(fr.means3d, specs, scales=fr.scales, rotations=fr.rotations)
    assert 0.02 < 1.0 - float(vis.float().mean())

    def frames(cull, expect, **kw):
        got = _with_cull(cull, lambda: (snap(fr.render_frames(specs, **kw)), R.last_block_visibility()))
        if not cull:
            assert got[1] is None
        else:
            assert got[1] is not None, "the frame call runs no block test"
            assert torch.equal(got[1], expect), "in-call bits differ from pgr_block_visibility's"
        return got[0]
    on = frames(True, vis)
    off = frames(False, vis)
    for k in keys:
        assert torch.equal(on[k], off[k]), k
    assert float(on["masks"].sum()) > 0
    # dynamic: every object flies far out of its rest box (a culled rest box must not hide it)
    Rz = lambda a: np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    poses = np.zeros((len(specs), fr.K, 20), np.float32)
    oid = cloud.object_id
    centers = [act["means3d"][oid == k].mean(0) for k in range(1, fr.K + 1)]
    for s in range(len(specs)):
        pairs = []
        for k in range(fr.K):
            T = Rz(0.4 * s + k)
            T[:3, 3] = [0.6 * np.sin(s + k), 0.6 * np.cos(2 * s + k), 0.05 * s]
            pairs.append((T, centers[k]))
        poses[s] = pose_table(pairs)
    # (a posed object's blocks are visible whatever their rest box says; every other block's bits are the static ones)
    n = int(fr.means3d.shape[0])
    posed_blocks = torch.nn.functional.pad(fr.semantic["object_id"] > 0, (0, (-n) % 64)).reshape(-1, 64).any(dim=1)
    assert bool(posed_blocks.any()) and not bool(posed_blocks.all())
    on = frames(True, vis | posed_blocks[:, None], poses=poses)
    off = frames(False, vis, poses=poses)
    for k in keys:
        assert torch.equal(on[k], off[k]), ("posed", k)


def test_more_than_64_views_per_batch(gpu_device):
    """The visibility words of a batch are built 64 views per ballot: 70 views cross a ballot and a word boundary -- in a
    call that runs the block test: the C3 scene at the smallest size at which a 70-view call does (asked of the library,
    not assumed), cut to a partial last block."""
    import torch
    from pegasus_amd import rasterizer as R
    from pegasus_amd.scene_order import spatial_order
    from test_block_cull_host import smallest_culling_n
    n = smallest_culling_n(70, 160, 112)
    n += n % 64 == 0
    cloud, views = scenes.scene_c3(scale=(n + 2000) / 2.0e6, n_views=70, width=160, height=112)
    assert cloud.n >= n
    act = cloud.activated()
    perm = spatial_order(act["means3d"], cloud.object_id)[:n]
    act_t = {k: torch.from_numpy(np.ascontiguousarray(a[perm])).to(gpu_device) for k, a in act.items()}
    specs = _specs(views, gpu_device)
    vis = R.block_visibility(act_t["means3d"], specs, scales=act_t["scales"], rotations=act_t["rotations"])
    on = _render_checked(act_t, specs, True, vis)
    off = _render_checked(act_t, specs, False)
    assert vis.shape[1] == 70 and 0.05 < 1.0 - float(vis.float().mean()) < 0.95
    for v in range(70):
        assert torch.equal(on[v]["radii"], off[v]["radii"]), v
        assert torch.equal(on[v]["n_contrib"], off[v]["n_contrib"]), v
        assert torch.equal(on[v]["color"], off[v]["color"]), v
