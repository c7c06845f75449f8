"""Full-size (BASELINE.json configs[2]: 2 M Gaussians, 800x800) checks through size-independent properties -- the CPU
oracle needs seconds per view at this size, so it checks ONE view; everything else is a property that must hold for
any correct rasterizer: depth-sorted complete lists, run-to-run determinism, colour linearity of compositing, layout
invariance, and the fused semantic image against a separate objects-only pass."""
import numpy as np
import pytest

from pegasus_amd import scenes

pytestmark = pytest.mark.gpu

SPREAD_VIEWS = (128, 300, 60, 500)      # elevations 14.5, 35.9, 6.7 and 77.5 degrees
GRAZING_VIEWS = (0, 1, 2, 3)            # elevations 0, 0.11, 0.22, 0.33 degrees (below the ~8.6 degrees rounds 1-4 started at)


@pytest.fixture(scope="module")
def c3_full(gpu_device):
    import torch
    from pegasus_amd.frames import FrameRenderer
    # configs[2]'s own camera set (the 512 Fibonacci views, elevation ascending): four spread over the hemisphere for the
    # property tests, and the four lowest (0 .. 0.34 degrees: the camera 5 cm above the ground plane, the longest
    # ground-plane lists) for the grazing-view tests
    cloud, all_views = scenes.scene_c3(n_views=512)
    views = [all_views[i] for i in SPREAD_VIEWS]
    act = cloud.activated()
    fr = FrameRenderer(act["means3d"], act["opacities"], act["scales"], act["rotations"], act["shs"], cloud.object_id,
                       device=gpu_device)
    fr.grazing_views = [all_views[i] for i in GRAZING_VIEWS]
    return cloud, views, act, fr


def test_lists_are_complete_and_depth_sorted(c3_full, gpu_device):
    """Every tile list of a full-size view is ascending in (depth bits, index) and the lists hold exactly the
    instances the binning counted; checked on the device (3.4 M entries)."""
    import torch
    from helpers import fetch_workspace
    from pegasus_amd import rasterizer as R
    cloud, views, act, fr = c3_full
    v = views[0]
    res = R.forward_views(fr.means3d, fr.opacities, [fr.view_spec(v)], shs=fr.shs, scales=fr.scales,
                          rotations=fr.rotations, sh_degree=3, want_radii=True, want_aux=True)
    torch.cuda.synchronize()
    w = fetch_workspace(0, cloud.n, v.width, v.height)
    I = R.last_forward_info()["num_instances"][0]
    assert I > 2_000_000 and w["gauss_sorted"].shape[0] == I
    ranges = w["ranges"].astype(np.int64)
    lens = ranges[:, 1] - ranges[:, 0]
    assert lens.sum() == I and (ranges[1:, 0] == ranges[:-1, 1]).all()       # contiguous, complete
    depth_bits = w["depth"].view(np.uint32).astype(np.uint64)
    keys = (depth_bits[w["gauss_sorted"]] << np.uint64(32)) | w["gauss_sorted"].astype(np.uint64)
    tile_of = np.repeat(np.arange(lens.size), lens)
    same_tile = tile_of[1:] == tile_of[:-1]
    assert (keys[1:][same_tile] > keys[:-1][same_tile]).all()                 # strictly ascending inside every tile
    assert (res[0]["radii"].cpu().numpy()[w["gauss_sorted"]] > 0).all()       # only visible Gaussians are listed
    # n_contrib never points past its tile's list
    nc = res[0]["n_contrib"].cpu().numpy()
    H, W = nc.shape
    per_tile_max = nc.reshape(H // 16, 16, W // 16, 16).max(axis=(1, 3)).reshape(-1)
    assert (per_tile_max <= lens).all()


def test_full_size_view_matches_oracle(c3_full, oracle, gpu_device):
    """One full-size view against the oracle (lists bit-exact, image within 1e-4)."""
    import torch
    from helpers import assert_images_match, fetch_workspace
    from pegasus_amd import rasterizer as R
    cloud, views, act, fr = c3_full
    v = views[1]
    perm = fr.order
    act_r = {k: np.ascontiguousarray(a[perm]) for k, a in act.items()}        # the resident (Morton) order
    res = R.forward_views(fr.means3d, fr.opacities, [fr.view_spec(v)], shs=fr.shs, scales=fr.scales,
                          rotations=fr.rotations, sh_degree=3, want_radii=True, want_aux=True)
    torch.cuda.synchronize()
    w = fetch_workspace(0, cloud.n, v.width, v.height)
    o = oracle.forward(**act_r, sh_degree=3, **v.raster_kwargs(), num_threads=8, cull_mode=1)
    np.testing.assert_array_equal(res[0]["radii"].cpu().numpy(), o["radii"])
    np.testing.assert_array_equal(w["gauss_sorted"], o["gauss_sorted"])
    g = dict(color=res[0]["color"].cpu().numpy(), out_depth=res[0]["depth"].cpu().numpy(),
             final_T=res[0]["final_T"].cpu().numpy(), n_contrib=res[0]["n_contrib"].cpu().numpy())
    assert_images_match(g, o)


def test_grazing_views_match_oracle(c3_full, oracle, gpu_device):
    """The four lowest cameras of configs[2]'s Fibonacci set (elevation < 0.4 degrees; rounds 1-4 skipped everything below
    ~8.6 degrees) at FULL size, as one batch: radii and per-tile lists bit-exact against the oracle, images within 1e-4,
    n_contrib exact -- and, for the lowest one, the same against the oracle's REFERENCE-STYLE lists."""
    import math
    import torch
    from helpers import assert_images_match, fetch_workspace
    from test_gpu_parity import _assert_same_ranges, _last_blended
    from pegasus_amd import rasterizer as R
    cloud, _, act, fr = c3_full
    views = fr.grazing_views
    for v in views:
        eye = -v.R_c2w @ v.t_w2c
        assert math.degrees(math.asin((eye[2] - 0.05) / np.linalg.norm(eye - np.array([0, 0, 0.05])))) < 0.4
    act_r = {k: np.ascontiguousarray(a[fr.order]) for k, a in act.items()}
    res = R.forward_views(fr.means3d, fr.opacities, [fr.view_spec(v) for v in views], shs=fr.shs, scales=fr.scales,
                          rotations=fr.rotations, sh_degree=3, want_radii=True, want_aux=True, tie_index=fr.tie_index)
    torch.cuda.synchronize()
    for i, v in enumerate(views):
        w = fetch_workspace(i, cloud.n, v.width, v.height)
        o = oracle.forward(**act_r, sh_degree=3, **v.raster_kwargs(), num_threads=8, cull_mode=1, tie_index=fr.order)
        lens = o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0]
        assert lens.max() > 16384 and o["num_instances"] > 3_000_000          # the ground plane seen edge-on
        np.testing.assert_array_equal(res[i]["radii"].cpu().numpy(), o["radii"])
        np.testing.assert_array_equal(w["gauss_sorted"], o["gauss_sorted"])
        _assert_same_ranges(w["ranges"], o["ranges"])
        g = dict(color=res[i]["color"].cpu().numpy(), out_depth=res[i]["depth"].cpu().numpy(),
                 final_T=res[i]["final_T"].cpu().numpy(), n_contrib=res[i]["n_contrib"].cpu().numpy())
        assert_images_match(g, o)
        if i == 0:
            o0 = oracle.forward(**act_r, sh_degree=3, **v.raster_kwargs(), num_threads=8, cull_mode=0, tie_index=fr.order)
            assert o0["num_instances"] > 1.3 * o["num_instances"]
            np.testing.assert_array_equal(res[i]["radii"].cpu().numpy(), o0["radii"])
            amb = o0["ambig"].astype(bool)
            assert amb.mean() <= 5e-4
            assert np.abs(g["color"] - o0["color"])[:, ~amb].max() <= 1e-4
            assert np.abs(g["out_depth"] - o0["out_depth"])[:, ~amb].max() <= 1e-4
            lg = _last_blended(w["gauss_sorted"], w["ranges"], g["n_contrib"], v.width, v.height)
            lo = _last_blended(o0["gauss_sorted"], o0["ranges"], o0["n_contrib"], v.width, v.height)
            np.testing.assert_array_equal(lg[~amb], lo[~amb])


def test_grazing_views_fused_frames_equal_separate_passes(c3_full, gpu_device):
    """The frames path (fused semantic image + masks + records) on the grazing cameras == the separate passes, bit for bit,
    and the masks see the objects standing on the plane."""
    import torch
    from pegasus_amd import masks as M
    cloud, _, act, fr = c3_full
    specs = [fr.view_spec(v) for v in fr.grazing_views]
    H, W = fr.grazing_views[0].height, fr.grazing_views[0].width
    fa = fr.alloc_frames(len(specs), H, W, records=True)
    fr.render_frames_async(specs, fa, slot=0).wait()
    sep = fr.render_batch(specs)
    for k in ("color", "depth", "seg", "masks"):
        assert torch.equal(fa[k], sep[k]), k
    assert fa["masks"].sum().item() > 10_000
    ref = M.pack_records(fa["color"], fa["depth"], fa["masks"])
    got, want = M.record_views(fa["records"], H, W, fr.K), M.record_views(ref, H, W, fr.K)
    for k in ("rgb", "depth_mm", "mask_bits"):
        assert torch.equal(got[k], want[k]), k


def test_full_size_view_against_reference_style_lists(c3_full, oracle, gpu_device):
    """The same full-size view against the oracle WITHOUT the tight-list predicate (cull_mode=0, the lists the
    reference's rasterizer emits: 5.8 M instances instead of 3.4 M): radii equal, images within 1e-4, and the last blended
    Gaussian of every pixel identical -- the HIP path checked against reference-style lists directly, not through the
    oracle's own tight mode."""
    import torch
    from helpers import fetch_workspace
    from test_gpu_parity import _last_blended
    from pegasus_amd import rasterizer as R
    cloud, views, act, fr = c3_full
    v = views[1]
    act_r = {k: np.ascontiguousarray(a[fr.order]) for k, a in act.items()}
    res = R.forward_views(fr.means3d, fr.opacities, [fr.view_spec(v)], shs=fr.shs, scales=fr.scales,
                          rotations=fr.rotations, sh_degree=3, want_radii=True, want_aux=True)
    torch.cuda.synchronize()
    w = fetch_workspace(0, cloud.n, v.width, v.height)
    o0 = oracle.forward(**act_r, sh_degree=3, **v.raster_kwargs(), num_threads=8, cull_mode=0)
    assert o0["num_instances"] > 1.3 * R.last_forward_info()["num_instances"][0]
    np.testing.assert_array_equal(res[0]["radii"].cpu().numpy(), o0["radii"])
    amb = o0["ambig"].astype(bool)
    assert amb.mean() <= 5e-4
    assert np.abs(res[0]["color"].cpu().numpy() - o0["color"])[:, ~amb].max() <= 1e-4
    assert np.abs(res[0]["depth"].cpu().numpy() - o0["out_depth"])[:, ~amb].max() <= 1e-4
    nc = res[0]["n_contrib"].cpu().numpy()
    lg = _last_blended(w["gauss_sorted"], w["ranges"], nc, v.width, v.height)
    lo = _last_blended(o0["gauss_sorted"], o0["ranges"], o0["n_contrib"], v.width, v.height)
    np.testing.assert_array_equal(lg[~amb], lo[~amb])


def test_frames_are_deterministic_and_layout_invariant(c3_full, gpu_device):
    """Two runs are bit-identical (the binning uses atomics; the sorted lists do not depend on their order), the
    pipelined path equals the blocking one, and the input-order scene gives the same frames as the Morton copy."""
    import torch
    from pegasus_amd.frames import FrameRenderer
    cloud, views, act, fr = c3_full
    specs = [fr.view_spec(v) for v in views]
    a = {k: t.clone() for k, t in fr.render_frames(specs).items()}
    b = fr.render_frames(specs)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    fa = fr.alloc_frames(len(specs), views[0].height, views[0].width)
    fr.render_frames_async(specs, fa, slot=1).wait()
    for k in a:
        assert torch.equal(a[k], fa[k]), k
    fr_in = FrameRenderer(act["means3d"], act["opacities"], act["scales"], act["rotations"], act["shs"],
                          cloud.object_id, device=gpu_device, spatial_order=False)
    c = fr_in.render_frames([fr_in.view_spec(v) for v in views])
    for k in ("color", "depth", "seg", "masks"):       # exact depth ties keep the caller's order (PgrScene.tie_index)
        assert torch.equal(a[k], c[k]), k
    del fr_in


def test_compositing_is_linear_in_colour(c3_full, gpu_device):
    """With a black background the image is a linear function of the per-Gaussian colours:
    image(c1 + c2) = image(c1) + image(c2) (up to fp32 accumulation), depth is colour-independent."""
    import torch
    from pegasus_amd import rasterizer as R
    cloud, views, act, fr = c3_full
    g = torch.Generator(device="cpu").manual_seed(1)
    c1 = torch.rand((cloud.n, 3), generator=g).to(gpu_device)
    c2 = torch.rand((cloud.n, 3), generator=g).to(gpu_device)
    spec = [fr.view_spec(views[2])]
    kw = dict(scales=fr.scales, rotations=fr.rotations, want_radii=False)
    r1 = R.forward_views(fr.means3d, fr.opacities, spec, colors_precomp=c1, **kw)[0]
    r2 = R.forward_views(fr.means3d, fr.opacities, spec, colors_precomp=c2, **kw)[0]
    r12 = R.forward_views(fr.means3d, fr.opacities, spec, colors_precomp=c1 + c2, **kw)[0]
    torch.cuda.synchronize()
    assert torch.equal(r1["depth"], r2["depth"]) and torch.equal(r1["depth"], r12["depth"])
    err = (r12["color"] - (r1["color"] + r2["color"])).abs().max().item()
    assert err < 2e-5 * max(1.0, r12["color"].abs().max().item()), err


def test_fused_semantic_equals_separate_pass_full_size(c3_full, gpu_device):
    """The semantic image accumulated in the scene's compositing walk == an objects-only pass, bit for bit."""
    import torch
    cloud, views, act, fr = c3_full
    specs = [fr.view_spec(v) for v in views[:2]]
    fused = {k: t.clone() for k, t in fr.render_frames(specs).items()}
    sep = fr.render_batch(specs)
    for k in ("color", "depth", "seg", "masks"):
        assert torch.equal(fused[k], sep[k]), k
    assert fused["masks"].sum().item() > 10_000


def test_c5_view_matches_oracle(oracle, gpu_device):
    """BASELINE.json configs[4] scene (5 M Gaussians): one view against the oracle -- lists bit-exact (this scene has
    tile lists of 16-30 k entries: the depth-partitioned sort path on real data, with the Morton copy's tie order),
    image within 1e-4."""
    import torch
    from helpers import assert_images_match, fetch_workspace
    from pegasus_amd import rasterizer as R
    from pegasus_amd.frames import FrameRenderer
    cloud, views = scenes.scene_c5(n_views=4)
    act = cloud.activated()
    fr = FrameRenderer(act["means3d"], act["opacities"], act["scales"], act["rotations"], act["shs"], cloud.object_id,
                       device=gpu_device)
    v = views[0]
    res = R.forward_views(fr.means3d, fr.opacities, [fr.view_spec(v)], shs=fr.shs, scales=fr.scales,
                          rotations=fr.rotations, sh_degree=3, want_radii=True, want_aux=True, tie_index=fr.tie_index)
    torch.cuda.synchronize()
    w = fetch_workspace(0, cloud.n, v.width, v.height)
    act_r = {k: np.ascontiguousarray(a[fr.order]) for k, a in act.items()}
    o = oracle.forward(**act_r, sh_degree=3, **v.raster_kwargs(), num_threads=8, cull_mode=1, tie_index=fr.order)
    lens = o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0]
    assert lens.max() > 16384
    np.testing.assert_array_equal(res[0]["radii"].cpu().numpy(), o["radii"])
    np.testing.assert_array_equal(w["gauss_sorted"], o["gauss_sorted"])
    g = dict(color=res[0]["color"].cpu().numpy(), out_depth=res[0]["depth"].cpu().numpy(),
             final_T=res[0]["final_T"].cpu().numpy(), n_contrib=res[0]["n_contrib"].cpu().numpy())
    assert_images_match(g, o)
    # ... and against the oracle's REFERENCE-STYLE lists (every tile of the 3-sigma rectangle, what the reference's rasterizer
    # emits): radii, images and every pixel's last blended Gaussian
    from test_gpu_parity import _last_blended
    o0 = oracle.forward(**act_r, sh_degree=3, **v.raster_kwargs(), num_threads=8, cull_mode=0, tie_index=fr.order)
    assert o0["num_instances"] > 1.3 * o["num_instances"]
    np.testing.assert_array_equal(res[0]["radii"].cpu().numpy(), o0["radii"])
    amb = o0["ambig"].astype(bool)
    assert amb.mean() <= 5e-4
    assert np.abs(g["color"] - o0["color"])[:, ~amb].max() <= 1e-4
    assert np.abs(g["out_depth"] - o0["out_depth"])[:, ~amb].max() <= 1e-4
    lg = _last_blended(w["gauss_sorted"], w["ranges"], g["n_contrib"], v.width, v.height)
    lo = _last_blended(o0["gauss_sorted"], o0["ranges"], o0["n_contrib"], v.width, v.height)
    np.testing.assert_array_equal(lg[~amb], lo[~amb])
    del fr
    torch.cuda.empty_cache()


def test_c5_posed_sequence_step_matches_oracle(oracle, gpu_device):
    """BASELINE.json configs[4] as SURVEY.md section 8d writes it: the 5 M-Gaussian scene, poses per time step from the
    reference's recorded trajectory (simulation_steps.json body 1, the committed fixture) with per-object phase offsets,
    posed inside the preprocess.  A batch of four time steps at FULL size; one mid-fall step against the oracle's posed
    preprocess: radii, per-tile lists and n_contrib bit-exact, images within 1e-4 -- and the step's BOP pose records
    against a numpy restatement of /root/reference/src/tools/pegasus_working.py:457-576."""
    import torch
    from helpers import assert_images_match, fetch_workspace
    from pegasus_amd import bop_pose, rasterizer as R, trajectory as TJ
    from pegasus_amd.frames import FrameRenderer
    cloud, views, rest = scenes.merged_scene(5, 3_400_000, 20, 80_000, 4)
    act = cloud.activated()
    oid = cloud.object_id
    fr = FrameRenderer(act["means3d"], act["opacities"], act["scales"], act["rotations"], act["shs"], oid, device=gpu_device)
    centers = [act["means3d"][oid == k].astype(np.float64).mean(0) for k in range(1, fr.K + 1)]
    tables, motions = TJ.sequence_poses(TJ.load_fixture(), centers, 200)
    steps = [0, 24, 60, 199]
    check = 1                                                        # step 24: objects 0.2-0.45 m above their resting places
    specs = [fr.view_spec(views[i]) for i in range(4)]
    posed = fr._posed(tables[steps], 4)
    res = R.forward_views(fr.means3d, fr.opacities, specs, shs=fr.shs, scales=fr.scales, rotations=fr.rotations, sh_degree=3,
                          want_radii=True, want_aux=True, tie_index=fr.tie_index, posed=posed)
    torch.cuda.synchronize()
    v = views[check]
    w = fetch_workspace(check, cloud.n, v.width, v.height)
    act_r = {k: np.ascontiguousarray(a[fr.order]) for k, a in act.items()}
    o = oracle.forward(**act_r, sh_degree=3, **v.raster_kwargs(), num_threads=8, cull_mode=1, tie_index=fr.order,
                       object_id=np.ascontiguousarray(oid[fr.order]), poses=tables[steps[check]])
    np.testing.assert_array_equal(res[check]["radii"].cpu().numpy(), o["radii"])
    np.testing.assert_array_equal(w["gauss_sorted"], o["gauss_sorted"])
    g = dict(color=res[check]["color"].cpu().numpy(), out_depth=res[check]["depth"].cpu().numpy(),
             final_T=res[check]["final_T"].cpu().numpy(), n_contrib=res[check]["n_contrib"].cpu().numpy())
    assert_images_match(g, o)
    # the poses do move the picture: the resting step (199 = identity poses) differs from the static render of the same camera
    static = R.forward_views(fr.means3d, fr.opacities, [specs[check]], shs=fr.shs, scales=fr.scales, rotations=fr.rotations,
                             sh_degree=3, want_radii=False, tie_index=fr.tie_index)
    assert (static[0]["color"] - res[check]["color"]).abs().max().item() > 0.05
    rest_static = R.forward_views(fr.means3d, fr.opacities, [specs[3]], shs=fr.shs, scales=fr.scales, rotations=fr.rotations,
                                  sh_degree=3, want_radii=False, tie_index=fr.tie_index)
    # step 199 IS the resting scene (identity poses; x - c + c rounds in fp32, so equal to a few 1e-4, not bit for bit)
    d_rest = (rest_static[0]["color"] - res[3]["color"]).abs()
    assert d_rest.max().item() < 5e-3 and d_rest.mean().item() < 1e-5
    # BOP records of the checked step
    m2w = {}
    for k in range(1, fr.K + 1):
        M = np.eye(4); M[:3, :3], M[:3, 3] = rest[k - 1]
        m2w[k] = motions[steps[check]][k] @ M
    gt, cam = bop_pose.batch_pose_records([v], [m2w])
    T_w2c = np.eye(4); T_w2c[:3, :3] = v.R_c2w.T; T_w2c[:3, 3] = v.t_w2c
    for e in gt["0"]:
        T = T_w2c @ m2w[e["obj_id"]]
        np.testing.assert_allclose(np.asarray(e["cam_R_m2c"]).reshape(3, 3), T[:3, :3], atol=1e-12)
        np.testing.assert_allclose(e["cam_t_m2c"], T[:3, 3], atol=1e-12)
        # the record places the model origin where the posed Gaussians of that object are: their mean in camera space
        sel = oid == e["obj_id"]
        Tk = tables[steps[check], e["obj_id"] - 1].astype(np.float64)
        Rk, tk, ck = Tk[0:9].reshape(3, 3), Tk[9:12], Tk[12:15]
        world = (Rk @ (act["means3d"][sel].astype(np.float64) - ck).T).T + ck + tk
        cam_mean = (T_w2c[:3, :3] @ world.mean(0)) + T_w2c[:3, 3]
        assert np.linalg.norm(cam_mean - T[:3, 3]) < 0.01            # 80 k box-surface samples: their mean is the box centre
    fx = v.width / (2 * v.tanfovx)
    np.testing.assert_allclose(cam["0"]["cam_K"][0], fx, rtol=1e-12)
    del fr
    torch.cuda.empty_cache()


def test_full_size_backward_matches_oracle_per_element(c3_full, oracle, gpu_device):
    """The backward at full size (2 M Gaussians, 800x800, SH degree 3: long lists from every sort tier, the forward's
    48-byte records and tie order re-read) on one spread and one grazing view: pgr_backward per view, and a batch pgr_backward
    on the two views together, against the oracle per element (tests/test_backward_parity_gpu.py's rules)."""
    import torch
    from helpers import assert_grads_match
    from test_backward_parity_gpu import BG, _settings, _weights, hip_backward
    from pegasus_amd import diff_gaussian_rasterization as dgr
    # Rounding bound for scales and rotations at this size (every other group keeps the bound 1): the worst elements
    # belong to flat Gaussians (axis ratios ~40-110, e.g. scales 0.00019 / 0.0016 / 0.008), whose smallest-axis scale and
    # quaternion gradients are small differences of large cov3D-gradient terms, summed from fp32 atomics over up to
    # thousands of 4x4 blocks in no fixed order -- the worst ratio moves between runs.  Measured on MI355X in two runs:
    # scales 5.25 and 1.30, rotations 2.87 (one element above 1 in 6 M; ~100 above 0.1); all other groups <= 0.11.
    bounds = dict(scales=15.0, rotations=15.0)
    cloud, views, act, fr = c3_full
    X = {k: np.ascontiguousarray(act[k], np.float32) for k in ("means3d", "opacities", "scales", "rotations", "shs")}
    pair = [views[1], fr.grazing_views[0]]
    wts, refs = [], []
    for k, v in enumerate(pair):
        gC, gD, o = _weights(oracle, X, v, 3, 1.0, 400 + k)
        assert o["ambig"].mean() <= 5e-4
        got, radii = hip_backward(X, v, 3, 1.0, gC, gD, gpu_device)
        np.testing.assert_array_equal(radii, o["radii"])
        ref = oracle.backward(**X, sh_degree=3, grad_color=gC, grad_depth=gD, **v.raster_kwargs(BG), num_threads=16)
        ref = {g: ref[g] for g in got}
        for g in got:
            assert not got[g][radii == 0].any(), g
        worst = assert_grads_match(got, ref, f"full size view {k}", bounds=bounds)
        print(f"\nBWD-RATIO full size view {k}: " + " ".join(f"{g} {r:.3g}" for g, r in worst.items()))
        wts.append((gC, gD))
        refs.append(ref)
    dev = gpu_device
    leaf = {k: torch.from_numpy(a.reshape(-1, 1) if k == "opacities" else a).to(dev).requires_grad_(True)
            for k, a in X.items()}
    m2d = torch.zeros((2,) + tuple(leaf["means3d"].shape), device=dev, requires_grad=True)
    color, radii, depth = dgr.rasterize_gaussians_batch(leaf["means3d"], m2d, leaf["opacities"],
                                                        [_settings(v, dev, 3, 1.0) for v in pair], shs=leaf["shs"],
                                                        scales=leaf["scales"], rotations=leaf["rotations"])
    loss = sum((color[k] * torch.from_numpy(gC).to(dev)).sum() + (depth[k, 0] * torch.from_numpy(gD).to(dev)).sum()
               for k, (gC, gD) in enumerate(wts))
    loss.backward()
    torch.cuda.synchronize()
    key = dict(means3d="means3d", opacities="opacities", scales="scales", rotations="rotations", shs="shs")
    got = {key[k]: t.grad.detach().cpu().numpy().reshape(X[k].shape) for k, t in leaf.items()}
    worst = assert_grads_match(got, {g: refs[0][g].astype(np.float64) + refs[1][g] for g in got}, "full size batch",
                               bounds=bounds)
    m2 = m2d.grad.detach().cpu().numpy()
    for k in range(2):
        worst[f"means2d[{k}]"] = assert_grads_match({"means2d": m2[k]}, {"means2d": refs[k]["means2d"]},
                                                    f"full size batch view {k}")["means2d"]
    print("\nBWD-RATIO full size batch: " + " ".join(f"{g} {r:.3g}" for g, r in worst.items()))
