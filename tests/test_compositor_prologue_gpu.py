"""The compositor's per-batch prologue (its own skip test quarter_may_contribute, the alive box) through the C ABI, on
small images with partial quarters and tiles on both edges: every kernel form -- plain, AUX, fused with masks (K = 3 and
K = 9: a second mask byte in the record), fused AUX, records only, layered silhouettes, a 3-view batch -- against the
CPU oracle at helpers.py's tolerances (n_contrib exactly), and masks / records against color_masks / pgr_pack_records of the
same frames bit for bit.  The scenes mix ordinary Gaussians with the families of tests/quarter_skip_sweep.cpp: isotropic and
1000:1 splats at 0 / 45 / 135 degrees, opacities at 0, around 1/255, 0.5, 0.99 and 1, centres inside the image, on quarter
edges, 1 and 8 pixels outside it and far away."""
import math

import numpy as np
import pytest

from pegasus_amd import graphics as G, scenes

pytestmark = pytest.mark.gpu

BG = (0.3, 0.05, 0.6)
FOVX = math.radians(50.0)
# seeds at which the oracle flags at most its allowed 5e-4 of the pixels as ambiguous (a 960-pixel image allows none)
SEED = {40: 2, 72: 1}


def _views(W, H):
    fovy = 2.0 * math.atan(math.tan(0.5 * FOVX) * H / W)
    out = []
    for eye in ((0.0, 0.0, -3.0), (0.5, 0.25, -2.8), (-0.4, -0.3, -3.2)):
        R, t = G.look_at_opencv(eye, (0.0, 0.0, 0.0), up=(0.0, -1.0, 0.0))
        out.append(scenes.make_view(R, t, W, H, fovx=FOVX, fovy=fovy))
    return out


def _rot_z(deg):
    h = math.radians(deg) * 0.5
    return np.array([math.cos(h), 0.0, 0.0, math.sin(h)], np.float32)          # (w, x, y, z)


def _scene(W, H, seed, ids=(1, 2, 3), clump_px=6.0, n_clump=300, n_env=1000, stack=False):
    """Activated arrays + object ids: environment first, then three objects (ids non-decreasing).  Lengths are in world
    units; u = world units per pixel at the environment's depth (camera 0)."""
    rng = np.random.default_rng(seed)
    u = 3.0 * 2.0 * math.tan(0.5 * FOVX) / W
    hx, hy = 0.5 * W * u, 0.5 * H * u
    parts = []          # (xyz, opacity, scales, rotations, object id)

    def ordinary(n, cx, cy, rx, ry, z0, z1, sigma_px, oid):
        xyz = np.stack([rng.uniform(cx - rx, cx + rx, n), rng.uniform(cy - ry, cy + ry, n), rng.uniform(z0, z1, n)], 1)
        sc = np.exp(rng.normal(math.log(sigma_px * u), 0.5, size=(n, 3)))
        rot = rng.normal(size=(n, 4))
        op = 1.0 / (1.0 + np.exp(-rng.normal(2.0, 1.5, n)))
        parts.append((xyz, op, sc, rot / np.linalg.norm(rot, axis=1, keepdims=True), np.full(n, oid)))

    def families(z, oid, ops, places):
        rows = []
        shapes = [((s, s, 0.2 * s), 0.0) for s in (0.55, 3.0, 10.0)]
        shapes += [((1000.0 * m, m, 0.5 * m), deg) for m in (0.55, 2.0) for deg in (0.0, 45.0, 135.0)]
        for op in ops:
            for sc, deg in shapes:
                for (x, y) in places:
                    rows.append(((x, y, z + 1e-3 * len(rows)), op, tuple(s * u for s in sc), _rot_z(deg)))
        parts.append((np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]),
                      np.stack([r[3] for r in rows]), np.full(len(rows), oid)))

    px = lambda i: (i + 0.5) * u - hx           # world x of pixel column i's centre (camera 0)
    py = lambda j: (j + 0.5) * u - hy
    ordinary(n_env, 0.0, 0.0, 1.3 * hx, 1.3 * hy, 0.0, 0.5, 1.5, 0)
    places = [(px(11), py(5)), (px(8) - 0.5 * u, py(16) - 0.5 * u), (px(-1), py(H // 2)), (px(W + 7), py(H + 7)), (1e6 * u, 0.0)]
    ops = [0.0, 1e-42, (1.0 / 255.0) * (1.0 - 1e-3), (1.0 / 255.0) * (1.0 + 1e-3), 0.5, 0.99, 1.0]
    families(0.6, 0, ops, places)
    if stack:       # > 128 faint entries over one quarter, in front of everything: its pixels saturate one after the other mid-list
        n = 320
        xyz = np.stack([px(19) + rng.normal(0, 2.5 * u, n), py(11) + rng.normal(0, 2.5 * u, n), np.linspace(-1.2, -1.0, n)], 1)
        parts.append((xyz, np.full(n, 0.1), np.full((n, 3), 3.0 * u) * np.array([1.0, 1.0, 0.1]), np.tile(_rot_z(0.0), (n, 1)),
                      np.zeros(n)))
    centres = [(-0.5 * hx, -0.3 * hy), (0.3 * hx, 0.25 * hy), (0.6 * hx, -0.55 * hy)]
    for oid, (cx, cy) in zip(ids, centres):
        r = clump_px * u
        ordinary(n_clump, cx, cy, r, r, -0.6, -0.4, min(1.2, 0.3 * clump_px), oid)
        if clump_px > 2.0:
            families(-0.3, oid, [0.5, 1.0], [(cx, cy)])
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([p[k] for p in parts], 0).astype(dt))
    n = sum(len(p[0]) for p in parts)
    shs = np.concatenate([rng.uniform(-1.5, 1.5, size=(n, 1, 3)), rng.normal(0.0, 0.1, size=(n, 15, 3))], 1).astype(np.float32)
    act = dict(means3d=cat(0, np.float32), opacities=cat(1, np.float32), scales=cat(2, np.float32), rotations=cat(3, np.float32),
               shs=shs)
    return act, cat(4, np.int32)


def _match_colour_depth(color, depth, o, tol=1e-4):
    """helpers.assert_images_match restricted to the two images the semantic pass has"""
    ok = ~o["ambig"].astype(bool)
    assert (~ok).mean() <= 5e-4
    assert np.abs(color - o["color"])[:, ok].max(initial=0) <= tol
    assert np.abs(depth.reshape(ok.shape) - o["out_depth"][0])[ok].max(initial=0) <= tol


def _check_scene(oracle, dev, W, H, act, oid, bg=BG, expect_sparse=False, background_planes=()):
    """``background_planes``: the mask planes that are 1 where no object reaches a pixel (bg within the threshold of their colour)"""
    import torch
    from helpers import assert_images_match, gpu_forward
    from pegasus_amd import frames as F, masks as M, rasterizer
    views = _views(W, H)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    orc = [oracle.forward(**act, sh_degree=3, **v.raster_kwargs(bg), num_threads=4, cull_mode=1) for v in views]

    # AUX kernel, one view, through the drop-in surface: lists, images, final_T, n_contrib (exact) against the oracle
    g = gpu_forward(act, views[0], sh_degree=3, bg=bg, device=str(dev))
    np.testing.assert_array_equal(g["gauss_sorted"], orc[0]["gauss_sorted"])
    assert_images_match(g, orc[0])

    # 3-view batch, AUX and plain: every view against the oracle; the plain kernel's images are the AUX kernel's
    specs = [rasterizer.ViewSpec(v.height, v.width, v.tanfovx, v.tanfovy, t(np.asarray(bg, np.float32)), t(v.world_view_transform),
                                 t(v.full_proj_transform), t(v.camera_center)) for v in views]
    cloud = dict(shs=t(act["shs"]), scales=t(act["scales"]), rotations=t(act["rotations"]), sh_degree=3)
    aux = rasterizer.forward_views(t(act["means3d"]), t(act["opacities"]), specs, want_radii=False, want_aux=True, **cloud)
    plain = rasterizer.forward_views(t(act["means3d"]), t(act["opacities"]), specs, want_radii=False, **cloud)
    torch.cuda.synchronize()
    for k, o in enumerate(orc):
        d = dict(color=aux[k]["color"].cpu().numpy(), out_depth=aux[k]["depth"].cpu().numpy(),
                 final_T=aux[k]["final_T"].cpu().numpy(), n_contrib=aux[k]["n_contrib"].cpu().numpy().astype(np.uint32))
        assert_images_match(d, o)
        assert torch.equal(plain[k]["color"], aux[k]["color"]) and torch.equal(plain[k]["depth"], aux[k]["depth"])
    np.testing.assert_array_equal(aux[0]["color"].cpu().numpy(), g["color"])
    np.testing.assert_array_equal(aux[0]["n_contrib"].cpu().numpy().astype(np.uint32), g["n_contrib"])

    # fused kernel with masks and records: scene images = the plain kernel's; semantic image, depth and masks = the separate
    # objects-only pass + color_masks; masks = color_masks of the fused semantic image; records = pgr_pack_records
    fr = F.FrameRenderer(act["means3d"], act["opacities"], act["scales"], act["rotations"], act["shs"], oid, sh_degree=3,
                         device=dev, bg=bg, spatial_order=False)
    K = fr.K
    fspecs = [fr.view_spec(v) for v in views]
    f = fr.alloc_frames(3, H, W, records=True)
    f["records"].fill_(0xAB)                        # nothing may survive from the allocation: every byte is written
    f["masks"].fill_(0xEE)
    f["seg"].fill_(-7.0)
    f["seg_depth"].fill_(-7.0)
    fr.render_frames(fspecs, f)
    sep = fr.render_batch(fspecs)
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(f["color"][k], plain[k]["color"]) and torch.equal(f["depth"][k], plain[k]["depth"])
    for key in ("color", "depth", "seg", "seg_depth", "masks"):
        assert torch.equal(f[key], sep[key]), key
    assert torch.equal(f["masks"], M.color_masks(f["seg"], fr.colors, M.MASK_THRESHOLD))
    want = M.record_views(M.pack_records(f["color"], f["depth"], f["masks"]), H, W, K)
    got = M.record_views(f["records"], H, W, K)
    assert want["mask_bits"].shape[-1] == (K + 7) // 8
    for key in want:
        assert torch.equal(got[key], want[key]), key
    covered = float(f["masks"].amax(1).float().mean())
    assert covered > 0.0
    # Pixels no object entry reaches hold the background, and their K verdicts are the background's: plane k is 1 exactly
    # where || bg - colour k || <= threshold -- in the planes and in the record's bits (byte k / 8, bit k % 8).  Whole
    # quarters of them take the background-only epilogue, which evaluates one colour per lane.
    bgv = torch.tensor(bg, dtype=torch.float32, device=dev)
    untouched = (f["seg_depth"][:, 0] == 0) & (f["seg"] == bgv.view(1, 3, 1, 1)).all(1)                  # [3, H, W]
    verdict = M.color_masks(bgv.view(1, 3, 1, 1).expand(1, 3, 16, 16).contiguous(), fr.colors, M.MASK_THRESHOLD)[0, :, 0, 0]
    assert sorted(int(k) for k in torch.nonzero(verdict).flatten()) == sorted(background_planes)
    assert torch.equal(f["masks"].permute(0, 2, 3, 1)[untouched], verdict.expand(int(untouched.sum()), K))
    bits = np.zeros((K + 7) // 8, np.uint8)
    for k in background_planes:
        bits[k // 8] |= 1 << (k % 8)
    assert torch.equal(got["mask_bits"][untouched].cpu(), torch.from_numpy(bits).expand(int(untouched.sum()), len(bits)))
    if expect_sparse:       # the background-only epilogue writes most of every plane
        assert covered < 0.05 + (1.0 if background_planes else 0.0) and float(untouched.float().mean()) > 0.9
    # the semantic image against the oracle's render of the objects alone in their semantic colours
    s = slice(fr.n_env, fr.n)
    sem_shs = fr.sem_shs.cpu().numpy()
    for k, v in enumerate(views):
        o = oracle.forward(means3d=act["means3d"][s], opacities=act["opacities"][s], scales=act["scales"][s],
                           rotations=act["rotations"][s], shs=sem_shs, sh_degree=0, **v.raster_kwargs(bg), num_threads=4, cull_mode=1)
        _match_colour_depth(f["seg"][k].cpu().numpy(), f["seg_depth"][k].cpu().numpy(), o)

    # fused AUX kernel: the same frames, and final_T / n_contrib of the plain AUX kernel bit for bit
    fa = fr.alloc_frames(3, H, W, records=True)
    fa["masks"].fill_(0xEE)
    outs = [dict(color=fa["color"][i], depth=fa["depth"][i], radii=None, sem_color=fa["seg"][i], sem_depth=fa["seg_depth"][i],
                 sem_masks=fa["masks"][i], record=fa["records"][i],
                 final_T=torch.empty((H, W), dtype=torch.float32, device=dev),
                 n_contrib=torch.empty((H, W), dtype=torch.int32, device=dev)) for i in range(3)]
    rasterizer.forward_views(fr.means3d, fr.opacities, fspecs, shs=fr.shs, scales=fr.scales, rotations=fr.rotations, sh_degree=3,
                             want_radii=False, outputs=outs, semantic=fr.semantic)
    torch.cuda.synchronize()
    for key in ("color", "depth", "seg", "seg_depth", "masks", "records"):
        assert torch.equal(fa[key], f[key]), key
    for k in range(3):
        assert torch.equal(outs[k]["final_T"], aux[k]["final_T"]) and torch.equal(outs[k]["n_contrib"], aux[k]["n_contrib"])

    # records-only views
    ro = fr.alloc_frames(3, H, W, records=True, images=False)
    ro["records"].fill_(0xCD)
    fr.render_frames_async(fspecs, ro, slot=0).wait()
    torch.cuda.synchronize()
    assert torch.equal(ro["records"], f["records"])

    # layered silhouette call against one pass + one mask launch per object
    assert torch.equal(fr.render_silhouettes(fspecs).clone(), fr.render_silhouettes_per_object(fspecs).clone())


@pytest.mark.parametrize("size", [(40, 24), (72, 56)])
@pytest.mark.parametrize("ids", [(1, 2, 3), (3, 6, 9)])
def test_every_kernel_form_on_small_ragged_images(oracle, gpu_device, size, ids):
    W, H = size
    act, oid = _scene(W, H, seed=SEED[W], ids=ids)
    assert 2000 <= len(oid) <= 4000
    _check_scene(oracle, gpu_device, W, H, act, oid)


@pytest.mark.parametrize("size", [(40, 24), (72, 56)])
def test_sparse_objects_on_a_nonzero_background(oracle, gpu_device, size):
    """Objects under 5 % of the image: nearly every quarter takes the background-only epilogue."""
    W, H = size
    act, oid = _scene(W, H, seed=1, clump_px=0.4, n_clump=30, n_env=1600)
    _check_scene(oracle, gpu_device, W, H, act, oid, expect_sparse=True)


# (ids of the three objects, index of the semantic colour the background takes, planes that are 1 over the background)
#   K = 3: one plane, first record byte;  K = 9: the plane of the SECOND record byte;  K = 70: the second trip of the
#   one-colour-per-lane loop (colours 64..69), neighbouring hues within the threshold of each other (five planes at once,
#   both sides of the 64-colour boundary), and the colour table read from memory (more than 64 objects)
BACKGROUND_ON = [((1, 2, 3), 1, (1,)), ((3, 6, 9), 8, (8,)), ((5, 66, 70), 66, (64, 65, 66, 67, 68))]


@pytest.mark.parametrize("size", [(40, 24), (72, 56)])
@pytest.mark.parametrize("ids,colour,planes", BACKGROUND_ON)
def test_background_inside_mask_colours(oracle, gpu_device, size, ids, colour, planes):
    """A background that IS one of the semantic colours: the background-only epilogue has to write ones -- into exactly the
    planes, record bytes and bits of the colours within the threshold of it."""
    from pegasus_amd import masks as M
    W, H = size
    bg = tuple(float(x) for x in M.generate_colors(ids[-1])[colour])
    act, oid = _scene(W, H, seed=1, ids=ids, clump_px=0.4, n_clump=30, n_env=1600)
    _check_scene(oracle, gpu_device, W, H, act, oid, bg=bg, expect_sparse=True, background_planes=planes)


@pytest.mark.parametrize("size", [(40, 24), (72, 56)])
def test_a_long_list_that_saturates_mid_list(oracle, gpu_device, size):
    """One quarter under 320 faint entries: its pixels saturate one after the other from the third batch on, so the alive box
    stays, shrinks and the walk ends before the list does."""
    W, H = size
    act, oid = _scene(W, H, seed=1, stack=True)
    views = _views(W, H)
    o = oracle.forward(**act, sh_degree=3, **views[0].raster_kwargs(BG), num_threads=4, cull_mode=1)
    tile = (11 // 16) * ((W + 15) // 16) + 19 // 16
    n_list = int(o["ranges"][tile, 1] - o["ranges"][tile, 0])
    nc = o["n_contrib"].reshape(H, W)[8:16, 16:24]
    assert n_list > 128 and 64 < int(nc.max()) < n_list and int(nc.max()) - int(nc.min()) > 8, (n_list, nc.min(), nc.max())
    assert float(o["final_T"].reshape(H, W)[11, 19]) < 1e-3
    _check_scene(oracle, gpu_device, W, H, act, oid)
