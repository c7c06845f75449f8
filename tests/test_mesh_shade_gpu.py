"""pgr_mesh_visibility and pgr_mesh_shade on the GPU: every output equals the float32 transcription
(tests/mesh_shade_reference.py) bit for bit, the depth equals pgr_mesh_depth's bytes, two runs give equal bytes, guard
regions stay untouched; then Renderer, vis_object_poses and the command line end to end."""
import ctypes as C
import json

import numpy as np
import pytest

import mesh_raster_cases as MC
import mesh_shade_cases as SC
import mesh_shade_reference as SR

pytestmark = pytest.mark.gpu
GUARD = 4096
OUTPUTS = {"depth": ("float32", 0), "face_id": ("int32", 0), "job_id": ("int32", 0), "xyz": ("float32", 3), "normal": ("float32", 3),
           "rgb": ("float32", 3)}


def upload(jobs, smooth, use_colors):
    """Concatenated device arrays and the PgrMeshJob array; jobs sharing a vertex array object share its range."""
    import torch
    from pegasus_amd import _lib
    ranges, vs, fs, ns, cs, v0, f0 = {}, [], [], [], [], 0, 0
    for j in jobs:
        key = id(j["vertices"])
        if key not in ranges:
            ranges[key] = (v0, len(j["vertices"]), f0, len(j["faces"]))
            vs.append(j["vertices"]); fs.append(np.asarray(j["faces"]).reshape(-1, 3))
            ns.append(j["normals"] if smooth else None); cs.append(j["colors"] if use_colors else None)
            v0 += len(j["vertices"]); f0 += len(j["faces"])
    dev = lambda parts, dt: torch.from_numpy(np.concatenate(parts).astype(dt).reshape(-1, 3)).cuda()
    arr = (_lib.PgrMeshJob * len(jobs))()
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32).reshape(-1).tolist()
    for k, j in enumerate(jobs):
        r = ranges[id(j["vertices"])]
        arr[k] = _lib.PgrMeshJob(vertex_first=r[0], vertex_count=r[1], face_first=r[2], face_count=r[3], R=(C.c_float * 9)(*f32(j["R"])),
                                 t=(C.c_float * 3)(*f32(j["t"])), fx=f32(j["fx"])[0], fy=f32(j["fy"])[0], cx=f32(j["cx"])[0],
                                 cy=f32(j["cy"])[0], slot=j["slot"])
    surf = np.array([j.get("surf_color", (0.5, 0.5, 0.5)) for j in jobs], np.float32).reshape(-1, 3)
    return (dev(vs, np.float32), dev(fs, np.int32), dev(ns, np.float32) if smooth else None, dev(cs, np.float32) if use_colors else None,
            arr, surf)


def guarded(n, dtype, fill):
    import torch
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")


def run_kernels(c, request=tuple(OUTPUTS), default_surf=False):
    """Both passes with guard regions around the keys, every output and both workspaces.  Returns {name: array} of the
    requested outputs plus keys, straddle and the bytes pgr_mesh_depth writes for the same call."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    jobs, W, H, near = c["jobs"], c["W"], c["H"], c["near"]
    o = dict(SR.DEFAULTS, **c["opts"])
    n_slots = SR._n_slots(jobs, c["n_slots"])
    vert, face, normals, colors, arr, surf = upload(jobs, o["smooth"], o["use_colors"])
    n = n_slots * H * W
    common = (_lib.ptr(vert), vert.shape[0], _lib.ptr(face), face.shape[0], len(jobs), arr, W, H, float(near))
    stream = _lib.stream_ptr(vert.device)
    cnt = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    # pgr_mesh_depth of the same call
    nb = int(L.pgr_mesh_depth_workspace_bytes(len(jobs), arr))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    depth_ref = torch.empty(n, dtype=torch.float32, device="cuda")
    _lib.check(L.pgr_mesh_depth(*common, _lib.ptr(depth_ref), n_slots, _lib.ptr(cnt[1:]), _lib.ptr(ws), nb, stream), "pgr_mesh_depth")
    straddle_ref = int(cnt[1])
    # the visibility pass
    nb = int(L.pgr_mesh_visibility_workspace_bytes(len(jobs), arr))
    assert nb > 0
    ws = guarded(nb, torch.uint8, 0xA5)
    keys = guarded(n, torch.int64, 0x5A5A5A5A5A5A5A5A)
    cnt[1] = -7
    _lib.check(L.pgr_mesh_visibility(*common, _lib.ptr(keys[GUARD:]), n_slots, _lib.ptr(cnt[1:]), _lib.ptr(ws[GUARD:]), nb, stream),
               "pgr_mesh_visibility")
    # the resolve pass
    nb2 = int(L.pgr_mesh_shade_workspace_bytes(len(jobs), arr))
    assert nb2 > 0
    ws2 = guarded(nb2, torch.uint8, 0xA5)
    bufs = {}
    for name in request:
        dt, ch = OUTPUTS[name]
        bufs[name] = guarded(n * max(ch, 1), getattr(torch, dt), 77)
    shade = _lib.PgrMeshShade(normals=_lib.ptr(normals), colors=_lib.ptr(colors),
                              surf_colors=None if default_surf else surf.ctypes.data_as(C.POINTER(C.c_float)),
                              light=(C.c_float * 3)(*np.asarray(o["light"], np.float32).tolist()), ambient=float(o["ambient"]),
                              bg=(C.c_float * 3)(*np.asarray(o["bg"], np.float32).tolist()),
                              **{name: _lib.ptr(b[GUARD:]) for name, b in bufs.items()})
    _lib.check(L.pgr_mesh_shade(*common, _lib.ptr(keys[GUARD:]), n_slots, C.byref(shade), _lib.ptr(ws2[GUARD:]), nb2, stream), "pgr_mesh_shade")
    torch.cuda.synchronize()
    for what, buf, count, fill in [("keys", keys, n, 0x5A5A5A5A5A5A5A5A), ("visibility workspace", ws, nb, 0xA5), ("shade workspace", ws2, nb2, 0xA5)] + \
            [(name, b, b.numel() - 2 * GUARD, 77) for name, b in bufs.items()]:
        assert (buf[:GUARD] == fill).all() and (buf[GUARD + count:] == fill).all(), f"guard of {what} overwritten"
    assert int(cnt[0]) == -7 and int(cnt[2]) == -7
    out = {name: b[GUARD:b.numel() - GUARD].reshape((n_slots, H, W) + ((OUTPUTS[name][1],) if OUTPUTS[name][1] else ())).cpu().numpy()
           for name, b in bufs.items()}
    out["keys"] = keys[GUARD:GUARD + n].reshape(n_slots, H, W).cpu().numpy().view(np.uint64)
    out["straddle"] = int(cnt[1])
    out["depth_ref"] = depth_ref.reshape(n_slots, H, W).cpu().numpy()
    assert out["straddle"] == straddle_ref
    return out


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_case(name, c, request=tuple(OUTPUTS)):
    got = run_kernels(c, request)
    again = run_kernels(c, request)
    for key in request + ("keys",):
        assert got[key].tobytes() == again[key].tobytes(), f"two runs differ in {key}"
    ref = SR.shade_f32(c["jobs"], c["W"], c["H"], c["near"], c["n_slots"], **c["opts"])
    print(f"{name}: {int((ref['job_id'] >= 0).sum())} covered pixels, straddle {got['straddle']} (reference {ref['straddle']})")
    assert got["straddle"] == ref["straddle"]
    if c["straddle"] is not None:
        assert got["straddle"] == c["straddle"]
    assert (got["keys"] >> np.uint64(32)).astype(np.uint32).tobytes() == got["depth_ref"].tobytes(), "the keys' high words are not pgr_mesh_depth's bytes"
    for key in ("keys",) + tuple(request):
        diff = bits(got[key]) != bits(ref[key])
        print(f"{name}: {key}: {int(diff.sum())} of {diff.size} elements differ from the transcription")
        assert not diff.any(), f"{key}: {int(diff.sum())} elements differ from the float32 transcription"
    if "depth" in request:
        assert got["depth"].tobytes() == got["depth_ref"].tobytes()
    return got


@pytest.mark.parametrize("name", list(SC.CASES))
def test_case_equals_the_transcription_bit_for_bit(name):
    c = SC.CASES[name]()
    got = check_case(name, c)
    if name == "zero faces":
        assert (got["keys"] == 0).all() and (got["rgb"] == np.float32([0.25, 0.5, 0.75])).all()
    else:
        assert (got["job_id"] >= 0).any()
    if name.startswith("rotated triangle"):
        assert got["depth"][0].tobytes() == MC.rotated_triangle_case()[3].tobytes()
    if name == "coincident faces and jobs":
        hit = got["job_id"][1] >= 0
        assert (got["face_id"][1][hit] == 0).all()                          # of two coincident faces the lower index
        assert set(np.unique(got["job_id"][0])) == {-1, 0, 2}               # of two coincident jobs the lower; job 2 is nearer


@pytest.mark.parametrize("request_", [("face_id",), ("rgb",)], ids=lambda r: r[0])
def test_only_one_output_requested(request_):
    check_case("icosphere smooth, only " + request_[0], SC.CASES["icosphere smooth"](), request_)


def test_default_surf_colour_is_the_toolkits_grey():
    c = SC.CASES["surf colours"]()
    for j in c["jobs"]:
        j.pop("surf_color")
    got = run_kernels(c, ("rgb",), default_surf=True)
    ref = SR.shade_f32(c["jobs"], c["W"], c["H"], c["near"], c["n_slots"], **c["opts"])
    assert got["rgb"].tobytes() == ref["rgb"].tobytes()


# ---- end to end ---------------------------------------------------------------------------------------------------------
def coloured_sphere(tmp_path, obj_id=1, radius=40.0, seed=12):
    """A coloured icosphere written as a BOP model file (millimetres); returns (path, job pieces for the transcription)."""
    from pegasus_amd import mesh_render as R
    from pegasus_amd.ply_io import write_ply_model
    v, f = MC.icosphere(2, radius)
    colors = np.random.default_rng(seed).integers(0, 256, (len(v), 3)).astype(np.uint8)
    normals = R.vertex_normals(v, f).astype(np.float32)
    path = tmp_path / "models" / f"obj_{obj_id:06d}.ply"
    write_ply_model(path, v, f, normals=normals, colors=colors)
    return path, dict(vertices=v, faces=f, normals=normals, colors=(colors.astype(np.float64) / 255.0).astype(np.float32))


def as_job(mesh, R, t, K, slot=0):
    return dict(mesh, R=np.asarray(R, np.float64), t=np.asarray(t, np.float64), fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], slot=slot)


def to_uint8(rgb):
    return np.rint(np.float32(255) * np.clip(rgb, np.float32(0), np.float32(1))).astype(np.uint8)


def test_renderer_render_object_on_a_model_file(tmp_path):
    from pegasus_amd import mesh_render as R
    path, mesh = coloured_sphere(tmp_path)
    W, H = 64, 48
    K = np.array([[120.0, 0, 31.5], [0, 120.0, 24.25], [0, 0, 1.0]])
    rot, t = MC.rotation((1, 2, 3), 0.7), np.array([5.0, -3.0, 400.0])
    for shading in ("phong", "flat"):
        ren = R.Renderer(W, H, mode="rgb+depth", shading=shading)
        ren.add_object(1, path)
        ren.set_light_cam_pos([100.0, -50.0, 0.0])
        ren.set_light_ambient_weight(0.4)
        out = ren.render_object(1, rot, t.reshape(3, 1), K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        ref = SR.shade_f32([as_job(mesh, rot, t, K)], W, H, R.DEFAULT_NEAR, smooth=shading == "phong", use_colors=True,
                           light=(100.0, -50.0, 0.0), ambient=0.4)
        assert out["rgb"].dtype == np.uint8 and out["rgb"].shape == (H, W, 3) and out["depth"].shape == (H, W)
        assert out["depth"].tobytes() == ref["depth"][0].tobytes() and (out["depth"] > 0).sum() > 300
        np.testing.assert_array_equal(out["rgb"], to_uint8(ref["rgb"][0]))
    grey = R.Renderer(W, H, mode="rgb", shading="flat")
    grey.add_object(1, path, surf_color=(0.2, 0.4, 0.6))
    out = grey.render_object(1, rot, t, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    ref = SR.shade_f32([dict(as_job(mesh, rot, t, K), surf_color=(0.2, 0.4, 0.6))], W, H, R.DEFAULT_NEAR)
    assert set(out) == {"rgb"}
    np.testing.assert_array_equal(out["rgb"], to_uint8(ref["rgb"][0]))
    grey.remove_object(1)
    with pytest.raises(KeyError):
        grey.render_object(1, rot, t, K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def numpy_overlay(rgb, images):
    """The NumPy composition of vis_object_poses: ``images`` = (composite uint8 [H,W,3], [each object's own uint8 image])."""
    from pegasus_amd.mesh_render import BBOX_GREY
    ren, own = images
    info = np.zeros_like(rgb)
    for m in own:
        ys, xs = (m > 0).any(2).nonzero()
        if len(ys):
            x0, y0, x1, y1 = xs.min(), ys.min(), xs.max(), ys.max()
            info[y0, x0:x1 + 1] = info[y1, x0:x1 + 1] = BBOX_GREY
            info[y0:y1 + 1, x0] = info[y0:y1 + 1, x1] = BBOX_GREY
    vis = 0.5 * rgb.astype(np.float32) + 0.5 * ren.astype(np.float32) + info.astype(np.float32)
    return np.minimum(vis, 255).astype(np.uint8)


def test_vis_object_poses_in_both_visibility_modes(tmp_path):
    from pegasus_amd import bop_dataset as BD, mesh_render as R
    path, mesh = coloured_sphere(tmp_path)
    meshes = R.MeshSet({1: path})
    W, H = 64, 48
    K = np.array([[120.0, 0, 31.5], [0, 120.0, 24.25], [0, 0, 1.0]])
    poses = [dict(obj_id=1, R=MC.rotation((1, 2, 3), 0.7), t=np.array([[-20.0], [-3.0], [400.0]])),
             dict(obj_id=1, R=MC.rotation((0, 1, 0), 0.3), t=np.array([[25.0], [6.0], [330.0]]))]
    rgb = np.random.default_rng(13).integers(0, 256, (H, W, 3)).astype(np.uint8)
    depth = np.full((H, W), 350.0, np.float32)
    depth[:, :5] = 0
    jobs = [as_job(mesh, p["R"], p["t"].reshape(3), K, slot=k) for k, p in enumerate(poses)]
    own = to_uint8(SR.shade_f32(jobs, W, H, R.DEFAULT_NEAR, smooth=True, use_colors=True)["rgb"])
    shared = SR.shade_f32([dict(j, slot=0) for j in jobs], W, H, R.DEFAULT_NEAR, smooth=True, use_colors=True)
    for resolve in (False, True):
        got = R.vis_object_poses(poses, K, meshes, rgb=rgb, depth=depth, vis_rgb_path=tmp_path / f"vis{int(resolve)}" / "a.png",
                                 vis_depth_diff_path=tmp_path / f"diff{int(resolve)}.png", vis_rgb_resolve_visib=resolve)
        ren = to_uint8(shared["rgb"][0]) if resolve else np.minimum(own.astype(np.int64).sum(0), 255).astype(np.uint8)
        want = numpy_overlay(rgb, (ren, own))
        np.testing.assert_array_equal(got["vis_rgb"], want)
        np.testing.assert_array_equal(BD.decode_png((tmp_path / f"vis{int(resolve)}" / "a.png").read_bytes()), want)
        valid = (depth > 0) & (shared["depth"][0] > 0)
        np.testing.assert_array_equal(got["depth_diff"], valid * (shared["depth"][0] - depth))
        assert valid.sum() > 100 and (got["depth_diff"] != 0).sum() > 100
        assert BD.decode_png((tmp_path / f"diff{int(resolve)}.png").read_bytes()).shape == (H, W, 3)
    assert (own[0].any(2) & own[1].any(2)).sum() > 20                        # the two spheres overlap: the modes differ


def test_command_line_writes_overlays(tmp_path):
    from pegasus_amd import bop_dataset as BD, mesh_render as R, pose_eval
    path, mesh = coloured_sphere(tmp_path)
    W, H = 64, 48
    K = np.array([[120.0, 0, 31.5], [0, 120.0, 24.25], [0, 0, 1.0]])
    scene = BD.BopScene(tmp_path / "data" / "train" / "000003")
    scene.make_dirs(("rgb",))
    rng = np.random.default_rng(14)
    gt, cam, photos = {}, {}, {}
    for i in range(2):
        pose = (MC.rotation((1, 2, 3), 0.4 + i), np.array([10.0 * i, -4.0, 380.0 + 30 * i]))
        gt[str(i)] = [{"cam_R_m2c": pose[0].reshape(-1).tolist(), "cam_t_m2c": pose[1].tolist(), "obj_id": 1}]
        cam[str(i)] = {"cam_K": K.reshape(-1).tolist(), "depth_scale": 1.0}
        photos[i] = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        scene.image_path("rgb", i).write_bytes(BD.encode_png(photos[i]))
    scene.write_json(BD.SCENE_GT, gt)
    scene.write_json(BD.SCENE_CAMERA, cam)
    out = tmp_path / "vis"
    assert R.main(["--dataset", str(tmp_path / "data"), "--models", str(path.parent), "--vis", str(out), "--translation_scale", "1000"]) == 0
    files = sorted(p.relative_to(out).as_posix() for p in out.rglob("*.png"))
    assert files == ["000003/000000.png", "000003/000001.png"]
    for i in range(2):
        Rm, t = BD.pose_of(gt[str(i)][0])
        own = to_uint8(SR.shade_f32([as_job(mesh, Rm, t, K)], W, H, R.DEFAULT_NEAR, smooth=True, use_colors=True)["rgb"])
        np.testing.assert_array_equal(BD.decode_png((out / "000003" / f"{i:06d}.png").read_bytes()), numpy_overlay(photos[i], (own[0], own)))
    # the estimates of a results file instead: only image 1 has one
    est = dict(scene_id=3, im_id=1, obj_id=1, score=1.0, R=MC.rotation((0, 0, 1), 0.2), t=np.array([0.0, 0.0, 350.0]), time=-1)
    pose_eval.write_results(tmp_path / "est.csv", [est])
    out2 = tmp_path / "vis_est"
    assert R.main(["--dataset", str(tmp_path / "data"), "--models", str(path.parent), "--vis", str(out2), "--results", str(tmp_path / "est.csv"),
                   "--translation_scale", "1000", "--shading", "flat", "--resolve_visib"]) == 0
    np.testing.assert_array_equal(BD.decode_png((out2 / "000003" / "000000.png").read_bytes()), numpy_overlay(photos[0], (np.zeros_like(photos[0]), [])))
    own = to_uint8(SR.shade_f32([as_job(mesh, est["R"], est["t"], K)], W, H, R.DEFAULT_NEAR, use_colors=True)["rgb"])
    np.testing.assert_array_equal(BD.decode_png((out2 / "000003" / "000001.png").read_bytes()), numpy_overlay(photos[1], (own[0], own)))
    assert not (scene.path / "mask").exists() and json.loads((scene.path / BD.SCENE_GT).read_text()) == gt      # --vis recomputes nothing
