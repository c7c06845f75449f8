"""pgr_mesh_shade_textured on the GPU: every output equals the restatement (tests/mesh_texture_reference.py) bit for bit, with
both filters, with outputs left out, and an all-untextured call gives pgr_mesh_shade's bytes; then MeshSet / render on files."""
import ctypes as C

import numpy as np
import pytest

import mesh_shade_reference as SR
import mesh_texture_cases as TC
import mesh_texture_reference as TR
from test_mesh_shade_gpu import GUARD, OUTPUTS, guarded, run_kernels, upload

pytestmark = pytest.mark.gpu
ALL = tuple(OUTPUTS) + ("uv",)
SHAPES = dict(OUTPUTS, uv=("float32", 2))


def run_textured(c, texels, table, bilinear, request=ALL, with_textures=True):
    """pgr_mesh_visibility + pgr_mesh_shade_textured with guard regions around every output, the texels and the workspace."""
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
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    nb = int(L.pgr_mesh_visibility_workspace_bytes(len(jobs), arr))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    _lib.check(L.pgr_mesh_visibility(*common, _lib.ptr(keys), n_slots, _lib.ptr(cnt), _lib.ptr(ws), nb, stream), "pgr_mesh_visibility")
    nb2 = int(L.pgr_mesh_shade_textured_workspace_bytes(len(jobs), arr))
    assert nb2 > int(L.pgr_mesh_shade_workspace_bytes(len(jobs), arr))
    ws2 = guarded(nb2, torch.uint8, 0xA5)
    bufs = {name: guarded(n * max(SHAPES[name][1], 1), getattr(torch, SHAPES[name][0]), 77) for name in request}
    corner_uv = torch.from_numpy(np.concatenate([np.asarray(j["corner_uv"], np.float32).reshape(-1, 3, 2) for j in jobs])).cuda()
    assert corner_uv.shape[0] == face.shape[0]
    # the texels end where the allocation's guard begins: a read past a texture's last byte meets 0xEE or the guard, never
    # a neighbouring texture's value by luck
    tex = guarded(len(texels), torch.uint8, 0x11)
    tex[GUARD:GUARD + len(texels)] = torch.from_numpy(texels).cuda()
    rows = (_lib.PgrMeshTexture * len(table))(*[_lib.PgrMeshTexture(offset=o_, width=w, height=h) for o_, w, h in table])
    job_texture = (C.c_int32 * len(jobs))(*[int(j.get("texture", -1)) if with_textures else -1 for j in jobs])
    shade = _lib.PgrMeshShade(normals=_lib.ptr(normals), colors=_lib.ptr(colors), surf_colors=surf.ctypes.data_as(C.POINTER(C.c_float)),
                              light=(C.c_float * 3)(*np.asarray(o["light"], np.float32).tolist()), ambient=float(o["ambient"]),
                              bg=(C.c_float * 3)(*np.asarray(o["bg"], np.float32).tolist()),
                              **{name: _lib.ptr(b[GUARD:]) for name, b in bufs.items() if name != "uv"})
    textures = _lib.PgrMeshTextures(corner_uv=_lib.ptr(corner_uv), texels=_lib.ptr(tex[GUARD:]), texel_bytes=len(texels), n_textures=len(table),
                                    textures=rows, job_texture=job_texture,
                                    filter=_lib.PGR_TEXTURE_BILINEAR if bilinear else _lib.PGR_TEXTURE_NEAREST,
                                    uv=_lib.ptr(bufs["uv"][GUARD:]) if "uv" in bufs else None)
    _lib.check(L.pgr_mesh_shade_textured(*common, _lib.ptr(keys), n_slots, C.byref(shade), C.byref(textures), _lib.ptr(ws2[GUARD:]), nb2,
                                         stream), "pgr_mesh_shade_textured")
    torch.cuda.synchronize()
    for what, buf, count, fill in [("workspace", ws2, nb2, 0xA5)] + [(name, b, b.numel() - 2 * GUARD, 77) for name, b in bufs.items()]:
        assert (buf[:GUARD] == fill).all() and (buf[GUARD + count:] == fill).all(), f"guard of {what} overwritten"
    out = {name: b[GUARD:b.numel() - GUARD].reshape((n_slots, H, W) + ((SHAPES[name][1],) if SHAPES[name][1] else ())).cpu().numpy()
           for name, b in bufs.items()}
    out["keys"] = keys.reshape(n_slots, H, W).cpu().numpy().view(np.uint64)
    return out


@pytest.fixture(scope="module")
def packed():
    return TR.pack_textures(TC.textures())


@pytest.fixture(scope="module")
def references(packed):
    c = TC.shade_case()
    return {b: TR.shade_textured_f32(c["jobs"], c["W"], c["H"], c["near"], *packed, c["n_slots"], bilinear=b, **c["opts"]) for b in (False, True)}


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
def test_every_output_equals_the_restatement(packed, references, bilinear):
    c = TC.shade_case()
    got = run_textured(c, *packed, bilinear)
    again = run_textured(c, *packed, bilinear)
    ref = references[bilinear]
    assert (got["keys"] == ref["keys"]).all()
    for name in ALL:
        assert got[name].tobytes() == again[name].tobytes(), f"two runs differ in {name}"
        diff = ~TR.same_bits(got[name], ref[name])
        print(f"{name}: {int(diff.sum())} of {diff.size} elements differ from the restatement")
        assert not diff.any(), name
    hit = ref["job_id"] >= 0
    assert set(np.unique(ref["job_id"][0])) == {-1, 0, 1, 2} and set(np.unique(ref["job_id"][1])) == {-1, 3, 4}
    assert np.isnan(got["uv"]).any() and not np.isnan(got["rgb"]).any()          # a NaN coordinate reads texel 0
    assert (got["uv"][~hit] == 0).all() and (got["rgb"][~hit] == np.float32(c["opts"]["bg"])).all()


@pytest.mark.parametrize("request_", [("rgb",), ("uv", "face_id"), ("depth",)], ids=lambda r: "+".join(r))
def test_outputs_left_out_change_nothing_else(packed, references, request_):
    got = run_textured(TC.shade_case(), *packed, True, request_)
    for name in request_:
        assert TR.same_bits(got[name], references[True][name]).all(), name


def test_untextured_jobs_give_the_bytes_of_pgr_mesh_shade(packed):
    c = TC.shade_case(textured=False)
    plain = run_kernels(c)
    for with_textures in (False, True):          # job_texture all -1 through the argument, and through the case
        got = run_textured(c, *packed, True, with_textures=with_textures)
        for name in OUTPUTS:
            assert got[name].tobytes() == plain[name].tobytes(), name
    # and the untextured job among textured ones
    mixed = run_textured(TC.shade_case(), *packed, False)
    own = mixed["job_id"] == 2
    assert own.sum() > 50 and TR.same_bits(mixed["rgb"][own], plain["rgb"][own]).all()


# ---- the atlas ----------------------------------------------------------------------------------------------------------
def run_atlas_points(v, f, cell):
    """pgr_mesh_atlas_points with guard regions around its three outputs."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    W, H = TR.atlas_layout(len(f), cell)[:2]
    n = W * H
    dv = torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    df = torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()
    bufs = dict(points=guarded(3 * n, torch.float32, 77), normals=guarded(3 * n, torch.float32, 77), owner=guarded(n, torch.int32, 77))
    _lib.check(L.pgr_mesh_atlas_points(len(v), _lib.ptr(dv), len(f), _lib.ptr(df), cell, W, H, *[_lib.ptr(b[GUARD:]) for b in bufs.values()],
                                       _lib.stream_ptr(dv.device)), "pgr_mesh_atlas_points")
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert (b[:GUARD] == 77).all() and (b[b.numel() - GUARD:] == 77).all(), f"guard of {name} overwritten"
    cut = lambda b: b[GUARD:b.numel() - GUARD].cpu().numpy()
    return cut(bufs["points"]).reshape(n, 3), cut(bufs["normals"]).reshape(n, 3), cut(bufs["owner"])


def run_atlas_pack(n_faces, cell, owner, colors, seen, face_fill, fill=(9, 99, 199)):
    """pgr_mesh_atlas_pack with guard regions around both outputs."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    W, H = TR.atlas_layout(n_faces, cell)[:2]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_owner, d_colors, d_seen, d_fill = dev(owner.astype(np.int32)), dev(colors.astype(np.float32)), dev(seen.astype(np.int32)), dev(face_fill)
    texture, face_seen = guarded(3 * W * H, torch.uint8, 77), guarded(n_faces, torch.int32, 77)
    _lib.check(L.pgr_mesh_atlas_pack(n_faces, cell, W, H, _lib.ptr(d_owner), _lib.ptr(d_colors), _lib.ptr(d_seen), _lib.ptr(d_fill),
                                     (C.c_uint8 * 3)(*fill), _lib.ptr(texture[GUARD:]), _lib.ptr(face_seen[GUARD:]),
                                     _lib.stream_ptr(d_owner.device)), "pgr_mesh_atlas_pack")
    torch.cuda.synchronize()
    for name, b in (("texture", texture), ("face_seen", face_seen)):
        assert (b[:GUARD] == 77).all() and (b[b.numel() - GUARD:] == 77).all(), f"guard of {name} overwritten"
    return texture[GUARD:GUARD + 3 * W * H].reshape(H, W, 3).cpu().numpy(), face_seen[GUARD:GUARD + n_faces].cpu().numpy()


@pytest.mark.parametrize("name", list(TC.atlas_meshes()))
def test_atlas_points_and_pack_equal_the_restatement(name):
    v, f, cell = TC.atlas_meshes()[name]
    want = TR.atlas_points_f32(v, f, cell)
    got, again = run_atlas_points(v, f, cell), run_atlas_points(v, f, cell)
    for what, g, a, w in zip(("points", "normals", "face_of_texel"), got, again, want):
        assert g.tobytes() == a.tobytes(), f"two runs differ in {what}"
        assert TR.same_bits(g, w).all(), f"{what}: {int((~TR.same_bits(g, w)).sum())} elements differ from the restatement"
    owner = got[2]
    assert (owner >= 0).any() and ((owner < 0).any() or len(f) % 2 == 0)
    colors, seen, face_fill = TC.pack_inputs(owner, len(f))
    kinds = {int(k) for k in np.unique(owner[owner >= 0] % 3)}
    for fill_rows in (face_fill, None):
        want_tex, want_seen = TR.atlas_pack(len(f), cell, owner, colors, seen, fill_rows, fill=(9, 99, 199))
        tex, face_seen = run_atlas_pack(len(f), cell, owner, colors, seen, fill_rows)
        tex2, face_seen2 = run_atlas_pack(len(f), cell, owner, colors, seen, fill_rows)
        assert tex.tobytes() == tex2.tobytes() and face_seen.tobytes() == face_seen2.tobytes(), "two runs differ"
        np.testing.assert_array_equal(face_seen, want_seen)
        assert (tex == want_tex).all(), f"{int((tex != want_tex).sum())} bytes differ from the restatement"
    if len(f) >= 3:
        assert kinds == {0, 1, 2} or name.startswith("degenerate")    # fully seen, partly seen and unseen faces


def device_views(raw):
    import torch
    from pegasus_amd.rasterizer import ViewSpec
    dev = lambda a: torch.as_tensor(np.asarray(a, np.float32), device="cuda")
    return [ViewSpec(v.height, v.width, v.tanfovx, v.tanfovy, dev(np.zeros(3)), dev(v.world_view_transform), dev(v.full_proj_transform),
                     dev(v.camera_center), depth_mode=1) for v in raw]


def test_bake_then_render_gives_the_views_colour_back(gpu_device):
    import torch
    from pegasus_amd import mesh as M, mesh_render as R
    r = TC.round_trip()
    assert r["share"] >= 0.5 and r["covered"] > 500                     # what the builder confirmed with the restatement
    c = r["case"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    info, stage_ms = {}, {}
    baked = M.bake_views(M.Mesh(r["vertices"], r["faces"]), dev(r["color"]), dev(c.depth), dev(c.final_T), device_views(c.raw),
                         cell=TC.ROUND_TRIP_CELL, depth_tol=r["depth_tol"], alpha_min=c.alpha_min, cos_min=c.cos_min, info=info,
                         stage_ms=stage_ms)
    assert baked.texture.dtype == np.uint8 and baked.texture.shape == r["texture"].shape and info["atlas"] == (56, 48)
    assert baked.corner_uv.tobytes() == r["corner_uv"].tobytes() and set(stage_ms) == {"atlas_points", "atlas_colors", "atlas_pack"}
    np.testing.assert_array_equal(info["face_seen"], r["face_seen"])
    np.testing.assert_array_equal(baked.texture, r["texture"])
    W, H = r["size"]
    p = r["pose"]
    K = np.array([[p["fx"], 0, p["cx"]], [0, p["fy"], p["cy"]], [0, 0, 1.0]])
    ms = R.MeshSet({1: baked}, device=gpu_device, textures=True)
    out = R.render(ms, [(1, p["R"], p["t"])], K, (W, H), outputs=("rgb", "face_id", "uv"), shading="flat", ambient=1.0, texture_filter="nearest")
    rgb, face = out["rgb"][0].cpu().numpy(), out["face_id"][0].cpu().numpy()
    covered = face >= 0
    good = covered & (info["face_seen"][np.where(covered, face, 0)] > 0)
    err = np.abs(rgb[good].astype(np.float64) - r["colour"].astype(np.float64)[None, :])
    print(f"view {r['view']}: {int(covered.sum())} covered pixels, {int(good.sum())} on seen faces, largest error {err.max():.3g}")
    assert good.sum() * 2 >= covered.sum() and covered.sum() == r["covered"]
    assert (err <= 0.5 / 255 + 2.0 ** -20).all()
    assert TR.same_bits(rgb, r["ref"]["rgb"][0]).all() and TR.same_bits(out["uv"][0].cpu().numpy(), r["ref"]["uv"][0]).all()


def test_decimate_texture_writes_a_model_that_renders_textured(gpu_device, tmp_path):
    from PIL import Image
    from pegasus_amd import decimate as D, mesh as M, mesh_render as R
    from pegasus_amd.ply_io import read_ply_model
    from test_mesh_attr_gpu import coloured_box_model, held_out_view
    model = coloured_box_model(n=20_000)
    model.save_ply(tmp_path / "model" / "point_cloud" / "iteration_30" / "point_cloud.ply")
    M.write_ply(tmp_path / "models" / "obj_000003.ply", M.extract_mesh(model, resolution=48, n_views=24, image_size=128), scale=1000.0)
    assert D.main(["--models", str(tmp_path / "models"), "--faces", "300", "--normals", "--texture", "-m", str(tmp_path / "model"),
                   "--texel_cell", "6", "--n_views", "24", "--image_size", "128"]) == 0
    out = tmp_path / "models_eval"
    m = read_ply_model(out / "obj_000003.ply", texture=True)
    F = len(m["faces"])
    w, h, _cols, _rows, uv = M.texture_atlas_layout(F, 6)
    assert 0 < F <= 300 and m["texture_file"] == "obj_000003.png" and "normals" in m
    np.testing.assert_array_equal(m["texture_uv_face"].astype(np.float32), uv.reshape(-1, 6))
    with Image.open(out / "obj_000003.png") as im:
        assert im.size == (w, h) and im.mode == "RGB"
        image = np.asarray(im)
    # the box's faces are painted 0.1 / 0.9 per channel: a baked atlas holds those colours, not the fill's grey alone
    assert (np.abs(image.astype(int) - 128) > 60).mean() > 0.3
    spec, Rm, t, K = held_out_view(96)
    size = (spec.image_width, spec.image_height)
    textured = R.MeshSet.from_dir(out, device=gpu_device, scale=0.001, textures=True)
    plain = R.MeshSet.from_dir(tmp_path / "models", device=gpu_device, scale=0.001)
    assert textured.texture_table == [(0, w, h)] and plain.texels is None
    a = R.render(textured, [(3, Rm, t)], K, size, outputs=("rgb", "depth"), ambient=1.0)
    b = R.render(plain, [(3, Rm, t)], K, size, outputs=("rgb", "depth"), shading="flat", ambient=1.0)
    hit = (a["depth"][0] > 0).cpu().numpy()
    rgb = a["rgb"][0].cpu().numpy()[hit]
    assert hit.sum() > 500 and (b["rgb"][0][b["depth"][0] > 0] == 0.5).all()          # the untextured model renders grey
    assert (np.abs(rgb - 0.5) > 0.25).mean() > 0.5                                   # the textured one in the box's colours


def test_renderer_picks_a_models_texture_up_as_the_toolkits_does(gpu_device, tmp_path):
    """A BOP model file with texture_u / texture_v and a TextureFile beside it: textured unless a surf_color is given."""
    from PIL import Image
    import mesh_raster_cases as MC
    from pegasus_amd import mesh_render as R
    from pegasus_amd.ply_io import write_ply_model
    from test_mesh_shade_gpu import as_job, to_uint8
    rng = np.random.default_rng(70)
    v, f = MC.icosphere(2, 40.0)
    uv = rng.random((len(v), 2)).astype(np.float32)
    image = rng.integers(0, 256, (7, 9, 3)).astype(np.uint8)
    colors = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    normals = R.vertex_normals(v, f).astype(np.float32)
    path = tmp_path / "models" / "obj_000001.ply"
    write_ply_model(path, v, f, normals=normals, colors=colors, texture_uv=uv, texture_file="obj_000001.png")
    Image.fromarray(image).save(path.with_suffix(".png"))
    W, H = 64, 48
    K = np.array([[120.0, 0, 31.5], [0, 120.0, 24.25], [0, 0, 1.0]])
    rot, t = MC.rotation((1, 2, 3), 0.7), np.array([5.0, -3.0, 400.0])
    mesh = dict(vertices=v, faces=f, normals=normals, colors=(colors.astype(np.float64) / 255.0).astype(np.float32), corner_uv=uv[f], texture=0)
    texels, table = TR.pack_textures([image], lead=0, gap=0)
    for filt in ("nearest", "bilinear"):
        ren = R.Renderer(W, H, mode="rgb+depth", texture_filter=filt)
        ren.add_object(1, path)
        out = ren.render_object(1, rot, t, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        ref = TR.shade_textured_f32([as_job(mesh, rot, t, K)], W, H, R.DEFAULT_NEAR, texels, table, bilinear=filt == "bilinear", smooth=True,
                                    use_colors=True)
        assert (out["depth"] > 0).sum() > 300 and out["depth"].tobytes() == ref["depth"][0].tobytes()
        np.testing.assert_array_equal(out["rgb"], to_uint8(ref["rgb"][0]))
    plain = SR.shade_f32([as_job(mesh, rot, t, K)], W, H, R.DEFAULT_NEAR, smooth=True, use_colors=True)
    assert (to_uint8(plain["rgb"][0]) != out["rgb"]).mean() > 0.05                    # the texture, not the vertex colours
    grey = R.Renderer(W, H, mode="rgb")
    grey.add_object(1, path, surf_color=(0.2, 0.4, 0.6))
    out = grey.render_object(1, rot, t, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    ref = SR.shade_f32([dict(as_job(mesh, rot, t, K), surf_color=(0.2, 0.4, 0.6))], W, H, R.DEFAULT_NEAR, smooth=True)
    np.testing.assert_array_equal(out["rgb"], to_uint8(ref["rgb"][0]))
    # the overlay of vis_object_poses shows the texture when the set was loaded with it
    meshes = R.MeshSet({1: path}, device=gpu_device, textures=True)
    photo = np.zeros((H, W, 3), np.uint8)
    got = R.vis_object_poses([dict(obj_id=1, R=rot, t=t.reshape(3, 1))], K, meshes, rgb=photo, vis_rgb_path=tmp_path / "vis.png")
    ref = TR.shade_textured_f32([as_job(mesh, rot, t, K)], W, H, R.DEFAULT_NEAR, texels, table, smooth=True, use_colors=True)
    own = to_uint8(ref["rgb"][0])
    inside = own.any(2)
    np.testing.assert_array_equal(got["vis_rgb"][inside][:, :], np.minimum(0.5 * own[inside].astype(np.float32) + _box(own)[inside], 255).astype(np.uint8))


def _box(own):
    """The grey bounding-box outline vis_object_poses adds, as float32 [H,W,3]."""
    from pegasus_amd.mesh_render import BBOX_GREY
    info = np.zeros(own.shape, np.float32)
    ys, xs = own.any(2).nonzero()
    x0, y0, x1, y1 = xs.min(), ys.min(), xs.max(), ys.max()
    info[y0, x0:x1 + 1] = info[y1, x0:x1 + 1] = BBOX_GREY
    info[y0:y1 + 1, x0] = info[y0:y1 + 1, x1] = BBOX_GREY
    return info


def test_mesh_command_line_writes_a_textured_visual(gpu_device, tmp_path):
    from PIL import Image
    from pegasus_amd import mesh as M
    from test_mesh_attr_gpu import coloured_box_model
    coloured_box_model(n=20_000).save_ply(tmp_path / "model" / "point_cloud" / "iteration_30" / "point_cloud.ply")
    args = ["-m", str(tmp_path / "model"), "--obj_id", "3", "--resolution", "48", "--n_views", "24", "--image_size", "128"]
    assert M.main(args + ["--out", str(tmp_path / "a"), "--collision_faces", "200"]) == 0
    assert M.main(args + ["--out", str(tmp_path / "b"), "--collision_faces", "200", "--texture", "--texel_cell", "6"]) == 0
    with pytest.raises(SystemExit):
        M.main(args + ["--out", str(tmp_path / "c"), "--texture"])                      # nothing to texture without --collision_faces
    a, b = tmp_path / "a" / "urdf", tmp_path / "b" / "urdf"
    for name in ("obj_000003.obj", "obj_000003_collision.obj"):
        assert (a / name).read_bytes() == (b / name).read_bytes()
    assert not (a / "obj_000003_textured.obj").exists()
    lines = (b / "obj_000003_textured.obj").read_text().splitlines()
    F = sum(l.startswith("f ") for l in lines)
    assert F == sum(l.startswith("f ") for l in (b / "obj_000003_collision.obj").read_text().splitlines()) and 0 < F <= 200
    assert sum(l.startswith("vt ") for l in lines) == 3 * F and "map_Kd obj_000003_textured.png" in (b / "obj_000003_textured.mtl").read_text()
    with Image.open(b / "obj_000003_textured.png") as im:
        assert im.size == M.texture_atlas_layout(F, 6)[:2]
    urdf = (b / "obj_000003.urdf").read_text()
    assert 'filename="obj_000003_textured.obj"' in urdf.split("<visual>")[1].split("</visual>")[0]
    assert 'filename="obj_000003_collision.obj"' in urdf.split("<collision>")[1]
    assert "textured" not in (a / "obj_000003.urdf").read_text()
