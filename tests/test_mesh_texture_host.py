"""Textured object models without a GPU: the PLY reader and writer, the OBJ + MTL writer, the atlas layout and its footprint
property, the mutants of the restatement (tests/mesh_texture_reference.py), and the argument checks of the new entries (host
code that runs before any launch: the pointers handed in are never dereferenced)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import mesh_raster_cases as MC
import mesh_texture_cases as TC
import mesh_texture_reference as TR
from pegasus_amd import _lib, ply_io as P

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
FAKE = C.c_void_p(4096)
NEW = ("pgr_mesh_shade_textured_workspace_bytes", "pgr_mesh_shade_textured", "pgr_mesh_atlas_points", "pgr_mesh_atlas_pack")

ASCII_TEXCOORD = """ply
format ascii 1.0
comment made by hand: the MeshLab layout
comment TextureFile skin.png
element vertex 4
property float x
property float y
property float z
element face 2
property list uchar int vertex_indices
property list uchar float texcoord
end_header
0 0 0
1 0 0
0 1 0
1 1 0.5
3 0 1 2 6 0 0 1 0 0 1
3 1 3 2 6 1 0 0.875 0.625 0.1 1
"""
UV_FACE = np.array([[0, 0, 1, 0, 0, 1], [1, 0, 0.875, 0.625, np.float32(0.1), 1]], np.float64)


# ---- files --------------------------------------------------------------------------------------------------------------
def test_reader_returns_the_toolkits_texture_uv_and_the_default_call_is_unchanged():
    g = np.load(GOLDEN / "bop_model.npz")
    m = P.read_ply_model(GOLDEN / "bop_model.ply", texture=True)
    assert set(m) == {"pts", "faces", "normals", "colors", "texture_uv"}
    assert m["texture_uv"].dtype == np.float64 and m["texture_uv"].shape == (42, 2)
    np.testing.assert_array_equal(m["texture_uv"], g["texture_uv"])
    plain = P.read_ply_model(GOLDEN / "bop_model.ply")
    assert set(plain) == {"pts", "faces", "normals", "colors"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], m[k])


def binary_twin(path, texcoord_first):
    """The hand-written file as binary little-endian, the two face lists in either order."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], "<f4")
    idx = [("n", "u1"), ("idx", "<i4", (3,))]
    uv = [("tn", "u1"), ("uv", "<f4", (6,))]
    rows = np.zeros(2, np.dtype(uv + idx if texcoord_first else idx + uv))
    rows["n"], rows["tn"], rows["idx"], rows["uv"] = 3, 6, [[0, 1, 2], [1, 3, 2]], UV_FACE
    lists = ["property list uchar int vertex_indices\n", "property list uint8 float32 texcoord\n"]
    header = ("ply\nformat binary_little_endian 1.0\ncomment TextureFile skin.png\nelement vertex 4\nproperty float x\nproperty float y\n"
              "property float z\nelement face 2\n" + "".join(lists[::-1] if texcoord_first else lists) + "end_header\n")
    path.write_bytes(header.encode() + v.tobytes() + rows.tobytes())


def test_texcoord_lists_read_equal_from_ascii_and_binary(tmp_path):
    (tmp_path / "a.ply").write_text(ASCII_TEXCOORD)
    a = P.read_ply_model(tmp_path / "a.ply", texture=True)
    assert set(a) == {"pts", "faces", "texture_uv_face", "texture_file"} and a["texture_file"] == "skin.png"
    assert a["texture_uv_face"].dtype == np.float64 and a["texture_uv_face"].shape == (2, 6)
    np.testing.assert_array_equal(a["texture_uv_face"].astype(np.float32), UV_FACE.astype(np.float32))
    np.testing.assert_array_equal(a["faces"], [[0, 1, 2], [1, 3, 2]])
    # texcoord in front of the index list, in ASCII
    swapped = re.sub(r"^3 (\S+ \S+ \S+) 6 (.*)$", r"6 \2 3 \1", ASCII_TEXCOORD, flags=re.M)
    swapped = swapped.replace("property list uchar int vertex_indices\nproperty list uchar float texcoord\n",
                              "property list uchar float texcoord\nproperty list uchar int vertex_indices\n")
    (tmp_path / "s.ply").write_text(swapped)
    files = [tmp_path / "s.ply"]
    for first in (False, True):
        binary_twin(tmp_path / f"b{int(first)}.ply", first)
        files.append(tmp_path / f"b{int(first)}.ply")
    for path in files:
        b = P.read_ply_model(path, texture=True)
        assert set(b) == set(a) and b["texture_file"] == "skin.png", path
        for k in ("pts", "faces"):
            np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a["texture_uv_face"].astype(np.float32), b["texture_uv_face"].astype(np.float32))
    # the default call still refuses the layout
    with pytest.raises(ValueError, match="unsupported face properties"):
        P.read_ply_model(tmp_path / "a.ply")


def test_a_texcoord_list_of_another_length_raises(tmp_path):
    (tmp_path / "five.ply").write_text(ASCII_TEXCOORD.replace("6 0 0 1 0 0 1", "5 0 0 1 0 0"))
    with pytest.raises(ValueError, match="texcoord"):
        P.read_ply_model(tmp_path / "five.ply", texture=True)
    v = np.zeros((3, 3), "<f4")
    rows = np.zeros(1, np.dtype([("n", "u1"), ("idx", "<i4", (3,)), ("tn", "u1"), ("uv", "<f4", (5,))]))
    rows["n"], rows["tn"], rows["idx"] = 3, 5, [[0, 1, 2]]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
              "property list uchar int vertex_indices\nproperty list uchar float texcoord\nend_header\n")
    (tmp_path / "five_b.ply").write_bytes(header.encode() + v.tobytes() + rows.tobytes())
    with pytest.raises(ValueError, match="texcoord"):
        P.read_ply_model(tmp_path / "five_b.ply", texture=True)


@pytest.mark.parametrize("ascii", [False, True], ids=["binary", "ascii"])
def test_write_then_read_round_trips_and_the_header_is_save_ply2s(tmp_path, ascii):
    rng = np.random.default_rng(3)
    v, f = MC.icosphere(0, 2.0)
    n, c = rng.normal(size=v.shape).astype(np.float32), rng.integers(0, 256, v.shape).astype(np.uint8)
    uv = rng.random((len(v), 2)).astype(np.float32)                   # floats with full mantissas: they survive both formats
    uvf = rng.random((len(f), 6)).astype(np.float32)
    P.write_ply_model(tmp_path / "m.ply", v, f, normals=n, colors=c, ascii=ascii, texture_uv=uv, texture_uv_face=uvf, texture_file="m.png")
    m = P.read_ply_model(tmp_path / "m.ply", texture=True)
    assert set(m) == {"pts", "faces", "normals", "colors", "texture_uv", "texture_uv_face", "texture_file"}
    assert m["texture_file"] == "m.png"
    np.testing.assert_array_equal(m["texture_uv"].astype(np.float32), uv)
    np.testing.assert_array_equal(m["texture_uv_face"].astype(np.float32), uvf)
    np.testing.assert_array_equal(m["pts"].astype(np.float32), v)
    np.testing.assert_array_equal(m["faces"], f)
    header = (tmp_path / "m.ply").read_bytes().split(b"end_header")[0].decode().split("\n")
    assert header[1].startswith("format ") and header[2] == "comment TextureFile m.png"
    assert [l.split()[-1] for l in header if l.startswith("property")] == \
        ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "texture_u", "texture_v", "vertex_indices", "texcoord"]
    assert "property list uchar float texcoord" in header
    # without the texture arguments the bytes are those of a call that never heard of them
    P.write_ply_model(tmp_path / "p.ply", v, f, normals=n, colors=c, ascii=ascii)
    P.write_ply_model(tmp_path / "q.ply", v, f, normals=n, colors=c, ascii=ascii, texture_uv=None, texture_uv_face=None, texture_file=None)
    assert (tmp_path / "p.ply").read_bytes() == (tmp_path / "q.ply").read_bytes()
    assert b"Texture" not in (tmp_path / "p.ply").read_bytes() and b"texcoord" not in (tmp_path / "p.ply").read_bytes()


def test_obj_and_mtl_parse_back_to_the_same_corner_uvs(tmp_path):
    from pegasus_amd import mesh as M
    v, f = MC.icosphere(1, 1.0)
    uv = M.texture_atlas_layout(len(f), 8)[4]
    mesh = M.Mesh(np.asarray(v, np.float32), np.asarray(f, np.int32), corner_uv=uv)
    M.write_obj_textured(tmp_path / "o" / "thing.obj", mesh, "thing.png")
    lines = (tmp_path / "o" / "thing.obj").read_text().splitlines()
    assert "mtllib thing.mtl" in lines
    vs = np.array([l.split()[1:] for l in lines if l.startswith("v ")], np.float64).astype(np.float32)
    vt = np.array([l.split()[1:] for l in lines if l.startswith("vt ")], np.float64).astype(np.float32)
    corners = np.array([[tuple(map(int, c.split("/"))) for c in l.split()[1:]] for l in lines if l.startswith("f ")])
    np.testing.assert_array_equal(vs, mesh.vertices)
    np.testing.assert_array_equal(corners[..., 0] - 1, mesh.faces)
    np.testing.assert_array_equal(vt[corners[..., 1] - 1], uv)
    mtl = (tmp_path / "o" / "thing.mtl").read_text().splitlines()
    assert "map_Kd thing.png" in mtl and any(l.startswith("newmtl ") for l in mtl)
    assert f"usemtl {[l for l in mtl if l.startswith('newmtl ')][0].split()[1]}" in lines
    assert not (tmp_path / "o" / "thing.png").exists()                # the image is the caller's to put there
    with pytest.raises(ValueError, match="corner_uv"):
        M.write_obj_textured(tmp_path / "x.obj", M.Mesh(mesh.vertices, mesh.faces), "x.png")
    # the URDF names it in <visual> only, and without the argument nothing changes
    closed = M.Mesh(mesh.vertices, mesh.faces)
    M.write_urdf(tmp_path / "a.urdf", "thing.obj", closed, 0.1, collision_filename="c.obj")
    M.write_urdf(tmp_path / "b.urdf", "thing.obj", closed, 0.1, collision_filename="c.obj", visual_filename=None)
    M.write_urdf(tmp_path / "c.urdf", "thing.obj", closed, 0.1, collision_filename="c.obj", visual_filename="thing_textured.obj")
    assert (tmp_path / "a.urdf").read_bytes() == (tmp_path / "b.urdf").read_bytes()
    text = (tmp_path / "c.urdf").read_text()
    visual, collision = text.split("<visual>")[1].split("</visual>")[0], text.split("<collision>")[1]
    assert 'filename="thing_textured.obj"' in visual and 'filename="c.obj"' in collision and "textured" not in collision


def test_write_ply_of_a_textured_mesh_writes_the_image_beside_it(tmp_path):
    from pegasus_amd import bop_dataset as BD, mesh as M
    v, f = TC.strip_mesh(5, 1)
    w, h, _c, _r, uv = M.texture_atlas_layout(5, 4)
    image = np.random.default_rng(4).integers(0, 256, (h, w, 3)).astype(np.uint8)
    M.write_ply(tmp_path / "models" / "obj_000007.ply", M.Mesh(v, f, corner_uv=uv, texture=image), scale=1000.0)
    m = P.read_ply_model(tmp_path / "models" / "obj_000007.ply", texture=True)
    assert m["texture_file"] == "obj_000007.png"
    np.testing.assert_array_equal(m["texture_uv_face"].astype(np.float32), uv.reshape(-1, 6))
    np.testing.assert_array_equal(BD.decode_png((tmp_path / "models" / "obj_000007.png").read_bytes()), image)
    np.testing.assert_array_equal(m["pts"].astype(np.float32), (v.astype(np.float64) * 1000.0).astype(np.float32))
    # an untextured mesh is written as before
    M.write_ply(tmp_path / "plain.ply", M.Mesh(v, f))
    P.write_ply_mesh(tmp_path / "want.ply", v, f)
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()


def test_mesh_set_loads_textures_and_refuses_what_it_cannot_read(tmp_path):
    from PIL import Image
    from pegasus_amd import mesh_render as R
    v, f = MC.icosphere(0, 2.0)
    rng = np.random.default_rng(5)
    uv = rng.random((len(v), 2)).astype(np.float32)
    uvf = rng.random((len(f), 6)).astype(np.float32)
    rgba = rng.integers(0, 256, (3, 5, 4)).astype(np.uint8)
    Image.fromarray(rgba).save(tmp_path / "one.png")
    Image.fromarray(rgba[..., 0]).save(tmp_path / "two.png")
    Image.fromarray(rgba[..., 0].astype(np.uint16) * 257).save(tmp_path / "deep.png")
    P.write_ply_model(tmp_path / "obj_000001.ply", v, f, texture_uv=uv, texture_file="one.png")
    P.write_ply_model(tmp_path / "obj_000002.ply", v, f, texture_uv=uv, texture_uv_face=uvf, texture_file="two.png")
    P.write_ply_model(tmp_path / "obj_000003.ply", v, f)
    files = {k: tmp_path / f"obj_{k:06d}.ply" for k in (1, 2, 3)}
    ms = R.MeshSet(files, device="cpu", textures=True)
    assert ms.texture_of == {1: 0, 2: 1, 3: -1} and ms.texture_table == [(0, 5, 3), (45, 5, 3)]
    cu = ms.corner_uv.numpy()
    np.testing.assert_array_equal(cu[:len(f)], uv[f])                                    # per-vertex UVs expanded to corners
    np.testing.assert_array_equal(cu[len(f):2 * len(f)], uvf.reshape(-1, 3, 2))         # per-face UVs win
    assert (cu[2 * len(f):] == 0).all() and len(cu) == 3 * len(f)
    tex = ms.texels.numpy()
    np.testing.assert_array_equal(tex[:45].reshape(3, 5, 3), rgba[..., :3])             # alpha dropped
    np.testing.assert_array_equal(tex[45:].reshape(3, 5, 3), np.repeat(rgba[..., :1], 3, 2))        # grey replicated
    # the default is today's behaviour for every file
    plain = R.MeshSet({1: files[1], 3: files[3]}, device="cpu")
    assert plain.corner_uv is None and plain.texels is None and plain.texture_table == []
    assert plain.vertices.numpy().tobytes() == R.MeshSet({1: files[1], 3: files[3]}, device="cpu", textures=True).vertices.numpy().tobytes()
    with pytest.raises(ValueError, match="unsupported face properties"):
        R.MeshSet(files, device="cpu")
    # a mesh object offers corner_uv and texture
    obj = type("M", (), dict(vertices=v, faces=f, corner_uv=uvf.reshape(-1, 3, 2), texture=rgba[..., :3].copy()))()
    assert R.MeshSet({4: obj}, device="cpu", textures=True).texture_table == [(0, 5, 3)]
    assert R.MeshSet({4: obj}, device="cpu").texels is None
    P.write_ply_model(tmp_path / "obj_000005.ply", v, f, texture_uv=uv, texture_file="deep.png")
    with pytest.raises(ValueError, match="16-bit"):
        R.MeshSet({5: tmp_path / "obj_000005.ply"}, device="cpu", textures=True)
    P.write_ply_model(tmp_path / "obj_000006.ply", v, f, texture_uv=uv, texture_file="gone.png")
    with pytest.raises(FileNotFoundError, match=r"gone\.png.*obj_000006\.ply"):
        R.MeshSet({6: tmp_path / "obj_000006.ply"}, device="cpu", textures=True)
    K = np.eye(3)
    with pytest.raises(ValueError, match="uv"):
        R.render(plain, [(1, np.eye(3), np.zeros(3))], K, (8, 8), outputs=("uv",), shading="flat")
    with pytest.raises(ValueError, match="texture_filter"):
        R.render(ms, [(1, np.eye(3), np.zeros(3))], K, (8, 8), shading="flat", texture_filter="cubic")


# ---- the atlas and the mutants ------------------------------------------------------------------------------------------
def test_layout_is_the_restatements_and_refuses_an_atlas_beyond_8192():
    from pegasus_amd import mesh as M
    for F in (1, 2, 3, 5, 80, 81, 25000):
        for s in (4, 5, 16):
            w, h, cols, rows, uv = M.texture_atlas_layout(F, s)
            W, H, C_, R_, _xy, UV = TR.atlas_layout(F, s)
            assert (w, h, cols, rows) == (W, H, C_, R_) and uv.dtype == np.float32 and uv.tobytes() == UV.tobytes(), (F, s)
            assert cols * cols >= (F + 1) // 2 > (cols - 1) * (cols - 1) and rows * cols >= (F + 1) // 2 > (rows - 1) * cols
    assert M.texture_atlas_layout(2 * 512 * 512, 16)[:2] == (8192, 8192)
    with pytest.raises(ValueError, match=r"8192.*largest cell that fits is 15"):
        M.texture_atlas_layout(2 * 512 * 512 + 1, 16)              # 513 columns: 513 * 15 = 7695 <= 8192 < 513 * 16
    with pytest.raises(ValueError, match="at least 4"):
        M.texture_atlas_layout(10, 3)
    with pytest.raises(ValueError, match="at least one face"):
        M.texture_atlas_layout(0, 16)


def inside_points(xy, rng, n_random=12):
    """Points of a triangle with corners xy [3,2]: the corners, the edge midpoints, the centroid and random interior points."""
    w = [np.eye(3)[k] for k in range(3)] + [np.array(p) for p in ((.5, .5, 0), (0, .5, .5), (.5, 0, .5), (1 / 3, 1 / 3, 1 / 3))]
    w += list(rng.dirichlet((1, 1, 1), n_random))
    return np.array(w) @ xy


@pytest.mark.parametrize("cell", [4, 5, 16])
@pytest.mark.parametrize("n_faces", [1, 2, 3, 5, 81])
def test_a_sample_inside_a_faces_triangle_reads_only_that_faces_texels(n_faces, cell):
    width, height, _cols, _rows, xy, _uv = TR.atlas_layout(n_faces, cell)
    owner = TR.atlas_owner(n_faces, cell)[0]
    rng = np.random.default_rng(60)
    bound = width * 2.0 ** -22
    worst = 0.0
    for f in range(n_faces):
        for X, Y in inside_points(xy[f], rng):
            # exact arithmetic (float64 on coordinates that are sums of few binary fractions): texel index coordinates
            x, y = X - 0.5, Y - 0.5
            x0, y0 = np.floor(x), np.floor(y)
            for i, wx in ((x0, 1 - (x - x0)), (x0 + 1, x - x0)):
                for j, wy in ((y0, 1 - (y - y0)), (y0 + 1, y - y0)):
                    if wx * wy > 0:
                        assert 0 <= i < width and 0 <= j < height and owner[int(j), int(i)] == f, ("bilinear", f, X, Y, i, j)
            assert owner[int(np.floor(Y)), int(np.floor(X))] == f, ("nearest", f, X, Y)
            # float32 as the kernel forms it, from the float32 (u, v) of the layout's rule
            u, v = np.float32(X / width), np.float32(1.0 - Y / height)
            for bilinear in (False, True):
                foreign = sum(wgt for i, j, wgt in TR.footprint((0, width, height), u, v, bilinear) if owner[height - 1 - j, i] != f)
                worst = max(worst, foreign)
                assert foreign <= bound, (bilinear, f, X, Y, foreign, bound)
    print(f"F={n_faces} s={cell}: largest foreign weight {worst:.3g}, bound {bound:.3g}")


def test_every_shade_mutant_changes_the_shade_case():
    c = TC.shade_case()
    texels, table = TR.pack_textures(TC.textures())
    run = lambda bilinear, mutant=None: TR.shade_textured_f32(c["jobs"], c["W"], c["H"], c["near"], texels, table, c["n_slots"],
                                                              bilinear=bilinear, mutant=mutant, **c["opts"])
    ref = {b: run(b) for b in (False, True)}
    for m in TR.SHADE_MUTANTS:
        changed = {b: int((~TR.same_bits(run(b, m)["rgb"], ref[b]["rgb"])).sum()) for b in (False, True)}
        print(m, changed)
        only = {"nearest_rounds": False, "bilinear_no_half_texel": True}.get(m)
        assert changed[only if only is not None else False] > 0 and (only is not None or changed[True] > 0), (m, changed)
    # what the case promises: a flipped face, UVs at 0 and 1 exactly, below, above and NaN, an untextured job in between
    uv, hit = ref[False]["uv"], ref[False]["job_id"] >= 0
    u, v = uv[..., 0][hit], uv[..., 1][hit]
    assert (u == 0).any() and (u == 1).any() and (v == 0).any() and (v == 1).any() and (u < 0).any() and (u > 1).any() and (v < 0).any()
    assert (v > 1).any() and np.isnan(u).any() and not np.isnan(ref[True]["rgb"]).any()
    plain = TR.shade_textured_f32(TC.shade_case(textured=False)["jobs"], c["W"], c["H"], c["near"], texels, table, c["n_slots"], **c["opts"])
    own = ref[False]["job_id"] == 2
    assert own.sum() > 50 and (ref[False]["rgb"][own] == plain["rgb"][own]).all() and (ref[False]["rgb"][hit & ~own] != plain["rgb"][hit & ~own]).any()


def test_every_atlas_mutant_changes_an_atlas_case():
    changed = {m: 0 for m in TR.ATLAS_MUTANTS}
    for name, (v, f, cell) in TC.atlas_meshes().items():
        pts, nrm, owner = TR.atlas_points_f32(v, f, cell)
        for m in ("half1_not_mirrored", "antidiagonal_to_half1"):
            p2, _n2, o2 = TR.atlas_points_f32(v, f, cell, mutant=m)
            changed[m] += int((~TR.same_bits(p2, pts)).sum()) + int((o2 != owner).sum())
        colors, seen, face_fill = TC.pack_inputs(owner, len(f))
        tex, face_seen = TR.atlas_pack(len(f), cell, owner, colors, seen, face_fill)
        tex2, _ = TR.atlas_pack(len(f), cell, owner, colors, seen, face_fill, mutant="unseen_mean_truncates")
        changed["unseen_mean_truncates"] += int((tex2 != tex).sum())
        # the restatement's own invariants
        W, H = TR.atlas_layout(len(f), cell)[:2]
        assert pts.shape == (W * H, 3) and tex.shape == (H, W, 3) and face_seen.shape == (len(f),)
        assert (pts[owner < 0] == 0).all() and (nrm[owner < 0] == 0).all()
        assert (tex.reshape(-1, 3)[owner < 0] == 128).all()
        if name.startswith("degenerate"):
            assert set(np.unique(owner)) == {-1, 0, 3}
    print(changed)
    assert all(n > 0 for n in changed.values()), changed


# ---- argument checks ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pegasus_amd import build
    build.build()
    return _lib.lib()


def jobs(n, faces=12):
    arr = (_lib.PgrMeshJob * max(n, 1))()
    for k in range(n):
        arr[k] = _lib.PgrMeshJob(vertex_first=0, vertex_count=8, face_first=0, face_count=faces, R=(C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1),
                                 t=(C.c_float * 3)(0, 0, 4), fx=100.0, fy=100.0, cx=8.0, cy=8.0, slot=0)
    return arr


def textured(lib, n=2, table=((0, 4, 4), (48, 2, 3)), job_texture=(0, 1), texel_bytes=66, filter=0, corner_uv=FAKE, texels=FAKE,
             tex="default", ws=FAKE, ws_bytes=None, keys=FAKE, n_textures=None, null_table=False, null_job_texture=False):
    arr = jobs(n)
    if ws_bytes is None:
        ws_bytes = lib.pgr_mesh_shade_textured_workspace_bytes(n, arr)
    shade = _lib.PgrMeshShade(ambient=0.5, rgb=FAKE)
    rows = (_lib.PgrMeshTexture * max(len(table), 1))(*[_lib.PgrMeshTexture(offset=o, width=w, height=h) for o, w, h in table])
    which = (C.c_int32 * max(n, 1))(*job_texture)
    if tex == "default":
        tex = _lib.PgrMeshTextures(corner_uv=corner_uv, texels=texels, texel_bytes=texel_bytes, n_textures=len(table) if n_textures is None else n_textures,
                                   textures=None if null_table else rows, job_texture=None if null_job_texture else which, filter=filter, uv=None)
    return lib.pgr_mesh_shade_textured(FAKE, 8, FAKE, 1 << 22, n, arr, 16, 16, 0.25, keys, 1, C.byref(shade), None if tex is None else C.byref(tex),
                                       ws, ws_bytes, None)


def test_the_new_symbols_are_declared_bound_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pegasus_raster.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(pgr_[a-z_0-9]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert set(_lib.SYMBOLS) == declared
    assert lib.pgr_abi_version() == 4
    assert "#define PGR_TEXTURE_NEAREST 0" in text and "#define PGR_TEXTURE_BILINEAR 1" in text
    assert (_lib.PGR_TEXTURE_NEAREST, _lib.PGR_TEXTURE_BILINEAR) == (0, 1)
    for struct in (_lib.PgrMeshTexture, _lib.PgrMeshTextures):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct.__name__, struct.__name__), text, flags=re.S).group(1)
        assert re.findall(r"\*?(\w+)\s*[;,]", fields) == [n for n, _ in struct._fields_], struct.__name__


def test_textured_workspace_is_host_only_and_holds_both_tables(lib):
    fn, plain = lib.pgr_mesh_shade_textured_workspace_bytes, lib.pgr_mesh_shade_workspace_bytes
    for n in (1, 2, 32, 33, 1024):
        assert fn(n, jobs(n)) >= plain(n, jobs(n)) + 16 * n
    assert fn(0, jobs(1)) == 0 and fn(-1, jobs(1)) == 0 and fn(1, None) == 0 and fn(1025, jobs(1025)) == 0
    assert fn(1, jobs(1, faces=(1 << 22) + 1)) == 0 and fn(1, jobs(1, faces=-1)) == 0


def test_textured_shade_refuses_bad_arguments_before_any_launch(lib):
    bad = [dict(tex=None), dict(keys=None), dict(n_textures=-1), dict(null_table=True), dict(null_job_texture=True),
           dict(job_texture=(0, 2)), dict(job_texture=(-2, 0)), dict(table=((0, 0, 4), (48, 2, 3))), dict(table=((0, 4, 8193), (48, 2, 3))),
           dict(table=((0, 4, 4), (48, 2, 4))),                      # 48 + 2 * 4 * 3 = 72 > 66
           dict(table=((-1, 4, 4), (48, 2, 3))), dict(texel_bytes=65), dict(texel_bytes=-1), dict(filter=2), dict(filter=-1),
           dict(corner_uv=None), dict(texels=None), dict(ws=C.c_void_p(4100)), dict(keys=C.c_void_p(4100))]
    for kw in bad:
        assert textured(lib, **kw) == _lib.PGR_ERR_INVALID_ARGUMENT, kw
    need = lib.pgr_mesh_shade_textured_workspace_bytes(2, jobs(2))
    assert textured(lib, ws_bytes=need - 1) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert textured(lib, ws=None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert textured(lib, ws_bytes=lib.pgr_mesh_shade_workspace_bytes(2, jobs(2))) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL


def test_atlas_entries_refuse_bad_arguments_before_any_launch(lib):
    fill = (C.c_uint8 * 3)(1, 2, 3)
    points = dict(n_vertices=8, vertices=FAKE, n_faces=5, faces=FAKE, cell=4, width=8, height=8, points=FAKE, normals=FAKE, face_of_texel=FAKE)
    pack = dict(n_faces=5, cell=4, width=8, height=8, face_of_texel=FAKE, colors=FAKE, seen=FAKE, face_fill=None, fill=fill, texture=FAKE,
                face_seen=None)
    for base, name, bads in ((points, "pgr_mesh_atlas_points", [dict(n_vertices=-1), dict(vertices=None), dict(faces=None), dict(points=None),
                                                               dict(normals=None), dict(face_of_texel=None)]),
                             (pack, "pgr_mesh_atlas_pack", [dict(face_of_texel=None), dict(colors=None), dict(seen=None), dict(fill=None),
                                                           dict(texture=None)])):
        common = [dict(n_faces=0), dict(n_faces=-3), dict(cell=3), dict(width=12), dict(height=4), dict(width=8, height=8, n_faces=9),
                  dict(n_faces=2 * 512 * 512 + 1, cell=16, width=8208, height=8192), dict(cell=8193, width=8193, height=8193, n_faces=1)]
        for kw in bads + common:
            assert getattr(lib, name)(*dict(base, **kw).values(), None) == _lib.PGR_ERR_INVALID_ARGUMENT, (name, kw)
