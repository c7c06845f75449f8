"""ply_io.read_ply_model / write_ply_model (BOP object model files), MeshSet's use of them and mesh_render.vertex_normals.
No GPU."""
from pathlib import Path

import numpy as np
import pytest

import mesh_raster_cases as MC
from pegasus_amd import ply_io as P

GOLDEN = Path(__file__).resolve().parent / "golden"


def small_model(seed=0):
    rng = np.random.default_rng(seed)
    v, f = MC.icosphere(0, 2.0)
    return v, f, rng.normal(size=v.shape).astype(np.float32), rng.integers(0, 256, v.shape).astype(np.uint8)


@pytest.mark.parametrize("ascii", [False, True], ids=["binary", "ascii"])
@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("colors", [None, "uint8", "float"])
def test_round_trip(tmp_path, ascii, with_normals, colors):
    v, f, n, c = small_model()
    cc = None if colors is None else (c if colors == "uint8" else (c / 255.0).astype(np.float32))
    P.write_ply_model(tmp_path / "m.ply", v, f, normals=n if with_normals else None, colors=cc, ascii=ascii)
    m = P.read_ply_model(tmp_path / "m.ply")
    assert set(m) == {"pts", "faces"} | ({"normals"} if with_normals else set()) | ({"colors"} if colors else set())
    assert m["pts"].dtype == np.float64 and (m["pts"].astype(np.float32) == v).all() and (m["faces"] == f).all()
    if with_normals:
        assert (m["normals"].astype(np.float32) == n).all()
    if colors:
        assert m["colors"].dtype == cc.dtype and (m["colors"] == cc).all()          # colours come back as stored
    header = (tmp_path / "m.ply").read_bytes().split(b"end_header")[0].decode().split("\n")
    props = [l.split()[-1] for l in header if l.startswith("property")]
    want = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + (["red", "green", "blue"] if colors else []) + ["vertex_indices"]
    assert props == want                                                          # the toolkit's save_ply order


def test_a_file_of_write_ply_mesh_reads_equal_to_read_ply_mesh(tmp_path):
    v, f, _n, _c = small_model(1)
    P.write_ply_mesh(tmp_path / "a.ply", v, f)
    m = P.read_ply_model(tmp_path / "a.ply")
    v2, f2 = P.read_ply_mesh(tmp_path / "a.ply")
    assert set(m) == {"pts", "faces"}
    assert (m["pts"].astype(np.float32).tobytes(), m["faces"].astype(np.int32).tobytes()) == (v2.tobytes(), f2.tobytes())
    P.write_ply_mesh(tmp_path / "empty.ply", np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    m = P.read_ply_model(tmp_path / "empty.ply")
    assert m["pts"].shape == (0, 3) and m["faces"].shape == (0, 3)


def test_the_toolkits_own_file_reads_equal():
    """tests/golden/bop_model.ply was written by the toolkit's inout.save_ply2, run once with ``imageio`` and ``png`` stubbed
    (tests/golden/make_golden_ply_model.py); bop_model.npz holds the arrays it was handed.  ASCII, normals, uint8 colours
    and texture_u / texture_v, which is skipped."""
    m = P.read_ply_model(GOLDEN / "bop_model.ply")
    g = np.load(GOLDEN / "bop_model.npz")
    assert set(m) == {"pts", "faces", "normals", "colors"}
    assert len(m["pts"]) == 42 and len(m["faces"]) == 80
    for k in ("pts", "normals", "colors", "faces"):
        np.testing.assert_array_equal(m[k], g[k], err_msg=k)
    assert m["colors"].dtype == np.uint8 and m["colors"].max() > 1


HEADER = "ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face {n}\n" \
         "property list uchar int vertex_indices\nend_header\n"
VERTS = "0 0 0\n1 0 0\n1 1 0\n0 1 0\n"


def test_any_scalar_properties_in_any_order_and_both_index_names(tmp_path):
    text = ("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty uchar blue\nproperty double z\nproperty float quality\n"
            "property float y\nproperty uchar red\nproperty short flags\nproperty float x\nproperty uchar green\nproperty float texture_u\n"
            "element face 1\nproperty list uint8 uint32 vertex_index\nend_header\n"
            "3 0.5 9 0.25 1 -4 0.125 2 0.75\n30 1.5 9 1.25 10 -4 1.125 20 0.75\n33 2.5 9 2.25 11 -4 2.125 22 0.75\n3 2 0 1\n")
    (tmp_path / "h.ply").write_text(text)
    m = P.read_ply_model(tmp_path / "h.ply")
    np.testing.assert_array_equal(m["pts"], [[0.125, 0.25, 0.5], [1.125, 1.25, 1.5], [2.125, 2.25, 2.5]])
    np.testing.assert_array_equal(m["colors"], [[1, 2, 3], [10, 20, 30], [11, 22, 33]])
    np.testing.assert_array_equal(m["faces"], [[2, 0, 1]])
    assert "normals" not in m
    # the same in binary, CRLF-free header, uint indices
    dt = np.dtype([("blue", "u1"), ("z", "<f8"), ("quality", "<f4"), ("y", "<f4"), ("red", "u1"), ("flags", "<i2"), ("x", "<f4"), ("green", "u1"),
                   ("texture_u", "<f4")])
    rows = np.zeros(3, dt)
    for k, name in enumerate("xyz"):
        rows[name] = m["pts"][:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rows[name] = m["colors"][:, k]
    face = np.zeros(1, np.dtype([("n", "u1"), ("idx", "<u4", (3,))]))
    face["n"], face["idx"] = 3, [[2, 0, 1]]
    head = text.split("end_header\n")[0].replace("format ascii", "format binary_little_endian") + "end_header\n"
    (tmp_path / "b.ply").write_bytes(head.encode() + rows.tobytes() + face.tobytes())
    b = P.read_ply_model(tmp_path / "b.ply")
    for k in ("pts", "colors", "faces"):
        np.testing.assert_array_equal(b[k], m[k])


def test_quads_truncated_files_and_bad_indices_raise(tmp_path):
    cases = {
        "quad": HEADER.format(n=1) + VERTS + "4 0 1 2 3\n",
        "truncated vertices": HEADER.format(n=1) + "0 0 0\n1 0 0\n",
        "truncated faces": HEADER.format(n=2) + VERTS + "3 0 1 2\n",
        "index out of range": HEADER.format(n=1) + VERTS + "3 0 1 4\n",
        "negative index": HEADER.format(n=1) + VERTS + "3 0 1 -1\n",
        "no header end": "ply\nformat ascii 1.0\nelement vertex 1\n",
        "big endian": HEADER.format(n=0).replace("ascii", "binary_big_endian") + VERTS,
    }
    for name, text in cases.items():
        (tmp_path / "bad.ply").write_text(text)
        with pytest.raises(ValueError):
            P.read_ply_model(tmp_path / "bad.ply")
            pytest.fail(name)
    v, f, n, c = small_model(2)
    P.write_ply_model(tmp_path / "ok.ply", v, f, normals=n, colors=c)
    data = (tmp_path / "ok.ply").read_bytes()
    for cut in (len(data) - 1, len(data) - 13 * len(f) + 5, len(data) - 13 * len(f) - 3):
        (tmp_path / "cut.ply").write_bytes(data[:cut])
        with pytest.raises(ValueError, match="ends inside"):
            P.read_ply_model(tmp_path / "cut.ply")
    quad = np.zeros(1, np.dtype([("n", "u1"), ("idx", "<i4", (4,))]))
    quad["n"] = 4
    head = data.split(b"element face")[0] + b"element face 1\nproperty list uchar int vertex_indices\nend_header\n"
    body = data[data.index(b"end_header\n") + 11:len(data) - 13 * len(f)]
    (tmp_path / "quad.ply").write_bytes(head + body + quad.tobytes())
    with pytest.raises(ValueError, match="triangles"):
        P.read_ply_model(tmp_path / "quad.ply")


def icosphere64(subdivisions):
    """MC.icosphere's construction kept in float64 (MC rounds its vertices to float32, which breaks the symmetry at 1e-8)."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v32, f = MC.icosphere(0)
    v = [np.asarray(p, np.float64) / np.sqrt(1.0 + g * g) for p in ((-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g),
                                                                    (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1))]
    assert np.allclose(np.asarray(v), v32, atol=1e-7)
    f = [tuple(int(x) for x in t) for t in f]
    for _ in range(subdivisions):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v), np.asarray(f, np.int32)


@pytest.mark.parametrize("subdivisions", [0, 1])
def test_vertex_normals_of_an_icosphere_are_radial(subdivisions):
    """Every vertex of the icosahedron, and of its first subdivision, lies on a rotation axis of the whole mesh (five-fold, or
    two-fold through an edge's midpoint), so the sum of the unit normals of its faces lies on that axis: the normal is the
    vertex's own direction up to float64 rounding (a few dozen operations of 2^-53 on numbers of size 1)."""
    from pegasus_amd.mesh_render import vertex_normals
    v, f = icosphere64(subdivisions)
    assert np.array_equal(f, MC.icosphere(subdivisions)[1])
    n = vertex_normals(v, f)
    assert n.dtype == np.float64
    np.testing.assert_allclose(n, v / np.linalg.norm(v, axis=1, keepdims=True), rtol=0, atol=64 * 2.0 ** -53)
    # a face wound the other way turns its share around; a vertex of no face gets 0
    n2 = vertex_normals(np.vstack([v, [[9.0, 9.0, 9.0]]]), f[:, ::-1])
    np.testing.assert_allclose(n2[:-1], -n, rtol=0, atol=64 * 2.0 ** -53)
    assert (n2[-1] == 0).all()


def test_mesh_set_loads_models_through_the_new_reader(tmp_path):
    from pegasus_amd import mesh_render as R
    v, f, n, c = small_model(3)
    v2, f2 = MC.box((1.0, 2.0, 3.0))
    P.write_ply_mesh(tmp_path / "obj_000001.ply", v, f)                        # the layout the project writes itself
    P.write_ply_model(tmp_path / "obj_000002.ply", v2, f2)
    ms = R.MeshSet.from_dir(tmp_path, device="cpu")
    old = R.MeshSet({1: type("M", (), dict(vertices=v, faces=f))(), 2: type("M", (), dict(vertices=v2, faces=f2))()}, device="cpu")
    assert ms.ranges == old.ranges == {1: (0, len(v), 0, len(f)), 2: (len(v), len(v2), len(f), len(f2))}
    assert ms.vertices.numpy().tobytes() == old.vertices.numpy().tobytes() == np.concatenate([v, v2]).tobytes()
    assert ms.faces.numpy().tobytes() == old.faces.numpy().tobytes() == np.concatenate([f, f2]).tobytes()
    assert ms.normals is None and ms.colors is None
    # only object 1 has colours (uint8: divided by 255) and normals: object 2 gets 0.5 and vertex_normals
    P.write_ply_model(tmp_path / "obj_000001.ply", v, f, normals=n, colors=c)
    ms = R.MeshSet.from_dir(tmp_path, device="cpu", scale=0.001)
    assert ms.vertices.numpy().tobytes() == (np.concatenate([v, v2]).astype(np.float64) * 0.001).astype(np.float32).tobytes()
    np.testing.assert_array_equal(ms.colors.numpy(), np.concatenate([(c / 255.0).astype(np.float32), np.full((8, 3), 0.5, np.float32)]))
    np.testing.assert_array_equal(ms.normals.numpy(), np.concatenate([n, R.vertex_normals(v2, f2).astype(np.float32)]))
    floats = R.MeshSet({5: type("M", (), dict(vertices=v, faces=f, colors=(c / 255.0).astype(np.float32)))()}, device="cpu", compute_normals=True)
    np.testing.assert_array_equal(floats.colors.numpy(), (c / 255.0).astype(np.float32))
    np.testing.assert_array_equal(floats.normals.numpy(), R.vertex_normals(v, f).astype(np.float32))
    P.write_ply_model(tmp_path / "obj_000003.ply", v, np.array([[0, 1, 12]]))
    with pytest.raises(ValueError, match="outside"):
        R.MeshSet.from_dir(tmp_path, device="cpu")
