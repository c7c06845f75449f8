"""Vertex clustering on the device (pgr_mesh_cluster_count / pgr_mesh_cluster_emit, pegasus_amd.decimate) against the NumPy
float64 reference of tests/decimate_reference.py.  DESIGN.md section 19 holds the rule and the tolerances:

  * cluster_of_vertex, K, F' and the faces are EQUAL;
  * two runs are equal as bytes, with guard regions around every output and around the workspace;
  * an average position differs by at most m 2^-52 voxel per axis for a cluster of m vertices;
  * a quadric position differs by at most the reference's derived per-cluster bound tol_k
    (decimate_reference.quadric_tolerance), clusters whose accept / reject decision lies within that error are compared on
    neither branch, and at most 1 % of a case's clusters may be such.

Worst err / tol observed on an MI355X: 0 in every case -- the kernel sums in the rule's own fixed order (64 partials and a fold),
so its positions came out equal to the reference's bit for bit; the bounds are what another summation order would have to meet.
"""
import ctypes as C
import json
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import decimate_cases as DC
from decimate_reference import cluster_reference, quadric_tolerance

pytestmark = pytest.mark.gpu

GUARD = 4096                 # bytes on either side of every buffer
FILL = 0xA5
_references = {}


def reference(name, build, contraction):
    """The case and its reference, computed once per session and never changed."""
    key = (name, contraction)
    if key not in _references:
        v, f, voxel = build()
        _references[key] = (v, f, voxel, cluster_reference(v, f, voxel, contraction))
    return _references[key]


class Guarded:
    """``nbytes`` of device memory with GUARD bytes of FILL on either side (the payload 256-byte aligned)."""

    def __init__(self, nbytes, device):
        import torch
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + 2 * GUARD + 256,), FILL, dtype=torch.uint8, device=device)
        self.off = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256
        self.view = self.raw[self.off:self.off + self.nbytes]

    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + self.off)

    def intact(self):
        return bool((self.raw[:self.off] == FILL).all()) and bool((self.raw[self.off + self.nbytes:] == FILL).all())

    def numpy(self, dtype, shape):
        return self.view.cpu().numpy().view(dtype).reshape(shape).copy()


def run_entries(device, v, f, voxel, contraction):
    """Both entries called directly, every buffer guarded.  Returns (K, F', vertices, faces, cluster_of_vertex, used) as host
    arrays; asserts that no guard byte changed."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    nv, nf = len(v), len(f)
    dv = torch.as_tensor(np.ascontiguousarray(v, np.float32), device=device)
    df = torch.as_tensor(np.ascontiguousarray(f, np.int32).reshape(-1, 3), device=device)
    lo = v.astype(np.float64).min(axis=0) - voxel / 2.0
    grid = (float(voxel), float(lo[0]), float(lo[1]), float(lo[2]))
    ws = Guarded(L.pgr_mesh_cluster_workspace_bytes(nv, nf), device)
    counts = Guarded(16, device)
    stream = _lib.stream_ptr(device)
    fp = _lib.ptr(df) if nf else None
    assert L.pgr_mesh_cluster_count(nv, _lib.ptr(dv), nf, fp, *grid, ws.ptr(), ws.nbytes, counts.ptr(), stream) == _lib.PGR_OK
    k, nfo = (int(x) for x in counts.numpy(np.int64, (2,)))
    assert 0 < k <= nv and 0 <= nfo <= nf
    out_v, out_f = Guarded(24 * k, device), Guarded(12 * nfo, device)
    cov, used = Guarded(4 * nv, device), Guarded(k, device)
    code = {"average": 0, "quadric": 1}[contraction]
    assert L.pgr_mesh_cluster_emit(nv, _lib.ptr(dv), nf, fp, *grid, code, ws.ptr(), ws.nbytes, k, nfo, out_v.ptr(),
                                   out_f.ptr() if nfo else None, cov.ptr(), used.ptr(), stream) == _lib.PGR_OK
    torch.cuda.synchronize(device)
    for name, g in dict(workspace=ws, counts=counts, vertices=out_v, faces=out_f, cluster_of_vertex=cov, used=used).items():
        assert g.intact(), f"{name}: a guard byte changed"
    return (k, nfo, out_v.numpy(np.float64, (k, 3)), out_f.numpy(np.int32, (nfo, 3)), cov.numpy(np.int32, (nv,)),
            used.numpy(np.uint8, (k,)))


def compare(got, ref, voxel, contraction, name):
    """The comparison of the module docstring; returns the worst err / tol over the compared quadric clusters."""
    k, nfo, gv, gf, gcov, gused = got
    assert k == len(ref.vertices) and nfo == len(ref.faces), name
    assert np.array_equal(gcov, ref.cluster_of_vertex), name
    assert np.array_equal(gf, ref.faces), name
    avg_tol = ref.members.astype(np.float64)[:, None] * 2.0 ** -52 * voxel
    if contraction == "average":
        assert not gused.any(), name
        err = np.abs(gv - ref.vertices)
        print(f"{name}: average, worst err / tol {float((err / avg_tol).max()):.3g}")
        assert (err <= avg_tol).all(), name
        return 0.0
    tol, masked = quadric_tolerance(ref, voxel)
    print(f"{name}: {int(masked.sum())} of {k} clusters masked")
    assert masked.sum() <= 0.01 * k, name
    keep = ~masked
    assert np.array_equal(gused[keep], ref.used_quadric[keep]), name
    on_avg = keep & (ref.used_quadric == 0)
    assert (np.abs(gv - ref.vertices)[on_avg] <= avg_tol[on_avg]).all(), name
    on_quad = keep & (ref.used_quadric == 1)
    worst = 0.0
    if on_quad.any():
        err = np.abs(gv - ref.vertices)[on_quad].max(axis=1)
        worst = float((err / tol[on_quad]).max())
        print(f"{name}: quadric on {int(on_quad.sum())} clusters, worst err / tol {worst:.3g}")
        assert (err <= tol[on_quad]).all(), name
    return worst


def check(gpu_device, name, build, contraction):
    v, f, voxel, ref = reference(name, build, contraction)
    a = run_entries(gpu_device, v, f, voxel, contraction)
    b = run_entries(gpu_device, v, f, voxel, contraction)
    for x, y in zip(a, b):                                  # bytes, vertices included (NaN would compare unequal: none expected)
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), name
    compare(a, ref, voxel, contraction, name)
    return a, ref


# ---- hand-worked and shape cases --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DC.HAND_CASES))
@pytest.mark.parametrize("contraction", ["average", "quadric"])
def test_hand_worked_cases(gpu_device, name, contraction):
    check(gpu_device, name, DC.HAND_CASES[name], contraction)


@pytest.mark.parametrize("name", sorted(DC.SHAPE_CASES))
@pytest.mark.parametrize("contraction", ["average", "quadric"])
def test_smallest_shapes_that_can_go_wrong(gpu_device, name, contraction):
    got, ref = check(gpu_device, name, DC.SHAPE_CASES[name], contraction)
    if name == "one_cluster":
        assert got[0] == 1 and got[1] == 0
    if name == "own_cells":
        assert got[0] == len(ref.cluster_of_vertex)
    if name == "dense_cell":
        assert ref.members.max() > 1024 and (contraction == "average" or ref.terms.max() > 1024)
    if name == "thin_slab":                                  # duplicates went, opposites stayed
        faces = {tuple(t) for t in got[3].tolist()}
        assert len(faces) == got[1] and any((a, c, b) in faces for a, b, c in faces)
    if name == "wide_extent":
        assert ref.cells[:, 0].max() == (1 << 20) - 2


@pytest.mark.parametrize("name", sorted(DC.AVERAGE_ONLY))
def test_vertices_exactly_on_cell_walls(gpu_device, name):
    check(gpu_device, name, DC.AVERAGE_ONLY[name], "average")


def test_more_than_2_to_the_21_clusters_take_the_two_stage_face_sort(gpu_device):
    got, ref = check(gpu_device, "big_lattice", DC.big_lattice, "average")
    assert got[0] == len(ref.cluster_of_vertex) > DC.PACKED_LIMIT and got[1] == 992


# ---- the surfaces of the quadric comparison ------------------------------------------------------------------------------
@pytest.mark.parametrize("cells_across", [8, 16, 32])
@pytest.mark.parametrize("surface", ["icosphere", "gyroid"])
def test_quadric_positions_within_the_derived_bound(gpu_device, surface, cells_across):
    def build():
        key = ("surface", surface)
        if key not in _references:
            _references[key] = DC.icosphere() if surface == "icosphere" else DC.gyroid_mesh()
        v, f = _references[key]
        return v, f, DC.voxel_for(v, cells_across)
    check(gpu_device, f"{surface}_{cells_across}", build, "quadric")


# ---- the Python layer -----------------------------------------------------------------------------------------------------
def test_cluster_vertices_returns_device_tensors_and_checks_the_contract(gpu_device):
    import torch
    from pegasus_amd import decimate as D
    v, f, voxel, ref = reference("beyond_a_tile", DC.SHAPE_CASES["beyond_a_tile"], "quadric")
    dv, df = torch.as_tensor(v, device=gpu_device), torch.as_tensor(f, device=gpu_device)
    out_v, out_f, cov, used = D.cluster_vertices(dv, df, voxel)
    assert out_v.dtype == torch.float64 and out_f.dtype == torch.int32 and cov.dtype == torch.int32 and used.dtype == torch.uint8
    assert all(t.device == dv.device for t in (out_v, out_f, cov, used))
    compare((len(out_v), len(out_f), out_v.cpu().numpy(), out_f.cpu().numpy(), cov.cpu().numpy(), used.cpu().numpy()), ref, voxel,
            "quadric", "cluster_vertices")
    bad = df.clone()
    bad[7, 1] = len(v)
    with pytest.raises(ValueError, match=r"\[0, V\)"):
        D.cluster_vertices(dv, bad, voxel)
    bad[7, 1] = -1
    with pytest.raises(ValueError, match=r"\[0, V\)"):
        D.cluster_vertices(dv, bad, voxel)
    with pytest.raises(ValueError, match="2\\^20"):
        D.cluster_vertices(dv, df, 1e-7)
    with pytest.raises(ValueError, match="positive"):
        D.cluster_vertices(dv, df, 0.0)
    nan = dv.clone()
    nan[3, 0] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        D.cluster_vertices(nan, df, voxel)


def test_simplify_to_meets_its_target_and_equals_clustering_at_its_voxel(gpu_device):
    from pegasus_amd import decimate as D
    from pegasus_amd.mesh import Mesh
    v, f = DC.icosphere()
    mesh = Mesh(v, f)
    for target in (512, 40, 0):
        small, voxel = D.simplify_to(mesh, target)
        assert len(small.faces) <= target and small.vertices.dtype == np.float32
        again = D.simplify_vertex_clustering(mesh, voxel)
        assert small.vertices.tobytes() == again.vertices.tobytes() and np.array_equal(small.faces, again.faces)
    small, voxel = D.simplify_to(mesh, 512)
    assert len(small.faces) > 256                            # the bisection came close: no coarser than twice the target
    ref = cluster_reference(v, f, voxel)
    assert np.array_equal(small.faces, ref.faces) and np.array_equal(small.vertices, ref.vertices.astype(np.float32))


def write_models(models, scale=1000.0):
    from pegasus_amd.mesh import Mesh, models_info, write_ply
    from mesh_raster_cases import icosphere
    info = {}
    for obj_id, (sub, radius) in {1: (4, 0.05), 4: (3, 0.08)}.items():
        v, f = icosphere(sub, radius)
        v = v * np.asarray([1.0, 0.6 + 0.1 * obj_id, 1.3], np.float32)
        write_ply(models / f"obj_{obj_id:06d}.ply", Mesh(v, f), scale=scale)
        info[str(obj_id)] = models_info(Mesh(v, f).scaled(scale))
    info["4"]["symmetries_continuous"] = [{"axis": [0.0, 0.0, 1.0], "offset": [0.0, 0.0, 0.0]}]
    info["1"]["symmetries_discrete"] = [[-1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]]
    (models / "models_info.json").write_text(json.dumps(info, indent=2) + "\n")
    return info


@pytest.mark.parametrize("through_cli", [False, True])
def test_write_models_eval(gpu_device, tmp_path, through_cli):
    from pegasus_amd import decimate as D
    from pegasus_amd.ply_io import read_ply_mesh
    from pegasus_amd.pose_error import PoseErrorModels
    models = tmp_path / "models"
    models.mkdir()
    src = write_models(models)
    if through_cli:
        out = tmp_path / "elsewhere"
        assert D.main(["--models", str(models), "--out", str(out), "--faces", "300", "--contraction", "average"]) == 0
        limit = {1: 300, 4: 300}
    else:
        out = tmp_path / "models_eval"
        report = D.write_models_eval(models, ratio=0.1)
        assert set(report) == {1, 4}
        limit = {1: 512, 4: 128}                             # a tenth of 5120 and of 1280 faces
    info = json.loads((out / "models_info.json").read_text())
    assert set(info) == {"1", "4"}
    for obj_id in (1, 4):
        v, f = read_ply_mesh(out / f"obj_{obj_id:06d}.ply")
        assert 0 < len(f) <= limit[obj_id] and f.max() < len(v)
        e, s = info[str(obj_id)], src[str(obj_id)]
        ext = v.max(axis=0).astype(np.float64) - v.min(axis=0)
        np.testing.assert_allclose([e[f"size_{a}"] for a in "xyz"], ext, rtol=1e-6)        # recomputed on the decimated mesh
        assert e["diameter"] != s["diameter"] and abs(e["diameter"] / s["diameter"] - 1.0) < 0.3
        assert {k: x for k, x in e.items() if k.startswith("symmetries")} == {k: x for k, x in s.items() if k.startswith("symmetries")}
    loaded = PoseErrorModels.from_dir(out)
    assert sorted(loaded.diameters) == [1, 4]
    assert len(loaded.symmetries(1)[0]) == 2 and len(loaded.symmetries(4)[0]) > 100


def test_mesh_cli_collision_faces(gpu_device, tmp_path, monkeypatch):
    """Without --collision_faces every file is byte for byte what the parent's call sequence writes; with it the URDF's
    collision mesh is the new, coarser file and everything else is unchanged."""
    from pegasus_amd import mesh as M
    from mesh_raster_cases import icosphere
    v, f = icosphere(4, 0.07)
    mesh = M.Mesh(v * np.asarray([1.0, 0.5, 1.4], np.float32), f)
    monkeypatch.setattr(M, "load_model", lambda *a, **k: None)
    monkeypatch.setattr(M, "extract_mesh", lambda *a, **k: mesh)
    args = ["-m", "unused", "--obj_id", "7", "--mass", "0.3"]
    plain, coarse, expect = tmp_path / "plain", tmp_path / "coarse", tmp_path / "expect"
    assert M.main(args + ["--out", str(plain)]) == 0
    assert M.main(args + ["--out", str(coarse), "--collision_faces", "200"]) == 0
    # the parent's sequence, from the functions as they were
    M.write_ply(expect / "models" / "obj_000007.ply", mesh, scale=1000.0)
    M.write_obj(expect / "urdf" / "obj_000007.obj", mesh)
    M.write_urdf(expect / "urdf" / "obj_000007.urdf", "obj_000007.obj", mesh, 0.3)
    for rel in ("models/obj_000007.ply", "urdf/obj_000007.obj", "urdf/obj_000007.urdf"):
        assert (plain / rel).read_bytes() == (expect / rel).read_bytes(), rel
    assert sorted(p.name for p in (plain / "urdf").iterdir()) == ["obj_000007.obj", "obj_000007.urdf"]
    for rel in ("models/obj_000007.ply", "models/models_info.json", "urdf/obj_000007.obj"):
        assert (plain / rel).read_bytes() == (coarse / rel).read_bytes(), rel
    a, c = ET.parse(plain / "urdf" / "obj_000007.urdf").getroot(), ET.parse(coarse / "urdf" / "obj_000007.urdf").getroot()
    assert c.find("link/collision/geometry/mesh").get("filename") == "obj_000007_collision.obj"
    assert c.find("link/visual/geometry/mesh").get("filename") == "obj_000007.obj"
    assert ET.tostring(a.find("link/inertial")) == ET.tostring(c.find("link/inertial"))
    lines = (coarse / "urdf" / "obj_000007_collision.obj").read_text().splitlines()
    assert 0 < sum(l.startswith("f ") for l in lines) <= 200 < len(mesh.faces)
