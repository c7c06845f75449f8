"""Mesh extraction without a device: the tetrahedron case table, the reference marcher on analytic fields, the mass
properties, the file writers and the C ABI's argument checks (pegasus_amd/mesh.py, tests/mesh_reference.py)."""
import ctypes as C
import itertools
import json
import math
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import mesh_cases as MC
import mesh_reference as R
from mesh_reference import assert_watertight, components
from pegasus_amd import _lib
from pegasus_amd.mesh import Grid, Mesh, models_info, write_obj, write_ply, write_urdf
from pegasus_amd.ply_io import read_ply_mesh


def corner_xyz(code):
    return np.array([(code >> a) & 1 for a in range(3)], np.float64)


def test_case_table_separates_inside_from_outside_with_outward_normals():
    T = R.tet_table()
    for t in range(6):
        P = np.stack([corner_xyz(c) for c in T["corner"][t]])
        assert abs(np.linalg.det(P[1:] - P[0])) == 1.0                           # a Kuhn tetrahedron, volume 1/6
        for c in range(16):
            ins = [q for q in range(4) if (c >> q) & 1]
            n_in = len(ins)
            assert T["ntri"][t, c] == (0 if n_in in (0, 4) else (2 if n_in == 2 else 1))
            # a linear field: -1 at inside vertices, +1 at outside ones; vertices at its zero crossings
            f = np.array([-1.0 if (c >> q) & 1 else 1.0 for q in range(4)])
            pts = {}
            for e, (u, w) in enumerate(R.TET_EDGES):
                if (f[u] < 0) != (f[w] < 0):
                    pts[e] = P[u] + f[u] / (f[u] - f[w]) * (P[w] - P[u])
            tri_edges = T["tri"][t, c, :3 * T["ntri"][t, c]]
            assert set(int(e) for e in tri_edges) == set(pts)                        # every crossed edge used, no other
            inside_c = P[ins].mean(axis=0) if ins else None
            for k in range(T["ntri"][t, c]):
                a, b, d = (pts[int(e)] for e in tri_edges[3 * k:3 * k + 3])
                nrm = np.cross(b - a, d - a)
                assert np.linalg.norm(nrm) > 1e-9
                # the triangle's plane separates: inside vertices on the back side, outside vertices in front
                side = (P - a) @ nrm
                assert all((side[q] < 0) == bool((c >> q) & 1) for q in range(4) if abs(side[q]) > 1e-9)
                assert (inside_c - a) @ nrm < 0
            # the owner of every edge is its lower corner, and the slot is the direction to the other end
            for e, (u, w) in enumerate(R.TET_EDGES):
                assert T["owner"][t, e] == T["corner"][t, u]
                assert R.EDGE_CODES[T["slot"][t, e]] == T["corner"][t, w] ^ T["corner"][t, u]


def sphere_sdf(n, r, center=(0.0, 0.0, 0.0), half=1.0):
    g = Grid(n, n, n, (-half, -half, -half), 2.0 * half / (n - 1))
    i, j, k, o, vox = R._axes(g)
    x, y, z = (R._coord(o[a], vox, idx) - np.float32(center[a]) for a, idx in enumerate((i, j, k)))
    return (np.sqrt(x * x + y * y + z * z) - np.float32(r)).astype(np.float32).reshape(g.shape), g


def test_reference_sphere_is_closed_genus_zero_and_has_the_volume():
    r = 0.7
    sdf, g = sphere_sdf(48, r)
    v, f = R.march_reference(sdf, g)
    n_edges = assert_watertight(f)
    assert len(v) - n_edges + len(f) == 2
    assert len(np.unique(f)) == len(v)                                           # every vertex is used
    m = Mesh(v, f)
    assert abs(m.volume() / (4.0 / 3.0 * math.pi * r ** 3) - 1.0) < 0.01
    assert np.abs(m.center_of_mass()).max() < 1e-3
    rad = np.linalg.norm(v.astype(np.float64), axis=1)
    assert np.abs(rad - r).max() < g.voxel


def test_sphere_through_the_grid_border_still_closes():
    sdf, g = sphere_sdf(32, 0.8, center=(0.6, 0.0, 0.0))
    sdf = sdf.copy()
    sdf[:, :, 0] = sdf[:, :, -1] = sdf[:, 0, :] = sdf[:, -1, :] = sdf[0] = sdf[-1] = 1.0       # the forced outer layer
    v, f = R.march_reference(sdf, g)
    n_edges = assert_watertight(f)
    assert len(v) - n_edges + len(f) == 2
    assert Mesh(v, f).volume() > 0


def unit_cube():
    v = np.array(list(itertools.product((0.0, 1.0), repeat=3)), np.float32)[:, ::-1].copy()     # index = x + 2y + 4z
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # outward
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return Mesh(v, f)


def test_mass_properties_of_the_unit_cube():
    m = unit_cube()
    assert_watertight(m.faces)
    assert m.volume() == pytest.approx(1.0)
    np.testing.assert_allclose(m.center_of_mass(), [0.5, 0.5, 0.5], atol=1e-12)
    np.testing.assert_allclose(m.inertia(3.0), np.eye(3) * 3.0 / 6.0, atol=1e-12)        # m (a^2 + a^2) / 12
    shifted = Mesh(m.vertices * np.float32(2.0) + np.float32(5.0), m.faces)              # side 2, volume 8
    assert shifted.volume() == pytest.approx(8.0)
    np.testing.assert_allclose(shifted.inertia(1.0), np.eye(3) * 8.0 / 12.0, atol=1e-9)
    info = models_info(m)
    assert info["diameter"] == pytest.approx(math.sqrt(3.0))
    assert [info[f"min_{a}"] for a in "xyz"] == [0.0, 0.0, 0.0] and [info[f"size_{a}"] for a in "xyz"] == [1.0, 1.0, 1.0]


def test_file_round_trips(tmp_path):
    m = unit_cube()
    write_ply(tmp_path / "c.ply", m, scale=1000.0)
    v, f = read_ply_mesh(tmp_path / "c.ply")
    np.testing.assert_array_equal(v, m.vertices * np.float32(1000.0))
    np.testing.assert_array_equal(f, m.faces)
    write_obj(tmp_path / "c.obj", m)
    lines = (tmp_path / "c.obj").read_text().splitlines()
    ov = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")])
    of = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith("f ")])
    np.testing.assert_array_equal(ov, m.vertices)
    np.testing.assert_array_equal(of - 1, m.faces)
    write_urdf(tmp_path / "c.urdf", "c.obj", m, 2.0)
    root = ET.parse(tmp_path / "c.urdf").getroot()
    assert float(root.find("link/inertial/mass").get("value")) == 2.0
    I = root.find("link/inertial/inertia")
    assert float(I.get("ixx")) == pytest.approx(2.0 / 6.0) and abs(float(I.get("ixy"))) < 1e-9
    assert [float(x) for x in root.find("link/inertial/origin").get("xyz").split()] == pytest.approx([0.5] * 3)
    assert [e.get("filename") for e in root.iter("mesh")] == ["c.obj", "c.obj"]
    json.dumps(models_info(m))                                                   # plain floats


def test_grid_around_a_box():
    g = Grid.around((0.0, 0.0, 0.0), (1.0, 0.5, 0.25), 101)
    assert (g.nx, g.ny, g.nz) == (101, 51, 26) and g.voxel == pytest.approx(0.01)
    assert g.origin[2] + 0.5 * g.voxel * (g.nz - 1) == pytest.approx(0.125)


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    fake = C.c_void_p(0x1000)
    good = _lib.PgrGrid(nx=8, ny=9, nz=10, origin=(C.c_float * 3)(0, 0, 0), voxel=0.1)
    assert L.pgr_march_workspace_bytes(8, 9, 10) >= 8 * 9 * 10 * 6
    assert L.pgr_march_workspace_bytes(512, 512, 512) > L.pgr_march_workspace_bytes(256, 256, 256) * 7
    for bad in ((1, 9, 10), (8, 0, 10), (8, 9, 1025), (-4, 9, 10)):
        assert L.pgr_march_workspace_bytes(*bad) == 0
    bad_grids = [_lib.PgrGrid(nx=1, ny=9, nz=10, voxel=0.1), _lib.PgrGrid(nx=8, ny=9, nz=2000, voxel=0.1),
                 _lib.PgrGrid(nx=8, ny=9, nz=10, voxel=0.0), _lib.PgrGrid(nx=8, ny=9, nz=10, voxel=float("nan"))]
    cam = _lib.PgrCamera(image_width=33, image_height=21, tanfovx=0.5, tanfovy=0.4, viewmatrix=fake)
    cams = (_lib.PgrCamera * 3)(cam, cam, cam)
    INV = _lib.PGR_ERR_INVALID_ARGUMENT

    def integ(grid=good, n=3, cameras=cams, depth=fake, ft=fake, trunc=0.1, amin=0.5, sdf=fake):
        return L.pgr_tsdf_integrate(C.byref(grid) if grid is not None else None, n, cameras, depth, ft, trunc, amin, sdf, None)
    for g in bad_grids:
        assert integ(grid=g) == INV
    assert integ(grid=None) == INV
    assert integ(n=0) == INV and integ(n=257) == INV
    assert integ(cameras=None) == INV
    assert integ(depth=None) == INV and integ(ft=None) == INV and integ(sdf=None) == INV
    assert integ(trunc=0.0) == INV and integ(trunc=-1.0) == INV
    mixed = (_lib.PgrCamera * 3)(cam, _lib.PgrCamera(image_width=32, image_height=21, tanfovx=0.5, tanfovy=0.4,
                                                     viewmatrix=fake), cam)
    assert integ(cameras=mixed) == INV
    no_view = (_lib.PgrCamera * 3)(cam, cam, _lib.PgrCamera(image_width=33, image_height=21, tanfovx=0.5, tanfovy=0.4))
    assert integ(cameras=no_view) == INV
    counts = fake
    ws_bytes = L.pgr_march_workspace_bytes(8, 9, 10)
    for g in bad_grids:
        assert L.pgr_march_count(C.byref(g), fake, fake, ws_bytes, counts, None) == INV
        assert L.pgr_march_emit(C.byref(g), fake, fake, ws_bytes, fake, fake, None) == INV
    assert L.pgr_march_count(C.byref(good), None, fake, ws_bytes, counts, None) == INV
    assert L.pgr_march_count(C.byref(good), fake, None, ws_bytes, counts, None) == INV
    assert L.pgr_march_count(C.byref(good), fake, fake, ws_bytes, None, None) == INV
    assert L.pgr_march_count(C.byref(good), fake, fake, ws_bytes - 1, counts, None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert L.pgr_march_emit(C.byref(good), fake, fake, ws_bytes, None, fake, None) == INV
    assert L.pgr_march_emit(C.byref(good), fake, fake, ws_bytes, fake, None, None) == INV
    assert L.pgr_march_emit(C.byref(good), fake, fake, ws_bytes - 1, fake, fake, None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL


def test_largest_component_keeps_the_body():
    small, big = unit_cube(), unit_cube()
    big = Mesh(big.vertices * np.float32(3.0) + np.float32(10.0), big.faces)
    both = Mesh(np.concatenate([small.vertices, big.vertices]), np.concatenate([small.faces, big.faces + 8]))
    assert components(len(both.vertices), both.faces) == 2
    body = both.largest_component()
    assert components(len(body.vertices), body.faces) == 1
    assert body.volume() == pytest.approx(27.0)
    np.testing.assert_array_equal(body.vertices, big.vertices)


# ---- the references against each other ------------------------------------------------------------------------------
MARCH_FIELDS = {
    "sphere": lambda: sphere_sdf(48, 0.7),
    "sphere-through-border": MC.off_centre_sphere,
    "checkerboard-37x35x33": MC.checkerboard,
    "random-signs-37x35x33": MC.random_signs,
    "inside-on-border-21x19x17": MC.inside_on_border,
    "all-inside": lambda: (-np.ones((5, 6, 7), np.float32), MC.unit_grid(7, 6, 5)),
    "2x2x2": lambda: (np.array([-1, 1, 1, -1, 1, -1, 1, 1], np.float32).reshape(2, 2, 2), MC.unit_grid(2, 2, 2)),
}


@pytest.mark.parametrize("name", list(MARCH_FIELDS))
def test_sparse_marching_reference_equals_the_dense_one_as_bytes(name):
    sdf, g = MARCH_FIELDS[name]()
    v_d, f_d = R.march_reference(sdf, g)
    v_s, f_s = R.march_reference(sdf, g, sparse=True)
    assert v_d.dtype == v_s.dtype and f_d.dtype == f_s.dtype and v_d.shape == v_s.shape and f_d.shape == f_s.shape
    assert v_d.tobytes() == v_s.tobytes() and f_d.tobytes() == f_s.tobytes()
    assert (len(f_d) == 0) == (name == "all-inside")
    assert np.isfinite(v_d).all()


def test_open_meshes_are_open_on_the_boundary_planes_only():
    for make in (MC.off_centre_sphere, MC.inside_on_border):
        sdf, g = make()
        v, f = R.march_reference(sdf, g, sparse=True)
        n_open, on_planes = MC.boundary_planes_hold_open_edges(v, f, g)
        assert n_open > 0 and on_planes
        assert_watertight(R.march_reference(MC.force_outer_layer(sdf), g, sparse=True)[1])


ALL_PAIRS = {(t, c) for t in range(6) for c in range(1, 15)}


def test_dense_fields_reach_every_entry_of_the_case_table():
    """The random-sign field reaches all 6 x 14 (tetrahedron, pattern) pairs that have triangles, with and without the
    forced outer layer.  The checkerboard reaches 12: in each tetrahedron the two patterns in which the sign alternates
    along the walk.  The sdf of the first device case (synthetic_case(), through tsdf_reference) reaches 84 of 84 as
    well: its noisy depth makes a rough surface, so no entry of the table was out of that case's reach, only unasserted."""
    sdf, _g = MC.random_signs()
    assert R.table_coverage(sdf) == ALL_PAIRS
    assert R.table_coverage(MC.force_outer_layer(sdf)) == ALL_PAIRS
    chk, _g = MC.checkerboard()
    assert R.table_coverage(chk) == {(t, c) for t in range(6) for c in (5, 10)}
    case = MC.TSDF_CASES["synthetic-41x33x29-7views"]()
    assert R.table_coverage(R.tsdf_reference(*case.reference_args())) == ALL_PAIRS
    # what the hostile field is made of
    assert (sdf == 0).sum() > 100 and np.signbit(sdf[sdf == 0]).any() and not np.signbit(sdf[sdf == 0]).all()
    tiny = np.abs(sdf[sdf != 0]) < np.finfo(np.float32).tiny
    assert tiny.sum() > 100


@pytest.mark.parametrize("name", list(MC.TSDF_CASES))
def test_float64_oracle_agrees_with_the_float32_transcription(name):
    case = MC.TSDF_CASES[name]()
    MC.check_against_oracle(case)
    assert np.isfinite(R.tsdf_reference(*case.reference_args())).all()


def test_oracle_tells_a_wrong_convention_from_the_right_one():
    """What the transcription could share with the kernel unnoticed, the oracle does not share: read the view matrix
    untransposed, centre the image at W/2, or truncate instead of rounding to the nearest pixel centre, and the
    agreement is gone."""
    case = MC.TSDF_CASES["synthetic-41x33x29-7views"]()
    args = list(case.reference_args())
    sdf, masked, tol, _census = R.tsdf_oracle(*args)

    def disagreement(want32):
        return float((~masked & ~(np.abs(want32.astype(np.float64) - sdf) <= tol)).mean())
    assert disagreement(R.tsdf_reference(*args)) == 0.0
    transposed = [np.asarray(m).reshape(4, 4).T.reshape(16).copy() for m in args[1]]
    assert disagreement(R.tsdf_reference(args[0], transposed, *args[2:])) > 0.1
    shifted = [np.asarray(m, np.float32).copy() for m in args[1]]
    for m, v in zip(shifted, case.raw):
        m[12] += np.float32(0.5 * 2.0 * v.tanfovx / case.depth.shape[2]) * m[14]      # half a pixel at z = m[14]: W/2 for (W-1)/2
    assert disagreement(R.tsdf_reference(args[0], shifted, *args[2:])) > 0.01


def test_carve_order_does_not_change_the_carved_set():
    a, b = MC.TSDF_CASES["carve-after-fusing"](), MC.TSDF_CASES["carve-before-fusing"]()
    sa, sb = R.tsdf_reference(*a.reference_args()), R.tsdf_reference(*b.reference_args())
    inside = R.interior(a.grid)
    np.testing.assert_array_equal((sa == 1.0) & inside, (sb == 1.0) & inside)
    assert ((sa == 1.0) & inside).mean() > 0.05 and not np.array_equal(sa, sb)
