"""Vertex clustering, host side: the reference (tests/decimate_reference.py) against hand-worked answers, every clause of the
rule shown to be observable by a mutant of the reference, the invariants that follow from the rule, and the host paths of
pegasus_amd.decimate and pegasus_amd.mesh that need no device.  DESIGN.md section 19."""
import math
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import decimate_cases as DC
from decimate_reference import cluster_reference, quadric_tolerance, segmented_sum


def run(name, contraction="quadric", mutant=None):
    v, f, voxel = DC.HAND_CASES[name]()
    return cluster_reference(v, f, voxel, contraction, mutant), v, f, voxel


# ---- hand-worked answers ------------------------------------------------------------------------------------------------
def test_two_triangles_in_one_cell_leave_one_vertex_and_no_face():
    r, v, _f, _voxel = run("two_triangles_one_cell")
    assert len(r.vertices) == 1 and r.faces.shape == (0, 3)
    assert (r.cluster_of_vertex == 0).all() and r.used_quadric.tolist() == [0]
    assert np.array_equal(r.vertices[0], v.astype(np.float64).mean(axis=0))      # dyadic: the mean is exact


def test_unit_square_over_four_cells():
    r, v, _f, _voxel = run("unit_square")
    assert r.cluster_of_vertex.tolist() == [0, 1, 2, 3]                          # (cy, cx) order
    assert r.faces.tolist() == [[0, 1, 3], [0, 3, 2]]                            # given as (3,0,1) and (2,0,3)
    assert np.array_equal(r.vertices, v.astype(np.float64))                      # one vertex per cell: itself, exactly
    assert not r.used_quadric.any()                                              # flat: rank-deficient everywhere


def test_duplicates_are_removed_and_opposites_both_stay():
    assert run("duplicate_pair")[0].faces.tolist() == [[0, 1, 2]]
    assert run("opposite_pair")[0].faces.tolist() == [[0, 1, 2], [0, 2, 1]]


def test_a_flat_cluster_takes_the_average():
    r, _v, _f, _voxel = run("flat_cluster")
    assert len(r.vertices) == 4 and not r.used_quadric.any()
    assert (r.terms > 0).all() and (np.abs(r.det) <= r.threshold).all()          # rank 1: det is 0 up to rounding
    assert np.array_equal(r.vertices, r.average)


def corner_cluster(r):
    k = np.nonzero((r.cells == np.asarray(DC.CORNER_CELL)).all(axis=1))[0]
    assert len(k) == 1
    return int(k[0])


def test_three_orthogonal_planes_meet_at_the_quadric_position():
    r, _v, _f, voxel = run("corner_inside")
    k = corner_cluster(r)
    assert r.used_quadric[k] == 1 and r.members[k] == 3 and r.terms[k] == 3
    assert np.abs(r.vertices[k] - np.asarray(DC.CORNER_INSIDE_APEX)).max() <= 1e-12 * voxel
    assert r.used_quadric.sum() == 1                                             # every other cluster sees one plane


def test_the_same_corner_in_the_neighbouring_cell_is_rejected_by_the_box_test():
    r, v, _f, voxel = run("corner_in_neighbour")
    k = corner_cluster(r)
    assert abs(r.det[k]) > r.threshold[k]                                        # well conditioned: only the box test says no
    assert np.abs(r.x[k] - np.asarray([1.125, 0.5, 0.5])).max() <= 1e-12 * voxel and r.x[k, 0] > voxel
    assert r.used_quadric[k] == 0
    assert np.abs(r.vertices[k] - v[1:4].astype(np.float64).mean(axis=0)).max() <= 1e-15      # the mean of its three vertices


# ---- every clause is observable -----------------------------------------------------------------------------------------
def differs(a, b):
    return (a.vertices.shape != b.vertices.shape or not np.array_equal(a.vertices, b.vertices) or
            not np.array_equal(a.faces, b.faces) or not np.array_equal(a.cluster_of_vertex, b.cluster_of_vertex) or
            not np.array_equal(a.used_quadric, b.used_quadric))


@pytest.mark.parametrize("mutant,case", [("no_half_voxel", "half_voxel_split"), ("count_once", "two_corner_face"),
                                         ("flip_rotation", "unit_square"), ("keep_duplicates", "duplicate_pair"),
                                         ("order_xyz", "unit_square"), ("no_box_test", "corner_in_neighbour")])
def test_each_mutant_of_the_reference_differs_on_its_named_case(mutant, case):
    assert differs(run(case)[0], run(case, mutant=mutant)[0])


def test_the_mutants_differ_where_they_should():
    assert len(run("half_voxel_split")[0].vertices) == 4 and len(run("half_voxel_split", mutant="no_half_voxel")[0].vertices) == 1
    twice, once = run("two_corner_face")[0], run("two_corner_face", mutant="count_once")[0]
    k = corner_cluster(twice)
    assert twice.used_quadric[k] == once.used_quadric[k] == 1 and twice.terms[k] == 5 and once.terms[k] == 4
    assert twice.vertices[k, 2] > once.vertices[k, 2] > 1.0                      # the doubled plane z = 1.25 pulls harder
    assert run("unit_square", mutant="flip_rotation")[0].faces.tolist() == [[0, 2, 3], [0, 3, 1]]
    assert run("duplicate_pair", mutant="keep_duplicates")[0].faces.tolist() == [[0, 1, 2], [0, 1, 2]]
    assert run("unit_square", mutant="order_xyz")[0].cluster_of_vertex.tolist() == [0, 2, 1, 3]
    free = run("corner_in_neighbour", mutant="no_box_test")[0]
    assert free.used_quadric[corner_cluster(free)] == 1


# ---- the fixed order of the sums ----------------------------------------------------------------------------------------
def test_segmented_sum_is_the_rule_written_out():
    rng = np.random.default_rng(0)
    sizes = [0, 1, 63, 64, 65, 200, 0, 1500]
    values = rng.standard_normal((sum(sizes), 2)) * 10.0 ** rng.integers(-8, 8, (sum(sizes), 1))
    start = np.concatenate([[0], np.cumsum(sizes)])
    got = segmented_sum(values, start)
    for k, m in enumerate(sizes):
        p = np.zeros((64, 2))
        for j in range(m):                                                       # partial j mod 64, ascending j
            p[j % 64] = p[j % 64] + values[start[k] + j]
        d = 32
        while d >= 1:                                                            # p[l] += p[l + d], l < d
            p[:d] = p[:d] + p[d:2 * d]
            d //= 2
        assert np.array_equal(got[k], p[0])


# ---- invariants -----------------------------------------------------------------------------------------------------
def surface_cases():
    ico = DC.icosphere()
    yield "icosphere_16", ico[0], ico[1], DC.voxel_for(ico[0], 16)
    for name in ("beyond_a_tile", "dense_cell", "thin_slab", "degenerate_faces"):
        yield (name, *DC.SHAPE_CASES[name]())


@pytest.mark.parametrize("contraction", ["average", "quadric"])
def test_every_output_vertex_lies_in_its_closed_cell_and_near_its_members(contraction):
    for name, v, f, voxel in surface_cases():
        r = cluster_reference(v, f, voxel, contraction)
        upper = r.corner + voxel
        assert ((r.vertices >= r.corner) & (r.vertices <= upper)).all(), name    # closed cell [corner, fl(corner + voxel)]
        # an input vertex lies in the same cell up to the rounding of its own cell index: (x - lo) / voxel and lo + c voxel
        # round three times, each by at most 2^-53 of a magnitude below |x| + |lo| + voxel
        slack = 4.0 * 2.0 ** -53 * (np.abs(v).max() + np.abs(r.lo).max() + voxel)
        x = v.astype(np.float64)
        own = r.cluster_of_vertex
        assert ((x >= r.corner[own] - slack) & (x <= upper[own] + slack)).all(), name
        dist = np.linalg.norm(x - r.vertices[own], axis=1)
        assert dist.max() <= math.sqrt(3.0) * (voxel + 2.0 * slack), name


def test_a_voxel_below_the_smallest_gap_returns_the_input_renumbered():
    rng = np.random.default_rng(3)
    g = np.arange(6, dtype=np.float32)
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[rng.permutation(216)]
    f = np.asarray([t for t in rng.integers(0, 216, (400, 3)) if len(set(t)) == 3], np.int32)
    r = cluster_reference(v, f, 0.5, "average")
    assert len(r.vertices) == 216 and sorted(r.cluster_of_vertex.tolist()) == list(range(216))
    assert np.array_equal(r.vertices[r.cluster_of_vertex], v.astype(np.float64))
    mapped = r.cluster_of_vertex[f]
    s = np.argmin(mapped, axis=1)[:, None]
    canon = np.take_along_axis(mapped, (s + np.arange(3)) % 3, axis=1)
    assert np.array_equal(r.faces, np.unique(canon, axis=0))


def test_tolerance_is_finite_where_the_quadric_is_used():
    v, f = DC.icosphere()
    voxel = DC.voxel_for(v, 16)
    r = cluster_reference(v, f, voxel)
    tol, masked = quadric_tolerance(r, voxel)
    used = r.used_quadric.astype(bool)
    assert used.sum() > 0 and np.isfinite(tol[used]).all()
    assert tol[used].max() < 1e-6 * voxel and masked.mean() <= 0.01


# ---- the host side of the package -----------------------------------------------------------------------------------
def test_write_urdf_collision_filename_changes_the_collision_element_only(tmp_path):
    from pegasus_amd.mesh import Mesh, write_urdf
    from mesh_raster_cases import icosphere
    mesh = Mesh(*icosphere(1, 0.05))
    write_urdf(tmp_path / "a.urdf", "obj_000001.obj", mesh, 0.1)
    write_urdf(tmp_path / "b.urdf", "obj_000001.obj", mesh, 0.1, collision_filename=None)
    write_urdf(tmp_path / "c.urdf", "obj_000001.obj", mesh, 0.1, collision_filename="obj_000001_collision.obj")
    assert (tmp_path / "a.urdf").read_bytes() == (tmp_path / "b.urdf").read_bytes()
    a, c = ET.parse(tmp_path / "a.urdf").getroot(), ET.parse(tmp_path / "c.urdf").getroot()
    assert c.find("link/collision/geometry/mesh").get("filename") == "obj_000001_collision.obj"
    assert c.find("link/visual/geometry/mesh").get("filename") == "obj_000001.obj"
    assert ET.tostring(a.find("link/inertial")) == ET.tostring(c.find("link/inertial"))
    assert a.find("link/collision/geometry/mesh").get("filename") == "obj_000001.obj"


def test_there_is_no_cpu_path_and_arguments_are_checked_first():
    import torch
    from pegasus_amd import decimate as D
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.cluster_vertices(v, f, 1.0)
    with pytest.raises(ValueError, match="float32"):
        D.cluster_vertices(v.double(), f, 1.0)
    with pytest.raises(ValueError, match="int32"):
        D.cluster_vertices(v, f.long(), 1.0)
    with pytest.raises(ValueError, match="contraction"):
        D.cluster_vertices(v, f, 1.0, contraction="median")
    with pytest.raises(SystemExit):
        D.main(["--models", "x", "--ratio", "0.1", "--faces", "10"])             # one size at a time
