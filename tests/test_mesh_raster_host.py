"""The mesh depth renderer's rules and host layers without a GPU: hand-derived coverage, planar triangulations, the analytic
sphere, a marching-tetrahedra silhouette, the BOP reductions against the toolkit's recorded results, argument checks."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import mesh_raster_cases as MC
import mesh_raster_reference as MR

GOLDEN = Path(__file__).resolve().parent / "golden"


def _plane_job(points_uv, faces, z=2.0, f=2.0):
    """Image points (u, v) on the plane Z = z: with f = z = 2 every product and quotient is exact."""
    P = np.array([[u * z / f, v * z / f, z] for u, v in points_uv], np.float32)
    return MC.job(P, faces, fx=f, fy=f)


def test_rectangle_covers_the_hand_computed_samples():
    # u in [1.5, 4.5], v in [0.5, 2.5]; pixel (i, j) samples (i + 0.5, j + 0.5).  The samples of columns 1 and 4 and rows 0
    # and 2 lie ON the edges: left and top edges take theirs (column 1, row 0), right and bottom edges do not.
    job = _plane_job([(1.5, 0.5), (4.5, 0.5), (4.5, 2.5), (1.5, 2.5)], [[0, 1, 2], [0, 2, 3]])
    want = np.zeros((4, 8), bool)
    want[0:2, 1:4] = True
    for flip in (False, True):                                   # no back-face culling: either winding
        j = dict(job, faces=job["faces"][:, ::-1] if flip else job["faces"])
        depth, straddle = MR.render_f32([j], 8, 4, 0.1)
        np.testing.assert_array_equal(depth[0] > 0, want)
        assert straddle == 0 and set(np.unique(depth)) == {0.0, 2.0}
    depth64, masked, bound = MR.render_f64([job], 8, 4, 0.1)
    assert MR.compare(depth, depth64, masked, bound) == 0.0


def _count_image(jobs_of_faces, W, H):
    """How many faces cover each sample: every face rendered alone."""
    return sum((MR.render_f32([j], W, H, 0.1)[0][0] > 0).astype(int) for j in jobs_of_faces)


def _classify_polygon(poly, W, H):
    """(strictly inside, on the boundary) of every sample (i + 0.5, j + 0.5) against a simple polygon with half-integer
    vertices: exact integers in doubled coordinates, an even-odd crossing count.  Knows nothing of triangles or fill rules."""
    P = np.rint(np.asarray(poly, np.float64) * 2).astype(np.int64)
    jj, ii = np.mgrid[0:H, 0:W]
    x, y = 2 * ii + 1, 2 * jj + 1
    inside, boundary = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for a, b in zip(P, np.roll(P, -1, 0)):
        cr = (b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0])
        boundary |= ((cr == 0) & (min(a[0], b[0]) <= x) & (x <= max(a[0], b[0])) & (min(a[1], b[1]) <= y) & (y <= max(a[1], b[1])))
        if a[1] != b[1]:                                          # the edge crosses the sample's row to its right
            inside ^= ((a[1] > y) != (b[1] > y)) & ((cr > 0) == (b[1] > a[1]))
    return inside & ~boundary, boundary


@pytest.mark.parametrize("seed", range(4))
def test_planar_fans_and_strips_cover_interior_samples_once(seed):
    rng = np.random.default_rng(100 + seed)
    W = H = 24
    # a fan around an interior point whose rim sits on half-integers (samples on edges; the hub itself is a sample), every
    # angular gap below pi so the rim is the fan's outline; and a strip with shared edges whose even points lie on one line
    n = 9
    ang = (np.arange(n) + rng.uniform(0.1, 0.9, n)) * 2 * np.pi / n
    rim = np.round((np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(5, 11, (n, 1)) + 12) * 2) / 2
    pts = np.vstack([[12.5, 12.5], rim])
    fan = [[0, 1 + k, 1 + (k + 1) % n] for k in range(n)]
    xs = np.round(np.cumsum(rng.uniform(1, 4, 8)) * 2) / 2
    strip_pts = np.array([[x, 3.5 + (k % 2) * rng.integers(4, 16)] for k, x in enumerate(xs)])
    strip = [[k, k + 1, k + 2] for k in range(len(xs) - 2)]
    outline = np.vstack([strip_pts[0::2], strip_pts[1::2][::-1]])
    for points, faces, poly in ((pts, fan, rim), (strip_pts, strip, outline)):
        job = _plane_job(points, faces)
        union = MR.render_f32([job], W, H, 0.1)[0][0] > 0
        counts = _count_image([dict(job, faces=np.asarray([f], np.int32)) for f in faces], W, H)
        inside, boundary = _classify_polygon(poly, W, H)
        assert inside.sum() > 20
        assert (counts[inside] == 1).all()                        # samples on inner edges and the hub included: no gap, never twice
        assert (counts[~inside & ~boundary] == 0).all()
        assert (counts[boundary] <= 1).all()                      # the fill rule decides on the outline
        np.testing.assert_array_equal(counts > 0, union)


def test_rotated_off_centre_triangle_matches_the_hand_derivation():
    job, W, H, want = MC.rotated_triangle_case()
    for faces in ([[0, 1, 2]], [[0, 2, 1]], [[2, 0, 1]]):        # either winding, any first vertex
        j = dict(job, faces=np.asarray(faces, np.int32))
        depth, straddle = MR.render_f32([j], W, H, 0.25)
        assert straddle == 0 and depth[0].tobytes() == want.tobytes()
        depth64, masked, bound = MR.render_f64([j], W, H, 0.25)
        assert not masked.any()
        np.testing.assert_array_equal(depth64[0] > 0, want > 0)
        assert (np.abs(depth64[0] - want) <= bound * want).all()


def test_shared_edge_at_all_eight_orientations():
    # two triangles sharing an edge through sample points, the edge pointing along the 8 compass directions
    for k in range(8):
        d = np.array([(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)][k], np.float64)
        a = np.array([10.5, 10.5]) - 4 * d
        b = np.array([10.5, 10.5]) + 4 * d
        nrm = np.array([-d[1], d[0]])
        pts = np.array([a, b, (a + b) / 2 + 6 * nrm, (a + b) / 2 - 6 * nrm])
        job = _plane_job(pts, [[0, 1, 2], [1, 0, 3]])
        counts = _count_image([dict(job, faces=np.asarray([f], np.int32)) for f in job["faces"]], 24, 24)
        assert counts.max() == 1
        on_edge = [(int(10 + s * d[0]), int(10 + s * d[1])) for s in range(-3, 4)]
        assert all(counts[j, i] == 1 for i, j in on_edge), k                      # the samples ON the edge: exactly one owner


def test_icosphere_depth_matches_the_analytic_sphere():
    # A chord of the unit icosphere with edge length e stays within the sagitta s = r - sqrt(r^2 - e^2 / 3) of the sphere (the
    # circumradius of a facet is at most e / sqrt 3), measured along the normal; along a view ray that meets the surface at
    # incidence angle a the depth error is at most s / cos a.  The snap moves a vertex by at most 1/512 pixel per axis, i.e.
    # the surface by (sqrt 2 / 512) Z / f sideways, which changes depth by at most that times tan a.  Samples with
    # cos a >= 0.5 are compared: bound = 2 s + 2 sqrt 2 / 512 * Z / f (+ float32 rounding, 1e-5).
    r, zc, f, W = 1.0, 5.0, 300.0, 200
    v, faces = MC.icosphere(4, r)
    e = np.linalg.norm(v[faces[:, 0]].astype(np.float64) - v[faces[:, 1]], axis=1).max()
    sagitta = r - np.sqrt(r * r - e * e / 3.0)
    depth = MR.render_f32([MC.job(v, faces, t=(0, 0, zc), fx=f, fy=f, cx=W / 2, cy=W / 2)], W, W, 0.1)[0][0]
    jj, ii = np.mgrid[0:W, 0:W]
    d = np.stack([(ii + 0.5 - W / 2) / f, (jj + 0.5 - W / 2) / f, np.ones_like(ii, float)], -1)
    dn = d / np.linalg.norm(d, axis=-1, keepdims=True)
    b = dn[..., 2] * zc
    disc = b * b - (zc * zc - r * r)
    hit = disc > 0
    s = b - np.sqrt(np.where(hit, disc, 0))
    z = s * dn[..., 2]
    normal = (s[..., None] * dn - np.array([0, 0, zc])) / r
    cos_a = -(normal * dn).sum(-1)
    sel = hit & (cos_a >= 0.5)
    assert sel.sum() > 5000 and (depth[sel] > 0).all()
    bound = 2 * sagitta + 2 * np.sqrt(2) / 512 * zc / f + 1e-5
    assert np.abs(depth[sel] - z[sel]).max() <= bound
    assert not depth[~hit & (np.hypot(ii + 0.5 - W / 2, jj + 0.5 - W / 2) > f * r / np.sqrt(zc * zc - r * r) + 1)].any()


def _latlon_sphere(n=24):
    """mesh.march has no CPU path (its sphere runs in tests/test_mesh_raster_gpu.py); here a closed latitude-longitude
    sphere with zero-area pole triangles and slivers stands in."""
    lat, lon = np.linspace(0, np.pi, n), np.linspace(0, 2 * np.pi, 2 * n, endpoint=False)
    v = np.array([[np.sin(a) * np.cos(b), np.sin(a) * np.sin(b), np.cos(a)] for a in lat for b in lon], np.float32)
    m = len(lon)
    f = [[i * m + j, (i + 1) * m + j, (i + 1) * m + (j + 1) % m] for i in range(n - 1) for j in range(m)]
    f += [[i * m + j, (i + 1) * m + (j + 1) % m, i * m + (j + 1) % m] for i in range(n - 1) for j in range(m)]
    return v, np.asarray(f, np.int32)


def test_closed_mesh_silhouette_has_no_holes():
    from scipy import ndimage
    v, f = _latlon_sphere()
    depth = MR.render_f32([MC.job(v, f, R=MC.rotation((1, 1, 0), 0.4), t=(0, 0, 4), fx=150, fy=150, cx=48, cy=48)], 96, 96, 0.1)[0][0]
    sil = depth > 0
    assert sil.sum() > 3000
    np.testing.assert_array_equal(ndimage.binary_fill_holes(sil), sil)


def test_gt_info_reduction_equals_the_toolkit():
    import torch
    from pegasus_amd import mesh_render as R
    g = np.load(GOLDEN / "mesh_gt_info.npz")
    W, H = (int(x) for x in g["size"])
    n = len(g["canvases"])
    mask, visib, stats = R.reduce_gt_info_torch(torch.from_numpy(g["canvases"]), (W, H), torch.from_numpy(g["scene_depth"]),
                                                np.arange(n), np.stack([g["K"]] * n), float(g["delta"]))
    np.testing.assert_array_equal(mask.numpy(), np.unpackbits(g["mask"], axis=-1)[..., :W])
    np.testing.assert_array_equal(visib.numpy(), np.unpackbits(g["mask_visib"], axis=-1)[..., :W])
    info = R.info_from_stats(stats)
    for k in ("px_count_all", "px_count_valid", "px_count_visib", "bbox_obj", "bbox_visib"):
        np.testing.assert_array_equal(info[k], g[k], err_msg=k)
    np.testing.assert_allclose(info["visib_fract"], g["visib_fract"], rtol=0, atol=1e-12)
    names = list(g["names"])
    t = names.index("truncated")
    assert g["px_count_all"][t] > np.unpackbits(g["mask"], axis=-1)[t, :, :W].sum() and g["bbox_obj"][t][1] < 0
    # the canvases are the transcription's own renders of the recorded poses
    for k in (0, t):
        job = MC.job(g["vertices"], g["faces"], MC.rotation((1, 2, 3), 0.7), g["t"][k], g["K"][0, 0], g["K"][1, 1],
                     g["K"][0, 2] + W, g["K"][1, 2] + H)
        np.testing.assert_array_equal(MR.render_f32([job], 3 * W, 3 * H, 1.0)[0][0], g["canvases"][k])


def test_vsd_equals_the_toolkit():
    import torch
    from pegasus_amd import mesh_render as R
    g = np.load(GOLDEN / "mesh_vsd.npz")
    meshes = R.MeshSet({1: MC_mesh(g)}, device="cpu")
    taus = [float(t) for t in g["taus"]]
    n = len(g["R_est"])
    for cost in ("step", "tlinear"):
        for norm in (0, 1):
            want = g[f"errors_{cost}_{norm}"]
            for k in range(n):
                stub = lambda jobs, K, size, k=k: np.stack([g["depth_est"][k], g["depth_gt"][k]])
                got = R.vsd(g["R_est"][k], g["t_est"][k].reshape(3, 1), g["R_gt"][k], g["t_gt"][k].reshape(3, 1), g["depth_test"][k],
                            g["K"], float(g["delta"]), taus, bool(norm), float(g["diameter"]), meshes, 1, cost, render=stub)
                np.testing.assert_allclose(got, want[k], rtol=0, atol=1e-9)
    # a batch of estimates against one test image
    got = R.vsd_from_depths(torch.from_numpy(g["depth_est"][3:5]), torch.from_numpy(g["depth_gt"][3]), torch.from_numpy(g["depth_test"][3]),
                            g["K"], float(g["delta"]), taus, False, float(g["diameter"]))
    np.testing.assert_allclose(got[0].numpy(), g["errors_step_0"][3], rtol=0, atol=1e-9)
    assert got.shape == (2, len(taus))
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.render_depth(meshes, [(1, np.eye(3), np.zeros(3))], g["K"], (8, 8))


class _M:
    def __init__(self, v, f):
        self.vertices, self.faces = v, f


def MC_mesh(g):
    return _M(g["vertices"], g["faces"])


def test_mesh_set_reads_the_ply_the_writer_writes(tmp_path):
    from pegasus_amd import mesh, mesh_render as R
    v, f = MC.icosphere(1, 0.05)
    mesh.write_ply(tmp_path / "obj_000003.ply", mesh.Mesh(v, f), scale=1000.0)
    b, bf = MC.box((0.01, 0.02, 0.03))
    mesh.write_ply(tmp_path / "obj_000001.ply", mesh.Mesh(b, bf), scale=1000.0)
    (tmp_path / "models_info.json").write_text('{"1": {"diameter": 74.8}, "3": {"diameter": 100.0}}')
    ms = R.MeshSet.from_dir(tmp_path, device="cpu", scale=0.001)
    assert ms.ranges == {1: (0, 8, 0, 12), 3: (8, len(v), 12, len(f))}
    np.testing.assert_allclose(ms.mesh(3)[0], v, rtol=1e-6)
    np.testing.assert_array_equal(ms.mesh(3)[1], f)
    assert abs(ms.diameters[3] - 0.1) < 1e-12
    with pytest.raises(ValueError):
        R.MeshSet({1: _M(v, f + len(v))}, device="cpu")


def test_entry_points_reject_bad_arguments_before_any_device():
    from pegasus_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(0x1000)
    bad = _lib.PGR_ERR_INVALID_ARGUMENT
    good = (_lib.PgrMeshJob * 1)(_lib.PgrMeshJob(vertex_first=0, vertex_count=8, face_first=0, face_count=12, slot=0))

    def depth(jobs=good, n_jobs=1, v=fake, f=fake, nv=8, nf=12, W=64, H=64, near=0.1, out=fake, slots=1, cnt=fake, ws=fake):
        return L.pgr_mesh_depth(v, nv, f, nf, n_jobs, jobs, W, H, near, out, slots, cnt, ws, 1 << 30, None)
    assert depth(out=None) == bad and depth(cnt=None) == bad and depth(v=None) == bad and depth(f=None) == bad
    assert depth(jobs=None) == bad and depth(n_jobs=-1) == bad
    for size in (0, 8193, -4):
        assert depth(W=size) == bad and depth(H=size) == bad
    assert depth(nf=11) == bad and depth(nv=7) == bad                           # a range outside the arrays
    for kw in (dict(face_first=-1), dict(vertex_count=-2), dict(slot=1), dict(slot=-1)):
        fields = dict(vertex_first=0, vertex_count=8, face_first=0, face_count=12, slot=0)
        fields.update(kw)
        assert depth(jobs=(_lib.PgrMeshJob * 1)(_lib.PgrMeshJob(**fields))) == bad, kw
    assert depth(near=0.0) == bad and depth(near=float("nan")) == bad
    assert depth(ws=None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    # workspace size: host-only, 0 for bad input
    assert L.pgr_mesh_depth_workspace_bytes(1, good) >= 12 * 16 + 8
    assert L.pgr_mesh_depth_workspace_bytes(0, good) == 0 and L.pgr_mesh_depth_workspace_bytes(-3, good) == 0
    assert L.pgr_mesh_depth_workspace_bytes(1, None) == 0
    assert L.pgr_mesh_depth_workspace_bytes(1, (_lib.PgrMeshJob * 1)(_lib.PgrMeshJob(face_count=-1))) == 0
    assert L.pgr_mesh_depth_workspace_bytes(1, (_lib.PgrMeshJob * 1)(_lib.PgrMeshJob(face_count=(1 << 22) + 1))) == 0
    many = (_lib.PgrMeshJob * 40)(*[_lib.PgrMeshJob(face_count=1000 * (k + 1)) for k in range(40)])
    assert L.pgr_mesh_depth_workspace_bytes(40, many) >= sum(1000 * (k + 1) for k in range(32)) * 16       # the larger of the two launches

    gj = (_lib.PgrGtInfoJob * 1)(_lib.PgrGtInfoJob(slot=0, frame=0, fx=100.0, fy=100.0, cx=10.0, cy=10.0))

    def info(canv=fake, slots=1, Wc=60, Hc=60, mx=20, my=20, scene=fake, frames=1, W=20, H=20, n=1, jobs=gj, mask=fake, vis=fake,
             stats=fake):
        return L.pgr_bop_gt_info(canv, slots, Wc, Hc, mx, my, scene, frames, W, H, n, jobs, 15.0, mask, vis, stats, None)
    for kw in (dict(canv=None), dict(scene=None), dict(mask=None), dict(vis=None), dict(stats=None), dict(jobs=None), dict(n=-1),
               dict(Wc=0), dict(Hc=8193), dict(mx=-1), dict(mx=41), dict(my=45), dict(W=0), dict(frames=0), dict(slots=0)):
        assert info(**kw) == bad, kw
    for kw in (dict(slot=1), dict(frame=2), dict(fx=0.0), dict(cy=float("inf"))):
        fields = dict(slot=0, frame=0, fx=100.0, fy=100.0, cx=10.0, cy=10.0)
        fields.update(kw)
        assert info(jobs=(_lib.PgrGtInfoJob * 1)(_lib.PgrGtInfoJob(**fields))) == bad, kw
    assert info(n=0) == _lib.PGR_OK
