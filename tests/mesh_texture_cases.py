"""The cases of the texture kernels shared by the host tests (every mutant of tests/mesh_texture_reference.py changes one) and
the GPU tests (kernels against the restatement).  No GPU; only ``round_trip`` runs the restatements (once, cached)."""
import functools

import numpy as np

import mesh_raster_cases as MC
import mesh_shade_cases as SC

TEXTURE_SIZES = ((1, 1), (2, 3), (5, 4), (64, 64))                    # width, height: odd widths leave rows off 4-byte boundaries


def textures(seed=21):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for w, h in TEXTURE_SIZES]


def shade_case(textured=True):
    """Canvas 33 x 19 (no multiple of the 16 x 4 wave tile), two slots.  Slot 0: job 0 (texture 64 x 64: a face with a 4 : 1
    depth ratio whose left and top edges carry u = 1 and v = 1 exactly, a face of the other winding with UVs below 0 and above
    1, a face with a NaN corner), job 1 (texture 5 x 4, nearer over a part, negative area: b and c swap) and job 2 (untextured,
    vertex colours) overlap.  Slot 1: job 3 (texture 2 x 3, u = 0 and v = 0 exactly along two edges, UVs above 1) and job 4
    (texture 1 x 1).  With ``textured`` False every job is untextured."""
    rng = np.random.default_rng(22)
    nan = np.nan
    pts0 = [(1.5, 1.5), (30.5, 1.5), (1.5, 17.5), (31.5, 18.25), (4.5, 18.25), (31.5, 3.5), (20.25, 0.5), (32.5, 0.5), (32.5, 2.75)]
    P0 = SC.plane_points(pts0, z=[1.0, 4.0, 2.0, 3.0, 2.5, 3.5, 0.75, 0.75, 0.75])
    j0 = SC.with_attributes(MC.job(P0, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], fx=2.0, fy=2.0), rng)
    j0["corner_uv"] = np.array([[[1, 1], [0, 1], [1, 0]], [[-0.3, 1.4], [1.2, -0.2], [0.5, 0.5]], [[nan, 0.25], [0.5, 0.5], [0.75, 1.0]]], np.float32)
    j0["texture"] = 3
    P1 = SC.plane_points([(8.5, 4.5), (8.5, 16.5), (24.5, 4.5)], z=[0.5, 0.75, 1.5])
    j1 = SC.with_attributes(MC.job(P1, [[0, 1, 2]], fx=2.0, fy=2.0), rng)
    j1["corner_uv"] = np.array([[[0.05, 0.1], [0.1, 0.95], [0.9, 0.2]]], np.float32)
    j1["texture"] = 2
    P2 = SC.plane_points([(12.5, 0.5), (28.5, 9.5), (10.5, 15.5)], z=[0.625, 1.25, 0.625])
    j2 = SC.with_attributes(MC.job(P2, [[0, 1, 2]], fx=2.0, fy=2.0), rng)
    j2["corner_uv"] = np.array([[[0.2, 0.2], [0.8, 0.3], [0.4, 0.9]]], np.float32)
    j2["texture"] = -1
    P3 = SC.plane_points([(0.5, 0.5), (32.5, 0.5), (0.5, 18.5), (32.25, 18.25), (2.5, 18.25), (32.25, 1.5)], z=[2.0, 1.0, 3.0, 2.0, 2.0, 2.0])
    j3 = SC.with_attributes(MC.job(P3, [[0, 1, 2], [3, 4, 5]], fx=2.0, fy=2.0, slot=1), rng)
    j3["corner_uv"] = np.array([[[0.0, 0.0], [1.5, 0.0], [0.0, 1.25]], [[1.0, 1.0], [0.0, 1.0], [1.0, 0.0]]], np.float32)
    j3["texture"] = 1
    P4 = SC.plane_points([(10.5, 5.5), (20.5, 5.5), (10.5, 12.5)], z=0.5)
    j4 = SC.with_attributes(MC.job(P4, [[0, 1, 2]], fx=2.0, fy=2.0, slot=1), rng)
    j4["corner_uv"] = np.array([[[0.3, 0.3], [7.0, -2.0], [0.1, 0.6]]], np.float32)
    j4["texture"] = 0
    jobs = [j0, j1, j2, j3, j4]
    if not textured:
        for j in jobs:
            j["texture"] = -1
    return SC.case(jobs, 33, 19, n_slots=2, smooth=True, use_colors=True, light=(1.5, -2.0, 0.5), ambient=0.4, bg=(0.25, 0.5, 0.75))


# ---- the atlas ----------------------------------------------------------------------------------------------------------
def strip_mesh(n_faces, seed):
    """A triangle strip of ``n_faces`` faces over random points (no face degenerate)."""
    rng = np.random.default_rng(seed)
    v = (rng.random((n_faces + 2, 3)) * 2.0 - 1.0).astype(np.float32)
    f = np.array([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(n_faces)], np.int32)
    return v, f


def atlas_meshes():
    """name -> (vertices, faces, cell): F in {1, 2, 3, 5} at s = 4 and s = 5 (odd F leaves half a cell empty, F = 5 a tail
    cell), the level-1 icosphere at s = 8 (80 faces: 40 cells in 7 columns, 2 tail cells), and five faces of which one has no
    area, one an index beyond the vertices and one a negative index."""
    out = {}
    for s in (4, 5):
        for F in (1, 2, 3, 5):
            v, f = strip_mesh(F, 30 + F)
            out[f"F={F} s={s}"] = (v, f, s)
    v, f = MC.icosphere(1, 1.0)
    out["icosphere s=8"] = (np.asarray(v, np.float32), np.asarray(f, np.int32), 8)
    v, f = strip_mesh(5, 40)
    f = f.copy()
    f[1] = [2, 2, 3]
    f[2] = [2, 3, 99]
    f[4] = [-1, 5, 6]
    out["degenerate faces s=5"] = (v, f, 5)
    return out


def pack_inputs(face_of_texel, n_faces, seed=50):
    """(colors float32 [T,3], seen int32 [T], face_fill uint8 [F,3]) for a pack: faces with f % 3 == 0 fully seen, f % 3 == 1
    seen on every other texel, f % 3 == 2 unseen; colours in [0, 1] with a NaN among the seen ones."""
    rng = np.random.default_rng(seed)
    owner = np.asarray(face_of_texel).reshape(-1)
    n = len(owner)
    colors = rng.random((n, 3)).astype(np.float32)
    kind = np.where(owner >= 0, owner % 3, 0)                          # texels of no face count as seen too: the pack ignores them
    seen = np.where(kind == 0, 1 + rng.integers(0, 3, n), np.where((kind == 1) & (np.arange(n) % 2 == 0), 2, 0)).astype(np.int32)
    lit = np.nonzero(seen > 0)[0]
    if len(lit):
        colors[lit[0], 1] = np.nan
    return colors, seen, rng.integers(0, 256, (n_faces, 3)).astype(np.uint8)


# ---- bake, then render: the round trip --------------------------------------------------------------------------------------
ROUND_TRIP_COLOUR = (0.2, 0.6, 0.4)                                    # 51, 153, 102 of 255: far from a rounding boundary
ROUND_TRIP_CELL = 8


@functools.lru_cache(maxsize=None)
def round_trip():
    """The level-1 icosphere inscribed in the analytic sphere of mesh_attr_cases, its twelve synthetic views with the colour
    images replaced by one constant colour, the atlas baked from them at s = 8 by the restatements, and the view (of those
    twelve) in which the largest share of the covered pixels lies on faces with face_seen > 0, rendered by the restatement
    with ambient 1 (light_w == 1) and the nearest filter.  Computed once on the CPU, shared by the host and the GPU test."""
    import mesh_attr_cases as AC
    import mesh_attr_reference as AR
    import mesh_texture_reference as TR
    c = AC.analytic_sphere(1, 0.3)
    v, f = np.asarray(c.vertices, np.float32), np.asarray(c.extra["faces"], np.int32)
    colour = np.asarray(ROUND_TRIP_COLOUR, np.float32)
    color = ((1.0 - c.final_T.astype(np.float64))[:, None] * colour[None, :, None, None].astype(np.float64)).astype(np.float32)
    # the flat faces lie up to R (1 - cos) inside the sphere the depth images show: the tolerance spans that sag and the slide
    depth_tol = float(c.depth_tol) + 0.25 * AC.SPHERE_RADIUS
    points, normals, owner = TR.atlas_points_f32(v, f, ROUND_TRIP_CELL)
    args = list(c.reference_args())
    args[0], args[1], args[6], args[9], args[12] = points, normals, color, depth_tol, (0.5, 0.5, 0.5)
    colors, seen = AR.colors_f32(*args)[:2]
    texture, face_seen = TR.atlas_pack(len(f), ROUND_TRIP_CELL, owner, colors, seen)
    W, H = c.raw[0].width, c.raw[0].height
    corner_uv = TR.atlas_layout(len(f), ROUND_TRIP_CELL)[5]
    texels, table = TR.pack_textures([texture], lead=0, gap=0)
    best = None
    for k, view in enumerate(c.raw):
        M = np.asarray(view.world_view_transform, np.float64).reshape(4, 4).T
        pose = dict(R=M[:3, :3], t=M[:3, 3], fx=W / (2 * view.tanfovx), fy=H / (2 * view.tanfovy), cx=W / 2.0, cy=H / 2.0)
        job = dict(MC.job(v, f, **pose), corner_uv=corner_uv, texture=0)
        ref = TR.shade_textured_f32([job], W, H, 1e-3, texels, table, ambient=1.0)
        hit = ref["job_id"][0] >= 0
        share = float((face_seen[ref["face_id"][0][hit]] > 0).mean()) if hit.any() else 0.0
        if best is None or share > best["share"]:
            best = dict(view=k, pose=pose, ref=ref, share=share, covered=int(hit.sum()))
    return dict(case=c, vertices=v, faces=f, color=color, depth_tol=depth_tol, texture=texture, face_seen=face_seen, corner_uv=corner_uv,
                size=(W, H), colour=colour, **best)
