"""The inputs of the vertex-attribute tests, built in NumPy alone so that the host tests run the references on exactly what
the device tests feed the kernels: meshes for pgr_mesh_vertex_normals, and meshes with views and images for
pgr_mesh_vertex_colors, each with the branches it is there to reach (mesh_attr_reference's census keys)."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

import mesh_attr_reference as AR
import mesh_cases as MC
import mesh_reference as MR

f32 = np.float32


# ---- meshes ---------------------------------------------------------------------------------------------------------
def icosphere(subdivisions, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(vertices float32 [V,3], faces int32 [F,3], outward winding): 10 * 4^s + 2 vertices."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(x, np.float64) / math.sqrt(1.0 + t * t) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    verts = np.asarray(center, np.float64)[None, :] + radius * np.asarray(v)
    return verts.astype(f32), np.asarray(f, np.int32)


CUBE_VERTICES = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], f32)          # index = x + 2 y + 4 z
# every face split along the diagonal that starts at its lowest corner index, outward winding
CUBE_FACES = np.array([[0, 2, 3], [0, 3, 1],          # z = 0 (normal -z): diagonal 0-3
                       [4, 5, 7], [4, 7, 6],          # z = 1 (+z): diagonal 4-7
                       [0, 1, 5], [0, 5, 4],          # y = 0 (-y): diagonal 0-5
                       [2, 6, 7], [2, 7, 3],          # y = 1 (+y): diagonal 2-7
                       [0, 4, 6], [0, 6, 2],          # x = 0 (-x): diagonal 0-6
                       [1, 3, 7], [1, 7, 5]], np.int32)   # x = 1 (+x): diagonal 1-7


def fan(n_triangles, wave=0.0):
    """Vertex 0 at the origin shared by ``n_triangles`` triangles to a rim of n + 1 points on a quarter circle in the plane
    z = 0 (counter-clockwise seen from +z), lifted by ``wave`` * sin(5 angle)."""
    ang = np.linspace(0.0, 0.5 * math.pi, n_triangles + 1)
    rim = np.stack([np.cos(ang), np.sin(ang), wave * np.sin(5.0 * ang)], axis=1)
    v = np.concatenate([np.zeros((1, 3)), rim]).astype(f32)
    k = np.arange(n_triangles, dtype=np.int32)
    return v, np.stack([np.zeros_like(k), 1 + k, 2 + k], axis=1)


def random_mesh(n_vertices, n_faces, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, size=(n_vertices, 3)).astype(f32)
    return v, rng.integers(0, n_vertices, size=(n_faces, 3)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def gyroid_mesh():
    grid = MC.unit_grid(*MC.RAGGED)
    return MR.march_reference(MC.force_outer_layer(MC.gyroid(grid)), grid)


def _hostile_faces():
    """A random mesh whose face list also holds zero-area faces (a repeated index, three points on a line) and faces with
    an index of V, -1, INT32_MIN and INT32_MAX."""
    v, f = random_mesh(40, 90, seed=5)
    v[30], v[31], v[32] = (0.0, 0.0, 0.0), (0.25, 0.5, -0.125), (0.5, 1.0, -0.25)        # collinear, exactly
    extra = np.array([[3, 3, 9], [7, 8, 7], [30, 31, 32], [40, 1, 2], [1, -1, 2], [1, 2, -2 ** 31], [2 ** 31 - 1, 0, 5]], np.int32)
    return v, np.concatenate([f[:45], extra, f[45:]])


def _mirrored():
    v, f = icosphere(2, 0.3, (0.1, -0.2, 0.05))
    return (v * np.array([-1.0, 1.0, 1.0], f32)).astype(f32), f


def _far_from_origin():
    v, f = icosphere(2, 0.25)
    return (v + np.array([1000.0, -2000.0, 500.0], f32)).astype(f32), f


# name -> (builder of (vertices, faces), census keys that must be > 0)
NORMAL_CASES = {
    "V1-one-degenerate-face": (lambda: (np.array([[0.5, -1.0, 2.0]], f32), np.zeros((1, 3), np.int32)), ("degenerate", "isolated")),
    "V63": (lambda: random_mesh(63, 200, 63), ("used",)),
    "V64": (lambda: random_mesh(64, 200, 64), ("used",)),
    "V65": (lambda: random_mesh(65, 200, 65), ("used",)),
    "V257-F300": (lambda: random_mesh(257, 300, 257), ("used", "isolated")),
    "F0": (lambda: (random_mesh(70, 1, 3)[0], np.zeros((0, 3), np.int32)), ("isolated",)),
    "icosphere-2": (lambda: icosphere(2, 0.1, (0.013, -0.021, 0.008)), ("used",)),
    "icosphere-3": (lambda: icosphere(3, 0.1, (0.013, -0.021, 0.008)), ("used",)),
    "gyroid-37x35x33": (gyroid_mesh, ("used",)),
    "fan-5000-on-one-vertex": (lambda: fan(5000, wave=0.3), ("used",)),
    "mirrored": (_mirrored, ("used",)),
    "degenerate-and-out-of-range": (_hostile_faces, ("used", "degenerate", "out_of_range")),
    "far-from-origin": (_far_from_origin, ("used",)),
}


# ---- colour cases -----------------------------------------------------------------------------------------------------
@dataclass
class ColorCase:
    vertices: np.ndarray             # float32 [V,3]
    normals: object                  # float32 [V,3] or None
    raw: list                        # scenes.View per view
    color: np.ndarray                # float32 [n,3,H,W], premultiplied over zero
    depth: np.ndarray                # float32 [n,H,W]
    final_T: np.ndarray              # float32 [n,H,W]
    depth_tol: float
    alpha_min: float = 0.5
    cos_min: float = 0.3
    fill: tuple = (0.5, 0.25, 0.75)
    reaches: tuple = ()              # census keys (mesh_attr_reference.COLOR_CENSUS) that must be > 0
    want_seen: bool = True           # False: the device test passes NULL for ``seen``
    extra: dict = field(default_factory=dict)

    def reference_args(self):
        return (self.vertices, self.normals, [v.world_view_transform.reshape(16) for v in self.raw],
                [v.tanfovx for v in self.raw], [v.tanfovy for v in self.raw],
                np.stack([np.asarray(v.camera_center, f32).reshape(3) for v in self.raw]), self.color, self.depth, self.final_T,
                self.depth_tol, self.alpha_min, self.cos_min, self.fill)


# the analytic case of the issue: a sphere whose surface colour is linear in the position
SPHERE_RADIUS, SPHERE_CENTER = 0.1, np.array([0.013, -0.021, 0.008])
SPHERE_A = np.array([[2.0, 1.0, -0.5], [-1.0, 1.5, 1.0], [0.5, -1.0, 2.0]])
SPHERE_ALPHA = 0.8


def sphere_color(points):
    return 0.5 + (np.asarray(points, np.float64) - SPHERE_CENTER) @ SPHERE_A.T


def sphere_images(raw, W, H, radius=SPHERE_RADIUS, center=SPHERE_CENTER, alpha=SPHERE_ALPHA):
    """Exact ray-sphere images: depth (view-space z of the first hit), final_T = 1 - alpha inside the silhouette and 1 outside,
    colour = alpha * sphere_color(hit), 0 outside."""
    n = len(raw)
    depth = np.zeros((n, H, W), f32)
    final_T = np.ones((n, H, W), f32)
    color = np.zeros((n, 3, H, W), f32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for k, v in enumerate(raw):
        M = v.world_view_transform.astype(np.float64).T                 # world -> view (column vectors)
        c = M[:3, :3] @ center + M[:3, 3]
        fx, fy = W / (2 * v.tanfovx), H / (2 * v.tanfovy)
        d = np.stack([(xx - (W - 1) / 2) / fx, (yy - (H - 1) / 2) / fy, np.ones_like(xx)], axis=-1)     # z = 1
        a = (d * d).sum(-1)
        b = (d * c).sum(-1)
        disc = b * b - a * (c @ c - radius * radius)
        hit = disc > 0
        t = (b - np.sqrt(np.where(hit, disc, 0))) / a
        world = (t[..., None] * d - M[:3, 3]) @ M[:3, :3]               # R^T (p_view - t)
        depth[k] = np.where(hit, t, 0)
        final_T[k] = np.where(hit, 1.0 - alpha, 1.0)
        color[k] = np.where(hit[None], alpha * np.moveaxis(sphere_color(world), -1, 0), 0.0)
    return color, depth, final_T


def sphere_slide(raw, cos_min, dist=0.6):
    """How far a pixel's footprint reaches along the tangent plane of a vertex seen at cos_min: half a pixel's diagonal at the
    farthest depth, over the cosine."""
    z_max = dist + SPHERE_RADIUS
    f_min = min(min(v.width / (2 * v.tanfovx), v.height / (2 * v.tanfovy)) for v in raw)
    return (0.5 * math.sqrt(2.0) * z_max / f_min) / cos_min


def analytic_sphere(subdivisions, cos_min, n_views=12, W=61, H=47, fov_deg=(24.0, 20.0), dist=0.6):
    raw = MC.raw_views_around(SPHERE_CENTER, dist, n_views, W, H, math.radians(fov_deg[0]), math.radians(fov_deg[1]))
    color, depth, final_T = sphere_images(raw, W, H)
    v, f = icosphere(subdivisions, SPHERE_RADIUS, SPHERE_CENTER)
    slide = sphere_slide(raw, cos_min, dist)
    return ColorCase(v, AR.normals_f32(v, f), raw, color, depth, final_T, 2.0 * slide, 0.5, cos_min,
                     reaches=("see_through", "depth_in_front", "facing_away", "used"), extra=dict(slide=slide, faces=f))


def _textured(rng, depth, final_T, gain=1.0):
    """A premultiplied colour image for given final_T: alpha times a smooth pattern plus pixel noise, times ``gain``."""
    n, H, W = depth.shape
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.4 * np.sin(0.4 * xx + 0.7 * c + 0.3 * k) * np.cos(0.3 * yy - 0.2 * c)
                     for k in range(n) for c in range(3)]).reshape(n, 3, H, W)
    base = gain * (base + 0.05 * rng.uniform(size=base.shape))
    return ((1.0 - final_T.astype(np.float64))[:, None] * base).astype(f32)


@functools.lru_cache(maxsize=None)
def _tsdf_mesh(name):
    """The marched mesh of a TSDF case of mesh_cases (both steps by the NumPy references), with its normals."""
    c = MC.TSDF_CASES[name]()
    sdf = MR.tsdf_reference(*c.reference_args())
    v, f = MR.march_reference(sdf, c.grid)
    return c, v, f, AR.normals_f32(v, f)


def over_tsdf_case(name, tol_voxels=2.0, cos_min=0.3, reaches=(), gain=1.0, seed=31, **kw):
    """The images of a TSDF case over the mesh marched from them."""
    c, v, f, n = _tsdf_mesh(name)
    rng = np.random.default_rng(seed)
    return ColorCase(v, n, c.raw, _textured(rng, c.depth, c.final_T, gain), c.depth, c.final_T, tol_voxels * c.grid.voxel,
                     c.alpha_min, cos_min, reaches=reaches, extra=dict(faces=f), **kw)


def thin_image(W, H):
    """The analytic sphere in one pixel column, one row or one pixel, 6 x 5 degrees wide: the sphere spills over every side."""
    c = analytic_sphere(3, 0.3, n_views=9, W=W, H=H, fov_deg=(6.0, 5.0))
    c.reaches = ("left", "right", "top", "bottom", "used")
    return c


def block_edge(n_vertices):
    """The first ``n_vertices`` vertices of the analytic case: the last workgroup is full, one lane short or one lane over."""
    c = analytic_sphere(3, 0.3)
    c.vertices, c.normals = c.vertices[:n_vertices].copy(), c.normals[:n_vertices].copy()
    c.reaches = ("used",)
    return c


def null_normals():
    c = analytic_sphere(2, 0.3)
    c.normals = None
    c.reaches = ("see_through", "depth_in_front", "used")
    return c


def null_seen():
    c = analytic_sphere(2, 0.5)
    c.want_seen = False
    return c


COLOR_CASES = {
    "sphere-162-cos0.3": lambda: analytic_sphere(2, 0.3),
    "sphere-162-cos0.5": lambda: analytic_sphere(2, 0.5),
    "sphere-642-cos0.3": lambda: analytic_sphere(3, 0.3),
    "sphere-642-cos0.5": lambda: analytic_sphere(3, 0.5),
    "smooth-images-over-marched-mesh": lambda: over_tsdf_case(
        "synthetic-41x33x29-7views", reaches=("see_through", "depth_in_front", "depth_behind", "facing_away", "used", "unseen")),
    "smooth-images-bright": lambda: over_tsdf_case(
        "synthetic-41x33x29-7views", tol_voxels=3.0, cos_min=0.1, gain=1.6, reaches=("used", "clamped")),
    "views-1": lambda: over_tsdf_case("views-1", reaches=("used",)),
    "views-255": lambda: over_tsdf_case("views-255", reaches=("depth_in_front", "depth_behind", "facing_away", "used")),
    "views-256": lambda: over_tsdf_case("views-256", reaches=("depth_in_front", "depth_behind", "facing_away", "used")),
    "image-1x1": lambda: thin_image(1, 1),
    "image-1x40": lambda: thin_image(1, 40),
    "image-40x1": lambda: thin_image(40, 1),
    "ring-through-grid": lambda: over_tsdf_case(
        "ring-through-grid-fov20", tol_voxels=3.0, reaches=("near", "left", "right", "top", "bottom", "see_through", "used")),
    "depth-nan": lambda: over_tsdf_case("depth-nan", reaches=("depth_nan", "used")),
    "depth-inf": lambda: over_tsdf_case("depth-inf", reaches=("depth_behind", "used")),
    "null-normals": null_normals,
    "null-seen": null_seen,
    "V255": lambda: block_edge(255),
    "V256": lambda: block_edge(256),
    "V257": lambda: block_edge(257),
}


@functools.lru_cache(maxsize=None)
def color_case(name):
    return COLOR_CASES[name]()


@functools.lru_cache(maxsize=None)
def color_reference(name):
    """(colors, seen, census) of the float32 transcription: computed once, shared by the host and the device tests."""
    return AR.colors_f32(*color_case(name).reference_args(), return_census=True)


@functools.lru_cache(maxsize=None)
def normal_case(name):
    return NORMAL_CASES[name][0]()


@functools.lru_cache(maxsize=None)
def normal_reference(name):
    return AR.normals_f32(*normal_case(name), return_census=True)


def check_colors_against_oracle(name, got=None):
    """The float64 oracle against the float32 transcription (or a device result): equal to its tolerance at every vertex
    without a masked pair, the masked share at most 1 % of the (vertex, view) pairs, ``seen`` equal outside the mask."""
    c = color_case(name)
    want, want_seen, _census = color_reference(name)
    colors, seen = (want, want_seen) if got is None else got
    ref, ref_seen, masked, tol = AR.colors_oracle(*c.reference_args())
    share = masked.mean() if masked.size else 0.0
    clean = ~masked.any(axis=1)
    diff = np.abs(colors.astype(np.float64) - ref)
    worst = float((diff[clean] / tol[clean, None]).max()) if clean.any() else 0.0
    print(f"{name}: masked {int(masked.sum())} of {masked.size} pairs ({share:.5f}), worst error / tolerance {worst:.3g}, "
          f"largest tolerance {float(tol.max()):.3g}")
    assert share <= 0.01, share
    if seen is not None:
        np.testing.assert_array_equal(np.asarray(seen)[clean], ref_seen[clean])
    bad = clean[:, None] & ~(diff <= tol[:, None])
    assert not bad.any(), (int(bad.sum()), float(diff[bad].max()))
    return share, worst


def check_sphere(name, colors, seen):
    """Every vertex seen, every colour within 2 * (max row sum of |A|) * slide of the true one: the pixel's footprint carried
    onto the tangent plane, doubled for the curvature.  The far side differs by up to 0.7."""
    c = color_case(name)
    slide = c.extra["slide"]
    bound = 2.0 * np.abs(SPHERE_A).sum(axis=1).max() * slide
    assert c.depth_tol == 2.0 * slide
    assert (seen >= 1).all(), int((seen == 0).sum())
    err = np.abs(colors.astype(np.float64) - sphere_color(c.vertices.astype(np.float64))).max()
    print(f"{name}: seen {int(seen.min())}..{int(seen.max())}, worst colour error {err:.4g}, bound {bound:.4g}")
    assert err <= bound, (err, bound)
    return err, bound
