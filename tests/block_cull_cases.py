"""Seeded fixtures that put 64-Gaussian blocks on the edges of the block-cull bound (pegasus_amd/csrc/blockcull.hip.h).

A block is 64 CONSECUTIVE Gaussians, built on purpose as one compact box.  A *sweep* moves such a box across one deciding
edge of the listing rule in steps of 1/8 px of view 0: a fine window around the place where the exact rule flips
(x + r < 1, x - r >= 16 grid) and a second one around the place where the documented bound says the block test flips;
between them nothing is decided.  C1-C3 sweeps also hold *control* blocks (one point, isotropic, rigid view, FOV <= 60
degrees, further outside than 10 radii + 16 px) that the block test has to cull: tests/test_block_cull_host.py shows on
the CPU that the documented bound demands it, the GPU test asserts it -- so a bound that no longer culls anything fails too.

Everything here is NumPy and float64 until the arrays are rounded to the float32 the kernels get."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

import block_cull_reference as ref
from pegasus_amd import graphics as G, scenes

Z0 = 4.0                          # view-space depth of the sweeps' blocks
STEP = 0.125
SIZES = [(400, 304), (333, 250), (17, 3), (1, 1)]      # 333x250: 16 grid > width and height; 17x3, 1x1: grid of 2x1, 1x1
SHAPES = ["iso", "aniso_in", "aniso_edge", "aniso_ray", "unnorm"]
EDGES = {"x": ("left", "right"), "y": ("top", "bottom")}
# pixel shifts (at depth Z0) of the views of a sweep case against view 0, and a shift along the optical axis: all of them
# keep every block within a pixel or so of where view 0 has it, at other sub-pixel phases
VIEW_SHIFTS = [(0.0, 0.0, 0.0), (0.0625, 0.3, 0.0), (-0.45, 0.2, 0.0), (0.7, -0.9, 0.0), (0.0, 0.0, 0.003)]


@dataclass
class Case:
    name: str
    means: np.ndarray
    views: list
    scales: np.ndarray = None
    rotations: np.ndarray = None
    cov6: np.ndarray = None
    scale_modifier: float = 1.0
    sweeps: dict = field(default_factory=dict)        # label -> block indices (controls included)
    exact: dict = field(default_factory=dict)         # label -> block indices of the window around the exact rule's edge
    controls: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    must_see: list = field(default_factory=list)      # (block, view): listed on purpose -- the bit has to be set
    posed_id: np.ndarray = None                       # int32 [n] object ids of a posed call
    poses: np.ndarray = None                          # float32 [n_views, K, 20]
    list_view: int = 0
    non_vacuous: bool = False                         # every sweep must show a set and a clear bit on the device

    @property
    def n(self):
        return int(self.means.shape[0])

    @property
    def groups(self):
        return (self.n + 63) // 64

    def opacities(self):
        return np.full(self.n, 0.9, np.float32)

    def colors(self):
        return np.random.default_rng(7).uniform(0.1, 1.0, size=(self.n, 3)).astype(np.float32)

    def cov3d(self):
        """float64 [n,3,3] of the float32 parameters the kernels get."""
        if self.cov6 is not None:
            return ref.cov3d_from_packed(self.cov6)
        return ref.cov3d_from_scale_rot(self.scales, self.rotations, np.float32(self.scale_modifier))

    def sig2(self):
        """Per Gaussian, what blockcull.hip.h bounds lambda_max(Sigma) with: the trace, or the Frobenius norm of a given matrix."""
        S = self.cov3d()
        with np.errstate(all="ignore"):
            if self.cov6 is not None:
                return np.sqrt((S * S).sum((1, 2)))
            return np.trace(S, axis1=1, axis2=2)

    def scene_kwargs(self):
        if self.cov6 is not None:
            return dict(cov3d_precomp=self.cov6)
        return dict(scales=self.scales, rotations=self.rotations)


# ------------------------------------------------------------------------------------------ cameras
def camera(M3, t, W, H, fovx, fovy):
    """A view whose world-to-view matrix is [[M3, t], [0, 1]] (M3 need not be a rotation); the projection is composed
    from that same matrix, as the callers do."""
    M3, t = np.asarray(M3, np.float64), np.asarray(t, np.float64)
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = M3, t
    wvt = w2c.T.astype(np.float32)
    proj = G.getProjectionMatrix(G.ZNEAR, G.ZFAR, fovx, fovy).T
    full = (wvt @ proj).astype(np.float32)
    v = scenes.View(W, H, fovx, fovy, np.linalg.inv(M3), t, wvt, full, np.linalg.inv(w2c)[:3, 3].astype(np.float32))
    v.M3, v.t = M3, t
    return v


def square_pixel_fov(W, H, fov_wide):
    """(fovx, fovy) with the wider side at ``fov_wide`` and square pixels."""
    tw = math.tan(0.5 * fov_wide)
    if W >= H:
        return fov_wide, 2.0 * math.atan(tw * H / W)
    return 2.0 * math.atan(tw * W / H), fov_wide


def shifted_views(M3, W, H, fovx, fovy, shifts=VIEW_SHIFTS, t0=(0.0, 0.0, 0.0)):
    fx, fy = W / (2 * math.tan(fovx / 2)), H / (2 * math.tan(fovy / 2))
    return [camera(M3, np.asarray(t0) + [sx * Z0 / fx, sy * Z0 / fy, sz], W, H, fovx, fovy) for sx, sy, sz in shifts]


def view_to_world(view, p_view):
    return (np.asarray(p_view, np.float64) - view.t) @ np.linalg.inv(view.M3).T


def place(view, pix_x, pix_y, z):
    """View-space point at depth z whose pixel centre is (pix_x, pix_y)."""
    W, H = view.width, view.height
    return np.array([z * view.tanfovx * ((2 * pix_x + 1) / W - 1), z * view.tanfovy * ((2 * pix_y + 1) / H - 1), z])


# ------------------------------------------------------------------------------------------ Gaussian shapes
def _quat_with_first_axis(d):
    """(w, x, y, z) of a rotation whose first column is the unit vector d."""
    from scipy.spatial.transform import Rotation as Rot
    d = d / np.linalg.norm(d)
    helper = np.eye(3)[int(np.argmin(np.abs(d)))]
    e2 = np.cross(d, helper)
    e2 /= np.linalg.norm(e2)
    x, y, z, w = Rot.from_matrix(np.stack([d, e2, np.cross(d, e2)], 1)).as_quat()
    return np.array([w, x, y, z])


UNNORM_Q = 37.0 * np.array([0.5, 0.5, -0.5, 0.5])


def shape_params(kind, view, p_view, axis):
    """(scales[3], quaternion[4]) of shape ``kind`` for a Gaussian at view-space p_view in a sweep along image axis ``axis``.
    iso: 1.7 px sigma.  aniso_*: 1000:1, long sigma 40 px at the image centre (aniso_corner: 5.3 px); long axis
      aniso_in   along the right singular vector of the (clamped) projection Jacobian's row of the sweep's axis -- the
                 direction that reaches furthest INTO the image, and the one for which |J|^2 lambda_max is attained,
      aniso_edge along the other image axis (parallel to the edge),
      aniso_ray  along the view ray,
      aniso_corner  (swept along one image axis at a place beyond the 1.3 tanfov clamp of BOTH axes, on a square image)
                 along the top right singular vector of the whole clamped Jacobian: with fx = fy and both clamps active
                 lambda_max(J J^T) = max(a, b) + |c| exactly, so the documented bound is attained up to its 1.02, 1.001, + 2
                 and + 0.92 paddings -- the tightest block this file knows how to build.
    unnorm: a quaternion of norm 37 (the matrix built from it is no rotation: its entries are in the thousands)."""
    f = (view.width / (2 * view.tanfovx), view.height / (2 * view.tanfovy))
    a, o = (0, 1) if axis == "x" else (1, 0)
    if kind == "iso":
        return np.full(3, 1.7 * Z0 / f[a]), np.array([1.0, 0, 0, 0])
    if kind == "unnorm":
        return 1.7 * Z0 / f[a] / 2737.0 * np.array([1.0, 0.5, 0.25]), UNNORM_Q
    lim = (1.3 * view.tanfovx, 1.3 * view.tanfovy)
    tc = [float(np.clip(p_view[k] / p_view[2], -lim[k], lim[k])) for k in (0, 1)]
    d = np.zeros(3)
    if kind == "aniso_corner":
        J = np.array([[f[0] / p_view[2], 0.0, -f[0] * tc[0] / p_view[2]], [0.0, f[1] / p_view[2], -f[1] * tc[1] / p_view[2]]])
        d = np.linalg.svd(J)[2][0]
    elif kind == "aniso_in":
        d[a], d[2] = 1.0, -tc[a]
    elif kind == "aniso_edge":
        d[o], d[2] = 1.0, -tc[o]
    else:
        d = np.asarray(p_view, np.float64).copy()
    L = (5.3 if kind == "aniso_corner" else 40.0) * Z0 / f[a]      # (corner: radius 24 px, so that the paddings that scale with it stay small)
    return np.array([L, L / 1000, L / 1000]), _quat_with_first_axis(np.linalg.inv(view.M3) @ d)


def cov_variant(mode, scales, quat):
    """float64 3x3 for the cov3d_precomp cases: the shape's own matrix (psd), an indefinite and a negative-definite
    relative, and one with a single huge off-diagonal entry."""
    M = ref.rotation_from_quaternion(quat[None])[0] * scales[None, :]
    S = M @ M.T
    if mode == "indef":
        S = M @ np.diag([1.0, -1.0, 1.0]) @ M.T
    elif mode == "negdef":
        S = -S
    elif mode in ("huge18", "huge20"):
        S = S.copy()
        S[0, 1] = S[1, 0] = 1e18 if mode == "huge18" else 1e20
    return S


# ------------------------------------------------------------------------------------------ sweeps
class _Builder:
    def __init__(self, views, seed, scale_modifier=1.0, cov_mode=None):
        self.views, self.mod, self.cov_mode = views, scale_modifier, cov_mode
        self.rng = np.random.default_rng(seed)
        self.means, self.scales, self.rots, self.covs = [], [], [], []
        f = min(views[0].width / (2 * views[0].tanfovx), views[0].height / (2 * views[0].tanfovy))
        self.jitter = 0.05 * Z0 / f          # half-size of a block's box: 0.05 px at depth Z0

    @property
    def blocks(self):
        return len(self.means)

    def gaussian(self, scales, quat, plain=False):
        if self.cov_mode is None:
            return ref.cov3d_from_scale_rot(np.float32(scales)[None], np.float32(quat)[None], np.float32(self.mod))[0]
        mode = "psd" if plain else self.cov_mode
        return ref.cov3d_from_packed(ref.pack_cov3d(cov_variant(mode, scales, quat)[None]).astype(np.float32))[0]

    def add_block(self, p_view, scales, quat, jitter=None, members=64, plain=False):
        """One block: 64 Gaussians of one shape in a box of half-size ``jitter`` (view space) around p_view; the first sits
        on p_view itself.  ``plain``: its own matrix even in a case of indefinite or huge ones.  Returns the block index."""
        j = self.jitter if jitter is None else jitter
        pts = np.asarray(p_view, np.float64) + self.rng.uniform(-j, j, size=(members, 3))
        pts[0] = p_view
        self.means.append(view_to_world(self.views[0], pts))
        self.scales.append(np.tile(scales, (members, 1)))
        self.rots.append(np.tile(quat, (members, 1)))
        if self.cov_mode is not None:
            mode = "psd" if plain else self.cov_mode
            self.covs.append(np.tile(ref.pack_cov3d(cov_variant(mode, np.asarray(scales), np.asarray(quat))[None]), (members, 1)))
        return self.blocks - 1

    def one(self, p_view, scales, quat, plain=False):
        """float64 listing of a single Gaussian at p_view in view 0 (used to aim the windows)."""
        r = ref.listing(view_to_world(self.views[0], np.asarray(p_view)[None]), self.gaussian(scales, quat, plain)[None],
                        self.views[0])
        return {k: v[0] for k, v in r.items()}

    def sig2_of(self, scales, quat):
        S = self.gaussian(scales, quat)
        with np.errstate(all="ignore"):
            return float(np.sqrt((S * S).sum())) if self.cov_mode is not None else float(np.trace(S))

    def edge_sweep(self, kind, edge, controls=True):
        """Blocks across ``edge`` of view 0.  Returns (all block indices, the exact window's, the controls')."""
        v = self.views[0]
        axis = "x" if edge in ("left", "right") else "y"
        low = edge in ("left", "top")
        g16 = 16 * (((v.width if axis == "x" else v.height) + 15) // 16)
        mid = ((v.width - 1) / 2, (v.height - 1) / 2)
        if kind == "aniso_corner":           # beyond the clamp of the other axis as well (ndc = -1.36)
            mid = (-0.18 * v.width, -0.18 * v.height)
        sign = -1.0 if low else 1.0          # outward

        def at(c):                           # view-space point with the swept coordinate at pixel c
            return place(v, c, mid[1], Z0) if axis == "x" else place(v, mid[0], c, Z0)

        def edge_of(r):                      # pixel coordinate at which a Gaussian of radius r stops being listed
            return 1.0 - r if low else g16 + r

        c, r = edge_of(3.0), 3.0
        for _ in range(4):                   # the radius depends (weakly) on the place: aim at the fixed point
            s, q = shape_params(kind, v, at(c), axis)
            r = self.one(at(c), s, q)["radius"]
            if not (np.isfinite(r) and r < 1e6):
                r = 0.0                      # no radius in float64 (indefinite matrix): the fp32 code lists it with radius 0
            c = edge_of(r)
        offsets = [c + k * STEP for k in range(-8, 9)]
        n_exact = len(offsets)
        with np.errstate(all="ignore"):
            rmax = float(ref.documented_rmax(self.sig2_of(s, q), v, Z0 - self.jitter))
        if np.isfinite(rmax) and rmax < 1e8:
            cb = edge_of(rmax + 1.0 + 1e-4 * abs(edge_of(rmax)))
            offsets += [cb + k * STEP for k in range(-12, 13)]
        blocks = []
        for cpix in offsets:
            s, q = shape_params(kind, v, at(cpix), axis)
            blocks.append(self.add_block(at(cpix), s, q))
        ctrl = []
        if controls:
            fa = (v.width / (2 * v.tanfovx)) if axis == "x" else (v.height / (2 * v.tanfovy))
            cs, cq = np.full(3, 0.5 * Z0 / fa), np.array([1.0, 0, 0, 0])
            for extra in (24.0, 60.0):
                rc, cc = 3.0, 0.0
                for _ in range(4):
                    cc = edge_of(0.0) + sign * (10.0 * rc + 16.0 + extra)
                    rc = self.one(at(cc), cs, cq, plain=True)["radius"]
                ctrl.append(self.add_block(at(cc), cs, cq, jitter=0.0, plain=True))
        return np.array(blocks + ctrl), np.array(blocks[:n_exact]), np.array(ctrl)

    def finish(self, name, **kw):
        f32 = lambda parts: np.concatenate(parts).astype(np.float32)
        case = Case(name, f32(self.means), self.views, scale_modifier=self.mod, **kw)
        if self.cov_mode is not None:
            with np.errstate(over="ignore"):
                case.cov6 = f32(self.covs)
        else:
            case.scales, case.rotations = f32(self.scales), f32(self.rots)
        return case


def sweep_views(W, H):
    fovx, fovy = square_pixel_fov(W, H, math.radians(60.0))
    return shifted_views(np.eye(3), W, H, fovx, fovy)


def sweep_case(name, views, kind, axis, scale_modifier=1.0, cov_mode=None, controls=True, seed=0):
    b = _Builder(views, seed, scale_modifier, cov_mode)
    sweeps, exact, ctrl = {}, {}, []
    for edge in EDGES[axis]:
        blocks, ex, c = b.edge_sweep(kind, edge, controls)
        sweeps[edge], exact[edge] = blocks, ex
        ctrl += list(c)
    return b.finish(name, sweeps=sweeps, exact=exact, controls=np.array(ctrl, np.int64), non_vacuous=controls)


# ------------------------------------------------------------------------------------------ the case table
def _c1(size, kind, axis):
    return lambda: sweep_case(f"c1-{size[0]}x{size[1]}-{kind}-{axis}", sweep_views(*size), kind, axis, seed=11)


def _c2(size, kind, mode, axis):
    return lambda: sweep_case(f"c2-{size[0]}x{size[1]}-{kind}-{mode}-{axis}", sweep_views(*size), kind, axis, cov_mode=mode, seed=12)


def _c3(size, kind, mod, axis):
    return lambda: sweep_case(f"c3-{size[0]}x{size[1]}-{kind}-x{mod}-{axis}", sweep_views(*size), kind, axis,
                              scale_modifier=mod, seed=13)


def _near_plane():
    """C4: boxes that end just below, at and just above z = 0.2 (in ulps of 0.2f and in steps of the block test's own
    1e-6-scale z margin), boxes across it, and boxes just in front of it far off-axis: |x/z| = 1.2 .. 5 tanfov with 1 m
    scales, so the clamp is active, the centre is far outside, the radius is thousands of pixels -- and the block is listed."""
    W, H = 400, 304
    fovx, fovy = square_pixel_fov(W, H, math.radians(60.0))
    shifts = [(0, 0, 0), (0.3, -0.2, 0), (0, 0, 2e-6), (0, 0, -2e-6), (0, 0, 3e-8)]
    views = [camera(np.eye(3), [sx * 0.2 / 346.0, sy * 0.2 / 346.0, sz], W, H, fovx, fovy) for sx, sy, sz in shifts]
    b = _Builder(views, 14)
    near = np.float32(0.2)
    ulp = float(np.spacing(near))
    tops = [float(near) + k * ulp for k in (-16, -2, -1, 0, 1, 2, 16)] + [float(near) + k * 1e-6 for k in range(-8, 9)]
    small, big, ident = np.full(3, 0.001), np.full(3, 1.0), np.array([1.0, 0, 0, 0])
    rng = np.random.default_rng(15)
    must_see = []

    def box(zlo, zhi, xz, scales):
        pts = np.stack([np.zeros(64), rng.uniform(-0.01, 0.01, 64), rng.uniform(zlo, zhi, 64)], 1)
        pts[0, 2], pts[1, 2] = zhi, zlo
        pts[:, 0] = xz * views[0].tanfovx * pts[:, 2] + rng.uniform(-0.001, 0.001, 64)
        b.means.append(view_to_world(views[0], pts))
        b.scales.append(np.tile(scales, (64, 1)))
        b.rots.append(np.tile(ident, (64, 1)))
        return b.blocks - 1

    for top in tops:                                   # ends below / at / above the plane
        box(0.1, top, 0.0, small)
        box(0.1, top, 1.4, big)
    for lo, hi in ((0.1, 0.3), (0.19999, 0.20001), (-5.0, 0.2001)):      # across it
        box(lo, hi, 0.0, small)
        box(lo, hi, 5.0, big)
    for xz in (0.0, 1.2, 1.3, 1.4, 5.0, -1.2, -1.3, -1.4, -5.0):          # just in front of it
        for zlo in [float(near) + k * ulp for k in (1, 2, 16)] + [float(near) + k * 1e-6 for k in (1, 3, 8)]:
            blk = box(zlo, zlo + 1e-3, xz, big)
            must_see.append((blk, 0))
    return b.finish("c4-near-plane", must_see=must_see)


def _rot(axis_angle):
    from scipy.spatial.transform import Rotation as Rot
    return Rot.from_rotvec(axis_angle).as_matrix()


CAMERAS = {      # C5: name -> (M3, fovx, fovy in degrees; None = square pixels from the wide side)
    "fov100x35": (np.eye(3), 100.0, 35.0),
    "fov20x90": (np.eye(3), 20.0, 90.0),
    "fov150": (np.eye(3), 150.0, None),
    "half": (0.5 * _rot([0.2, -0.3, 0.1]), 60.0, None),
    "triple": (3.0 * _rot([-0.1, 0.25, 0.4]), 60.0, None),
    "diag": (np.diag([1.0, 2.0, 0.5]) @ _rot([0.3, 0.1, -0.2]), 60.0, None),
}


def _c5(cam, kind, axis):
    def build():
        M3, fx, fy = CAMERAS[cam]
        W, H = 400, 304
        fovx, fovy = (math.radians(fx), math.radians(fy)) if fy else square_pixel_fov(W, H, math.radians(fx))
        views = shifted_views(M3, W, H, fovx, fovy, t0=(0.1, -0.2, 0.3))
        return sweep_case(f"c5-{cam}-{kind}-{axis}", views, kind, axis, controls=False, seed=16)
    return build


def _cloud():
    """C5: cameras of every kind above inside a cloud of compact blocks, several of them looking away from most of it."""
    rng = np.random.default_rng(17)
    W, H = 333, 250
    views = []
    for M3, fx, fy in CAMERAS.values():
        fovx, fovy = (math.radians(fx), math.radians(fy)) if fy else square_pixel_fov(W, H, math.radians(fx))
        for away in (False, True):
            eye = rng.uniform(-1.5, 1.5, size=3)
            Rw = _rot(rng.normal(0, 2.0, size=3))
            if away:                              # look along the direction from the cloud's centre through the eye
                Rl, _ = G.look_at_opencv(tuple(eye), tuple(3.0 * eye), up=(0.0, -1.0, 0.1))
                Rw = Rl
            M = M3 @ Rw
            views.append(camera(M, -M @ eye, W, H, fovx, fovy))
    b = _Builder(views, 18)
    n_blocks = 96
    means, scales, rots = [], [], []
    for k in range(n_blocks):
        c = rng.uniform(-3.0, 3.0, size=3)
        m = 1 if k == n_blocks - 1 else 64         # 64 k + 1 Gaussians: the last block has one real lane
        means.append(c + rng.uniform(-0.03, 0.03, size=(m, 3)))
        scales.append(np.exp(rng.normal(math.log(0.02), 0.7, size=(m, 3))))
        q = rng.normal(size=(m, 4))
        rots.append(q / np.linalg.norm(q, axis=1, keepdims=True))
    b.means, b.scales, b.rots = means, scales, rots
    return b.finish("c5-cloud", list_view=3)


def _sizes(n):
    """C6: a C1 sweep cut to n Gaussians (1, 63, 64, 65) or extended to 64 k + 1 by one copy of a control Gaussian."""
    def build():
        base = sweep_case("base", sweep_views(400, 304), "iso", "x", seed=11)
        if n > 0:
            keep = n
        else:
            keep = base.n + 1
        idx = np.arange(keep)
        idx[idx >= base.n] = int(base.controls[0]) * 64
        case = Case(f"c6-n{keep}", base.means[idx], base.views, scales=base.scales[idx], rotations=base.rotations[idx])
        if n <= 0:
            case.sweeps, case.exact, case.controls = base.sweeps, base.exact, np.append(base.controls, base.groups)
            case.sweeps = {k: np.append(v, base.groups) if k == "left" else v for k, v in case.sweeps.items()}
            case.non_vacuous = True
        return case
    return build


def _make_up():
    """C6: blocks that would be culled where they are, each with ONE odd member -- 50 m away (in the middle of the image, and
    off to the side), a NaN or an infinite coordinate, a zero scale -- and plain ones between them."""
    views = sweep_views(400, 304)
    b = _Builder(views, 19)
    v = views[0]
    s, q = np.full(3, 1.7 * Z0 / (v.width / (2 * v.tanfovx))), np.array([1.0, 0, 0, 0])
    must_see = []
    kinds = ["plain", "far_visible", "far_side", "nan", "inf", "neg_inf", "zero_scale", "zero_scales", "plain"]
    for k, kind in enumerate(kinds):
        blk = b.add_block(place(v, -150.0 - 3 * k, 150.0, Z0), s, q)
        m = 17 + k
        if kind == "far_visible":
            b.means[blk][m] = view_to_world(v, place(v, 200.0, 150.0, Z0 + 50.0))
            must_see += [(blk, vi) for vi in range(len(views))]
        elif kind == "far_side":
            b.means[blk][m] = view_to_world(v, place(v, -150.0, 150.0, Z0) + [-50.0, 0, 0])
        elif kind == "nan":
            b.means[blk][m, 1] = np.nan
        elif kind == "inf":
            b.means[blk][m, 0] = np.inf
        elif kind == "neg_inf":
            b.means[blk][m, 2] = -np.inf
        elif kind == "zero_scale":
            b.scales[blk][m, 2] = 0.0
        elif kind == "zero_scales":
            b.scales[blk][m] = 0.0
    case = b.finish("c6-make-up", must_see=must_see)
    case.controls = np.array([0, len(kinds) - 1])          # the plain blocks: culled, or the fixture is not where it says
    return case


def _posed():
    """C6: a posed call.  Block 1 belongs to object 1 and rests where a control block would be; the poses move it into the
    image in some views.  A posed object's block is never culled, whatever its rest box says."""
    from pegasus_amd.compose import pose_table
    views = sweep_views(400, 304)
    b = _Builder(views, 20)
    v = views[0]
    s, q = np.full(3, 1.7 * Z0 / (v.width / (2 * v.tanfovx))), np.array([1.0, 0, 0, 0])
    for k in range(4):
        b.add_block(place(v, -150.0 - 40 * k, 150.0, Z0), s, q)
    b.add_block(place(v, 200.0, 150.0, Z0), s, q)
    case = b.finish("c6-posed")
    oid = np.zeros(case.n, np.int32)
    oid[64:128] = 1
    centre = case.means[64:128].astype(np.float64).mean(0)
    poses = np.zeros((len(views), 1, 20), np.float32)
    for i in range(len(views)):
        T = np.eye(4)
        T[:3, :3] = _rot([0.0, 0.0, 0.3 * i])
        T[:3, 3] = view_to_world(v, place(v, 60.0 + 70.0 * i, 100.0, Z0)) - centre if i % 2 == 0 else [0.0, 0.0, 0.0]
        poses[i] = pose_table([(T, centre)])
    case.posed_id, case.poses = oid, poses
    case.controls = np.array([0, 2, 3])
    case.must_see = [(1, i) for i in range(0, len(views), 2)]      # (the other views leave it at rest: bit set all the same)
    return case


def _table():
    t = {}
    for size in SIZES:
        for axis in ("x", "y"):
            for kind in SHAPES:
                t[f"c1-{size[0]}x{size[1]}-{kind}-{axis}"] = _c1(size, kind, axis)
                t[f"c2-{size[0]}x{size[1]}-{kind}-psd-{axis}"] = _c2(size, kind, "psd", axis)
            for kind, mode in (("iso", "indef"), ("iso", "negdef"), ("aniso_in", "indef"), ("aniso_in", "huge18"), ("aniso_in", "huge20")):
                t[f"c2-{size[0]}x{size[1]}-{kind}-{mode}-{axis}"] = _c2(size, kind, mode, axis)
            for kind in SHAPES[:4]:
                for mod in (0.25, 4.0):          # (modifier 1 is C1 itself)
                    t[f"c3-{size[0]}x{size[1]}-{kind}-x{mod}-{axis}"] = _c3(size, kind, mod, axis)
    for axis in ("x", "y"):
        t[f"c1-96x96-aniso_corner-{axis}"] = _c1((96, 96), "aniso_corner", axis)
        t[f"c2-96x96-aniso_corner-psd-{axis}"] = _c2((96, 96), "aniso_corner", "psd", axis)
        t[f"c3-96x96-aniso_corner-x4.0-{axis}"] = _c3((96, 96), "aniso_corner", 4.0, axis)
    t["c4-near-plane"] = _near_plane
    for cam in CAMERAS:
        for kind, axis in (("iso", "x"), ("aniso_in", "x"), ("aniso_in", "y")):
            t[f"c5-{cam}-{kind}-{axis}"] = _c5(cam, kind, axis)
    t["c5-cloud"] = _cloud
    for n in (1, 63, 64, 65, 0):
        t[f"c6-n{n if n else '64k+1'}"] = _sizes(n)
    t["c6-make-up"] = _make_up
    t["c6-posed"] = _posed
    return t


TABLE = _table()
NAMES = list(TABLE)


@functools.lru_cache(maxsize=8)
def get(name) -> Case:
    return TABLE[name]()


# ------------------------------------------------------------------------------------------ checks shared by host and GPU tests
def blocks_any(flag, n):
    """bool [n] per Gaussian -> bool [groups]: does any Gaussian of the block carry the flag."""
    pad = (-n) % 64
    return np.pad(np.asarray(flag, bool), (0, pad)).reshape(-1, 64).any(1)


def blocks_min(value, n, fill=np.inf):
    pad = (-n) % 64
    return np.pad(np.asarray(value, np.float64), (0, pad), constant_values=fill).reshape(-1, 64).min(1)


def reference_listing(case: Case):
    """Per view: block_cull_reference.listing of the case's float32 arrays (posed cases: not available -> None)."""
    if case.posed_id is not None:
        return None
    S = case.cov3d()
    return [ref.listing(case.means, S, v) for v in case.views]


def oracle_radii(case: Case, oracle):
    """Per view: the C oracle's radii (no HIP code involved)."""
    out = []
    kw = case.scene_kwargs()
    for i, v in enumerate(case.views):
        extra = {}
        if case.posed_id is not None:
            extra = dict(object_id=case.posed_id, poses=case.poses[i])
        out.append(oracle.forward(case.means, case.opacities(), colors_precomp=case.colors(), scale_modifier=case.scale_modifier,
                                  stage="preprocess", num_threads=4, **kw, **extra, **v.raster_kwargs())["radii"])
    return out
