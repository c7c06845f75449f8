"""float64 NumPy restatement of the per-Gaussian LISTING rule of pegasus_amd/csrc/preprocess.hip.h: is Gaussian i listed in
a view (non-zero radius, non-empty tile rectangle), and how far is that decision from flipping.  It is the third,
HIP-free and C-free radius source the block-cull tests hold the visibility bits against; it is NOT a restatement of the
block test (blockcull.hip.h).  Only `documented_rmax` restates something of that file: the radius bound its comment
derives, which the host test uses to show that the control blocks of a fixture must be culled.

Matrices are the row-vector 4x4 arrays the rasterizer surface takes (View.world_view_transform, .full_proj_transform):
t = [p, 1] @ M, which is the kernels' vm[4 c + r] = M[c][r] indexing."""
import numpy as np

NEAR_Z = 0.2
LOWPASS = 0.3
TILE = 16


def rotation_from_quaternion(q):
    """[n,4] (w,x,y,z), NOT normalised by the kernels either -> [n,3,3] exactly as cov3d_from_scale_rot builds it."""
    q = np.asarray(q, np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def cov3d_from_scale_rot(scales, rotations, scale_modifier=1.0):
    """[n,3,3] Sigma = (R S)(R S)^T with S = diag(modifier * scales)."""
    M = rotation_from_quaternion(rotations) * (float(scale_modifier) * np.asarray(scales, np.float64))[:, None, :]
    return M @ M.transpose(0, 2, 1)


def cov3d_from_packed(c6):
    """[n,6] (xx, xy, xz, yy, yz, zz) as cov3d_precomp stores it -> [n,3,3]."""
    c = np.asarray(c6, np.float64)
    return np.stack([np.stack([c[:, 0], c[:, 1], c[:, 2]], 1), np.stack([c[:, 1], c[:, 3], c[:, 4]], 1),
                     np.stack([c[:, 2], c[:, 4], c[:, 5]], 1)], 1)


def pack_cov3d(S):
    S = np.asarray(S)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


def listing(means, cov3d, view):
    """The listing rule for every Gaussian in one view.  Returns a dict of [n] arrays:
    z            view-space depth
    pix_x, pix_y pixel centre;  radius  ceil(3 sqrt(lambda1)) as a float (NaN where the rule has no number)
    listed       the decision: z > 0.2, det != 0, non-empty tile rectangle
    margin       pixels by which `listed` is away from flipping: for a listed Gaussian the smallest distance of pix +- radius
                 from the four deciding edges (x + r >= 1, x - r < 16 grid_x, same in y); for an unlisted one in front of the
                 near plane the LARGEST violation (every violated edge has to flip).  One pixel is taken off where
                 3 sqrt(lambda1) is within 1e-3 of an integer (the ceil may round the other way in fp32).  0 where the rule
                 yields no number in float64 (non-finite input, lambda1 <= 0, |det| tiny): no claim there.  +inf for z <= 0.2
                 (only z_margin counts).
    z_margin     |z - 0.2|"""
    means = np.asarray(means, np.float64)
    V = np.asarray(view.world_view_transform, np.float64)
    P = np.asarray(view.full_proj_transform, np.float64)
    W, H = int(view.width), int(view.height)
    tanx, tany = float(np.float32(view.tanfovx)), float(np.float32(view.tanfovy))
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    n = means.shape[0]
    with np.errstate(all="ignore"):
        hom = np.concatenate([means, np.ones((n, 1))], 1)
        t = hom @ V
        h = hom @ P
        z = t[:, 2]
        front = z > NEAR_Z
        zs = np.where(front, z, 1.0)
        p_w = 1.0 / (h[:, 3] + 0.0000001)
        pix_x = ((h[:, 0] * p_w + 1.0) * W - 1.0) * 0.5
        pix_y = ((h[:, 1] * p_w + 1.0) * H - 1.0) * 0.5
        tx = np.clip(t[:, 0] / zs, -1.3 * tanx, 1.3 * tanx) * zs
        ty = np.clip(t[:, 1] / zs, -1.3 * tany, 1.3 * tany) * zs
        J = np.zeros((n, 2, 3))
        J[:, 0, 0] = fx / zs; J[:, 0, 2] = -(fx * tx) / (zs * zs)
        J[:, 1, 1] = fy / zs; J[:, 1, 2] = -(fy * ty) / (zs * zs)
        Wm = V[:3, :3].T                       # W[r][c] = vm[4 c + r]
        T = J @ Wm                             # [n,2,3]
        cov2d = T @ np.asarray(cov3d, np.float64) @ T.transpose(0, 2, 1)
        a, b, c = cov2d[:, 0, 0] + LOWPASS, cov2d[:, 0, 1], cov2d[:, 1, 1] + LOWPASS
        det = a * c - b * b
        mid = 0.5 * (a + c)
        lam = mid + np.sqrt(np.maximum(0.1, mid * mid - det))
        r3 = 3.0 * np.sqrt(lam)
        radius = np.ceil(r3)
        edges = np.stack([pix_x + radius - 1.0, TILE * gx - (pix_x - radius),        # >= 0 / > 0: not empty on that side
                          pix_y + radius - 1.0, TILE * gy - (pix_y - radius)], 1)
        inside = edges >= 0
        inside[:, 1] = edges[:, 1] > 0
        inside[:, 3] = edges[:, 3] > 0
        defined = np.isfinite(edges).all(1) & np.isfinite(r3) & (lam > 0) & (np.abs(det) > 1e-9 * np.maximum(1.0, mid * mid))
        listed = front & defined & inside.all(1) & (det != 0)
        dist = np.abs(edges)
        margin = np.where(inside.all(1), dist.min(1), np.where(inside, 0.0, dist).max(1))
        margin = np.where(np.abs(r3 - np.round(r3)) < 1e-3, margin - 1.0, margin)
        margin = np.where(defined, np.maximum(margin, 0.0), 0.0)
        margin = np.where(front, margin, np.inf)
        margin = np.where(np.isfinite(z), margin, 0.0)
        radius = np.where(front & defined, radius, np.nan)
    return dict(z=z, pix_x=pix_x, pix_y=pix_y, radius=radius, listed=listed, margin=margin, z_margin=np.abs(z - NEAR_Z))


def claims(ref, px=0.5, dz=1e-4):
    """Where the restatement's decision binds fp32 code: margin above ``px`` pixels and z more than ``dz`` from 0.2."""
    with np.errstate(invalid="ignore"):
        return (ref["margin"] > px) & (ref["z_margin"] > dz)


def documented_rmax(sig2, view, zmin):
    """The radius bound blockcull.hip.h documents above its arithmetic, in float64:
        r <= 3 sqrt(lambda_max(cov2D) + 0.32) 1.001 + 2 rounded up as the kernel does (1.02 sig2 wn jn + 0.92 under the root),
        lambda_max(cov2D) <= |J|^2 |W|^2 sig2 + 0.3,  |W|^2 <= largest absolute row sum of W^T W,
        |J|^2 <= (max(fx^2 (1 + lx^2), fy^2 (1 + ly^2)) + fx fy lx ly) / zmin^2,  lx = 1.3 tanfovx, ly = 1.3 tanfovy."""
    V = np.asarray(view.world_view_transform, np.float64)
    Wm = V[:3, :3].T
    wn = np.abs(Wm.T @ Wm).sum(1).max()
    W, H = int(view.width), int(view.height)
    tanx, tany = float(view.tanfovx), float(view.tanfovy)
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    lx, ly = 1.3 * tanx, 1.3 * tany
    jn = (max(fx * fx * (1 + lx * lx), fy * fy * (1 + ly * ly)) + fx * fy * lx * ly) / (np.asarray(zmin, np.float64) ** 2)
    return 3.0 * np.sqrt(1.02 * np.asarray(sig2, np.float64) * wn * jn + 0.92) * 1.001 + 2.0


def outside_distance(ref, view):
    """How far a pixel centre lies outside the rule's image box [1, 16 grid) in pixels (<= 0: not outside): the radius a
    Gaussian there would need to be listed."""
    gx, gy = (int(view.width) + TILE - 1) // TILE, (int(view.height) + TILE - 1) // TILE
    x, y = ref["pix_x"], ref["pix_y"]
    return np.maximum.reduce([1.0 - x, x - TILE * gx, 1.0 - y, y - TILE * gy])
