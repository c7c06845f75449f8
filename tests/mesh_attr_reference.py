"""NumPy references of the vertex-attribute kernels (pegasus_amd/csrc/meshattr.hip.h), written from the contract in
include/pegasus_raster.h and sharing nothing with the package.

normals_f32 and colors_f32 are transcriptions: the same float32 (and, for the normals' last step, float64) operations in
the same order, so the GPU tests compare with them bit for bit.  colors_oracle is the second, independent reference of
the colour rule: float64 throughout, with every (vertex, view) pair marked where a float32 rounding may decide
otherwise than float64 does."""
from __future__ import annotations

import numpy as np

f32 = np.float32
NEAR_Z = f32(0.2)
SCALE = f32(2.0 ** 30)
U = 2.0 ** -24                                # the unit roundoff of float32

NORMAL_CENSUS = ("faces", "out_of_range", "degenerate", "used", "isolated")
COLOR_CENSUS = ("pairs", "near", "left", "right", "top", "bottom", "see_through", "depth_in_front", "depth_behind", "depth_nan",
                "facing_away", "used", "vertices", "unseen", "clamped")


# ---- normals --------------------------------------------------------------------------------------------------------
def normal_sums(vertices, faces):
    """(int64 sums [V,3], census) of the accumulate pass."""
    v = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    sums = np.zeros((V, 3), np.int64)
    in_range = ((f >= 0) & (f < V)).all(axis=1) if len(f) else np.zeros(0, bool)
    census = dict(faces=len(f), out_of_range=int((~in_range).sum()), degenerate=0, used=0)
    f = f[in_range]
    if len(f):
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        e1, e2 = (b - a).astype(f32), (c - a).astype(f32)
        m = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(f32)
        with np.errstate(over="ignore", invalid="ignore"):
            length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]).astype(f32)
        ok = (length > 0) & np.isfinite(length)
        census["degenerate"] = int((~ok).sum())
        census["used"] = int(ok.sum())
        m, length, f = m[ok], length[ok], f[ok]
        u = (m / length[:, None]).astype(f32)
        q = np.rint((u * SCALE).astype(f32)).astype(np.int64)
        for corner in range(3):
            np.add.at(sums, f[:, corner], q)
    census["isolated"] = int((sums == 0).all(axis=1).sum())
    return sums, census


def normals_f32(vertices, faces, return_census=False):
    """float32 [V,3] of pgr_mesh_vertex_normals."""
    sums, census = normal_sums(vertices, faces)
    s = sums.astype(np.float64)
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    out = np.divide(s, length[:, None], out=np.zeros_like(s), where=length[:, None] > 0).astype(f32)
    return (out, census) if return_census else out


# ---- colours: the float32 transcription -----------------------------------------------------------------------------
def colors_f32(vertices, normals, viewmats, tanfovx, tanfovy, campos, color, depth, final_T, depth_tol, alpha_min=0.5,
               cos_min=0.3, fill=(0.5, 0.5, 0.5), return_census=False):
    """(colors float32 [V,3], seen int32 [V]) of pgr_mesh_vertex_colors.  viewmats [n,16] (world_view_transform, transposed
    storage), campos [n,3], color [n,3,H,W], depth / final_T [n,H,W]; normals [V,3] or None."""
    p = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    n_views, H, W = depth.shape
    color = np.asarray(color, f32).reshape(n_views, 3, H, W)
    tol, amin, cmin = f32(depth_tol), f32(alpha_min), f32(cos_min)
    cx, cy = f32(W - 1) * f32(0.5), f32(H - 1) * f32(0.5)
    V = len(p)
    acc = np.zeros((V, 3), f32)
    wsum = np.zeros(V, f32)
    seen = np.zeros(V, np.int32)
    census = dict.fromkeys(COLOR_CENSUS, 0)
    census["pairs"], census["vertices"] = V * n_views, V
    campos = np.asarray(campos, f32).reshape(n_views, 3)
    if normals is not None:
        nrm = np.ascontiguousarray(normals, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for k in range(n_views):
            m = np.asarray(viewmats[k], f32).reshape(16)
            x = m[0] * px + m[4] * py + m[8] * pz + m[12]
            y = m[1] * px + m[5] * py + m[9] * pz + m[13]
            z = m[2] * px + m[6] * py + m[10] * pz + m[14]
            front = ~(z <= NEAR_Z)                               # (a NaN z walks on and fails the image test)
            fx = f32(W / (2.0 * float(f32(tanfovx[k]))))
            fy = f32(H / (2.0 * float(f32(tanfovy[k]))))
            u = ((x / z).astype(f32) * fx).astype(f32) + cx
            vv = ((y / z).astype(f32) * fy).astype(f32) + cy
            fu, fv = np.floor(u + f32(0.5)), np.floor(vv + f32(0.5))
            inside = (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            census["near"] += int((~front).sum())
            census["left"] += int((front & (fu < 0)).sum())
            census["right"] += int((front & (fu >= W)).sum())
            census["top"] += int((front & (fv < 0)).sum())
            census["bottom"] += int((front & (fv >= H)).sum())
            ok = front & inside
            iu = np.where(ok, fu, 0).astype(np.int64)
            iv = np.where(ok, fv, 0).astype(np.int64)
            alpha = (f32(1) - final_T[k][iv, iu].astype(f32)).astype(f32)
            opaque = ok & ~(alpha < amin)
            census["see_through"] += int((ok & ~opaque).sum())
            d = (depth[k][iv, iu].astype(f32) - z).astype(f32)
            near_enough = opaque & (np.abs(d) <= tol)
            census["depth_nan"] += int((opaque & np.isnan(d)).sum())
            census["depth_in_front"] += int((opaque & (d < -tol)).sum())      # the view sees something nearer: occluded
            census["depth_behind"] += int((opaque & (d > tol)).sum())        # the view's surface lies behind the vertex
            use = near_enough
            w = np.ones(V, f32)
            if normals is not None:
                ex, ey, ez = campos[k, 0] - px, campos[k, 1] - py, campos[k, 2] - pz
                el = np.sqrt((ex * ex + ey * ey) + ez * ez).astype(f32)
                cs = (((nrm[:, 0] * ex + nrm[:, 1] * ey) + nrm[:, 2] * ez) / el).astype(f32)
                use = near_enough & (cs > cmin)
                census["facing_away"] += int((near_enough & ~use).sum())
                w = (cs * cs).astype(f32)
            for ch in range(3):
                term = (w * (color[k, ch][iv, iu] / alpha).astype(f32)).astype(f32)
                acc[:, ch] = np.where(use, acc[:, ch] + term, acc[:, ch]).astype(f32)
            wsum = np.where(use, wsum + w, wsum).astype(f32)
            seen += use
        census["used"] = int(seen.sum())
        census["unseen"] = int((seen == 0).sum())
        raw = (acc / wsum[:, None]).astype(f32)
        census["clamped"] = int(((seen > 0)[:, None] & ((raw > 1) | (raw < 0))).sum())
        out = np.where((seen > 0)[:, None], np.fmin(np.fmax(raw, f32(0)), f32(1)), np.asarray(fill, f32)[None, :]).astype(f32)
    return (out, seen, census) if return_census else (out, seen)


# ---- colours: the float64 oracle --------------------------------------------------------------------------------------
# Written from the header's contract: float64 throughout, the view transform as a 4x4 product, pixel centres at integer
# coordinates.  The device decides in float32, so next to every decision stands a bound on the float32 error of the
# quantity it tests; a (vertex, view) pair with a decision inside its bound is masked, and so is its vertex.  First-order
# rounding analysis with u = 2^-24 and gamma(n) = n u / (1 - n u):
#   x = c0 px + c1 py + c2 pz + c3   the vertex is exact; three products and three additions, every intermediate at most
#                                B = sum |c_r p_r| + |c3|                                             -> E_lin = gamma(6) B
#   q = x / z                    (E_lin + |q| E_lin) / (z - E_lin) from the operands, u |q| from the division   -> E_q
#   t = q * fx                   fx itself is rounded to float32, and so is the product              -> fx E_q + gamma(2) |t|
#   u = t + cx, h = u + 0.5      cx and 0.5 are exact; each addition rounds its result               -> + u |u| + u |h|
#   a = 1 - final_T              one rounding                                                        -> u |a|
#   d = depth - z, |d| <= tol    the error of z and one rounding                                     -> E_lin + u |d|
#   e = campos - p               one rounding per component; n . e: three products, two additions; |e|: as many and the
#                                root; the division                                 -> E_cs = gamma(6) |n| + gamma(8) |cs|
# Outside the mask both precisions use the same views, and the colour differs through the values only: a term
# w * (color / alpha) carries 2 E_cs / cs + 3 u relatively (cs * cs, the division, the product), the two running sums of
# n terms gamma(n - 1) each and the last division u; a weighted mean moves by at most (the largest relative error of a
# weight) * (the spread of the values), which is at most twice the largest value.  The bound is doubled, as the other
# oracles of this suite double theirs.
def _gamma(n):
    return n * U / (1.0 - n * U)


def colors_oracle(vertices, normals, viewmats, tanfovx, tanfovy, campos, color, depth, final_T, depth_tol, alpha_min=0.5,
                  cos_min=0.3, fill=(0.5, 0.5, 0.5)):
    """(colors float64 [V,3], seen [V], masked bool [V, n_views], tol float64 [V])."""
    p = np.ascontiguousarray(vertices, f32).reshape(-1, 3).astype(np.float64)
    n_views, H, W = depth.shape
    V = len(p)
    color = np.asarray(color, f32).reshape(n_views, 3, H, W).astype(np.float64)
    tol_d, amin, cmin = float(f32(depth_tol)), float(f32(alpha_min)), float(f32(cos_min))
    near = float(NEAR_Z)
    acc = np.zeros((V, 3))
    wsum = np.zeros(V)
    seen = np.zeros(V, np.int64)
    masked = np.zeros((V, n_views), bool)
    worst_rel = np.zeros(V)
    largest = np.zeros(V)
    hom = np.concatenate([p, np.ones((V, 1))], axis=1)
    nrm = None if normals is None else np.ascontiguousarray(normals, f32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        for k in range(n_views):
            M = np.asarray(viewmats[k], f32).reshape(4, 4).astype(np.float64)         # row vectors: hom @ M
            cam = hom @ M
            x, y, z = cam[:, 0], cam[:, 1], cam[:, 2]
            B = np.abs(hom[:, None, :] * M.T[None, :3, :]).sum(axis=2)               # [V,3]: sum |c_r p_r| + |c3| per row
            E = _gamma(6) * B
            live = np.ones(V, bool)
            amb = np.abs(z - near) <= E[:, 2]
            live &= z > near
            masked[:, k] |= amb
            zs = np.where(live, z, 1.0)
            fx = W / (2.0 * float(f32(tanfovx[k])))
            fy = H / (2.0 * float(f32(tanfovy[k])))
            pix = []
            for c_, Ec, foc, half, size in ((x, E[:, 0], fx, (W - 1) / 2.0, W), (y, E[:, 1], fy, (H - 1) / 2.0, H)):
                q = c_ / zs
                Eq = (Ec + np.abs(q) * E[:, 2]) / np.maximum(zs - E[:, 2], 1e-300) + U * np.abs(q)
                t = q * foc
                uu = t + half
                h = uu + 0.5
                Eh = foc * Eq + _gamma(2) * np.abs(t) + U * np.abs(uu) + U * np.abs(h)
                masked[:, k] |= live & (np.abs(h - np.round(h)) <= Eh)
                fl = np.floor(h)
                pix.append((fl, (fl >= 0) & (fl < size)))
            live = live & pix[0][1] & pix[1][1]
            iu = np.where(live, pix[0][0], 0).astype(np.int64)
            iv = np.where(live, pix[1][0], 0).astype(np.int64)
            alpha = 1.0 - final_T[k][iv, iu].astype(np.float64)
            masked[:, k] |= live & (np.abs(alpha - amin) <= U * np.abs(alpha))
            live = live & ~(alpha < amin)
            d = np.abs(depth[k][iv, iu].astype(np.float64) - z)
            masked[:, k] |= live & np.isfinite(d) & (np.abs(d - tol_d) <= E[:, 2] + U * d)      # (an infinite depth is far)
            live = live & (d <= tol_d)
            w = np.ones(V)
            rel = np.zeros(V)
            if nrm is not None:
                e = np.asarray(campos[k], f32).astype(np.float64)[None, :] - p
                cs = (nrm * e).sum(axis=1) / np.linalg.norm(e, axis=1)
                Ecs = _gamma(6) * np.linalg.norm(nrm, axis=1) + _gamma(8) * np.abs(cs)
                masked[:, k] |= live & (np.abs(cs - cmin) <= Ecs)
                live = live & (cs > cmin)
                w = cs * cs
                rel = 2.0 * Ecs / np.maximum(np.abs(cs), 1e-300)
            value = color[k][:, iv, iu].T / alpha[:, None]                           # [V,3]
            acc += np.where(live[:, None], w[:, None] * value, 0.0)
            wsum += np.where(live, w, 0.0)
            seen += live
            worst_rel = np.maximum(worst_rel, np.where(live, rel + 3 * U, 0.0))
            largest = np.maximum(largest, np.where(live, np.abs(value).max(axis=1), 0.0))
        raw = acc / wsum[:, None]
        out = np.where((seen > 0)[:, None], np.clip(raw, 0.0, 1.0), np.asarray(fill, np.float64)[None, :])
    tol = 2.0 * (2.0 * (worst_rel + 2.0 * _gamma(np.maximum(seen, 1))) * largest + U)
    return out, seen, masked, tol
