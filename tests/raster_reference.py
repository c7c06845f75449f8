"""NumPy float64 reference of the forward rasterizer WITH PER-ELEMENT ERROR BOUNDS AND DECISION SETS, independent of the
code under test (pegasus_amd/csrc/preprocess.hip.h, tilebin.hip.h, composite.hip.h) and of oracle/pgr_oracle.c.

The formulas are the literal forms of SURVEY.md section 8a rows a5 / a10; the only import from the project is the SH basis of
oracle/dense_ref.py (Legendre recurrences, its own constants) and, for posed objects, tests/pose_reference.py.  Inputs are the
float32 values the kernels get, widened to float64.

Bounds.  u = 2^-24 is float32's unit roundoff.  Every quantity is carried as a pair (v, e): the float64 value and a bound on
|x - v| for ANY float32 evaluation x of the same formula (any association, fused or not).  The pair arithmetic below is a
running error analysis: a k-term sum costs k - 1 roundings of at most u * sum |terms| each (the magnitude sum, not the result:
that is where cancellation, e.g. in det = a c - b^2, enters), a product / quotient / square root one rounding of u * |result|,
and the operands' own bounds are propagated to first order with the second-order term kept.  An operation whose exact result
is a float32 number and whose operands carry no error costs nothing (x * 1, x + 0, 0.5 * x, a float32 input itself): that is
what lets a constructed case sit EXACTLY on a threshold with a zero bound.  The number of roundings on each path is written
next to the line that spends them.

Decisions.  A comparison of a pair against a threshold is DECIDED iff |v - threshold| > e, or e == 0 (then every float32
evaluation gives v itself).  A Gaussian's membership is decided iff its near cull, its four rectangle truncations (for
either outcome of an undecided ceil of the radius) and its empty-rectangle test are; a pixel is decided iff every decision on its path up to its stop is, every Gaussian
that could blend there has a decided membership, and no two entries blended there could swap their depth order.

Every constant and the strictness of every discontinuous comparison is a keyword of ``Model`` (mutation checks,
tests/test_raster_decisions_host.py).  The comparisons that only SELECT between two values that are equal at equality (the
1.3 tanfov clamps, max(0.1, .), min(0.99, .), max(colour, 0)) have no strictness to flip."""
import dataclasses

import numpy as np

from oracle.dense_ref import real_sh_basis

U = 2.0 ** -24
_f32c = lambda x: float(np.float32(x))         # the model's constants are float32 literals


@dataclasses.dataclass(frozen=True)
class Model:
    near: float = _f32c(0.2)
    clamp: float = _f32c(1.3)
    lowpass: float = _f32c(0.3)
    disc_floor: float = _f32c(0.1)
    radius_factor: float = 3.0
    tile: int = 16
    alpha_min: float = _f32c(np.float32(1.0) / np.float32(255.0))
    alpha_max: float = _f32c(0.99)
    t_eps: float = _f32c(1e-4)
    color_offset: float = 0.5
    hom_eps: float = _f32c(1e-7)
    near_cull_inclusive: bool = True          # cull iff z <= near
    power_skip_strict: bool = True            # skip iff power > 0
    alpha_skip_strict: bool = True            # skip iff alpha < alpha_min
    stop_strict: bool = True                  # stop iff T (1 - alpha) < t_eps
    empty_inclusive: bool = True              # no instance iff max <= min on an axis


# ---- (value, bound) arithmetic ---------------------------------------------------------------------------------------------
class B:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    def __getitem__(self, k):
        return B(self.v[k], self.e[k])

    def __neg__(self):
        return B(-self.v, self.e)


def _b(x):
    return x if isinstance(x, B) else B(x)


def _is32(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return v.astype(np.float32).astype(np.float64) == v


def _round(v, clean):
    """One float32 rounding of a result v: u |v|, nothing where the operands are clean and v is a float32 number."""
    return np.where(clean & _is32(v), 0.0, U * np.abs(v))


def bsum(*terms):
    """k-term sum, any association: k - 1 roundings, each at most u (sum |terms| + their bounds).  Terms that are exactly
    zero are not terms; two clean terms whose sum is a float32 number cost nothing."""
    ts = [_b(t) for t in terms]
    v = sum(t.v for t in ts)
    e_in = sum(t.e for t in ts)
    mag = sum(np.abs(t.v) for t in ts) + e_in
    k = sum(((t.v != 0) | (t.e != 0)).astype(np.int64) for t in ts)
    rnd = np.maximum(k - 1, 0) * U * mag
    rnd = np.where((k == 2) & (e_in == 0) & _is32(v), 0.0, rnd)
    return B(v, e_in + rnd)


def bmul(a, b):
    a, b = _b(a), _b(b)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        v = a.v * b.v
        prop = np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e
        # a clean power of two scales exactly (2 x, 0.5 x, -x)
        pow2 = ((a.e == 0) & (np.frexp(a.v)[0] == np.sign(a.v) * 0.5)) | ((b.e == 0) & (np.frexp(b.v)[0] == np.sign(b.v) * 0.5))
    return B(v, prop + np.where(pow2, 0.0, _round(v, prop == 0) + U * prop))


def bdiv(a, b):
    a, b = _b(a), _b(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = a.v / b.v
        den = np.maximum(np.abs(b.v) - b.e, 1e-300)
        prop = (a.e + np.abs(v) * b.e) / den
    return B(v, prop + _round(v, prop == 0) + U * prop)


def bsqrt(a):
    a = _b(a)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.sqrt(a.v)
        prop = np.where(a.e == 0, 0.0, a.e / (np.sqrt(np.maximum(a.v - a.e, 0.0)) + v + 1e-300))
    return B(v, prop + _round(v, prop == 0) + U * prop)


def bclip_lo(a, lo):
    """max(a, lo): exact selection; the bound is a's, and nothing where a is certainly below lo."""
    a = _b(a)
    return B(np.maximum(a.v, lo), np.where(a.v + a.e < lo, 0.0, a.e))


def bclip_hi(a, hi):
    a = _b(a)
    return B(np.minimum(a.v, hi), np.where(a.v - a.e > hi, 0.0, a.e))


def bexp(p):
    """exp(power) as the GPU evaluates it, v_exp_f32(power * log2e), or as expf: the product rounds once (u |power log2e| in
    the exponent = u |power| relative in the result), log2e is a float32 constant (half a rounding, u / 2 |power|), and the
    exponential itself is good to one ulp = 2 u relative: (1.5 |power| + 2) u, counted as (2 |power| + 2) u.  A result in the
    subnormal range may be flushed: 2^-126 absolute.  exp(0) of a clean zero is exactly 1 on both."""
    p = _b(p)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.exp(p.v)
        e = v * np.expm1(p.e) + (2.0 * np.abs(p.v) + 2.0) * U * v + 2.0 ** -126
    return B(v, np.where((p.v == 0) & (p.e == 0), 0.0, e))


def decided(x, thr):
    x = _b(x)
    return (np.abs(x.v - thr) > x.e) | (x.e == 0)


def _clamp_trunc(f, hi):
    """min(hi, max(0, int(f))) with C truncation toward zero."""
    with np.errstate(invalid="ignore"):
        return np.where(f > 0, np.minimum(np.floor(np.where(f > 0, f, 0.0)), hi), 0).astype(np.int64)


# ---- per Gaussian ----------------------------------------------------------------------------------------------------------
def _w(a, shape=None):
    """float32 values widened to float64."""
    a = np.asarray(a, np.float32).astype(np.float64)
    return a if shape is None else a.reshape(shape)


def _dot(row, cols):
    """sum_k row[k] * cols[k]: len(row) products (1 rounding each) + len(row) - 1 additions."""
    return bsum(*[bmul(r, c) for r, c in zip(row, cols)])


def preprocess(means3d, opacities, *, scales=None, rotations=None, cov3d_precomp=None, shs=None, colors_precomp=None,
               sh_degree=0, scale_modifier=1.0, width, height, tanfovx, tanfovy, viewmatrix, projmatrix, campos, bg=None,
               object_id=None, poses=None, tie_index=None, model=Model(), **_ignored):
    """Every per-Gaussian value of row a5 as a (value, bound) pair over all n Gaussians, and the decisions.  Values of
    Gaussians behind the camera are meaningless (and may be non-finite); ``projected`` tells."""
    md = model
    W, H = int(width), int(height)
    x = _w(means3d, (-1, 3))
    n = x.shape[0]
    vm, pm, cam = _w(viewmatrix, 16), _w(projmatrix, 16), _w(campos, 3)
    tfx, tfy = _f32c(tanfovx), _f32c(tanfovy)
    mod = _f32c(scale_modifier)
    gx, gy = (W + md.tile - 1) // md.tile, (H + md.tile - 1) // md.tile
    posed = np.zeros(n, bool)
    Rp = None
    with np.errstate(all="ignore"):
        # position: the input itself, or R (x - c) + c + t of a posed object: pose_reference's count, K_XYZ u on its magnitude
        p = [B(x[:, k]) for k in range(3)]
        if object_id is not None:
            import pose_reference as PR
            oid = np.asarray(object_id, np.int64)
            P = _w(poses, (-1, 20))
            posed = oid > 0
            Rp = np.tile(np.eye(3), (n, 1, 1))
            pv, pe = x.copy(), np.zeros_like(x)
            for k in np.unique(oid[posed]):
                m = oid == k
                row = np.asarray(poses, np.float32).reshape(-1, 20)[k - 1]
                out, mag = PR.positions(np.asarray(means3d, np.float32).reshape(-1, 3)[m], row[0:9], row[9:12],
                                        center=row[12:15])
                pv[m], pe[m] = out, PR.K_XYZ * U * mag
                Rp[m] = P[k - 1, 0:9].reshape(3, 3)
            p = [B(pv[:, k], pe[:, k]) for k in range(3)]
        one = np.ones(n)
        # view space and homogeneous projection: 3 products + 3 additions each (a zero matrix entry spends nothing)
        tx = _dot(p + [one], [vm[0], vm[4], vm[8], vm[12]])
        ty = _dot(p + [one], [vm[1], vm[5], vm[9], vm[13]])
        tz = _dot(p + [one], [vm[2], vm[6], vm[10], vm[14]])
        hx = _dot(p + [one], [pm[0], pm[4], pm[8], pm[12]])
        hy = _dot(p + [one], [pm[1], pm[5], pm[9], pm[13]])
        hw = _dot(p + [one], [pm[3], pm[7], pm[11], pm[15]])
        near_dec = decided(tz, md.near)
        culled = (tz.v <= md.near) if md.near_cull_inclusive else (tz.v < md.near)
        p_w = bdiv(1.0, bsum(hw, md.hom_eps))                                  # +1 addition, +1 division
        ndc_x, ndc_y = bmul(hx, p_w), bmul(hy, p_w)                            # +1
        pix_x = bmul(bsum(bmul(bsum(ndc_x, 1.0), float(W)), -1.0), 0.5)        # +1, +1, +1, x 0.5 exact
        pix_y = bmul(bsum(bmul(bsum(ndc_y, 1.0), float(H)), -1.0), 0.5)

        # Sigma3D = R diag(mod s)^2 R^T
        if cov3d_precomp is not None:
            c6 = _w(cov3d_precomp, (-1, 6))
            S = [[B(c6[:, j]) for j in row] for row in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]
        else:
            q = _w(rotations, (-1, 4))
            if posed.any():
                # posed: q_pose (x) q / max(|q|, 1e-12); the product's 16 products + 12 additions + the normalisation are
                # counted by the pair arithmetic like everything else
                import pose_reference as PR
                qn, _ = PR.normalize_rule(np.asarray(rotations, np.float32))
                nrm = bsqrt(bsum(*[bmul(q[:, k], q[:, k]) for k in range(4)]))
                inv = bdiv(1.0, bclip_lo(nrm, 1e-12))
                qb = [bmul(q[:, k], inv) for k in range(4)]
                assert np.allclose(np.stack([c.v for c in qb], 1), qn, rtol=0, atol=1e-12)
                a, b, c, d = (np.where(posed, P[np.maximum(oid, 1) - 1, 15 + k], (1.0, 0.0, 0.0, 0.0)[k]) for k in range(4))
                w_, x_, y_, z_ = qb
                comp = [bsum(bmul(a, w_), -bmul(b, x_), -bmul(c, y_), -bmul(d, z_)),
                        bsum(bmul(a, x_), bmul(b, w_), bmul(c, z_), -bmul(d, y_)),
                        bsum(bmul(a, y_), -bmul(b, z_), bmul(c, w_), bmul(d, x_)),
                        bsum(bmul(a, z_), bmul(b, y_), -bmul(c, x_), bmul(d, w_))]
                qq = [B(np.where(posed, cq.v, q[:, k]), np.where(posed, cq.e, 0.0)) for k, cq in enumerate(comp)]
            else:
                qq = [B(q[:, k]) for k in range(4)]
            r_, x_, y_, z_ = qq
            two = lambda t: bmul(2.0, t)                                        # exact
            mm = lambda s, t: bmul(s, t)
            Rm = [[bsum(1.0, -two(bsum(mm(y_, y_), mm(z_, z_)))), two(bsum(mm(x_, y_), -mm(r_, z_))), two(bsum(mm(x_, z_), mm(r_, y_)))],
                  [two(bsum(mm(x_, y_), mm(r_, z_))), bsum(1.0, -two(bsum(mm(x_, x_), mm(z_, z_)))), two(bsum(mm(y_, z_), -mm(r_, x_)))],
                  [two(bsum(mm(x_, z_), -mm(r_, y_))), two(bsum(mm(y_, z_), mm(r_, x_))), bsum(1.0, -two(bsum(mm(x_, x_), mm(y_, y_))))]]
            sc = _w(scales, (-1, 3))
            s = [bmul(mod, sc[:, k]) for k in range(3)]                         # 1
            M = [[bmul(Rm[i][k], s[k]) for k in range(3)] for i in range(3)]    # 1
            S = [[_dot(M[i], M[j]) for j in range(3)] for i in range(3)]        # 3 + 2
        cov3d = [S[0][0], S[0][1], S[0][2], S[1][1], S[1][2], S[2][2]]

        # EWA projection
        fx, fy = bdiv(float(W), bmul(2.0, tfx)), bdiv(float(H), bmul(2.0, tfy))   # 1
        limx, limy = bmul(md.clamp, tfx), bmul(md.clamp, tfy)                     # 1
        txtz, tytz = bdiv(tx, tz), bdiv(ty, tz)                                   # 1
        clamp_dec = np.stack([decided(txtz, limx.v) & decided(txtz, -limx.v), decided(tytz, limy.v) & decided(tytz, -limy.v)], 1)
        clamped = np.stack([np.abs(txtz.v) > limx.v, np.abs(tytz.v) > limy.v], 1)

        def clip(r, lim):
            e = np.where(np.abs(r.v) - r.e > lim.v, lim.e, np.where(np.abs(r.v) + r.e < lim.v, r.e, np.maximum(r.e, lim.e)))
            return B(np.clip(r.v, -lim.v, lim.v), e)
        txc, tyc = bmul(clip(txtz, limx), tz), bmul(clip(tytz, limy), tz)         # 1
        tz2 = bmul(tz, tz)
        j00, j11 = bdiv(fx, tz), bdiv(fy, tz)
        j02, j12 = -bdiv(bmul(fx, txc), tz2), -bdiv(bmul(fy, tyc), tz2)
        T0 = [bsum(bmul(j00, vm[4 * c + 0]), bmul(j02, vm[4 * c + 2])) for c in range(3)]
        T1 = [bsum(bmul(j11, vm[4 * c + 1]), bmul(j12, vm[4 * c + 2])) for c in range(3)]
        U0 = [_dot(T0, [S[0][c], S[1][c], S[2][c]]) for c in range(3)]
        U1 = [_dot(T1, [S[0][c], S[1][c], S[2][c]]) for c in range(3)]
        c_xx = bsum(_dot(U0, T0), md.lowpass)
        c_xy = _dot(U0, T1)
        c_yy = bsum(_dot(U1, T1), md.lowpass)
        det = bsum(bmul(c_xx, c_yy), -bmul(c_xy, c_xy))                           # 2 products + 1 subtraction of a c + b^2
        det_cond = (np.abs(c_xx.v * c_yy.v) + c_xy.v ** 2) / np.abs(det.v)
        det_zero = det.v == 0
        det_inv = bdiv(1.0, det)
        conic = [bmul(c_yy, det_inv), -bmul(c_xy, det_inv), bmul(c_xx, det_inv)]
        mid = bmul(0.5, bsum(c_xx, c_yy))
        d2 = bsum(bmul(mid, mid), -det)
        floor_dec = decided(d2, md.disc_floor)
        disc = bsqrt(bclip_lo(d2, md.disc_floor))
        lam = bsum(mid, disc)                                                     # max(mid + disc, mid - disc), disc >= 0
        rr = bmul(md.radius_factor, bsqrt(lam))
        r_lo, r_hi, r_c = np.ceil(rr.v - rr.e), np.ceil(rr.v + rr.e), np.ceil(rr.v)
        radius_dec = r_lo == r_hi

        def edges(r):
            rf = B(r)                                                             # an integer below 2^24: exact
            return [bdiv(bsum(pix_x, -rf), float(md.tile)), bdiv(bsum(pix_y, -rf), float(md.tile)),
                    bdiv(bsum(pix_x, rf, float(md.tile - 1)), float(md.tile)), bdiv(bsum(pix_y, rf, float(md.tile - 1)), float(md.tile))]
        his = (gx, gy, gx, gy)
        e_c = edges(r_c)
        rect = np.stack([_clamp_trunc(e.v, hi) for e, hi in zip(e_c, his)], 1)
        cands = []
        for r in (r_lo, r_hi):
            for e, hi in zip(edges(r), his):
                cands += [_clamp_trunc(e.v - e.e, hi), _clamp_trunc(e.v + e.e, hi)]
        cands = np.stack(cands, 1).reshape(n, 2, 4, 2)
        rect_lo, rect_hi = cands.min(axis=(1, 3)), cands.max(axis=(1, 3))
        edge_dec = rect_lo == rect_hi

        def empty(rc, lo_side, hi_side):
            w_, h_ = hi_side[:, 2] - lo_side[:, 0], hi_side[:, 3] - lo_side[:, 1]
            return ((w_ <= 0) | (h_ <= 0)) if md.empty_inclusive else ((w_ < 0) | (h_ < 0))
        is_empty = empty(rect, rect, rect)
        empty_dec = empty(None, rect_hi, rect_lo) == empty(None, rect_lo, rect_hi)   # smallest and largest possible rectangle

        # colour: SH(dir) + offset, clamp at 0
        if colors_precomp is not None:
            cp = _w(colors_precomp, (-1, 3))
            raw = B(cp)
            rgb = B(cp)
        else:
            sh = _w(shs).reshape(n, -1, 3)
            ncoef = (sh_degree + 1) ** 2
            dvec = np.stack([c.v for c in p], 1) - cam
            dlen = np.linalg.norm(dvec, axis=1)
            dn = dvec / dlen[:, None]
            # direction error: the subtraction (1 rounding of |p| + |c|, plus p's own bound), three squares + two additions +
            # square root + division (<= 5 roundings relative on a unit vector); rotated into the object's frame: 3 + 2 more
            derr = (np.stack([c.e for c in p], 1) + U * (np.abs(np.stack([c.v for c in p], 1)) + np.abs(cam))).sum(1) / dlen + 5 * U
            if Rp is not None:
                dn = np.where(posed[:, None], np.einsum("nji,nj->ni", Rp, dn), dn)
                derr = np.where(posed, 3 * derr + 5 * U, derr)
            basis = np.stack([real_sh_basis(sh_degree, d) if np.isfinite(d).all() else np.zeros(ncoef) for d in dn])
            # a basis function of band l is a homogeneous polynomial of degree l with |gradient| <= GRAD[l] on the unit ball and
            # is evaluated in at most POLY[l] roundings of at most AMAX[l]: its constant, which is a float32 number in any
            # float32 evaluation (1, band 0 included: C0 itself is rounded), and 1 + 2 l operations
            band = np.repeat(np.arange(4), (1, 3, 5, 7))[:ncoef]
            GRAD, POLY, AMAX = np.array([0.0, 0.5, 2.5, 7.0]), np.array([1.0, 3.0, 6.0, 9.0]), np.array([0.3, 0.5, 1.3, 3.0])
            berr = GRAD[band][None, :] * derr[:, None] + (POLY * AMAX)[band][None, :] * U
            terms = [bmul(B(basis[:, k:k + 1], berr[:, k:k + 1]), sh[:, k, :]) for k in range(ncoef)]   # 1 each
            raw = bsum(bsum(*terms) if ncoef > 1 else terms[0], md.color_offset)                     # ncoef - 1, + 1
            rgb = bclip_lo(raw, 0.0)
        color_dec = decided(raw, 0.0) if colors_precomp is None else np.ones((n, 3), bool)

    projected = ~culled & ~det_zero & ~is_empty & np.isfinite(rr.v)
    # the radius reaches the pixels only through the rectangle, whose candidates above cover both of its outcomes
    member_dec = near_dec & (culled | (edge_dec.all(1) & empty_dec))
    # could be an entry at all in some float32 evaluation
    possible = (~culled | ~near_dec) & ~det_zero & np.isfinite(rr.v) & ~(is_empty & empty_dec) & (tz.v + tz.e > 0)
    tie = np.arange(n) if tie_index is None else np.asarray(tie_index, np.int64)
    return dict(n=n, W=W, H=H, grid=(gx, gy), model=md, p=p, z=tz, tx=tx, ty=ty, xy=(pix_x, pix_y), cov3d=cov3d,
                cov2d=(c_xx, c_xy, c_yy), det=det, det_inv=det_inv, det_cond=det_cond, det_zero=det_zero, conic=conic, rr=rr, radius=r_c.astype(np.int64),
                radius_lo=r_lo, radius_hi=r_hi, edges=e_c, rect=rect, rect_lo=rect_lo, rect_hi=rect_hi, raw_color=raw, rgb=rgb,
                opacity=_w(opacities, -1), culled=culled, projected=projected, possible=possible, tie=tie,
                clamped=clamped, txtz=(txtz, tytz), lim=(limx, limy),
                dec=dict(near=near_dec, clamp=clamp_dec.all(1), floor=floor_dec, radius=radius_dec, edges=edge_dec.all(1),
                         empty=empty_dec, color=color_dec.all(1), member=member_dec),
                bg=np.zeros(3) if bg is None else _w(bg, 3))


def undecided_shares(pre):
    """{decision kind: undecided Gaussians / projected Gaussians}."""
    m = pre["projected"] | ~pre["dec"]["near"]
    tot = max(1, int(pre["projected"].sum()))
    return {k: float((~v & m).sum()) / tot for k, v in pre["dec"].items()}


def pair_alpha(pre, g, X, Y):
    """(power, opacity * exp(power)) pairs of Gaussian g at pixel centres X, Y (integer coordinates, exact).

    power = -1/2 (A dx^2 + C dy^2) - B dx dy = -1/2 d^T S^-1 d with S = Sigma2D, (A, B, C) = (c_yy, -c_xy, c_xx) / det.
    Charging the bounds of A, B, C on the magnitude sum of the three terms counts the error S inherits from the projection
    three times (in the entry, in det, and once more as if the three entries erred independently); the first derivation did
    and left every pixel near a needle undecided.  The bound below is the first-order sensitivity instead, with
    g = S^-1 d = (A dx + B dy, B dx + C dy):
      (a) S's own bounds e_xx, e_xy, e_yy (everything up to the + 0.3):  d power = 1/2 g^T dS g  <=  1/2 (g_x^2 e_xx + 2 |g_x g_y| e_xy
          + g_y^2 e_yy): the cancellation of a needle's conic is in g, per pixel, not in a global factor;
      (b) the pixel position's bound and the subtraction's rounding, e_dx, e_dy:  |g_x| e_dx + |g_y| e_dy + 1/2 (A e_dx^2 + C e_dy^2);
      (c) det's own 3 roundings (2 products, 1 subtraction), each at most u (c_xx c_yy + c_xy^2):  3 u cond |power|;
      (d) 1 / det: 1 rounding, u |power|;  the conic entries: 1 each, u on the magnitude sum m = 1/2 A dx^2 + 1/2 C dy^2 + |B dx dy|;
      (e) the evaluation: at most 3 products per term and 2 additions: 5 u m.
    (a) - (c) are first order in the relative error eta of det; they are divided by (1 - eta)^2, and no claim is made
    (infinite bound) from eta = 1/2 on."""
    px, py = pre["xy"][0][g], pre["xy"][1][g]
    c_xx, c_xy, c_yy = (c[g] for c in pre["cov2d"])
    det = pre["det"][g]
    A, Bc, C = c_yy.v / det.v, -c_xy.v / det.v, c_xx.v / det.v
    dx, dy = bsum(px, -X), bsum(py, -Y)                                            # 1 each
    gx, gy = A * dx.v + Bc * dy.v, Bc * dx.v + C * dy.v
    v = -0.5 * (A * dx.v * dx.v + C * dy.v * dy.v) - Bc * dx.v * dy.v
    m = 0.5 * A * dx.v * dx.v + 0.5 * C * dy.v * dy.v + np.abs(Bc * dx.v * dy.v)
    first = (0.5 * (gx * gx * c_xx.e + 2.0 * np.abs(gx * gy) * c_xy.e + gy * gy * c_yy.e)
             + np.abs(gx) * dx.e + np.abs(gy) * dy.e + 0.5 * (A * dx.e ** 2 + C * dy.e ** 2)
             + 3.0 * U * pre["det_cond"][g] * np.abs(v))
    eta = det.e / np.abs(det.v)
    with np.errstate(divide="ignore"):
        e = np.where(eta < 0.5, first / (1.0 - np.minimum(eta, 0.5)) ** 2, np.inf) + U * np.abs(v) + 6.0 * U * m
    q = B(v, e)
    ex = bexp(B(np.minimum(q.v, 0.0), q.e))
    return q, bmul(pre["opacity"][g], ex)                                          # 1


def depth_order(pre, which):
    """Indices ``which`` in compositing order: float32 bits of the float64 z, then tie index."""
    z32 = pre["z"].v[which].astype(np.float32).view(np.uint32).astype(np.int64)
    return which[np.lexsort((pre["tie"][which], z32))]


def composite(pre):
    """Row a10 over the entries in depth order, each restricted to its rectangle: per-pixel (value, bound) pairs of colour,
    depth and T, the decided mask, and what every pixel blended."""
    md = pre["model"]
    W, H, ts = pre["W"], pre["H"], pre["model"].tile
    order = depth_order(pre, np.flatnonzero(pre["possible"]))
    z = pre["z"]
    # entries that could swap: neighbours in depth whose z bounds overlap (equal z of equal inputs is a tie, not a swap)
    chain = np.zeros(len(order), np.int64)
    amb_chain = np.zeros(len(order), bool)
    pv = np.stack([c.v for c in pre["p"]], 1)
    cid = 0
    for k in range(1, len(order)):
        a, b = order[k - 1], order[k]
        dz = abs(z.v[b] - z.v[a])
        swap = (dz <= z.e[a] + z.e[b]) and not (dz == 0 and (z.e[a] == 0 or np.array_equal(pv[a], pv[b])))
        # float32 rounding of two distinct clean values cannot swap them either
        if swap and z.e[a] == 0 and z.e[b] == 0:
            swap = False
        if not swap:
            cid += 1
        chain[k] = cid
        if swap:
            amb_chain[k] = amb_chain[k - 1] = True
    Tv, Te = np.ones((H, W)), np.zeros((H, W))
    Cv, Ce = np.zeros((3, H, W)), np.zeros((3, H, W))
    Dv, De = np.zeros((H, W)), np.zeros((H, W))
    done, und = np.zeros((H, W), bool), np.zeros((H, W), bool)
    nblend = np.zeros((H, W), np.int64)
    last = np.full((H, W), -1, np.int64)
    stop_g = np.full((H, W), -1, np.int64)
    last_chain = np.full((H, W), -1, np.int64)
    bp, bg_, sp, sg = [], [], [], []
    und_kinds = dict(power=0, alpha_min=0, alpha_max=0, stop=0, member=0, order=0)
    pix_index = np.arange(H * W).reshape(H, W)
    for k, g in enumerate(order):
        central = bool(pre["projected"][g])
        mdec = bool(pre["dec"]["member"][g]) and central
        lo = pre["rect"][g] if mdec else np.minimum(pre["rect_lo"][g], pre["rect"][g])
        hi = pre["rect"][g] if mdec else np.maximum(pre["rect_hi"][g], pre["rect"][g])
        x0, y0, x1, y1 = ts * lo[0], ts * lo[1], min(W, ts * hi[2]), min(H, ts * hi[3])
        if x1 <= x0 or y1 <= y0:
            continue
        sl = (slice(y0, y1), slice(x0, x1))
        active = ~done[sl]
        if not active.any():
            continue
        Y, X = np.mgrid[y0:y1, x0:x1].astype(np.float64)
        q, araw = pair_alpha(pre, g, X, Y)
        skip_p = (q.v > 0) if md.power_skip_strict else (q.v >= 0)
        d_p = decided(q, 0.0)
        alpha = bclip_hi(araw, md.alpha_max)
        skip_a = (alpha.v < md.alpha_min) if md.alpha_skip_strict else (alpha.v <= md.alpha_min)
        d_amin = decided(alpha, md.alpha_min) | skip_p
        d_amax = decided(araw, md.alpha_max) | skip_p | skip_a
        if not mdec:
            # membership open: wherever it could blend, the pixel is open
            could = active & ~((skip_p & d_p) | (skip_a & d_amin & d_p))
            und_kinds["member"] += int((could & ~und[sl]).sum())
            und[sl] |= could
            if not central:
                continue
            cr = pre["rect"][g]
            inr = (X >= ts * cr[0]) & (X < ts * cr[2]) & (Y >= ts * cr[1]) & (Y < ts * cr[3])
            active = active & inr
        valid = active & ~skip_p & ~skip_a
        T = B(Tv[sl], Te[sl])
        test = bmul(T, bsum(1.0, -alpha))                                          # 1 - alpha: 1; the product: 1 (T's bound rides)
        d_stop = decided(test, md.t_eps)
        stop = valid & ((test.v < md.t_eps) if md.stop_strict else (test.v <= md.t_eps))
        blend = valid & ~stop
        for name, bad in (("power", active & ~d_p), ("alpha_min", active & ~skip_p & ~d_amin),
                          ("alpha_max", valid & ~d_amax), ("stop", valid & ~d_stop)):
            und_kinds[name] += int((bad & ~und[sl]).sum())
            und[sl] |= bad
        if amb_chain[k]:
            bad = blend & (last_chain[sl] == chain[k])
            und_kinds["order"] += int((bad & ~und[sl]).sum())
            und[sl] |= bad
            last_chain[sl] = np.where(blend, chain[k], last_chain[sl])
        wgt = bmul(alpha, T)                                                       # 1
        for c in range(3):
            acc = bsum(B(Cv[c][sl], Ce[c][sl]), bmul(pre["rgb"][g][c], wgt))       # 1 product + 1 addition per blend
            Cv[c][sl] = np.where(blend, acc.v, Cv[c][sl])
            Ce[c][sl] = np.where(blend, acc.e, Ce[c][sl])
        acc = bsum(B(Dv[sl], De[sl]), bmul(z[g], wgt))
        Dv[sl] = np.where(blend, acc.v, Dv[sl])
        De[sl] = np.where(blend, acc.e, De[sl])
        Tv[sl] = np.where(blend, test.v, Tv[sl])
        Te[sl] = np.where(blend, test.e, Te[sl])
        nblend[sl] += blend
        last[sl] = np.where(blend, g, last[sl])
        stop_g[sl] = np.where(stop, g, stop_g[sl])
        done[sl] |= stop
        if blend.any():
            idx = pix_index[sl][blend]
            bp.append(idx); bg_.append(np.full(idx.size, g, np.int64))
        if stop.any():
            idx = pix_index[sl][stop]
            sp.append(idx); sg.append(np.full(idx.size, g, np.int64))
    T = B(Tv, Te)
    bgc = pre["bg"]
    color = [bsum(B(Cv[c], Ce[c]), bmul(T, bgc[c])) for c in range(3)]             # 1 product + 1 addition
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return dict(color=B(np.stack([c.v for c in color]), np.stack([c.e for c in color])), depth=B(Dv, De), final_T=T,
                decided=~und, und_kinds=und_kinds, nblend=nblend, last=last, stop_g=stop_g, order=order,
                blend_pix=cat(bp), blend_g=cat(bg_), stop_pix=cat(sp), stop_g_pairs=cat(sg))


def forward(means3d, opacities, **kw):
    pre = preprocess(means3d, opacities, **kw)
    return pre, composite(pre)


# ---- comparison of an implementation's outputs (the HIP path's, or the C oracle's) with the reference ------------------------
def _ratio(got, ref, mask=None):
    """Worst |got - v| / e over ``mask``; an element with e == 0 must be equal."""
    err = np.abs(np.asarray(got, np.float64) - ref.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / ref.e)
    r = np.where(np.isnan(r), np.inf, r)
    if mask is not None:
        r = r[mask]
    return float(r.max(initial=0.0))


def compare(pre, img, out, tight):
    """Every check of an implementation's output dict ``out`` (keys as oracle.forward / helpers.gpu_forward return them)
    against the reference.  Returns (ratios, failures): the worst err / bound per continuous quantity and a list of
    messages, empty when everything holds.  ``tight``: the lists may omit (Gaussian, tile) instances whose alpha is below
    alpha_min at every pixel of the tile."""
    md, n, W, H = pre["model"], pre["n"], pre["W"], pre["H"]
    gx, gy = pre["grid"]
    ts = md.tile
    fails = []
    ratios = {}
    dec = pre["dec"]
    surv = np.asarray(out["radii"]) > 0
    both = surv & pre["projected"] & dec["member"]
    # culled set and integer outputs on decided Gaussians
    dm = dec["member"]
    if not np.array_equal(surv[dm], pre["projected"][dm]):
        bad = np.flatnonzero(dm & (surv != pre["projected"]))
        fails.append(f"culled set differs on decided Gaussians {bad[:5]} (of {bad.size})")
    rad = np.asarray(out["radii"], np.int64)
    rdec = both & dec["radius"]
    if not np.array_equal(rad[rdec], pre["radius"][rdec]):
        bad = np.flatnonzero(rdec & (rad != pre["radius"]))
        fails.append(f"radius differs on decided Gaussians {bad[:5]}: {rad[bad[:5]]} vs {pre['radius'][bad[:5]]}")
    open_r = surv & pre["possible"] & ~dec["radius"]
    if not ((rad[open_r] >= pre["radius_lo"][open_r]) & (rad[open_r] <= pre["radius_hi"][open_r])).all():
        fails.append("radius of an undecided Gaussian is neither neighbouring outcome")
    if "rects" in out:
        rc = np.asarray(out["rects"], np.int64)
        if not np.array_equal(rc[both], pre["rect"][both]):
            bad = np.flatnonzero(both & (rc != pre["rect"]).any(1))
            fails.append(f"rectangle differs on decided Gaussians {bad[:5]}: {rc[bad[:5]]} vs {pre['rect'][bad[:5]]}")
        o = surv & pre["possible"] & ~dm
        if not ((rc[o] >= pre["rect_lo"][o]) & (rc[o] <= pre["rect_hi"][o])).all():
            fails.append("rectangle edge of an undecided Gaussian is neither neighbouring outcome")
    if "tiles_touched" in out:
        tt = (pre["rect"][:, 2] - pre["rect"][:, 0]) * (pre["rect"][:, 3] - pre["rect"][:, 1])
        if not np.array_equal(np.asarray(out["tiles_touched"], np.int64)[both], tt[both]):
            fails.append("tiles_touched differs on decided Gaussians")
    # continuous per-Gaussian outputs, wherever both sides project the Gaussian
    m = surv & pre["projected"]
    ratios["xy"] = max(_ratio(out["xy"][:, 0], pre["xy"][0], m), _ratio(out["xy"][:, 1], pre["xy"][1], m))
    ratios["depth"] = _ratio(out["depth"], pre["z"], m)
    ratios["conic"] = max(_ratio(out["conic_opacity"][:, k], pre["conic"][k], m) for k in range(3))
    if not np.array_equal(np.asarray(out["conic_opacity"], np.float64)[m, 3], pre["opacity"][m]):
        fails.append("opacity is not passed through")
    rgb = out["rgb4"][:, :3] if "rgb4" in out else out["rgb"]
    ratios["rgb"] = _ratio(rgb, pre["rgb"], m[:, None] & np.ones(3, bool)[None, :])
    if "cov3d" in out and np.asarray(out["cov3d"]).any():
        ratios["cov3d"] = max(_ratio(out["cov3d"][:, k], pre["cov3d"][k], m) for k in range(6))
    # lists
    gs, ranges = np.asarray(out["gauss_sorted"], np.int64), np.asarray(out["ranges"], np.int64)
    tiles = gx * gy
    if ranges.shape[0] != tiles:
        return ratios, fails + [f"the tile grid has {ranges.shape[0]} tiles, not {tiles}"]
    pos = np.full((tiles, n), -1, np.int64)
    zbits = np.asarray(out["depth"], np.float32).view(np.uint32).astype(np.int64)
    for t in range(tiles):
        s, e = ranges[t]
        ids = gs[s:e]
        if ids.size == 0:
            continue
        pos[t, ids] = np.arange(ids.size)
        key = zbits[ids] * (2 * n) + pre["tie"][ids]
        if not (np.diff(key) > 0).all():
            fails.append(f"tile {t}: list is not sorted by (depth bits, index)")
        txx, tyy = t % gx, t // gx
        r = pre["rect"][ids]
        outside = both[ids] & ~((txx >= r[:, 0]) & (txx < r[:, 2]) & (tyy >= r[:, 1]) & (tyy < r[:, 3]))
        if outside.any():
            fails.append(f"tile {t}: instance outside the float64 rectangle of decided Gaussian {ids[outside][:5]}")
    # instances of the float64 rectangle that are not listed
    n_missing = 0
    for g in np.flatnonzero(both):
        r = pre["rect"][g]
        for tyy in range(r[1], r[3]):
            for txx in range(r[0], r[2]):
                if pos[tyy * gx + txx, g] >= 0:
                    continue
                n_missing += 1
                if not tight:
                    fails.append(f"Gaussian {g}: tile ({txx},{tyy}) of its rectangle is not listed")
                    continue
                Y, X = np.mgrid[ts * tyy:min(H, ts * tyy + ts), ts * txx:min(W, ts * txx + ts)].astype(np.float64)
                q, a = pair_alpha(pre, g, X, Y)
                if not ((a.v + a.e < md.alpha_min) | ((q.v - q.e > 0) & (q.e < np.inf))).all():
                    fails.append(f"Gaussian {g}: dropped tile ({txx},{tyy}) holds a pixel with alpha {a.v.max():.6g} "
                                 f"not below alpha_min by its bound")
    ratios["dropped_instances"] = n_missing
    # per pixel
    ok = img["decided"]
    ratios["color"] = _ratio(out["color"], img["color"], np.broadcast_to(ok, (3, H, W)))
    ratios["out_depth"] = _ratio(np.asarray(out["out_depth"]).reshape(H, W), img["depth"], ok)
    ratios["final_T"] = _ratio(out["final_T"], img["final_T"], ok)
    nc = np.asarray(out["n_contrib"], np.int64).reshape(-1)
    tile_of = ((np.arange(H)[:, None] // ts) * gx + (np.arange(W)[None, :] // ts)).reshape(-1)
    okf = ok.reshape(-1)
    start = ranges[tile_of, 0]
    glast = np.where(nc > 0, gs[np.minimum(start + nc - 1, max(gs.size - 1, 0))] if gs.size else -1, -1)
    if (nc > ranges[tile_of, 1] - start).any():
        fails.append("n_contrib beyond the tile's list")
    if not np.array_equal(glast[okf], img["last"].reshape(-1)[okf]):
        bad = np.flatnonzero(okf & (glast != img["last"].reshape(-1)))
        fails.append(f"last blended Gaussian differs at decided pixels {bad[:5]} (of {bad.size}): "
                     f"{glast[bad[:5]]} vs {img['last'].reshape(-1)[bad[:5]]}")
    bpix, bg_ = img["blend_pix"], img["blend_g"]
    pb = pos[tile_of[bpix], bg_]
    inside = (pb >= 0) & (pb < nc[bpix])
    if not inside[okf[bpix]].all():
        bad = np.flatnonzero(okf[bpix] & ~inside)
        fails.append(f"{bad.size} blended (pixel, Gaussian) pairs of float64 are not within n_contrib of the list, "
                     f"e.g. pixel {bpix[bad[0]]} Gaussian {bg_[bad[0]]}")
    spix, sg = img["stop_pix"], img["stop_g_pairs"]
    ps = pos[tile_of[spix], sg]
    if not ((ps >= nc[spix]) | ~okf[spix]).all():
        bad = np.flatnonzero(okf[spix] & ~(ps >= nc[spix]))
        fails.append(f"{bad.size} decided pixels are not stopped at the float64 entry (entry blended or not listed)")
    # nothing else was blended: between two listed float64 entries of a pixel only skipped entries can lie, so the count of
    # float64-blended entries within n_contrib must be the float64 blend count and the last one the float64 last one
    cnt = np.bincount(bpix[inside], minlength=H * W)
    if not np.array_equal(cnt[okf], img["nblend"].reshape(-1)[okf]):
        fails.append("blend count differs at decided pixels")
    for k, v in ratios.items():
        if k != "dropped_instances" and not v <= 1.0:
            fails.append(f"{k}: worst err / bound {v:.3g} > 1")
    return ratios, fails
