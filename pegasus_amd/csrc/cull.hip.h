// cull.hip.h -- the "can this splat reach alpha >= 1/255 anywhere in this pixel rectangle?" predicate.
// Used by the binning kernels (tile rectangle: tight lists) and by the backward pass.  Conservative by construction,
// bit-reproducible (no transcendental), and mirrored operation-for-operation by the oracle
// (pgr_oracle_tile_may_contribute).  The forward compositor's per-wave skip mask has a test of its own at the end of this
// file (quarter_may_contribute): conservative too, but free to differ from the oracle's decisions.
#pragma once
#include "pgr_common.h"

namespace pgr {

// ---- tight-list predicate ----------------------------------------------------------------------
// A (Gaussian, tile) instance only matters if alpha = min(0.99, op*exp(power)) >= 1/255 at some pixel of the
// tile.  With q = A dx^2 + 2B dx dy + C dy^2 (power = -q/2) that needs q <= 2 ln(255 op) somewhere.  The
// test bounds q from BELOW over the tile's continuous pixel rectangle (0 if the centre is inside, else the
// smaller of the minima over the two edges facing the centre) and 2 ln(255 op) from ABOVE (exponent + chord of
// log2 on the mantissa + 0.0861), adds a rounding margin, and keeps the instance unless the lower bound
// clears the upper bound.  Dropped instances would be skipped at every pixel, so no pixel's arithmetic
// changes (oracle: pgr_oracle_tile_may_contribute, same operation order, bit-identical decisions; measured
// on the C3 scene: 55-63 % of the 3-sigma-rectangle instances survive).
__device__ __forceinline__ float edge_min_q(float A, float B, float C, float r, float d_fixed, float lo, float hi) {
    // minimise over t in [lo,hi]:  A*d^2 + 2*B*d*t + C*t^2   with r = B / C precomputed per Gaussian
    float t = -(d_fixed * r);
    t = fminf(hi, fmaxf(lo, t));
    return A * d_fixed * d_fixed + 2.0f * B * d_fixed * t + C * t * t;
}

struct CullSplat { float mx, my, A, B, C, rBC, rBA, tau; uint32_t flags; };   // flags: 1 = never, 2 = always

// rBC = B / C and rBA = B / A are computed once per Gaussian and view by the preprocess (IEEE divisions, the same
// expressions as here) and ride in the record's last two floats: the binning walks and every quarter-tile walk of the
// compositor rebuild this record per use.
__device__ __forceinline__ CullSplat make_cull_splat(float2 xy, float4 co, float rBC, float rBA) {
    CullSplat s;
    s.mx = xy.x; s.my = xy.y; s.A = co.x; s.B = co.y; s.C = co.z;
    s.flags = (co.w < ALPHA_MIN ? 1u : 0u)                      // alpha <= op < 1/255 at every pixel, exactly
            | ((!(co.x > 0.0f) || !(co.z > 0.0f)) ? 2u : 0u);   // degenerate conic: no claim
    s.rBC = rBC;
    s.rBA = rBA;
    const float t = 255.0f * co.w;
    const uint32_t bits = __float_as_uint(t);
    const float e = (float)((int)((bits >> 23) & 0xffu) - 127);
    const float m = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u);
    s.tau = 1.3862944f * (e + (m - 1.0f) + 0.0861f);
    return s;
}

__device__ __forceinline__ CullSplat make_cull_splat(float2 xy, float4 co) {
    return make_cull_splat(xy, co, co.y / co.z, co.y / co.x);
}

// rectangle of pixel CENTRES [x0,x1] x [y0,y1] (inclusive)
__device__ __forceinline__ bool rect_may_contribute(const CullSplat& s, float x0, float y0, float x1, float y1) {
    if (s.flags & 1u) return false;
    if (s.flags & 2u) return true;
    if (s.mx >= x0 && s.mx <= x1 && s.my >= y0 && s.my <= y1) return true;
    const float dx0 = x0 - s.mx, dx1 = x1 - s.mx, dy0 = y0 - s.my, dy1 = y1 - s.my;
    // q grows along every ray from the centre: its minimum over the rectangle lies on an edge FACING the centre
    // (an axis whose range contains the centre has no facing edge; the one taken then only adds a larger candidate)
    const float dxn = s.mx < x0 ? dx0 : dx1, dyn = s.my < y0 ? dy0 : dy1;
    const float q = fminf(edge_min_q(s.A, s.B, s.C, s.rBC, dxn, dy0, dy1), edge_min_q(s.C, s.B, s.A, s.rBA, dyn, dx0, dx1));
    const float DX = fmaxf(fabsf(dx0), fabsf(dx1)), DY = fmaxf(fabsf(dy0), fabsf(dy1));
    const float M = s.A * DX * DX + 2.0f * fabsf(s.B) * DX * DY + s.C * DY * DY;
    return !(q > s.tau + 0.00001f * M + 0.01f);       // a NaN anywhere keeps the instance
}

__device__ __forceinline__ bool tile_may_contribute(const CullSplat& s, int tx, int ty, int W, int H) {
    const float x0 = (float)(tx * TILE), y0 = (float)(ty * TILE);
    const float x1 = fminf(x0 + (float)(TILE - 1), (float)(W - 1));
    const float y1 = fminf(y0 + (float)(TILE - 1), (float)(H - 1));
    return rect_may_contribute(s, x0, y0, x1, y1);
}

// ---- the compositor's skip test ----------------------------------------------------------------
// The compositor parks a list entry only if it may count at one of the wave's pixels.  An entry that counts nowhere
// blends with weight 0 at every pixel (fma(c, 0, C) == C) and moves no pixel state, so WHICH conservative test decides
// the parking changes no output bit: this test need not reproduce the oracle's list decisions, and it is built for few
// instructions, not for bit-reproducibility (it uses v_log_f32 on the device and log2f on the host).
//
// Contract.  May return true for anything.  Returns false only if NO pixel centre (px, py) of [x0,x1] x [y0,y1] reaches
// `power <= 0 && alpha >= 1/255` in the pair loop's fp32 arithmetic (power = fl(-q/2), alpha = min(0.99, op * exp(power)),
// q = A dx^2 + 2 B dx dy + C dy^2 over the offsets dx = px - mx, dy = py - my).  Precondition: x0 <= x1, y0 <= y1,
// rBC = fl(B / C), rBA = fl(B / A) (the record's last two floats).
//
// Soundness, step by step.  Offsets below are box minus centre; D^2 = dx0^2 + dx1^2 + dy0^2 + dy1^2 (at least the
// square of the largest offset of a box point along either axis, and a sum so that a NaN offset stays a NaN),
// S = A + C + 2 |B|, M = S D^2: every product A dx^2, 2 B dx dy, C dy^2 at a point of the box is at most M in magnitude.
//  (1) Guard.  !(min(A, C) > 0) returns true: from here on A, C > 0 or one of them is a NaN (min drops it), which
//      (7) keeps.
//  (2) Candidates.  dxc = med3(0, dx0, dx1) is the x offset of the box nearest the centre, dyc likewise.
//      e1 = min over dy in [dy0,dy1] of q(dxc, dy), e2 = min over dx in [dx0,dx1] of q(dx, dyc): with C > 0 (A > 0)
//      each is a convex parabola whose minimiser -dxc B / C (-dyc B / A) is clamped into the range.
//  (3) min(e1, e2) <= max(q(P), 0) for every box point P.  Centre inside the box: dxc = dyc = 0 and
//      e1 <= q(0, 0) = 0.  Centre outside: let P' = lambda P be the point where the segment from the centre to P
//      enters the box, 0 < lambda <= 1.  q(lambda P) = lambda^2 q(P), so q(P') <= max(q(P), 0).  P' lies on an edge that FACES
//      the centre -- dx = dx0 if dx0 > 0, dx = dx1 if dx1 < 0, and the same in y -- which is the segment dx = dxc,
//      dy in [dy0,dy1] with dxc != 0 (then e1 <= q(P')) or dy = dyc, dx in [dx0,dx1] with dyc != 0 (then e2 <= q(P')).
//      Along an axis whose range contains the centre (dxc = 0) the candidate is taken on the line through the centre
//      instead: one more candidate can only lower the minimum, and being a value of q at a point of the box it does
//      not lower it below the box's own minimum.  So a skip (min(e1, e2) > thr) means max(q(P), 0) > thr at every
//      point: q(P) > thr, or thr < 0, which by (6) needs op < 1/255 -- no pixel counts then.  No definiteness test is
//      needed: a conic that is not positive definite only makes q(P) < 0 possible, which this covers.
//  (4) Rounding of the candidates.  The clamped minimiser t is computed from rBC (two roundings): evaluating the
//      parabola at t instead of at the exact minimiser raises the value by C (t - t*)^2 <= C D^2 2^-44.  A NaN from
//      0 * inf (rBC overflowed: |B| > 3.4e38 C) makes med3 return the range's lower end; with d = 0 the value is then
//      C t^2 <= C D^2 < 2 |B| D^2 / 6.8e38 <= M 2^-128.  The value itself, fmaf(t, fmaf(C, t, (B + B) d), (A d) d), is
//      five roundings of terms bounded by M: within 5 * 2^-24 M of the exact parabola at t.
//  (5) The pair loop's power at a pixel of the box is -q/2 within 4 * 2^-24 M/2, its exp2 argument carries 2^-23
//      relative error more (<= 2^-23 * 0.73 M), v_exp_f32 and the product with op are 1 ulp each (2.4e-7 in ln alpha).
//      (4) and (5) together are below 1e-6 M + 1e-6 in units of q: the margin 1e-5 M (rect_may_contribute's 0.00001, on an M that is
//      not smaller than rect_may_contribute's A DX^2 + 2|B| DX DY + C DY^2) and part of the absolute 0.01 cover them.
//  (6) Threshold.  alpha >= 1/255 needs op * exp(-q/2) >= 1/255, i.e. q <= 2 ln(255 op) = 2 ln 2 * log2(255 op).
//      L = log2(fl(255 op)) within 1 ulp (v_log_f32 / log2f) plus 2^-24 * 1.45 from the product; |L| <= 136, so L and
//      the product TAU_K * L are within 2.3e-5 and 1.6e-5 absolute.  TAU_K = 1.3862944f exceeds 2 ln 2 by 3.8e-9: for
//      L >= 0 that only raises the bound; for L < 0 (op < 1/255: alpha < 1/255 at every pixel, nothing to protect)
//      it lowers it by at most 5.2e-7.  TAU_ABS = 0.0101 = rect_may_contribute's 0.01 + 1e-4 for all of that.
//  (7) Poison.  A NaN in A, B, C or the centre reaches M and with it the threshold (min(e1, e2) may drop a NaN, the
//      threshold cannot), a NaN in op reaches it through L, and !(q > NaN) keeps the entry.  An infinite A, B, C or
//      centre makes M (and the threshold) +inf or NaN: kept.  op = +inf: threshold +inf, kept.  op = 0 or (device)
//      denormal: L = -inf, every finite q clears it -- skipped, rightly: alpha <= op < 1/255.  op < 0: L = NaN, kept.
//      Intermediate overflow: every intermediate is bounded by M up to rounding, so it can only overflow with
//      M >= 3.4e38 / 1.0001, where the threshold exceeds 3e33 and the exact q does too, or M = inf (kept).
constexpr float QUARTER_TAU_K = 1.3862944f;      // the float above 2 ln 2
constexpr float QUARTER_TAU_ABS = 0.0101f;
constexpr float QUARTER_MARGIN = 0.00001f;

__host__ __device__ __forceinline__ float cull_med3(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(a, b, c);
#else
    return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));      // a NaN in `a` alone returns min(b, c), like v_med3_f32
#endif
}

__host__ __device__ __forceinline__ float cull_log2(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_logf(v);                       // v_log_f32: 1 ulp, a denormal argument counts as 0
#else
    return log2f(v);
#endif
}

// min(a, b) as the bare instruction: fminf() on a loaded value costs a canonicalising v_max per operand first.  Like fminf
// it returns the other operand for a NaN.
__host__ __device__ __forceinline__ float cull_min_raw(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    float m;
    asm("v_min_f32 %0, %1, %2" : "=v"(m) : "v"(a), "v"(b));
    return m;
#else
    return fminf(a, b);
#endif
}

// minimum over t in [lo,hi] of  A d^2 + 2 B d t + C t^2,  r = B / C
__host__ __device__ __forceinline__ float quarter_edge_min(float A, float B2, float C, float r, float d, float lo, float hi) {
    const float t = cull_med3(-(d * r), lo, hi);
    return fmaf(t, fmaf(C, t, B2 * d), (A * d) * d);
}

// rectangle of pixel CENTRES [x0,x1] x [y0,y1] (inclusive)
__host__ __device__ __forceinline__ bool quarter_may_contribute(float mx, float my, float A, float B, float C, float op,
                                                                float rBC, float rBA, float x0, float y0, float x1, float y1) {
    const float dx0 = x0 - mx, dx1 = x1 - mx, dy0 = y0 - my, dy1 = y1 - my;
    const float dxc = cull_med3(0.0f, dx0, dx1), dyc = cull_med3(0.0f, dy0, dy1);
    const float B2 = B + B;
    const float q = fminf(quarter_edge_min(A, B2, C, rBC, dxc, dy0, dy1), quarter_edge_min(C, B2, A, rBA, dyc, dx0, dx1));
    const float D2 = fmaf(dx0, dx0, fmaf(dx1, dx1, fmaf(dy0, dy0, dy1 * dy1)));      // (a max would drop a NaN)
    const float M = fmaf(2.0f, fabsf(B), A + C) * D2;
    const float thr = fmaf(QUARTER_MARGIN, M, fmaf(QUARTER_TAU_K, cull_log2(255.0f * op), QUARTER_TAU_ABS));
    return !(cull_min_raw(A, C) > 0.0f) || !(q > thr);
}


}  // namespace pgr
