// undistort.hip.h -- undistortion of COLMAP projects: the camera models, their inverse, the image remap
// and the box pyramid.  Included by io.hip only.
//
// THE RULE (float64 throughout; the build compiles with contraction off, so every line below is the expression tree):
//   Pixel (x, y) has its centre at image coordinates (x + 0.5, y + 0.5).  A camera is fx, fy, cx, cy and up to 8 coefficients.
//   distort(u, v) -> (du, dv), with u2 = u u, v2 = v v, r2 = u2 + v2, uv = u v, r4 = r2 r2, r6 = r4 r2:
//     pinhole        du = dv = 0
//     SIMPLE_RADIAL  rad = k r2;                          du = u rad;  dv = v rad
//     RADIAL         rad = k1 r2 + k2 r4;                 du = u rad;  dv = v rad
//     OPENCV         rad = k1 r2 + k2 r4;                 du = (u rad + ((2 p1) uv)) + p2 (r2 + 2 u2)
//                                                         dv = (v rad + ((2 p2) uv)) + p1 (r2 + 2 v2)
//     FULL_OPENCV    rad = (((1 + k1 r2) + k2 r4) + k3 r6) / (((1 + k4 r2) + k5 r4) + k6 r6)
//                                                         du = ((u rad + ((2 p1) uv)) + p2 (r2 + 2 u2)) - u;  dv likewise
//     OPENCV_FISHEYE r = sqrt(r2); zero when r < 1e-12; t = atan(r); t2 = t t; t4 = t2 t2; t6 = t4 t2; t8 = t4 t4;
//                    td = t ((((1 + k1 t2) + k2 t4) + k3 t6) + k4 t8);  s = td / r - 1;  du = u s;  dv = v s
//   Image coordinates: X = fx (u + du) + cx, Y = fy (v + dv) + cy.
//   Inverse: Newton on F(x) = (x + d(x)) - x_d with the analytic Jacobian J = I + dd/dx, from x = x_d, at most 100 steps:
//     step = J^-1 F by Cramer's rule; x -= step; converged when |step|^2 < 1e-20.  A step whose Jacobian has det <= 0 or trace <= 0
//     ends the point as failed: the iterate has left the sheet of the distortion that holds the origin, and a root found
//     beyond a fold is a wrong one.  A converged point is ok when |(x + d(x)) - x_d|_inf <= 1e-12 max(1, |x_d|_inf).
//     A point that is not ok is NaN, NaN with flag 0.
//   Remap of output pixel (x, y) of a job: u = ((x + 0.5) - cx') / fx', v likewise; (X, Y) as above with the SOURCE camera;
//     sx = X - 0.5, sy = Y - 0.5.  Inside when 0 <= sx <= w - 1 and 0 <= sy <= h - 1 (a NaN is outside): x0 = floor(sx),
//     ax = sx - x0, x1 = min(x0 + 1, w - 1) (the clamp only meets ax = 0), the same in y;
//     val = (1 - ay) ((1 - ax) p00 + ax p01) + ay ((1 - ax) p10 + ax p11); byte = min(255, floor(val + 0.5)).  Outside: 0.
//   Box mean of factor f: out = (sum of the f x f source bytes + f f / 2) / (f f) in integers, per channel.
//
// THE KERNELS.  und_points_kernel / und_distort_kernel: one lane per point.  und_remap_kernel and und_box_kernel: a job table
// in the kernel arguments (job_table.hip.h), a workgroup is 64 lanes across by 4 rows, a lane makes 4 consecutive pixels of a
// row and stores them as whole dwords (1, 3 or 4 for gray, RGB, RGBA) when all four exist and the address allows, bytewise
// otherwise.  The model and the channel count are template parameters: the pixel loop holds no switch, and the job's cameras
// are wave-uniform kernel arguments (scalar registers).  Taps are byte loads through the cache; nothing uses LDS.
#pragma once
#include "job_table.hip.h"       // pose_job_of_block
#include "pgr_common.h"

namespace pgr {

constexpr int UND_THREADS = 256;
constexpr int UND_LANES_X = 64;                      // lanes across a row: one wave
constexpr int UND_ROWS = UND_THREADS / UND_LANES_X;  // rows of a workgroup
constexpr int UND_PX = 4;                            // pixels of a lane
constexpr int UND_BLOCK_W = UND_LANES_X * UND_PX;    // 256 pixels
constexpr int UND_JOBS_PER_LAUNCH = 16;              // 184 B each: the table stays under the 4 KiB of kernel arguments
constexpr int UND_NEWTON_STEPS = 100;

enum UndModel : int { UND_PINHOLE = 0, UND_SIMPLE_RADIAL, UND_RADIAL, UND_OPENCV, UND_FULL_OPENCV, UND_FISHEYE, UND_MODELS };

struct UndCam {
    double fx, fy, cx, cy;
    double k[8];        // SIMPLE_RADIAL k; RADIAL k1 k2; OPENCV k1 k2 p1 p2; FULL_OPENCV k1 k2 p1 p2 k3 k4 k5 k6; FISHEYE k1..k4
};

struct UndJobDev {
    const uint8_t* src;
    uint8_t* dst;
    int64_t src_stride, dst_stride;
    int32_t sw, sh, dw, dh;
    uint32_t block0;                                 // first workgroup of the job in the launch
    uint32_t blocks_x;                               // workgroups across a row of the job
    UndCam cam;                                      // the source camera
    double pfx, pfy, pcx, pcy;                       // the output pinhole
};

struct UndJobTable {
    int32_t count, factor;
    int32_t pad[2];
    UndJobDev job[UND_JOBS_PER_LAUNCH];
};
static_assert(sizeof(UndJobTable) <= 3840, "UndJobTable must fit the kernel argument segment");

template <int M>
__host__ __device__ __forceinline__ void und_distort(const UndCam& c, double u, double v, double& du, double& dv) {
    if constexpr (M == UND_PINHOLE) {
        du = 0.0; dv = 0.0;
    } else if constexpr (M == UND_FISHEYE) {
        const double r = sqrt(u * u + v * v);
        if (r < 1e-12) { du = 0.0; dv = 0.0; return; }
        const double t = atan(r);
        const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
        const double td = t * ((((1.0 + c.k[0] * t2) + c.k[1] * t4) + c.k[2] * t6) + c.k[3] * t8);
        const double s = td / r - 1.0;
        du = u * s; dv = v * s;
    } else {
        const double u2 = u * u, v2 = v * v, r2 = u2 + v2;
        if constexpr (M == UND_SIMPLE_RADIAL) {
            const double rad = c.k[0] * r2;
            du = u * rad; dv = v * rad;
        } else if constexpr (M == UND_RADIAL) {
            const double r4 = r2 * r2;
            const double rad = c.k[0] * r2 + c.k[1] * r4;
            du = u * rad; dv = v * rad;
        } else {
            const double uv = u * v, r4 = r2 * r2;
            const double p1 = c.k[2], p2 = c.k[3];
            if constexpr (M == UND_OPENCV) {
                const double rad = c.k[0] * r2 + c.k[1] * r4;
                du = (u * rad + ((2.0 * p1) * uv)) + p2 * (r2 + 2.0 * u2);
                dv = (v * rad + ((2.0 * p2) * uv)) + p1 * (r2 + 2.0 * v2);
            } else {
                const double r6 = r4 * r2;
                const double rad = (((1.0 + c.k[0] * r2) + c.k[1] * r4) + c.k[4] * r6) / (((1.0 + c.k[5] * r2) + c.k[6] * r4) + c.k[7] * r6);
                du = ((u * rad + ((2.0 * p1) * uv)) + p2 * (r2 + 2.0 * u2)) - u;
                dv = ((v * rad + ((2.0 * p2) * uv)) + p1 * (r2 + 2.0 * v2)) - v;
            }
        }
    }
}

// J = I + dd/dx with d = (u rad + tangential): rad and its derivative by r2 per model, then one formula
template <int M>
__host__ __device__ __forceinline__ void und_jacobian(const UndCam& c, double u, double v, double& j00, double& j01, double& j10, double& j11) {
    if constexpr (M == UND_PINHOLE) {
        j00 = 1.0; j01 = 0.0; j10 = 0.0; j11 = 1.0;
    } else {
        const double u2 = u * u, v2 = v * v, r2 = u2 + v2, uv = u * v;
        double rad = 0.0, drad = 0.0, p1 = 0.0, p2 = 0.0;
        if constexpr (M == UND_SIMPLE_RADIAL) {
            rad = c.k[0] * r2; drad = c.k[0];
        } else if constexpr (M == UND_RADIAL || M == UND_OPENCV) {
            rad = c.k[0] * r2 + c.k[1] * (r2 * r2);
            drad = c.k[0] + (2.0 * c.k[1]) * r2;
            if constexpr (M == UND_OPENCV) { p1 = c.k[2]; p2 = c.k[3]; }
        } else if constexpr (M == UND_FULL_OPENCV) {
            const double r4 = r2 * r2, r6 = r4 * r2;
            const double num = ((1.0 + c.k[0] * r2) + c.k[1] * r4) + c.k[4] * r6;
            const double den = ((1.0 + c.k[5] * r2) + c.k[6] * r4) + c.k[7] * r6;
            const double dnum = (c.k[0] + (2.0 * c.k[1]) * r2) + (3.0 * c.k[4]) * r4;
            const double dden = (c.k[5] + (2.0 * c.k[6]) * r2) + (3.0 * c.k[7]) * r4;
            rad = num / den - 1.0;
            drad = (dnum * den - num * dden) / (den * den);
            p1 = c.k[2]; p2 = c.k[3];
        } else {
            const double r = sqrt(r2);
            if (r >= 1e-12) {
                const double t = atan(r);
                const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
                const double td = t * ((((1.0 + c.k[0] * t2) + c.k[1] * t4) + c.k[2] * t6) + c.k[3] * t8);
                const double dtd = (((1.0 + (3.0 * c.k[0]) * t2) + (5.0 * c.k[1]) * t4) + (7.0 * c.k[2]) * t6) + (9.0 * c.k[3]) * t8;
                rad = td / r - 1.0;
                drad = ((dtd / (1.0 + r2)) * r - td) / (r2 * (2.0 * r));     // d(td / r)/dr / (2 r)
            }
        }
        const double cross = ((2.0 * uv) * drad + (2.0 * p1) * u) + (2.0 * p2) * v;
        j00 = 1.0 + (((rad + (2.0 * u2) * drad) + (2.0 * p1) * v) + (6.0 * p2) * u);
        j01 = cross;
        j10 = cross;
        j11 = 1.0 + (((rad + (2.0 * v2) * drad) + (2.0 * p2) * u) + (6.0 * p1) * v);
    }
}

// normalised (x, y) of the distorted normalised point (xd, yd); false (and NaN) when the rule above fails the point
template <int M>
__host__ __device__ __forceinline__ bool und_invert(const UndCam& c, double xd, double yd, double& x, double& y) {
    x = xd; y = yd;
    bool converged = false;
    for (int it = 0; it < UND_NEWTON_STEPS; ++it) {
        double du, dv, j00, j01, j10, j11;
        und_distort<M>(c, x, y, du, dv);
        und_jacobian<M>(c, x, y, j00, j01, j10, j11);
        const double det = j00 * j11 - j01 * j10;
        if (!(det > 0.0 && j00 + j11 > 0.0)) break;
        const double rx = (x + du) - xd, ry = (y + dv) - yd;
        const double sx = (j11 * rx - j01 * ry) / det, sy = (j00 * ry - j10 * rx) / det;
        x -= sx; y -= sy;
        if (sx * sx + sy * sy < 1e-20) { converged = true; break; }
    }
    bool ok = false;
    if (converged) {
        double du, dv;
        und_distort<M>(c, x, y, du, dv);
        const double res = fmax(fabs((x + du) - xd), fabs((y + dv) - yd));
        ok = res <= 1e-12 * fmax(1.0, fmax(fabs(xd), fabs(yd)));     // a NaN residual compares false
    }
    if (!ok) { x = __builtin_nan(""); y = x; }
    return ok;
}

// image points xy [n,2] -> normalised points uv [n,2], ok [n] (may be null)
template <int M>
__global__ __launch_bounds__(UND_THREADS) void und_points_kernel(const UndCam c, long long n, const double* __restrict__ xy,
                                                                double* __restrict__ uv, uint8_t* __restrict__ ok) {
    const long long i = (long long)blockIdx.x * UND_THREADS + threadIdx.x;
    if (i >= n) return;
    const double xd = (xy[2 * i] - c.cx) / c.fx, yd = (xy[2 * i + 1] - c.cy) / c.fy;
    double x, y;
    const bool good = und_invert<M>(c, xd, yd, x, y);
    uv[2 * i] = x; uv[2 * i + 1] = y;
    if (ok) ok[i] = good ? 1 : 0;
}

// normalised points uv [n,2] -> image points xy [n,2]
template <int M>
__global__ __launch_bounds__(UND_THREADS) void und_distort_kernel(const UndCam c, long long n, const double* __restrict__ uv,
                                                                 double* __restrict__ xy) {
    const long long i = (long long)blockIdx.x * UND_THREADS + threadIdx.x;
    if (i >= n) return;
    const double u = uv[2 * i], v = uv[2 * i + 1];
    double du, dv;
    und_distort<M>(c, u, v, du, dv);
    xy[2 * i] = c.fx * (u + du) + c.cx;
    xy[2 * i + 1] = c.fy * (v + dv) + c.cy;
}

// the UND_PX pixels of a lane, C bytes each, to `d`: n of them exist
template <int C>
__device__ __forceinline__ void und_store_pixels(uint8_t* d, const uint8_t (&b)[UND_PX * C], int n) {
    if (n == UND_PX && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
        uint32_t w[C];
#pragma unroll
        for (int i = 0; i < C; ++i)
            w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
        if constexpr (C == 4) {
            if ((reinterpret_cast<uintptr_t>(d) & 15) == 0) {
                *(PGR_GLOBAL u32x4_t*)d = u32x4_t{w[0], w[1], w[2], w[3]};
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < C; ++i) gstore(reinterpret_cast<uint32_t*>(d) + i, w[i]);
    } else {
        for (int i = 0; i < n * C; ++i) gstore(d + i, b[i]);
    }
}

// where a lane works: its job, its first pixel and its row; false when the lane has no pixel
__device__ __forceinline__ bool und_lane_place(const UndJobTable& T, int& k, int& x0, int& y) {
    k = pose_job_of_block(T, blockIdx.x);
    const UndJobDev& J = T.job[k];
    const uint32_t rel = blockIdx.x - J.block0;
    const uint32_t bx = rel % J.blocks_x, by = rel / J.blocks_x;
    x0 = (int)(bx * UND_BLOCK_W + (threadIdx.x % UND_LANES_X) * UND_PX);
    y = (int)(by * UND_ROWS + threadIdx.x / UND_LANES_X);
    return y < J.dh && x0 < J.dw;
}

template <int M, int C>
__global__ __launch_bounds__(UND_THREADS) void und_remap_kernel(const UndJobTable T) {
    int k, x0, y;
    if (!und_lane_place(T, k, x0, y)) return;
    const UndJobDev& J = T.job[k];
    const double v = (((double)y + 0.5) - J.pcy) / J.pfy;
    const double x_last = (double)(J.sw - 1), y_last = (double)(J.sh - 1);
    uint8_t out[UND_PX * C];
#pragma unroll
    for (int p = 0; p < UND_PX; ++p) {
        const double u = (((double)(x0 + p) + 0.5) - J.pcx) / J.pfx;
        double du, dv;
        und_distort<M>(J.cam, u, v, du, dv);
        const double sx = (J.cam.fx * (u + du) + J.cam.cx) - 0.5, sy = (J.cam.fy * (v + dv) + J.cam.cy) - 0.5;
        const bool inside = sx >= 0.0 && sx <= x_last && sy >= 0.0 && sy <= y_last;
        if (inside) {
            const double fx0 = floor(sx), fy0 = floor(sy);
            const double ax = sx - fx0, ay = sy - fy0;
            const int ix0 = (int)fx0, iy0 = (int)fy0;
            const int ix1 = min(ix0 + 1, J.sw - 1), iy1 = min(iy0 + 1, J.sh - 1);
            const uint8_t* r0 = J.src + (int64_t)iy0 * J.src_stride;
            const uint8_t* r1 = J.src + (int64_t)iy1 * J.src_stride;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const double p00 = (double)gload(r0 + ix0 * C + ch), p01 = (double)gload(r0 + ix1 * C + ch);
                const double p10 = (double)gload(r1 + ix0 * C + ch), p11 = (double)gload(r1 + ix1 * C + ch);
                const double val = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11);
                out[p * C + ch] = (uint8_t)min(255u, (uint32_t)floor(val + 0.5));
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) out[p * C + ch] = 0;
        }
    }
    und_store_pixels<C>(J.dst + (int64_t)y * J.dst_stride + (int64_t)x0 * C, out, min(UND_PX, J.dw - x0));
}

// T.factor x T.factor box means: the host has checked that dw * factor <= sw and dh * factor <= sh
template <int C>
__global__ __launch_bounds__(UND_THREADS) void und_box_kernel(const UndJobTable T) {
    int k, x0, y;
    if (!und_lane_place(T, k, x0, y)) return;
    const UndJobDev& J = T.job[k];
    const int f = T.factor;
    const uint32_t area = (uint32_t)(f * f);
    const int n = min(UND_PX, J.dw - x0);
    uint8_t out[UND_PX * C];
#pragma unroll
    for (int p = 0; p < UND_PX; ++p) {
        uint32_t sum[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) sum[ch] = 0;
        if (p < n) {
            for (int dy = 0; dy < f; ++dy) {
                const uint8_t* r = J.src + (int64_t)(y * f + dy) * J.src_stride + (int64_t)(x0 + p) * f * C;
                for (int dx = 0; dx < f; ++dx)
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) sum[ch] += gload(r + dx * C + ch);
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) out[p * C + ch] = (uint8_t)((sum[ch] + area / 2) / area);
    }
    und_store_pixels<C>(J.dst + (int64_t)y * J.dst_stride + (int64_t)x0 * C, out, n);
}

}  // namespace pgr
