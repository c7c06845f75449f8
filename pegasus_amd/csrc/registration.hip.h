// registration.hip.h -- rigid registration of one point cloud to another: nearest-neighbour correspondences under a pose, the
// sums of both ICP estimators, and normals by radius (open3d's evaluate_registration / registration_icp and
// estimate_normals(KDTreeSearchParamRadius(r)): /root/reference/submodules/aruco-estimator/aruco_estimator/utils.py:82-98,
// /root/reference/src/gs/ao_test.py:21).  Not on the render path.  DESIGN.md section 17 holds the rules and what was measured.
//
// The grid is radius.hip.h's, unchanged (insert, ranges, scatter, radius_cell, radius_key, RADIUS_CELL_MARGIN): it is built
// over the TARGET once per registration with the cell edge max_distance * RADIUS_CELL_MARGIN, and stays valid over the
// iterations because the target does not move.
//
// Correspondences.  One lane per source point.  s' = R s + t in float64: s is float32 widened exactly, T a row-major float64
// 4x4 that arrives by value, every coordinate ((r0*x + r1*y) + r2*z) + t with every operation rounded on its own.  The lane
// walks the 27 cells around s'; d2 = ((dx*dx) + dy*dy) + dz*dz with dx = q.x - s'.x (the float32 target widened exactly); the
// correspondent is the target of smallest d2, among equal d2 the one of lowest ORIGINAL index (the index rides in the sorted
// point's w), so neither the order of the cells nor the order in which the scatter's atomics landed can show.  It is accepted
// iff d2 < max_distance * max_distance, the product rounded once on the host, the comparison strict.
//
// No accepted pair lies more than one cell apart: radius.hip.h's argument with step (a) redone.  s' is a float64 that is not
// a float32, so dx = fl(q.x - s'.x) is rounded where it was exact there: the true |q.x - s'.x| <= |dx| (1 + u), which is the
// bound (a) already allowed for, and |q.x - s'.x| < max_distance (1 + 2^-51) stands.  The cell of s' is taken from the float64
// itself (registration_cell below: radius_cell's expression without the float32 argument, one rounding in t(x) as in (b)).
// Rounding s' to float32 first would not do: where a float32 ulp is a third of max_distance, s' = q + 0.9 r rounds to
// q + 1.05 r, which can lie two cells from q.  Domain: target coordinates and every s' finite with |x| / max_distance < 2^30
// (the caller's contract; pegasus_amd/registration.py checks it with one reduction per cloud); outside it the cell index is
// clamped, so every access stays in bounds and only the results are wrong.
//
// Lane order.  `order` (optional) names the source point of every lane: pgr_nn_source_order files the source under the
// initial pose into a grid of its own (the same three kernels) and returns the points in cell order, so that a wave probes
// the same slots and walks the same candidates; ICP moves the points little, so the order is made once.
//
// Sums.  One pass over the source in ROW order given `index`: a lane's 45 terms go through a shuffle tree per wave, the four
// waves of a workgroup are added in wave order, and one workgroup adds the workgroups' partials, each of its 16 waves a
// contiguous run of them in workgroup order, then a tree over the 16.  No floating-point atomics: equal inputs give equal
// bytes.  The count is a sum of ones in float64, exact below 2^53.
//
// Normals by radius.  One lane per point in cell order over a grid of the cloud itself (cell edge radius *
// RADIUS_CELL_MARGIN): the float64 second moments of the differences q - p over every q that passes radius_within (strict,
// the point itself included), the covariance from them, its eigenvectors by cyclic Jacobi sweeps.  The normal is the unit
// eigenvector of the smallest eigenvalue, signed so that its component of largest magnitude is positive; fewer than 3
// neighbours give (0, 0, 1).  The neighbour sums run in grid order, which follows the scatter's atomics: the counts are exact,
// the normals are NOT required to be bit-repeatable (they are held to an angle).
#pragma once
#include "radius.hip.h"

namespace pgr {

constexpr int REG_BLOCK = RADIUS_BLOCK;
constexpr int REG_SUMS = PGR_ICP_SUMS;             // doubles per partial and in the result (45 used)
constexpr int REG_FINAL_BLOCK = 1024;              // the second pass of the sums: 16 waves
// where the sums lie (pegasus_amd/registration.py reads the same numbers): the point-to-plane estimator needs [0, 32), the
// point-to-point estimator [16, 48)
constexpr int REG_JTJ = 0, REG_JTR = 21, REG_COUNT = 27, REG_D2 = 28, REG_S = 29, REG_Q = 32, REG_SQ = 35, REG_SS = 44;

struct RegPose { double r[9]; double t[3]; };

// radius_cell for a float64 coordinate (see the header comment: s' must not be rounded to float32 first)
__device__ __forceinline__ int registration_cell(double x, double inv_h) {
    const double t = floor(x * inv_h);
    return (int)fmin(fmax(t, -RADIUS_CELL_LIMIT), RADIUS_CELL_LIMIT);
}

__device__ __forceinline__ void registration_apply(const RegPose& T, const float* __restrict__ p, double& x, double& y, double& z) {
#pragma clang fp contract(off)
    const double sx = (double)p[0], sy = (double)p[1], sz = (double)p[2];
    const double ax = T.r[0] * sx, bx = T.r[1] * sy, cx = T.r[2] * sz;
    const double ay = T.r[3] * sx, by = T.r[4] * sy, cy = T.r[5] * sz;
    const double az = T.r[6] * sx, bz = T.r[7] * sy, cz = T.r[8] * sz;
    x = ((ax + bx) + cx) + T.t[0];
    y = ((ay + by) + cy) + T.t[1];
    z = ((az + bz) + cz) + T.t[2];
}

// the posed source as float32, only to be filed into a grid for the lane order (its rounding decides no result)
__global__ __launch_bounds__(REG_BLOCK) void registration_pose_kernel(int n, const float* __restrict__ src, RegPose T,
                                                                      float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    registration_apply(T, src + 3 * i, x, y, z);
    out[3 * i] = (float)x; out[3 * i + 1] = (float)y; out[3 * i + 2] = (float)z;
}

__global__ __launch_bounds__(REG_BLOCK) void registration_order_kernel(int n, const float4* __restrict__ sorted,
                                                                       int32_t* __restrict__ order) {
    const int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    if (i < n) order[i] = __float_as_int(sorted[i].w);
}

// nt == 0: no grid is read and every source point is without a correspondent
__global__ __launch_bounds__(REG_BLOCK) void registration_correspond_kernel(
    int ns, const float* __restrict__ src, const int32_t* __restrict__ order, RegPose T, int nt,
    const float4* __restrict__ sorted, const RadiusSlot* __restrict__ slots, const uint32_t* __restrict__ end, uint32_t mask,
    double inv_h, double r2, int32_t* __restrict__ index, double* __restrict__ d2_out) {
#pragma clang fp contract(off)
    const int64_t lane = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    if (lane >= ns) return;
    const uint32_t i = order ? (uint32_t)order[lane] : (uint32_t)lane;
    if (i >= (uint32_t)ns) return;                               // (a permutation never is; a bad one writes nothing)
    double best = INFINITY;
    int best_j = -1;
    if (nt > 0) {
        double x, y, z;
        registration_apply(T, src + 3 * (size_t)i, x, y, z);
        const int cx = registration_cell(x, inv_h), cy = registration_cell(y, inv_h), cz = registration_cell(z, inv_h);
        for (int c = 0; c < 27; ++c) {
            const RadiusKey k = radius_key(cx + c % 3 - 1, cy + c / 3 % 3 - 1, cz + c / 9 - 1);
            uint32_t at = k.hash & mask;
            uint32_t cell_count = 0;                             // 0: no such cell
            for (uint32_t probes = 0; probes <= mask; ++probes, at = (at + 1) & mask) {
                const RadiusSlot slot = slots[at];
                if (slot.xy == 0ull) break;
                if (slot.xy == k.xy && slot.z == k.z) { cell_count = slot.count; break; }
            }
            if (cell_count == 0) continue;
            const uint32_t last = min(end[at], (uint32_t)nt);    // (never more than nt: the counts sum to nt)
            for (uint32_t j = last - min(cell_count, last); j < last; ++j) {
                const float4 q = sorted[j];
                const double dx = (double)q.x - x, dy = (double)q.y - y, dz = (double)q.z - z;
                const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                const double xy = xx + yy;
                const double d2 = xy + zz;
                const int orig = __float_as_int(q.w);
                if (d2 < best || (d2 == best && orig < best_j)) { best = d2; best_j = orig; }
            }
        }
    }
    const bool hit = best_j >= 0 && best_j < nt && best < r2;
    index[i] = hit ? best_j : -1;
    d2_out[i] = hit ? best : 0.0;
}

// lane 0 of the wave ends up with the wave's sum, the same tree whatever the values
__device__ __forceinline__ double registration_wave_sum(double v) {
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_down(v, d, WAVE);
    return v;
}

// partials[blockIdx.x][REG_SUMS]: the workgroup's sums.  normals may be NULL: the point-to-plane terms are then 0.
__global__ __launch_bounds__(REG_BLOCK) void registration_sums_kernel(
    int ns, const float* __restrict__ src, RegPose T, const int32_t* __restrict__ index, const double* __restrict__ d2_in,
    int nt, const float* __restrict__ tgt, const double* __restrict__ normals, double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double wave_sums[REG_BLOCK / WAVE][REG_SUMS];
    const int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    double v[REG_SUMS];
#pragma unroll
    for (int k = 0; k < REG_SUMS; ++k) v[k] = 0.0;
    const int j = i < ns ? index[i] : -1;
    if ((uint32_t)j < (uint32_t)nt) {
        double s[3];
        registration_apply(T, src + 3 * i, s[0], s[1], s[2]);
        const double q[3] = {(double)tgt[3 * (size_t)j], (double)tgt[3 * (size_t)j + 1], (double)tgt[3 * (size_t)j + 2]};
        v[REG_COUNT] = 1.0;
        v[REG_D2] = d2_in[i];
        if (normals) {
            const double n[3] = {normals[3 * (size_t)j], normals[3 * (size_t)j + 1], normals[3 * (size_t)j + 2]};
            const double ex = s[0] - q[0], ey = s[1] - q[1], ez = s[2] - q[2];
            const double r = ((ex * n[0]) + ey * n[1]) + ez * n[2];
            const double J[6] = {s[1] * n[2] - s[2] * n[1], s[2] * n[0] - s[0] * n[2], s[0] * n[1] - s[1] * n[0],
                                 n[0], n[1], n[2]};
            int at = REG_JTJ;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) v[at++] = J[a] * J[b];
#pragma unroll
            for (int a = 0; a < 6; ++a) v[REG_JTR + a] = J[a] * r;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v[REG_S + a] = s[a];
            v[REG_Q + a] = q[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) v[REG_SQ + 3 * a + b] = s[a] * q[b];
        }
        v[REG_SS] = ((s[0] * s[0]) + s[1] * s[1]) + s[2] * s[2];
    }
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < REG_SUMS; ++k) {
        const double w = registration_wave_sum(v[k]);
        if (lane == 0) wave_sums[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < REG_SUMS) {
        double w = wave_sums[0][threadIdx.x];
#pragma unroll
        for (int g = 1; g < REG_BLOCK / WAVE; ++g) w += wave_sums[g][threadIdx.x];
        partials[(size_t)blockIdx.x * REG_SUMS + threadIdx.x] = w;
    }
}

// one workgroup: wave g adds partials [g * run, (g + 1) * run) in order, lane k term k; then a tree over the 16 waves
__global__ __launch_bounds__(REG_FINAL_BLOCK) void registration_sums_final_kernel(int blocks, const double* __restrict__ partials,
                                                                                  double* __restrict__ sums) {
#pragma clang fp contract(off)
    constexpr int WAVES = REG_FINAL_BLOCK / WAVE;
    __shared__ double part[WAVES][WAVE];
    const int k = threadIdx.x & (WAVE - 1), g = threadIdx.x / WAVE;
    const int run = (blocks + WAVES - 1) / WAVES;
    double w = 0.0;
    if (k < REG_SUMS)
        for (int b = g * run; b < min((g + 1) * run, blocks); ++b) w += partials[(size_t)b * REG_SUMS + k];
    part[g][k] = w;
    __syncthreads();
#pragma unroll
    for (int d = WAVES / 2; d >= 1; d >>= 1) {
        if (g < d) part[g][k] += part[g + d][k];
        __syncthreads();
    }
    if (g == 0 && k < REG_SUMS) sums[k] = part[0][k];
}

// One Jacobi rotation of the symmetric 3x3 A (full storage) in the (P, Q) plane, accumulated into the eigenvector columns V.
template <int P, int Q>
__device__ __forceinline__ void registration_jacobi_rotate(double (&A)[3][3], double (&V)[3][3]) {
    constexpr int R = 3 - P - Q;
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    const double arp = A[R][P], arq = A[R][Q];
    A[R][P] = A[P][R] = c * arp - s * arq;
    A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = V[k][P], vq = V[k][Q];
        V[k][P] = c * vp - s * vq;
        V[k][Q] = s * vp + c * vq;
    }
}

constexpr int REG_JACOBI_SWEEPS = 12;              // a 3x3 is at rounding level after 5 or 6; the rest find nothing to rotate

// one lane per point, in cell order.  `end`: the scatter's cursors, each one past its cell's last point.
__global__ __launch_bounds__(REG_BLOCK) void registration_normals_kernel(int n, const float4* __restrict__ sorted,
                                                                         const RadiusSlot* __restrict__ slots,
                                                                         const uint32_t* __restrict__ end, uint32_t mask,
                                                                         double inv_h, double r2, double* __restrict__ normals,
                                                                         int32_t* __restrict__ counts) {
    const int64_t s = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    if (s >= n) return;
    const float4 p = sorted[s];
    const int cx = radius_cell(p.x, inv_h), cy = radius_cell(p.y, inv_h), cz = radius_cell(p.z, inv_h);
    int count = 0;
    double m[3] = {0.0, 0.0, 0.0}, mm[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // sums of d and of xx, xy, xz, yy, yz, zz
    for (int c = 0; c < 27; ++c) {
        const RadiusKey k = radius_key(cx + c % 3 - 1, cy + c / 3 % 3 - 1, cz + c / 9 - 1);
        uint32_t at = k.hash & mask;
        uint32_t cell_count = 0;
        for (uint32_t probes = 0; probes <= mask; ++probes, at = (at + 1) & mask) {
            const RadiusSlot slot = slots[at];
            if (slot.xy == 0ull) break;
            if (slot.xy == k.xy && slot.z == k.z) { cell_count = slot.count; break; }
        }
        if (cell_count == 0) continue;
        const uint32_t last = min(end[at], (uint32_t)n);
        for (uint32_t j = last - min(cell_count, last); j < last; ++j) {
            const float4 q = sorted[j];
            if (!radius_within(p, q, r2)) continue;
            const double dx = (double)q.x - (double)p.x, dy = (double)q.y - (double)p.y, dz = (double)q.z - (double)p.z;
            ++count;
            m[0] += dx; m[1] += dy; m[2] += dz;
            mm[0] += dx * dx; mm[1] += dx * dy; mm[2] += dx * dz; mm[3] += dy * dy; mm[4] += dy * dz; mm[5] += dz * dz;
        }
    }
    double nx = 0.0, ny = 0.0, nz = 1.0;
    if (count >= 3) {
        const double inv = 1.0 / (double)count;
        const double ex = m[0] * inv, ey = m[1] * inv, ez = m[2] * inv;
        double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        A[0][0] = mm[0] * inv - ex * ex;
        A[0][1] = A[1][0] = mm[1] * inv - ex * ey;
        A[0][2] = A[2][0] = mm[2] * inv - ex * ez;
        A[1][1] = mm[3] * inv - ey * ey;
        A[1][2] = A[2][1] = mm[4] * inv - ey * ez;
        A[2][2] = mm[5] * inv - ez * ez;
        // scaled to a largest entry of 1, so that no product below under- or overflows whatever the radius
        const double big = fmax(fmax(fabs(A[0][0]), fabs(A[1][1])), fmax(fmax(fabs(A[0][1]), fabs(A[0][2])), fmax(fabs(A[1][2]), fabs(A[2][2]))));
        if (big > 0.0) {
            const double scale = 1.0 / big;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) A[a][b] *= scale;
            for (int sweep = 0; sweep < REG_JACOBI_SWEEPS; ++sweep) {
                registration_jacobi_rotate<0, 1>(A, V);
                registration_jacobi_rotate<0, 2>(A, V);
                registration_jacobi_rotate<1, 2>(A, V);
            }
        }
        // the smallest eigenvalue, the lowest column among equal ones
        // (selects, not a column index: an indexed read would put V into scratch memory)
        const bool second = A[1][1] < A[0][0];
        const bool third = A[2][2] < (second ? A[1][1] : A[0][0]);
        double vx = third ? V[0][2] : (second ? V[0][1] : V[0][0]);
        double vy = third ? V[1][2] : (second ? V[1][1] : V[1][0]);
        double vz = third ? V[2][2] : (second ? V[2][1] : V[2][0]);
        const double len = sqrt(vx * vx + vy * vy + vz * vz);
        if (len > 0.0) {
            vx /= len; vy /= len; vz /= len;
            // the component of largest magnitude (the first among equal ones) is positive
            double lead = vx;
            if (fabs(vy) > fabs(lead)) lead = vy;
            if (fabs(vz) > fabs(lead)) lead = vz;
            const double sign = lead < 0.0 ? -1.0 : 1.0;
            nx = sign * vx; ny = sign * vy; nz = sign * vz;
        }
    }
    const int orig = __float_as_int(p.w);
    if ((uint32_t)orig < (uint32_t)n) {
        normals[3 * (size_t)orig] = nx; normals[3 * (size_t)orig + 1] = ny; normals[3 * (size_t)orig + 2] = nz;
        counts[orig] = count;
    }
}

}  // namespace pgr
