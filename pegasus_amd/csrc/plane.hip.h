// plane.hip.h -- the dominant plane of a point cloud by RANSAC (open3d's segment_plane, which the reference's
// ReconstructionAlignment.align2plane rests on: /root/reference/src/reconstruction/environment_reconstruction.py:53-66).  Not on
// the render path.  DESIGN.md section 18 holds the rules and what was measured.
//
// Hypotheses.  One lane per triple of point rows (i0, i1, i2).  The float32 points widened exactly to float64, every operation
// rounded on its own: e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2 (each component (a*b) - (c*d)), norm = sqrt(((cx*cx) + cy*cy) +
// cz*cz), nrm = c / norm, d = -(((nx*x0) + ny*y0) + nz*z0).  A triple with a row outside [0, n) or with two equal rows is never
// dereferenced; it, a norm of 0 and a norm that is not finite give the plane (0, 0, 0, 0) and valid = 0.
//
// Scores.  dist = |((nx*x + ny*y) + nz*z) + d| in float64, every operation rounded on its own; the point is an inlier iff
// dist < threshold, STRICTLY; a hypothesis scores the count of its inliers (int32, exact) and the sum of their dist*dist
// (float64).  A plane of four zeros scores 0 and 0.  Every hypothesis is scored on every point: nothing is subsampled and
// nothing stops early.
//
// plane_score_kernel.  A workgroup of PLANE_BLOCK lanes owns PLANE_BLOCK * PLANE_POINTS_PER_LANE consecutive points, read from
// memory once per call -- once per group of hypothesis batches where the cloud alone has too few tiles to fill the chip
// (PLANE_SCORE_MIN_BLOCKS) -- and kept as float64 in registers (lane t holds rows base + k * PLANE_BLOCK + t, so the loads of
// a wave are consecutive; a row past n is held as NaN, which fails the strict comparison under every plane).  The hypotheses
// pass by in batches of PLANE_HYP_BATCH through LDS: every lane reads the same four doubles, a broadcast.  Per hypothesis a
// lane adds its own count and sum over its points in the order k = 0, 1, ..; the wave adds the lanes in a fixed shuffle tree;
// the waves of the workgroup are added in wave order; the workgroup's partials [blocks, n_hyp] go to the workspace and
// plane_score_final_kernel adds them in workgroup order, one lane per hypothesis.  No floating-point atomics: equal inputs
// give equal bytes.
//
// plane_inliers_kernel.  One pass over the points under ONE plane (by value): the mask (optional), and PLANE_SUMS terms per
// point with q = p - pivot in float64 -- 1, q, the upper triangle of q q^T row by row, dist*dist, 0 -- through the reduction of
// registration_sums_kernel: a shuffle tree per wave, the waves in wave order, then one workgroup over the partials in
// workgroup order.  The count is a sum of ones in float64, exact below 2^53.
#pragma once
#include "registration.hip.h"

namespace pgr {

constexpr int PLANE_BLOCK = 256;
constexpr int PLANE_POINTS_PER_LANE = 8;
constexpr int PLANE_HYP_BATCH = 64;
constexpr int PLANE_TILE = PLANE_BLOCK * PLANE_POINTS_PER_LANE;   // points of one workgroup of plane_score_kernel
constexpr int PLANE_WAVES = PLANE_BLOCK / WAVE;
constexpr int PLANE_SUM_TERMS = PGR_PLANE_SUMS;                   // doubles per partial and in the result (11 used)
constexpr int PLANE_FINAL_BLOCK = 1024;                           // the second pass of the inlier sums: 16 waves
// a cloud of fewer tiles than this spreads the batches of hypotheses over gridDim.y, so that the launch still fills the chip
// (every group then reads the points once more; a result does not depend on it)
constexpr int PLANE_SCORE_MIN_BLOCKS = 1024;
static_assert(PLANE_HYP_BATCH * 4 <= PLANE_BLOCK, "one lane per double of a batch of planes");
static_assert(PLANE_HYP_BATCH <= PLANE_BLOCK && PLANE_SUM_TERMS <= WAVE, "one lane per partial");

struct PlaneModel { double n[3]; double d; double pivot[3]; };

__device__ __forceinline__ double plane_distance(double nx, double ny, double nz, double d, double x, double y, double z) {
#pragma clang fp contract(off)
    const double a = nx * x, b = ny * y, c = nz * z;
    const double ab = a + b;
    const double abc = ab + c;
    return fabs(abc + d);
}

// one lane per hypothesis
__global__ __launch_bounds__(PLANE_BLOCK) void plane_hypotheses_kernel(int n, const float* __restrict__ xyz, int n_hyp,
                                                                       const int32_t* __restrict__ triples,
                                                                       double* __restrict__ planes, uint8_t* __restrict__ valid) {
#pragma clang fp contract(off)
    const int h = blockIdx.x * PLANE_BLOCK + threadIdx.x;
    if (h >= n_hyp) return;
    const int32_t i0 = triples[3 * (size_t)h], i1 = triples[3 * (size_t)h + 1], i2 = triples[3 * (size_t)h + 2];
    double nx = 0.0, ny = 0.0, nz = 0.0, d = 0.0;
    bool ok = (uint32_t)i0 < (uint32_t)n && (uint32_t)i1 < (uint32_t)n && (uint32_t)i2 < (uint32_t)n && i0 != i1 && i0 != i2 &&
              i1 != i2;
    if (ok) {
        const float* p0 = xyz + 3 * (size_t)i0;
        const float* p1 = xyz + 3 * (size_t)i1;
        const float* p2 = xyz + 3 * (size_t)i2;
        const double x0 = (double)p0[0], y0 = (double)p0[1], z0 = (double)p0[2];
        const double ax = (double)p1[0] - x0, ay = (double)p1[1] - y0, az = (double)p1[2] - z0;
        const double bx = (double)p2[0] - x0, by = (double)p2[1] - y0, bz = (double)p2[2] - z0;
        const double cx = (ay * bz) - (az * by), cy = (az * bx) - (ax * bz), cz = (ax * by) - (ay * bx);
        const double norm = sqrt(((cx * cx) + cy * cy) + cz * cz);
        ok = norm != 0.0 && isfinite(norm);
        if (ok) {
            nx = cx / norm; ny = cy / norm; nz = cz / norm;
            d = -(((nx * x0) + ny * y0) + nz * z0);
        }
    }
    planes[4 * (size_t)h] = nx; planes[4 * (size_t)h + 1] = ny; planes[4 * (size_t)h + 2] = nz; planes[4 * (size_t)h + 3] = d;
    valid[h] = ok ? 1 : 0;
}

// lane 0 of the wave ends up with the wave's sum, the same tree whatever the values
__device__ __forceinline__ int plane_wave_sum(int v) {
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_down(v, d, WAVE);
    return v;
}

// part_sumsq, part_count: [gridDim.x, n_hyp].  Workgroup (x, y) scores batches [y * batches_per_group, (y + 1) *
// batches_per_group) of the hypotheses on tile x of the points.
__global__ __launch_bounds__(PLANE_BLOCK) void plane_score_kernel(int n, const float* __restrict__ xyz, int n_hyp,
                                                                  const double* __restrict__ planes, double threshold,
                                                                  int batches_per_group, double* __restrict__ part_sumsq,
                                                                  int32_t* __restrict__ part_count) {
#pragma clang fp contract(off)
    __shared__ double s_plane[PLANE_HYP_BATCH * 4];
    __shared__ double s_sumsq[PLANE_WAVES][PLANE_HYP_BATCH];
    __shared__ int32_t s_count[PLANE_WAVES][PLANE_HYP_BATCH];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
    const int64_t base = (int64_t)blockIdx.x * PLANE_TILE;
    double px[PLANE_POINTS_PER_LANE], py[PLANE_POINTS_PER_LANE], pz[PLANE_POINTS_PER_LANE];
#pragma unroll
    for (int k = 0; k < PLANE_POINTS_PER_LANE; ++k) {
        const int64_t i = base + (int64_t)k * PLANE_BLOCK + t;
        const bool in = i < n;
        px[k] = in ? (double)xyz[3 * i] : (double)NAN;
        py[k] = in ? (double)xyz[3 * i + 1] : (double)NAN;
        pz[k] = in ? (double)xyz[3 * i + 2] : (double)NAN;
    }
    const int64_t group_first = (int64_t)blockIdx.y * batches_per_group * PLANE_HYP_BATCH;
    const int group_end = (int)min((int64_t)n_hyp, group_first + (int64_t)batches_per_group * PLANE_HYP_BATCH);
    for (int first = (int)min(group_first, (int64_t)n_hyp); first < group_end; first += PLANE_HYP_BATCH) {
        const int batch = min(PLANE_HYP_BATCH, group_end - first);
        __syncthreads();                                         // the batch before has been read and added up
        if (t < 4 * batch) s_plane[t] = planes[4 * (size_t)first + t];
        __syncthreads();
        for (int h = 0; h < batch; ++h) {
            const double nx = s_plane[4 * h], ny = s_plane[4 * h + 1], nz = s_plane[4 * h + 2], d = s_plane[4 * h + 3];
            int count = 0;
            double sumsq = 0.0;
            if (nx != 0.0 || ny != 0.0 || nz != 0.0 || d != 0.0) {       // (the same for every lane)
#pragma unroll
                for (int k = 0; k < PLANE_POINTS_PER_LANE; ++k) {
                    const double dist = plane_distance(nx, ny, nz, d, px[k], py[k], pz[k]);
                    const bool in = dist < threshold;             // false for the NaN of a row past n
                    count += in ? 1 : 0;
                    sumsq += in ? dist * dist : 0.0;
                }
            }
            count = plane_wave_sum(count);
            sumsq = registration_wave_sum(sumsq);
            if (lane == 0) { s_count[wave][h] = count; s_sumsq[wave][h] = sumsq; }
        }
        __syncthreads();
        if (t < batch) {
            int count = s_count[0][t];
            double sumsq = s_sumsq[0][t];
#pragma unroll
            for (int g = 1; g < PLANE_WAVES; ++g) { count += s_count[g][t]; sumsq += s_sumsq[g][t]; }
            const size_t at = (size_t)blockIdx.x * n_hyp + first + t;
            part_count[at] = count;
            part_sumsq[at] = sumsq;
        }
    }
}

// one lane per hypothesis: the workgroups' partials in workgroup order
__global__ __launch_bounds__(PLANE_BLOCK) void plane_score_final_kernel(int blocks, int n_hyp, const double* __restrict__ part_sumsq,
                                                                        const int32_t* __restrict__ part_count,
                                                                        int32_t* __restrict__ counts, double* __restrict__ sumsq) {
#pragma clang fp contract(off)
    const int h = blockIdx.x * PLANE_BLOCK + threadIdx.x;
    if (h >= n_hyp) return;
    int count = 0;
    double sum = 0.0;
    for (int b = 0; b < blocks; ++b) {
        count += part_count[(size_t)b * n_hyp + h];
        sum += part_sumsq[(size_t)b * n_hyp + h];
    }
    counts[h] = count;
    sumsq[h] = sum;
}

// partials[blockIdx.x][PLANE_SUM_TERMS]: the workgroup's sums.  mask may be NULL.  A plane of four zeros has no inliers.
__global__ __launch_bounds__(PLANE_BLOCK) void plane_inliers_kernel(int n, const float* __restrict__ xyz, PlaneModel P,
                                                                    double threshold, uint8_t* __restrict__ mask,
                                                                    double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double wave_sums[PLANE_WAVES][PLANE_SUM_TERMS];
    const int64_t i = (int64_t)blockIdx.x * PLANE_BLOCK + threadIdx.x;
    double v[PLANE_SUM_TERMS];
#pragma unroll
    for (int k = 0; k < PLANE_SUM_TERMS; ++k) v[k] = 0.0;
    if (i < n) {
        const double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1], z = (double)xyz[3 * i + 2];
        const double dist = plane_distance(P.n[0], P.n[1], P.n[2], P.d, x, y, z);
        const bool zero = P.n[0] == 0.0 && P.n[1] == 0.0 && P.n[2] == 0.0 && P.d == 0.0;
        const bool in = !zero && dist < threshold;
        if (mask) mask[i] = in ? 1 : 0;
        if (in) {
            const double qx = x - P.pivot[0], qy = y - P.pivot[1], qz = z - P.pivot[2];
            v[0] = 1.0;
            v[1] = qx; v[2] = qy; v[3] = qz;
            v[4] = qx * qx; v[5] = qx * qy; v[6] = qx * qz; v[7] = qy * qy; v[8] = qy * qz; v[9] = qz * qz;
            v[10] = dist * dist;
        }
    }
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < PLANE_SUM_TERMS; ++k) {
        const double w = registration_wave_sum(v[k]);
        if (lane == 0) wave_sums[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < PLANE_SUM_TERMS) {
        double w = wave_sums[0][threadIdx.x];
#pragma unroll
        for (int g = 1; g < PLANE_WAVES; ++g) w += wave_sums[g][threadIdx.x];
        partials[(size_t)blockIdx.x * PLANE_SUM_TERMS + threadIdx.x] = w;
    }
}

// one workgroup: wave g adds partials [g * run, (g + 1) * run) in order, lane k term k; then a tree over the 16 waves
// (registration_sums_final_kernel for PLANE_SUM_TERMS terms)
__global__ __launch_bounds__(PLANE_FINAL_BLOCK) void plane_inliers_final_kernel(int blocks, const double* __restrict__ partials,
                                                                                double* __restrict__ sums) {
#pragma clang fp contract(off)
    constexpr int WAVES = PLANE_FINAL_BLOCK / WAVE;
    __shared__ double part[WAVES][WAVE];
    const int k = threadIdx.x & (WAVE - 1), g = threadIdx.x / WAVE;
    const int run = (blocks + WAVES - 1) / WAVES;
    double w = 0.0;
    if (k < PLANE_SUM_TERMS)
        for (int b = g * run; b < min((g + 1) * run, blocks); ++b) w += partials[(size_t)b * PLANE_SUM_TERMS + k];
    part[g][k] = w;
    __syncthreads();
#pragma unroll
    for (int d = WAVES / 2; d >= 1; d >>= 1) {
        if (g < d) part[g][k] += part[g + d][k];
        __syncthreads();
    }
    if (g == 0 && k < PLANE_SUM_TERMS) sums[k] = part[0][k];
}

}  // namespace pgr
