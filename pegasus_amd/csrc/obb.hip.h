// obb.hip.h -- minimal oriented bounding boxes by open3d's rule (one candidate box per triangle, pgr_obb_candidates) and the
// largest point-to-point distance (pgr_point_diameter, the toolkit's misc.calc_pts_diameter).  DESIGN.md section 16.
//
// pgr_obb_candidates: the rules (tests/obb_reference.py restates them in NumPy)
//
//   Frame.      Triangle (i0, i1, i2) of a job, float32 points widened to float64, every operation float64:
//                   a = p[i0], u = p[i1] - a, v = p[i2] - a, w = u x v, v = w x u, each of u, v, w divided by its norm
//               (cross product c.x = a.y b.z - a.z b.y, each product and the difference rounded; norm = sqrt((x x + y y) + z z)).
//   Projection. q = ((p - a) . u, (p - a) . v, (p - a) . w) with d . e = fma(d.z, e.z, fma(d.y, e.y, d.x e.x)).
//   Candidate.  lo, hi = per-axis min, max of q over the job's points; extent = hi - lo; volume = (extent.x extent.y) extent.z.
//               A zero of either sign in lo or hi is written as +0, so no result depends on the order of the min and max.
//   Not finite. A degenerate triangle has NaN axes: fmin and fmax drop every NaN q, lo stays +inf and hi -inf, the volume is
//               -inf.  A point that is Inf or NaN makes every candidate of its job lo = -inf, hi = +inf, volume +inf (the staging
//               lanes see it; fmin alone would drop a NaN).  Neither is ever chosen.
//   Choice.     The finite volume that is smallest, the lowest triangle index among equal ones; -1 if none is finite.
//
// Work.  A lane owns one triangle and keeps its frame (12 values) and six running extremes in registers.  A workgroup of
// OBB_TF lanes stages OBB_TP points at a time in LDS as float64; every lane reads the same address (a broadcast, no bank
// conflict).  A job's points are cut into `splits` chunks of whole tiles, so that a job of few triangles and many points still
// fills the chip: workgroup (triangle block, chunk) writes partial extremes [chunk][6][triangle] to the workspace, a second
// launch merges a triangle's chunks in order (min and max: any order gives the same bytes) and writes the volume, a third
// reduces (volume, index) per job and writes the chosen candidate's lo and hi.  No float atomics.  Triangle indices are NOT
// clamped: the entry checks them against the job's point_count on the host when it is given a host copy of the triangles.
//
// pgr_point_diameter: the rules
//
//   d2(i, j) = fma(dz, dz, fma(dy, dy, dx dx)),  d = p[j] - p[i] in float64, for i < j.  The pair of largest d2, the
//   lexicographically lowest pair among equal ones.  A NaN d2 is never chosen.  One point: pair (0, 0), d2 0.  None: (-1, -1), 0.
//
// Work.  Lane i of a workgroup owns point i of a block of DIAM_TILE, and walks the staged points j > i of its chunk of
// [block start, P): strict > in ascending j keeps the lowest j per lane.  Workgroup (block, chunk) writes one partial
// (d2, i, j); a second launch reduces a job's partials.  The order (larger d2, then lower i, then lower j) is total, so the
// result does not depend on how the work was cut.
#pragma once
#include "pgr_common.h"

namespace pgr {

constexpr int OBB_TF = PGR_OBB_TRI_TILE;             // triangles per workgroup, one per lane
constexpr int OBB_TP = PGR_OBB_POINT_TILE;           // points staged per tile: 12 KiB of LDS as float64
constexpr int OBB_JOBS_PER_LAUNCH = 64;              // 40 B each
constexpr int OBB_TARGET_BLOCKS = 2048;              // what the host aims a job's launch at: 8 workgroups per CU
constexpr int DIAM_TILE = PGR_DIAMETER_TILE;
static_assert(OBB_TP % OBB_TF == 0, "every lane stages the same number of points");

struct ObbJobDev {
    int32_t p0, np, t0, nt;
    uint32_t block0;                                 // first workgroup of the job in the partial launch
    uint32_t mblock0;                                // first workgroup of the job in the merge launch
    uint32_t splits;                                 // chunks the job's points are cut into (>= 1)
    uint32_t chunk;                                  // points per chunk, a multiple of the tile
    uint64_t part0;                                  // first partial of the job in the workspace, in doubles (obb) or records
};

struct ObbJobTable {
    int32_t count, first;
    int32_t pad[2];
    ObbJobDev job[OBB_JOBS_PER_LAUNCH];
};
static_assert(sizeof(ObbJobTable) <= 3840, "ObbJobTable must fit the kernel argument segment");

struct DiamPartial { double d2; int32_t i, j; };
static_assert(sizeof(DiamPartial) == 16, "DiamPartial is 16 B");

__device__ __forceinline__ int obb_job_of_block(const ObbJobTable& T, uint32_t block, bool merge) {
    int k = 0;
    for (int q = 1; q < T.count; ++q)
        if (block >= (merge ? T.job[q].mblock0 : T.job[q].block0) && T.job[q].nt > 0) k = q;
    return k;
}

__device__ __forceinline__ double obb_dot(double dx, double dy, double dz, double ex, double ey, double ez) {
    return fma(dz, ez, fma(dy, ey, dx * ex));
}

__device__ __forceinline__ bool obb_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }    // false for NaN

__global__ __launch_bounds__(OBB_TF) void obb_partial_kernel(const ObbJobTable T, const float* __restrict__ points,
                                                             const int32_t* __restrict__ tris, double* __restrict__ partials) {
    __shared__ double s_pt[OBB_TP][3];
    __shared__ int s_bad;
    const int k = obb_job_of_block(T, blockIdx.x, false);
    const ObbJobDev& J = T.job[k];
    const int tid = threadIdx.x;
    const uint32_t rel = blockIdx.x - J.block0;
    const uint32_t tri_block = rel / J.splits, split = rel % J.splits;
    const int64_t t = (int64_t)tri_block * OBB_TF + tid;
    const bool has = t < J.nt;
    const float* base = points + 3 * (size_t)J.p0;
    if (tid == 0) s_bad = 0;

    int32_t i0 = 0, i1 = 0, i2 = 0;                               // lanes past the job's triangles walk along with point 0
    if (has) {
        const int32_t* f = tris + 3 * ((size_t)J.t0 + (size_t)t);
        i0 = gload(f); i1 = gload(f + 1); i2 = gload(f + 2);
    }
    const double ax = (double)gload(base + 3 * (size_t)i0), ay = (double)gload(base + 3 * (size_t)i0 + 1),
                 az = (double)gload(base + 3 * (size_t)i0 + 2);
    double ux = (double)gload(base + 3 * (size_t)i1) - ax, uy = (double)gload(base + 3 * (size_t)i1 + 1) - ay,
           uz = (double)gload(base + 3 * (size_t)i1 + 2) - az;
    double vx = (double)gload(base + 3 * (size_t)i2) - ax, vy = (double)gload(base + 3 * (size_t)i2 + 1) - ay,
           vz = (double)gload(base + 3 * (size_t)i2 + 2) - az;
    double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    vx = wy * uz - wz * uy; vy = wz * ux - wx * uz; vz = wx * uy - wy * ux;
    const double nu = sqrt((ux * ux + uy * uy) + uz * uz), nv = sqrt((vx * vx + vy * vy) + vz * vz),
                 nw = sqrt((wx * wx + wy * wy) + wz * wz);
    ux /= nu; uy /= nu; uz /= nu;
    vx /= nv; vy /= nv; vz /= nv;
    wx /= nw; wy /= nw; wz /= nw;

    double lo0 = INFINITY, lo1 = INFINITY, lo2 = INFINITY, hi0 = -INFINITY, hi1 = -INFINITY, hi2 = -INFINITY;
    const int c0 = (int)((int64_t)split * J.chunk);               // < np by the host's count of chunks
    const int c1 = (int)min((int64_t)J.np, (int64_t)c0 + J.chunk);
    for (int p0 = c0; p0 < c1; p0 += OBB_TP) {
        const int n = min(OBB_TP, c1 - p0);                       // nothing past the job's range is read
        __syncthreads();                                          // the previous tile is read, s_bad is cleared
#pragma unroll
        for (int r = 0; r < OBB_TP / OBB_TF; ++r) {
            const int j = tid + r * OBB_TF;
            if (j < n) {
                const float* p = base + 3 * ((size_t)p0 + (size_t)j);
                const float x = gload(p), y = gload(p + 1), z = gload(p + 2);
                s_pt[j][0] = (double)x; s_pt[j][1] = (double)y; s_pt[j][2] = (double)z;
                if (!(obb_finite(x) && obb_finite(y) && obb_finite(z))) s_bad = 1;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const double dx = s_pt[j][0] - ax, dy = s_pt[j][1] - ay, dz = s_pt[j][2] - az;
            const double q0 = obb_dot(dx, dy, dz, ux, uy, uz), q1 = obb_dot(dx, dy, dz, vx, vy, vz),
                         q2 = obb_dot(dx, dy, dz, wx, wy, wz);
            lo0 = fmin(lo0, q0); hi0 = fmax(hi0, q0);
            lo1 = fmin(lo1, q1); hi1 = fmax(hi1, q1);
            lo2 = fmin(lo2, q2); hi2 = fmax(hi2, q2);
        }
    }
    __syncthreads();
    if (s_bad) { lo0 = lo1 = lo2 = -INFINITY; hi0 = hi1 = hi2 = INFINITY; }
    if (!has) return;
    double* out = partials + J.part0 + (size_t)split * 6 * (size_t)J.nt + (size_t)t;
    const size_t s = (size_t)J.nt;
    out[0] = lo0; out[s] = lo1; out[2 * s] = lo2; out[3 * s] = hi0; out[4 * s] = hi1; out[5 * s] = hi2;
}

// component c (0..2 lo, 3..5 hi) of triangle t of the job over its chunks, zeros written as +0
__device__ __forceinline__ double obb_merged(const ObbJobDev& J, const double* __restrict__ partials, int64_t t, int c) {
    const double* in = partials + J.part0 + (size_t)c * (size_t)J.nt + (size_t)t;
    double m = in[0];
    for (uint32_t s = 1; s < J.splits; ++s) {
        const double x = in[(size_t)s * 6 * (size_t)J.nt];
        m = c < 3 ? fmin(m, x) : fmax(m, x);
    }
    return m + 0.0;                                               // -0 + 0 = +0
}

__global__ __launch_bounds__(OBB_TF) void obb_merge_kernel(const ObbJobTable T, const double* __restrict__ partials,
                                                           double* __restrict__ volumes) {
    const int k = obb_job_of_block(T, blockIdx.x, true);
    const ObbJobDev& J = T.job[k];
    const int64_t t = (int64_t)(blockIdx.x - J.mblock0) * OBB_TF + threadIdx.x;
    if (t >= J.nt) return;
    const double e0 = obb_merged(J, partials, t, 3) - obb_merged(J, partials, t, 0);
    const double e1 = obb_merged(J, partials, t, 4) - obb_merged(J, partials, t, 1);
    const double e2 = obb_merged(J, partials, t, 5) - obb_merged(J, partials, t, 2);
    volumes[(size_t)J.t0 + (size_t)t] = (e0 * e1) * e2;
}

__device__ __forceinline__ bool obb_f64_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// one workgroup per job: the finite volume that is smallest, the lowest index among equal ones
__global__ __launch_bounds__(256) void obb_argmin_kernel(const ObbJobTable T, const double* __restrict__ partials,
                                                         const double* __restrict__ volumes, int32_t* __restrict__ best,
                                                         double* __restrict__ lohi) {
    __shared__ double s_v[256];
    __shared__ int32_t s_i[256];
    const ObbJobDev& J = T.job[blockIdx.x];
    const int tid = threadIdx.x;
    double bv = INFINITY;
    int32_t bi = -1;
    for (int32_t t = tid; t < J.nt; t += 256) {                   // ascending t: strict < keeps the lane's lowest index
        const double v = volumes[(size_t)J.t0 + (size_t)t];
        if (obb_f64_finite(v) && (bi < 0 || v < bv)) { bv = v; bi = t; }
    }
    s_v[tid] = bv; s_i[tid] = bi;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) {
            const double ov = s_v[tid + d];
            const int32_t oi = s_i[tid + d];
            const int32_t mi = s_i[tid];
            if (oi >= 0 && (mi < 0 || ov < s_v[tid] || (ov == s_v[tid] && oi < mi))) { s_v[tid] = ov; s_i[tid] = oi; }
        }
        __syncthreads();
    }
    const int32_t b = s_i[0];
    const size_t job = (size_t)T.first + blockIdx.x;
    if (tid == 0) best[job] = b;
    if (tid < 6) lohi[6 * job + tid] = b < 0 ? (double)NAN : obb_merged(J, partials, b, tid);
}

// ---- diameter
__device__ __forceinline__ bool diam_better(double d2, int32_t i, int32_t j, double e2, int32_t ei, int32_t ej) {
    if (ei < 0) return i >= 0;
    if (i < 0) return false;
    return d2 > e2 || (d2 == e2 && (i < ei || (i == ei && j < ej)));
}

__global__ __launch_bounds__(DIAM_TILE) void diameter_partial_kernel(const ObbJobTable T, const float* __restrict__ points,
                                                                     DiamPartial* __restrict__ partials) {
    __shared__ double s_pt[DIAM_TILE][3];
    __shared__ double s_d[DIAM_TILE];
    __shared__ int32_t s_i[DIAM_TILE], s_j[DIAM_TILE];
    int k = 0;
    for (int q = 1; q < T.count; ++q)
        if (blockIdx.x >= T.job[q].block0 && T.job[q].np > 0) k = q;
    const ObbJobDev& J = T.job[k];
    const int tid = threadIdx.x;
    const uint32_t rel = blockIdx.x - J.block0;
    const uint32_t ib = rel / J.splits, split = rel % J.splits;
    const float* base = points + 3 * (size_t)J.p0;
    const int i_first = (int)ib * DIAM_TILE;                      // < np by the host's count of blocks
    const int i = i_first + tid;
    const bool has = i < J.np;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (has) {
        px = (double)gload(base + 3 * (size_t)i); py = (double)gload(base + 3 * (size_t)i + 1);
        pz = (double)gload(base + 3 * (size_t)i + 2);
    }
    // the block's points j lie in [i_first, np): `splits` chunks of whole tiles
    const int len = J.np - i_first;
    const int tiles = (len + DIAM_TILE - 1) / DIAM_TILE;
    const int chunk = (int)((tiles + J.splits - 1) / J.splits) * DIAM_TILE;
    const int64_t c0 = (int64_t)i_first + (int64_t)split * chunk;
    const int c1 = (int)min((int64_t)J.np, c0 + chunk);
    double bd = -1.0;
    int32_t bj = -1;
    for (int64_t j0 = c0; j0 < c1; j0 += DIAM_TILE) {             // an empty chunk (c0 >= c1) walks nothing
        const int n = min(DIAM_TILE, c1 - (int)j0);
        __syncthreads();
        if (tid < n) {
            const float* p = base + 3 * ((size_t)j0 + (size_t)tid);
            s_pt[tid][0] = (double)gload(p); s_pt[tid][1] = (double)gload(p + 1); s_pt[tid][2] = (double)gload(p + 2);
        }
        __syncthreads();
        const int first = max(0, i + 1 - (int)j0);                // only j > i
#pragma unroll 4
        for (int jj = first; jj < n; ++jj) {
            const double dx = s_pt[jj][0] - px, dy = s_pt[jj][1] - py, dz = s_pt[jj][2] - pz;
            const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
            if (d2 > bd) { bd = d2; bj = (int32_t)j0 + jj; }
        }
    }
    s_d[tid] = bd; s_i[tid] = has && bj >= 0 ? i : -1; s_j[tid] = bj;
    __syncthreads();
    for (int d = DIAM_TILE / 2; d > 0; d >>= 1) {
        if (tid < d && diam_better(s_d[tid + d], s_i[tid + d], s_j[tid + d], s_d[tid], s_i[tid], s_j[tid])) {
            s_d[tid] = s_d[tid + d]; s_i[tid] = s_i[tid + d]; s_j[tid] = s_j[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) partials[J.part0 + rel] = DiamPartial{s_d[0], s_i[0], s_j[0]};
}

// one workgroup per job over its partials
__global__ __launch_bounds__(256) void diameter_reduce_kernel(const ObbJobTable T, const DiamPartial* __restrict__ partials,
                                                              int32_t* __restrict__ pair, double* __restrict__ d2) {
    __shared__ double s_d[256];
    __shared__ int32_t s_i[256], s_j[256];
    const ObbJobDev& J = T.job[blockIdx.x];
    const int tid = threadIdx.x;
    const uint64_t n_part = J.np > 0 ? (uint64_t)((J.np + DIAM_TILE - 1) / DIAM_TILE) * J.splits : 0;
    double bd = -1.0;
    int32_t bi = -1, bj = -1;
    for (uint64_t q = tid; q < n_part; q += 256) {
        const DiamPartial P = partials[J.part0 + q];
        if (diam_better(P.d2, P.i, P.j, bd, bi, bj)) { bd = P.d2; bi = P.i; bj = P.j; }
    }
    s_d[tid] = bd; s_i[tid] = bi; s_j[tid] = bj;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d && diam_better(s_d[tid + d], s_i[tid + d], s_j[tid + d], s_d[tid], s_i[tid], s_j[tid])) {
            s_d[tid] = s_d[tid + d]; s_i[tid] = s_i[tid + d]; s_j[tid] = s_j[tid + d];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const size_t job = (size_t)T.first + blockIdx.x;
    const bool one = J.np == 1;                                   // one point: the pair (0, 0) at distance 0
    pair[2 * job] = s_i[0] >= 0 ? s_i[0] : (one ? 0 : -1);
    pair[2 * job + 1] = s_i[0] >= 0 ? s_j[0] : (one ? 0 : -1);
    d2[job] = s_i[0] >= 0 ? s_d[0] : 0.0;
}

}  // namespace pgr
