// poseerr.hip.h -- the BOP pose errors of (estimate, ground truth) pairs: MSSD, MSPD, ADD, proj, re, te (pgr_pose_errors) and
// ADI (pgr_pose_adi), the functions of the toolkit's bop_toolkit_lib/pose_error.py.
//
// pgr_pose_errors: the rules (tests/pose_error_reference.py restates them in NumPy, errors_f32)
//
//   Transforms. The estimate (R_est, t_est) is rounded to float32 once.  For symmetry s = (R_s, t_s) of the job the ground
//               truth is composed in float64, in this order, then rounded to float32 once:
//                   R_gs[i][j] = (R_gt[i][0] R_s[0][j] + R_gt[i][1] R_s[1][j]) + R_gt[i][2] R_s[2][j]
//                   t_gs[i]    = ((R_gt[i][0] t_s[0] + R_gt[i][1] t_s[1]) + R_gt[i][2] t_s[2]) + t_gt[i]
//               With the identity symmetry every product is the element itself or a zero: (R_gs, t_gs) is (R_gt, t_gt)
//               bit for bit, so est == gt gives 0 for mssd, mspd, add and proj exactly.
//   Vertex.     As the mesh rasterizer does, in float32 without contraction:
//                   X = ((R[0] p.x + R[1] p.y) + R[2] p.z) + t[0]         u = (fx X) / Z + cx      v = (fy Y) / Z + cy
//               (IEEE division, no special case for Z <= 0).  d3 = (dx dx + dy dy) + dz dz between the estimated and the
//               ground-truth point, d2 = du du + dv dv between their projections.
//   mssd, mspd. min over the symmetries of sqrt(max over the vertices of d3) (of d2): the square root is monotonic, so it is
//               taken once per (job, symmetry chunk).  fmaxf drops a NaN distance.  The minimum over chunks is an unsigned
//               atomic min on the float's bits (the values are >= 0, so the bits order like the floats); the init kernel of
//               the same call sets +inf.  No float atomics: the result does not depend on arrival order.
//   add, proj.  Mean of sqrt(d3) (sqrt(d2)) for symmetry index 0, which is the identity (misc.get_symmetry_transformations
//               lists it first).  Lane l of the workgroup sums its vertices l, l + 256, ... in float32 in that order; the 256
//               lane sums are added in float64: xor-butterfly over each wave (strides 1, 2, .. 32), then wave 0 + 1 + 2 + 3,
//               divided by the vertex count, rounded to float32.
//   re, te.     In float64 by one lane:  c = 0.5 (trace - 1) with trace = sum_i (R_est[i][0] R_gt[i][0] + R_est[i][1] R_gt[i][1])
//               + R_est[i][2] R_gt[i][2]  (the trace of R_est R_gt^T), re = acos(min(1, max(-1, c))) 180 / pi;
//               te = sqrt((dx dx + dy dy) + dz dz) of t_gt - t_est.
//
// Work.  One workgroup of 256 lanes per (job, chunk of PERR_SYM_CHUNK symmetries).  The chunk's composed transforms, the
// estimate and the intrinsics are wave-uniform and are pinned into SGPRs (readfirstlane): 12 x (PERR_SYM_CHUNK + 1) + 4 = 64
// values at PERR_SYM_CHUNK = 4 (the compiler reports 103 SGPRs in all, no spill); 8 would need 112 for the values alone,
// above the 102 a wave has.  Each lane loads a vertex once, computes the
// estimated point and projection once and PERR_SYM_CHUNK ground-truth ones.  A chunk's unused slots repeat its first
// transform, which leaves the minimum unchanged.  Jobs reach the device as a by-value table per launch, as PgrMeshJob does.
//
// pgr_pose_adi: the rules (adi_f32 restates them)
//
//   Query.      The nearest neighbour of R_gt p + t_gt among {R_est q + t_est} is the nearest neighbour of M p + c among
//               the model's own points:  M = R_est^T R_gt, c = R_est^T (t_gt - t_est), composed on the host in float64,
//                   M[i][j] = (R_est[0][i] R_gt[0][j] + R_est[1][i] R_gt[1][j]) + R_est[2][i] R_gt[2][j]
//                   c[i]    = (R_est[0][i] d[0] + R_est[1][i] d[1]) + R_est[2][i] d[2],     d = t_gt - t_est
//               and rounded to float32 once.  R_est == R_gt element for element makes M the identity exactly (R^T R of a
//               rotation is the identity; its float64 product only approximates it), so est == gt gives the query p itself
//               and ADI 0 exactly.  The query point is  ((M[0] p.x + M[1] p.y) + M[2] p.z) + c[0]  etc. in float32.
//   Search.     Exact brute force: one query per lane, the model's vertices streamed through LDS in tiles of 256, a running
//               fminf of d = (dx dx + dy dy) + dz dz per lane, the square root at the end.
//   Mean.       Per workgroup the 256 distances (0 for lanes without a query) are added in float64, butterfly then waves in
//               order, into one partial; a second kernel adds a job's partials in order, divides by the vertex count and
//               rounds to float32.
#pragma once
#include "job_table.hip.h"       // pose_job_of_block
#include "pgr_common.h"
#include "wave_ops.hip.h"        // wave_max_f

namespace pgr {

constexpr int PERR_THREADS = 256;
constexpr int PERR_WAVES = PERR_THREADS / WAVE;
constexpr int PERR_SYM_CHUNK = PGR_POSE_SYM_CHUNK;
constexpr int PERR_JOBS_PER_LAUNCH = 16;             // 232 B each: the table stays under the 4 KiB of kernel arguments
constexpr int ADI_JOBS_PER_LAUNCH = 48;              // 64 B each
constexpr int ADI_TILE = 256;

struct PoseErrJobDev {
    int32_t v0, nv, s0, ns;
    double Re[9], te[3], Rg[9], tg[3];
    float fx, fy, cx, cy;
    uint32_t block0;                                 // first workgroup of the job in the launch
    uint32_t pad;
};

struct PoseErrJobTable {
    int32_t count, first;
    int32_t pad[2];
    PoseErrJobDev job[PERR_JOBS_PER_LAUNCH];
};
static_assert(sizeof(PoseErrJobTable) <= 3840, "PoseErrJobTable must fit the kernel argument segment");

struct AdiJobDev {
    int32_t v0, nv;
    float M[9], c[3];
    uint32_t block0;                                 // first workgroup of the job in the launch
    uint32_t part0;                                  // first partial sum of the job in the workspace
};

struct AdiJobTable {
    int32_t count, first;
    AdiJobDev job[ADI_JOBS_PER_LAUNCH];
};
static_assert(sizeof(AdiJobTable) <= 3840, "AdiJobTable must fit the kernel argument segment");

__device__ __forceinline__ float pose_uniform(float v) {         // a wave-uniform value, kept in an SGPR
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// sum over the wave in float64, xor butterfly: every lane ends with the same bits
__device__ __forceinline__ double pose_wave_sum(double v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

// errors [n_jobs,6]: mssd and mspd start at +inf, the rest at 0
__global__ __launch_bounds__(256) void pose_init_kernel(float* __restrict__ errors, int n_jobs) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_jobs * PGR_POSE_ERRORS) return;
    errors[e] = (e % PGR_POSE_ERRORS) < 2 ? INFINITY : 0.f;
}

__global__ __launch_bounds__(PERR_THREADS) void pose_errors_kernel(const PoseErrJobTable T, const float* __restrict__ vertices,
                                                                  const double* __restrict__ syms, float* __restrict__ errors,
                                                                  double* __restrict__ re_te) {
    __shared__ float s_xf[PERR_SYM_CHUNK][12];
    __shared__ float s_max[PERR_WAVES][2 * PERR_SYM_CHUNK];
    __shared__ double s_sum[PERR_WAVES][2];
    const int k = pose_job_of_block(T, blockIdx.x);
    const PoseErrJobDev& J = T.job[k];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int chunk = (int)(blockIdx.x - J.block0);
    const int s_begin = chunk * PERR_SYM_CHUNK;
    const int ns = min(PERR_SYM_CHUNK, J.ns - s_begin);           // >= 1 by the host's block count
    if (tid < PERR_SYM_CHUNK) {
        const int s = tid < ns ? tid : 0;                         // unused slots repeat the chunk's first symmetry
        const double* S = syms + 12 * ((size_t)J.s0 + (size_t)(s_begin + s));
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                s_xf[tid][3 * i + j] = (float)((J.Rg[3 * i] * S[j] + J.Rg[3 * i + 1] * S[3 + j]) + J.Rg[3 * i + 2] * S[6 + j]);
            s_xf[tid][9 + i] = (float)(((J.Rg[3 * i] * S[9] + J.Rg[3 * i + 1] * S[10]) + J.Rg[3 * i + 2] * S[11]) + J.tg[i]);
        }
    }
    __syncthreads();
    float G[PERR_SYM_CHUNK][12], E[12];
#pragma unroll
    for (int s = 0; s < PERR_SYM_CHUNK; ++s)
#pragma unroll
        for (int e = 0; e < 12; ++e) G[s][e] = pose_uniform(s_xf[s][e]);
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = pose_uniform((float)J.Re[e]);
#pragma unroll
    for (int e = 0; e < 3; ++e) E[9 + e] = pose_uniform((float)J.te[e]);
    const float fx = pose_uniform(J.fx), fy = pose_uniform(J.fy), cx = pose_uniform(J.cx), cy = pose_uniform(J.cy);

    float max3[PERR_SYM_CHUNK], max2[PERR_SYM_CHUNK];
#pragma unroll
    for (int s = 0; s < PERR_SYM_CHUNK; ++s) max3[s] = max2[s] = 0.f;
    float sum3 = 0.f, sum2 = 0.f;
    const float* base = vertices + 3 * (size_t)J.v0;
    for (int i = tid; i < J.nv; i += PERR_THREADS) {
        const float px = gload(base + 3 * (size_t)i), py = gload(base + 3 * (size_t)i + 1), pz = gload(base + 3 * (size_t)i + 2);
        const float Xe = ((E[0] * px + E[1] * py) + E[2] * pz) + E[9];
        const float Ye = ((E[3] * px + E[4] * py) + E[5] * pz) + E[10];
        const float Ze = ((E[6] * px + E[7] * py) + E[8] * pz) + E[11];
        const float ue = (fx * Xe) / Ze + cx, ve = (fy * Ye) / Ze + cy;
#pragma unroll
        for (int s = 0; s < PERR_SYM_CHUNK; ++s) {
            const float X = ((G[s][0] * px + G[s][1] * py) + G[s][2] * pz) + G[s][9];
            const float Y = ((G[s][3] * px + G[s][4] * py) + G[s][5] * pz) + G[s][10];
            const float Z = ((G[s][6] * px + G[s][7] * py) + G[s][8] * pz) + G[s][11];
            const float dx = Xe - X, dy = Ye - Y, dz = Ze - Z;
            const float d3 = (dx * dx + dy * dy) + dz * dz;
            const float du = ue - ((fx * X) / Z + cx), dv = ve - ((fy * Y) / Z + cy);
            const float d2 = du * du + dv * dv;
            max3[s] = fmaxf(max3[s], d3);
            max2[s] = fmaxf(max2[s], d2);
            if (s == 0 && chunk == 0) {                           // symmetry index 0 of the job: ADD and proj
                sum3 += sqrtf(d3);
                sum2 += sqrtf(d2);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < PERR_SYM_CHUNK; ++s) {
        const float m3 = wave_max_f(max3[s]), m2 = wave_max_f(max2[s]);      // in lane 63
        if (lane == WAVE - 1) { s_max[wave][2 * s] = m3; s_max[wave][2 * s + 1] = m2; }
    }
    if (chunk == 0) {
        const double a = pose_wave_sum((double)sum3), b = pose_wave_sum((double)sum2);
        if (lane == 0) { s_sum[wave][0] = a; s_sum[wave][1] = b; }
    }
    __syncthreads();
    if (tid != 0) return;
    float* out = errors + (size_t)PGR_POSE_ERRORS * ((size_t)T.first + (size_t)k);
    float best3 = INFINITY, best2 = INFINITY;
#pragma unroll
    for (int s = 0; s < PERR_SYM_CHUNK; ++s) {
        float m3 = s_max[0][2 * s], m2 = s_max[0][2 * s + 1];
#pragma unroll
        for (int w = 1; w < PERR_WAVES; ++w) { m3 = fmaxf(m3, s_max[w][2 * s]); m2 = fmaxf(m2, s_max[w][2 * s + 1]); }
        best3 = fminf(best3, m3);
        best2 = fminf(best2, m2);
    }
    __hip_atomic_fetch_min((PGR_GLOBAL uint32_t*)(out + 0), __float_as_uint(sqrtf(best3)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min((PGR_GLOBAL uint32_t*)(out + 1), __float_as_uint(sqrtf(best2)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (chunk != 0) return;
    const double n = (double)J.nv;
    gstore(out + 2, (float)((((s_sum[0][0] + s_sum[1][0]) + s_sum[2][0]) + s_sum[3][0]) / n));
    gstore(out + 3, (float)((((s_sum[0][1] + s_sum[1][1]) + s_sum[2][1]) + s_sum[3][1]) / n));
    double trace = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        trace += (J.Re[3 * i] * J.Rg[3 * i] + J.Re[3 * i + 1] * J.Rg[3 * i + 1]) + J.Re[3 * i + 2] * J.Rg[3 * i + 2];
    const double c = fmin(1.0, fmax(-1.0, 0.5 * (trace - 1.0)));
    const double re = 180.0 * acos(c) / 3.14159265358979323846;
    const double dx = J.tg[0] - J.te[0], dy = J.tg[1] - J.te[1], dz = J.tg[2] - J.te[2];
    const double te = sqrt((dx * dx + dy * dy) + dz * dz);
    gstore(out + 4, (float)re);
    gstore(out + 5, (float)te);
    if (re_te) {
        double* o = re_te + 2 * ((size_t)T.first + (size_t)k);
        o[0] = re;
        o[1] = te;
    }
}

__global__ __launch_bounds__(ADI_TILE) void pose_adi_kernel(const AdiJobTable T, const float* __restrict__ vertices,
                                                           double* __restrict__ partials) {
    __shared__ float4 s_tile[ADI_TILE];
    __shared__ double s_sum[ADI_TILE / WAVE];
    const int k = pose_job_of_block(T, blockIdx.x);
    const AdiJobDev& J = T.job[k];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const uint32_t group = blockIdx.x - J.block0;
    const float* base = vertices + 3 * (size_t)J.v0;
    const long long qi = (long long)group * ADI_TILE + tid;
    const bool has_query = qi < J.nv;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (has_query) {
        const float px = gload(base + 3 * (size_t)qi), py = gload(base + 3 * (size_t)qi + 1), pz = gload(base + 3 * (size_t)qi + 2);
        qx = ((J.M[0] * px + J.M[1] * py) + J.M[2] * pz) + J.c[0];
        qy = ((J.M[3] * px + J.M[4] * py) + J.M[5] * pz) + J.c[1];
        qz = ((J.M[6] * px + J.M[7] * py) + J.M[8] * pz) + J.c[2];
    }
    float best = INFINITY;
    for (int t0 = 0; t0 < J.nv; t0 += ADI_TILE) {
        const int n = min(ADI_TILE, J.nv - t0);                   // points of this tile: nothing past the job's range is read
        if (tid < n) {
            const float* p = base + 3 * ((size_t)t0 + (size_t)tid);
            s_tile[tid] = make_float4(gload(p), gload(p + 1), gload(p + 2), 0.f);
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float4 m = s_tile[j];
            const float dx = qx - m.x, dy = qy - m.y, dz = qz - m.z;
            best = fminf(best, (dx * dx + dy * dy) + dz * dz);
        }
        __syncthreads();
    }
    const double sum = pose_wave_sum(has_query ? (double)sqrtf(best) : 0.0);
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (tid == 0) partials[(size_t)J.part0 + group] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
}

__global__ __launch_bounds__(64) void pose_adi_mean_kernel(const AdiJobTable T, const double* __restrict__ partials,
                                                          float* __restrict__ adi) {
    const int k = threadIdx.x;
    if (k >= T.count) return;
    const AdiJobDev& J = T.job[k];
    const int groups = (J.nv + ADI_TILE - 1) / ADI_TILE;
    double sum = 0.0;
    for (int g = 0; g < groups; ++g) sum += partials[(size_t)J.part0 + g];
    adi[(size_t)T.first + k] = (float)(sum / (double)J.nv);
}

}  // namespace pgr
