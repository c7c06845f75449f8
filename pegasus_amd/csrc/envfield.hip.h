// envfield.hip.h -- the environment as a distance field: pgr_sdf_from_tsdf turns a carved, truncated volume (pgr_tsdf_integrate)
// into a signed distance field over the whole grid, which pgr_sdf_sample, pgr_sdf_sweep and the rigid-body kernels can take as
// the ground.  pegasus_amd/environment.py is the caller; tests/environment_reference.py restates every rule in float64 and in
// float32 operation by operation; DESIGN.md section 25 holds the derivations.  All arithmetic is float32 without contraction,
// every operation rounded on its own; the distances are integers.
//
// pgr_sdf_from_tsdf: the rules
//
//   Sign.      inside(p) <=> tsdf(p) < 0 (marching's convention: a NaN is outside).  s = -1 inside, +1 outside.
//   Distance.  D2(p) = min |p - q|^2 over the grid points q with inside(q) != inside(p), in integer voxel units: exact.  Without
//              such a q it is NONE, written as -1 to dist2.
//   Band.      p is a band point if one of its in-grid 6-neighbours n has the other sign; the neighbours are taken in the order
//              -x, +x, -y, +y, -z, +z.  beta(p) = min_n a / (a + b), a = |tsdf(p)|, b = |tsdf(n)|, the minimum by fminf in that
//              order: where pgr_march_emit puts its vertex on that edge (t = fa / (fa - fb)).  A value that is not finite counts
//              as 1 for a and b.  (a + b > 0: one of the two is < 0.)
//   Value.     band point:            phi = s (voxel beta)
//              other points with D2:  phi = s (voxel (sqrtf((float)D2) - 0.5f))
//              NONE:                  phi = s (voxel (float)(nx + ny + nz))
//   Limits.    Every axis holds 2 .. 1024 points, so D2 <= 3 * 1023^2 < 2^22.
//
// Work.  The squared distance transform is separable: after the pass along an axis every point holds the squared distance to the
//   nearest point of a class (inside, outside) within the lines done so far, and the next axis takes min_k g(k) + (i - k)^2 along
//   its line.  Two uint32 arrays, "nearest inside" and "nearest outside", go through the three passes in the workspace; a point
//   without one holds ENV_FAR = 2^30 or more (2^30 + 3 * 2^20 does not wrap).  Every minimum is the plain one: each lane
//   takes the integer minimum over the whole line from LDS, O(n^2) per line, branch-free and independent of order.
//   env_x_kernel: 256 lanes take max(1, 256 / nx) consecutive x lines (consecutive addresses) and read the class flags of their
//   line from LDS (lanes of one line read the same byte: a broadcast).  env_line_kernel (y, then z): the lanes lie along x, `tx`
//   (64, 32, 16 by line length, so that line x tx x 4 B <= 64 KiB) columns per workgroup and 256 / tx rows of lanes; column c of
//   the line lives in LDS as [k][c], so a wave reads consecutive words; blockIdx.z names the array.  It works in place: a
//   workgroup owns its lines and reads them all before it writes.  env_value_kernel: one lane per point picks the array of the
//   other class, takes the band from the six neighbours and writes phi and dist2.  No atomic anywhere: two runs give equal bytes.
#pragma once
#include "mesh.hip.h"
#include "pgr_common.h"

namespace pgr {

constexpr int ENV_THREADS = 256;
constexpr uint32_t ENV_FAR = 1u << 30;
constexpr int ENV_MAX_AXIS = 1024;
constexpr int ENV_LINE_WORDS = 16384;                // LDS words of env_line_kernel: 64 KiB

__device__ __forceinline__ bool env_inside(float t) { return t < 0.f; }

__global__ __launch_bounds__(ENV_THREADS) void env_x_kernel(int32_t nx, long long n_points, int32_t lines_per_block,
                                                           const float* __restrict__ tsdf, uint32_t* __restrict__ near_in,
                                                           uint32_t* __restrict__ near_out) {
    __shared__ uint8_t s_in[ENV_MAX_AXIS];
    const int items = lines_per_block * nx;          // <= max(256, nx) <= 1024
    const long long base = (long long)blockIdx.x * items;
    for (int e = threadIdx.x; e < items; e += ENV_THREADS)
        s_in[e] = (base + e < n_points && env_inside(gload(tsdf + base + e))) ? 1 : 0;
    __syncthreads();
    for (int e = threadIdx.x; e < items; e += ENV_THREADS) {
        if (base + e >= n_points) break;
        const int line = e / nx, i = e - line * nx;
        const uint8_t* f = s_in + line * nx;
        uint32_t best_in = ENV_FAR, best_out = ENV_FAR;
        for (int k = 0; k < nx; ++k) {
            const int d = i - k;
            const uint32_t d2 = (uint32_t)(d * d);
            const bool in = f[k] != 0;
            best_in = min(best_in, in ? d2 : ENV_FAR);
            best_out = min(best_out, in ? ENV_FAR : d2);
        }
        gstore(near_in + base + e, best_in);
        gstore(near_out + base + e, best_out);
    }
}

// lines of n points `line_stride` apart; column x and outer index blockIdx.y (`outer_stride` apart) name a line
__global__ __launch_bounds__(ENV_THREADS) void env_line_kernel(int32_t nx, int32_t n, long long line_stride,
                                                              long long outer_stride, int32_t tx, uint32_t* __restrict__ near_in,
                                                              uint32_t* __restrict__ near_out) {
    extern __shared__ uint32_t s_g[];                // [k][c], n * tx words
    uint32_t* g = (blockIdx.z == 0 ? near_in : near_out) + (long long)blockIdx.y * outer_stride;
    const int c = threadIdx.x % tx, r = threadIdx.x / tx, rows = ENV_THREADS / tx;
    const int x = blockIdx.x * tx + c;
    const bool has = x < nx;
    for (int k = r; k < n; k += rows) s_g[k * tx + c] = has ? gload(g + (long long)k * line_stride + x) : ENV_FAR;
    __syncthreads();
    if (!has) return;
    for (int i = r; i < n; i += rows) {
        uint32_t best = 0xFFFFFFFFu;
        for (int k = 0; k < n; ++k) {
            const int d = i - k;
            best = min(best, s_g[k * tx + c] + (uint32_t)(d * d));
        }
        gstore(g + (long long)i * line_stride + x, best);
    }
}

__device__ __forceinline__ float env_abs(float t) { return isfinite(t) ? fabsf(t) : 1.f; }

__global__ __launch_bounds__(ENV_THREADS) void env_value_kernel(const MeshGrid g, const float* __restrict__ tsdf,
                                                               const uint32_t* __restrict__ near_in,
                                                               const uint32_t* __restrict__ near_out, float* __restrict__ sdf,
                                                               int32_t* __restrict__ dist2) {
    const long long n_points = (long long)g.nx * g.ny * g.nz;
    const long long idx = (long long)blockIdx.x * ENV_THREADS + threadIdx.x;
    if (idx >= n_points) return;
    const int i = (int)(idx % g.nx), j = (int)((idx / g.nx) % g.ny), k = (int)(idx / ((long long)g.nx * g.ny));
    const long long sy = g.nx, sz = (long long)g.nx * g.ny;
    const float t = gload(tsdf + idx);
    const bool in = env_inside(t);
    const float a = env_abs(t);
    bool band = false;
    float beta = INFINITY;
    auto neighbour = [&](bool exists, long long at) {
        if (!exists) return;
        const float tn = gload(tsdf + at);
        if (env_inside(tn) == in) return;
        band = true;
        beta = fminf(beta, a / (a + env_abs(tn)));
    };
    neighbour(i > 0, idx - 1);
    neighbour(i < g.nx - 1, idx + 1);
    neighbour(j > 0, idx - sy);
    neighbour(j < g.ny - 1, idx + sy);
    neighbour(k > 0, idx - sz);
    neighbour(k < g.nz - 1, idx + sz);
    const uint32_t d2 = gload((in ? near_out : near_in) + idx);
    const bool none = d2 >= ENV_FAR;
    float m;
    if (band) m = g.voxel * beta;
    else if (!none) m = g.voxel * (sqrtf((float)d2) - 0.5f);
    else m = g.voxel * (float)(g.nx + g.ny + g.nz);
    gstore(sdf + idx, in ? -m : m);
    if (dist2) gstore((uint32_t*)dist2 + idx, none ? 0xFFFFFFFFu : d2);
}

}  // namespace pgr
