// decimate.hip.h -- vertex clustering of a triangle mesh (after open3d's TriangleMesh.simplify_vertex_clustering: Rossignac and
// Borrel's clustering, Lindstrom's quadric placement).  Not on the render path.  DESIGN.md section 19 holds the rule, the
// tolerances and what was measured; parity with open3d is NOT pinned (open3d is not available to the project).
//
// The rule.  Input: vertices float32 [V,3], faces int32 [F,3], voxel float64 > 0, lo float64 [3], contraction in {average,
// quadric}.  All arithmetic is float64 on the float32 coordinates widened exactly; every product, quotient, square root and sum
// is rounded on its own (dec_cell() and dec_position_kernel() switch contraction off for themselves) and no divide becomes a
// multiply by a reciprocal.
//  1. Cells.  lo = (min over the vertices) - voxel / 2 per axis (the caller's reduction).  c = floor((x - lo) / voxel) per axis,
//     clamped to [0, 2^20 - 1].  A cluster is an occupied cell; clusters are numbered in ascending (cz, cy, cx); K is their
//     number.  Every vertex belongs to a cluster, referenced by a face or not.  corner = lo + c * voxel per axis.
//  2. Sums.  The terms of a cluster are taken in a fixed order j = 0, 1, ..: term j goes to partial j mod 64, each partial adds
//     its terms in ascending j starting from 0.0, and the 64 partials are folded p[l] += p[l + d] (l < d) for d = 32, 16, .., 1.
//     The sum is p[0].  (One wave per cluster: a lane per partial, the fold a shuffle butterfly.)
//  3. Average position.  Terms: (x_v - corner) per axis for the cluster's vertices in ascending vertex index.  mean = sum / m,
//     clamped to [0, voxel]; position = corner + mean.
//  4. Quadric position.  Terms: the corners (f, j) whose vertex lies in the cluster, in ascending 3 f + j (so a face with two
//     corners in the cluster counts twice, as open3d's per-vertex walk does).  With q_i = p_i - corner (the corner of the cluster
//     being summed), e1 = q1 - q0, e2 = q2 - q0: n = e1 x e2 (each component (a*b) - (c*d)), a2 = sqrt(((nx*nx) + ny*ny) + nz*nz).
//     A face with a repeated index, an index outside [0, V) or not a2 > 0 is a term of nine zeros.  u = n / a2, w = a2 / 2,
//     d = -(((ux*q0x) + uy*q0y) + uz*q0z), wu = w * u; the term adds wu_r * u_c to A (upper triangle, r <= c) and (w*d) * u to b.
//     Cofactors c00 = Ayy*Azz - Ayz*Ayz, c01 = Axz*Ayz - Axy*Azz, c02 = Axy*Ayz - Axz*Ayy, c11 = Axx*Azz - Axz*Axz,
//     c12 = Axy*Axz - Axx*Ayz, c22 = Axx*Ayy - Axy*Axy; det = ((Axx*c00) + Axy*c01) + Axz*c02;
//     x_r = -((((c_r0*bx) + c_r1*by) + c_r2*bz) / det).  tr = (Axx + Ayy) + Azz, t = tr / 3, threshold = 1e-4 * ((t*t)*t).
//     x is accepted iff |det| > threshold and 0 <= x_r <= voxel on every axis (the second condition is not open3d's: it is
//     what bounds the displacement); then position = corner + x and used_quadric = 1.  Otherwise the average position.
//  5. Faces.  Map the three indices to clusters; drop the face unless all three differ (or an index lies outside [0, V)); rotate
//     it, keeping orientation, so that its smallest index comes first; remove exact duplicates (opposite orientations are
//     different faces and both stay); output in ascending lexicographic (a, b, c).
// The result need not be closed or manifold.
//
// Count, then emit.  The count pass sorts the vertices by cell key (cz << 40 | cy << 20 | cx) and the canonical face triples,
// numbers clusters and distinct faces with two scans and leaves K and F' in counts[2]; nothing in it is floating point beyond
// the cell index.  The emit pass reads what the count pass left in the workspace, groups the 3 F corners by cluster with a third
// sort and runs one wave per cluster.  Everything is deterministic: the sorts are stable LSD radix sorts (8-bit digits; the
// only atomics are LDS integer counts, whose totals do not depend on arrival order), the scans are plain, and there is no
// floating-point atomic anywhere.
//
// The face sort.  With V < 2^21 a triple packs into one key of 3 b bits, b = bits of V (a dropped face's key is V << 2 b, behind
// every kept one).  From V = 2^21 on the triples are sorted in two stable stages: by c, then by (a << 32 | b).  The choice is
// by V, not by K, because K is only known on the device.
#pragma once
#include "pgr_common.h"

namespace pgr {

constexpr int DEC_BLOCK = 256;                      // threads of every kernel here but the scan
constexpr int DEC_ROUNDS = 8;                       // a workgroup walks DEC_ROUNDS * DEC_BLOCK consecutive items
constexpr int DEC_TILE = DEC_BLOCK * DEC_ROUNDS;
constexpr int DEC_SCAN_BLOCK = 1024;
constexpr int DEC_WAVES = DEC_BLOCK / WAVE;
constexpr double DEC_CELL_MAX = 1048575.0;          // 2^20 - 1
constexpr int DEC_PACKED_MAX_BITS = 21;

struct DecGrid { double lo[3]; double voxel; };

__device__ __forceinline__ uint32_t dec_cell(float x, double lo, double voxel) {
#pragma clang fp contract(off)
    const double t = floor(((double)x - lo) / voxel);
    return (uint32_t)fmin(fmax(t, 0.0), DEC_CELL_MAX);                      // (fmax drops a NaN)
}

// ---- scans -----------------------------------------------------------------------------------------------------------
// inclusive scan of v over the workgroup's threads; `wsum` holds one word per wave.  Returns the inclusive value, *total the
// workgroup's sum.  Ends with a barrier, so wsum may be reused at once.
template <int THREADS>
__device__ __forceinline__ uint32_t dec_block_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += t;
    }
    if (lane == WAVE - 1) wsum[w] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < THREADS / WAVE; ++k) {
        const uint32_t s = wsum[k];
        if (k < w) before += s;
        all += s;
    }
    __syncthreads();
    *total = all;
    return incl + before;
}

// in place: a[i] = a[0] + .. + a[i-1]; one workgroup
__global__ __launch_bounds__(DEC_SCAN_BLOCK) void dec_scan_kernel(uint32_t* __restrict__ a, uint32_t n) {
    __shared__ uint32_t wsum[DEC_SCAN_BLOCK / WAVE];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += DEC_SCAN_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n ? a[i] : 0u;
        uint32_t total;
        const uint32_t incl = dec_block_scan<DEC_SCAN_BLOCK>(v, wsum, &total);
        if (i < n) a[i] = carry + incl - v;
        carry += total;
    }
}

// block_tot[b] = the flags of tile b
__global__ __launch_bounds__(DEC_BLOCK) void dec_flag_reduce_kernel(uint32_t n, const uint32_t* __restrict__ flag,
                                                                    uint32_t* __restrict__ block_tot) {
    __shared__ uint32_t wsum[DEC_WAVES];
    const uint32_t base = blockIdx.x * (uint32_t)DEC_TILE;
    uint32_t mine = 0;
    for (int r = 0; r < DEC_ROUNDS; ++r) {
        const uint32_t i = base + r * DEC_BLOCK + threadIdx.x;
        if (i < n) mine += flag[i];
    }
    uint32_t total;
    dec_block_scan<DEC_BLOCK>(mine, wsum, &total);
    if (threadIdx.x == 0) block_tot[blockIdx.x] = total;
}

// out[i] = flag[0] + .. + flag[i]; block_base: the exclusive scan of block_tot
__global__ __launch_bounds__(DEC_BLOCK) void dec_flag_apply_kernel(uint32_t n, const uint32_t* __restrict__ flag,
                                                                   const uint32_t* __restrict__ block_base,
                                                                   uint32_t* __restrict__ out) {
    __shared__ uint32_t wsum[DEC_WAVES];
    const uint32_t base = blockIdx.x * (uint32_t)DEC_TILE;
    uint32_t carry = block_base[blockIdx.x];
    for (int r = 0; r < DEC_ROUNDS; ++r) {
        if (base + r * DEC_BLOCK >= n) break;                               // (the whole workgroup leaves together)
        const uint32_t i = base + r * DEC_BLOCK + threadIdx.x;
        const uint32_t v = i < n ? flag[i] : 0u;
        uint32_t total;
        const uint32_t incl = dec_block_scan<DEC_BLOCK>(v, wsum, &total);
        if (i < n) out[i] = carry + incl;
        carry += total;
    }
}

// ---- the stable radix sort: one 8-bit digit per pass, (key, value) pairs ---------------------------------------------------
// hist[d * n_blocks + b] = the keys of tile b whose digit is d: scanned in that (digit-major) order it is where tile b's first
// key of digit d goes
__global__ __launch_bounds__(DEC_BLOCK) void dec_sort_hist_kernel(uint32_t n, const uint64_t* __restrict__ keys, int shift,
                                                                  uint32_t* __restrict__ hist, uint32_t n_blocks) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)DEC_TILE;
    for (int r = 0; r < DEC_ROUNDS; ++r) {
        const uint32_t i = base + r * DEC_BLOCK + threadIdx.x;
        if (i < n) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];
}

// `offs`: the scanned histogram.  Within a tile the keys go out in input order: round by round, wave by wave, lane by lane.
__global__ __launch_bounds__(DEC_BLOCK) void dec_sort_scatter_kernel(uint32_t n, const uint64_t* __restrict__ keys_in,
                                                                     const uint32_t* __restrict__ vals_in,
                                                                     uint64_t* __restrict__ keys_out,
                                                                     uint32_t* __restrict__ vals_out, int shift,
                                                                     const uint32_t* __restrict__ offs, uint32_t n_blocks) {
    __shared__ uint32_t run[256];                   // where the tile's next key of each digit goes
    __shared__ uint32_t wc[DEC_WAVES][256];         // this round's keys per wave and digit
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    run[threadIdx.x] = offs[(size_t)threadIdx.x * n_blocks + blockIdx.x];
#pragma unroll
    for (int k = 0; k < DEC_WAVES; ++k) wc[k][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)DEC_TILE;
    for (int r = 0; r < DEC_ROUNDS; ++r) {
        if (base + r * DEC_BLOCK >= n) break;                               // (the whole workgroup leaves together)
        const uint32_t i = base + r * DEC_BLOCK + threadIdx.x;
        const bool active = i < n;
        const uint64_t key = active ? keys_in[i] : 0ull;
        const uint32_t val = active ? vals_in[i] : 0u;
        const uint32_t digit = (uint32_t)(key >> shift) & 255u;
        unsigned long long peers = __ballot(active);                        // the wave's lanes that hold the same digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long with = __ballot(active && bit);
            peers &= bit ? with : ~with;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (active && rank == 0) wc[w][digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (active) {
            uint32_t at = run[digit] + rank;
            for (int k = 0; k < w; ++k) at += wc[k][digit];
            if (at < n) {                                                   // (always: the histogram counted these keys)
                keys_out[at] = key;
                vals_out[at] = val;
            }
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int k = 0; k < DEC_WAVES; ++k) { add += wc[k][threadIdx.x]; wc[k][threadIdx.x] = 0; }
        run[threadIdx.x] += add;
        __syncthreads();
    }
}

// ---- clusters ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEC_BLOCK) void dec_vertex_key_kernel(uint32_t n, const float* __restrict__ xyz, DecGrid g,
                                                                   uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * (uint32_t)DEC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t cx = dec_cell(xyz[3 * (size_t)i], g.lo[0], g.voxel), cy = dec_cell(xyz[3 * (size_t)i + 1], g.lo[1], g.voxel),
                   cz = dec_cell(xyz[3 * (size_t)i + 2], g.lo[2], g.voxel);
    keys[i] = (cz << 40) | (cy << 20) | cx;
    vals[i] = i;
}

__global__ __launch_bounds__(DEC_BLOCK) void dec_key_heads_kernel(uint32_t n, const uint64_t* __restrict__ keys,
                                                                  uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * (uint32_t)DEC_BLOCK + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// keys / vals: the sorted vertices; number[i]: clusters up to and including sorted vertex i.  start has n + 1 entries.
__global__ __launch_bounds__(DEC_BLOCK) void dec_cluster_write_kernel(uint32_t n, const uint64_t* __restrict__ keys,
                                                                      const uint32_t* __restrict__ vals,
                                                                      const uint32_t* __restrict__ number,
                                                                      int32_t* __restrict__ cluster_of_vertex,
                                                                      uint32_t* __restrict__ order, uint32_t* __restrict__ start,
                                                                      uint64_t* __restrict__ cluster_key,
                                                                      long long* __restrict__ counts) {
    const uint32_t i = blockIdx.x * (uint32_t)DEC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = number[i] - 1u, v = vals[i];
    if (k >= n || v >= n) return;                                           // (never: number[0] is 1 and vals is a permutation)
    cluster_of_vertex[v] = (int32_t)k;
    order[i] = v;
    if (i == 0 || number[i - 1] != number[i]) {
        start[k] = i;
        cluster_key[k] = keys[i];
    }
    if (i == n - 1) {
        start[k + 1] = n;
        counts[0] = (long long)k + 1;
    }
}

// ---- faces -------------------------------------------------------------------------------------------------------------
// tri[f]: the canonical triple of face f, or (-1, -1, -1) for a dropped one.  bits > 0: the packed key; bits == 0: the key of
// the first of the two stages, c.
__global__ __launch_bounds__(DEC_BLOCK) void dec_face_key_kernel(uint32_t n_faces, const int32_t* __restrict__ faces,
                                                                 uint32_t n_vertices, const int32_t* __restrict__ cluster_of_vertex,
                                                                 int bits, int32_t* __restrict__ tri, uint64_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ vals) {
    const uint32_t f = blockIdx.x * (uint32_t)DEC_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const uint32_t i0 = (uint32_t)faces[3 * (size_t)f], i1 = (uint32_t)faces[3 * (size_t)f + 1], i2 = (uint32_t)faces[3 * (size_t)f + 2];
    int32_t a = -1, b = -1, c = -1;
    if (i0 < n_vertices && i1 < n_vertices && i2 < n_vertices) {
        const int32_t k0 = cluster_of_vertex[i0], k1 = cluster_of_vertex[i1], k2 = cluster_of_vertex[i2];
        if (k0 != k1 && k1 != k2 && k0 != k2) {
            if (k0 < k1 && k0 < k2) { a = k0; b = k1; c = k2; }
            else if (k1 < k0 && k1 < k2) { a = k1; b = k2; c = k0; }
            else { a = k2; b = k0; c = k1; }
        }
    }
    tri[3 * (size_t)f] = a; tri[3 * (size_t)f + 1] = b; tri[3 * (size_t)f + 2] = c;
    uint64_t key;
    if (bits > 0) key = a < 0 ? (uint64_t)n_vertices << (2 * bits) : ((uint64_t)a << (2 * bits)) | ((uint64_t)b << bits) | (uint64_t)c;
    else key = a < 0 ? 0ull : (uint64_t)c;
    keys[f] = key;
    vals[f] = f;
}

// the second stage's key of the face at sorted position i: a << 32 | b; a dropped face's a is n_vertices
__global__ __launch_bounds__(DEC_BLOCK) void dec_face_key2_kernel(uint32_t n_faces, const int32_t* __restrict__ tri,
                                                                  const uint32_t* __restrict__ vals, uint32_t n_vertices,
                                                                  uint64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * (uint32_t)DEC_BLOCK + threadIdx.x;
    if (i >= n_faces) return;
    const uint32_t f = vals[i] < n_faces ? vals[i] : 0u;
    const int32_t a = tri[3 * (size_t)f], b = tri[3 * (size_t)f + 1];
    keys[i] = a < 0 ? (uint64_t)n_vertices << 32 : ((uint64_t)(uint32_t)a << 32) | (uint32_t)b;
}

// perm[i]: the face at sorted position i; flag[i]: it is kept and differs from the one before it
__global__ __launch_bounds__(DEC_BLOCK) void dec_face_heads_kernel(uint32_t n_faces, const int32_t* __restrict__ tri,
                                                                   const uint32_t* __restrict__ vals, uint32_t* __restrict__ perm,
                                                                   uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * (uint32_t)DEC_BLOCK + threadIdx.x;
    if (i >= n_faces) return;
    const uint32_t f = vals[i] < n_faces ? vals[i] : 0u;
    perm[i] = f;
    const int32_t a = tri[3 * (size_t)f], b = tri[3 * (size_t)f + 1], c = tri[3 * (size_t)f + 2];
    bool head = a >= 0;
    if (head && i > 0) {
        const uint32_t g = vals[i - 1] < n_faces ? vals[i - 1] : 0u;
        head = tri[3 * (size_t)g] != a || tri[3 * (size_t)g + 1] != b || tri[3 * (size_t)g + 2] != c;
    }
    flag[i] = head ? 1u : 0u;
}

__global__ void dec_face_total_kernel(uint32_t n_faces, const uint32_t* __restrict__ rank, long long* __restrict__ counts) {
    counts[1] = n_faces ? (long long)rank[n_faces - 1] : 0ll;
}

// rank: the inclusive scan of the head flags
__global__ __launch_bounds__(DEC_BLOCK) void dec_face_emit_kernel(uint32_t n_faces, const int32_t* __restrict__ tri,
                                                                  const uint32_t* __restrict__ perm,
                                                                  const uint32_t* __restrict__ rank, long long capacity,
                                                                  int32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * (uint32_t)DEC_BLOCK + threadIdx.x;
    if (i >= n_faces) return;
    const uint32_t r = rank[i];
    if (r == (i ? rank[i - 1] : 0u) || (long long)r > capacity) return;
    const uint32_t f = perm[i] < n_faces ? perm[i] : 0u;
    out[3 * (size_t)(r - 1)] = tri[3 * (size_t)f];
    out[3 * (size_t)(r - 1) + 1] = tri[3 * (size_t)f + 1];
    out[3 * (size_t)(r - 1) + 2] = tri[3 * (size_t)f + 2];
}

// ---- corners by cluster ----------------------------------------------------------------------------------------------------
// corner t = 3 f + j: its key is the cluster of its vertex, n_vertices for an index outside [0, V)
__global__ __launch_bounds__(DEC_BLOCK) void dec_corner_key_kernel(uint32_t n_corners, const int32_t* __restrict__ faces,
                                                                   uint32_t n_vertices, const int32_t* __restrict__ cluster_of_vertex,
                                                                   uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t t = blockIdx.x * (uint32_t)DEC_BLOCK + threadIdx.x;
    if (t >= n_corners) return;
    const uint32_t v = (uint32_t)faces[t];
    keys[t] = v < n_vertices ? (uint64_t)(uint32_t)cluster_of_vertex[v] : (uint64_t)n_vertices;
    vals[t] = t;
}

// begin / end (zeroed): cluster k's corners are sorted positions [begin[k], end[k])
__global__ __launch_bounds__(DEC_BLOCK) void dec_corner_ranges_kernel(uint32_t n_corners, const uint64_t* __restrict__ keys,
                                                                      uint32_t n_vertices, uint32_t* __restrict__ begin,
                                                                      uint32_t* __restrict__ end) {
    const uint32_t i = blockIdx.x * (uint32_t)DEC_BLOCK + threadIdx.x;
    if (i >= n_corners) return;
    const uint64_t k = keys[i];
    if (k >= n_vertices) return;
    if (i == 0 || keys[i - 1] != k) begin[k] = i;
    if (i == n_corners - 1 || keys[i + 1] != k) end[k] = i + 1;
}

// ---- positions: one wave per cluster ---------------------------------------------------------------------------------------
__device__ __forceinline__ double dec_fold(double p) {
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) p += __shfl_down(p, d, WAVE);   // lane 0 ends with the rule's p[0]
    return p;
}

struct DecPositionArgs {
    DecGrid g;
    uint32_t n_vertices, n_faces;
    const float* xyz;
    const int32_t* faces;
    const uint32_t* order;          // vertices in cluster order
    const uint32_t* start;          // [V + 1]
    const uint64_t* cluster_key;
    const uint32_t* corner;         // corners in cluster order (quadric only)
    const uint32_t* corner_begin;
    const uint32_t* corner_end;
    long long n_clusters;           // the caller's K
    int quadric;
    double* out;
    uint8_t* used_quadric;
};

__global__ __launch_bounds__(DEC_BLOCK) void dec_position_kernel(DecPositionArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (WAVE - 1);
    const long long k = (long long)blockIdx.x * DEC_WAVES + threadIdx.x / WAVE;
    if (k >= a.n_clusters || k >= (long long)a.n_vertices) return;            // (a whole wave leaves; no barrier below)
    const uint64_t key = a.cluster_key[k];
    const double voxel = a.g.voxel;
    double corner[3];
    corner[0] = a.g.lo[0] + (double)(uint32_t)(key & 0xFFFFFu) * voxel;
    corner[1] = a.g.lo[1] + (double)(uint32_t)((key >> 20) & 0xFFFFFu) * voxel;
    corner[2] = a.g.lo[2] + (double)(uint32_t)((key >> 40) & 0xFFFFFu) * voxel;

    const uint32_t v_begin = a.start[k], v_end = min(a.start[k + 1], a.n_vertices);
    double s[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = v_begin + lane; j < v_end; j += WAVE) {
        const uint32_t v = a.order[j];
        if (v >= a.n_vertices) continue;                                    // (never)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += (double)a.xyz[3 * (size_t)v + c] - corner[c];
    }
    const double m = (double)(v_end > v_begin ? v_end - v_begin : 1u);
    double pos[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double mean = dec_fold(s[c]) / m;
        pos[c] = corner[c] + fmin(fmax(mean, 0.0), voxel);
    }
    bool accepted = false;
    if (a.quadric) {
        double q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // Axx Axy Axz Ayy Ayz Azz bx by bz
        const uint32_t c_begin = a.corner_begin[k], c_end = min(a.corner_end[k], 3u * a.n_faces);
        for (uint32_t j = c_begin + lane; j < c_end; j += WAVE) {
            const uint32_t f = a.corner[j] / 3u;
            if (f >= a.n_faces) continue;                                   // (never)
            const uint32_t i0 = (uint32_t)a.faces[3 * (size_t)f], i1 = (uint32_t)a.faces[3 * (size_t)f + 1],
                           i2 = (uint32_t)a.faces[3 * (size_t)f + 2];
            if (i0 >= a.n_vertices || i1 >= a.n_vertices || i2 >= a.n_vertices || i0 == i1 || i1 == i2 || i0 == i2) continue;
            double q0[3], e1[3], e2[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                q0[c] = (double)a.xyz[3 * (size_t)i0 + c] - corner[c];
                e1[c] = ((double)a.xyz[3 * (size_t)i1 + c] - corner[c]) - q0[c];
                e2[c] = ((double)a.xyz[3 * (size_t)i2 + c] - corner[c]) - q0[c];
            }
            const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
            const double a2 = sqrt((nx * nx + ny * ny) + nz * nz);
            if (!(a2 > 0.0)) continue;                                      // (adding the nine zeros changes nothing)
            const double ux = nx / a2, uy = ny / a2, uz = nz / a2, w = a2 / 2.0;
            const double d = -((ux * q0[0] + uy * q0[1]) + uz * q0[2]);
            const double wx = w * ux, wy = w * uy, wz = w * uz, wd = w * d;
            q[0] += wx * ux; q[1] += wx * uy; q[2] += wx * uz; q[3] += wy * uy; q[4] += wy * uz; q[5] += wz * uz;
            q[6] += wd * ux; q[7] += wd * uy; q[8] += wd * uz;
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) q[c] = dec_fold(q[c]);
        const double Axx = q[0], Axy = q[1], Axz = q[2], Ayy = q[3], Ayz = q[4], Azz = q[5];
        const double c00 = Ayy * Azz - Ayz * Ayz, c01 = Axz * Ayz - Axy * Azz, c02 = Axy * Ayz - Axz * Ayy;
        const double c11 = Axx * Azz - Axz * Axz, c12 = Axy * Axz - Axx * Ayz, c22 = Axx * Ayy - Axy * Axy;
        const double det = (Axx * c00 + Axy * c01) + Axz * c02;
        const double t = ((Axx + Ayy) + Azz) / 3.0;
        const double threshold = 1e-4 * ((t * t) * t);
        const double x0 = -(((c00 * q[6] + c01 * q[7]) + c02 * q[8]) / det);
        const double x1 = -(((c01 * q[6] + c11 * q[7]) + c12 * q[8]) / det);
        const double x2 = -(((c02 * q[6] + c12 * q[7]) + c22 * q[8]) / det);
        accepted = fabs(det) > threshold && x0 >= 0.0 && x0 <= voxel && x1 >= 0.0 && x1 <= voxel && x2 >= 0.0 && x2 <= voxel;
        if (accepted) { pos[0] = corner[0] + x0; pos[1] = corner[1] + x1; pos[2] = corner[2] + x2; }
    }
    if (lane == 0) {
        a.out[3 * k] = pos[0]; a.out[3 * k + 1] = pos[1]; a.out[3 * k + 2] = pos[2];
        a.used_quadric[k] = accepted ? 1 : 0;
    }
}

}  // namespace pgr
