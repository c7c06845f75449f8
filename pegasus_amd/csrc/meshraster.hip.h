// meshraster.hip.h -- depth images of triangle meshes at given poses (the BOP toolkit's depth renderer) and their reduction
// to BOP ground truth (scene_gt_info, mask, mask_visib).
//
// pgr_mesh_depth: the rules (tests/mesh_raster_reference.py restates them in NumPy and reproduces the output bit for bit)
//
//   Vertex.     A model point p goes to the camera in float32, no contraction, in this order:
//                   X = ((R[0] p.x + R[1] p.y) + R[2] p.z) + t[0]        (Y with R[3..5], t[1]; Z with R[6..8], t[2])
//               The camera looks along +z:  u = (fx X) / Z + cx,  v = (fy Y) / Z + cy  (IEEE division),  w = 1 / Z.
//   Snap.       Pixel (i, j) samples the image point (i + 0.5, j + 0.5).  Coordinates are snapped to 1/256 pixel in a frame
//               whose integers*256 are the samples:  q = u * 256 - 128 (the product is exact, the difference rounds once),
//               s = rint(min(max(q, -2^30), 2^30)) as int32, round to nearest even; a NaN snaps to -2^30 (fmaxf).
//   Near plane. A face whose three Z are all < near is dropped.  A face with one or two Z < near straddles the plane: it
//               is dropped whole and counted in *straddle_count.  There is no clipping.  A face with a vertex index
//               outside its mesh's vertex range is dropped.
//   Coverage.   Exact integers.  For the edge p -> q:  E_pq(x, y) = (q.x - p.x)(y - p.y) - (q.y - p.y)(x - p.x)  in int64
//               (it is twice a triangle's area inside a box of side <= 2^31: |E| <= 2^62).  area2 = E_ab(c); zero: the
//               face is dropped; negative: b and c swap (no back-face culling), so area2 > 0 and the inside has E > 0.
//               Sample (x, y) = (256 i, 256 j) is covered when every edge has E >= 0 if it is a top or a left edge
//               (q.y - p.y < 0, or q.y == p.y and q.x - p.x > 0; y points down) and E >= 1 otherwise.  Two faces on
//               opposite sides of a shared edge walk it in opposite directions, so a sample on it belongs to exactly one.
//   Depth.      Perspective-correct from the integer edge values, in float32, in this order:
//                   den = ((float)E_bc * w_a + (float)E_ca * w_b) + (float)E_ab * w_c,    z = (float)area2 / den
//               (int64 -> float32 rounds to nearest even, IEEE division).  The sample counts when den > 0 and 0 < z < inf.
//   Nearest.    The canvas holds the float's bits; an integer atomic min picks the nearest surface (positive floats order
//               like their bits), so the result does not depend on the execution order.  Empty pixels (0xFFFFFFFF during
//               the call) end as 0.0.  No float atomics.
//
// Work.  One lane per face: it redoes the three vertex transforms (a vertex is shared by ~6 faces of a marching-tetrahedra
// mesh, but 3 x ~40 VALU instructions per face stay far under the 48 bytes per face the gather costs, and a per-job vertex
// workspace would add a launch and 24 bytes per vertex), clips the face's box to the canvas and walks it when it holds at
// most MESHR_LARGE_BOX samples.  A larger box goes to a queue: one ballot and ONE 64-bit vector atomic per wave hands out
// both the entries and their first 16x16 tile (count << 41 | tiles, so entries are sorted by first tile), and a second
// launch of MESHR_LARGE_WAVES waves splits the total tile count evenly: a wave finds its first entry by bisection, then
// walks tiles, 4 samples per lane.  A 12-face box over a 2400^2 canvas is 45 k tiles over 8192 waves.
//
// pgr_mesh_visibility: the same jobs, vertex, snap, near-plane, coverage and depth rules, the same two launches and the
// same queue (one template parameter on the canvas element), but the canvas element is a 64-bit key
//       key = (uint64)float_bits(z) << 32 | (uint32)(job_index_in_call << 22 | face_index_in_job)
// combined with ONE 64-bit integer atomic min at agent scope: the nearest surface wins; on equal depth bits the lower job
// index, then the lower face index.  Empty pixels are all-ones during the call and 0 after it (z > 0: no valid key is 0).
// A job has at most 2^22 faces, a call at most MESHV_MAX_JOBS = 1024 jobs.  The high word of a finished key equals, bit for
// bit, what pgr_mesh_depth writes for the same call.
//
// pgr_mesh_shade: one lane per canvas pixel turns a key into per-pixel quantities, see the rule above mesh_shade_kernel.
// pgr_mesh_shade_textured: the same kernel's second instantiation reads a textured job's colour from its texture, see the second
// rule above mesh_shade_kernel.
//
// pgr_bop_gt_info: per canvas pixel the sequence of the toolkit's calc_gt_info.py, see the kernel.
#pragma once
#include "pgr_common.h"

namespace pgr {

constexpr int MESHR_JOBS_PER_LAUNCH = 32;
constexpr int MESHR_THREADS = 256;
constexpr int MESHR_LARGE_BOX = 256;                 // samples in the clipped box above which a face is queued
constexpr int MESHR_TILE = 16;
constexpr int MESHR_LARGE_WAVES = 8192;
constexpr int MESHR_TILE_BITS = 41;                  // 2^22 faces x 2^18 tiles of an 8192^2 canvas < 2^41
constexpr int64_t MESHR_MAX_GROUP_FACES = (int64_t)1 << 22;
constexpr int MESHV_MAX_JOBS = PGR_MESH_VISIBILITY_MAX_JOBS;     // jobs of one pgr_mesh_visibility call: 10 bits of the key
constexpr int MESHV_FACE_BITS = 22;                  // 2^22 = MESHR_MAX_GROUP_FACES faces of a job: the key's other 22
static_assert(MESHV_MAX_JOBS <= (1 << (32 - MESHV_FACE_BITS)) && MESHR_MAX_GROUP_FACES <= ((int64_t)1 << MESHV_FACE_BITS), "the key's low word");
constexpr int MESHS_TILE_W = 16, MESHS_TILE_H = 4;   // pgr_mesh_shade: the pixels of one wave
constexpr int MESHS_THREADS = 256;                   // four waves: a 16 x 16 block of pixels
constexpr float MESHR_SNAP_LIMIT = 1073741824.0f;    // 2^30

struct MeshJobDev {
    int32_t v0, nv, f0, nf;
    float R[9], t[3];
    float fx, fy, cx, cy;
    int32_t slot;
    uint32_t block0;                                 // first workgroup of the job in the small launch
};

struct MeshJobTable {
    int32_t count, width, height;
    float near;
    int32_t first;                                   // index in the call of job[0] (the keys of pgr_mesh_visibility)
    MeshJobDev job[MESHR_JOBS_PER_LAUNCH];
};

struct MeshQueueEntry {
    int32_t job, face;
    unsigned long long tile_base;
};

struct MeshTri {
    int32_t ax, ay, bx, by, cx, cy;                  // snapped, area2 > 0
    float wa, wb, wc;
    long long area2;
    int32_t i0, i1, j0, j1;                          // clipped box in pixels, inclusive
};

// what the resolve pass needs besides: a, b, c (after the swap) as vertex indices in the mesh and as camera-frame points
struct MeshCorners {
    int32_t vi[3];
    float P[3][3];
    int32_t flipped;                                 // b and c were swapped: per-corner attributes swap with them
};

__device__ __forceinline__ int32_t mesh_snap(float u) {
    const float q = u * 256.0f - 128.0f;
    return (int32_t)rintf(fminf(fmaxf(q, -MESHR_SNAP_LIMIT), MESHR_SNAP_LIMIT));
}

__device__ __forceinline__ long long mesh_edge(int32_t px, int32_t py, int32_t qx, int32_t qy, int32_t x, int32_t y) {
    return ((long long)qx - px) * ((long long)y - py) - ((long long)qy - py) * ((long long)x - px);
}

// smallest E that still covers: 0 for a top or left edge, 1 otherwise
__device__ __forceinline__ long long mesh_edge_bias(int32_t px, int32_t py, int32_t qx, int32_t qy) {
    const long long dx = (long long)qx - px, dy = (long long)qy - py;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
}

// 0: dropped, 1: to rasterise, 2: dropped because it straddles the near plane
template <bool CORNERS = false>
__device__ __forceinline__ int mesh_setup(const MeshJobDev& J, const float* __restrict__ vertices,
                                          const int32_t* __restrict__ faces, int face, int W, int H, float near, MeshTri& T,
                                          MeshCorners* corners = nullptr) {
    const int32_t* f = faces + 3 * ((size_t)J.f0 + (size_t)face);
    int32_t sx[3], sy[3];
    float w[3];
    int32_t vid[3];
    float cam[3][3];
    int behind = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int32_t vi = f[q];
        if (vi < 0 || vi >= J.nv) return 0;
        const float* p = vertices + 3 * ((size_t)J.v0 + (size_t)vi);
        const float px = p[0], py = p[1], pz = p[2];
        const float X = ((J.R[0] * px + J.R[1] * py) + J.R[2] * pz) + J.t[0];
        const float Y = ((J.R[3] * px + J.R[4] * py) + J.R[5] * pz) + J.t[1];
        const float Z = ((J.R[6] * px + J.R[7] * py) + J.R[8] * pz) + J.t[2];
        behind += Z < near ? 1 : 0;
        if constexpr (CORNERS) { vid[q] = vi; cam[q][0] = X; cam[q][1] = Y; cam[q][2] = Z; }
        sx[q] = mesh_snap((J.fx * X) / Z + J.cx);
        sy[q] = mesh_snap((J.fy * Y) / Z + J.cy);
        w[q] = 1.0f / Z;
    }
    if (behind == 3) return 0;
    if (behind) return 2;
    long long area2 = mesh_edge(sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
    if (area2 == 0) return 0;
    int b = 1, c = 2;
    if (area2 < 0) { b = 2; c = 1; area2 = -area2; }
    T.ax = sx[0]; T.ay = sy[0]; T.bx = sx[b]; T.by = sy[b]; T.cx = sx[c]; T.cy = sy[c];
    T.wa = w[0]; T.wb = w[b]; T.wc = w[c];
    T.area2 = area2;
    if constexpr (CORNERS) {
        const int order[3] = {0, b, c};
        corners->flipped = b == 2 ? 1 : 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            corners->vi[q] = vid[order[q]];
#pragma unroll
            for (int d = 0; d < 3; ++d) corners->P[q][d] = cam[order[q]][d];
        }
    }
    const int32_t minx = min(sx[0], min(sx[1], sx[2])), maxx = max(sx[0], max(sx[1], sx[2]));
    const int32_t miny = min(sy[0], min(sy[1], sy[2])), maxy = max(sy[0], max(sy[1], sy[2]));
    T.i0 = max(0, (minx + 255) >> 8);
    T.i1 = min(W - 1, maxx >> 8);
    T.j0 = max(0, (miny + 255) >> 8);
    T.j1 = min(H - 1, maxy >> 8);
    return (T.i0 <= T.i1 && T.j0 <= T.j1) ? 1 : 0;
}

// the canvas element: the depth's bits (pgr_mesh_depth), or the key depth << 32 | id (pgr_mesh_visibility)
__device__ __forceinline__ void mesh_min(uint32_t* pix, uint32_t zbits, uint32_t) {
    __hip_atomic_fetch_min((PGR_GLOBAL uint32_t*)pix, zbits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void mesh_min(uint64_t* pix, uint32_t zbits, uint32_t id) {
    __hip_atomic_fetch_min((PGR_GLOBAL uint64_t*)pix, ((uint64_t)zbits << 32) | id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename Pix>
__device__ __forceinline__ void mesh_sample(const MeshTri& T, long long ea, long long eb, long long ec, Pix* pix, uint32_t id) {
    const float den = ((float)ea * T.wa + (float)eb * T.wb) + (float)ec * T.wc;
    const float z = (float)T.area2 / den;
    if (den > 0.f && z > 0.f && z < INFINITY) mesh_min(pix, __float_as_uint(z), id);
}

// the job of a workgroup of the small launch
__device__ __forceinline__ int mesh_job_of_block(const MeshJobTable& T, uint32_t block) {
    int k = 0;
    for (int q = 1; q < T.count; ++q)
        if (block >= T.job[q].block0) k = q;
    return k;
}

template <typename Pix>
__global__ __launch_bounds__(MESHR_THREADS) void mesh_small_kernel(const MeshJobTable T, const float* __restrict__ vertices,
                                                                  const int32_t* __restrict__ faces, Pix* __restrict__ out,
                                                                  size_t plane, unsigned long long* __restrict__ qctr,
                                                                  MeshQueueEntry* __restrict__ queue, long long queue_cap,
                                                                  int32_t* __restrict__ straddle) {
    const int k = mesh_job_of_block(T, blockIdx.x);
    const MeshJobDev& J = T.job[k];
    const int lane = threadIdx.x & (WAVE - 1);
    const long long face = (long long)(blockIdx.x - J.block0) * MESHR_THREADS + threadIdx.x;
    MeshTri tri;
    int status = 0;
    if (face < J.nf) status = mesh_setup(J, vertices, faces, (int)face, T.width, T.height, T.near, tri);
    const unsigned long long sb = __ballot(status == 2);
    if (sb && lane == 0) atomicAdd(straddle, (int32_t)__popcll(sb));
    unsigned long long ntiles = 0;
    if (status == 1) {
        const long long bw = tri.i1 - tri.i0 + 1, bh = tri.j1 - tri.j0 + 1;
        if (bw * bh > MESHR_LARGE_BOX)
            ntiles = (unsigned long long)(((bw + MESHR_TILE - 1) / MESHR_TILE) * ((bh + MESHR_TILE - 1) / MESHR_TILE));
    }
    const bool large = ntiles != 0;
    const unsigned long long lb = __ballot(large);
    if (lb) {                                        // wave-uniform: every lane takes part in the scan
        unsigned long long incl = ntiles;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d, WAVE);
            if (lane >= d) incl += up;
        }
        const unsigned long long total = __shfl(incl, WAVE - 1, WAVE);
        unsigned long long base = 0;
        if (lane == 0)
            base = __hip_atomic_fetch_add((PGR_GLOBAL unsigned long long*)qctr,
                                          ((unsigned long long)__popcll(lb) << MESHR_TILE_BITS) | total, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
        base = __shfl(base, 0, WAVE);
        if (large) {
            const long long idx = (long long)(base >> MESHR_TILE_BITS) + __popcll(lb & ((1ull << lane) - 1ull));
            if (idx < queue_cap)
                queue[idx] = MeshQueueEntry{k, (int32_t)face, (base & ((1ull << MESHR_TILE_BITS) - 1ull)) + incl - ntiles};
        }
    }
    if (status != 1 || large) return;
    // walk the box: edge values at the row's first sample, then one add per sample
    Pix* canvas = out + (size_t)J.slot * plane;
    const uint32_t id = ((uint32_t)(T.first + k) << MESHV_FACE_BITS) | (uint32_t)face;
    const long long ba = mesh_edge_bias(tri.bx, tri.by, tri.cx, tri.cy), bb = mesh_edge_bias(tri.cx, tri.cy, tri.ax, tri.ay),
                    bc = mesh_edge_bias(tri.ax, tri.ay, tri.bx, tri.by);
    const long long sa = -256ll * ((long long)tri.cy - tri.by), sbx = -256ll * ((long long)tri.ay - tri.cy),
                    sc = -256ll * ((long long)tri.by - tri.ay);
    for (int j = tri.j0; j <= tri.j1; ++j) {
        long long ea = mesh_edge(tri.bx, tri.by, tri.cx, tri.cy, tri.i0 << 8, j << 8);
        long long eb = mesh_edge(tri.cx, tri.cy, tri.ax, tri.ay, tri.i0 << 8, j << 8);
        long long ec = mesh_edge(tri.ax, tri.ay, tri.bx, tri.by, tri.i0 << 8, j << 8);
        for (int i = tri.i0; i <= tri.i1; ++i) {
            if (ea >= ba && eb >= bb && ec >= bc) mesh_sample(tri, ea, eb, ec, canvas + (size_t)j * T.width + i, id);
            ea += sa; eb += sbx; ec += sc;
        }
    }
}

template <typename Pix>
__global__ __launch_bounds__(MESHR_THREADS) void mesh_large_kernel(const MeshJobTable T, const float* __restrict__ vertices,
                                                                  const int32_t* __restrict__ faces, Pix* __restrict__ out,
                                                                  size_t plane, const unsigned long long* __restrict__ qctr,
                                                                  const MeshQueueEntry* __restrict__ queue, long long queue_cap) {
    const unsigned long long packed = *qctr;
    const unsigned long long total = packed & ((1ull << MESHR_TILE_BITS) - 1ull);
    const long long count = min((long long)(packed >> MESHR_TILE_BITS), queue_cap);
    if (total == 0 || count == 0) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long wave = ((unsigned long long)blockIdx.x * MESHR_THREADS + threadIdx.x) / WAVE;
    const unsigned long long n_waves = (unsigned long long)gridDim.x * (MESHR_THREADS / WAVE);
    const unsigned long long per = (total + n_waves - 1) / n_waves;
    unsigned long long k = wave * per;
    const unsigned long long k_end = min(total, k + per);
    if (k >= k_end) return;
    long long lo = 0, hi = count - 1;                // the last entry whose first tile is <= k
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (queue[mid].tile_base <= k) lo = mid; else hi = mid - 1;
    }
    for (long long e = lo; e < count && k < k_end; ++e) {
        const MeshQueueEntry q = queue[e];
        const unsigned long long next = e + 1 < count ? queue[e + 1].tile_base : total;
        const unsigned long long stop = min(k_end, next);
        const int job = __builtin_amdgcn_readfirstlane(q.job);           // the entry is the wave's: a scalar index into the table
        if (job < 0 || job >= T.count) { k = stop; continue; }
        const MeshJobDev& J = T.job[job];
        MeshTri tri;
        if (q.face < 0 || q.face >= J.nf || mesh_setup(J, vertices, faces, q.face, T.width, T.height, T.near, tri) != 1) {
            k = stop;
            continue;
        }
        Pix* canvas = out + (size_t)J.slot * plane;
        const uint32_t id = ((uint32_t)(T.first + job) << MESHV_FACE_BITS) | (uint32_t)q.face;
        const unsigned long long tiles_x = (unsigned long long)((tri.i1 - tri.i0 + MESHR_TILE) / MESHR_TILE);
        const long long ba = mesh_edge_bias(tri.bx, tri.by, tri.cx, tri.cy), bb = mesh_edge_bias(tri.cx, tri.cy, tri.ax, tri.ay),
                        bc = mesh_edge_bias(tri.ax, tri.ay, tri.bx, tri.by);
        for (; k < stop; ++k) {
            const unsigned long long t = k - q.tile_base;
            const int i = tri.i0 + (int)(t % tiles_x) * MESHR_TILE + (lane & (MESHR_TILE - 1));
            const int jt = tri.j0 + (int)(t / tiles_x) * MESHR_TILE + (lane >> 4);
            if (i > tri.i1) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = jt + 4 * r;
                if (j > tri.j1) break;
                const long long ea = mesh_edge(tri.bx, tri.by, tri.cx, tri.cy, i << 8, j << 8);
                const long long eb = mesh_edge(tri.cx, tri.cy, tri.ax, tri.ay, i << 8, j << 8);
                const long long ec = mesh_edge(tri.ax, tri.ay, tri.bx, tri.by, i << 8, j << 8);
                if (ea >= ba && eb >= bb && ec >= bc) mesh_sample(tri, ea, eb, ec, canvas + (size_t)j * T.width + i, id);
            }
        }
    }
}

// empty pixels end as 0.0 (as key 0)
template <typename Pix>
__global__ __launch_bounds__(256) void mesh_finalize_kernel(Pix* __restrict__ out, size_t n) {
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256)
        if (out[p] == (Pix)~(Pix)0) out[p] = 0u;
}

// ---- pgr_mesh_shade: a visibility buffer resolved to per-pixel quantities ----------------------------------------------
// One lane per canvas pixel (i, j) of a slot.  key == 0: the pixel is empty.  Otherwise job = low word >> 22, face = low
// word & (2^22 - 1); the lane redoes mesh_setup for that face of that job (the same snapped coordinates, the same swap of b
// and c when area2 < 0) and takes the three int64 edge values at the sample (256 i, 256 j).  All arithmetic is float32
// without contraction, in the order written here (tests/mesh_shade_reference.py restates it in NumPy):
//
//   Weights.    la = (float)E_bc * w_a,  lb = (float)E_ca * w_b,  lc = (float)E_ab * w_c,  den = (la + lb) + lc  (the depth
//               rule's den).  An attribute A with vertex values A_a, A_b, A_c is  ((la A_a + lb A_b) + lc A_c) / den;  the
//               values are swapped together with b and c when the face was flipped.
//   depth       the key's high word; 0 where empty.          face_id, job_id   int32; -1 where empty.
//   xyz         the attribute rule on the face's model vertices (the model coordinates of the surface point); 0 where empty.
//   Eye point.  P = R xyz + t in the vertex rule's order.  d = light - P,  L = d / sqrt((d.x d.x + d.y d.y) + d.z d.z)
//               (every component divided by the root).
//   normal      camera frame, unit length; 0 where empty.
//               flat (normals == NULL):  m = cross(P_b - P_a, P_c - P_a) of the three camera-frame vertices of the vertex
//                   rule, m.x = u.y v.z - u.z v.y and cyclic;  n = m / sqrt((m.x m.x + m.y m.y) + m.z m.z);  n is negated
//                   when (n.x P.x + n.y P.y) + n.z P.z > 0: it faces the viewer whatever the winding.
//               smooth:  the attribute rule on the model normals, m = R a in the vertex rule's order without t, normalised
//                   alike; no flip.
//               A root that is zero or not finite gives normal 0 and diffuse 0.
//   rgb         diffuse = fmax((L.x n.x + L.y n.y) + L.z n.z, 0)  (a NaN counts as 0),  light_w = fmin(ambient + diffuse, 1),
//               rgb = light_w * colour;  colour is the attribute rule on `colors`, or the job's surf_color when colors == NULL.
//               Empty pixels get bg.
// Division and sqrtf are the correctly rounded ones (hipcc's default; the build sets no fast-math flag).
//
// A wave owns a 16 x 4 pixel tile, a workgroup 16 x 16: the lanes of a wave gather few distinct faces.  No LDS.  The job
// table does not fit a kernel argument (1024 jobs): the entry writes it to the workspace, 32 jobs per tiny launch.
struct MeshShadeJobDev {
    MeshJobDev job;
    float surf[3];
};

struct MeshShadeTable {
    int32_t count, first;
    MeshShadeJobDev job[MESHR_JOBS_PER_LAUNCH];
};

struct MeshShadeArgs {
    int32_t n_jobs, width, height, n_slots;
    float near, ambient;
    float light[3], bg[3];
    const float* vertices;
    const int32_t* faces;
    const float* normals;
    const float* colors;
    const uint64_t* keys;
    const MeshShadeJobDev* jobs;
    float* depth;
    int32_t* face_id;
    int32_t* job_id;
    float* xyz;
    float* normal;
    float* rgb;
};

__global__ __launch_bounds__(64) void mesh_shade_table_kernel(const MeshShadeTable T, MeshShadeJobDev* __restrict__ table) {
    if ((int)threadIdx.x < T.count) table[T.first + threadIdx.x] = T.job[threadIdx.x];
}

__device__ __forceinline__ float mesh_attr(float la, float lb, float lc, float den, float a, float b, float c) {
    return ((la * a + lb * b) + lc * c) / den;
}

__device__ __forceinline__ void mesh_store3(float* out, size_t p, float x, float y, float z) {
    if (!out) return;
    out[3 * p + 0] = x; out[3 * p + 1] = y; out[3 * p + 2] = z;
}

// ---- pgr_mesh_shade_textured: the same resolve, the colour read from a texture ------------------------------------------
// The second instantiation of mesh_shade_kernel.  Everything above holds unchanged; in addition (float32, no contraction,
// correctly rounded division; tests/mesh_texture_reference.py restates it in NumPy):
//
//   uv          (u, v) = the attribute rule on the face's three corner values corner_uv[face][a, b, c], b's and c's swapped
//               when the face was flipped: perspective-correct, like xyz.  Written for every covered pixel when corner_uv
//               is given (whatever the job's texture), 0 where empty or without corner_uv.
//   Texture.    W x H texels of 3 bytes, rows tightly packed at a byte offset of the texel buffer; stored row 0 is the
//               image's top row.  v = 0 is the image's BOTTOM row (the toolkit flips the image before OpenGL sees it):
//               texel (i, j) is stored at row H - 1 - j.  Clamp to edge:
//                   clamp(x, n) = x >= 0 ? (x < n ? (int)x : n - 1) : 0          (so a NaN gives index 0)
//   nearest     i = clamp(floorf(u * W), W),  j = clamp(floorf(v * H), H),  colour = (float)texel / 255.0f.
//   bilinear    x = u * W - 0.5f,  x0 = floorf(x),  fx = x - x0 (0 when that is a NaN: a NaN or infinite coordinate),
//               i0 = clamp(x0, W),  i1 = clamp(x0 + 1, W);  y, y0, fy, j0, j1 alike from v and H.  With c = (float)texel / 255.0f:
//                   top = (1 - fx) c(i0, j0) + fx c(i1, j0),   bot = (1 - fx) c(i0, j1) + fx c(i1, j1),
//                   colour = (1 - fy) top + fy bot             every operation rounded on its own.
//   rgb         light_w * colour with light_w as above.  A job whose texture index is -1 follows the colour rule above
//               (vertex colours or its surf colour): all its outputs are pgr_mesh_shade's, bit for bit.
// Plain byte loads: gfx950 has no image-sampling path for HIP, and the result is pinned bit for bit anyway.
struct MeshJobTexDev {
    unsigned long long offset;                       // of the texture's first byte in the texel buffer
    int32_t w, h;                                    // w == 0: the job is untextured
};

struct MeshTexTable {
    int32_t count, first;
    MeshJobTexDev tex[MESHR_JOBS_PER_LAUNCH];
};

struct MeshTextureArgs {
    const float* corner_uv;
    const uint8_t* texels;
    const MeshJobTexDev* job_tex;
    int32_t bilinear;
    float* uv;
};

__global__ __launch_bounds__(64) void mesh_tex_table_kernel(const MeshTexTable T, MeshJobTexDev* __restrict__ table) {
    if ((int)threadIdx.x < T.count) table[T.first + threadIdx.x] = T.tex[threadIdx.x];
}

__device__ __forceinline__ int mesh_tex_clamp(float x, int n) { return x >= 0.f ? (x < (float)n ? (int)x : n - 1) : 0; }

// channel d of texel (i, j), j counted from the image's bottom row
__device__ __forceinline__ float mesh_texel(const uint8_t* __restrict__ tex, int w, int h, int i, int j, int d) {
    return (float)tex[((size_t)(h - 1 - j) * (size_t)w + (size_t)i) * 3 + d] / 255.0f;
}

__device__ __forceinline__ void mesh_tex_sample(const uint8_t* __restrict__ tex, int w, int h, float u, float v, bool bilinear,
                                                float col[3]) {
    if (!bilinear) {
        const int i = mesh_tex_clamp(floorf(u * (float)w), w), j = mesh_tex_clamp(floorf(v * (float)h), h);
#pragma unroll
        for (int d = 0; d < 3; ++d) col[d] = mesh_texel(tex, w, h, i, j, d);
        return;
    }
    const float x = u * (float)w - 0.5f, y = v * (float)h - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    float fx = x - x0, fy = y - y0;
    if (fx != fx) fx = 0.f;
    if (fy != fy) fy = 0.f;
    const int i0 = mesh_tex_clamp(x0, w), i1 = mesh_tex_clamp(x0 + 1.0f, w);
    const int j0 = mesh_tex_clamp(y0, h), j1 = mesh_tex_clamp(y0 + 1.0f, h);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float top = (1.0f - fx) * mesh_texel(tex, w, h, i0, j0, d) + fx * mesh_texel(tex, w, h, i1, j0, d);
        const float bot = (1.0f - fx) * mesh_texel(tex, w, h, i0, j1, d) + fx * mesh_texel(tex, w, h, i1, j1, d);
        col[d] = (1.0f - fy) * top + fy * bot;
    }
}

template <bool TEXTURED>
__global__ __launch_bounds__(MESHS_THREADS) void mesh_shade_kernel(const MeshShadeArgs A, const MeshTextureArgs X) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int i = blockIdx.x * MESHS_TILE_W + (lane & (MESHS_TILE_W - 1));
    const int j = (blockIdx.y * (MESHS_THREADS / WAVE) + wave) * MESHS_TILE_H + lane / MESHS_TILE_W;
    if (i >= A.width || j >= A.height) return;
    const size_t plane = (size_t)A.width * A.height;
    for (int slot = blockIdx.z; slot < A.n_slots; slot += gridDim.z) {
        const size_t p = (size_t)slot * plane + (size_t)j * A.width + i;
        const uint64_t key = A.keys[p];
        float depth = 0.f, x[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f}, rgb[3] = {A.bg[0], A.bg[1], A.bg[2]};
        float uv[2] = {0.f, 0.f};
        int32_t fid = -1, jid = -1;
        const int job = (int)((uint32_t)key >> MESHV_FACE_BITS), face = (int)((uint32_t)key & ((1u << MESHV_FACE_BITS) - 1u));
        MeshTri tri;
        MeshCorners cor;
        // a key the visibility pass wrote names a face that sets up; anything else is treated as empty, never followed
        if (key != 0 && job < A.n_jobs && face < A.jobs[job].job.nf &&
            mesh_setup<true>(A.jobs[job].job, A.vertices, A.faces, face, A.width, A.height, A.near, tri, &cor) == 1) {
            const MeshShadeJobDev& S = A.jobs[job];
            const MeshJobDev& J = S.job;
            depth = __uint_as_float((uint32_t)(key >> 32));
            fid = face; jid = job;
            const float la = (float)mesh_edge(tri.bx, tri.by, tri.cx, tri.cy, i << 8, j << 8) * tri.wa;
            const float lb = (float)mesh_edge(tri.cx, tri.cy, tri.ax, tri.ay, i << 8, j << 8) * tri.wb;
            const float lc = (float)mesh_edge(tri.ax, tri.ay, tri.bx, tri.by, i << 8, j << 8) * tri.wc;
            const float den = (la + lb) + lc;
            const float* va = A.vertices + 3 * ((size_t)J.v0 + (size_t)cor.vi[0]);
            const float* vb = A.vertices + 3 * ((size_t)J.v0 + (size_t)cor.vi[1]);
            const float* vc = A.vertices + 3 * ((size_t)J.v0 + (size_t)cor.vi[2]);
#pragma unroll
            for (int d = 0; d < 3; ++d) x[d] = mesh_attr(la, lb, lc, den, va[d], vb[d], vc[d]);
            float P[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) P[d] = ((J.R[3 * d] * x[0] + J.R[3 * d + 1] * x[1]) + J.R[3 * d + 2] * x[2]) + J.t[d];
            float m[3];
            if (A.normals) {
                const float* na = A.normals + 3 * ((size_t)J.v0 + (size_t)cor.vi[0]);
                const float* nb = A.normals + 3 * ((size_t)J.v0 + (size_t)cor.vi[1]);
                const float* nc = A.normals + 3 * ((size_t)J.v0 + (size_t)cor.vi[2]);
                float a[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) a[d] = mesh_attr(la, lb, lc, den, na[d], nb[d], nc[d]);
#pragma unroll
                for (int d = 0; d < 3; ++d) m[d] = (J.R[3 * d] * a[0] + J.R[3 * d + 1] * a[1]) + J.R[3 * d + 2] * a[2];
            } else {
                float u[3], v[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) { u[d] = cor.P[1][d] - cor.P[0][d]; v[d] = cor.P[2][d] - cor.P[0][d]; }
                m[0] = u[1] * v[2] - u[2] * v[1];
                m[1] = u[2] * v[0] - u[0] * v[2];
                m[2] = u[0] * v[1] - u[1] * v[0];
            }
            const float mlen = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
            float diffuse = 0.f;
            if (mlen > 0.f && mlen < INFINITY) {
#pragma unroll
                for (int d = 0; d < 3; ++d) n[d] = m[d] / mlen;
                if (!A.normals && (n[0] * P[0] + n[1] * P[1]) + n[2] * P[2] > 0.f) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) n[d] = -n[d];
                }
                float L[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) L[d] = A.light[d] - P[d];
                const float llen = sqrtf((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]);
#pragma unroll
                for (int d = 0; d < 3; ++d) L[d] = L[d] / llen;
                diffuse = fmaxf((L[0] * n[0] + L[1] * n[1]) + L[2] * n[2], 0.f);
            }
            const float light_w = fminf(A.ambient + diffuse, 1.f);
            bool textured = false;
            if constexpr (TEXTURED) {
                if (X.corner_uv) {
                    const float* c = X.corner_uv + 6 * ((size_t)J.f0 + (size_t)face);
                    const int qb = cor.flipped ? 2 : 1, qc = cor.flipped ? 1 : 2;
#pragma unroll
                    for (int d = 0; d < 2; ++d) uv[d] = mesh_attr(la, lb, lc, den, c[d], c[2 * qb + d], c[2 * qc + d]);
                    const MeshJobTexDev tex = X.job_tex[job];
                    if (A.rgb && tex.w > 0) {
                        textured = true;
                        float col[3];
                        mesh_tex_sample(X.texels + tex.offset, tex.w, tex.h, uv[0], uv[1], X.bilinear != 0, col);
#pragma unroll
                        for (int d = 0; d < 3; ++d) rgb[d] = light_w * col[d];
                    }
                }
            }
            if (A.rgb && !textured) {
                float col[3] = {S.surf[0], S.surf[1], S.surf[2]};
                if (A.colors) {
                    const float* ca = A.colors + 3 * ((size_t)J.v0 + (size_t)cor.vi[0]);
                    const float* cb = A.colors + 3 * ((size_t)J.v0 + (size_t)cor.vi[1]);
                    const float* cc = A.colors + 3 * ((size_t)J.v0 + (size_t)cor.vi[2]);
#pragma unroll
                    for (int d = 0; d < 3; ++d) col[d] = mesh_attr(la, lb, lc, den, ca[d], cb[d], cc[d]);
                }
#pragma unroll
                for (int d = 0; d < 3; ++d) rgb[d] = light_w * col[d];
            }
        }
        if (A.depth) A.depth[p] = depth;
        if (A.face_id) A.face_id[p] = fid;
        if (A.job_id) A.job_id[p] = jid;
        mesh_store3(A.xyz, p, x[0], x[1], x[2]);
        mesh_store3(A.normal, p, n[0], n[1], n[2]);
        mesh_store3(A.rgb, p, rgb[0], rgb[1], rgb[2]);
        if constexpr (TEXTURED) {
            if (X.uv) { X.uv[2 * p + 0] = uv[0]; X.uv[2 * p + 1] = uv[1]; }
        }
    }
}

// ---- BOP ground truth from a depth canvas ---------------------------------------------------------------------------
// The toolkit's scripts/calc_gt_info.py:117-177 for one (object, image) pair, per pixel of the canvas:
//   silhouette over the WHOLE canvas: depth > 0 (px_count_all, bbox_obj in image coordinates = canvas - margin);
//   inside the image window: distance images as misc.depth_im_to_dist_im_fast computes them, in float64 --
//       dist = sqrt(((x - cx) / fx * d)^2 + ((y - cy) / fy * d)^2 + d^2)   at the integer pixel index, summed left to right
//   -- both rounded to float32, d_diff = dist_model - dist_test in float32, and (visibility.py:34-37, mode bop19)
//       visib = (d_diff <= delta or dist_test == 0) and dist_model > 0.
// One int32 row per job: px_count_all, px_count_valid, px_count_visib, then min x, min y, max x, max y of the silhouette
// and of the visible mask (image coordinates, INT32_MAX / INT32_MIN when empty).  Integer atomics only.
constexpr int GT_JOBS_PER_LAUNCH = PGR_GT_INFO_JOBS_PER_LAUNCH;
constexpr int GT_STATS = 11;
constexpr int GT_BLOCKS_X = PGR_GT_INFO_BLOCKS_X;

struct GtJobDev {
    int32_t slot, frame;
    double fx, fy, cx, cy;
};

struct GtJobTable {
    int32_t count, first;
    int32_t canvas_w, canvas_h, width, height, mx, my;
    float delta;
    GtJobDev job[GT_JOBS_PER_LAUNCH];
};

__global__ __launch_bounds__(256) void gt_info_init_kernel(int32_t* __restrict__ stats, int n_jobs) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_jobs * GT_STATS) return;
    const int s = e % GT_STATS;
    stats[e] = s < 3 ? 0 : (((s - 3) & 2) ? INT32_MIN : INT32_MAX);
}

__device__ __forceinline__ double gt_dist(double d, int x, int y, double fx, double fy, double cx, double cy) {
    const double X = (((double)x - cx) / fx) * d, Y = (((double)y - cy) / fy) * d;
    return sqrt((X * X + Y * Y) + d * d);
}

__global__ __launch_bounds__(256) void gt_info_kernel(const GtJobTable T, const float* __restrict__ canvases,
                                                      const float* __restrict__ scene_depth, uint8_t* __restrict__ mask,
                                                      uint8_t* __restrict__ mask_visib, int32_t* __restrict__ stats) {
    const GtJobDev& J = T.job[blockIdx.y];
    const size_t job = (size_t)T.first + blockIdx.y;
    const size_t plane = (size_t)T.canvas_w * T.canvas_h, image = (size_t)T.width * T.height;
    const float* canvas = canvases + (size_t)J.slot * plane;
    const float* scene = scene_depth + (size_t)J.frame * image;
    int32_t v[GT_STATS];
#pragma unroll
    for (int s = 0; s < GT_STATS; ++s) v[s] = s < 3 ? 0 : (((s - 3) & 2) ? INT32_MIN : INT32_MAX);
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < plane; p += (size_t)gridDim.x * 256) {
        const int yc = (int)(p / T.canvas_w), xc = (int)(p % T.canvas_w);
        const int x = xc - T.mx, y = yc - T.my;
        const float d = canvas[p];
        if (d > 0.f) {
            v[0] += 1;
            v[3] = min(v[3], x); v[4] = min(v[4], y); v[5] = max(v[5], x); v[6] = max(v[6], y);
        }
        if (x < 0 || y < 0 || x >= T.width || y >= T.height) continue;
        const float dt = scene[(size_t)y * T.width + x];
        const float dist_model = (float)gt_dist((double)d, x, y, J.fx, J.fy, J.cx, J.cy);
        const float dist_test = (float)gt_dist((double)dt, x, y, J.fx, J.fy, J.cx, J.cy);
        const float diff = dist_model - dist_test;
        const bool in_mask = dist_model > 0.f;
        const bool visible = (diff <= T.delta || dist_test == 0.f) && in_mask;
        mask[job * image + (size_t)y * T.width + x] = in_mask ? 1 : 0;
        mask_visib[job * image + (size_t)y * T.width + x] = visible ? 1 : 0;
        if (in_mask && dist_test > 0.f) v[1] += 1;
        if (visible) {
            v[2] += 1;
            v[7] = min(v[7], x); v[8] = min(v[8], y); v[9] = max(v[9], x); v[10] = max(v[10], y);
        }
    }
    if (!__ballot(v[0] != 0 || v[1] != 0 || v[2] != 0)) return;      // nothing of the object in this wave's pixels
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
#pragma unroll
        for (int s = 0; s < GT_STATS; ++s) {
            const int32_t o = __shfl_xor(v[s], d, WAVE);
            v[s] = s < 3 ? v[s] + o : (((s - 3) & 2) ? max(v[s], o) : min(v[s], o));
        }
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        int32_t* row = stats + job * GT_STATS;
#pragma unroll
        for (int s = 0; s < GT_STATS; ++s) {
            if (s < 3) { if (v[s]) atomicAdd(row + s, v[s]); }
            else if ((s - 3) & 2) atomicMax(row + s, v[s]);
            else atomicMin(row + s, v[s]);
        }
    }
}

}  // namespace pgr
