// mesh.hip.h -- object meshes from rendered views: TSDF fusion with space carving, then marching tetrahedra.
//
// tsdf_integrate: one thread per grid point, 256-thread workgroups over 8x8x4 bricks (a wave's points project onto
// neighbouring pixels); the views' constants sit in LDS.  Every point walks the views in order in float32 with no
// fused multiply-adds, so tests/mesh_reference.py reproduces it bit for bit.
//
// Marching tetrahedra: every cell splits into the 6 Kuhn tetrahedra around its (0,0,0)-(1,1,1) diagonal, so
// neighbouring cells agree on every face diagonal and the mesh is closed and manifold by construction.  Each grid point
// owns 7 edges (+x, +y, +z, +x+y, +x+z, +y+z, +x+y+z) and emits the vertex of every crossed one.  The output order is
// fixed -- vertices by (point, edge), faces by (cell, tetrahedron, triangle) -- through a device-wide reduce-then-scan:
// march_count reduces the per-point vertex and triangle counts of a tile of MARCH_TILE points, march_scan scans the
// tile totals, and march_vbase rescans inside each tile to give every point its first vertex's index; the face kernel
// rescans the triangle counts the same way.  No float atomics anywhere: the results are identical from run to run.
#pragma once
#include "pgr_common.h"

namespace pgr {

constexpr int TSDF_MAX_VIEWS = 256;
constexpr int TSDF_BX = 8, TSDF_BY = 8, TSDF_BZ = 4;     // the brick of one 256-thread workgroup
constexpr int MARCH_THREADS = 256;
constexpr int MARCH_PER_THREAD = 4;
constexpr int MARCH_TILE = MARCH_THREADS * MARCH_PER_THREAD;
constexpr int MARCH_SCAN_THREADS = 1024;

struct MeshGrid {
    int nx, ny, nz;
    float ox, oy, oz, voxel;
};

struct TsdfArgs {
    MeshGrid g;
    int n_views, width, height;
    float cx, cy;                                  // (W-1)/2, (H-1)/2
    float truncation, alpha_min;
    const float* depth;                            // [V,H,W]
    const float* final_T;                          // [V,H,W]
    float* sdf;                                    // [nz,ny,nx]
    const float* view[TSDF_MAX_VIEWS];             // world_view_transform, transposed storage
    float fx[TSDF_MAX_VIEWS], fy[TSDF_MAX_VIEWS];  // W / (2 tanfovx), H / (2 tanfovy)
};

__device__ __forceinline__ float grid_coord(float o, float voxel, int i) { return o + voxel * (float)i; }

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const TsdfArgs a) {
    // per view: the three rows of the view transform that give x, y, z, then fx, fy (16 floats)
    __shared__ float vc[TSDF_MAX_VIEWS * 16];
    const int tid = threadIdx.x + TSDF_BX * (threadIdx.y + TSDF_BY * threadIdx.z);
    for (int e = tid; e < a.n_views * 16; e += 256) {
        const int v = e >> 4, k = e & 15;
        float val = 0.f;
        if (k < 12) val = a.view[v][(k & 3) * 4 + (k >> 2)];      // row r = k/4 of x,y,z: vm[r], vm[4+r], vm[8+r], vm[12+r]
        else if (k == 12) val = a.fx[v];
        else if (k == 13) val = a.fy[v];
        vc[e] = val;
    }
    __syncthreads();
    const MeshGrid& g = a.g;
    const int i = blockIdx.x * TSDF_BX + threadIdx.x;
    const int j = blockIdx.y * TSDF_BY + threadIdx.y;
    const int k = blockIdx.z * TSDF_BZ + threadIdx.z;
    if (i >= g.nx || j >= g.ny || k >= g.nz) return;
    const size_t idx = ((size_t)k * g.ny + j) * g.nx + i;
    if (i == 0 || j == 0 || k == 0 || i == g.nx - 1 || j == g.ny - 1 || k == g.nz - 1) {
        a.sdf[idx] = 1.0f;                         // the outermost layer is outside: the surface always closes
        return;
    }
    const float px = grid_coord(g.ox, g.voxel, i), py = grid_coord(g.oy, g.voxel, j), pz = grid_coord(g.oz, g.voxel, k);
    const size_t plane = (size_t)a.width * a.height;
    float s = 0.f;
    int w = 0;
    bool carved = false;
    for (int v = 0; v < a.n_views; ++v) {
        const float* c = vc + 16 * v;
        const float x = c[0] * px + c[1] * py + c[2] * pz + c[3];
        const float y = c[4] * px + c[5] * py + c[6] * pz + c[7];
        const float z = c[8] * px + c[9] * py + c[10] * pz + c[11];
        if (z <= NEAR_Z) continue;
        const float u = (x / z) * c[12] + a.cx;
        const float vv = (y / z) * c[13] + a.cy;
        const float fu = floorf(u + 0.5f), fv = floorf(vv + 0.5f);
        if (!(fu >= 0.f && fu < (float)a.width && fv >= 0.f && fv < (float)a.height)) continue;
        const size_t pix = (size_t)v * plane + (size_t)(int)fv * a.width + (size_t)(int)fu;
        if (1.0f - a.final_T[pix] < a.alpha_min) { carved = true; break; }   // seen through: outside, whatever follows
        const float d = a.depth[pix] - z;
        if (d < -a.truncation) continue;           // behind the visible surface: no information
        s += fminf(d, a.truncation) / a.truncation;
        w += 1;
    }
    a.sdf[idx] = carved ? 1.0f : (w == 0 ? -1.0f : s / (float)w);
}

// ---- marching tetrahedra ------------------------------------------------------------------------------------------
// Corner code of a cell: bit 0 = +x, bit 1 = +y, bit 2 = +z.  Tetrahedron t walks 0 -> e_a -> e_a+e_b -> 7 for the t-th
// permutation (a,b,c) of (x,y,z) in lexicographic order.  Its 6 edges (u,w), u < w along the walk, are owned by corner
// code(u) and run along code(w) ^ code(u), one of the owner's 7 edge directions.
struct MarchTable {
    int8_t corner[6][4];         // corner code of the tetrahedron's vertices
    int8_t owner[6][6];          // corner code owning edge e
    int8_t slot[6][6];           // its slot among the owner's 7 edges
    int8_t ntri[6][16];          // triangles of the sign pattern (bit q = vertex q inside)
    int8_t tri[6][16][6];        // their vertices as edge ids, outward winding
};

constexpr int march_edge_id(int u, int w) {      // (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    return u == 0 ? w - 1 : (u == 1 ? w + 1 : 5);
}
constexpr int march_slot(int dmask) {            // +x +y +z +xy +xz +yz +xyz
    return dmask == 1 ? 0 : dmask == 2 ? 1 : dmask == 4 ? 2 : dmask == 3 ? 3 : dmask == 5 ? 4 : dmask == 6 ? 5 : 6;
}
constexpr int march_orient(const int (&P)[4][3], int i, int j, int k, int l) {   // sign of det[Pj-Pi, Pk-Pi, Pl-Pi]
    const int a0 = P[j][0] - P[i][0], a1 = P[j][1] - P[i][1], a2 = P[j][2] - P[i][2];
    const int b0 = P[k][0] - P[i][0], b1 = P[k][1] - P[i][1], b2 = P[k][2] - P[i][2];
    const int c0 = P[l][0] - P[i][0], c1 = P[l][1] - P[i][1], c2 = P[l][2] - P[i][2];
    const int d = a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0);
    return d > 0 ? 1 : -1;
}

constexpr MarchTable build_march_table() {
    MarchTable T{};
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int t = 0; t < 6; ++t) {
        const int code[4] = {0, 1 << perms[t][0], (1 << perms[t][0]) | (1 << perms[t][1]), 7};
        int P[4][3] = {};
        for (int q = 0; q < 4; ++q) {
            T.corner[t][q] = (int8_t)code[q];
            for (int ax = 0; ax < 3; ++ax) P[q][ax] = (code[q] >> ax) & 1;
        }
        for (int u = 0; u < 4; ++u)
            for (int w = u + 1; w < 4; ++w) {
                T.owner[t][march_edge_id(u, w)] = (int8_t)code[u];
                T.slot[t][march_edge_id(u, w)] = (int8_t)march_slot(code[w] ^ code[u]);
            }
        for (int c = 0; c < 16; ++c) {
            int in[4] = {}, out[4] = {}, n_in = 0, n_out = 0;
            for (int q = 0; q < 4; ++q) {
                if ((c >> q) & 1) in[n_in++] = q;
                else out[n_out++] = q;
            }
            auto E = [](int p, int q) { return p < q ? march_edge_id(p, q) : march_edge_id(q, p); };
            int8_t* r = T.tri[t][c];
            if (n_in == 1 || n_in == 3) {
                // the lone vertex x and the others j < k < l: the triangle cuts x's corner, facing away from x when x is
                // inside and towards it when x is outside
                const int x = n_in == 1 ? in[0] : out[0];
                const int* o = n_in == 1 ? out : in;
                const bool ccw = (march_orient(P, x, o[0], o[1], o[2]) > 0) == (n_in == 1);
                r[0] = (int8_t)E(x, o[0]);
                r[1] = (int8_t)E(x, ccw ? o[1] : o[2]);
                r[2] = (int8_t)E(x, ccw ? o[2] : o[1]);
                T.ntri[t][c] = 1;
            } else if (n_in == 2) {
                // the quad i1o1, i1o2, i2o2, i2o1 (a cycle); outward when orient(i1, i2, o1, o2) > 0, else reversed
                int q[4] = {E(in[0], out[0]), E(in[0], out[1]), E(in[1], out[1]), E(in[1], out[0])};
                if (march_orient(P, in[0], in[1], out[0], out[1]) < 0) { const int tmp = q[1]; q[1] = q[3]; q[3] = tmp; }
                r[0] = (int8_t)q[0]; r[1] = (int8_t)q[1]; r[2] = (int8_t)q[2];
                r[3] = (int8_t)q[0]; r[4] = (int8_t)q[2]; r[5] = (int8_t)q[3];
                T.ntri[t][c] = 2;
            }
        }
    }
    return T;
}

__constant__ MarchTable kMarch = build_march_table();

// cell corner c of point (i,j,k) as an offset in the [nz,ny,nx] array
__device__ __forceinline__ size_t corner_offset(const MeshGrid& g, int c) {
    return (size_t)(c & 1) + (size_t)((c >> 1) & 1) * g.nx + (size_t)((c >> 2) & 1) * g.nx * g.ny;
}

__device__ __forceinline__ int slot_dmask(int s) { return s < 3 ? 1 << s : (s == 3 ? 3 : (s == 4 ? 5 : (s == 5 ? 6 : 7))); }

// inside-ness of the cell's 8 corners as bits (a corner outside the grid copies corner 0: no crossing towards it)
__device__ __forceinline__ int corner_signs(const MeshGrid& g, const float* __restrict__ sdf, size_t p, bool hx, bool hy,
                                            bool hz) {
    const int in0 = sdf[p] < 0.f;
    int bits = in0;
#pragma unroll
    for (int c = 1; c < 8; ++c) {
        const bool ok = (!(c & 1) || hx) && (!(c & 2) || hy) && (!(c & 4) || hz);
        const int b = ok ? (int)(sdf[p + corner_offset(g, c)] < 0.f) : in0;
        bits |= b << c;
    }
    return bits;
}

// the grid point's crossed-edge mask (bit = slot) and, when it is a cell's origin, the cell's triangle count
__device__ __forceinline__ void march_point(const MeshGrid& g, const float* __restrict__ sdf, size_t p, int& mask, int& ntri) {
    const int i = (int)(p % g.nx), j = (int)((p / g.nx) % g.ny), k = (int)(p / ((size_t)g.nx * g.ny));
    const bool hx = i + 1 < g.nx, hy = j + 1 < g.ny, hz = k + 1 < g.nz;
    const int in = corner_signs(g, sdf, p, hx, hy, hz);
    mask = 0;
#pragma unroll
    for (int s = 0; s < 7; ++s)
        if (((in >> slot_dmask(s)) & 1) != (in & 1)) mask |= 1 << s;
    ntri = 0;
    if (hx && hy && hz) {
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            int c = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) c |= ((in >> kMarch.corner[t][q]) & 1) << q;
            ntri += kMarch.ntri[t][c];
        }
    }
}

// exclusive block scan of two counts (256 threads, 4 waves); returns the block totals through ta / tb
__device__ __forceinline__ void block_scan2(int a, int b, int& ea, int& eb, int& ta, int& tb, int* lds /* [8] */) {
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    int sa = a, sb = b;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int xa = __shfl_up(sa, d, WAVE), xb = __shfl_up(sb, d, WAVE);
        if (lane >= d) { sa += xa; sb += xb; }
    }
    if (lane == WAVE - 1) { lds[wid] = sa; lds[4 + wid] = sb; }
    __syncthreads();
    int pa = 0, pb = 0;
    ta = 0; tb = 0;
#pragma unroll
    for (int w = 0; w < MARCH_THREADS / WAVE; ++w) {
        if (w < wid) { pa += lds[w]; pb += lds[4 + w]; }
        ta += lds[w]; tb += lds[4 + w];
    }
    ea = pa + sa - a;
    eb = pb + sb - b;
    __syncthreads();                               // lds is reused by the next round
}

// per point: crossed-edge mask and triangle count; per tile: the two totals
__global__ __launch_bounds__(MARCH_THREADS) void march_count_kernel(MeshGrid g, const float* __restrict__ sdf, size_t n,
                                                                   uint8_t* __restrict__ mask_out,
                                                                   uint8_t* __restrict__ ntri_out,
                                                                   long long* __restrict__ tile_tot) {
    __shared__ int lds[8];
    const size_t base = (size_t)blockIdx.x * MARCH_TILE;
    int va = 0, fa = 0;
#pragma unroll
    for (int r = 0; r < MARCH_PER_THREAD; ++r) {
        const size_t p = base + (size_t)r * MARCH_THREADS + threadIdx.x;
        if (p < n) {
            int m, t;
            march_point(g, sdf, p, m, t);
            mask_out[p] = (uint8_t)m;
            ntri_out[p] = (uint8_t)t;
            va += __popc(m);
            fa += t;
        }
    }
    int ea, eb, ta, tb;
    block_scan2(va, fa, ea, eb, ta, tb, lds);
    if (threadIdx.x == 0) { tile_tot[2 * blockIdx.x] = ta; tile_tot[2 * blockIdx.x + 1] = tb; }
}

// one workgroup: exclusive scan of the tile totals (each thread a contiguous run of tiles); counts = the two totals
__global__ __launch_bounds__(MARCH_SCAN_THREADS) void march_scan_kernel(const long long* __restrict__ tile_tot, int n_tiles,
                                                                       long long* __restrict__ tile_off,
                                                                       long long* __restrict__ counts) {
    __shared__ long long sa[MARCH_SCAN_THREADS], sb[MARCH_SCAN_THREADS];
    const int per = (n_tiles + MARCH_SCAN_THREADS - 1) / MARCH_SCAN_THREADS;
    const int t0 = threadIdx.x * per, t1 = min(n_tiles, t0 + per);
    long long a = 0, b = 0;
    for (int t = t0; t < t1; ++t) { a += tile_tot[2 * t]; b += tile_tot[2 * t + 1]; }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int d = 1; d < MARCH_SCAN_THREADS; d <<= 1) {       // inclusive Hillis-Steele scan of the run totals
        long long xa = 0, xb = 0;
        if ((int)threadIdx.x >= d) { xa = sa[threadIdx.x - d]; xb = sb[threadIdx.x - d]; }
        __syncthreads();
        sa[threadIdx.x] += xa;
        sb[threadIdx.x] += xb;
        __syncthreads();
    }
    long long oa = sa[threadIdx.x] - a, ob = sb[threadIdx.x] - b;
    for (int t = t0; t < t1; ++t) {
        tile_off[2 * t] = oa;
        tile_off[2 * t + 1] = ob;
        oa += tile_tot[2 * t];
        ob += tile_tot[2 * t + 1];
    }
    if (threadIdx.x == MARCH_SCAN_THREADS - 1) { counts[0] = sa[threadIdx.x]; counts[1] = sb[threadIdx.x]; }
}

// the index of every point's first vertex (the tile's base + the scan inside the tile); the last step of march_count
__global__ __launch_bounds__(MARCH_THREADS) void march_vbase_kernel(size_t n, const uint8_t* __restrict__ mask_in,
                                                                   const long long* __restrict__ tile_off,
                                                                   int32_t* __restrict__ vbase) {
    __shared__ int lds[8];
    const size_t base = (size_t)blockIdx.x * MARCH_TILE;
    long long carry = tile_off[2 * blockIdx.x];
    for (int r = 0; r < MARCH_PER_THREAD; ++r) {
        const size_t p = base + (size_t)r * MARCH_THREADS + threadIdx.x;
        const int m = p < n ? mask_in[p] : 0;
        int e, unused_e, tot, unused_t;
        block_scan2(__popc(m), 0, e, unused_e, tot, unused_t, lds);
        if (p < n) vbase[p] = (int32_t)(carry + e);
        carry += tot;
    }
}

// vertices in (point, edge) order, at pa + t (pb - pa), t = fa / (fa - fb), a = the owner
__global__ __launch_bounds__(MARCH_THREADS) void march_vertices_kernel(MeshGrid g, const float* __restrict__ sdf, size_t n,
                                                                      const uint8_t* __restrict__ mask_in,
                                                                      const int32_t* __restrict__ vbase,
                                                                      float* __restrict__ vertices) {
    const size_t p = (size_t)blockIdx.x * MARCH_THREADS + threadIdx.x;
    if (p >= n) return;
    const int m = mask_in[p];
    if (!m) return;
    size_t vid = (size_t)(uint32_t)vbase[p];
    const int i = (int)(p % g.nx), j = (int)((p / g.nx) % g.ny), k = (int)(p / ((size_t)g.nx * g.ny));
    const float ax = grid_coord(g.ox, g.voxel, i), ay = grid_coord(g.oy, g.voxel, j), az = grid_coord(g.oz, g.voxel, k);
    const float fa = sdf[p];
    for (int s = 0; s < 7; ++s) {
        if (!((m >> s) & 1)) continue;
        const int dm = slot_dmask(s);
        const float bx = grid_coord(g.ox, g.voxel, i + (dm & 1)), by = grid_coord(g.oy, g.voxel, j + ((dm >> 1) & 1)),
                    bz = grid_coord(g.oz, g.voxel, k + ((dm >> 2) & 1));
        const float fb = sdf[p + corner_offset(g, dm)];
        const float t = fa / (fa - fb);
        vertices[3 * vid + 0] = ax + t * (bx - ax);
        vertices[3 * vid + 1] = ay + t * (by - ay);
        vertices[3 * vid + 2] = az + t * (bz - az);
        ++vid;
    }
}

// faces in (cell, tetrahedron, triangle) order
__global__ __launch_bounds__(MARCH_THREADS) void march_faces_kernel(MeshGrid g, const float* __restrict__ sdf, size_t n,
                                                                   const uint8_t* __restrict__ mask_in,
                                                                   const uint8_t* __restrict__ ntri_in,
                                                                   const long long* __restrict__ tile_off,
                                                                   const int32_t* __restrict__ vbase,
                                                                   int32_t* __restrict__ faces) {
    __shared__ int lds[8];
    const size_t base = (size_t)blockIdx.x * MARCH_TILE;
    long long carry = tile_off[2 * blockIdx.x + 1];
    for (int r = 0; r < MARCH_PER_THREAD; ++r) {
        const size_t p = base + (size_t)r * MARCH_THREADS + threadIdx.x;
        const int nt = p < n ? ntri_in[p] : 0;
        int e, unused_e, tot, unused_t;
        block_scan2(nt, 0, e, unused_e, tot, unused_t, lds);
        if (nt) {
            long long fid = carry + e;
            const int in = corner_signs(g, sdf, p, true, true, true);     // a cell with triangles has all 8 corners
            for (int t = 0; t < 6; ++t) {
                int cs = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) cs |= ((in >> kMarch.corner[t][q]) & 1) << q;
                for (int tr = 0; tr < kMarch.ntri[t][cs]; ++tr) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const int ed = kMarch.tri[t][cs][3 * tr + q];
                        const size_t owner = p + corner_offset(g, kMarch.owner[t][ed]);
                        const int slot = kMarch.slot[t][ed];
                        faces[3 * fid + q] = vbase[owner] + __popc(mask_in[owner] & ((1 << slot) - 1));
                    }
                    ++fid;
                }
            }
        }
        carry += tot;
    }
}

}  // namespace pgr
