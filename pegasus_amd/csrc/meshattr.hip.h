// meshattr.hip.h -- per-vertex attributes of an extracted mesh: normals from the faces, colours from the rendered views.
//
// Vertex normals (the rule of mesh_render.vertex_normals / open3d's compute_vertex_normals: the unit normals of the
// faces, summed per vertex, normalised).  The sum is a scatter; to make it repeatable to the bit without an inverted
// index every unit face normal is quantised to integers of 2^-30 and added with 64-bit INTEGER atomics, whose result
// does not depend on the order of arrival.  Per face, in float32 with every operation rounded on its own:
//   e1 = b - a, e2 = c - a, m = e1 x e2, len = sqrtf((m.x m.x + m.y m.y) + m.z m.z); nothing when !(len > 0) or len = inf
//   q = (int64) rintf((m / len) * 2^30), added to the three sums of each of the face's three vertices
// then per vertex, in float64: s = (double) sum, l = sqrt((s.x s.x + s.y s.y) + s.z s.z), normal = (float)(s / l), or 0
// where !(l > 0).  A face with an index outside [0, V) is skipped whole.
//
// Vertex colours: one lane per vertex, the views' constants in LDS as in tsdf_integrate_kernel (mesh.hip.h), the views
// walked in order in float32 with no fused multiply-adds.  Per vertex p (normal n) and view:
//   (x,y,z) = viewmatrix . p as the TSDF kernel computes it; skipped when z <= NEAR_Z
//   pixel = floor((x/z) fx + (W-1)/2 + 0.5), likewise y; skipped outside the image (NaN is outside)
//   alpha = 1 - final_T; skipped when alpha < alpha_min; skipped unless |depth - z| <= depth_tol (a NaN depth fails)
//   with normals: e = campos - p, cs = (n . e) / |e|; skipped unless cs > cos_min; w = cs cs.  Without: w = 1
//   acc += w * (color / alpha) per channel, wsum += w, seen += 1
// colour = clamp(acc / wsum, 0, 1) where seen > 0, else `fill`.  The pixel is the nearest one: the pixel the TSDF kernel
// fused the surface from.
#pragma once
#include "mesh.hip.h"
#include "pgr_common.h"

namespace pgr {

constexpr int MESHATTR_THREADS = 256;
constexpr float MESHATTR_SCALE = 1073741824.0f;            // 2^30: scaling by it is exact
constexpr int VCOLOR_STRIDE = 20;                          // floats per view in LDS: 12 of the transform, fx, fy, campos[3]

__device__ __forceinline__ void attr_add(long long* p, long long v) {
    __hip_atomic_fetch_add((PGR_GLOBAL long long*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one lane per face: its quantised unit normal into the sums of its three vertices
__global__ __launch_bounds__(MESHATTR_THREADS) void vertex_normals_accumulate_kernel(int n_vertices,
                                                                                    const float* __restrict__ vertices,
                                                                                    int n_faces,
                                                                                    const int32_t* __restrict__ faces,
                                                                                    long long* __restrict__ sums) {
    const size_t f = (size_t)blockIdx.x * MESHATTR_THREADS + threadIdx.x;
    if (f >= (size_t)n_faces) return;
    const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if ((uint32_t)ia >= (uint32_t)n_vertices || (uint32_t)ib >= (uint32_t)n_vertices || (uint32_t)ic >= (uint32_t)n_vertices)
        return;
    const float* a = vertices + 3 * (size_t)ia;
    const float* b = vertices + 3 * (size_t)ib;
    const float* c = vertices + 3 * (size_t)ic;
    const float ax = a[0], ay = a[1], az = a[2];
    const float e1x = b[0] - ax, e1y = b[1] - ay, e1z = b[2] - az;
    const float e2x = c[0] - ax, e2y = c[1] - ay, e2z = c[2] - az;
    const float mx = e1y * e2z - e1z * e2y;
    const float my = e1z * e2x - e1x * e2z;
    const float mz = e1x * e2y - e1y * e2x;
    const float len = sqrtf((mx * mx + my * my) + mz * mz);
    if (!(len > 0.f) || !(len < INFINITY)) return;
    const long long qx = (long long)rintf((mx / len) * MESHATTR_SCALE);
    const long long qy = (long long)rintf((my / len) * MESHATTR_SCALE);
    const long long qz = (long long)rintf((mz / len) * MESHATTR_SCALE);
    const int32_t idx[3] = {ia, ib, ic};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        long long* s = sums + 3 * (size_t)idx[k];
        attr_add(s + 0, qx);
        attr_add(s + 1, qy);
        attr_add(s + 2, qz);
    }
}

// one lane per vertex: the integer sum normalised in float64
__global__ __launch_bounds__(MESHATTR_THREADS) void vertex_normals_finalize_kernel(int n_vertices,
                                                                                  const long long* __restrict__ sums,
                                                                                  float* __restrict__ normals) {
    const size_t v = (size_t)blockIdx.x * MESHATTR_THREADS + threadIdx.x;
    if (v >= (size_t)n_vertices) return;
    const double sx = (double)sums[3 * v], sy = (double)sums[3 * v + 1], sz = (double)sums[3 * v + 2];
    const double l = sqrt((sx * sx + sy * sy) + sz * sz);
    const bool ok = l > 0.0;
    normals[3 * v + 0] = ok ? (float)(sx / l) : 0.f;
    normals[3 * v + 1] = ok ? (float)(sy / l) : 0.f;
    normals[3 * v + 2] = ok ? (float)(sz / l) : 0.f;
}

struct VertexColorArgs {
    int n_vertices, n_views, width, height;
    float cx, cy;                                  // (W-1)/2, (H-1)/2
    float depth_tol, alpha_min, cos_min;
    float fill[3];
    const float* vertices;                         // [V,3]
    const float* normals;                          // [V,3] or NULL
    const float* color;                            // [n_views,3,H,W]
    const float* depth;                            // [n_views,H,W]
    const float* final_T;                          // [n_views,H,W]
    float* colors;                                 // [V,3]
    int32_t* seen;                                 // [V] or NULL
    const float* view[TSDF_MAX_VIEWS];             // world_view_transform, transposed storage
    const float* campos[TSDF_MAX_VIEWS];
    float fx[TSDF_MAX_VIEWS], fy[TSDF_MAX_VIEWS];  // W / (2 tanfovx), H / (2 tanfovy)
};

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

__global__ __launch_bounds__(MESHATTR_THREADS) void vertex_colors_kernel(const VertexColorArgs a) {
    __shared__ float vc[TSDF_MAX_VIEWS * VCOLOR_STRIDE];
    for (int e = threadIdx.x; e < a.n_views * VCOLOR_STRIDE; e += MESHATTR_THREADS) {
        const int v = e / VCOLOR_STRIDE, k = e - v * VCOLOR_STRIDE;
        float val = 0.f;
        if (k < 12) val = a.view[v][(k & 3) * 4 + (k >> 2)];      // row r = k/4 of x,y,z: vm[r], vm[4+r], vm[8+r], vm[12+r]
        else if (k == 12) val = a.fx[v];
        else if (k == 13) val = a.fy[v];
        else if (k < 17) val = a.campos[v][k - 14];
        vc[e] = val;
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * MESHATTR_THREADS + threadIdx.x;
    if (i >= (size_t)a.n_vertices) return;
    const float px = a.vertices[3 * i], py = a.vertices[3 * i + 1], pz = a.vertices[3 * i + 2];
    const bool angled = a.normals != nullptr;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (angled) { nx = a.normals[3 * i]; ny = a.normals[3 * i + 1]; nz = a.normals[3 * i + 2]; }
    const size_t plane = (size_t)a.width * a.height;
    float r = 0.f, g = 0.f, b = 0.f, wsum = 0.f;
    int seen = 0;
    for (int v = 0; v < a.n_views; ++v) {
        const float* c = vc + VCOLOR_STRIDE * v;
        const float x = c[0] * px + c[1] * py + c[2] * pz + c[3];
        const float y = c[4] * px + c[5] * py + c[6] * pz + c[7];
        const float z = c[8] * px + c[9] * py + c[10] * pz + c[11];
        if (z <= NEAR_Z) continue;
        const float u = (x / z) * c[12] + a.cx;
        const float vv = (y / z) * c[13] + a.cy;
        const float fu = floorf(u + 0.5f), fv = floorf(vv + 0.5f);
        if (!(fu >= 0.f && fu < (float)a.width && fv >= 0.f && fv < (float)a.height)) continue;
        const size_t at = (size_t)(int)fv * a.width + (size_t)(int)fu;
        const size_t pix = (size_t)v * plane + at;
        const float alpha = 1.0f - a.final_T[pix];
        if (alpha < a.alpha_min) continue;                       // seen through
        if (!(fabsf(a.depth[pix] - z) <= a.depth_tol)) continue; // the far side, occluded, or a NaN depth
        float w = 1.0f;
        if (angled) {
            const float ex = c[14] - px, ey = c[15] - py, ez = c[16] - pz;
            const float el = sqrtf((ex * ex + ey * ey) + ez * ez);
            const float cs = ((nx * ex + ny * ey) + nz * ez) / el;
            if (!(cs > a.cos_min)) continue;
            w = cs * cs;
        }
        const float* col = a.color + 3 * (size_t)v * plane + at;
        r += w * (col[0] / alpha);                               // un-premultiplied: the render is sum T alpha c over zero
        g += w * (col[plane] / alpha);
        b += w * (col[2 * plane] / alpha);
        wsum += w;
        seen += 1;
    }
    a.colors[3 * i + 0] = seen > 0 ? clamp01(r / wsum) : a.fill[0];
    a.colors[3 * i + 1] = seen > 0 ? clamp01(g / wsum) : a.fill[1];
    a.colors[3 * i + 2] = seen > 0 ? clamp01(b / wsum) : a.fill[2];
    if (a.seen) a.seen[i] = seen;
}

// ---- a per-face texture atlas: pgr_mesh_atlas_points, pgr_mesh_atlas_pack ---------------------------------------------------
// Layout (pegasus_amd.mesh.texture_atlas_layout computes it on the host; the entries check the size they are handed against
// it).  Cell side s >= 4 texels, leg L = s - 3.  cells = ceil(F / 2), cols = the smallest integer with cols^2 >= cells,
// rows = ceil(cells / cols); the atlas is cols s wide and rows s high, each at most 8192.  Face f lies in cell c = f >> 1, half
// f & 1; the cell's origin is ((c % cols) s, (c / cols) s) from the image's top-left.  In cell-local texel-centre coordinates
// (x right, y down, the centre of texel (i, j) at (i + 0.5, j + 0.5)) half 0 has corner a at (0.5, 0.5), b at (0.5 + L, 0.5),
// c at (0.5, 0.5 + L); half 1 is its mirror image through the cell's centre: a at (s - 0.5, s - 0.5), b at (s - 0.5 - L,
// s - 0.5), c at (s - 0.5, s - 0.5 - L).  Texel (i, j) belongs to half 0 when i + j <= s - 1, else to half 1.  In exact
// arithmetic a sample inside half 0's triangle reads, with non-zero weight, only texels with i + j <= s - 2 and one inside half
// 1's only texels with i + j >= s, under the nearest and the bilinear filter: the antidiagonal i + j = s - 1 between them takes
// what float32 rounding of u and of u W adds (tests/test_mesh_texture_host.py checks both).
//
// pgr_mesh_atlas_points: one lane per atlas texel.  Its face f = 2 c + half; face_of_texel = -1 (and point = normal = 0) when
// f >= F, when one of the face's indices is outside [0, V) (never dereferenced), or when the face normal's length is zero or
// not finite.  Else, float32, every operation rounded on its own:
//   (di, dj) = (i, j) in half 0, (s - 1 - i, s - 1 - j) in half 1;   beta = (float)di / (float)L,  gamma = (float)dj / (float)L
//   p = (A + beta (B - A)) + gamma (C - A) per component (texels whose centre lies outside the triangle extrapolate)
//   normal = m / sqrtf((m.x m.x + m.y m.y) + m.z m.z),  m = (B - A) x (C - A) as pgr_mesh_shade's flat rule, model frame, no flip
//
// pgr_mesh_atlas_pack: one wave per cell, the texels of the cell in strides of 64.  A texel counts as its face's when
// face_of_texel names that face.  Per owned texel with seen > 0:  q = (uint8)rintf(255 c) per channel (a NaN gives 0; c is
// clamped by pgr_mesh_vertex_colors).  Per face, in integers:  cnt = its seen texels,  sum = the per-channel sum of their q
// (wave reductions over 64-bit integers: no float atomics, equal bytes from run to run).  Its unseen texels get
// (2 sum + cnt) / (2 cnt) (the mean rounded half up); with cnt == 0 row f of face_fill (uint8 [F,3]), or `fill` without
// face_fill.  Texels of no face get `fill`.  face_seen[f] = cnt.
constexpr int ATLAS_MAX_SIDE = 8192;
constexpr int ATLAS_PACK_THREADS = 256;                    // four waves: four cells

struct AtlasArgs {
    int32_t n_vertices, n_faces, cell, cols, width, height;
    const float* vertices;
    const int32_t* faces;
};

__global__ __launch_bounds__(MESHATTR_THREADS) void atlas_points_kernel(const AtlasArgs a, float* __restrict__ points,
                                                                        float* __restrict__ normals,
                                                                        int32_t* __restrict__ face_of_texel) {
    const size_t t = (size_t)blockIdx.x * MESHATTR_THREADS + threadIdx.x;
    if (t >= (size_t)a.width * (size_t)a.height) return;
    const int X = (int)(t % (size_t)a.width), Y = (int)(t / (size_t)a.width);
    const int s = a.cell, L = s - 3;
    const int cx = X / s, cy = Y / s;
    const int i = X - cx * s, j = Y - cy * s;
    const int half = i + j <= s - 1 ? 0 : 1;
    const long long f = 2ll * ((long long)cy * a.cols + cx) + half;
    float p[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
    int32_t owner = -1;
    if (f < (long long)a.n_faces) {
        const int32_t ia = a.faces[3 * f], ib = a.faces[3 * f + 1], ic = a.faces[3 * f + 2];
        if ((uint32_t)ia < (uint32_t)a.n_vertices && (uint32_t)ib < (uint32_t)a.n_vertices && (uint32_t)ic < (uint32_t)a.n_vertices) {
            const float* A = a.vertices + 3 * (size_t)ia;
            const float* B = a.vertices + 3 * (size_t)ib;
            const float* C = a.vertices + 3 * (size_t)ic;
            float e1[3], e2[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) { e1[d] = B[d] - A[d]; e2[d] = C[d] - A[d]; }
            const float mx = e1[1] * e2[2] - e1[2] * e2[1];
            const float my = e1[2] * e2[0] - e1[0] * e2[2];
            const float mz = e1[0] * e2[1] - e1[1] * e2[0];
            const float len = sqrtf((mx * mx + my * my) + mz * mz);
            if (len > 0.f && len < INFINITY) {
                owner = (int32_t)f;
                const int di = half ? s - 1 - i : i, dj = half ? s - 1 - j : j;
                const float beta = (float)di / (float)L, gamma = (float)dj / (float)L;
#pragma unroll
                for (int d = 0; d < 3; ++d) p[d] = (A[d] + beta * e1[d]) + gamma * e2[d];
                n[0] = mx / len; n[1] = my / len; n[2] = mz / len;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) { points[3 * t + d] = p[d]; normals[3 * t + d] = n[d]; }
    face_of_texel[t] = owner;
}

__device__ __forceinline__ unsigned long long atlas_wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

__device__ __forceinline__ uint32_t atlas_quantise(float c) {
    const float v = 255.0f * c;
    return v == v ? (uint32_t)min(max((int)rintf(v), 0), 255) : 0u;
}

struct AtlasPackArgs {
    int32_t n_faces, cell, cols, width, height;
    long long n_cells;
    uint8_t fill[3];
    const int32_t* face_of_texel;
    const float* colors;                           // [height*width,3]
    const int32_t* seen;                           // [height*width]
    const uint8_t* face_fill;                      // [F,3] or NULL
    uint8_t* texture;                              // [height,width,3]
    int32_t* face_seen;                            // [F] or NULL
};

__global__ __launch_bounds__(ATLAS_PACK_THREADS) void atlas_pack_kernel(const AtlasPackArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long c = (long long)blockIdx.x * (ATLAS_PACK_THREADS / WAVE) + threadIdx.x / WAVE;     // wave-uniform
    if (c >= a.n_cells) return;
    const int s = a.cell, n = s * s;
    const size_t x0 = (size_t)(c % a.cols) * s, y0 = (size_t)(c / a.cols) * s;
    unsigned long long cnt[2] = {0, 0}, sum[2][3] = {{0, 0, 0}, {0, 0, 0}};
    for (int e = lane; e < n; e += WAVE) {
        const int j = e / s, i = e - j * s;
        const int half = i + j <= s - 1 ? 0 : 1;
        const size_t t = (y0 + j) * (size_t)a.width + x0 + i;
        if ((long long)a.face_of_texel[t] == 2 * c + half && a.seen[t] > 0) {
            cnt[half] += 1;
#pragma unroll
            for (int d = 0; d < 3; ++d) sum[half][d] += atlas_quantise(a.colors[3 * t + d]);
        }
    }
    uint8_t mean[2][3];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        cnt[h] = atlas_wave_sum(cnt[h]);
        const long long f = 2 * c + h;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            sum[h][d] = atlas_wave_sum(sum[h][d]);
            if (cnt[h] > 0) mean[h][d] = (uint8_t)((2 * sum[h][d] + cnt[h]) / (2 * cnt[h]));
            else mean[h][d] = (a.face_fill && f < a.n_faces) ? a.face_fill[3 * f + d] : a.fill[d];
        }
        if (a.face_seen && lane == 0 && f < a.n_faces) a.face_seen[f] = (int32_t)cnt[h];
    }
    for (int e = lane; e < n; e += WAVE) {
        const int j = e / s, i = e - j * s;
        const int half = i + j <= s - 1 ? 0 : 1;
        const size_t t = (y0 + j) * (size_t)a.width + x0 + i;
        const bool owned = (long long)a.face_of_texel[t] == 2 * c + half;
        const bool seen = owned && a.seen[t] > 0;
#pragma unroll
        for (int d = 0; d < 3; ++d)
            a.texture[3 * t + d] = seen ? (uint8_t)atlas_quantise(a.colors[3 * t + d]) : owned ? mean[half][d] : a.fill[d];
    }
}

}  // namespace pgr
