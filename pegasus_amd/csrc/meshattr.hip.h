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

}  // namespace pgr
