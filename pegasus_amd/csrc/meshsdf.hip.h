// meshsdf.hip.h -- collision geometry: the signed distance field of a triangle mesh (pgr_mesh_sdf), its trilinear samples
// (pgr_sdf_sample) and distance / sweep queries between posed bodies (pgr_sdf_sweep).  pegasus_amd/collision.py is the caller;
// tests/collision_reference.py restates every rule in float64; DESIGN.md section 22 holds the derivations.  All arithmetic is
// float32 without contraction, every operation rounded on its own, except where float64 is named.
//
// pgr_mesh_sdf: the rules
//
//   Point.      Grid point (i,j,k) is  origin + voxel * (float)(i,j,k)  per axis: one product, one sum.
//   Magnitude.  Per face (a,b,c), with A = a - p, the exact distance from p to the triangle is the smallest of
//                 - its three segments (a,b), (b,c), (c,a): for a segment (u,v), U = u - p, e = v - u, ee = e.e,
//                   t = ee > 0 ? clamp(-(U.e) / ee, 0, 1) : 0,  q = U + t e,  d2 = q.q        (a zero-length segment is its point)
//                 - its interior: e1 = b - a, e2 = c - a, g11 = e1.e1, g12 = e1.e2, g22 = e2.e2, h1 = -(A.e1), h2 = -(A.e2),
//                   det = g11 g22 - g12 g12; where det > 0: v = (g22 h1 - g12 h2) / det, w = (g11 h2 - g12 h1) / det, and where
//                   v >= 0, w >= 0, v + w <= 1:  q = (A + v e1) + w e2,  d2 = q.q
//               Every candidate is the squared distance to a point OF the triangle, so a badly conditioned interior solve (a
//               sliver, a zero-area face whose det rounds above 0) can only fail to improve on the segments, never undercut the
//               true distance by more than the rounding of q.  Dots are (x x + y y) + z z.  The minimum over all faces is taken
//               per lane in face order with fminf; one sqrtf at the end.  F = 0 gives +inf.
//   Sign.       Generalized winding number: per face the signed solid angle in Van Oosterom-Strackee form,
//                   num = A . (B x C),   den = ((la lb lc + (A.B) lc) + (A.C) lb) + (B.C) la,   la = sqrtf(A.A) ..
//                   omega = 2 atan2f(num, den)
//               added in face order into a float64 sum per lane; winding = sum / (4 pi) in float64.  The distance is negated where
//               winding >= 0.5.  Outward-wound closed meshes give 1 inside and 0 outside; an open mesh gives the fraction of the
//               sphere around p that the surface covers.  atan2f(0, 0) is 0: a point on a vertex adds nothing for that face.
//   Faces.      A face with an index outside [0, n_vertices) is never dereferenced and adds nothing to either.
//   Work.       One lane per grid point, 256 per workgroup.  Faces stream through LDS in tiles of SDF_TILE = 256, one face
//               loaded per lane, three float4 each (12 KiB); the inner loop reads them as broadcasts (ds_read_b128, every lane
//               the same address: no bank conflict).  No atomics; the order of every sum and minimum is fixed.  Cost: points x
//               faces, brute force by design: it is meant for collision meshes of a few 10^4 faces.
//
// pgr_sdf_sample: the rules (sdf_eval below)
//
//   Cell.       g = (p - origin) / voxel per axis, gc = fminf(fmaxf(g, 0), n - 1) (a NaN coordinate clamps to 0),
//               i = min((int)gc, n - 2), f = gc - (float)i in [0, 1].
//   Value.      lerp(a, b, t) = a + t (b - a); four lerps along x, two along y, one along z.
//   Gradient.   The analytic derivative of that trilinear cell at (f), divided by voxel: d/dx lerps the four x-differences along
//               y then z, and so on.  Outside the grid it is the derivative at the clamped point.
//   Outside.    o = (g - gc) * voxel per axis, rr = (o.x o.x + o.y o.y) + o.z o.z, m = fmaxf(phi, 0).  Where rr > 0 the value is
//               sqrtf(rr + m m): the distance r to the grid's box and the clamped field, added in quadrature.  This is a lower
//               bound of the distance to the surface as long as the grid encloses the mesh: a surface point s lies in the box
//               and at least m from the clamped point c, and p - c points out of the box at c, so (p - c).(s - c) <= 0 and
//               |p - s|^2 >= r^2 + m^2.  (The plain sum r + m is an UPPER bound, by the triangle inequality: stepping by it is
//               not safe.)
//
// pgr_sdf_sweep: the rules
//
//   Transform.  Shell point p of mover a in the world: x = ((Ra[0] p.x + Ra[1] p.y) + Ra[2] p.z) + ta[0] .. (R row-major).
//               After a travel s along dir, in the frame of target b:
//                   y = R_b^T ((R_a p + t_a) + s dir - t_b):   z = (x + s dir) - t_b per axis,
//                   y.x = (Rb[0] z.x + Rb[3] z.y) + Rb[6] z.z ..
//   Field.      phi(s) = sdf_eval of b's field at y; for the plane (n, d): phi0 = ((n.x x.x + n.y x.y) + n.z x.z) - d.
//   Travel.     s = 0, phi = phi0; while (steps < max_steps and phi > tol and s < max_travel): s = fminf(s + phi, max_travel),
//               phi = phi(s).  A point that runs out of steps reports the s it reached: every step was at most the free distance.
//               Plane: c = -(n . dir); s = phi0 <= tol ? 0 : (c > 0 ? fminf(phi0 / c, max_travel) : max_travel).
//   Reduce.     Per job two 64-bit words, each  (order-preserving bits of the float) << 32 | point index  (the packing of
//               pgr_mesh_visibility, extended to negative floats: bits ^ 0x80000000 for a positive float, ~bits for a negative
//               one).  word 0: min phi0, word 1: min s.  Wave minimum by xor butterfly, then ONE 64-bit integer atomic min per
//               wave and word at agent scope; the init kernel of the same call sets all bits.  Integer minima do not depend on
//               arrival order; equal floats resolve to the lowest point index.  A job without shell points keeps all bits set.
#pragma once
#include "job_table.hip.h"       // pose_job_of_block
#include "mesh.hip.h"
#include "pgr_common.h"

namespace pgr {

constexpr int SDF_THREADS = 256;
constexpr int SDF_TILE = PGR_SDF_FACE_TILE;
constexpr int SWEEP_THREADS = 256;
constexpr int SWEEP_JOBS_PER_LAUNCH = 16;            // 192 B each: the table stays under the 4 KiB of kernel arguments
static_assert(SDF_TILE == SDF_THREADS, "one face per lane and tile");

struct SweepJobDev {
    const float* shell;                              // mover's shell points, body frame
    const float* sdf;                                // target's field; unused for the plane
    int32_t n_shell;
    int32_t is_plane;
    MeshGrid g;                                      // target's grid
    float Ra[9], ta[3], Rb[9], tb[3], dir[3], plane[4];
    uint32_t block0;                                 // first workgroup of the job in the launch
};

struct SweepJobTable {
    int32_t count, first;
    float tol, max_travel;
    int32_t max_steps, pad;
    SweepJobDev job[SWEEP_JOBS_PER_LAUNCH];
};
static_assert(sizeof(SweepJobTable) <= 3840, "SweepJobTable must fit the kernel argument segment");

__device__ __forceinline__ float sdf_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// squared distance from the origin to the segment U .. U + e
__device__ __forceinline__ float sdf_segment_d2(float ux, float uy, float uz, float ex, float ey, float ez) {
    const float ee = sdf_dot(ex, ey, ez, ex, ey, ez);
    float t = 0.f;
    if (ee > 0.f) t = fminf(fmaxf(-sdf_dot(ux, uy, uz, ex, ey, ez) / ee, 0.f), 1.f);
    const float qx = ux + t * ex, qy = uy + t * ey, qz = uz + t * ez;
    return sdf_dot(qx, qy, qz, qx, qy, qz);
}

__global__ __launch_bounds__(SDF_THREADS) void mesh_sdf_kernel(const MeshGrid g, const float* __restrict__ vertices,
                                                              int32_t n_vertices, const int32_t* __restrict__ faces,
                                                              int32_t n_faces, float* __restrict__ sdf,
                                                              float* __restrict__ winding) {
    __shared__ float4 s_a[SDF_TILE], s_b[SDF_TILE], s_c[SDF_TILE];       // .w of s_a: 1 for a face that counts
    const int tid = threadIdx.x;
    const long long n_points = (long long)g.nx * g.ny * g.nz;
    const long long idx = (long long)blockIdx.x * SDF_THREADS + tid;
    const bool has_point = idx < n_points;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (has_point) {
        const int i = (int)(idx % g.nx), j = (int)((idx / g.nx) % g.ny), k = (int)(idx / ((long long)g.nx * g.ny));
        px = g.ox + g.voxel * (float)i;
        py = g.oy + g.voxel * (float)j;
        pz = g.oz + g.voxel * (float)k;
    }
    float best = INFINITY;
    double omega = 0.0;
    for (int t0 = 0; t0 < n_faces; t0 += SDF_TILE) {
        const int n = min(SDF_TILE, n_faces - t0);                       // faces of this tile: nothing past n_faces is read
        if (tid < n) {
            const int32_t* f = faces + 3 * ((size_t)t0 + (size_t)tid);
            const int32_t ia = gload(f), ib = gload(f + 1), ic = gload(f + 2);
            const bool ok = ia >= 0 && ia < n_vertices && ib >= 0 && ib < n_vertices && ic >= 0 && ic < n_vertices;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
            if (ok) {
                const float *pa = vertices + 3 * (size_t)ia, *pb = vertices + 3 * (size_t)ib, *pc = vertices + 3 * (size_t)ic;
                a = make_float4(gload(pa), gload(pa + 1), gload(pa + 2), 1.f);
                b = make_float4(gload(pb), gload(pb + 1), gload(pb + 2), 0.f);
                c = make_float4(gload(pc), gload(pc + 1), gload(pc + 2), 0.f);
            }
            s_a[tid] = a;
            s_b[tid] = b;
            s_c[tid] = c;
        }
        __syncthreads();
        for (int f = 0; f < n; ++f) {
            const float4 a = s_a[f], b = s_b[f], c = s_c[f];
            if (a.w == 0.f) continue;                                    // the same in every lane: a broadcast value
            const float Ax = a.x - px, Ay = a.y - py, Az = a.z - pz;
            const float Bx = b.x - px, By = b.y - py, Bz = b.z - pz;
            const float Cx = c.x - px, Cy = c.y - py, Cz = c.z - pz;
            const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
            const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
            const float e3x = c.x - b.x, e3y = c.y - b.y, e3z = c.z - b.z;
            float d2 = sdf_segment_d2(Ax, Ay, Az, e1x, e1y, e1z);
            d2 = fminf(d2, sdf_segment_d2(Bx, By, Bz, e3x, e3y, e3z));
            d2 = fminf(d2, sdf_segment_d2(Cx, Cy, Cz, -e2x, -e2y, -e2z));
            const float g11 = sdf_dot(e1x, e1y, e1z, e1x, e1y, e1z), g12 = sdf_dot(e1x, e1y, e1z, e2x, e2y, e2z);
            const float g22 = sdf_dot(e2x, e2y, e2z, e2x, e2y, e2z);
            const float h1 = -sdf_dot(Ax, Ay, Az, e1x, e1y, e1z), h2 = -sdf_dot(Ax, Ay, Az, e2x, e2y, e2z);
            const float det = g11 * g22 - g12 * g12;
            if (det > 0.f) {
                const float v = (g22 * h1 - g12 * h2) / det, w = (g11 * h2 - g12 * h1) / det;
                if (v >= 0.f && w >= 0.f && v + w <= 1.f) {
                    const float qx = (Ax + v * e1x) + w * e2x, qy = (Ay + v * e1y) + w * e2y, qz = (Az + v * e1z) + w * e2z;
                    d2 = fminf(d2, sdf_dot(qx, qy, qz, qx, qy, qz));
                }
            }
            best = fminf(best, d2);
            const float la = sqrtf(sdf_dot(Ax, Ay, Az, Ax, Ay, Az)), lb = sqrtf(sdf_dot(Bx, By, Bz, Bx, By, Bz));
            const float lc = sqrtf(sdf_dot(Cx, Cy, Cz, Cx, Cy, Cz));
            const float cx = By * Cz - Bz * Cy, cy = Bz * Cx - Bx * Cz, cz = Bx * Cy - By * Cx;
            const float num = sdf_dot(Ax, Ay, Az, cx, cy, cz);
            const float den = (((la * lb) * lc + sdf_dot(Ax, Ay, Az, Bx, By, Bz) * lc) + sdf_dot(Ax, Ay, Az, Cx, Cy, Cz) * lb) +
                              sdf_dot(Bx, By, Bz, Cx, Cy, Cz) * la;
            omega += (double)(2.f * atan2f(num, den));
        }
        __syncthreads();
    }
    if (!has_point) return;
    const double wn = omega / (4.0 * 3.14159265358979323846);
    const float d = sqrtf(best);
    gstore(sdf + idx, wn >= 0.5 ? -d : d);
    if (winding) gstore(winding + idx, (float)wn);
}

__device__ __forceinline__ float sdf_lerp(float a, float b, float t) { return a + t * (b - a); }

// the field of grid `g` at p by the rules above; grad (may be NULL) receives the gradient
__device__ __forceinline__ float sdf_eval(const MeshGrid& g, const float* __restrict__ field, float px, float py, float pz,
                                          float* grad) {
    const float gx = (px - g.ox) / g.voxel, gy = (py - g.oy) / g.voxel, gz = (pz - g.oz) / g.voxel;
    const float cx = fminf(fmaxf(gx, 0.f), (float)(g.nx - 1)), cy = fminf(fmaxf(gy, 0.f), (float)(g.ny - 1));
    const float cz = fminf(fmaxf(gz, 0.f), (float)(g.nz - 1));
    const int i = min((int)cx, g.nx - 2), j = min((int)cy, g.ny - 2), k = min((int)cz, g.nz - 2);
    const float fx = cx - (float)i, fy = cy - (float)j, fz = cz - (float)k;
    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * (size_t)g.ny;
    const float* c = field + ((size_t)k * sz + (size_t)j * sy + (size_t)i);
    const float f000 = gload(c), f100 = gload(c + 1), f010 = gload(c + sy), f110 = gload(c + sy + 1);
    const float f001 = gload(c + sz), f101 = gload(c + sz + 1), f011 = gload(c + sz + sy), f111 = gload(c + sz + sy + 1);
    const float x00 = sdf_lerp(f000, f100, fx), x10 = sdf_lerp(f010, f110, fx);
    const float x01 = sdf_lerp(f001, f101, fx), x11 = sdf_lerp(f011, f111, fx);
    const float y0 = sdf_lerp(x00, x10, fy), y1 = sdf_lerp(x01, x11, fy);
    const float phi = sdf_lerp(y0, y1, fz);
    if (grad) {
        const float dx = sdf_lerp(sdf_lerp(f100 - f000, f110 - f010, fy), sdf_lerp(f101 - f001, f111 - f011, fy), fz);
        const float dy = sdf_lerp(x10 - x00, x11 - x01, fz);
        const float dz = y1 - y0;
        grad[0] = dx / g.voxel;
        grad[1] = dy / g.voxel;
        grad[2] = dz / g.voxel;
    }
    const float ox = (gx - cx) * g.voxel, oy = (gy - cy) * g.voxel, oz = (gz - cz) * g.voxel;
    const float rr = sdf_dot(ox, oy, oz, ox, oy, oz), m = fmaxf(phi, 0.f);
    return rr > 0.f ? sqrtf(rr + m * m) : phi;
}

__global__ __launch_bounds__(256) void sdf_sample_kernel(const MeshGrid g, const float* __restrict__ field, long long n_points,
                                                        const float* __restrict__ points, float* __restrict__ values,
                                                        float* __restrict__ gradients) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_points) return;
    const float* p = points + 3 * (size_t)idx;
    float grad[3];
    const float phi = sdf_eval(g, field, gload(p), gload(p + 1), gload(p + 2), gradients ? grad : nullptr);
    gstore(values + idx, phi);
    if (gradients) {
        gstore(gradients + 3 * (size_t)idx, grad[0]);
        gstore(gradients + 3 * (size_t)idx + 1, grad[1]);
        gstore(gradients + 3 * (size_t)idx + 2, grad[2]);
    }
}

// the float's bits in an order that unsigned integers keep: -inf < .. < -0 < +0 < .. < +inf < NaN
__device__ __forceinline__ uint32_t sdf_order_bits(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

__device__ __forceinline__ uint64_t sdf_wave_min(uint64_t v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d, WAVE);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void sdf_sweep_init_kernel(uint64_t* __restrict__ out, int n_words) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n_words) gstore(out + e, ~(uint64_t)0);
}

__global__ __launch_bounds__(SWEEP_THREADS) void sdf_sweep_kernel(const SweepJobTable T, uint64_t* __restrict__ out) {
    const int k = pose_job_of_block(T, blockIdx.x);
    const SweepJobDev& J = T.job[k];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const long long pi = (long long)(blockIdx.x - J.block0) * SWEEP_THREADS + tid;
    uint64_t key_phi = ~(uint64_t)0, key_s = ~(uint64_t)0;
    if (pi < J.n_shell) {
        const float* p = J.shell + 3 * (size_t)pi;
        const float lx = gload(p), ly = gload(p + 1), lz = gload(p + 2);
        const float x = ((J.Ra[0] * lx + J.Ra[1] * ly) + J.Ra[2] * lz) + J.ta[0];
        const float y = ((J.Ra[3] * lx + J.Ra[4] * ly) + J.Ra[5] * lz) + J.ta[1];
        const float z = ((J.Ra[6] * lx + J.Ra[7] * ly) + J.Ra[8] * lz) + J.ta[2];
        float phi0, s = 0.f;
        if (J.is_plane) {
            phi0 = sdf_dot(J.plane[0], J.plane[1], J.plane[2], x, y, z) - J.plane[3];
            const float c = -sdf_dot(J.plane[0], J.plane[1], J.plane[2], J.dir[0], J.dir[1], J.dir[2]);
            s = phi0 <= T.tol ? 0.f : (c > 0.f ? fminf(phi0 / c, T.max_travel) : T.max_travel);
        } else {
            auto field_at = [&](float travel) {
                const float zx = (x + travel * J.dir[0]) - J.tb[0], zy = (y + travel * J.dir[1]) - J.tb[1];
                const float zz = (z + travel * J.dir[2]) - J.tb[2];
                return sdf_eval(J.g, J.sdf, (J.Rb[0] * zx + J.Rb[3] * zy) + J.Rb[6] * zz, (J.Rb[1] * zx + J.Rb[4] * zy) + J.Rb[7] * zz,
                                (J.Rb[2] * zx + J.Rb[5] * zy) + J.Rb[8] * zz, nullptr);
            };
            phi0 = field_at(0.f);
            float phi = phi0;
            for (int step = 0; step < T.max_steps && phi > T.tol && s < T.max_travel; ++step) {
                s = fminf(s + phi, T.max_travel);
                phi = field_at(s);
            }
        }
        key_phi = ((uint64_t)sdf_order_bits(phi0) << 32) | (uint32_t)pi;
        key_s = ((uint64_t)sdf_order_bits(s) << 32) | (uint32_t)pi;
    }
    key_phi = sdf_wave_min(key_phi);
    key_s = sdf_wave_min(key_s);
    if (lane != 0 || key_phi == ~(uint64_t)0) return;
    uint64_t* o = out + 2 * ((size_t)T.first + (size_t)k);
    __hip_atomic_fetch_min((PGR_GLOBAL uint64_t*)o, key_phi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min((PGR_GLOBAL uint64_t*)(o + 1), key_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace pgr
