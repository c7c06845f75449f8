// rigid.hip.h -- rigid-body drops: contacts from mesh distance fields (pgr_rigid_contacts) and a batched sequential-impulse
// solver (pgr_rigid_simulate).  pegasus_amd/dynamics.py is the caller; tests/dynamics_reference.py restates every rule in
// float64; DESIGN.md section 24 holds the derivations and what is measured.  All arithmetic is float32 without contraction,
// every operation rounded on its own.  Dots are (x x + y y) + z z (sdf_dot), cross products a.y b.z - a.z b.y ..
//
// Bodies and worlds.  S independent worlds of B <= PGR_RIGID_MAX_BODIES slots.  A HOST table of at most PGR_RIGID_MAX_TYPES
//   body TYPES holds per type a geometry as pgr_sdf_sweep takes it (grid, device field, device shell points in the MESH frame,
//   n_shell), mass, the centre of mass c in the mesh frame, the inverse inertia about c in the mesh frame (3x3, row-major),
//   friction and the bounding radius max |shell - c|.  The device array type[S,B] (int32) names the type of every slot; a value
//   outside [0, n_types) is an empty slot.  State per (world, slot) is float32[13]: x (centre of mass, world), q (x, y, z, w;
//   unit), v, omega (world).  R(q) = [1 - 2(yy + zz), 2(xy - zw), 2(xz + yw); 2(xy + zw), 1 - 2(xx + zz), 2(yz - xw);
//   2(xz - yw), 2(yz + xw), 1 - 2(xx + yy)];  T = x - R c per axis ((R0 c.x + R1 c.y) + R2 c.z subtracted from x).  The ground is
//   the plane n.x = d, or (the *_ground entries, kernels instantiated with GROUND) a static field in world coordinates, as
//   pgr_sdf_from_tsdf writes it: then pair slot a B + a holds mover a against that field.  Spheres: sdf_eval(ground, x_a) -
//   radius_a - 2 voxel_g > margin: no contacts.  Point: (phi, grad) = pgr_sdf_sample's rule at the world point p, outside rule
//   included; a point without gn >= 1e-6 is no candidate; normal = grad / gn per component, no rotation.  mu_b is the ground's
//   friction; the rows are the plane's rows, the ground has no velocity; the plane of the parameters is checked and not used.
//
// One step (step h, gravity g), in this order:
//   1 Gravity and damping.  v <- (v + h g) fl,  omega <- omega fa  with  fl = (float) pow(1 - lin_damp, h),  fa likewise, taken
//     on the host in float64.  No gyroscopic term.
//   2 Contacts, from the poses at the START of the step.  For every ordered pair: mover a against the plane, then against every
//     b != a in ascending order; the pair's slot in the word array is a B + b, the plane's a B + a.
//       Spheres.  Plane: (n.x_a - d) - radius_a > margin: no contacts.  Body: sqrt(|x_a - x_b|^2) - (radius_a + radius_b) > margin.
//       Point.    Per shell point i of a:  p = ((R_a0 s.x + R_a1 s.y) + R_a2 s.z) + T_a ..;  against the plane phi = n.p - d and the
//                 normal is n; against b:  z = p - T_b, y = R_b^T z as in pgr_sdf_sweep, (phi, grad) = pgr_sdf_sample's rule on b's
//                 field at y (outside rule included), gn = sqrt(grad.grad); a point without gn >= 1e-6 is no candidate;
//                 u = grad / gn per component, normal = R_b u.
//       Candidates are the points with phi <= margin.
//       Words.    Seven 64-bit words per pair, each  order_bits(value) << 32 | i  (pgr_sdf_sweep's packing), reduced by integer
//                 minimum over the candidates: word 0 phi; words 1..6 the components of r = p - x_a as +r.x, -r.x, +r.y, -r.y, +r.z,
//                 -r.z.  A pair without candidates keeps all bits set.  Integer minima do not depend on arrival order: a run
//                 repeats to the bit, equal values resolve to the lowest index.
//       List.     The pair's contacts are the distinct indices of its words in ascending order (at most 7); the world's list is
//                 pair-major in the order above.
//   3 Rows.  Per contact p, phi, normal are evaluated again by the same rule (the same bits).  r_a = p - x_a, r_b = p - x_b.
//     t1 = normalize(normal x e), e = x^ where |normal.x| < 0.9 else y^ (division by sqrt of the dot); t2 = normal x t1.  Per
//     direction dir of (normal, t1, t2):  c_a = r_a x dir,  W_a = R_a (Iinv_a (R_a^T c_a)),  k = (1/m_a + c_a.W_a) [+ (1/m_b + c_b.W_b)],
//     m_eff = 1 / k.  bias = phi / h for phi > 0 (a speculative contact: the gap may close, not cross), else
//     -(beta max(-phi - slop, 0)) / h.  mu = mu_a mu_b, with the plane's friction as mu_b for a plane contact.  No restitution.
//   4 Solve.  `iterations` sweeps over the list in order.  Per contact the normal row first:
//       vrel = (dir.v_a + c_a.omega_a) [- (dir.v_b + c_b.omega_b)],  dl = -(vrel + bias) m_eff,  l' = max(l + dl, 0), dl = l' - l,
//       v_a += (dl / m_a) dir, omega_a += dl W_a, v_b -= (dl / m_b) dir, omega_b -= dl W_b;
//     then t1 and t2 with bias 0 and l' = clamp(l + dl, -mu l_n, mu l_n), l_n the normal row's accumulated impulse.
//   5 Integrate.  x <- x + h v.  q' = q + (h/2) (omega, 0) (x) q  with  (omega, 0) (x) (u, w) = (w omega + omega x u, -omega.u);
//     q <- q' / sqrt(q'.q').
//   6 Rest.  A per-world counter rises after each step in which every body has sqrt(v.v) < v_sleep and sqrt(omega.omega) < w_sleep,
//     else it returns to 0.  When it reaches sleep_steps (> 0) the world sleeps: velocities become zero, poses repeat,
//     rest_step[w] is that step's index.
//   7 Guard.  A world whose new state holds a value that is not finite keeps the state it had at the start of the step, is
//     frozen there and flagged in status[w] = 1; nothing that is not finite reaches the state or the trajectory.
// Record.  After every record_every-th step the mesh-frame pose (T = x - R c, q) goes to trajectory[S, n_records, B, 7]; an empty
//   slot writes (0,0,0, 0,0,0,1).
//
// Work.  rigid_contacts_kernel: one lane per shell point, 256 per workgroup, the grid over (world, pair, point block).  Slot,
//   sphere and sleep tests are the same in every lane, so they return before any field read.  A wave without a candidate writes
//   nothing; the others reduce their seven keys by xor butterfly (sdf_wave_min) and issue one 64-bit integer atomic minimum per
//   word at agent scope.  No LDS.  rigid_solve_kernel: one lane per world, 64 per workgroup (one wave: no barrier).  The bodies'
//   state lives in LDS as [slot][component][lane]; the rows go to the workspace as [contact][field][world] so that the lanes
//   of a wave read consecutive floats.  The kernel resets the words it consumed to all bits set for the next step.  A single
//   world uses one lane: accepted, the solver is sequential by its rule.  There is no floating-point atomic anywhere.  The type
//   table reaches both kernels through the workspace (rigid_table_kernel): indexed as a kernel argument it would live in scratch.
#pragma once
#include "meshsdf.hip.h"
#include "pgr_common.h"

namespace pgr {

constexpr int RIGID_MAX_BODIES = PGR_RIGID_MAX_BODIES;
constexpr int RIGID_MAX_TYPES = PGR_RIGID_MAX_TYPES;
constexpr int RIGID_WORDS = PGR_RIGID_WORDS;
constexpr int RIGID_STATE = PGR_RIGID_STATE;
constexpr int RIGID_CONTACT_THREADS = 256;
constexpr int RIGID_SOLVE_THREADS = WAVE;
constexpr int RIGID_ROW_FIELDS = 56;
constexpr uint32_t RIGID_NO_BODY = 0xFFu;

struct RigidTypeDev {
    MeshGrid g;
    float mass;
    const float* sdf;
    const float* shell;
    int32_t n_shell;
    float friction, radius;
    float com[3];
    float iinv[9];
};

struct RigidTable {                                   // the host's table as a kernel argument: rigid_table_kernel writes it to memory
    RigidTypeDev t[RIGID_MAX_TYPES];
};
static_assert(sizeof(RigidTable) <= 2048, "RigidTable must fit the kernel argument segment");

struct RigidParamsDev {
    float h, gx, gy, gz;
    float nx, ny, nz, d;
    float plane_friction, lin_factor, ang_factor, beta;
    float slop, margin, v_sleep, w_sleep;
    int32_t iterations, sleep_steps, n_types, pad;
};

struct RigidGroundDev {                              // the ground as a field in world coordinates (GROUND kernels only)
    MeshGrid g;
    const float* sdf;
    float friction;
};

struct RigidFrame {                                  // a body's pose: R(q) row-major and T = x - R c
    float R[9], T[3];
};

__device__ __forceinline__ RigidFrame rigid_frame(const float* x, const float* q, const float* c) {
    RigidFrame F;
    const float xx = q[0] * q[0], yy = q[1] * q[1], zz = q[2] * q[2];
    const float xy = q[0] * q[1], xz = q[0] * q[2], yz = q[1] * q[2];
    const float xw = q[0] * q[3], yw = q[1] * q[3], zw = q[2] * q[3];
    F.R[0] = 1.f - 2.f * (yy + zz);
    F.R[1] = 2.f * (xy - zw);
    F.R[2] = 2.f * (xz + yw);
    F.R[3] = 2.f * (xy + zw);
    F.R[4] = 1.f - 2.f * (xx + zz);
    F.R[5] = 2.f * (yz - xw);
    F.R[6] = 2.f * (xz - yw);
    F.R[7] = 2.f * (yz + xw);
    F.R[8] = 1.f - 2.f * (xx + yy);
    F.T[0] = x[0] - ((F.R[0] * c[0] + F.R[1] * c[1]) + F.R[2] * c[2]);
    F.T[1] = x[1] - ((F.R[3] * c[0] + F.R[4] * c[1]) + F.R[5] * c[2]);
    F.T[2] = x[2] - ((F.R[6] * c[0] + F.R[7] * c[1]) + F.R[8] * c[2]);
    return F;
}

// shell point s of a mover at frame A against the plane (`plane`) or against the field of `target` at frame Bf:
// the point p, the field value phi and the unit normal in the world.  false: the gradient gives no normal.  GROUND: the
// plane's place is taken by the field G, sampled at p itself; its gradient is the normal, with no rotation.
template <bool GROUND>
__device__ __forceinline__ bool rigid_point(const RigidFrame& A, float sx, float sy, float sz, const RigidParamsDev& P,
                                            const RigidGroundDev& G, bool plane, const RigidTypeDev& target, const RigidFrame& Bf,
                                            float* p, float& phi, float* n) {
    p[0] = ((A.R[0] * sx + A.R[1] * sy) + A.R[2] * sz) + A.T[0];
    p[1] = ((A.R[3] * sx + A.R[4] * sy) + A.R[5] * sz) + A.T[1];
    p[2] = ((A.R[6] * sx + A.R[7] * sy) + A.R[8] * sz) + A.T[2];
    if (plane) {
        if constexpr (GROUND) {
            float g[3];
            phi = sdf_eval(G.g, G.sdf, p[0], p[1], p[2], g);
            const float gn = sqrtf(sdf_dot(g[0], g[1], g[2], g[0], g[1], g[2]));
            if (!(gn >= 1e-6f)) return false;
            n[0] = g[0] / gn;
            n[1] = g[1] / gn;
            n[2] = g[2] / gn;
            return true;
        }
        phi = sdf_dot(P.nx, P.ny, P.nz, p[0], p[1], p[2]) - P.d;
        n[0] = P.nx;
        n[1] = P.ny;
        n[2] = P.nz;
        return true;
    }
    const float zx = p[0] - Bf.T[0], zy = p[1] - Bf.T[1], zz = p[2] - Bf.T[2];
    float g[3];
    phi = sdf_eval(target.g, target.sdf, (Bf.R[0] * zx + Bf.R[3] * zy) + Bf.R[6] * zz, (Bf.R[1] * zx + Bf.R[4] * zy) + Bf.R[7] * zz,
                   (Bf.R[2] * zx + Bf.R[5] * zy) + Bf.R[8] * zz, g);
    const float gn = sqrtf(sdf_dot(g[0], g[1], g[2], g[0], g[1], g[2]));
    if (!(gn >= 1e-6f)) return false;
    const float ux = g[0] / gn, uy = g[1] / gn, uz = g[2] / gn;
    n[0] = (Bf.R[0] * ux + Bf.R[1] * uy) + Bf.R[2] * uz;
    n[1] = (Bf.R[3] * ux + Bf.R[4] * uy) + Bf.R[5] * uz;
    n[2] = (Bf.R[6] * ux + Bf.R[7] * uy) + Bf.R[8] * uz;
    return true;
}

__device__ __forceinline__ int32_t rigid_type_of(const int32_t* type, size_t slot, int32_t n_types) {
    const int32_t t = gload(type + slot);
    return (t >= 0 && t < n_types) ? t : -1;
}

// The kernels index the type table with a number they read from memory; indexing a kernel ARGUMENT that way would move the
// whole table to scratch.  So one lane copies it, entry by entry with constant indices, into the workspace.
__global__ __launch_bounds__(WAVE) void rigid_table_kernel(const RigidTable T, RigidTypeDev* __restrict__ table) {
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < RIGID_MAX_TYPES; ++k) table[k] = T.t[k];
}

__global__ __launch_bounds__(256) void rigid_init_kernel(uint64_t* __restrict__ words, long long n_words, int32_t* __restrict__ halt,
                                                        int32_t* __restrict__ rest_count, int32_t* __restrict__ rest_step,
                                                        int32_t* __restrict__ status, int32_t S) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < n_words) gstore(words + e, ~(uint64_t)0);
    if (halt && e < S) {
        gstore((uint32_t*)halt + e, 0u);
        gstore((uint32_t*)rest_count + e, 0u);
        gstore((uint32_t*)rest_step + e, 0xFFFFFFFFu);
        gstore((uint32_t*)status + e, 0u);
    }
}

template <bool GROUND>
__global__ __launch_bounds__(RIGID_CONTACT_THREADS) void rigid_contacts_kernel(const RigidTypeDev* __restrict__ table,
                                                                               const RigidParamsDev P, const RigidGroundDev G,
                                                                               int32_t B,
                                                                               const int32_t* __restrict__ type,
                                                                               const float* __restrict__ state,
                                                                               const int32_t* __restrict__ halt,
                                                                               uint64_t* __restrict__ words) {
    const int w = blockIdx.x, pair = blockIdx.y, a = pair / B, b = pair - a * B;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    if (halt && gload(halt + w) != 0) return;
    const int ta = __builtin_amdgcn_readfirstlane(rigid_type_of(type, (size_t)w * B + a, P.n_types));
    if (ta < 0) return;
    const RigidTypeDev A = table[ta];
    if ((long long)blockIdx.z * RIGID_CONTACT_THREADS >= A.n_shell) return;
    const float* sa = state + ((size_t)w * B + a) * RIGID_STATE;
    float xa[3], qa[4];
    for (int k = 0; k < 3; ++k) xa[k] = gload(sa + k);
    for (int k = 0; k < 4; ++k) qa[k] = gload(sa + 3 + k);
    const bool plane = b == a;
    RigidTypeDev Bt{};
    RigidFrame Fb{};
    if (plane) {
        if constexpr (GROUND) {                          // two voxels: the field's error and slope
            if ((sdf_eval(G.g, G.sdf, xa[0], xa[1], xa[2], nullptr) - A.radius) - 2.f * G.g.voxel > P.margin) return;
        } else {
            if ((sdf_dot(P.nx, P.ny, P.nz, xa[0], xa[1], xa[2]) - P.d) - A.radius > P.margin) return;
        }
    } else {
        const int tb = __builtin_amdgcn_readfirstlane(rigid_type_of(type, (size_t)w * B + b, P.n_types));
        if (tb < 0) return;
        Bt = table[tb];
        const float* sb = state + ((size_t)w * B + b) * RIGID_STATE;
        float xb[3], qb[4];
        for (int k = 0; k < 3; ++k) xb[k] = gload(sb + k);
        for (int k = 0; k < 4; ++k) qb[k] = gload(sb + 3 + k);
        const float dx = xa[0] - xb[0], dy = xa[1] - xb[1], dz = xa[2] - xb[2];
        if (sqrtf(sdf_dot(dx, dy, dz, dx, dy, dz)) - (A.radius + Bt.radius) > P.margin) return;
        Fb = rigid_frame(xb, qb, Bt.com);
    }
    const RigidFrame Fa = rigid_frame(xa, qa, A.com);
    const long long pi = (long long)blockIdx.z * RIGID_CONTACT_THREADS + tid;
    uint64_t key[RIGID_WORDS];
#pragma unroll
    for (int k = 0; k < RIGID_WORDS; ++k) key[k] = ~(uint64_t)0;
    if (pi < A.n_shell) {
        const float* s = A.shell + 3 * (size_t)pi;
        float p[3], n[3], phi;
        if (rigid_point<GROUND>(Fa, gload(s), gload(s + 1), gload(s + 2), P, G, plane, Bt, Fb, p, phi, n) && phi <= P.margin) {
            const float rx = p[0] - xa[0], ry = p[1] - xa[1], rz = p[2] - xa[2];
            const float value[RIGID_WORDS] = {phi, rx, -rx, ry, -ry, rz, -rz};
#pragma unroll
            for (int k = 0; k < RIGID_WORDS; ++k) key[k] = ((uint64_t)sdf_order_bits(value[k]) << 32) | (uint32_t)pi;
        }
    }
#pragma unroll
    for (int k = 0; k < RIGID_WORDS; ++k) key[k] = sdf_wave_min(key[k]);
    if (lane != 0 || key[0] == ~(uint64_t)0) return;
    uint64_t* o = words + ((size_t)w * B * B + pair) * RIGID_WORDS;
#pragma unroll
    for (int k = 0; k < RIGID_WORDS; ++k)
        __hip_atomic_fetch_min((PGR_GLOBAL uint64_t*)(o + k), key[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the fields of a row, [contact][field][world] in the workspace
enum RigidRowField : int {
    ROW_BODIES = 0,                                  // a | b << 8 as an integer's bits; b = RIGID_NO_BODY for the plane
    ROW_DIR = 1,                                     // normal, t1, t2: 9
    ROW_CA = 10,                                     // r_a x dir: 9
    ROW_WA = 19,                                     // R_a Iinv_a R_a^T (r_a x dir): 9
    ROW_CB = 28,
    ROW_WB = 37,
    ROW_MEFF = 46,                                   // 3
    ROW_BIAS = 49,
    ROW_MU = 50,
    ROW_IMA = 51,                                    // 1 / m_a
    ROW_IMB = 52,
    ROW_LAMBDA = 53,                                 // 3
};
static_assert(ROW_LAMBDA + 3 == RIGID_ROW_FIELDS, "row layout");

// W = R (Iinv (R^T c)) for a body at rotation R with inverse inertia Iinv in its own frame
__device__ __forceinline__ void rigid_apply_iinv(const float* R, const float* I, float cx, float cy, float cz, float* W) {
    const float lx = (R[0] * cx + R[3] * cy) + R[6] * cz, ly = (R[1] * cx + R[4] * cy) + R[7] * cz;
    const float lz = (R[2] * cx + R[5] * cy) + R[8] * cz;
    const float mx = (I[0] * lx + I[1] * ly) + I[2] * lz, my = (I[3] * lx + I[4] * ly) + I[5] * lz;
    const float mz = (I[6] * lx + I[7] * ly) + I[8] * lz;
    W[0] = (R[0] * mx + R[1] * my) + R[2] * mz;
    W[1] = (R[3] * mx + R[4] * my) + R[5] * mz;
    W[2] = (R[6] * mx + R[7] * my) + R[8] * mz;
}

template <bool GROUND>
__global__ __launch_bounds__(RIGID_SOLVE_THREADS) void rigid_solve_kernel(
    const RigidTypeDev* __restrict__ table, const RigidParamsDev P, const RigidGroundDev G, int32_t S, int32_t B,
    const int32_t* __restrict__ type,
    float* __restrict__ state,
    uint64_t* __restrict__ words, float* __restrict__ rows, int32_t* __restrict__ halt, int32_t* __restrict__ rest_count,
    int32_t step, int32_t record, int32_t n_records, float* __restrict__ trajectory, int32_t* __restrict__ rest_step,
    int32_t* __restrict__ status) {
    __shared__ float s_state[RIGID_MAX_BODIES * RIGID_STATE * WAVE];             // [slot][component][lane]: 26 KiB
    __shared__ int32_t s_type[RIGID_MAX_BODIES * WAVE];
    const int lane = threadIdx.x;
    const long long w = (long long)blockIdx.x * RIGID_SOLVE_THREADS + lane;
    if (w >= S) return;                                                          // one wave, no barrier: a lane may leave
#define RIGID_ST(slot, comp) s_state[((slot) * RIGID_STATE + (comp)) * WAVE + lane]
    const size_t S_ = (size_t)S;
    float* my_state = state + (size_t)w * B * RIGID_STATE;
    auto load_state = [&]() {
        for (int a = 0; a < B; ++a)
            for (int k = 0; k < RIGID_STATE; ++k) RIGID_ST(a, k) = gload(my_state + a * RIGID_STATE + k);
    };
    for (int a = 0; a < B; ++a) s_type[a * WAVE + lane] = rigid_type_of(type, (size_t)w * B + a, P.n_types);
    load_state();
    int halted = gload(halt + w);
    if (!halted) {
        // 1: gravity and damping
        const float hgx = P.h * P.gx, hgy = P.h * P.gy, hgz = P.h * P.gz;
        for (int a = 0; a < B; ++a) {
            if (s_type[a * WAVE + lane] < 0) continue;
            RIGID_ST(a, 7) = (RIGID_ST(a, 7) + hgx) * P.lin_factor;
            RIGID_ST(a, 8) = (RIGID_ST(a, 8) + hgy) * P.lin_factor;
            RIGID_ST(a, 9) = (RIGID_ST(a, 9) + hgz) * P.lin_factor;
            for (int k = 10; k < 13; ++k) RIGID_ST(a, k) = RIGID_ST(a, k) * P.ang_factor;
        }
        // 2, 3: the contact list from the words, and its rows
        int nc = 0;
        for (int a = 0; a < B; ++a) {
            const int ta = s_type[a * WAVE + lane];
            if (ta < 0) continue;
            const RigidTypeDev A = table[ta];
            const float xa[3] = {RIGID_ST(a, 0), RIGID_ST(a, 1), RIGID_ST(a, 2)};
            const float qa[4] = {RIGID_ST(a, 3), RIGID_ST(a, 4), RIGID_ST(a, 5), RIGID_ST(a, 6)};
            const RigidFrame Fa = rigid_frame(xa, qa, A.com);
            const float ima = 1.f / A.mass;
            for (int j = 0; j < B; ++j) {
                const int b = j == 0 ? a : (j - 1 < a ? j - 1 : j);              // the plane first, then b != a ascending
                const bool plane = b == a;
                uint64_t* o = words + ((size_t)w * B * B + (size_t)a * B + b) * RIGID_WORDS;
                if (gload(o) == ~(uint64_t)0) continue;
                uint32_t idx[RIGID_WORDS];
#pragma unroll
                for (int k = 0; k < RIGID_WORDS; ++k) {
                    idx[k] = (uint32_t)gload(o + k);
                    gstore(o + k, ~(uint64_t)0);
                }
                const int tb = plane ? -1 : s_type[b * WAVE + lane];
                if (!plane && tb < 0) continue;
                RigidTypeDev Bt{};
                if (!plane) Bt = table[tb];
                RigidFrame Fb{};
                float xb[3] = {0.f, 0.f, 0.f}, imb = 0.f, mu = A.friction * (GROUND ? G.friction : P.plane_friction);
                if (!plane) {
                    xb[0] = RIGID_ST(b, 0);
                    xb[1] = RIGID_ST(b, 1);
                    xb[2] = RIGID_ST(b, 2);
                    const float qb[4] = {RIGID_ST(b, 3), RIGID_ST(b, 4), RIGID_ST(b, 5), RIGID_ST(b, 6)};
                    Fb = rigid_frame(xb, qb, Bt.com);
                    imb = 1.f / Bt.mass;
                    mu = A.friction * Bt.friction;
                }
                long long last = -1;
                for (int k = 0; k < RIGID_WORDS; ++k) {
                    uint32_t m = 0xFFFFFFFFu;
#pragma unroll
                    for (int i = 0; i < RIGID_WORDS; ++i)
                        if ((long long)idx[i] > last && idx[i] < m) m = idx[i];
                    if (m == 0xFFFFFFFFu || m >= (uint32_t)A.n_shell) break;
                    last = m;
                    const float* s = A.shell + 3 * (size_t)m;
                    float p[3], n[3], phi;
                    if (!rigid_point<GROUND>(Fa, gload(s), gload(s + 1), gload(s + 2), P, G, plane, Bt, Fb, p, phi, n)) continue;
                    float* row = rows + ((size_t)nc * RIGID_ROW_FIELDS) * S_ + (size_t)w;
                    const float ra[3] = {p[0] - xa[0], p[1] - xa[1], p[2] - xa[2]};
                    const float rb[3] = {p[0] - xb[0], p[1] - xb[1], p[2] - xb[2]};
                    // t1 = normalize(n x e), t2 = n x t1
                    float t1[3], t2[3];
                    if (fabsf(n[0]) < 0.9f) {
                        t1[0] = 0.f;
                        t1[1] = n[2];
                        t1[2] = -n[1];
                    } else {
                        t1[0] = -n[2];
                        t1[1] = 0.f;
                        t1[2] = n[0];
                    }
                    const float tn = sqrtf(sdf_dot(t1[0], t1[1], t1[2], t1[0], t1[1], t1[2]));
                    t1[0] = t1[0] / tn;
                    t1[1] = t1[1] / tn;
                    t1[2] = t1[2] / tn;
                    t2[0] = n[1] * t1[2] - n[2] * t1[1];
                    t2[1] = n[2] * t1[0] - n[0] * t1[2];
                    t2[2] = n[0] * t1[1] - n[1] * t1[0];
                    const float dir[9] = {n[0], n[1], n[2], t1[0], t1[1], t1[2], t2[0], t2[1], t2[2]};
                    gstore((uint32_t*)row + ROW_BODIES * S_, (uint32_t)a | ((plane ? RIGID_NO_BODY : (uint32_t)b) << 8));
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const float dx = dir[3 * d], dy = dir[3 * d + 1], dz = dir[3 * d + 2];
                        const float ca[3] = {ra[1] * dz - ra[2] * dy, ra[2] * dx - ra[0] * dz, ra[0] * dy - ra[1] * dx};
                        float Wa[3], cb[3] = {0.f, 0.f, 0.f}, Wb[3] = {0.f, 0.f, 0.f};
                        rigid_apply_iinv(Fa.R, A.iinv, ca[0], ca[1], ca[2], Wa);
                        float kk = ima + sdf_dot(ca[0], ca[1], ca[2], Wa[0], Wa[1], Wa[2]);
                        if (!plane) {
                            cb[0] = rb[1] * dz - rb[2] * dy;
                            cb[1] = rb[2] * dx - rb[0] * dz;
                            cb[2] = rb[0] * dy - rb[1] * dx;
                            rigid_apply_iinv(Fb.R, Bt.iinv, cb[0], cb[1], cb[2], Wb);
                            kk = kk + (imb + sdf_dot(cb[0], cb[1], cb[2], Wb[0], Wb[1], Wb[2]));
                        }
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            gstore(row + (ROW_DIR + 3 * d + c) * S_, dir[3 * d + c]);
                            gstore(row + (ROW_CA + 3 * d + c) * S_, ca[c]);
                            gstore(row + (ROW_WA + 3 * d + c) * S_, Wa[c]);
                            gstore(row + (ROW_CB + 3 * d + c) * S_, cb[c]);
                            gstore(row + (ROW_WB + 3 * d + c) * S_, Wb[c]);
                        }
                        gstore(row + (ROW_MEFF + d) * S_, 1.f / kk);
                        gstore(row + (ROW_LAMBDA + d) * S_, 0.f);
                    }
                    gstore(row + ROW_BIAS * S_, phi > 0.f ? phi / P.h : -(P.beta * fmaxf(-phi - P.slop, 0.f)) / P.h);
                    gstore(row + ROW_MU * S_, mu);
                    gstore(row + ROW_IMA * S_, ima);
                    gstore(row + ROW_IMB * S_, imb);
                    ++nc;
                }
            }
        }
        // 4: sequential impulses
        for (int it = 0; it < P.iterations; ++it) {
            for (int c = 0; c < nc; ++c) {
                float* row = rows + ((size_t)c * RIGID_ROW_FIELDS) * S_ + (size_t)w;
                const uint32_t ab = gload((const uint32_t*)row + ROW_BODIES * S_);
                const int a = (int)(ab & 0xFFu), b = (int)(ab >> 8);
                const bool two = (uint32_t)b != RIGID_NO_BODY;
                const float ima = gload(row + ROW_IMA * S_), imb = gload(row + ROW_IMB * S_);
                const float mu = gload(row + ROW_MU * S_), bias = gload(row + ROW_BIAS * S_);
                float ln = 0.f;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    float dir[3], ca[3], Wa[3], cb[3], Wb[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        dir[k] = gload(row + (ROW_DIR + 3 * d + k) * S_);
                        ca[k] = gload(row + (ROW_CA + 3 * d + k) * S_);
                        Wa[k] = gload(row + (ROW_WA + 3 * d + k) * S_);
                        cb[k] = gload(row + (ROW_CB + 3 * d + k) * S_);
                        Wb[k] = gload(row + (ROW_WB + 3 * d + k) * S_);
                    }
                    const float meff = gload(row + (ROW_MEFF + d) * S_), l0 = gload(row + (ROW_LAMBDA + d) * S_);
                    float vrel = sdf_dot(dir[0], dir[1], dir[2], RIGID_ST(a, 7), RIGID_ST(a, 8), RIGID_ST(a, 9)) +
                                 sdf_dot(ca[0], ca[1], ca[2], RIGID_ST(a, 10), RIGID_ST(a, 11), RIGID_ST(a, 12));
                    if (two)
                        vrel = vrel - (sdf_dot(dir[0], dir[1], dir[2], RIGID_ST(b, 7), RIGID_ST(b, 8), RIGID_ST(b, 9)) +
                                       sdf_dot(cb[0], cb[1], cb[2], RIGID_ST(b, 10), RIGID_ST(b, 11), RIGID_ST(b, 12)));
                    float l1;
                    if (d == 0) {
                        l1 = fmaxf(l0 + -(vrel + bias) * meff, 0.f);
                        ln = l1;
                    } else {
                        const float lim = mu * ln;
                        l1 = fminf(fmaxf(l0 + -vrel * meff, -lim), lim);
                    }
                    const float dl = l1 - l0;
                    gstore(row + (ROW_LAMBDA + d) * S_, l1);
                    const float ja = dl * ima;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        RIGID_ST(a, 7 + k) = RIGID_ST(a, 7 + k) + ja * dir[k];
                        RIGID_ST(a, 10 + k) = RIGID_ST(a, 10 + k) + dl * Wa[k];
                    }
                    if (two) {
                        const float jb = dl * imb;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            RIGID_ST(b, 7 + k) = RIGID_ST(b, 7 + k) - jb * dir[k];
                            RIGID_ST(b, 10 + k) = RIGID_ST(b, 10 + k) - dl * Wb[k];
                        }
                    }
                }
            }
        }
        // 5: integrate; 6: rest; 7: guard
        bool finite = true, calm = true;
        const float hh = 0.5f * P.h;
        for (int a = 0; a < B; ++a) {
            if (s_type[a * WAVE + lane] < 0) continue;
            const float vx = RIGID_ST(a, 7), vy = RIGID_ST(a, 8), vz = RIGID_ST(a, 9);
            const float ox = RIGID_ST(a, 10), oy = RIGID_ST(a, 11), oz = RIGID_ST(a, 12);
            const float qx = RIGID_ST(a, 3), qy = RIGID_ST(a, 4), qz = RIGID_ST(a, 5), qw = RIGID_ST(a, 6);
            RIGID_ST(a, 0) = RIGID_ST(a, 0) + P.h * vx;
            RIGID_ST(a, 1) = RIGID_ST(a, 1) + P.h * vy;
            RIGID_ST(a, 2) = RIGID_ST(a, 2) + P.h * vz;
            const float nx = qx + hh * (qw * ox + (oy * qz - oz * qy)), ny = qy + hh * (qw * oy + (oz * qx - ox * qz));
            const float nz = qz + hh * (qw * oz + (ox * qy - oy * qx)), nw = qw + hh * -sdf_dot(ox, oy, oz, qx, qy, qz);
            const float len = sqrtf((nx * nx + ny * ny) + (nz * nz + nw * nw));
            RIGID_ST(a, 3) = nx / len;
            RIGID_ST(a, 4) = ny / len;
            RIGID_ST(a, 5) = nz / len;
            RIGID_ST(a, 6) = nw / len;
            calm = calm && sqrtf(sdf_dot(vx, vy, vz, vx, vy, vz)) < P.v_sleep && sqrtf(sdf_dot(ox, oy, oz, ox, oy, oz)) < P.w_sleep;
            for (int k = 0; k < RIGID_STATE; ++k) finite = finite && isfinite(RIGID_ST(a, k));
        }
        if (!finite) {
            load_state();                                                        // the state of the step's start, still in memory
            gstore((uint32_t*)status + w, 1u);
            gstore((uint32_t*)halt + w, 2u);
        } else {
            const int32_t count = calm ? gload(rest_count + w) + 1 : 0;
            gstore((uint32_t*)rest_count + w, (uint32_t)count);
            if (P.sleep_steps > 0 && count >= P.sleep_steps) {
                for (int a = 0; a < B; ++a)
                    for (int k = 7; k < RIGID_STATE; ++k)
                        if (s_type[a * WAVE + lane] >= 0) RIGID_ST(a, k) = 0.f;
                gstore((uint32_t*)rest_step + w, (uint32_t)step);
                gstore((uint32_t*)halt + w, 1u);
            }
            for (int a = 0; a < B; ++a)
                for (int k = 0; k < RIGID_STATE; ++k) gstore(my_state + a * RIGID_STATE + k, RIGID_ST(a, k));
        }
    }
    if (record < 0) return;
    for (int a = 0; a < B; ++a) {
        float* out = trajectory + ((((size_t)w * n_records + record) * B) + a) * 7;
        const int ta = s_type[a * WAVE + lane];
        float pose[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        if (ta >= 0) {
            const float x[3] = {RIGID_ST(a, 0), RIGID_ST(a, 1), RIGID_ST(a, 2)};
            const float q[4] = {RIGID_ST(a, 3), RIGID_ST(a, 4), RIGID_ST(a, 5), RIGID_ST(a, 6)};
            const float c[3] = {gload(table[ta].com), gload(table[ta].com + 1), gload(table[ta].com + 2)};
            const RigidFrame F = rigid_frame(x, q, c);
            pose[0] = F.T[0];
            pose[1] = F.T[1];
            pose[2] = F.T[2];
            pose[3] = q[0];
            pose[4] = q[1];
            pose[5] = q[2];
            pose[6] = q[3];
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) gstore(out + k, pose[k]);
    }
#undef RIGID_ST
}

}  // namespace pgr
