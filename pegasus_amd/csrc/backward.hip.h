// backward.hip.h -- backward pass of the rasterizer (the in-tree user is training:
// /root/reference/src/gs/gs_training.py:7,46).  Same conventions as oracle/pgr_oracle_backward.c: the 0.99 clamp
// of alpha is not differentiated, the screen-space mean gradient is NDC-scaled (pixel gradient * W/2, H/2),
// colours clamped at 0 and clamped view-space coordinates pass no gradient.
//
// pgr_backward, for one view as for a batch, runs the same two kernels on a table of per-view entries; a one-view call
// runs their ONE instances (n_views pinned to 1, view 0).
//   composite_backward_batch_kernel  one wave per 4x4-pixel block, four list entries per step (below), for every
//       (view, tile) item of the forward's interleaved work order in one launch, into per-view rows [n_views, n, GRAD_ROW]:
//       the ten per-Gaussian partial gradients of an entry are summed over the block's pixels and land as one 10-lane
//       float atomic on the Gaussian's row.  An optional dL/dalpha [H,W] (alpha = 1 - final_T, the accumulated opacity)
//       adds g_alpha T_final / (1 - alpha_i) to the opacity-side gradient of every blended entry i.
//   preprocess_backward_batch_kernel  one thread per Gaussian over the views in order, summing in registers: conic ->
//       cov2D -> (cov3D, view-space mean); projection; SH -> coefficients and view direction; cov3D -> scale / rotation
//       once, on the sum.
#pragma once
#include <type_traits>
#include "composite.hip.h"
#include "pgr_common.h"
#include "preprocess.hip.h"

namespace pgr {

// per-Gaussian accumulator row written by the compositor backward (same shape as the forward record)
//   [0] d/dx_pix  [1] d/dy_pix  [2] d/dA  [3] d/dB  [4] d/dC  [5] d/dopacity  [6..8] d/drgb  [9] d/dz
constexpr int GRAD_ROW = 12;

// ---- compositor backward: one wave per 4x4-pixel block, four list entries per step ------------------------------
// The tile's list is walked BACK to front from the deepest contributor of any pixel of the block, in 64-entry batches
// gathered one batch ahead (composite.hip.h's gather); only the entries the forward's skip test lets through for this
// block are parked (an entry that cannot reach alpha >= 1/255 in the block was blended by none of its pixels).
// With ONE view per launch (training) a kernel lasts as long as its longest wave; the first round-2 form -- one wave
// per 8x8 quarter, one entry per step, 0.72 ms on the 2 M-Gaussian scene after 1.97 ms for round 1's 16x8 half tiles
// with two pixels per lane -- spent 1 000 dependent steps on a quarter whose pixels blended 1 000 entries.  Here
// lane = 4 * pixel + slot, and the four lanes of a pixel take four CONSECUTIVE parked entries at once.  What is sequential in the walk -- T <- T / (1 - alpha) and the suffix sums
// of colour and depth -- is a prefix product and four prefix sums over the four lanes of a quad (two quad_perm steps
// each); everything else is per entry.  The ten partials are summed over the block's 16 pixels (two row shifts, then a
// 640-byte LDS transpose that also lines the 4 x 10 totals up for ONE atomic instruction).
// The walk of one block (`item` = 4 * tile + quarter of the view, block = blockIdx.x & 3 inside the quarter).  The view's
// images are read as global memory (gload): through the table's generic pointers a load is a flat one, and the 64-bit
// per-lane addresses cost the walk two VGPRs.
// ALPHA: the walk takes a dL/dalpha image (g_alpha, which may still be NULL).  The alpha term keeps one more register live
// over the walk, so the launches without one use the ALPHA = false instance: the walk as it was before the term existed,
// instruction for instruction.
template <bool ALPHA>
__device__ __forceinline__ void composite_backward_block(
    const CameraDev* __restrict__ camp, const uint2* __restrict__ ranges, const uint32_t* __restrict__ gauss_sorted,
    const float4* __restrict__ splats, const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
    const float* __restrict__ g_color, const float* __restrict__ g_depth, const float* __restrict__ g_alpha,
    float* __restrict__ g_rows, uint32_t item) {
    const CameraDev& cam = *camp;
    const int W = cam.width, H = cam.height;
    const int tile = (int)(item >> 2), quarter = (int)(item & 3), sub = (int)(blockIdx.x & 3);
    const int tile_x = tile % cam.grid_x, tile_y = tile / cam.grid_x;
    const int lane = threadIdx.x, slot = lane & 3, pl = lane >> 2;
    const int bx0 = tile_x * TILE + (quarter & 1) * 8 + (sub & 1) * 4, by0 = tile_y * TILE + (quarter >> 1) * 8 + (sub >> 1) * 4;
    if (bx0 >= W || by0 >= H) return;
    const int px = bx0 + (pl & 3), py = by0 + (pl >> 2);
    const bool inside = px < W && py < H;
    const size_t P = (size_t)W * H;
    const size_t pix = inside ? (size_t)py * W + px : 0;
    const uint2 range = gload(ranges + tile);

    const uint32_t last = inside ? gload(n_contrib + pix) : 0u;
    float T = inside ? gload(final_T + pix) : 0.0f;        // per-pixel state, the same in the four lanes of a pixel
    float S[3], gC[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gC[c] = inside ? gload(g_color + c * P + pix) : 0.0f;
        S[c] = T * cam.bg[c];
    }
    const float gD = (inside && g_depth) ? gload(g_depth + pix) : 0.0f;
    // alpha = 1 - T_final, dalpha/dalpha_i = T_final / (1 - alpha_i): the FORWARD's final T (the walk overwrites T) times r
    const float gAT = (ALPHA && inside && g_alpha) ? gload(g_alpha + pix) * T : 0.0f;
    float SD = 0.0f;
    uint32_t n_used = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n_used = max(n_used, (uint32_t)__shfl_xor((int)n_used, d, WAVE));
    n_used = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_used);
    if (n_used == 0) return;

    __shared__ float4 s_q0[WAVE_BATCH], s_q1[WAVE_BATCH], s_q2[WAVE_BATCH];
    __shared__ uint2 s_gi[WAVE_BATCH];           // (Gaussian, list position)
    __shared__ float s_red[10 * 16];             // [value][row of the wave][slot]
    const float pxf = (float)px, pyf = (float)py;
    const float rx0 = (float)bx0, ry0 = (float)by0;
    const float rx1 = fminf(rx0 + 3.0f, (float)(W - 1)), ry1 = fminf(ry0 + 3.0f, (float)(H - 1));
    const bool ge1 = slot >= 1, ge2 = slot >= 2;
    const int out_slot = lane / 10, out_k = lane - out_slot * 10;      // lanes 0..39: (entry slot, value) of the atomic

    f32x4_t q0 = {0.f, 0.f, 0.f, 0.f}, q1 = q0, q2 = q0;
    uint32_t g_cur = 0, g_next = 0;
    auto fetch_index = [&](int base) {
        const int i = base + lane;
        return (base >= 0 && i < (int)n_used) ? gload(gauss_sorted + range.x + i) : 0u;
    };
    auto fetch_record = [&](int base, uint32_t g) {
        g_cur = g;
        if (base >= 0 && base + lane < (int)n_used) {
            const float4* rec = splats + (size_t)g * 3;
            q0 = gload_quad(rec); q1 = gload_quad(rec + 1); q2 = gload_quad(rec + 2);
        }
    };
    // quad_perm lane exchange inside the four lanes of a pixel
    auto quad = [](float v, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xF, 0xF, true));
    };
    using QP_0012 = std::integral_constant<int, 0x90>;    // quad_perm [0,0,1,2]: the lane one slot down
    using QP_0101 = std::integral_constant<int, 0x44>;    // quad_perm [0,1,0,1]: the lane two slots down
    using QP_3333 = std::integral_constant<int, 0xFF>;    // quad_perm [3,3,3,3]: the pixel's last slot
    auto prefix_prod = [&](float x) {
        const float a = quad(x, QP_0012{}); x = ge1 ? x * a : x;
        const float b = quad(x, QP_0101{}); x = ge2 ? x * b : x;
        return x;
    };
    auto prefix_sum = [&](float x) {
        const float a = quad(x, QP_0012{}); x = ge1 ? x + a : x;
        const float b = quad(x, QP_0101{}); x = ge2 ? x + b : x;
        return x;
    };

    const int first = (int)((n_used - 1) / WAVE_BATCH) * WAVE_BATCH;
    fetch_record(first, fetch_index(first));
    g_next = fetch_index(first - WAVE_BATCH);

    for (int base = first; base >= 0; base -= WAVE_BATCH) {
        asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(g_cur));      // the quads are taken as they arrive, here
        const bool have = base + lane < (int)n_used;
        const bool live = have && rect_may_contribute(make_cull_splat(make_float2(q0.x, q0.y), make_float4(q0.z, q0.w, q1.x, q1.y),
                                                                      q1.z, q1.w), rx0, ry0, rx1, ry1);
        const unsigned long long mask = __ballot(live);
        const int cnt = __popcll(mask);
        if (live) {
            const int pos = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            s_q0[pos] = make_float4(q0.x, q0.y, q0.z, q0.w);
            s_q1[pos] = make_float4(q1.x, q1.y, q1.z, q1.w);
            s_q2[pos] = make_float4(q2.x, q2.y, q2.z, q2.w);
            s_gi[pos] = make_uint2(g_cur, (uint32_t)(base + lane));
        }
        __syncthreads();
        fetch_record(base - WAVE_BATCH, g_next);      // lands while this batch is walked
        g_next = fetch_index(base - 2 * WAVE_BATCH);
        for (int hi = cnt - 1; hi >= 0; hi -= 4) {     // slot 0 takes entry hi (the deepest), slot 3 entry hi - 3
            const int j = hi - slot;
            const int jc = j < 0 ? 0 : j;
            const float4 e0 = s_q0[jc], e1 = s_q1[jc], e2 = s_q2[jc];
            const uint2 gi = s_gi[jc];
            const float A = e0.z, B = e0.w, Cc = e1.x, op = e1.y;
            const float dx = e0.x - pxf, dy = e0.y - pyf;
            const float power = fmaf(dx, fmaf(-0.5f * A, dx, -B * dy), (-0.5f * Cc * dy) * dy);
            const float G = __builtin_amdgcn_exp2f(power * 1.4426950408889634f);
            const float alpha = fminf(ALPHA_MAX, op * G);
            const bool valid = j >= 0 && gi.y < last && !(power > 0.0f) && !(alpha < ALPHA_MIN);
            if (__builtin_amdgcn_ballot_w64(valid) == 0ull) continue;
            const float av = valid ? alpha : 0.0f;
            const float r = valid ? 1.0f / (1.0f - alpha) : 1.0f;
            const float Tin = T * prefix_prod(r);          // transmittance in front of this lane's entry
            const float w = av * Tin;
            const float col[3] = {e2.x, e2.y, e2.z};
            const float z = e2.w;
            float cin[4], cinc[4];
#pragma unroll
            for (int c = 0; c < 3; ++c) cin[c] = w * col[c];
            cin[3] = w * z;
#pragma unroll
            for (int c = 0; c < 4; ++c) cinc[c] = prefix_sum(cin[c]);
            float acc[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) acc[k] = 0.0f;
            if (valid) {
                float dL_dalpha = 0.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float Sb = S[c] + (cinc[c] - cin[c]);         // the sum behind this lane's entry
                    dL_dalpha += gC[c] * (Tin * col[c] - Sb * r);
                    acc[6 + c] = w * gC[c];
                }
                dL_dalpha += gD * (Tin * z - (SD + (cinc[3] - cin[3])) * r);
                if constexpr (ALPHA) dL_dalpha += gAT * r;
                acc[9] = w * gD;
                acc[5] = G * dL_dalpha;
                const float dLp = G * op * dL_dalpha;    // dL/dpower
                acc[2] = -0.5f * dx * dx * dLp;
                acc[3] = -dx * dy * dLp;
                acc[4] = -0.5f * dy * dy * dLp;
                acc[0] = -(A * dx + B * dy) * dLp;
                acc[1] = -(Cc * dy + B * dx) * dLp;
            }
            // the pixel's state after these four entries: what its last slot holds
            T = quad(Tin, QP_3333{});
#pragma unroll
            for (int c = 0; c < 3; ++c) S[c] += quad(cinc[c], QP_3333{});
            SD += quad(cinc[3], QP_3333{});
            // sums over the 16 pixels: lanes 4 apart inside a row of 16, then the four rows through LDS
            // A DPP operand read needs two wait states after the VALU write of that register.  Both row steps and the s_nop
            // in front of them are ONE asm statement: the hazard recognizer does not look into inline asm, and between separate
            // statements the compiler may place register copies for the "+v" operands (a v_mov right in front of a DPP read of
            // its destination).  Inside the block every register's two steps are ten instructions apart.
#define PGR_ROW_STEP(CTRL)                                                                                                  \
    "v_add_f32_dpp %0, %0, %0 " CTRL "\n\tv_add_f32_dpp %1, %1, %1 " CTRL "\n\tv_add_f32_dpp %2, %2, %2 " CTRL "\n\t"            \
    "v_add_f32_dpp %3, %3, %3 " CTRL "\n\tv_add_f32_dpp %4, %4, %4 " CTRL "\n\tv_add_f32_dpp %5, %5, %5 " CTRL "\n\t"            \
    "v_add_f32_dpp %6, %6, %6 " CTRL "\n\tv_add_f32_dpp %7, %7, %7 " CTRL "\n\tv_add_f32_dpp %8, %8, %8 " CTRL "\n\t"            \
    "v_add_f32_dpp %9, %9, %9 " CTRL "\n\t"
            asm volatile("s_nop 1\n\t"
                         PGR_ROW_STEP("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                         PGR_ROW_STEP("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                         : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]),
                           "+v"(acc[7]), "+v"(acc[8]), "+v"(acc[9]));
#undef PGR_ROW_STEP
            if ((lane & 12) == 12) {
#pragma unroll
                for (int k = 0; k < 10; ++k) s_red[k * 16 + (lane >> 4) * 4 + slot] = acc[k];
            }
            __builtin_amdgcn_wave_barrier();
            if (lane < 40 && hi - out_slot >= 0) {
                const float* red = s_red + out_k * 16 + out_slot;
                const float tot = (red[0] + red[4]) + (red[8] + red[12]);
                if (tot != 0.0f) atomicAdd(g_rows + (size_t)s_gi[hi - out_slot].x * GRAD_ROW + out_k, tot);
            }
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
    }
}

// ---- batch backward (pgr_backward): the backward of a pgr_forward call of any number of views -------------------------
// One entry per view, in device memory (written by backward_table_kernel from the launch arguments), read through the
// scalar cache: the forward's lists in the workspace, the view's image gradients and forward outputs, and the view's own
// rows of the [n_views, n, GRAD_ROW] accumulator (screen-space partials: they cannot be summed over views).  The packed
// cameras are a kernel argument instead (the workspace's array, one per view): a camera reached through a pointer loaded
// from the table is read with per-lane flat loads into VGPRs, one through the argument with scalar loads.
struct alignas(16) BwdViewDev {
    const uint2* ranges;
    const uint32_t* gauss_sorted;
    const float4* splats;
    const uint32_t* counters;    // [1] != 0: the forward overflowed this view (it was not composited; nothing to walk)
    const float* g_color;        // [3,H,W]
    const float* g_depth;        // [H,W] or NULL
    const float* final_T;        // [H,W]
    const uint32_t* n_contrib;   // [H,W]
    const int32_t* radii;        // [n]
    float* rows;                 // [n, GRAD_ROW]
    const float* g_alpha;        // [H,W] or NULL: dL/dalpha, alpha = 1 - final_T
};
static_assert(sizeof(BwdViewDev) == 96, "BWD_TABLE_CHUNK sizes the table launch's kernel arguments by 96-byte entries");
constexpr int BWD_TABLE_CHUNK = 16;            // views per table launch (kernel arguments: 16 x 96 bytes)
struct BwdTableChunk { BwdViewDev v[BWD_TABLE_CHUNK]; };
__global__ __launch_bounds__(64) void backward_table_kernel(BwdTableChunk chunk, int count, BwdViewDev* __restrict__ out) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(chunk.v);
    uint32_t* dst = reinterpret_cast<uint32_t*>(out);
    const int words = count * (int)(sizeof(BwdViewDev) / 4);
    for (int k = threadIdx.x; k < words; k += blockDim.x) dst[k] = src[k];
}

// The compositor backward of EVERY view in one launch: the forward's interleaved work order (item = view * items_per_view +
// 4 * tile + quarter, as composite_quarter_kernel reads it), so no view waits on its own slowest tile -- the single-view
// launch lasts as long as its longest wave.  ONE: the instance for a one-view call (n_views = 1, view 0).
template <bool ALPHA, bool ONE>
__global__ __launch_bounds__(WAVE) void composite_backward_batch_kernel(const BwdViewDev* __restrict__ views,
                                                                        const CameraDev* __restrict__ cams, uint32_t n_views,
                                                                        uint32_t items_per_view,
                                                                        const uint32_t* __restrict__ work_order) {
    if (ONE) n_views = 1;
    uint32_t item = work_order[blockIdx.x >> 2];
    if (item == INVALID_ITEM) return;
    const uint32_t view = ONE ? 0u : item / items_per_view;
    if (view >= n_views) return;
    item -= view * items_per_view;
    const BwdViewDev& bv = views[view];
    if (gload(bv.counters + 1)) return;
    composite_backward_block<ALPHA>(cams + view, bv.ranges, bv.gauss_sorted, bv.splats, bv.final_T, bv.n_contrib, bv.g_color,
                                    bv.g_depth, bv.g_alpha, bv.rows, item);
}

struct GradOut {
    float* means2d;    // [n,3] or NULL
    float* means3d;    // [n,3] or NULL
    float* opacities;  // [n]   or NULL
    float* colors;     // [n,3] or NULL (gradient wrt the per-Gaussian rgb)
    float* shs;        // [n,sh_stride,3] or NULL
    float* cov3d;      // [n,6] or NULL
    float* scales;     // [n,3] or NULL
    float* rotations;  // [n,4] or NULL
};

template <int DEG>
__device__ __forceinline__ void sh_basis_grad(float x, float y, float z, float b[16], float bx[16], float by[16],
                                              float bz[16]) {
    constexpr float C1 = 0.4886025119029199f;
    constexpr float C2_0 = 1.0925484305920792f, C2_1 = -1.0925484305920792f, C2_2 = 0.31539156525252005f,
                    C2_3 = -1.0925484305920792f, C2_4 = 0.5462742152960396f;
    constexpr float C3_0 = -0.5900435899266435f, C3_1 = 2.890611442640554f, C3_2 = -0.4570457994644658f,
                    C3_3 = 0.3731763325901154f, C3_4 = -0.4570457994644658f, C3_5 = 1.445305721320277f,
                    C3_6 = -0.5900435899266435f;
#pragma unroll
    for (int k = 0; k < 16; ++k) b[k] = bx[k] = by[k] = bz[k] = 0.0f;
    b[0] = 0.28209479177387814f;
    if constexpr (DEG > 0) {
        b[1] = -C1 * y; by[1] = -C1;
        b[2] = C1 * z;  bz[2] = C1;
        b[3] = -C1 * x; bx[3] = -C1;
    }
    if constexpr (DEG > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        b[4] = C2_0 * xy;                  bx[4] = C2_0 * y;  by[4] = C2_0 * x;
        b[5] = C2_1 * yz;                  by[5] = C2_1 * z;  bz[5] = C2_1 * y;
        b[6] = C2_2 * (2 * zz - xx - yy);  bx[6] = C2_2 * -2 * x; by[6] = C2_2 * -2 * y; bz[6] = C2_2 * 4 * z;
        b[7] = C2_3 * xz;                  bx[7] = C2_3 * z;  bz[7] = C2_3 * x;
        b[8] = C2_4 * (xx - yy);           bx[8] = C2_4 * 2 * x; by[8] = C2_4 * -2 * y;
        if constexpr (DEG > 2) {
            b[9] = C3_0 * y * (3 * xx - yy);   bx[9] = C3_0 * 6 * xy; by[9] = C3_0 * (3 * xx - 3 * yy);
            b[10] = C3_1 * xy * z;             bx[10] = C3_1 * yz; by[10] = C3_1 * xz; bz[10] = C3_1 * xy;
            b[11] = C3_2 * y * (4 * zz - xx - yy);
            bx[11] = C3_2 * -2 * xy; by[11] = C3_2 * (4 * zz - xx - 3 * yy); bz[11] = C3_2 * 8 * yz;
            b[12] = C3_3 * z * (2 * zz - 3 * xx - 3 * yy);
            bx[12] = C3_3 * -6 * xz; by[12] = C3_3 * -6 * yz; bz[12] = C3_3 * (6 * zz - 3 * xx - 3 * yy);
            b[13] = C3_4 * x * (4 * zz - xx - yy);
            bx[13] = C3_4 * (4 * zz - 3 * xx - yy); by[13] = C3_4 * -2 * xy; bz[13] = C3_4 * 8 * xz;
            b[14] = C3_5 * z * (xx - yy);      bx[14] = C3_5 * 2 * xz; by[14] = C3_5 * -2 * yz; bz[14] = C3_5 * (xx - yy);
            b[15] = C3_6 * x * (xx - 3 * yy);  bx[15] = C3_6 * (3 * xx - 3 * yy); by[15] = C3_6 * -6 * xy;
        }
    }
}

// The (DEG+1)^2 x 3 active SH coefficients of Gaussian i into shv (16-byte quads where the rows allow: sh_quads)
template <int DEG>
__device__ __forceinline__ void load_sh_active(const PgrScene& sc, int i, bool sh_quads, float* shv) {
    constexpr int NC = (DEG + 1) * (DEG + 1);
    const float* sh = sc.shs + (size_t)i * sc.sh_stride * 3;
    if (sh_quads) {
#pragma unroll
        for (int q = 0; q < (3 * NC + 3) / 4; ++q) {
            const float4 x = reinterpret_cast<const float4*>(sh)[q];
            const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (4 * q + c < 3 * NC) shv[4 * q + c] = e[c];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * NC; ++k) shv[k] = sh[k];
    }
}

// The SH step of one view: the rgb gradient gc (zero on a channel clamped at 0) -> coefficients (ADDED to gsh) and the
// unit view direction u (gu, set).  The direction u = (p - campos) / |p - campos| passes (gu - u (u . gu)) / |p - campos|
// on to the mean, and its negative to campos.
// load_sh_active and sh_backward are the camera kernel's.  preprocess_backward_batch_kernel keeps the same steps written
// out in its body: called there, either helper changes how that kernel is scheduled (its ISA differs), and the existing
// instances are held to the code they compiled to.
template <int DEG>
__device__ __forceinline__ void sh_backward(const float* shv, const float gc[3], const float u[3], float* gsh, float gu[3]) {
    constexpr int NC = (DEG + 1) * (DEG + 1);
    float bb[16], bx[16], by[16], bz[16];
    sh_basis_grad<DEG>(u[0], u[1], u[2], bb, bx, by, bz);
    gu[0] = 0.f; gu[1] = 0.f; gu[2] = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float accv = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) accv += bb[k] * shv[3 * k + ch];
        const float g = (accv + 0.5f < 0.0f) ? 0.f : gc[ch];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            gsh[3 * k + ch] += bb[k] * g;
            gu[0] += g * shv[3 * k + ch] * bx[k];
            gu[1] += g * shv[3 * k + ch] * by[k];
            gu[2] += g * shv[3 * k + ch] * bz[k];
        }
    }
}

// 3D covariance of Gaussian i as the forward formed it (recomputed from scale / rotation, or the precomputed one)
__device__ __forceinline__ void load_cov3d(const PgrScene& sc, int i, float cov[6]) {
    if (sc.cov3d_precomp) {
#pragma unroll
        for (int k = 0; k < 6; ++k) cov[k] = sc.cov3d_precomp[6 * (size_t)i + k];
    } else {
        const float4 q = reinterpret_cast<const float4*>(sc.rotations)[i];
        cov3d_from_scale_rot(sc.scales[3 * i], sc.scales[3 * i + 1], sc.scales[3 * i + 2], sc.scale_modifier, q, cov);
    }
}

// One view's geometry chain for a Gaussian the view rendered: the compositor's row -> NDC-scaled screen gradient (gndc, set),
// conic -> cov2D -> the six cov3D partials (gS, set) and the view-space / projected position -> mean gradient (ADDED to gp).
// CAM (camera_backward_kernel): also the partials of the 32 matrix entries the forward reads, ADDED to gcam[0..31]
// (viewmatrix [0..15], projmatrix [16..31], both in PgrCamera's transposed storage), from the same intermediate terms:
//   the projection  h = p pm (row vector p = (x, y, z, 1)), ndc = h.xy / (h.w + 1e-7): dL/dpm[4k+c] = dL/dh_c p_k;
//   the view space  t_r = p . vm[4k+r]: dL/dvm[4k+r] += gt_r p_k (gt: the full view-space gradient, depth and clamps in);
//   the Jacobian    T = J W, W[r][k] = vm[4k+r]: dL/dvm[4k+0] += gT0_k j00, [4k+1] += gT1_k j11, [4k+2] += gT0_k j02 + gT1_k j12.
// vm[4k+3] and pm[4k+2] are never read and receive nothing.  The CAM = false instance is the chain as it was before.
template <bool CAM = false>
__device__ __forceinline__ void view_geometry_backward(const CameraDev& cam, const float* row, const float p[3],
                                                       const float cov[6], float gp[3], float gS[6], float gndc[2],
                                                       float* gcam = nullptr) {
    const float* vm = cam.view;
    const float* pm = cam.proj;
    // ---- screen position
    gndc[0] = row[0] * 0.5f * (float)cam.width;
    gndc[1] = row[1] * 0.5f * (float)cam.height;
    {
        const float hx = pm[0] * p[0] + pm[4] * p[1] + pm[8] * p[2] + pm[12];
        const float hy = pm[1] * p[0] + pm[5] * p[1] + pm[9] * p[2] + pm[13];
        const float hw = pm[3] * p[0] + pm[7] * p[1] + pm[11] * p[2] + pm[15];
        const float mw = 1.0f / (hw + 0.0000001f);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            gp[k] += gndc[0] * (pm[4 * k + 0] * mw - hx * mw * mw * pm[4 * k + 3]) +
                     gndc[1] * (pm[4 * k + 1] * mw - hy * mw * mw * pm[4 * k + 3]);
        if constexpr (CAM) {
            const float ghx = gndc[0] * mw, ghy = gndc[1] * mw, ghw = -(gndc[0] * hx + gndc[1] * hy) * mw * mw;
            const float ph[4] = {p[0], p[1], p[2], 1.0f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                gcam[16 + 4 * k + 0] += ghx * ph[k];
                gcam[16 + 4 * k + 1] += ghy * ph[k];
                gcam[16 + 4 * k + 3] += ghw * ph[k];
            }
        }
    }
    // ---- view-space position
    float t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = vm[r] * p[0] + vm[4 + r] * p[1] + vm[8 + r] * p[2] + vm[12 + r];
    float gt[3] = {0.f, 0.f, row[9]};

    // ---- 3D covariance
    const float S3[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
    const float fx = cam.focal_x, fy = cam.focal_y;
    const float limx = 1.3f * cam.tanfovx, limy = 1.3f * cam.tanfovy;
    const float txtz = t[0] / t[2], tytz = t[1] / t[2];
    const float cx = fminf(limx, fmaxf(-limx, txtz)) * t[2], cy = fminf(limy, fmaxf(-limy, tytz)) * t[2];
    const float xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f, ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
    const float j00 = fx / t[2], j02 = -fx * cx / (t[2] * t[2]), j11 = fy / t[2], j12 = -fy * cy / (t[2] * t[2]);
    float T0[3], T1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T0[k] = j00 * vm[4 * k + 0] + j02 * vm[4 * k + 2];
        T1[k] = j11 * vm[4 * k + 1] + j12 * vm[4 * k + 2];
    }
    float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            a += T0[r] * S3[r][s] * T0[s];
            b += T0[r] * S3[r][s] * T1[s];
            c += T1[r] * S3[r][s] * T1[s];
        }
    a += LOWPASS; c += LOWPASS;
    const float det = a * c - b * b, d2 = 1.0f / (det * det);
    const float gA = row[2], gB = row[3], gCc = row[4];
    const float ga = d2 * (-c * c * gA + b * c * gB - b * b * gCc);
    const float gb = d2 * (2 * b * c * gA - (det + 2 * b * b) * gB + 2 * a * b * gCc);
    const float gc = d2 * (-b * b * gA + a * b * gB - a * a * gCc);
    gS[0] = ga * T0[0] * T0[0] + gb * T0[0] * T1[0] + gc * T1[0] * T1[0];
    gS[3] = ga * T0[1] * T0[1] + gb * T0[1] * T1[1] + gc * T1[1] * T1[1];
    gS[5] = ga * T0[2] * T0[2] + gb * T0[2] * T1[2] + gc * T1[2] * T1[2];
    gS[1] = 2 * ga * T0[0] * T0[1] + gb * (T0[0] * T1[1] + T0[1] * T1[0]) + 2 * gc * T1[0] * T1[1];
    gS[2] = 2 * ga * T0[0] * T0[2] + gb * (T0[0] * T1[2] + T0[2] * T1[0]) + 2 * gc * T1[0] * T1[2];
    gS[4] = 2 * ga * T0[1] * T0[2] + gb * (T0[1] * T1[2] + T0[2] * T1[1]) + 2 * gc * T1[1] * T1[2];
    float gj00 = 0.f, gj02 = 0.f, gj11 = 0.f, gj12 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int s = 0; s < 3; ++s) { s0 += S3[k][s] * T0[s]; s1 += S3[k][s] * T1[s]; }
        const float gT0 = 2 * ga * s0 + gb * s1, gT1 = 2 * gc * s1 + gb * s0;
        gj00 += gT0 * vm[4 * k + 0]; gj02 += gT0 * vm[4 * k + 2];
        gj11 += gT1 * vm[4 * k + 1]; gj12 += gT1 * vm[4 * k + 2];
        if constexpr (CAM) {
            gcam[4 * k + 0] += gT0 * j00;
            gcam[4 * k + 1] += gT1 * j11;
            gcam[4 * k + 2] += gT0 * j02 + gT1 * j12;
        }
    }
    const float tz2 = 1.0f / (t[2] * t[2]), tz3 = tz2 / t[2];
    gt[0] += xmul * -fx * tz2 * gj02;
    gt[1] += ymul * -fy * tz2 * gj12;
    gt[2] += -fx * tz2 * gj00 - fy * tz2 * gj11 + 2 * fx * cx * tz3 * gj02 + 2 * fy * cy * tz3 * gj12;
    if (xmul == 0.f) gt[2] += -fx * tz2 * gj02 * (cx / t[2]);
    if (ymul == 0.f) gt[2] += -fy * tz2 * gj12 * (cy / t[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) gp[k] += vm[4 * k + 0] * gt[0] + vm[4 * k + 1] * gt[1] + vm[4 * k + 2] * gt[2];
    if constexpr (CAM) {
        const float ph[4] = {p[0], p[1], p[2], 1.0f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int r = 0; r < 3; ++r) gcam[4 * k + r] += gt[r] * ph[k];
    }
}

// cov3D = (R S)(R S)^T -> scale and rotation (gS: the six partials of cov3D; linear in them)
__device__ __forceinline__ void scale_rot_backward(const PgrScene& sc, int i, const float gS[6], float gs[3], float gq[4]) {
    const float4 q4 = reinterpret_cast<const float4*>(sc.rotations)[i];
    const float r = q4.x, x = q4.y, y = q4.z, z = q4.w;
    const float R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)},
                           {2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)},
                           {2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)}};
    const float s[3] = {sc.scale_modifier * sc.scales[3 * i], sc.scale_modifier * sc.scales[3 * i + 1],
                        sc.scale_modifier * sc.scales[3 * i + 2]};
    const float Gf[3][3] = {{gS[0], 0.5f * gS[1], 0.5f * gS[2]}, {0.5f * gS[1], gS[3], 0.5f * gS[4]},
                            {0.5f * gS[2], 0.5f * gS[4], gS[5]}};
    float gR[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float accs = 0.f;
#pragma unroll
        for (int a_ = 0; a_ < 3; ++a_) {
            float gM = 0.f;
#pragma unroll
            for (int m = 0; m < 3; ++m) gM += 2 * Gf[a_][m] * R[m][k] * s[k];
            accs += gM * R[a_][k];
            gR[a_][k] = gM * s[k];
        }
        gs[k] = accs * sc.scale_modifier;
    }
    gq[0] = 2 * (-z * gR[0][1] + y * gR[0][2] + z * gR[1][0] - x * gR[1][2] - y * gR[2][0] + x * gR[2][1]);
    gq[1] = 2 * (y * gR[0][1] + z * gR[0][2] + y * gR[1][0] - 2 * x * gR[1][1] - r * gR[1][2] + z * gR[2][0] +
                 r * gR[2][1] - 2 * x * gR[2][2]);
    gq[2] = 2 * (-2 * y * gR[0][0] + x * gR[0][1] + r * gR[0][2] + x * gR[1][0] + z * gR[1][2] - r * gR[2][0] +
                 z * gR[2][1] - 2 * y * gR[2][2]);
    gq[3] = 2 * (-2 * z * gR[0][0] - r * gR[0][1] + x * gR[0][2] + r * gR[1][0] - 2 * z * gR[1][1] + y * gR[1][2] +
                 x * gR[2][0] + y * gR[2][1]);
}

// Per-Gaussian backward: one thread per Gaussian walks the views in a fixed order (0 .. n_views-1), as the forward
// preprocess walks them, and sums in registers what each view that rendered the Gaussian contributes: mean, the six cov3D
// partials, opacity, rgb and the (DEG+1)^2 x 3 SH coefficients.  means2d[v] (the screen-space gradient densification reads
// per view) is written per view; the cov3D -> scale / rotation chain is linear in the cov3D gradient and runs ONCE, on the
// sum.  Every output is written exactly once, no atomics.
// Registers: cov3D and the active SH coefficients are loaded where they are first used, and colour / opacity summed after
// the SH step, so that none of them is live across the geometry chain.  ONE: the one-view instance (n_views == 1); at
// DEG 0-1 it is bounded to 8 waves per SIMD (64 VGPRs, no spills) -- left alone the scheduler stops at 65-66.
template <int DEG, bool ONE>
__global__ __launch_bounds__(256, ONE && DEG < 2 ? 8 : 1) void preprocess_backward_batch_kernel(
    PgrScene sc, const BwdViewDev* __restrict__ views, const CameraDev* __restrict__ cams, int n_views, GradOut o) {
    if (ONE) n_views = 1;
    constexpr int NC = (DEG + 1) * (DEG + 1);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sc.n) return;
    const bool sh_quads = sc.shs && sc.sh_stride == 16 && (reinterpret_cast<uintptr_t>(sc.shs) & 15u) == 0 &&
                          (!o.shs || (reinterpret_cast<uintptr_t>(o.shs) & 15u) == 0);
    const float p[3] = {sc.means3d[3 * i], sc.means3d[3 * i + 1], sc.means3d[3 * i + 2]};
    float gp[3] = {0.f, 0.f, 0.f}, gS[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gcol[3] = {0.f, 0.f, 0.f}, gop = 0.f;
    float shv[3 * NC], gsh[3 * NC];      // the active coefficients (k, channel) and their summed gradients
#pragma unroll
    for (int k = 0; k < 3 * NC; ++k) { shv[k] = 0.f; gsh[k] = 0.f; }
    bool any = false;
    float cov[6];
    for (int v = 0; v < n_views; ++v) {
        const BwdViewDev& bv = views[v];
        const bool live = gload(bv.radii + i) > 0 && !gload(bv.counters + 1);
        float gndc[2] = {0.f, 0.f};
        if (live) {
            if (!any) load_cov3d(sc, i, cov);      // per-Gaussian inputs: read once, at the first view that rendered it
            const CameraDev& cam = cams[v];
            const float* row = bv.rows + (size_t)i * GRAD_ROW;
            const float gc[3] = {row[6], row[7], row[8]};
            float gpv[3] = {0.f, 0.f, 0.f}, gSv[6];
            view_geometry_backward(cam, row, p, cov, gpv, gSv, gndc);
            if (sc.shs) {
                if (!any) {      // the active coefficients, loaded where they are first used
                    const float* sh = sc.shs + (size_t)i * sc.sh_stride * 3;
                    if (sh_quads) {
#pragma unroll
                        for (int q = 0; q < (3 * NC + 3) / 4; ++q) {
                            const float4 x = reinterpret_cast<const float4*>(sh)[q];
                            const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                            for (int c = 0; c < 4; ++c)
                                if (4 * q + c < 3 * NC) shv[4 * q + c] = e[c];
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < 3 * NC; ++k) shv[k] = sh[k];
                    }
                }
                const float d[3] = {p[0] - cam.campos[0], p[1] - cam.campos[1], p[2] - cam.campos[2]};
                const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                const float u[3] = {d[0] / len, d[1] / len, d[2] / len};
                float bb[16], bx[16], by[16], bz[16];
                sh_basis_grad<DEG>(u[0], u[1], u[2], bb, bx, by, bz);
                float gu[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float accv = 0.f;
#pragma unroll
                    for (int k = 0; k < NC; ++k) accv += bb[k] * shv[3 * k + ch];
                    const float g = (accv + 0.5f < 0.0f) ? 0.f : gc[ch];
#pragma unroll
                    for (int k = 0; k < NC; ++k) {
                        gsh[3 * k + ch] += bb[k] * g;
                        gu[0] += g * shv[3 * k + ch] * bx[k];
                        gu[1] += g * shv[3 * k + ch] * by[k];
                        gu[2] += g * shv[3 * k + ch] * bz[k];
                    }
                }
                const float dot = u[0] * gu[0] + u[1] * gu[1] + u[2] * gu[2];
#pragma unroll
                for (int k = 0; k < 3; ++k) gpv[k] += (gu[k] - u[k] * dot) / len;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) gp[k] += gpv[k];
#pragma unroll
            for (int k = 0; k < 6; ++k) gS[k] += gSv[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) gcol[c] += gc[c];
            gop += row[5];
            any = true;
        }
        if (o.means2d) {
            float* m2 = o.means2d + ((size_t)v * sc.n + i) * 3;
            m2[0] = gndc[0]; m2[1] = gndc[1]; m2[2] = 0.f;
        }
    }
    if (o.shs) {     // coefficients above the active degree (and every coefficient of an unseen Gaussian) receive zero
        if (sh_quads) {
            float4* dst = reinterpret_cast<float4*>(o.shs + (size_t)i * 48);
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                float e[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) e[c] = 4 * q + c < 3 * NC ? gsh[4 * q + c] : 0.f;
                dst[q] = make_float4(e[0], e[1], e[2], e[3]);
            }
        } else {
            float* dst = o.shs + (size_t)i * sc.sh_stride * 3;
#pragma unroll
            for (int k = 0; k < 3 * NC; ++k) dst[k] = gsh[k];
            for (int k = 3 * NC; k < sc.sh_stride * 3; ++k) dst[k] = 0.f;
        }
    }
    if (o.scales || o.rotations) {
        float gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};
        if (any && sc.scales && sc.rotations) scale_rot_backward(sc, i, gS, gs, gq);
        if (o.scales) { o.scales[3 * i] = gs[0]; o.scales[3 * i + 1] = gs[1]; o.scales[3 * i + 2] = gs[2]; }
        if (o.rotations) reinterpret_cast<float4*>(o.rotations)[i] = make_float4(gq[0], gq[1], gq[2], gq[3]);
    }
    if (o.means3d) { o.means3d[3 * i] = gp[0]; o.means3d[3 * i + 1] = gp[1]; o.means3d[3 * i + 2] = gp[2]; }
    if (o.opacities) o.opacities[i] = gop;
    if (o.colors) { o.colors[3 * i] = gcol[0]; o.colors[3 * i + 1] = gcol[1]; o.colors[3 * i + 2] = gcol[2]; }
    if (o.cov3d) {
#pragma unroll
        for (int k = 0; k < 6; ++k) o.cov3d[6 * (size_t)i + k] = gS[k];
    }
}

// ---- camera backward (PgrBackwardCall::camera_grads) -------------------------------------------------------------------
// The exact partials of the loss with respect to the 35 camera numbers the forward reads per view (viewmatrix [16],
// projmatrix [16], campos [3]; treated as independent inputs), after the two launches above and from their rows:
//   camera_backward_kernel      one thread per Gaussian over the views in order, as preprocess_backward_batch_kernel: the
//       view's geometry chain (view_geometry_backward<true>) and SH step (sh_backward: dL/dcampos = -(gu - u (u . gu)) / len)
//       of every Gaussian the view rendered, summed over the workgroup in a fixed order -- within each row of 16 lanes by
//       DPP shifts, the 16 row totals through LDS -- into one CAM_GRAD-float partial per (view, workgroup);
//   camera_grad_finish_kernel   one workgroup per view: the view's partials summed in a fixed order, WRITTEN to the caller's
//       outputs.  No float atomics: every workgroup adding into one 35-float row would serialise on it.
// Discrete decisions (near cull, radius and tile rectangle, sort order) have no gradient; Gaussians a view did not render
// (radii 0) or a view that overflowed contribute nothing.
constexpr int CAM_GRAD = 35;
constexpr int CAM_BLOCK = 256;                 // threads per workgroup of both kernels: 16 rows of 16 lanes

template <int CTRL>
__device__ __forceinline__ float dpp_shift(float v) {      // row_shr / bound_ctrl: lanes shifted in from outside the row read 0
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// Sum of g[k] over the CAM_BLOCK threads of the workgroup, returned to thread k (k < CAM_GRAD); every thread must call it.
// Inclusive scans over each row of 16 lanes (row_shr 1, 2, 4, 8: lane 15 ends with the row's sum), the 16 row sums through
// LDS, added in row order.  Deterministic: the same inputs give the same bits.
__device__ __forceinline__ float camera_block_sum(const float g[CAM_GRAD], float* s_red) {
    const int t = threadIdx.x, row = t >> 4;
#pragma unroll
    for (int k = 0; k < CAM_GRAD; ++k) {
        float v = g[k];
        v += dpp_shift<0x111>(v);
        v += dpp_shift<0x112>(v);
        v += dpp_shift<0x114>(v);
        v += dpp_shift<0x118>(v);
        if ((t & 15) == 15) s_red[row * CAM_GRAD + k] = v;
    }
    __syncthreads();
    float tot = 0.f;
    if (t < CAM_GRAD) {
#pragma unroll
        for (int r = 0; r < CAM_BLOCK / 16; ++r) tot += s_red[r * CAM_GRAD + t];
    }
    __syncthreads();      // s_red is rewritten by the next call
    return tot;
}

// partials [n_views, gridDim.x, CAM_GRAD]: every (view, workgroup) entry is written.  ONE: the one-view instance.
template <int DEG, bool ONE>
__global__ __launch_bounds__(CAM_BLOCK) void camera_backward_kernel(PgrScene sc, const BwdViewDev* __restrict__ views,
                                                                    const CameraDev* __restrict__ cams, int n_views,
                                                                    float* __restrict__ partials) {
    if (ONE) n_views = 1;
    constexpr int NC = (DEG + 1) * (DEG + 1);
    __shared__ float s_red[(CAM_BLOCK / 16) * CAM_GRAD];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool real = i < sc.n;          // (threads past the end take part in the sums with zeros)
    const bool sh_quads = sc.shs && sc.sh_stride == 16 && (reinterpret_cast<uintptr_t>(sc.shs) & 15u) == 0;
    float p[3] = {0.f, 0.f, 0.f};
    if (real) { p[0] = sc.means3d[3 * i]; p[1] = sc.means3d[3 * i + 1]; p[2] = sc.means3d[3 * i + 2]; }
    float cov[6], shv[3 * NC];
#pragma unroll
    for (int k = 0; k < 3 * NC; ++k) shv[k] = 0.f;
    bool have = false;
    for (int v = 0; v < n_views; ++v) {
        const BwdViewDev& bv = views[v];
        float g[CAM_GRAD];
#pragma unroll
        for (int k = 0; k < CAM_GRAD; ++k) g[k] = 0.f;
        if (real && gload(bv.radii + i) > 0 && !gload(bv.counters + 1)) {
            if (!have) {
                load_cov3d(sc, i, cov);
                if (sc.shs) load_sh_active<DEG>(sc, i, sh_quads, shv);
                have = true;
            }
            const CameraDev& cam = cams[v];
            const float* row = bv.rows + (size_t)i * GRAD_ROW;
            float gp[3] = {0.f, 0.f, 0.f}, gS[6], gndc[2];
            view_geometry_backward<true>(cam, row, p, cov, gp, gS, gndc, g);
            if (sc.shs) {
                const float gc[3] = {row[6], row[7], row[8]};
                const float d[3] = {p[0] - cam.campos[0], p[1] - cam.campos[1], p[2] - cam.campos[2]};
                const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                const float u[3] = {d[0] / len, d[1] / len, d[2] / len};
                float gsh[3 * NC], gu[3];
#pragma unroll
                for (int k = 0; k < 3 * NC; ++k) gsh[k] = 0.f;
                sh_backward<DEG>(shv, gc, u, gsh, gu);
                const float dot = u[0] * gu[0] + u[1] * gu[1] + u[2] * gu[2];
#pragma unroll
                for (int k = 0; k < 3; ++k) g[32 + k] = -(gu[k] - u[k] * dot) / len;
            }
        }
        const float tot = camera_block_sum(g, s_red);
        if (threadIdx.x < CAM_GRAD) partials[((size_t)v * gridDim.x + blockIdx.x) * CAM_GRAD + threadIdx.x] = tot;
    }
}

// The caller's outputs of up to BWD_TABLE_CHUNK views per launch (kernel arguments), any NULL = not wanted
struct CamGradChunk {
    float* view[BWD_TABLE_CHUNK];
    float* proj[BWD_TABLE_CHUNK];
    float* campos[BWD_TABLE_CHUNK];
};

// One workgroup per view of the chunk (view v0 + blockIdx.x): its n_parts partials summed, thread b taking the partials
// b, b + CAM_BLOCK, ... in order, then camera_block_sum.
__global__ __launch_bounds__(CAM_BLOCK) void camera_grad_finish_kernel(const float* __restrict__ partials, int n_parts,
                                                                       int v0, CamGradChunk out) {
    __shared__ float s_red[(CAM_BLOCK / 16) * CAM_GRAD];
    const int vl = blockIdx.x;
    const float* src = partials + (size_t)(v0 + vl) * n_parts * CAM_GRAD;
    float g[CAM_GRAD];
#pragma unroll
    for (int k = 0; k < CAM_GRAD; ++k) g[k] = 0.f;
    for (int b = threadIdx.x; b < n_parts; b += CAM_BLOCK) {
#pragma unroll
        for (int k = 0; k < CAM_GRAD; ++k) g[k] += gload(src + (size_t)b * CAM_GRAD + k);
    }
    const float tot = camera_block_sum(g, s_red);
    const int t = threadIdx.x;
    if (t < 16) {
        if (out.view[vl]) out.view[vl][t] = tot;
    } else if (t < 32) {
        if (out.proj[vl]) out.proj[vl][t - 16] = tot;
    } else if (t < CAM_GRAD) {
        if (out.campos[vl]) out.campos[vl][t - 32] = tot;
    }
}

}  // namespace pgr
