// train.hip.h -- the per-iteration kernels of a 3DGS training step that are not the rasterizer itself:
//   pgr_image_loss     fused L1 + D-SSIM over a [3,H,W] image: the value and dloss/dx in one call (three launches)
//   pgr_image_loss_masked  the same kernels against a masked target, plus an alpha term (below)
//   pgr_adam_step      torch.optim.Adam's single-tensor arithmetic for every parameter group in one launch
//   pgr_densify_stats  the densification statistics of one render (gradient norm, visit count, largest screen radius)
//
// Loss (the 3DGS training loss): loss = (1-l) mean|x-y| + l (1 - mean SSIM(x,y)), SSIM with an 11x11 Gaussian window
// (sigma 1.5, normalised), one window per channel, zero padding 5, C1 = 0.01^2, C2 = 0.03^2.  Writing the per-pixel SSIM
// as s(mu_x, mu_y, E[x^2], E[y^2], E[xy]), its derivative with respect to x at pixel q is
//     sum_p G(p-q) [A_p + 2 x_q B_p + y_q C_p],   A = ds/dmu_x (moments held), B = ds/dE[x^2], C = ds/dE[xy]
// i.e. blur(A) + 2x blur(B) + y blur(C) with the same window (symmetric, zero padded: the blur is its own adjoint).
// Pass A blurs the five moment maps of a 16x16 tile from a 26x26 halo in LDS and stores A, B, C and one partial sum per
// workgroup; pass B blurs A, B, C the same way and writes the gradient; pass C sums the partials in a fixed order
// (doubles, no atomics: the loss value is the same on every run).
//
// Masked form (pgr_image_loss_masked): with a mask m [H,W], a background bg [3] and the rendered alpha a [H,W], the target
// is y' = y m + bg (1 - m), formed where y is read (the halo load, and the gradient pass), so no [3,H,W] target is
// written; loss += lambda_a mean|a - m|, whose gradient sign(a - m) lambda_a / (H W) pass A writes, and whose sum is one
// more partial per channel-0 workgroup, reduced in pass C in a fixed order.  A NULL mask is the unmasked path unchanged.
//
// The partials are written so that x == y gives s == 1, A == 0 and 2x blur(B) + y blur(C) == 0 exactly (every term pair
// is formed by the same operations up to exact factors of two): the loss and gradient of identical images are zero.
#pragma once
#include "pgr_common.h"

namespace pgr {

constexpr int LOSS_TILE = 16;
constexpr int LOSS_R = 5;                              // window radius (11 taps)
constexpr int LOSS_HALO = LOSS_TILE + 2 * LOSS_R;      // 26
constexpr float SSIM_C1 = 0.01f * 0.01f;
constexpr float SSIM_C2 = 0.03f * 0.03f;

struct LossWindow { float w[2 * LOSS_R + 1]; };

// the masked loss target y' = y m + bg (1 - m) of one value
__device__ __forceinline__ float masked_target(float y, float m, float bg) { return fmaf(y, m, bg * (1.0f - m)); }

// loads the 26x26 halo of `src` (channel plane, zero outside the image) around the tile at (tx0, ty0); with a mask
// [H,W], the masked target of src over the background value bg
__device__ __forceinline__ void loss_load_halo(float (*dst)[LOSS_HALO + 1], const float* __restrict__ src, int H, int W,
                                               int tx0, int ty0, const float* __restrict__ mask = nullptr,
                                               float bg = 0.0f) {
    for (int i = threadIdx.x; i < LOSS_HALO * LOSS_HALO; i += blockDim.x) {
        const int r = i / LOSS_HALO, q = i - r * LOSS_HALO;
        const int gy = ty0 - LOSS_R + r, gx = tx0 - LOSS_R + q;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t o = in ? (size_t)gy * W + gx : 0;
        float v = in ? gload(src + o) : 0.0f;
        if (mask && in) v = masked_target(v, gload(mask + o), bg);
        dst[r][q] = v;
    }
}

__device__ double block_sum_256(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// grid (tiles_x, tiles_y, 3), 256 threads.  mask / bg: the masked target (NULL: y); alpha: the alpha term, summed by the
// channel-0 workgroups into partial_a[tile] (grad_alpha, if not NULL, = coef_a sign(a - m)).
__global__ __launch_bounds__(256) void loss_ssim_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                        int W, LossWindow win, float* __restrict__ mapA,
                                                        float* __restrict__ mapB, float* __restrict__ mapC,
                                                        double* __restrict__ partial, const float* __restrict__ mask,
                                                        const float* __restrict__ bg, const float* __restrict__ alpha,
                                                        float coef_a, float* __restrict__ grad_alpha,
                                                        double* __restrict__ partial_a) {
    __shared__ float sx[LOSS_HALO][LOSS_HALO + 1], sy[LOSS_HALO][LOSS_HALO + 1];
    __shared__ float hb[5][LOSS_HALO][LOSS_TILE + 1];
    __shared__ double red[256];
    const int c = blockIdx.z, tx0 = blockIdx.x * LOSS_TILE, ty0 = blockIdx.y * LOSS_TILE;
    const size_t plane = (size_t)H * W;
    loss_load_halo(sx, x + c * plane, H, W, tx0, ty0);
    loss_load_halo(sy, y + c * plane, H, W, tx0, ty0, mask, mask ? bg[c] : 0.0f);
    __syncthreads();
    // horizontal pass: 26 rows x 16 columns of the five moment maps
    for (int i = threadIdx.x; i < LOSS_HALO * LOSS_TILE; i += blockDim.x) {
        const int r = i / LOSS_TILE, q = i - r * LOSS_TILE;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * LOSS_R + 1; ++k) {
            const float a = sx[r][q + k], b = sy[r][q + k], w = win.w[k];
            m0 = fmaf(w, a, m0);
            m1 = fmaf(w, b, m1);
            m2 = fmaf(w, a * a, m2);
            m3 = fmaf(w, b * b, m3);
            m4 = fmaf(w, a * b, m4);
        }
        hb[0][r][q] = m0; hb[1][r][q] = m1; hb[2][r][q] = m2; hb[3][r][q] = m3; hb[4][r][q] = m4;
    }
    __syncthreads();
    const int ly = threadIdx.x / LOSS_TILE, lx = threadIdx.x % LOSS_TILE;
    float mu_x = 0.f, mu_y = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
    for (int k = 0; k < 2 * LOSS_R + 1; ++k) {
        const float w = win.w[k];
        mu_x = fmaf(w, hb[0][ly + k][lx], mu_x);
        mu_y = fmaf(w, hb[1][ly + k][lx], mu_y);
        exx = fmaf(w, hb[2][ly + k][lx], exx);
        eyy = fmaf(w, hb[3][ly + k][lx], eyy);
        exy = fmaf(w, hb[4][ly + k][lx], exy);
    }
    const int gy = ty0 + ly, gx = tx0 + lx;
    double s_sum = 0.0, l1_sum = 0.0;
    if (gy < H && gx < W) {
        const float sxx = exx - mu_x * mu_x, syy = eyy - mu_y * mu_y, sxy = exy - mu_x * mu_y;
        const float n1 = (2.0f * mu_x) * mu_y + SSIM_C1, d1 = (mu_x * mu_x + mu_y * mu_y) + SSIM_C1;
        const float n2 = 2.0f * sxy + SSIM_C2, d2 = (sxx + syy) + SSIM_C2;
        const float d12 = d1 * d2;
        const float s = (n1 * n2) / d12;
        const float r1 = n1 / d1;
        const float dmu = (2.0f * n2) * (mu_y * d1 - mu_x * n1) / (d1 * d12);
        const float B = -s / d2;
        const float Cc = (2.0f * r1) / d2;
        const float A = dmu + 2.0f * (mu_x * s - mu_y * r1) / d2;
        const size_t o = c * plane + (size_t)gy * W + gx;
        gstore(mapA + o, A);
        gstore(mapB + o, B);
        gstore(mapC + o, Cc);
        s_sum = (double)s;
        l1_sum = (double)fabsf(sx[ly + LOSS_R][lx + LOSS_R] - sy[ly + LOSS_R][lx + LOSS_R]);
    }
    const int bid = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const double l1_total = block_sum_256(l1_sum, red);
    __syncthreads();
    const double s_total = block_sum_256(s_sum, red);
    if (threadIdx.x == 0) {
        partial[2 * bid] = l1_total;
        partial[2 * bid + 1] = s_total;
    }
    if (alpha && c == 0) {                 // (uniform over the workgroup)
        double a_sum = 0.0;
        if (gy < H && gx < W) {
            const size_t o = (size_t)gy * W + gx;
            const float d = gload(alpha + o) - gload(mask + o);
            a_sum = (double)fabsf(d);
            if (grad_alpha) gstore(grad_alpha + o, coef_a * (d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.0f)));
        }
        __syncthreads();
        const double a_total = block_sum_256(a_sum, red);
        if (threadIdx.x == 0) partial_a[blockIdx.y * gridDim.x + blockIdx.x] = a_total;
    }
}

// grid (tiles_x, tiles_y, 3), 256 threads: grad = coef_s (blur(A) + 2x blur(B) + y blur(C)) + coef_l1 sign(x - y)
__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                        int W, LossWindow win, const float* __restrict__ mapA,
                                                        const float* __restrict__ mapB, const float* __restrict__ mapC,
                                                        float coef_s, float coef_l1, float* __restrict__ grad,
                                                        const float* __restrict__ mask, const float* __restrict__ bg) {
    __shared__ float sm[3][LOSS_HALO][LOSS_HALO + 1];
    __shared__ float hb[3][LOSS_HALO][LOSS_TILE + 1];
    const int c = blockIdx.z, tx0 = blockIdx.x * LOSS_TILE, ty0 = blockIdx.y * LOSS_TILE;
    const size_t plane = (size_t)H * W;
    loss_load_halo(sm[0], mapA + c * plane, H, W, tx0, ty0);
    loss_load_halo(sm[1], mapB + c * plane, H, W, tx0, ty0);
    loss_load_halo(sm[2], mapC + c * plane, H, W, tx0, ty0);
    __syncthreads();
    for (int i = threadIdx.x; i < LOSS_HALO * LOSS_TILE; i += blockDim.x) {
        const int r = i / LOSS_TILE, q = i - r * LOSS_TILE;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * LOSS_R + 1; ++k) {
            const float w = win.w[k];
            m0 = fmaf(w, sm[0][r][q + k], m0);
            m1 = fmaf(w, sm[1][r][q + k], m1);
            m2 = fmaf(w, sm[2][r][q + k], m2);
        }
        hb[0][r][q] = m0; hb[1][r][q] = m1; hb[2][r][q] = m2;
    }
    __syncthreads();
    const int ly = threadIdx.x / LOSS_TILE, lx = threadIdx.x % LOSS_TILE;
    const int gy = ty0 + ly, gx = tx0 + lx;
    if (gy >= H || gx >= W) return;
    float bA = 0.f, bB = 0.f, bC = 0.f;
#pragma unroll
    for (int k = 0; k < 2 * LOSS_R + 1; ++k) {
        const float w = win.w[k];
        bA = fmaf(w, hb[0][ly + k][lx], bA);
        bB = fmaf(w, hb[1][ly + k][lx], bB);
        bC = fmaf(w, hb[2][ly + k][lx], bC);
    }
    const size_t o = c * plane + (size_t)gy * W + gx;
    const float xv = gload(x + o);
    float yv = gload(y + o);
    if (mask) yv = masked_target(yv, gload(mask + (size_t)gy * W + gx), bg[c]);
    const float d = xv - yv;
    const float sgn = d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.0f);
    const float g_ssim = (bA + (2.0f * xv) * bB) + yv * bC;
    gstore(grad + o, coef_s * g_ssim + coef_l1 * sgn);
}

// one workgroup of 256: the partials in a fixed order -> out[0] loss, out[1] mean |x-y|, out[2] mean SSIM; with partial_a
// (n_a tiles) out[0] += lambda_a mean|a-m| and out_a = mean|a-m|; out_a without partial_a: 0
__global__ __launch_bounds__(256) void loss_reduce_kernel(const double* __restrict__ partial, int n_blocks, double inv_n,
                                                          double lambda, float* __restrict__ out,
                                                          const double* __restrict__ partial_a, int n_a, double inv_hw,
                                                          double lambda_a, float* __restrict__ out_a) {
    __shared__ double red[256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += blockDim.x) {
        a += partial[2 * i];
        b += partial[2 * i + 1];
    }
    const double l1 = block_sum_256(a, red) * inv_n;
    __syncthreads();
    const double ss = block_sum_256(b, red) * inv_n;
    double loss = (1.0 - lambda) * l1 + lambda * (1.0 - ss);
    double am = 0.0;
    if (partial_a) {
        double s = 0.0;
        for (int i = threadIdx.x; i < n_a; i += blockDim.x) s += partial_a[i];
        __syncthreads();
        am = block_sum_256(s, red) * inv_hw;
        loss += lambda_a * am;
    }
    if (threadIdx.x == 0) {
        out[0] = (float)loss;
        out[1] = (float)l1;
        out[2] = (float)ss;
        if (out_a) *out_a = (float)am;
    }
}

// ---- Adam -----------------------------------------------------------------------------------------------------------------
constexpr int ADAM_MAX_GROUPS = 16;                    // = PGR_ADAM_MAX_GROUPS
constexpr int ADAM_PER_THREAD = 4;
constexpr int ADAM_BLOCK_ELEMS = 256 * ADAM_PER_THREAD;

struct AdamGroupArgs {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    int64_t first_block;
    float neg_step_size;                               // (float)(-(lr / (1 - beta1^t)))
    float inv_bc2_sqrt;                                // (float)(1 / sqrt(1 - beta2^t)), the reciprocal formed in double
};
struct AdamArgs {
    AdamGroupArgs grp[ADAM_MAX_GROUPS];
    int n_groups;
    float w1;                                          // (float)(1 - beta1): exp_avg.lerp_(g, w1)
    float beta2;                                       // (float)beta2
    float w2;                                          // (float)(1 - beta2): exp_avg_sq.mul_(beta2).addcmul_(g, g, w2)
    float eps;
};

// torch's single-tensor Adam, element by element, in its order and rounding (each torch op is its own rounding step; the
// multiply-adds inside one torch op are fused, as the compiled torch kernels contract them):
//   m = lerp(m, g, w1)                  = fma(w1, g - m, m)          (|w1| < 0.5 branch of at::lerp)
//   v = v * beta2 ; v = fma(w2, g*g, v)                              (mul_, addcmul_)
//   denom = sqrt(v) * inv_bc2_sqrt + eps                             (div by a host scalar = multiply by its reciprocal)
//   p = fma(-step_size, m / denom, p)                                (addcdiv_)
__global__ __launch_bounds__(256) void adam_step_kernel(AdamArgs a) {
    int gi = 0;
    while (gi + 1 < a.n_groups && (int64_t)blockIdx.x >= a.grp[gi + 1].first_block) ++gi;
    const AdamGroupArgs& G = a.grp[gi];
    const int64_t base = ((int64_t)blockIdx.x - G.first_block) * ADAM_BLOCK_ELEMS + threadIdx.x;
#pragma unroll
    for (int k = 0; k < ADAM_PER_THREAD; ++k) {
        const int64_t i = base + (int64_t)k * 256;
        if (i >= G.n) break;
        const float g = gload(G.g + i);
        float m = gload(G.m + i), v = gload(G.v + i), p = gload(G.p + i);
        m = fmaf(a.w1, g - m, m);
        v = v * a.beta2;
        v = fmaf(a.w2, g * g, v);
        const float denom = sqrtf(v) * G.inv_bc2_sqrt + a.eps;
        p = fmaf(G.neg_step_size, m / denom, p);
        gstore(G.m + i, m);
        gstore(G.v + i, v);
        gstore(G.p + i, p);
    }
}

// ---- densification statistics -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void densify_stats_kernel(int n, const float* __restrict__ vgrad, int stride,
                                                            const int32_t* __restrict__ radii, float* __restrict__ accum,
                                                            float* __restrict__ denom, float* __restrict__ max_r) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t r = gload(radii + i);
    if (r <= 0) return;
    const float gx = gload(vgrad + (size_t)i * stride), gy = gload(vgrad + (size_t)i * stride + 1);
    gstore(accum + i, gload(accum + i) + sqrtf(fmaf(gy, gy, gx * gx)));
    gstore(denom + i, gload(denom + i) + 1.0f);
    gstore(max_r + i, fmaxf(gload(max_r + i), (float)r));
}

}  // namespace pgr
