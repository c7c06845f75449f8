// train.hip -- host side of the training entries of libpegasus_raster.so: fused image loss, Adam, densification statistics.
// Owns its kernel headers: no other translation unit includes them (DESIGN.md "Source layout").
#include <hip/hip_runtime.h>

#include <cmath>

#include "host_common.h"
#include "train.hip.h"

using namespace pgr;

// ---- training step: fused L1 + D-SSIM loss, Adam over all parameter groups, densification statistics (train.hip.h) ------
namespace {
struct LossLayout { size_t a, b, c, partial, total, partial_a, total_masked; int tiles_x, tiles_y; };
LossLayout loss_layout(int32_t height, int32_t width) {
    LossLayout L{};
    L.tiles_x = (width + LOSS_TILE - 1) / LOSS_TILE;
    L.tiles_y = (height + LOSS_TILE - 1) / LOSS_TILE;
    const size_t map = (size_t)3 * height * width * sizeof(float);
    Carver c;
    L.a = c.take(map);
    L.b = c.take(map);
    L.c = c.take(map);
    L.partial = c.take((size_t)3 * L.tiles_x * L.tiles_y * 2 * sizeof(double));
    L.total = c.off;
    L.partial_a = c.take((size_t)L.tiles_x * L.tiles_y * sizeof(double));      // the masked loss's alpha partials
    L.total_masked = c.off;
    return L;
}
LossWindow ssim_window() {
    LossWindow w{};
    double g[2 * LOSS_R + 1], sum = 0.0;
    for (int k = 0; k <= 2 * LOSS_R; ++k) { g[k] = std::exp(-(double)((k - LOSS_R) * (k - LOSS_R)) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
    for (int k = 0; k <= 2 * LOSS_R; ++k) w.w[k] = (float)(g[k] / sum);
    return w;
}
// the three launches of pgr_image_loss / pgr_image_loss_masked (arguments checked by the callers)
int32_t image_loss_launch(const LossLayout& L, const float* x, const float* y, const float* mask, const float* bg,
                          const float* alpha, int32_t height, int32_t width, double lambda_dssim, double lambda_alpha,
                          float* out3, float* out_a, float* grad, float* grad_alpha, void* workspace,
                          hipStream_t stream);
}  // namespace

size_t pgr_image_loss_workspace_bytes(int32_t height, int32_t width) {
    return (height <= 0 || width <= 0) ? 0 : loss_layout(height, width).total;
}

int32_t pgr_image_loss(const float* x, const float* y, int32_t height, int32_t width, double lambda_dssim, float* out3,
                       float* grad, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (height <= 0 || width <= 0 || !x || !y || !out3 || !workspace) return PGR_ERR_INVALID_ARGUMENT;
    if (!(lambda_dssim >= 0.0 && lambda_dssim <= 1.0)) return PGR_ERR_INVALID_ARGUMENT;
    if ((int64_t)height * width > (int64_t)1 << 28) return PGR_ERR_INVALID_ARGUMENT;
    const LossLayout L = loss_layout(height, width);
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    return image_loss_launch(L, x, y, nullptr, nullptr, nullptr, height, width, lambda_dssim, 0.0, out3, nullptr, grad,
                             nullptr, workspace, as_stream(stream_v));
}

size_t pgr_image_loss_masked_workspace_bytes(int32_t height, int32_t width) {
    return (height <= 0 || width <= 0) ? 0 : loss_layout(height, width).total_masked;
}

int32_t pgr_image_loss_masked(const float* x, const float* y, const float* mask, const float* bg, const float* alpha,
                              int32_t height, int32_t width, double lambda_dssim, double lambda_alpha, float* out4,
                              float* grad, float* grad_alpha, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (height <= 0 || width <= 0 || !x || !y || !out4 || !workspace) return PGR_ERR_INVALID_ARGUMENT;
    if (!(lambda_dssim >= 0.0 && lambda_dssim <= 1.0) || !(lambda_alpha >= 0.0)) return PGR_ERR_INVALID_ARGUMENT;
    if ((int64_t)height * width > (int64_t)1 << 28) return PGR_ERR_INVALID_ARGUMENT;
    if ((mask && !bg) || (alpha && !mask) || (lambda_alpha > 0.0 && !alpha) || (grad_alpha && !alpha))
        return PGR_ERR_INVALID_ARGUMENT;
    const LossLayout L = loss_layout(height, width);
    if (workspace_bytes < L.total_masked) return PGR_ERR_WORKSPACE_TOO_SMALL;
    return image_loss_launch(L, x, y, mask, bg, alpha, height, width, lambda_dssim, lambda_alpha, out4, out4 + 3, grad,
                             grad_alpha, workspace, as_stream(stream_v));
}

namespace {
int32_t image_loss_launch(const LossLayout& L, const float* x, const float* y, const float* mask, const float* bg,
                          const float* alpha, int32_t height, int32_t width, double lambda_dssim, double lambda_alpha,
                          float* out3, float* out_a, float* grad, float* grad_alpha, void* workspace,
                          hipStream_t stream) {
    auto* A = ws_at<float>(workspace, L.a);
    auto* B = ws_at<float>(workspace, L.b);
    auto* Cm = ws_at<float>(workspace, L.c);
    auto* partial = ws_at<double>(workspace, L.partial);
    const LossWindow win = ssim_window();
    const dim3 grid(L.tiles_x, L.tiles_y, 3);
    const int n_blocks = 3 * L.tiles_x * L.tiles_y;
    const double n_values = 3.0 * (double)height * (double)width;
    const double n_pix = (double)height * (double)width;
    auto* partial_a = alpha ? ws_at<double>(workspace, L.partial_a) : nullptr;
    loss_ssim_kernel<<<grid, 256, 0, stream>>>(x, y, height, width, win, A, B, Cm, partial, mask, bg, alpha,
                                               (float)(lambda_alpha / n_pix), grad_alpha, partial_a);
    if (grad)
        loss_grad_kernel<<<grid, 256, 0, stream>>>(x, y, height, width, win, A, B, Cm, (float)(-lambda_dssim / n_values),
                                                   (float)((1.0 - lambda_dssim) / n_values), grad, mask, bg);
    loss_reduce_kernel<<<1, 256, 0, stream>>>(partial, n_blocks, 1.0 / n_values, lambda_dssim, out3, partial_a,
                                              L.tiles_x * L.tiles_y, 1.0 / n_pix, lambda_alpha, out_a);
    return launch_status("image loss launch");
}
}  // namespace

int32_t pgr_adam_step(const PgrAdamGroup* groups, int32_t n_groups, double beta1, double beta2, double eps,
                      void* stream_v) {
    if (n_groups < 0 || n_groups > PGR_ADAM_MAX_GROUPS || (n_groups > 0 && !groups)) return PGR_ERR_INVALID_ARGUMENT;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return PGR_ERR_INVALID_ARGUMENT;
    AdamArgs a{};
    int64_t blocks = 0;
    for (int32_t k = 0; k < n_groups; ++k) {
        const PgrAdamGroup& G = groups[k];
        if (G.n < 0 || G.step < 1 || !(G.lr >= 0.0)) return PGR_ERR_INVALID_ARGUMENT;
        if (G.n > 0 && (!G.param || !G.grad || !G.exp_avg || !G.exp_avg_sq)) return PGR_ERR_INVALID_ARGUMENT;
        if (G.n == 0) continue;                        // nothing to launch for an empty group
        // the scalars exactly as torch.optim.Adam forms them on the host: double arithmetic, then one float rounding each
        const double bc1 = 1.0 - std::pow(beta1, (double)G.step);
        const double bc2 = 1.0 - std::pow(beta2, (double)G.step);
        AdamGroupArgs& d = a.grp[a.n_groups++];
        d.p = G.param; d.g = G.grad; d.m = G.exp_avg; d.v = G.exp_avg_sq; d.n = G.n;
        d.first_block = blocks;
        d.neg_step_size = (float)(-(G.lr / bc1));
        d.inv_bc2_sqrt = (float)(1.0 / std::pow(bc2, 0.5));   // (torch: reciprocal of the host scalar in double)
        blocks += (G.n + ADAM_BLOCK_ELEMS - 1) / ADAM_BLOCK_ELEMS;
    }
    if (blocks == 0) return PGR_OK;
    if (blocks > 0x7fffffff) return PGR_ERR_INVALID_ARGUMENT;
    a.w1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.w2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    adam_step_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream_v)>>>(a);
    return launch_status("adam launch");
}

int32_t pgr_densify_stats(int32_t n, const float* viewspace_grad, int32_t grad_stride, const int32_t* radii,
                          float* grad_accum, float* denom, float* max_radii2d, void* stream_v) {
    if (n < 0 || grad_stride < 2) return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    if (!viewspace_grad || !radii || !grad_accum || !denom || !max_radii2d) return PGR_ERR_INVALID_ARGUMENT;
    densify_stats_kernel<<<(n + 255) / 256, 256, 0, as_stream(stream_v)>>>(
        n, viewspace_grad, grad_stride, radii, grad_accum, denom, max_radii2d);
    return launch_status("densify stats launch");
}
