// pointcloud.hip -- host side of the point-cloud entries of libpegasus_raster.so: 3-nearest-neighbour distances, radius
// neighbour counts, registration (correspondences, ICP sums, normals) and the ground plane by RANSAC.
// Owns its kernel headers: no other translation unit includes them (DESIGN.md "Source layout").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "host_common.h"
#include "knn.hip.h"
#include "plane.hip.h"
#include "radius.hip.h"
#include "registration.hip.h"

using namespace pgr;

// ---- 3-nearest-neighbour mean squared distance (simple_knn.distCUDA2) ---------------------------------------------
namespace {
struct KnnLayout { size_t grid, count, start, sorted, total; int target; size_t cells; };
KnnLayout knn_layout(int32_t n) {
    KnnLayout K{};
    int target = 1;
    while (target < KNN_MAX_GRID && (double)target * target * target < 0.5 * (double)n) ++target;   // ~2 points per cell
    K.target = target;
    K.cells = (size_t)target * target * target;
    Carver c;
    K.grid = c.take(sizeof(KnnGrid));
    K.count = c.take(K.cells * 4);
    K.start = c.take((K.cells + 1) * 4);
    K.sorted = c.take((size_t)(n > 0 ? n : 1) * 16);
    K.total = c.off;
    return K;
}
}  // namespace

size_t pgr_knn_workspace_bytes(int32_t n) { return n < 0 ? 0 : knn_layout(n).total; }

int32_t pgr_knn_mean_dist2(int32_t n, const float* xyz, float* out, void* workspace, size_t workspace_bytes,
                           void* stream_v) {
    if (n < 0) return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    if (!xyz || !out || !workspace) return PGR_ERR_INVALID_ARGUMENT;
    const KnnLayout K = knn_layout(n);
    if (workspace_bytes < K.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    auto* grid = ws_at<KnnGrid>(workspace, K.grid);
    auto* count = ws_at<uint32_t>(workspace, K.count);
    auto* start = ws_at<uint32_t>(workspace, K.start);
    auto* sorted = ws_at<float4>(workspace, K.sorted);
    KnnGrid init{};
    for (int a = 0; a < 3; ++a) { init.lo[a] = 0xffffffffu; init.hi[a] = 0u; }
    if (!hip_ok(hipMemcpyAsync(grid, &init, sizeof(init), hipMemcpyHostToDevice, stream), "memcpy knn grid") ||
        !hip_ok(hipMemsetAsync(count, 0, K.cells * 4, stream), "memset knn counts"))
        return PGR_ERR_LAUNCH_FAILURE;
    const int blocks = (n + 255) / 256;
    knn_bbox_kernel<<<blocks, 256, 0, stream>>>(n, xyz, grid);
    knn_grid_kernel<<<1, 1, 0, stream>>>(grid, K.target);
    knn_count_kernel<<<blocks, 256, 0, stream>>>(n, xyz, grid, count);
    knn_scan_kernel<<<1, 1024, 0, stream>>>(grid, count, start);
    // the counts become the cursors
    if (!hip_ok(hipMemcpyAsync(count, start, K.cells * 4, hipMemcpyDeviceToDevice, stream), "memcpy knn cursors"))
        return PGR_ERR_LAUNCH_FAILURE;
    knn_scatter_kernel<<<blocks, 256, 0, stream>>>(n, xyz, grid, count, sorted);
    knn_search_kernel<<<blocks, 256, 0, stream>>>(n, grid, start, sorted, out);
    return launch_status("knn launch");
}

// ---- radius neighbour counts (open3d's remove_radius_outlier; radius.hip.h) ---------------------------------------------
namespace {
struct RadiusLayout { size_t total_word, slots, begin, point_slot, sorted, total; size_t n_slots; };
RadiusLayout radius_layout(int32_t n) {
    RadiusLayout R{};
    R.n_slots = RADIUS_BLOCK;                                  // a power of two, a multiple of the block, at least 2 n
    while (R.n_slots < 2 * (size_t)(n > 0 ? n : 0)) R.n_slots *= 2;
    Carver c;
    R.total_word = c.take(sizeof(uint32_t));
    R.slots = c.take(R.n_slots * sizeof(RadiusSlot));
    R.begin = c.take(R.n_slots * sizeof(uint32_t));
    R.point_slot = c.take((size_t)(n > 0 ? n : 1) * sizeof(uint32_t));
    R.sorted = c.take((size_t)(n > 0 ? n : 1) * sizeof(float4));
    R.total = c.off;
    return R;
}
struct RadiusGrid { uint32_t* total; RadiusSlot* slots; uint32_t* begin; uint32_t* point_slot; float4* sorted; uint32_t mask; };
RadiusGrid radius_grid(const RadiusLayout& R, void* ws) {
    return RadiusGrid{ws_at<uint32_t>(ws, R.total_word), ws_at<RadiusSlot>(ws, R.slots), ws_at<uint32_t>(ws, R.begin),
                      ws_at<uint32_t>(ws, R.point_slot), ws_at<float4>(ws, R.sorted), (uint32_t)(R.n_slots - 1)};
}
// files the n points of `xyz` into the grid (what every entry over a grid starts with); afterwards begin[] holds the ends
bool radius_grid_build(int32_t n, const float* xyz, double inv_h, const RadiusLayout& R, const RadiusGrid& G, hipStream_t stream) {
    // the running total and the table lie one behind the other: one memset
    if (!hip_ok(hipMemsetAsync(G.total, 0, R.begin - R.total_word, stream), "memset radius table")) return false;
    const int blocks = (n + RADIUS_BLOCK - 1) / RADIUS_BLOCK;
    radius_insert_kernel<<<blocks, RADIUS_BLOCK, 0, stream>>>(n, xyz, inv_h, G.slots, G.mask, G.point_slot);
    radius_ranges_kernel<<<(unsigned)(R.n_slots / RADIUS_BLOCK), RADIUS_BLOCK, 0, stream>>>(G.slots, G.begin, G.total);
    radius_scatter_kernel<<<blocks, RADIUS_BLOCK, 0, stream>>>(n, xyz, G.point_slot, G.begin, G.sorted);
    return true;
}
}  // namespace

size_t pgr_radius_count_workspace_bytes(int32_t n) { return n < 0 ? 0 : radius_layout(n).total; }

int32_t pgr_radius_count(int32_t n, const float* xyz, double radius, int32_t cap, int32_t* counts, void* workspace,
                         size_t workspace_bytes, void* stream_v) {
    if (n < 0 || cap < 1 || !std::isfinite(radius) || !(radius > 0.0)) return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    if (!xyz || !counts || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    const RadiusLayout R = radius_layout(n);
    if (workspace_bytes < R.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    const RadiusGrid G = radius_grid(R, workspace);
    const double inv_h = 1.0 / (radius * RADIUS_CELL_MARGIN), r2 = radius * radius;
    if (!radius_grid_build(n, xyz, inv_h, R, G, stream)) return PGR_ERR_LAUNCH_FAILURE;
    radius_count_kernel<<<(n + RADIUS_BLOCK - 1) / RADIUS_BLOCK, RADIUS_BLOCK, 0, stream>>>(n, G.sorted, G.slots, G.begin, G.mask,
                                                                                          inv_h, r2, cap, counts);
    return launch_status("radius count launch");
}

// ---- registration: correspondences, ICP sums, normals by radius (registration.hip.h) --------------------------------------
namespace {
bool distance_ok(double d) { return std::isfinite(d) && d > 0.0; }
// the 3x4 of a row-major 4x4 (the last row is not read); false for NULL or a value that is not finite
bool reg_pose(const double* T, RegPose& P) {
    if (!T) return false;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P.r[3 * r + c] = T[4 * r + c];
        P.t[r] = T[4 * r + 3];
    }
    for (double v : P.r) if (!std::isfinite(v)) return false;
    for (double v : P.t) if (!std::isfinite(v)) return false;
    return true;
}
int32_t reg_blocks(int32_t n) { return (n + REG_BLOCK - 1) / REG_BLOCK; }
// the posed source as float32 in front of a grid's layout
struct OrderLayout { size_t posed, grid, total; };
OrderLayout order_layout(int32_t n) {
    Carver c;
    OrderLayout L{};
    L.posed = c.take((size_t)(n > 0 ? n : 1) * 3 * sizeof(float));
    L.grid = c.off;
    L.total = L.grid + radius_layout(n).total;
    return L;
}
}  // namespace

size_t pgr_nn_grid_build_workspace_bytes(int32_t n_target) { return n_target < 0 ? 0 : radius_layout(n_target).total; }

int32_t pgr_nn_grid_build(int32_t n_target, const float* target, double max_distance, void* workspace, size_t workspace_bytes,
                          void* stream_v) {
    if (n_target < 0 || !distance_ok(max_distance)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_target == 0) return PGR_OK;
    if (!target || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    const RadiusLayout R = radius_layout(n_target);
    if (workspace_bytes < R.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    if (!radius_grid_build(n_target, target, 1.0 / (max_distance * RADIUS_CELL_MARGIN), R, radius_grid(R, workspace), stream))
        return PGR_ERR_LAUNCH_FAILURE;
    return launch_status("nn grid launch");
}

size_t pgr_nn_source_order_workspace_bytes(int32_t n_source) { return n_source < 0 ? 0 : order_layout(n_source).total; }

int32_t pgr_nn_source_order(int32_t n_source, const float* source, const double* transformation, double max_distance,
                            int32_t* order, void* workspace, size_t workspace_bytes, void* stream_v) {
    RegPose P;
    if (n_source < 0 || !distance_ok(max_distance) || !reg_pose(transformation, P)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_source == 0) return PGR_OK;
    if (!source || !order || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    const OrderLayout L = order_layout(n_source);
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    char* ws = static_cast<char*>(workspace);
    auto* posed = ws_at<float>(ws, L.posed);
    const RadiusLayout R = radius_layout(n_source);
    const RadiusGrid G = radius_grid(R, ws + L.grid);
    registration_pose_kernel<<<reg_blocks(n_source), REG_BLOCK, 0, stream>>>(n_source, source, P, posed);
    if (!radius_grid_build(n_source, posed, 1.0 / (max_distance * RADIUS_CELL_MARGIN), R, G, stream)) return PGR_ERR_LAUNCH_FAILURE;
    registration_order_kernel<<<reg_blocks(n_source), REG_BLOCK, 0, stream>>>(n_source, G.sorted, order);
    return launch_status("nn source order launch");
}

int32_t pgr_nn_correspond(int32_t n_source, const float* source, const int32_t* order, const double* transformation,
                          int32_t n_target, double max_distance, const void* grid, size_t grid_bytes, int32_t* index,
                          double* d2, void* stream_v) {
    RegPose P;
    if (n_source < 0 || n_target < 0 || !distance_ok(max_distance) || !reg_pose(transformation, P)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_source == 0) return PGR_OK;
    if (!source || !index || !d2) return PGR_ERR_INVALID_ARGUMENT;
    const RadiusLayout R = radius_layout(n_target);
    RadiusGrid G{};
    if (n_target > 0) {
        if (!grid || !workspace_aligned_16(grid)) return PGR_ERR_INVALID_ARGUMENT;
        if (grid_bytes < R.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
        G = radius_grid(R, const_cast<void*>(grid));
    }
    registration_correspond_kernel<<<reg_blocks(n_source), REG_BLOCK, 0, as_stream(stream_v)>>>(
        n_source, source, order, P, n_target, G.sorted, G.slots, G.begin, G.mask, 1.0 / (max_distance * RADIUS_CELL_MARGIN),
        max_distance * max_distance, index, d2);
    return launch_status("nn correspond launch");
}

size_t pgr_icp_sums_workspace_bytes(int32_t n_source) {
    return n_source < 0 ? 0 : align_up((size_t)std::max(reg_blocks(n_source), 1) * REG_SUMS * sizeof(double));
}

int32_t pgr_icp_sums(int32_t n_source, const float* source, const double* transformation, const int32_t* index,
                     const double* d2, int32_t n_target, const float* target, const double* target_normals, double* sums,
                     void* workspace, size_t workspace_bytes, void* stream_v) {
    RegPose P;
    if (n_source < 0 || n_target < 0 || !reg_pose(transformation, P) || !sums) return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = as_stream(stream_v);
    if (n_source == 0 || n_target == 0)                          // nothing corresponds: every sum is 0
        return hip_ok(hipMemsetAsync(sums, 0, REG_SUMS * sizeof(double), stream), "memset icp sums") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
    if (!source || !index || !d2 || !target || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < pgr_icp_sums_workspace_bytes(n_source)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    auto* partials = static_cast<double*>(workspace);
    const int32_t blocks = reg_blocks(n_source);
    registration_sums_kernel<<<blocks, REG_BLOCK, 0, stream>>>(n_source, source, P, index, d2, n_target, target, target_normals,
                                                               partials);
    registration_sums_final_kernel<<<1, REG_FINAL_BLOCK, 0, stream>>>(blocks, partials, sums);
    return launch_status("icp sums launch");
}

size_t pgr_radius_normals_workspace_bytes(int32_t n) { return n < 0 ? 0 : radius_layout(n).total; }

int32_t pgr_radius_normals(int32_t n, const float* xyz, double radius, double* normals, int32_t* counts, void* workspace,
                           size_t workspace_bytes, void* stream_v) {
    if (n < 0 || !distance_ok(radius)) return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    if (!xyz || !normals || !counts || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    const RadiusLayout R = radius_layout(n);
    if (workspace_bytes < R.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    const RadiusGrid G = radius_grid(R, workspace);
    const double inv_h = 1.0 / (radius * RADIUS_CELL_MARGIN);
    if (!radius_grid_build(n, xyz, inv_h, R, G, stream)) return PGR_ERR_LAUNCH_FAILURE;
    registration_normals_kernel<<<reg_blocks(n), REG_BLOCK, 0, stream>>>(n, G.sorted, G.slots, G.begin, G.mask, inv_h,
                                                                        radius * radius, normals, counts);
    return launch_status("radius normals launch");
}

// ---- ground plane by RANSAC: hypotheses, scores, the inlier pass (plane.hip.h) --------------------------------------------
namespace {
static_assert(PLANE_TILE == PGR_PLANE_TILE, "include/pegasus_raster.h names the tile of plane_score_kernel");
int32_t plane_blocks(int32_t n, int32_t per_block) { return std::max((int32_t)(((int64_t)n + per_block - 1) / per_block), 1); }
// the workgroups' partials of pgr_plane_score: the sums [blocks, n_hyp] in front of the counts [blocks, n_hyp]
struct PlaneScoreLayout { size_t sumsq, count, total; int32_t blocks; };
PlaneScoreLayout plane_score_layout(int32_t n, int32_t n_hyp) {
    PlaneScoreLayout L{};
    L.blocks = plane_blocks(n, PLANE_TILE);
    const size_t cells = (size_t)L.blocks * (size_t)std::max(n_hyp, 1);
    Carver c;
    L.sumsq = c.take(cells * sizeof(double));
    L.count = c.take(cells * sizeof(int32_t));
    L.total = c.off;
    return L;
}
}  // namespace

int32_t pgr_plane_hypotheses(int32_t n, const float* xyz, int32_t n_hyp, const int32_t* triples, double* planes, uint8_t* valid,
                             void* stream_v) {
    if (n < 0 || n_hyp < 0) return PGR_ERR_INVALID_ARGUMENT;
    if (n_hyp == 0) return PGR_OK;
    if (!triples || !planes || !valid || (n > 0 && !xyz)) return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = as_stream(stream_v);
    if (n == 0) {                                                // no row is inside [0, 0): every hypothesis is invalid
        if (!hip_ok(hipMemsetAsync(planes, 0, (size_t)n_hyp * 4 * sizeof(double), stream), "memset planes") ||
            !hip_ok(hipMemsetAsync(valid, 0, (size_t)n_hyp, stream), "memset plane validity"))
            return PGR_ERR_LAUNCH_FAILURE;
        return PGR_OK;
    }
    plane_hypotheses_kernel<<<plane_blocks(n_hyp, PLANE_BLOCK), PLANE_BLOCK, 0, stream>>>(n, xyz, n_hyp, triples, planes, valid);
    return launch_status("plane hypotheses launch");
}

size_t pgr_plane_score_workspace_bytes(int32_t n, int32_t n_hyp) {
    return n < 0 || n_hyp < 0 ? 0 : plane_score_layout(n, n_hyp).total;
}

int32_t pgr_plane_score(int32_t n, const float* xyz, int32_t n_hyp, const double* planes, double threshold, int32_t* counts,
                        double* sumsq, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (n < 0 || n_hyp < 0 || !distance_ok(threshold)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_hyp == 0) return PGR_OK;
    if (!counts || !sumsq) return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = as_stream(stream_v);
    if (n == 0) {                                                // no point: every score is 0
        if (!hip_ok(hipMemsetAsync(counts, 0, (size_t)n_hyp * sizeof(int32_t), stream), "memset plane counts") ||
            !hip_ok(hipMemsetAsync(sumsq, 0, (size_t)n_hyp * sizeof(double), stream), "memset plane sums"))
            return PGR_ERR_LAUNCH_FAILURE;
        return PGR_OK;
    }
    if (!xyz || !planes || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    const PlaneScoreLayout L = plane_score_layout(n, n_hyp);
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    auto* part_sumsq = ws_at<double>(workspace, L.sumsq);
    auto* part_count = ws_at<int32_t>(workspace, L.count);
    // few tiles: the batches of hypotheses are spread over gridDim.y (at most PLANE_SCORE_MIN_BLOCKS groups)
    const int32_t batches = plane_blocks(n_hyp, PLANE_HYP_BATCH);
    const int32_t wanted = std::min(batches, (PLANE_SCORE_MIN_BLOCKS + L.blocks - 1) / L.blocks);
    const int32_t per_group = (batches + wanted - 1) / wanted;
    const dim3 grid((unsigned)L.blocks, (unsigned)((batches + per_group - 1) / per_group));
    plane_score_kernel<<<grid, PLANE_BLOCK, 0, stream>>>(n, xyz, n_hyp, planes, threshold, per_group, part_sumsq, part_count);
    if (int32_t rc = launch_status("plane score launch")) return rc;     // (no second pass over nothing)
    plane_score_final_kernel<<<plane_blocks(n_hyp, PLANE_BLOCK), PLANE_BLOCK, 0, stream>>>(L.blocks, n_hyp, part_sumsq, part_count,
                                                                                        counts, sumsq);
    return launch_status("plane score final launch");
}

size_t pgr_plane_inliers_workspace_bytes(int32_t n) {
    return n < 0 ? 0 : align_up((size_t)plane_blocks(n, PLANE_BLOCK) * PLANE_SUM_TERMS * sizeof(double));
}

int32_t pgr_plane_inliers(int32_t n, const float* xyz, const double* plane, const double* pivot, double threshold, uint8_t* mask,
                          double* sums, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (n < 0 || !distance_ok(threshold) || !plane || !pivot || !sums) return PGR_ERR_INVALID_ARGUMENT;
    PlaneModel P{{plane[0], plane[1], plane[2]}, plane[3], {pivot[0], pivot[1], pivot[2]}};
    for (double v : {P.n[0], P.n[1], P.n[2], P.d, P.pivot[0], P.pivot[1], P.pivot[2]})
        if (!std::isfinite(v)) return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = as_stream(stream_v);
    if (n == 0)                                                  // no point: every sum is 0
        return hip_ok(hipMemsetAsync(sums, 0, PLANE_SUM_TERMS * sizeof(double), stream), "memset plane sums") ? PGR_OK
                                                                                                                 : PGR_ERR_LAUNCH_FAILURE;
    if (!xyz || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < pgr_plane_inliers_workspace_bytes(n)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    auto* partials = static_cast<double*>(workspace);
    const int32_t blocks = plane_blocks(n, PLANE_BLOCK);
    plane_inliers_kernel<<<blocks, PLANE_BLOCK, 0, stream>>>(n, xyz, P, threshold, mask, partials);
    if (int32_t rc = launch_status("plane inliers launch")) return rc;
    plane_inliers_final_kernel<<<1, PLANE_FINAL_BLOCK, 0, stream>>>(blocks, partials, sums);
    return launch_status("plane inliers final launch");
}
