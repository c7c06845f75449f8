// eval.hip -- host side of the evaluation entries of libpegasus_raster.so: BOP pose errors, oriented boxes and diameters,
// mask run-length encoding and COCO scores.
// Owns its kernel headers: no other translation unit includes them (DESIGN.md "Source layout").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "cocoeval.hip.h"
#include "cocorle.hip.h"
#include "host_common.h"
#include "obb.hip.h"
#include "poseerr.hip.h"

using namespace pgr;

// ---- BOP pose errors (poseerr.hip.h) -----------------------------------------------------------------------------------
namespace {
bool pose_vertices_ok(const float* vertices, int64_t n_vertices, int32_t n_jobs, const PgrPoseErrorJob* jobs) {
    if (n_jobs < 0 || n_vertices < 0 || (n_jobs > 0 && (!jobs || !vertices))) return false;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrPoseErrorJob& j = jobs[k];
        if (j.vertex_first < 0 || j.vertex_count <= 0 || (int64_t)j.vertex_first + j.vertex_count > n_vertices) return false;
    }
    return true;
}
int64_t adi_groups(const PgrPoseErrorJob& j) { return ((int64_t)j.vertex_count + ADI_TILE - 1) / ADI_TILE; }
// pgr_pose_adi's workspace: one float64 partial sum per tile of queries, the jobs' tiles back to back
struct AdiLayout { size_t partials, total; };
AdiLayout adi_layout(int32_t n_jobs, const PgrPoseErrorJob* jobs) {
    AdiLayout L{};
    if (n_jobs <= 0 || !jobs) return L;
    int64_t groups = 0;
    for (int32_t k = 0; k < n_jobs; ++k) {
        if (jobs[k].vertex_count <= 0) return L;
        groups += adi_groups(jobs[k]);
    }
    if (groups > INT32_MAX) return L;
    Carver c;
    L.partials = c.take((size_t)groups * sizeof(double));
    L.total = c.off;
    return L;
}
}  // namespace

int32_t pgr_pose_errors(const float* vertices, int64_t n_vertices, const double* syms, int64_t n_syms, int32_t n_jobs,
                        const PgrPoseErrorJob* jobs, float* errors, double* re_te, void* stream_v) {
    if (!pose_vertices_ok(vertices, n_vertices, n_jobs, jobs) || n_syms < 0 || (n_jobs > 0 && (!syms || !errors)))
        return PGR_ERR_INVALID_ARGUMENT;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrPoseErrorJob& j = jobs[k];
        if (j.sym_first < 0 || j.sym_count <= 0 || (int64_t)j.sym_first + j.sym_count > n_syms) return PGR_ERR_INVALID_ARGUMENT;
    }
    if (n_jobs == 0) return PGR_OK;
    hipStream_t stream = as_stream(stream_v);
    pose_init_kernel<<<(n_jobs * PGR_POSE_ERRORS + 255) / 256, 256, 0, stream>>>(errors, n_jobs);
    for (int32_t k0 = 0; k0 < n_jobs; k0 += PERR_JOBS_PER_LAUNCH) {
        PoseErrJobTable T{};
        T.count = std::min(PERR_JOBS_PER_LAUNCH, n_jobs - k0);
        T.first = k0;
        uint32_t blocks = 0;
        for (int32_t k = 0; k < T.count; ++k) {
            const PgrPoseErrorJob& j = jobs[k0 + k];
            PoseErrJobDev& d = T.job[k];
            d.v0 = j.vertex_first; d.nv = j.vertex_count; d.s0 = j.sym_first; d.ns = j.sym_count;
            std::memcpy(d.Re, j.R_est, sizeof(d.Re));
            std::memcpy(d.te, j.t_est, sizeof(d.te));
            std::memcpy(d.Rg, j.R_gt, sizeof(d.Rg));
            std::memcpy(d.tg, j.t_gt, sizeof(d.tg));
            d.fx = (float)j.fx; d.fy = (float)j.fy; d.cx = (float)j.cx; d.cy = (float)j.cy;
            d.block0 = blocks;
            blocks += (uint32_t)((j.sym_count + PERR_SYM_CHUNK - 1) / PERR_SYM_CHUNK);
        }
        pose_errors_kernel<<<blocks, PERR_THREADS, 0, stream>>>(T, vertices, syms, errors, re_te);
    }
    return launch_status("pose_errors launch");
}

size_t pgr_pose_adi_workspace_bytes(int32_t n_jobs, const PgrPoseErrorJob* jobs) { return adi_layout(n_jobs, jobs).total; }

int32_t pgr_pose_adi(const float* vertices, int64_t n_vertices, int32_t n_jobs, const PgrPoseErrorJob* jobs, float* adi,
                     void* workspace, size_t workspace_bytes, void* stream_v) {
    if (!pose_vertices_ok(vertices, n_vertices, n_jobs, jobs) || (n_jobs > 0 && !adi)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return PGR_OK;
    const AdiLayout L = adi_layout(n_jobs, jobs);
    if (!L.total) return PGR_ERR_INVALID_ARGUMENT;
    if (!workspace || workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    auto* partials = ws_at<double>(workspace, L.partials);
    uint32_t part = 0;
    for (int32_t k0 = 0; k0 < n_jobs; k0 += ADI_JOBS_PER_LAUNCH) {
        AdiJobTable T{};
        T.count = std::min(ADI_JOBS_PER_LAUNCH, n_jobs - k0);
        T.first = k0;
        uint32_t blocks = 0;
        for (int32_t k = 0; k < T.count; ++k) {
            const PgrPoseErrorJob& j = jobs[k0 + k];
            AdiJobDev& d = T.job[k];
            d.v0 = j.vertex_first; d.nv = j.vertex_count;
            const double* Re = j.R_est;
            const double* Rg = j.R_gt;
            const bool same_R = std::memcmp(Re, Rg, sizeof(j.R_est)) == 0;    // R^T R of a rotation: the identity, exactly
            const double dt[3] = {j.t_gt[0] - j.t_est[0], j.t_gt[1] - j.t_est[1], j.t_gt[2] - j.t_est[2]};
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c)
                    d.M[3 * r + c] = same_R ? (r == c ? 1.f : 0.f)
                                            : (float)((Re[r] * Rg[c] + Re[3 + r] * Rg[3 + c]) + Re[6 + r] * Rg[6 + c]);
                d.c[r] = (float)((Re[r] * dt[0] + Re[3 + r] * dt[1]) + Re[6 + r] * dt[2]);
            }
            d.block0 = blocks;
            d.part0 = part;
            const uint32_t g = (uint32_t)adi_groups(j);
            blocks += g;
            part += g;
        }
        pose_adi_kernel<<<blocks, ADI_TILE, 0, stream>>>(T, vertices, partials);
        pose_adi_mean_kernel<<<1, 64, 0, stream>>>(T, partials, adi);
    }
    return launch_status("pose_adi launch");
}

// ---- minimal oriented boxes and diameters (obb.hip.h) --------------------------------------------------------------------
namespace {
// how a job's points are cut: `splits` chunks of `chunk` points (whole tiles), none of them empty
struct ObbCut { uint32_t splits, chunk; };
ObbCut obb_cut(const PgrObbJob& j) {
    const int64_t tri_blocks = ((int64_t)j.tri_count + OBB_TF - 1) / OBB_TF;
    const int64_t tiles = ((int64_t)j.point_count + OBB_TP - 1) / OBB_TP;
    const int64_t want = std::min(tiles, std::max<int64_t>(1, (OBB_TARGET_BLOCKS + tri_blocks - 1) / tri_blocks));
    const int64_t chunk = (tiles + want - 1) / want * OBB_TP;
    return ObbCut{(uint32_t)(((int64_t)j.point_count + chunk - 1) / chunk), (uint32_t)chunk};
}
// the j range of a block of points is cut into at most this many chunks (diameter_partial_kernel sizes them per block)
uint32_t diameter_splits(const PgrObbJob& j) {
    const int64_t blocks = ((int64_t)j.point_count + DIAM_TILE - 1) / DIAM_TILE;
    return (uint32_t)std::min(blocks, std::max<int64_t>(1, (OBB_TARGET_BLOCKS + blocks - 1) / blocks));
}
bool obb_points_ok(int64_t n_points, int32_t n_jobs, const PgrObbJob* jobs) {
    if (n_jobs < 0 || n_points < 0 || (n_jobs > 0 && !jobs)) return false;
    for (int32_t k = 0; k < n_jobs; ++k)
        if (jobs[k].point_first < 0 || jobs[k].point_count < 0 || (int64_t)jobs[k].point_first + jobs[k].point_count > n_points)
            return false;
    return true;
}
}  // namespace

// float64 partial extremes [chunk][6][triangle], the jobs one behind the other
size_t pgr_obb_candidates_workspace_bytes(int32_t n_jobs, const PgrObbJob* jobs) {
    if (n_jobs <= 0 || !jobs) return 0;
    size_t doubles = 0;
    for (int32_t k = 0; k < n_jobs; ++k) {
        if (jobs[k].tri_count < 0 || jobs[k].point_count < 0 || (jobs[k].tri_count > 0 && jobs[k].point_count == 0)) return 0;
        if (jobs[k].tri_count > 0) doubles += (size_t)jobs[k].tri_count * 6 * obb_cut(jobs[k]).splits;
    }
    Carver c;
    c.take(doubles * sizeof(double));
    return c.off;
}

int32_t pgr_obb_candidates(const float* points, int64_t n_points, const int32_t* triangles, int64_t n_triangles,
                           const int32_t* triangles_host, int32_t n_jobs, const PgrObbJob* jobs, double* volumes,
                           int32_t* best, double* lohi, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (!obb_points_ok(n_points, n_jobs, jobs) || n_triangles < 0) return PGR_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return PGR_OK;
    if (!best || !lohi) return PGR_ERR_INVALID_ARGUMENT;
    int64_t total_tris = 0;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrObbJob& j = jobs[k];
        if (j.tri_first < 0 || j.tri_count < 0 || (int64_t)j.tri_first + j.tri_count > n_triangles) return PGR_ERR_INVALID_ARGUMENT;
        if (j.tri_count > 0 && j.point_count == 0) return PGR_ERR_INVALID_ARGUMENT;       // no index can be valid
        total_tris += j.tri_count;
        if (triangles_host)
            for (int64_t e = 3 * (int64_t)j.tri_first; e < 3 * ((int64_t)j.tri_first + j.tri_count); ++e)
                if (triangles_host[e] < 0 || triangles_host[e] >= j.point_count) return PGR_ERR_INVALID_ARGUMENT;
    }
    if (total_tris > 0 && (!points || !triangles || !volumes)) return PGR_ERR_INVALID_ARGUMENT;
    const size_t need = pgr_obb_candidates_workspace_bytes(n_jobs, jobs);
    if (total_tris > 0 && (!workspace || !workspace_aligned_16(workspace))) return PGR_ERR_INVALID_ARGUMENT;
    if (total_tris > 0 && workspace_bytes < need) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    auto* partials = static_cast<double*>(workspace);
    uint64_t part = 0;
    for (int32_t k0 = 0; k0 < n_jobs; k0 += OBB_JOBS_PER_LAUNCH) {
        ObbJobTable T{};
        T.count = std::min(OBB_JOBS_PER_LAUNCH, n_jobs - k0);
        T.first = k0;
        uint32_t blocks = 0, mblocks = 0;
        for (int32_t k = 0; k < T.count; ++k) {
            const PgrObbJob& j = jobs[k0 + k];
            ObbJobDev& d = T.job[k];
            d.p0 = j.point_first; d.np = j.point_count; d.t0 = j.tri_first; d.nt = j.tri_count;
            d.block0 = blocks; d.mblock0 = mblocks; d.part0 = part;
            d.splits = 1; d.chunk = OBB_TP;
            if (j.tri_count == 0) continue;
            const ObbCut cut = obb_cut(j);
            d.splits = cut.splits; d.chunk = cut.chunk;
            const uint32_t tri_blocks = (uint32_t)(((int64_t)j.tri_count + OBB_TF - 1) / OBB_TF);
            blocks += tri_blocks * cut.splits;
            mblocks += tri_blocks;
            part += (uint64_t)j.tri_count * 6 * cut.splits;
        }
        if (blocks) {
            obb_partial_kernel<<<blocks, OBB_TF, 0, stream>>>(T, points, triangles, partials);
            obb_merge_kernel<<<mblocks, OBB_TF, 0, stream>>>(T, partials, volumes);
        }
        obb_argmin_kernel<<<(unsigned)T.count, 256, 0, stream>>>(T, partials, volumes, best, lohi);
    }
    return launch_status("obb_candidates launch");
}

// one DiamPartial per (block of points, chunk), the jobs one behind the other
size_t pgr_point_diameter_workspace_bytes(int32_t n_jobs, const PgrObbJob* jobs) {
    if (n_jobs <= 0 || !jobs) return 0;
    size_t records = 0;
    for (int32_t k = 0; k < n_jobs; ++k) {
        if (jobs[k].point_count < 0) return 0;
        if (jobs[k].point_count > 0)
            records += (size_t)(((int64_t)jobs[k].point_count + DIAM_TILE - 1) / DIAM_TILE) * diameter_splits(jobs[k]);
    }
    Carver c;
    c.take(records * sizeof(DiamPartial));
    return c.off;
}

int32_t pgr_point_diameter(const float* points, int64_t n_points, int32_t n_jobs, const PgrObbJob* jobs, int32_t* pair,
                           double* d2, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (!obb_points_ok(n_points, n_jobs, jobs)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return PGR_OK;
    if (!pair || !d2) return PGR_ERR_INVALID_ARGUMENT;
    int64_t total_points = 0;
    for (int32_t k = 0; k < n_jobs; ++k) total_points += jobs[k].point_count;
    if (total_points > 0 && (!points || !workspace || !workspace_aligned_16(workspace))) return PGR_ERR_INVALID_ARGUMENT;
    if (total_points > 0 && workspace_bytes < pgr_point_diameter_workspace_bytes(n_jobs, jobs)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    auto* partials = static_cast<DiamPartial*>(workspace);
    uint64_t part = 0;
    for (int32_t k0 = 0; k0 < n_jobs; k0 += OBB_JOBS_PER_LAUNCH) {
        ObbJobTable T{};
        T.count = std::min(OBB_JOBS_PER_LAUNCH, n_jobs - k0);
        T.first = k0;
        uint32_t blocks = 0;
        for (int32_t k = 0; k < T.count; ++k) {
            const PgrObbJob& j = jobs[k0 + k];
            ObbJobDev& d = T.job[k];
            d.p0 = j.point_first; d.np = j.point_count;
            d.block0 = blocks; d.part0 = part;
            d.splits = j.point_count > 0 ? diameter_splits(j) : 1;
            const uint32_t n = (uint32_t)(((int64_t)j.point_count + DIAM_TILE - 1) / DIAM_TILE) * d.splits;
            blocks += n;
            part += n;
        }
        if (blocks) diameter_partial_kernel<<<blocks, DIAM_TILE, 0, stream>>>(T, points, partials);
        diameter_reduce_kernel<<<(unsigned)T.count, 256, 0, stream>>>(T, partials, pair, d2);
    }
    return launch_status("point_diameter launch");
}

// ---- COCO annotations: mask run-length encoding, decoding, overlap counts (cocorle.hip.h) -------------------------------
namespace {
constexpr int32_t RLE_MAX_SIDE = 8192;
struct RleLayout { size_t planes, columns, total; int S, Wp, col_tiles, row_groups, col_blocks; int64_t plane_blocks, column_blocks; };
bool rle_shape_ok(int64_t n_masks, int32_t width, int32_t height) {
    return n_masks >= 1 && n_masks <= INT32_MAX && width >= 1 && width <= RLE_MAX_SIDE && height >= 1 && height <= RLE_MAX_SIDE;
}
// the encoder's workspace: the bit planes, then 16 bytes per column; launches that would not fit a grid make it invalid
RleLayout rle_layout(int32_t n_masks, int32_t width, int32_t height) {
    RleLayout L{};
    if (!rle_shape_ok(n_masks, width, height)) return L;
    L.S = (height + RLE_WORD_ROWS - 1) / RLE_WORD_ROWS;
    L.Wp = (width + 3) / 4 * 4;
    L.col_tiles = (width + RLE_TILE_COLS - 1) / RLE_TILE_COLS;
    L.row_groups = (height + RLE_BLOCK_ROWS - 1) / RLE_BLOCK_ROWS;
    L.col_blocks = (width + RLE_THREADS - 1) / RLE_THREADS;
    L.plane_blocks = (int64_t)n_masks * L.col_tiles * L.row_groups;
    L.column_blocks = (int64_t)n_masks * L.col_blocks;
    if (L.plane_blocks > MAX_GRID_BLOCKS || L.column_blocks > MAX_GRID_BLOCKS) return L;
    Carver c;
    L.planes = c.take((size_t)n_masks * L.S * L.Wp * sizeof(uint32_t));
    L.columns = c.take((size_t)n_masks * width * sizeof(RleColumn));
    L.total = c.off;
    return L;
}
}  // namespace

size_t pgr_mask_rle_workspace_bytes(int32_t n_masks, int32_t width, int32_t height) { return rle_layout(n_masks, width, height).total; }

int32_t pgr_mask_rle_count(const uint8_t* masks, int32_t n_masks, int32_t width, int32_t height, int32_t* stats, void* workspace,
                           size_t workspace_bytes, void* stream_v) {
    const RleLayout L = rle_layout(n_masks, width, height);
    if (!masks || !stats || !workspace || !workspace_aligned_16(workspace) || !L.total) return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    auto* planes = ws_at<uint32_t>(workspace, L.planes);
    auto* columns = ws_at<RleColumn>(workspace, L.columns);
    rle_planes_kernel<<<(unsigned)L.plane_blocks, RLE_THREADS, 0, stream>>>(masks, width, height, L.S, L.Wp, L.col_tiles,
                                                                            L.row_groups, planes);
    rle_columns_kernel<<<(unsigned)L.column_blocks, RLE_THREADS, 0, stream>>>(planes, width, height, L.S, L.Wp, L.col_blocks,
                                                                              columns);
    rle_scan_kernel<<<(unsigned)n_masks, RLE_THREADS, 0, stream>>>(columns, width, height, stats);
    return launch_status("mask_rle_count launch");
}

int32_t pgr_mask_rle_emit(const uint8_t* masks, int32_t n_masks, int32_t width, int32_t height, const int64_t* offsets,
                          int64_t total, int32_t* counts, int64_t capacity, const void* workspace, size_t workspace_bytes,
                          void* stream_v) {
    const RleLayout L = rle_layout(n_masks, width, height);
    if (!masks || !offsets || !counts || !workspace || !workspace_aligned_16(workspace) || !L.total) return PGR_ERR_INVALID_ARGUMENT;
    // every mask has at least one count and at most one per pixel plus one
    if (total < n_masks || total > (int64_t)n_masks * ((int64_t)width * height + 1) || capacity < total)
        return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    rle_emit_kernel<<<(unsigned)L.column_blocks, RLE_THREADS, 0, as_stream(stream_v)>>>(
        ws_at<const uint32_t>(workspace, L.planes), ws_at<const RleColumn>(workspace, L.columns), width, height, L.S,
        L.Wp, L.col_blocks, reinterpret_cast<const long long*>(offsets), counts, (long long)total);
    return launch_status("mask_rle_emit launch");
}

int32_t pgr_mask_rle_decode(const int32_t* counts, const int64_t* offsets, int32_t n_masks, int32_t width, int32_t height,
                            uint8_t* masks, void* stream_v) {
    if (!counts || !offsets || !masks || !rle_shape_ok(n_masks, width, height)) return PGR_ERR_INVALID_ARGUMENT;
    const int64_t HW = (int64_t)width * height;
    const int64_t slice = std::max<int64_t>(RLE_DECODE_MIN_SLICE, (HW + RLE_DECODE_MAX_SLICES - 1) / RLE_DECODE_MAX_SLICES);
    const int64_t slices = (HW + slice - 1) / slice;
    if ((int64_t)n_masks * slices > MAX_GRID_BLOCKS) return PGR_ERR_INVALID_ARGUMENT;
    rle_decode_kernel<<<(unsigned)(n_masks * slices), RLE_THREADS, 0, as_stream(stream_v)>>>(
        counts, reinterpret_cast<const long long*>(offsets), width, height, (int)slices, (int)slice, masks);
    return launch_status("mask_rle_decode launch");
}

int32_t pgr_mask_overlap(const uint8_t* a, int32_t n_a, const uint8_t* b, int32_t n_b, int32_t width, int32_t height,
                         int32_t* inter, int32_t* area_a, int32_t* area_b, void* stream_v) {
    if (!a || !b || !inter || !area_a || !area_b || !rle_shape_ok(n_a, width, height) || !rle_shape_ok(n_b, width, height))
        return PGR_ERR_INVALID_ARGUMENT;
    const size_t HW = (size_t)width * height;
    const int64_t chunks = (int64_t)((HW + OVERLAP_CHUNK - 1) / OVERLAP_CHUNK);
    const int64_t pairs = (int64_t)n_a * n_b;
    if (pairs > MAX_GRID_BLOCKS || pairs * chunks > MAX_GRID_BLOCKS) return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = as_stream(stream_v);
    if (!hip_ok(hipMemsetAsync(inter, 0, (size_t)pairs * sizeof(int32_t), stream), "mask_overlap clear") ||
        !hip_ok(hipMemsetAsync(area_a, 0, (size_t)n_a * sizeof(int32_t), stream), "mask_overlap clear") ||
        !hip_ok(hipMemsetAsync(area_b, 0, (size_t)n_b * sizeof(int32_t), stream), "mask_overlap clear"))
        return PGR_ERR_LAUNCH_FAILURE;
    mask_overlap_kernel<<<(unsigned)(pairs * chunks), RLE_THREADS, 0, stream>>>(a, n_a, b, n_b, HW, (int)chunks, inter, area_a,
                                                                               area_b);
    return launch_status("mask_overlap launch");
}

// ---- COCO scores: IoU inside groups, matching, accumulation (cocoeval.hip.h) ----------------------------------------------
namespace {
// a group table a kernel may index with: slices inside the arrays, ascending and disjoint (no two groups write one element)
bool coco_groups_ok(const PgrCocoGroup* groups, int32_t n_groups, int32_t n_dt, int32_t n_gt, int64_t iou_total) {
    if (n_groups < 0 || n_dt < 0 || n_gt < 0 || iou_total < 0 || (n_groups > 0 && !groups)) return false;
    int64_t dt_end = 0, gt_end = 0, iou_end = 0;
    for (int32_t k = 0; k < n_groups; ++k) {
        const PgrCocoGroup& G = groups[k];
        if (G.dt_count < 0 || G.gt_count < 0 || G.dt_begin < dt_end || G.gt_begin < gt_end || G.iou_offset < iou_end) return false;
        dt_end = (int64_t)G.dt_begin + G.dt_count;
        gt_end = (int64_t)G.gt_begin + G.gt_count;
        iou_end = G.iou_offset + (int64_t)G.dt_count * G.gt_count;
        if (dt_end > n_dt || gt_end > n_gt || iou_end > iou_total) return false;
    }
    return true;
}
struct CocoIouLayout { size_t groups, dt_ends, dt_cover, gt_ends, gt_cover, total; };
CocoIouLayout coco_iou_layout(int32_t n_groups, int64_t dt_total, int64_t gt_total) {
    CocoIouLayout L{};
    if (n_groups < 0 || dt_total < 0 || gt_total < 0 || dt_total > ((int64_t)1 << 40) || gt_total > ((int64_t)1 << 40)) return L;
    Carver c;
    L.groups = c.take((size_t)n_groups * sizeof(PgrCocoGroup));
    L.dt_ends = c.take((size_t)dt_total * sizeof(int32_t));
    L.dt_cover = c.take((size_t)dt_total * sizeof(int32_t));      // (read for the detections' areas only)
    L.gt_ends = c.take((size_t)gt_total * sizeof(int32_t));
    L.gt_cover = c.take((size_t)gt_total * sizeof(int32_t));
    L.total = c.off;
    return L;
}
struct CocoBoxLayout { size_t groups, total; };
CocoBoxLayout coco_box_layout(int32_t n_groups) {
    CocoBoxLayout L{};
    if (n_groups < 0) return L;
    Carver c;
    L.groups = c.take((size_t)n_groups * sizeof(PgrCocoGroup));
    L.total = c.off;
    return L;
}
// pgr_coco_match's workspace: the group table, then per area range the order in which each GT is tried
struct CocoMatchLayout { size_t groups, order, total; };
CocoMatchLayout coco_match_layout(int32_t n_groups, int32_t n_gt, int32_t n_area) {
    CocoMatchLayout L{};
    if (n_groups < 0 || n_gt < 0 || n_area < 1 || n_area > COCO_MAX_LANES) return L;
    Carver c;
    L.groups = c.take((size_t)n_groups * sizeof(PgrCocoGroup));
    L.order = c.take((size_t)n_area * n_gt * sizeof(int32_t));
    L.total = c.off;
    return L;
}
// pgr_coco_accumulate's workspace: three arrays of one cell per (area range, maxDets entry, detection)
struct CocoAccumulateLayout { size_t tp, idx, pr, total; };
CocoAccumulateLayout coco_accumulate_layout(int32_t n_dt, int32_t n_area, int32_t n_max_dets) {
    CocoAccumulateLayout L{};
    if (n_dt < 0 || n_area < 1 || n_area > COCO_MAX_LANES || n_max_dets < 1 || n_max_dets > PGR_COCO_MAX_MAXDETS) return L;
    const size_t cells = (size_t)n_area * n_max_dets * n_dt;
    Carver c;
    L.tp = c.take(cells * sizeof(int32_t));
    L.idx = c.take(cells * sizeof(int32_t));
    L.pr = c.take(cells * sizeof(double));
    L.total = c.off;
    return L;
}
// the table goes to the device in stream order and has been read when this returns: the caller may free it after the call
bool coco_groups_upload(void* dst, const PgrCocoGroup* groups, int32_t n_groups, hipStream_t stream) {
    return n_groups == 0 || hip_ok(hipMemcpyWithStream(dst, groups, (size_t)n_groups * sizeof(PgrCocoGroup), hipMemcpyHostToDevice, stream),
                                   "memcpy coco groups");
}
}  // namespace

size_t pgr_rle_iou_workspace_bytes(int32_t n_groups, int64_t dt_total, int64_t gt_total) {
    return coco_iou_layout(n_groups, dt_total, gt_total).total;
}

int32_t pgr_rle_iou(const int32_t* dt_counts, const int64_t* dt_offsets, int32_t n_dt, int64_t dt_total,
                    const int32_t* gt_counts, const int64_t* gt_offsets, int32_t n_gt, int64_t gt_total, const uint8_t* gt_crowd,
                    int32_t width, int32_t height, const PgrCocoGroup* groups, int32_t n_groups, int64_t iou_total,
                    int64_t* inter, double* iou, int64_t* dt_area, int64_t* gt_area, void* workspace, size_t workspace_bytes,
                    void* stream_v) {
    const CocoIouLayout L = coco_iou_layout(n_groups, dt_total, gt_total);
    if (width < 1 || width > RLE_MAX_SIDE || height < 1 || height > RLE_MAX_SIDE || !coco_groups_ok(groups, n_groups, n_dt, n_gt, iou_total) ||
        !L.total || !workspace || !workspace_aligned_16(workspace))
        return PGR_ERR_INVALID_ARGUMENT;
    if ((n_dt > 0 && (!dt_offsets || !dt_area || (dt_total > 0 && !dt_counts))) ||
        (n_gt > 0 && (!gt_offsets || !gt_area || !gt_crowd || (gt_total > 0 && !gt_counts))) || (iou_total > 0 && (!inter || !iou)))
        return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    auto* groups_dev = ws_at<PgrCocoGroup>(workspace, L.groups);
    auto* dt_ends = ws_at<int32_t>(workspace, L.dt_ends);
    auto* gt_ends = ws_at<int32_t>(workspace, L.gt_ends);
    auto* gt_cover = ws_at<int32_t>(workspace, L.gt_cover);
    auto* dt_cover = ws_at<int32_t>(workspace, L.dt_cover);
    if (!coco_groups_upload(groups_dev, groups, n_groups, stream)) return PGR_ERR_LAUNCH_FAILURE;
    const int HW = width * height;
    if (n_dt > 0)
        coco_rle_prefix_kernel<<<(unsigned)n_dt, COCO_THREADS, 0, stream>>>(dt_counts, reinterpret_cast<const long long*>(dt_offsets),
                                                                           (long long)dt_total, HW, dt_ends, dt_cover,
                                                                           reinterpret_cast<long long*>(dt_area));
    if (n_gt > 0)
        coco_rle_prefix_kernel<<<(unsigned)n_gt, COCO_THREADS, 0, stream>>>(gt_counts, reinterpret_cast<const long long*>(gt_offsets),
                                                                           (long long)gt_total, HW, gt_ends, gt_cover,
                                                                           reinterpret_cast<long long*>(gt_area));
    if (n_groups > 0 && iou_total > 0)
        coco_rle_iou_kernel<<<(unsigned)n_groups, COCO_THREADS, 0, stream>>>(
            groups_dev, reinterpret_cast<const long long*>(dt_offsets), (long long)dt_total,
            reinterpret_cast<const long long*>(gt_offsets), (long long)gt_total, gt_crowd, dt_ends, gt_ends, gt_cover,
            reinterpret_cast<const long long*>(dt_area), reinterpret_cast<const long long*>(gt_area),
            reinterpret_cast<long long*>(inter), iou);
    return launch_status("rle_iou launch");
}

size_t pgr_box_iou_workspace_bytes(int32_t n_groups) { return coco_box_layout(n_groups).total; }

int32_t pgr_box_iou(const double* dt_boxes, int32_t n_dt, const double* gt_boxes, int32_t n_gt, const uint8_t* gt_crowd,
                    const PgrCocoGroup* groups, int32_t n_groups, int64_t iou_total, double* iou, void* workspace,
                    size_t workspace_bytes, void* stream_v) {
    const CocoBoxLayout L = coco_box_layout(n_groups);
    if (!coco_groups_ok(groups, n_groups, n_dt, n_gt, iou_total) || !L.total || !workspace || !workspace_aligned_16(workspace) ||
        (n_dt > 0 && !dt_boxes) || (n_gt > 0 && (!gt_boxes || !gt_crowd)) || (iou_total > 0 && !iou))
        return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    if (n_groups == 0 || iou_total == 0) return PGR_OK;
    hipStream_t stream = as_stream(stream_v);
    auto* groups_dev = ws_at<PgrCocoGroup>(workspace, L.groups);
    if (!coco_groups_upload(groups_dev, groups, n_groups, stream)) return PGR_ERR_LAUNCH_FAILURE;
    coco_box_iou_kernel<<<(unsigned)n_groups, COCO_THREADS, 0, stream>>>(groups_dev, dt_boxes, gt_boxes, gt_crowd, iou);
    return launch_status("box_iou launch");
}

size_t pgr_coco_match_workspace_bytes(int32_t n_groups, int32_t n_gt, int32_t n_area) {
    return coco_match_layout(n_groups, n_gt, n_area).total;
}

int32_t pgr_coco_match(const PgrCocoGroup* groups, int32_t n_groups, int64_t iou_total, const double* iou, const double* dt_area,
                       int32_t n_dt, const double* gt_area, const uint8_t* gt_flag, const uint8_t* gt_crowd, int32_t n_gt,
                       const double* iou_thrs, int32_t n_thr, const double* area_rng, int32_t n_area, int32_t* dt_match,
                       uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore, void* workspace, size_t workspace_bytes,
                       void* stream_v) {
    const CocoMatchLayout L = coco_match_layout(n_groups, n_gt, n_area);
    if (n_thr < 1 || !L.total || (int64_t)n_thr * n_area > COCO_MAX_LANES || !iou_thrs || !area_rng ||
        !coco_groups_ok(groups, n_groups, n_dt, n_gt, iou_total) || !workspace || !workspace_aligned_16(workspace) ||
        (n_dt > 0 && (!dt_area || !dt_match || !dt_ignore)) ||
        (n_gt > 0 && (!gt_area || !gt_flag || !gt_crowd || !gt_match || !gt_ignore)) || (iou_total > 0 && !iou))
        return PGR_ERR_INVALID_ARGUMENT;
    CocoMatchParams P{};
    P.n_thr = n_thr;
    P.n_area = n_area;
    for (int32_t a = 0; a < n_area; ++a)
        for (int32_t t = 0; t < n_thr; ++t) {
            if (!(iou_thrs[t] == iou_thrs[t]) || !(area_rng[2 * a] <= area_rng[2 * a + 1])) return PGR_ERR_INVALID_ARGUMENT;
            P.thr[a * n_thr + t] = std::min(iou_thrs[t], 1.0 - 1e-10);
            P.lo[a * n_thr + t] = area_rng[2 * a];
            P.hi[a * n_thr + t] = area_rng[2 * a + 1];
        }
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    if (n_groups == 0) return PGR_OK;
    hipStream_t stream = as_stream(stream_v);
    auto* groups_dev = ws_at<PgrCocoGroup>(workspace, L.groups);
    auto* order = ws_at<int32_t>(workspace, L.order);
    if (!coco_groups_upload(groups_dev, groups, n_groups, stream)) return PGR_ERR_LAUNCH_FAILURE;
    coco_match_kernel<<<(unsigned)n_groups, WAVE, 0, stream>>>(groups_dev, P, iou, dt_area, gt_area, gt_flag, gt_crowd, (long long)n_dt,
                                                              (long long)n_gt, order, dt_match, dt_ignore, gt_match, gt_ignore);
    return launch_status("coco_match launch");
}

size_t pgr_coco_accumulate_workspace_bytes(int32_t n_dt, int32_t n_area, int32_t n_max_dets) {
    return coco_accumulate_layout(n_dt, n_area, n_max_dets).total;
}

int32_t pgr_coco_accumulate(const int64_t* perm, const int64_t* seg_start, int32_t n_cat, const int32_t* rank,
                            const int32_t* dt_match, const uint8_t* dt_ignore, const double* dt_scores, int32_t n_dt,
                            const int32_t* npig, const int32_t* max_dets, int32_t n_max_dets, const double* rec_thrs,
                            int32_t n_rec, int32_t n_thr, int32_t n_area, double* precision, double* scores, double* recall,
                            void* workspace, size_t workspace_bytes, void* stream_v) {
    const CocoAccumulateLayout L = coco_accumulate_layout(n_dt, n_area, n_max_dets);
    if (!L.total || n_cat < 0 || n_rec < 1 || n_thr < 1 || (int64_t)n_thr * n_area > COCO_MAX_LANES || !max_dets || !rec_thrs ||
        !workspace || !workspace_aligned_16(workspace) || (n_dt > 0 && (!perm || !rank || !dt_match || !dt_ignore || !dt_scores)))
        return PGR_ERR_INVALID_ARGUMENT;
    if (n_cat > 0 && (!seg_start || !npig || !precision || !scores || !recall)) return PGR_ERR_INVALID_ARGUMENT;
    if ((int64_t)n_cat * n_area * n_max_dets > MAX_GRID_BLOCKS) return PGR_ERR_INVALID_ARGUMENT;
    CocoAccumulateParams P{};
    for (int32_t m = 0; m < n_max_dets; ++m) {
        if (max_dets[m] < 0) return PGR_ERR_INVALID_ARGUMENT;
        P.max_dets[m] = max_dets[m];
    }
    P.K = n_cat; P.A = n_area; P.M = n_max_dets; P.T = n_thr; P.R = n_rec;
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    if (n_cat == 0) return PGR_OK;
    auto* ws_tp = ws_at<int32_t>(workspace, L.tp);
    auto* ws_idx = ws_at<int32_t>(workspace, L.idx);
    auto* ws_pr = ws_at<double>(workspace, L.pr);
    coco_accumulate_kernel<<<(unsigned)(n_cat * n_area * n_max_dets), COCO_THREADS, 0, as_stream(stream_v)>>>(
        P, reinterpret_cast<const long long*>(perm), reinterpret_cast<const long long*>(seg_start), (long long)n_dt, rank, dt_match,
        dt_ignore, npig, rec_thrs, dt_scores, ws_tp, ws_idx, ws_pr, precision, scores, recall);
    return launch_status("coco_accumulate launch");
}
