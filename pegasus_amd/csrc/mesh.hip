// mesh.hip -- host side of the object-mesh entries of libpegasus_raster.so: TSDF fusion and marching tetrahedra, the mesh
// the environment field, depth / visibility / shade renderers and BOP ground truth, vertex clustering, vertex attributes, distance fields and sweeps, rigid-body drops.
// Owns its kernel headers: no other translation unit includes them (DESIGN.md "Source layout").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "decimate.hip.h"
#include "envfield.hip.h"
#include "host_common.h"
#include "mesh.hip.h"
#include "meshattr.hip.h"
#include "meshraster.hip.h"
#include "meshsdf.hip.h"
#include "rigid.hip.h"

using namespace pgr;

// ---- object meshes: TSDF fusion of rendered views, marching tetrahedra (mesh.hip.h) ------------------------------------
namespace {
constexpr int32_t MESH_MAX_AXIS = 1024;
bool grid_ok(const PgrGrid* g) {
    if (!g) return false;
    for (int32_t a : {g->nx, g->ny, g->nz})
        if (a < 2 || a > MESH_MAX_AXIS) return false;
    return std::isfinite(g->origin[0]) && std::isfinite(g->origin[1]) && std::isfinite(g->origin[2]) &&
           std::isfinite(g->voxel) && g->voxel > 0.f;
}
MeshGrid mesh_grid(const PgrGrid* g) { return MeshGrid{g->nx, g->ny, g->nz, g->origin[0], g->origin[1], g->origin[2], g->voxel}; }
size_t grid_points(const PgrGrid* g) { return (size_t)g->nx * g->ny * g->nz; }
struct MarchLayout { size_t mask, ntri, vbase, tile_tot, tile_off, total; int tiles; };
MarchLayout march_layout(size_t n) {
    MarchLayout M{};
    M.tiles = (int)((n + MARCH_TILE - 1) / MARCH_TILE);
    Carver c;
    M.mask = c.take(n);
    M.ntri = c.take(n);
    M.vbase = c.take(n * sizeof(int32_t));
    M.tile_tot = c.take((size_t)M.tiles * 2 * sizeof(long long));
    M.tile_off = c.take((size_t)M.tiles * 2 * sizeof(long long));
    M.total = c.off;
    return M;
}
// The pinhole views that pgr_tsdf_integrate and pgr_mesh_vertex_colors take alike, checked and packed into their launch
// arguments (TsdfArgs, VertexColorArgs): one image size for all, a view matrix and positive tangents per view,
// fx = W / (2 tan), cx = (W - 1) / 2.  `campos` non-NULL: every view must also give its camera position, stored there.
template <typename Args>
bool pack_pinhole_views(int32_t n_views, const PgrCamera* cameras, Args& a, const float** campos = nullptr) {
    const int32_t W = cameras[0].image_width, H = cameras[0].image_height;
    if (W <= 0 || H <= 0 || (int64_t)W * H > (int64_t)1 << 28) return false;
    for (int32_t v = 0; v < n_views; ++v) {
        const PgrCamera& c = cameras[v];
        if (c.image_width != W || c.image_height != H || !c.viewmatrix || (campos && !c.campos) || !(c.tanfovx > 0.f) ||
            !(c.tanfovy > 0.f))
            return false;
        a.view[v] = c.viewmatrix;
        if (campos) campos[v] = c.campos;
        a.fx[v] = (float)((double)W / (2.0 * (double)c.tanfovx));
        a.fy[v] = (float)((double)H / (2.0 * (double)c.tanfovy));
    }
    a.n_views = n_views;
    a.width = W;
    a.height = H;
    a.cx = (float)(W - 1) * 0.5f;
    a.cy = (float)(H - 1) * 0.5f;
    return true;
}
}  // namespace

int32_t pgr_tsdf_integrate(const PgrGrid* grid, int32_t n_views, const PgrCamera* cameras, const float* depth,
                           const float* final_T, float truncation, float alpha_min, float* sdf, void* stream_v) {
    if (!grid_ok(grid) || n_views < 1 || n_views > TSDF_MAX_VIEWS || !cameras || !depth || !final_T || !sdf)
        return PGR_ERR_INVALID_ARGUMENT;
    if (!(truncation > 0.f) || !std::isfinite(truncation) || std::isnan(alpha_min)) return PGR_ERR_INVALID_ARGUMENT;
    TsdfArgs a{};
    if (!pack_pinhole_views(n_views, cameras, a)) return PGR_ERR_INVALID_ARGUMENT;
    a.g = mesh_grid(grid);
    a.truncation = truncation;
    a.alpha_min = alpha_min;
    a.depth = depth;
    a.final_T = final_T;
    a.sdf = sdf;
    const dim3 block(TSDF_BX, TSDF_BY, TSDF_BZ);
    const dim3 blocks((grid->nx + TSDF_BX - 1) / TSDF_BX, (grid->ny + TSDF_BY - 1) / TSDF_BY, (grid->nz + TSDF_BZ - 1) / TSDF_BZ);
    tsdf_integrate_kernel<<<blocks, block, 0, as_stream(stream_v)>>>(a);
    return launch_status("tsdf_integrate launch");
}

// ---- the environment as a distance field (envfield.hip.h) ---------------------------------------------------------------------
namespace {
struct EnvLayout { size_t near_in, near_out, total; };
EnvLayout env_layout(size_t n) {
    EnvLayout L{};
    Carver c;
    L.near_in = c.take(n * sizeof(uint32_t));
    L.near_out = c.take(n * sizeof(uint32_t));
    L.total = c.off;
    return L;
}
int32_t env_columns(int32_t n) { return n <= 256 ? 64 : (n <= 512 ? 32 : 16); }   // n * columns <= ENV_LINE_WORDS
}  // namespace

size_t pgr_sdf_from_tsdf_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    const PgrGrid g{nx, ny, nz, {0.f, 0.f, 0.f}, 1.f};
    return grid_ok(&g) ? env_layout(grid_points(&g)).total : 0;
}

int32_t pgr_sdf_from_tsdf(const PgrGrid* grid, const float* tsdf, float* sdf, int32_t* dist2, void* workspace,
                          size_t workspace_bytes, void* stream_v) {
    static_assert(MESH_MAX_AXIS == ENV_MAX_AXIS && ENV_MAX_AXIS * 16 <= ENV_LINE_WORDS, "line tiles of env_line_kernel");
    if (!grid_ok(grid) || !tsdf || !sdf || sdf == tsdf || !workspace || !workspace_aligned_16(workspace))
        return PGR_ERR_INVALID_ARGUMENT;
    const size_t n = grid_points(grid);
    const EnvLayout L = env_layout(n);
    if (workspace_bytes < L.total) return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = as_stream(stream_v);
    auto* near_in = ws_at<uint32_t>(workspace, L.near_in);
    auto* near_out = ws_at<uint32_t>(workspace, L.near_out);
    const int32_t nx = grid->nx, ny = grid->ny, nz = grid->nz;
    const int32_t lines_per_block = std::max(1, ENV_THREADS / nx);
    const long long lines = (long long)ny * nz;
    env_x_kernel<<<(uint32_t)((lines + lines_per_block - 1) / lines_per_block), ENV_THREADS, 0, stream>>>(
        nx, (long long)n, lines_per_block, tsdf, near_in, near_out);
    const long long slab = (long long)nx * ny;
    int32_t tx = env_columns(ny);
    env_line_kernel<<<dim3((uint32_t)((nx + tx - 1) / tx), (uint32_t)nz, 2), ENV_THREADS, (size_t)ny * tx * sizeof(uint32_t), stream>>>(
        nx, ny, (long long)nx, slab, tx, near_in, near_out);
    tx = env_columns(nz);
    env_line_kernel<<<dim3((uint32_t)((nx + tx - 1) / tx), (uint32_t)ny, 2), ENV_THREADS, (size_t)nz * tx * sizeof(uint32_t), stream>>>(
        nx, nz, slab, (long long)nx, tx, near_in, near_out);
    env_value_kernel<<<(uint32_t)((n + ENV_THREADS - 1) / ENV_THREADS), ENV_THREADS, 0, stream>>>(mesh_grid(grid), tsdf, near_in,
                                                                                                 near_out, sdf, dist2);
    return launch_status("sdf_from_tsdf launch");
}

size_t pgr_march_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    const PgrGrid g{nx, ny, nz, {0.f, 0.f, 0.f}, 1.f};
    return grid_ok(&g) ? march_layout(grid_points(&g)).total : 0;
}

int32_t pgr_march_count(const PgrGrid* grid, const float* sdf, void* workspace, size_t workspace_bytes, int64_t* counts,
                        void* stream_v) {
    if (!grid_ok(grid) || !sdf || !workspace || !counts) return PGR_ERR_INVALID_ARGUMENT;
    const size_t n = grid_points(grid);
    const MarchLayout M = march_layout(n);
    if (workspace_bytes < M.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    auto* tile_tot = ws_at<long long>(workspace, M.tile_tot);
    march_count_kernel<<<M.tiles, MARCH_THREADS, 0, stream>>>(mesh_grid(grid), sdf, n, ws_at<uint8_t>(workspace, M.mask),
                                                              ws_at<uint8_t>(workspace, M.ntri), tile_tot);
    auto* tile_off = ws_at<long long>(workspace, M.tile_off);
    march_scan_kernel<<<1, MARCH_SCAN_THREADS, 0, stream>>>(tile_tot, M.tiles, tile_off, reinterpret_cast<long long*>(counts));
    march_vbase_kernel<<<M.tiles, MARCH_THREADS, 0, stream>>>(n, ws_at<uint8_t>(workspace, M.mask), tile_off,
                                                              ws_at<int32_t>(workspace, M.vbase));
    return launch_status("march_count launch");
}

int32_t pgr_march_emit(const PgrGrid* grid, const float* sdf, const void* workspace, size_t workspace_bytes, float* vertices,
                       int32_t* faces, void* stream_v) {
    if (!grid_ok(grid) || !sdf || !workspace || !vertices || !faces) return PGR_ERR_INVALID_ARGUMENT;
    const size_t n = grid_points(grid);
    const MarchLayout M = march_layout(n);
    if (workspace_bytes < M.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    const auto* mask = ws_at<const uint8_t>(workspace, M.mask);
    const auto* tile_off = ws_at<const long long>(workspace, M.tile_off);
    const auto* vbase = ws_at<const int32_t>(workspace, M.vbase);
    march_vertices_kernel<<<(unsigned)((n + MARCH_THREADS - 1) / MARCH_THREADS), MARCH_THREADS, 0, stream>>>(
        mesh_grid(grid), sdf, n, mask, vbase, vertices);
    march_faces_kernel<<<M.tiles, MARCH_THREADS, 0, stream>>>(mesh_grid(grid), sdf, n, mask,
                                                              ws_at<const uint8_t>(workspace, M.ntri), tile_off, vbase, faces);
    return launch_status("march_emit launch");
}

// ---- mesh depth renderer and BOP ground truth (meshraster.hip.h) ------------------------------------------------------
namespace {
constexpr int32_t MESHR_MAX_CANVAS = 8192;
bool mesh_jobs_ok(int32_t n_jobs, const PgrMeshJob* jobs) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return false;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrMeshJob& j = jobs[k];
        if (j.vertex_first < 0 || j.vertex_count < 0 || j.face_first < 0 || j.face_count < 0 ||
            j.face_count > MESHR_MAX_GROUP_FACES)
            return false;
    }
    return true;
}
// what pgr_mesh_depth, pgr_mesh_visibility and pgr_mesh_shade ask alike of the meshes, the jobs and the canvases
bool mesh_call_ok(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t n_jobs,
                  const PgrMeshJob* jobs, int32_t width, int32_t height, float near_z, int32_t n_slots) {
    if (!mesh_jobs_ok(n_jobs, jobs) || n_slots < 1 || n_vertices < 0 || n_faces < 0 || width < 1 || width > MESHR_MAX_CANVAS ||
        height < 1 || height > MESHR_MAX_CANVAS || !(near_z > 0.f) || !std::isfinite(near_z))
        return false;
    bool any_faces = false;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrMeshJob& j = jobs[k];
        if ((int64_t)j.vertex_first + j.vertex_count > n_vertices || (int64_t)j.face_first + j.face_count > n_faces ||
            j.slot < 0 || j.slot >= n_slots)
            return false;
        any_faces = any_faces || j.face_count > 0;
    }
    return !any_faces || (vertices && faces);
}
MeshJobDev mesh_job_dev(const PgrMeshJob& j) {
    MeshJobDev d{};
    d.v0 = j.vertex_first; d.nv = j.vertex_count; d.f0 = j.face_first; d.nf = j.face_count;
    std::memcpy(d.R, j.R, sizeof(d.R));
    std::memcpy(d.t, j.t, sizeof(d.t));
    d.fx = j.fx; d.fy = j.fy; d.cx = j.cx; d.cy = j.cy;
    d.slot = j.slot;
    return d;
}
// jobs [k0, end) of one launch: at most MESHR_JOBS_PER_LAUNCH jobs and MESHR_MAX_GROUP_FACES faces
int32_t mesh_group_end(int32_t n_jobs, const PgrMeshJob* jobs, int32_t k0, int64_t* faces_out) {
    int64_t faces = 0;
    int32_t k = k0;
    while (k < n_jobs && k - k0 < MESHR_JOBS_PER_LAUNCH && (k == k0 || faces + jobs[k].face_count <= MESHR_MAX_GROUP_FACES))
        faces += jobs[k++].face_count;
    *faces_out = faces;
    return k;
}
int64_t mesh_queue_capacity(int32_t n_jobs, const PgrMeshJob* jobs) {
    int64_t cap = 0, faces = 0;
    for (int32_t k0 = 0; k0 < n_jobs;) {
        k0 = mesh_group_end(n_jobs, jobs, k0, &faces);
        cap = std::max(cap, faces);
    }
    return cap;
}
// pgr_mesh_depth's workspace: the queue's counter, then a queue that holds the faces of the largest launch
struct MeshDepthLayout { size_t qctr, queue, total; };
MeshDepthLayout mesh_depth_layout(int32_t n_jobs, const PgrMeshJob* jobs) {
    MeshDepthLayout L{};
    if (n_jobs <= 0 || !mesh_jobs_ok(n_jobs, jobs)) return L;
    Carver c;
    L.qctr = c.take(sizeof(unsigned long long));
    L.queue = c.take((size_t)mesh_queue_capacity(n_jobs, jobs) * sizeof(MeshQueueEntry));
    L.total = c.off;
    return L;
}
}  // namespace

namespace {
// pgr_mesh_depth (Pix = uint32_t: the depth's bits) and pgr_mesh_visibility (Pix = uint64_t: depth << 32 | job << 22 | face)
template <typename Pix>
int32_t mesh_raster_run(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t n_jobs,
                        const PgrMeshJob* jobs, int32_t width, int32_t height, float near_z, Pix* out, int32_t n_slots,
                        int32_t* straddle_count, void* workspace, size_t workspace_bytes, void* stream_v, const char* what) {
    if (!out || !straddle_count || !mesh_call_ok(vertices, n_vertices, faces, n_faces, n_jobs, jobs, width, height, near_z, n_slots))
        return PGR_ERR_INVALID_ARGUMENT;
    const MeshDepthLayout L = mesh_depth_layout(n_jobs, jobs);
    if (n_jobs > 0 && (!L.total || !workspace || workspace_bytes < L.total)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    const size_t plane = (size_t)width * height, total = plane * (size_t)n_slots;
    if (!hip_ok(hipMemsetAsync(out, 0xFF, total * sizeof(Pix), stream), what) ||
        !hip_ok(hipMemsetAsync(straddle_count, 0, sizeof(int32_t), stream), what))
        return PGR_ERR_LAUNCH_FAILURE;
    auto* qctr = ws_at<unsigned long long>(workspace, L.qctr);
    auto* queue = ws_at<MeshQueueEntry>(workspace, L.queue);
    int64_t group_faces = 0;
    for (int32_t k0 = 0; k0 < n_jobs;) {
        const int32_t k1 = mesh_group_end(n_jobs, jobs, k0, &group_faces);
        MeshJobTable T{};
        T.count = k1 - k0;
        T.width = width;
        T.height = height;
        T.near = near_z;
        T.first = k0;
        uint32_t blocks = 0;
        for (int32_t k = k0; k < k1; ++k) {
            T.job[k - k0] = mesh_job_dev(jobs[k]);
            T.job[k - k0].block0 = blocks;
            blocks += (uint32_t)((jobs[k].face_count + MESHR_THREADS - 1) / MESHR_THREADS);
        }
        k0 = k1;
        if (!blocks) continue;
        if (!hip_ok(hipMemsetAsync(qctr, 0, sizeof(unsigned long long), stream), what)) return PGR_ERR_LAUNCH_FAILURE;
        mesh_small_kernel<Pix><<<blocks, MESHR_THREADS, 0, stream>>>(T, vertices, faces, out, plane, qctr, queue,
                                                                     (long long)group_faces, straddle_count);
        mesh_large_kernel<Pix><<<MESHR_LARGE_WAVES / (MESHR_THREADS / WAVE), MESHR_THREADS, 0, stream>>>(
            T, vertices, faces, out, plane, qctr, queue, (long long)group_faces);
    }
    mesh_finalize_kernel<Pix><<<(unsigned)std::min<size_t>((total + 255) / 256, 65536), 256, 0, stream>>>(out, total);
    return launch_status(what);
}
}  // namespace

size_t pgr_mesh_depth_workspace_bytes(int32_t n_jobs, const PgrMeshJob* jobs) { return mesh_depth_layout(n_jobs, jobs).total; }

int32_t pgr_mesh_depth(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t n_jobs,
                       const PgrMeshJob* jobs, int32_t width, int32_t height, float near_z, float* depth, int32_t n_slots,
                       int32_t* straddle_count, void* workspace, size_t workspace_bytes, void* stream_v) {
    return mesh_raster_run(vertices, n_vertices, faces, n_faces, n_jobs, jobs, width, height, near_z,
                           reinterpret_cast<uint32_t*>(depth), n_slots, straddle_count, workspace, workspace_bytes, stream_v,
                           "mesh_depth launch");
}

// the key leaves 10 bits for the job: a call takes at most MESHV_MAX_JOBS jobs, the caller chunks
size_t pgr_mesh_visibility_workspace_bytes(int32_t n_jobs, const PgrMeshJob* jobs) {
    return n_jobs > MESHV_MAX_JOBS ? 0 : mesh_depth_layout(n_jobs, jobs).total;
}

int32_t pgr_mesh_visibility(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t n_jobs,
                            const PgrMeshJob* jobs, int32_t width, int32_t height, float near_z, uint64_t* keys,
                            int32_t n_slots, int32_t* straddle_count, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (n_jobs > MESHV_MAX_JOBS || reinterpret_cast<uintptr_t>(keys) % sizeof(uint64_t)) return PGR_ERR_INVALID_ARGUMENT;
    return mesh_raster_run(vertices, n_vertices, faces, n_faces, n_jobs, jobs, width, height, near_z, keys, n_slots,
                           straddle_count, workspace, workspace_bytes, stream_v, "mesh_visibility launch");
}

// pgr_mesh_shade's workspace: the device-side job table
size_t pgr_mesh_shade_workspace_bytes(int32_t n_jobs, const PgrMeshJob* jobs) {
    if (n_jobs <= 0 || n_jobs > MESHV_MAX_JOBS || !mesh_jobs_ok(n_jobs, jobs)) return 0;
    return align_up((size_t)n_jobs * sizeof(MeshShadeJobDev), 256);
}

// pgr_mesh_shade_textured's workspace: the job table, then one MeshJobTexDev per job
size_t pgr_mesh_shade_textured_workspace_bytes(int32_t n_jobs, const PgrMeshJob* jobs) {
    const size_t table = pgr_mesh_shade_workspace_bytes(n_jobs, jobs);
    return table ? table + align_up((size_t)n_jobs * sizeof(MeshJobTexDev), 256) : 0;
}

namespace {
// what pgr_mesh_shade_textured asks of its textures beyond pgr_mesh_shade's arguments
bool mesh_textures_ok(const PgrMeshTextures* tex, int32_t n_jobs) {
    if (!tex || tex->n_textures < 0 || tex->texel_bytes < 0 || (tex->n_textures > 0 && !tex->textures) || (n_jobs > 0 && !tex->job_texture) ||
        (tex->filter != PGR_TEXTURE_NEAREST && tex->filter != PGR_TEXTURE_BILINEAR))
        return false;
    for (int32_t q = 0; q < tex->n_textures; ++q) {
        const PgrMeshTexture& t = tex->textures[q];
        if (t.width < 1 || t.width > MESHR_MAX_CANVAS || t.height < 1 || t.height > MESHR_MAX_CANVAS || t.offset < 0 ||
            t.offset > tex->texel_bytes || (int64_t)t.width * t.height * 3 > tex->texel_bytes - t.offset)
            return false;
    }
    bool any = false;
    for (int32_t k = 0; k < n_jobs; ++k) {
        if (tex->job_texture[k] < -1 || tex->job_texture[k] >= tex->n_textures) return false;
        any = any || tex->job_texture[k] >= 0;
    }
    return !any || (tex->corner_uv && tex->texels);
}

// pgr_mesh_shade (tex == NULL) and pgr_mesh_shade_textured: the job table through the workspace, then one launch
int32_t mesh_shade_run(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t n_jobs,
                       const PgrMeshJob* jobs, int32_t width, int32_t height, float near_z, const uint64_t* keys, int32_t n_slots,
                       const PgrMeshShade* shade, const PgrMeshTextures* tex, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (n_jobs > MESHV_MAX_JOBS || !keys || !shade || std::isnan(shade->ambient) || reinterpret_cast<uintptr_t>(keys) % sizeof(uint64_t) ||
        reinterpret_cast<uintptr_t>(workspace) % (tex ? alignof(MeshJobTexDev) : alignof(MeshShadeJobDev)) ||
        !mesh_call_ok(vertices, n_vertices, faces, n_faces, n_jobs, jobs, width, height, near_z, n_slots) ||
        (tex && !mesh_textures_ok(tex, n_jobs)))
        return PGR_ERR_INVALID_ARGUMENT;
    const size_t need = tex ? pgr_mesh_shade_textured_workspace_bytes(n_jobs, jobs) : pgr_mesh_shade_workspace_bytes(n_jobs, jobs);
    if (n_jobs > 0 && (!need || !workspace || workspace_bytes < need)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    auto* table = static_cast<MeshShadeJobDev*>(workspace);
    auto* tex_table = tex && n_jobs > 0 ? ws_at<MeshJobTexDev>(workspace, pgr_mesh_shade_workspace_bytes(n_jobs, jobs)) : nullptr;
    for (int32_t k0 = 0; tex && k0 < n_jobs; k0 += MESHR_JOBS_PER_LAUNCH) {
        MeshTexTable T{};
        T.count = std::min(MESHR_JOBS_PER_LAUNCH, n_jobs - k0);
        T.first = k0;
        for (int32_t k = 0; k < T.count; ++k) {
            const int32_t q = tex->job_texture[k0 + k];
            if (q >= 0) T.tex[k] = MeshJobTexDev{(unsigned long long)tex->textures[q].offset, tex->textures[q].width, tex->textures[q].height};
        }
        mesh_tex_table_kernel<<<1, 64, 0, stream>>>(T, tex_table);
    }
    for (int32_t k0 = 0; k0 < n_jobs; k0 += MESHR_JOBS_PER_LAUNCH) {
        MeshShadeTable T{};
        T.count = std::min(MESHR_JOBS_PER_LAUNCH, n_jobs - k0);
        T.first = k0;
        for (int32_t k = 0; k < T.count; ++k) {
            T.job[k].job = mesh_job_dev(jobs[k0 + k]);
            for (int d = 0; d < 3; ++d) T.job[k].surf[d] = shade->surf_colors ? shade->surf_colors[3 * (size_t)(k0 + k) + d] : 0.5f;
        }
        mesh_shade_table_kernel<<<1, 64, 0, stream>>>(T, table);
    }
    MeshShadeArgs A{};
    A.n_jobs = n_jobs; A.width = width; A.height = height; A.n_slots = n_slots;
    A.near = near_z; A.ambient = shade->ambient;
    std::memcpy(A.light, shade->light, sizeof(A.light));
    std::memcpy(A.bg, shade->bg, sizeof(A.bg));
    A.vertices = vertices; A.faces = faces; A.normals = shade->normals; A.colors = shade->colors;
    A.keys = keys; A.jobs = table;
    A.depth = shade->depth; A.face_id = shade->face_id; A.job_id = shade->job_id;
    A.xyz = shade->xyz; A.normal = shade->normal; A.rgb = shade->rgb;
    const dim3 grid((unsigned)((width + MESHS_TILE_W - 1) / MESHS_TILE_W),
                    (unsigned)((height + MESHS_TILE_H * (MESHS_THREADS / WAVE) - 1) / (MESHS_TILE_H * (MESHS_THREADS / WAVE))),
                    (unsigned)std::min(n_slots, 65535));
    if (!tex) {
        mesh_shade_kernel<false><<<grid, MESHS_THREADS, 0, stream>>>(A, MeshTextureArgs{});
        return launch_status("mesh_shade launch");
    }
    MeshTextureArgs X{};
    X.corner_uv = tex->corner_uv; X.texels = tex->texels; X.job_tex = tex_table;
    X.bilinear = tex->filter == PGR_TEXTURE_BILINEAR ? 1 : 0;
    X.uv = tex->uv;
    mesh_shade_kernel<true><<<grid, MESHS_THREADS, 0, stream>>>(A, X);
    return launch_status("mesh_shade_textured launch");
}
}  // namespace

int32_t pgr_mesh_shade(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t n_jobs,
                       const PgrMeshJob* jobs, int32_t width, int32_t height, float near_z, const uint64_t* keys,
                       int32_t n_slots, const PgrMeshShade* shade, void* workspace, size_t workspace_bytes, void* stream_v) {
    return mesh_shade_run(vertices, n_vertices, faces, n_faces, n_jobs, jobs, width, height, near_z, keys, n_slots, shade, nullptr,
                          workspace, workspace_bytes, stream_v);
}

int32_t pgr_mesh_shade_textured(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t n_jobs,
                                const PgrMeshJob* jobs, int32_t width, int32_t height, float near_z, const uint64_t* keys,
                                int32_t n_slots, const PgrMeshShade* shade, const PgrMeshTextures* textures, void* workspace,
                                size_t workspace_bytes, void* stream_v) {
    if (!textures) return PGR_ERR_INVALID_ARGUMENT;
    return mesh_shade_run(vertices, n_vertices, faces, n_faces, n_jobs, jobs, width, height, near_z, keys, n_slots, shade, textures,
                          workspace, workspace_bytes, stream_v);
}

int32_t pgr_bop_gt_info(const float* canvases, int32_t n_slots, int32_t canvas_width, int32_t canvas_height, int32_t margin_x,
                        int32_t margin_y, const float* scene_depth, int32_t n_frames, int32_t width, int32_t height,
                        int32_t n_jobs, const PgrGtInfoJob* jobs, float delta, uint8_t* mask, uint8_t* mask_visib,
                        int32_t* stats, void* stream_v) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs) || !canvases || !scene_depth || !mask || !mask_visib || !stats || n_slots < 1 ||
        n_frames < 1 || canvas_width < 1 || canvas_width > MESHR_MAX_CANVAS || canvas_height < 1 ||
        canvas_height > MESHR_MAX_CANVAS || width < 1 || height < 1 || margin_x < 0 || margin_y < 0 ||
        (int64_t)margin_x + width > canvas_width || (int64_t)margin_y + height > canvas_height || std::isnan(delta))
        return PGR_ERR_INVALID_ARGUMENT;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrGtInfoJob& j = jobs[k];
        if (j.slot < 0 || j.slot >= n_slots || j.frame < 0 || j.frame >= n_frames || !(j.fx != 0.0) || !(j.fy != 0.0) ||
            !std::isfinite(j.fx) || !std::isfinite(j.fy) || !std::isfinite(j.cx) || !std::isfinite(j.cy))
            return PGR_ERR_INVALID_ARGUMENT;
    }
    if (n_jobs == 0) return PGR_OK;
    hipStream_t stream = as_stream(stream_v);
    gt_info_init_kernel<<<(n_jobs * GT_STATS + 255) / 256, 256, 0, stream>>>(stats, n_jobs);
    const size_t plane = (size_t)canvas_width * canvas_height;
    const unsigned blocks_x = (unsigned)std::min<size_t>((plane + 255) / 256, GT_BLOCKS_X);
    for (int32_t k0 = 0; k0 < n_jobs; k0 += GT_JOBS_PER_LAUNCH) {
        GtJobTable T{};
        T.count = std::min(GT_JOBS_PER_LAUNCH, n_jobs - k0);
        T.first = k0;
        T.canvas_w = canvas_width; T.canvas_h = canvas_height; T.width = width; T.height = height;
        T.mx = margin_x; T.my = margin_y;
        T.delta = delta;
        for (int32_t k = 0; k < T.count; ++k) {
            const PgrGtInfoJob& j = jobs[k0 + k];
            T.job[k] = GtJobDev{j.slot, j.frame, j.fx, j.fy, j.cx, j.cy};
        }
        gt_info_kernel<<<dim3(blocks_x, (unsigned)T.count), 256, 0, stream>>>(T, canvases, scene_depth, mask, mask_visib, stats);
    }
    return launch_status("bop_gt_info launch");
}

// ---- mesh decimation by vertex clustering (decimate.hip.h) ---------------------------------------------------------------
namespace {
constexpr int32_t DEC_MAX_VERTICES = 1 << 30, DEC_MAX_FACES = 0x7fffffff / 3;
struct DecLayout {
    size_t key_a, key_b, val_a, val_b, hist, flag, number, block_tot;       // scratch of either pass
    size_t cluster_of_vertex, order, start, cluster_key, tri, perm, rank;   // what the count pass leaves for the emit pass
    size_t corner_begin, corner_end, total;
    uint32_t items, blocks;                                                 // the longest array sorted, and its tiles
};
DecLayout dec_layout(int32_t n_vertices, int32_t n_faces) {
    DecLayout D{};
    const size_t V = (size_t)n_vertices, F = (size_t)n_faces;
    D.items = (uint32_t)std::max(std::max(V, 3 * F), (size_t)1);
    D.blocks = (D.items + DEC_TILE - 1) / DEC_TILE;
    Carver c;
    D.key_a = c.take(D.items * sizeof(uint64_t));
    D.key_b = c.take(D.items * sizeof(uint64_t));
    D.val_a = c.take(D.items * sizeof(uint32_t));
    D.val_b = c.take(D.items * sizeof(uint32_t));
    D.hist = c.take((size_t)256 * D.blocks * sizeof(uint32_t));
    D.flag = c.take(D.items * sizeof(uint32_t));
    D.number = c.take(D.items * sizeof(uint32_t));
    D.block_tot = c.take((size_t)D.blocks * sizeof(uint32_t));
    D.cluster_of_vertex = c.take(V * sizeof(int32_t));
    D.order = c.take(V * sizeof(uint32_t));
    D.start = c.take((V + 1) * sizeof(uint32_t));
    D.cluster_key = c.take(V * sizeof(uint64_t));
    D.tri = c.take(3 * F * sizeof(int32_t));
    D.perm = c.take(F * sizeof(uint32_t));
    D.rank = c.take(F * sizeof(uint32_t));
    D.corner_begin = c.take(V * sizeof(uint32_t));
    D.corner_end = c.take(V * sizeof(uint32_t));
    D.total = c.off;
    return D;
}
int dec_bits(uint32_t v) {                                                  // the smallest b with v < 2^b
    int b = 1;
    while (b < 32 && (v >> b) != 0u) ++b;
    return b;
}
unsigned dec_blocks(uint32_t n) { return (n + DEC_BLOCK - 1) / DEC_BLOCK; }
struct DecSortBuffers { uint64_t* key[2]; uint32_t* val[2]; uint32_t* hist; };
// sorts the n pairs in (key[0], val[0]) by bits [0, bits) of the key, stably; returns which buffer holds the result
int dec_sort(uint32_t n, int bits, const DecSortBuffers& S, hipStream_t stream) {
    const uint32_t tiles = (n + DEC_TILE - 1) / DEC_TILE;
    int at = 0;
    for (int shift = 0; shift < bits; shift += 8, at ^= 1) {
        dec_sort_hist_kernel<<<tiles, DEC_BLOCK, 0, stream>>>(n, S.key[at], shift, S.hist, tiles);
        dec_scan_kernel<<<1, DEC_SCAN_BLOCK, 0, stream>>>(S.hist, 256u * tiles);
        dec_sort_scatter_kernel<<<tiles, DEC_BLOCK, 0, stream>>>(n, S.key[at], S.val[at], S.key[at ^ 1], S.val[at ^ 1], shift,
                                                                 S.hist, tiles);
    }
    return at;
}
// out[i] = flag[0] + .. + flag[i]
void dec_flag_scan(uint32_t n, const uint32_t* flag, uint32_t* block_tot, uint32_t* out, hipStream_t stream) {
    const uint32_t tiles = (n + DEC_TILE - 1) / DEC_TILE;
    dec_flag_reduce_kernel<<<tiles, DEC_BLOCK, 0, stream>>>(n, flag, block_tot);
    dec_scan_kernel<<<1, DEC_SCAN_BLOCK, 0, stream>>>(block_tot, tiles);
    dec_flag_apply_kernel<<<tiles, DEC_BLOCK, 0, stream>>>(n, flag, block_tot, out);
}
bool dec_sizes_ok(int32_t n_vertices, int32_t n_faces) {
    return n_vertices >= 0 && n_vertices <= DEC_MAX_VERTICES && n_faces >= 0 && n_faces <= DEC_MAX_FACES;
}
bool dec_grid_ok(double voxel, double lo_x, double lo_y, double lo_z) {
    return std::isfinite(voxel) && voxel > 0.0 && std::isfinite(lo_x) && std::isfinite(lo_y) && std::isfinite(lo_z);
}
}  // namespace

size_t pgr_mesh_cluster_workspace_bytes(int32_t n_vertices, int32_t n_faces) {
    return dec_sizes_ok(n_vertices, n_faces) ? dec_layout(n_vertices, n_faces).total : 0;
}

int32_t pgr_mesh_cluster_count(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, double voxel,
                               double lo_x, double lo_y, double lo_z, void* workspace, size_t workspace_bytes, int64_t* counts,
                               void* stream_v) {
    if (!dec_sizes_ok(n_vertices, n_faces) || !dec_grid_ok(voxel, lo_x, lo_y, lo_z)) return PGR_ERR_INVALID_ARGUMENT;
    if (!counts || !workspace || !workspace_aligned_16(workspace) || (n_vertices > 0 && !vertices) || (n_faces > 0 && !faces))
        return PGR_ERR_INVALID_ARGUMENT;
    const DecLayout D = dec_layout(n_vertices, n_faces);
    if (workspace_bytes < D.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    if (!hip_ok(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), stream), "memset cluster counts")) return PGR_ERR_LAUNCH_FAILURE;
    if (n_vertices == 0) return PGR_OK;                                     // (no vertex: no cluster, and no face can be kept)
    const DecSortBuffers S{{ws_at<uint64_t>(workspace, D.key_a), ws_at<uint64_t>(workspace, D.key_b)},
                           {ws_at<uint32_t>(workspace, D.val_a), ws_at<uint32_t>(workspace, D.val_b)},
                           ws_at<uint32_t>(workspace, D.hist)};
    auto* flag = ws_at<uint32_t>(workspace, D.flag);
    auto* number = ws_at<uint32_t>(workspace, D.number);
    auto* block_tot = ws_at<uint32_t>(workspace, D.block_tot);
    auto* cluster_of_vertex = ws_at<int32_t>(workspace, D.cluster_of_vertex);
    auto* tri = ws_at<int32_t>(workspace, D.tri);
    auto* rank = ws_at<uint32_t>(workspace, D.rank);
    const uint32_t V = (uint32_t)n_vertices, F = (uint32_t)n_faces;
    const DecGrid g{{lo_x, lo_y, lo_z}, voxel};

    dec_vertex_key_kernel<<<dec_blocks(V), DEC_BLOCK, 0, stream>>>(V, vertices, g, S.key[0], S.val[0]);
    int at = dec_sort(V, 60, S, stream);
    dec_key_heads_kernel<<<dec_blocks(V), DEC_BLOCK, 0, stream>>>(V, S.key[at], flag);
    dec_flag_scan(V, flag, block_tot, number, stream);
    dec_cluster_write_kernel<<<dec_blocks(V), DEC_BLOCK, 0, stream>>>(
        V, S.key[at], S.val[at], number, cluster_of_vertex, ws_at<uint32_t>(workspace, D.order),
        ws_at<uint32_t>(workspace, D.start), ws_at<uint64_t>(workspace, D.cluster_key), reinterpret_cast<long long*>(counts));
    if (F > 0) {
        const int bits = dec_bits(V);
        const bool packed = bits <= DEC_PACKED_MAX_BITS;
        dec_face_key_kernel<<<dec_blocks(F), DEC_BLOCK, 0, stream>>>(F, faces, V, cluster_of_vertex, packed ? bits : 0, tri,
                                                                     S.key[0], S.val[0]);
        at = dec_sort(F, packed ? 3 * bits : bits, S, stream);
        if (!packed) {
            // the second stage sorts from buffer 0: the first stage's values go there unless they already are
            if (at == 1 && !hip_ok(hipMemcpyAsync(S.val[0], S.val[1], (size_t)F * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream),
                                   "memcpy face order"))
                return PGR_ERR_LAUNCH_FAILURE;
            dec_face_key2_kernel<<<dec_blocks(F), DEC_BLOCK, 0, stream>>>(F, tri, S.val[0], V, S.key[0]);
            at = dec_sort(F, 32 + bits, S, stream);
        }
        dec_face_heads_kernel<<<dec_blocks(F), DEC_BLOCK, 0, stream>>>(F, tri, S.val[at], ws_at<uint32_t>(workspace, D.perm),
                                                                       flag);
        dec_flag_scan(F, flag, block_tot, rank, stream);
        dec_face_total_kernel<<<1, 1, 0, stream>>>(F, rank, reinterpret_cast<long long*>(counts));
    }
    return launch_status("mesh_cluster_count launch");
}

int32_t pgr_mesh_cluster_emit(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, double voxel,
                              double lo_x, double lo_y, double lo_z, int32_t contraction, void* workspace,
                              size_t workspace_bytes, int64_t n_clusters, int64_t n_out_faces, double* out_vertices,
                              int32_t* out_faces, int32_t* cluster_of_vertex, uint8_t* used_quadric, void* stream_v) {
    if (!dec_sizes_ok(n_vertices, n_faces) || !dec_grid_ok(voxel, lo_x, lo_y, lo_z)) return PGR_ERR_INVALID_ARGUMENT;
    if (contraction != PGR_CONTRACTION_AVERAGE && contraction != PGR_CONTRACTION_QUADRIC) return PGR_ERR_INVALID_ARGUMENT;
    if (n_clusters < 0 || n_clusters > n_vertices || n_out_faces < 0 || n_out_faces > n_faces) return PGR_ERR_INVALID_ARGUMENT;
    if (!workspace || !workspace_aligned_16(workspace) || (n_vertices > 0 && (!vertices || !cluster_of_vertex)) ||
        (n_faces > 0 && !faces) || (n_clusters > 0 && (!out_vertices || !used_quadric)) || (n_out_faces > 0 && !out_faces))
        return PGR_ERR_INVALID_ARGUMENT;
    const DecLayout D = dec_layout(n_vertices, n_faces);
    if (workspace_bytes < D.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    if (n_vertices == 0) return PGR_OK;
    hipStream_t stream = as_stream(stream_v);
    const DecSortBuffers S{{ws_at<uint64_t>(workspace, D.key_a), ws_at<uint64_t>(workspace, D.key_b)},
                           {ws_at<uint32_t>(workspace, D.val_a), ws_at<uint32_t>(workspace, D.val_b)},
                           ws_at<uint32_t>(workspace, D.hist)};
    const auto* cov = ws_at<const int32_t>(workspace, D.cluster_of_vertex);
    auto* corner_begin = ws_at<uint32_t>(workspace, D.corner_begin);
    auto* corner_end = ws_at<uint32_t>(workspace, D.corner_end);
    const uint32_t V = (uint32_t)n_vertices, F = (uint32_t)n_faces;
    if (!hip_ok(hipMemcpyAsync(cluster_of_vertex, cov, (size_t)V * sizeof(int32_t), hipMemcpyDeviceToDevice, stream),
                "memcpy cluster_of_vertex"))
        return PGR_ERR_LAUNCH_FAILURE;
    if (n_out_faces > 0)
        dec_face_emit_kernel<<<dec_blocks(F), DEC_BLOCK, 0, stream>>>(
            F, ws_at<const int32_t>(workspace, D.tri), ws_at<const uint32_t>(workspace, D.perm),
            ws_at<const uint32_t>(workspace, D.rank), n_out_faces, out_faces);
    if (n_clusters > 0) {
        const bool quadric = contraction == PGR_CONTRACTION_QUADRIC && F > 0;
        int at = 0;
        if (quadric) {
            // the two range tables lie one behind the other: one memset
            if (!hip_ok(hipMemsetAsync(corner_begin, 0, D.total - D.corner_begin, stream), "memset corner ranges"))
                return PGR_ERR_LAUNCH_FAILURE;
            dec_corner_key_kernel<<<dec_blocks(3 * F), DEC_BLOCK, 0, stream>>>(3 * F, faces, V, cov, S.key[0], S.val[0]);
            at = dec_sort(3 * F, dec_bits(V), S, stream);
            dec_corner_ranges_kernel<<<dec_blocks(3 * F), DEC_BLOCK, 0, stream>>>(3 * F, S.key[at], V, corner_begin, corner_end);
        }
        DecPositionArgs a{};
        a.g = DecGrid{{lo_x, lo_y, lo_z}, voxel};
        a.n_vertices = V;
        a.n_faces = F;
        a.xyz = vertices;
        a.faces = faces;
        a.order = ws_at<const uint32_t>(workspace, D.order);
        a.start = ws_at<const uint32_t>(workspace, D.start);
        a.cluster_key = ws_at<const uint64_t>(workspace, D.cluster_key);
        a.corner = S.val[at];
        a.corner_begin = corner_begin;
        a.corner_end = corner_end;
        a.n_clusters = n_clusters;
        a.quadric = quadric ? 1 : 0;
        a.out = out_vertices;
        a.used_quadric = used_quadric;
        dec_position_kernel<<<(unsigned)((n_clusters + DEC_WAVES - 1) / DEC_WAVES), DEC_BLOCK, 0, stream>>>(a);
    }
    return launch_status("mesh_cluster_emit launch");
}

// ---- vertex normals and colours of an extracted mesh (meshattr.hip.h) ------------------------------------------------------
namespace {
unsigned attr_blocks(int32_t n) { return (unsigned)(((int64_t)n + MESHATTR_THREADS - 1) / MESHATTR_THREADS); }
}  // namespace

size_t pgr_mesh_vertex_normals_workspace_bytes(int32_t n_vertices) {
    return n_vertices < 1 ? 0 : (size_t)n_vertices * 3 * sizeof(int64_t);
}

int32_t pgr_mesh_vertex_normals(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, float* normals,
                                void* workspace, size_t workspace_bytes, void* stream_v) {
    if (n_vertices < 0 || n_faces < 0 || (n_faces > 0 && !faces)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_vertices == 0) return PGR_OK;                                     // (no vertex: nothing to write, no face is kept)
    if (!vertices || !normals || !workspace || reinterpret_cast<uintptr_t>(workspace) % sizeof(int64_t) != 0 ||
        workspace_bytes < pgr_mesh_vertex_normals_workspace_bytes(n_vertices))
        return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = as_stream(stream_v);
    auto* sums = static_cast<long long*>(workspace);
    if (!hip_ok(hipMemsetAsync(sums, 0, pgr_mesh_vertex_normals_workspace_bytes(n_vertices), stream), "memset normal sums"))
        return PGR_ERR_LAUNCH_FAILURE;
    if (n_faces > 0)
        vertex_normals_accumulate_kernel<<<attr_blocks(n_faces), MESHATTR_THREADS, 0, stream>>>(n_vertices, vertices, n_faces, faces,
                                                                                               sums);
    vertex_normals_finalize_kernel<<<attr_blocks(n_vertices), MESHATTR_THREADS, 0, stream>>>(n_vertices, sums, normals);
    return launch_status("mesh_vertex_normals launch");
}

int32_t pgr_mesh_vertex_colors(int32_t n_vertices, const float* vertices, const float* normals, int32_t n_views,
                               const PgrCamera* cameras, const float* color, const float* depth, const float* final_T,
                               float depth_tol, float alpha_min, float cos_min, const float* fill, float* colors, int32_t* seen,
                               void* stream_v) {
    if (n_vertices < 0 || n_views < 1 || n_views > TSDF_MAX_VIEWS || !cameras || !color || !depth || !final_T || !fill)
        return PGR_ERR_INVALID_ARGUMENT;
    if (!(alpha_min > 0.f) || !(depth_tol >= 0.f) || std::isnan(cos_min)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_vertices > 0 && (!vertices || !colors)) return PGR_ERR_INVALID_ARGUMENT;
    VertexColorArgs a{};
    if (!pack_pinhole_views(n_views, cameras, a, a.campos)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_vertices == 0) return PGR_OK;
    a.n_vertices = n_vertices;
    a.depth_tol = depth_tol;
    a.alpha_min = alpha_min;
    a.cos_min = cos_min;
    for (int k = 0; k < 3; ++k) a.fill[k] = fill[k];
    a.vertices = vertices;
    a.normals = normals;
    a.color = color;
    a.depth = depth;
    a.final_T = final_T;
    a.colors = colors;
    a.seen = seen;
    vertex_colors_kernel<<<attr_blocks(n_vertices), MESHATTR_THREADS, 0, as_stream(stream_v)>>>(a);
    return launch_status("mesh_vertex_colors launch");
}

namespace {
// the per-face atlas of meshattr.hip.h; width == 0: refused
struct AtlasLayout { int32_t cols, rows, width, height; };
AtlasLayout atlas_layout(int32_t n_faces, int32_t cell) {
    AtlasLayout L{};
    if (n_faces < 1 || cell < 4 || cell > ATLAS_MAX_SIDE) return L;
    const int64_t cells = ((int64_t)n_faces + 1) / 2;
    int64_t cols = (int64_t)std::sqrt((double)cells);
    while (cols * cols < cells) ++cols;
    while (cols > 1 && (cols - 1) * (cols - 1) >= cells) --cols;
    const int64_t rows = (cells + cols - 1) / cols;
    if (cols * cell > ATLAS_MAX_SIDE || rows * cell > ATLAS_MAX_SIDE) return L;
    L.cols = (int32_t)cols; L.rows = (int32_t)rows; L.width = (int32_t)(cols * cell); L.height = (int32_t)(rows * cell);
    return L;
}
}  // namespace

int32_t pgr_mesh_atlas_points(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, int32_t cell,
                              int32_t width, int32_t height, float* points, float* normals, int32_t* face_of_texel, void* stream_v) {
    const AtlasLayout L = atlas_layout(n_faces, cell);
    if (n_vertices < 0 || !L.width || width != L.width || height != L.height || !faces || (n_vertices > 0 && !vertices) || !points ||
        !normals || !face_of_texel)
        return PGR_ERR_INVALID_ARGUMENT;
    AtlasArgs a{};
    a.n_vertices = n_vertices; a.n_faces = n_faces; a.cell = cell; a.cols = L.cols; a.width = width; a.height = height;
    a.vertices = vertices; a.faces = faces;
    const size_t texels = (size_t)width * (size_t)height;
    atlas_points_kernel<<<(unsigned)((texels + MESHATTR_THREADS - 1) / MESHATTR_THREADS), MESHATTR_THREADS, 0, as_stream(stream_v)>>>(
        a, points, normals, face_of_texel);
    return launch_status("mesh_atlas_points launch");
}

int32_t pgr_mesh_atlas_pack(int32_t n_faces, int32_t cell, int32_t width, int32_t height, const int32_t* face_of_texel,
                            const float* colors, const int32_t* seen, const uint8_t* face_fill, const uint8_t* fill, uint8_t* texture,
                            int32_t* face_seen, void* stream_v) {
    const AtlasLayout L = atlas_layout(n_faces, cell);
    if (!L.width || width != L.width || height != L.height || !face_of_texel || !colors || !seen || !fill || !texture)
        return PGR_ERR_INVALID_ARGUMENT;
    AtlasPackArgs a{};
    a.n_faces = n_faces; a.cell = cell; a.cols = L.cols; a.width = width; a.height = height;
    a.n_cells = (long long)L.cols * L.rows;
    for (int d = 0; d < 3; ++d) a.fill[d] = fill[d];
    a.face_of_texel = face_of_texel; a.colors = colors; a.seen = seen; a.face_fill = face_fill;
    a.texture = texture; a.face_seen = face_seen;
    constexpr int per_block = ATLAS_PACK_THREADS / WAVE;
    atlas_pack_kernel<<<(unsigned)((a.n_cells + per_block - 1) / per_block), ATLAS_PACK_THREADS, 0, as_stream(stream_v)>>>(a);
    return launch_status("mesh_atlas_pack launch");
}

// ---- collision geometry: mesh distance fields, samples and sweeps (meshsdf.hip.h) ----------------------------------------
namespace {
bool unit_vector(const float* v) {
    if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) return false;
    const double n2 = (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2];
    return std::fabs(std::sqrt(n2) - 1.0) <= 1e-4;
}
}  // namespace

int32_t pgr_mesh_sdf(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, const PgrGrid* grid,
                     float* sdf, float* winding, void* stream_v) {
    if (!grid_ok(grid) || n_vertices < 0 || n_faces < 0 || !sdf) return PGR_ERR_INVALID_ARGUMENT;
    if (n_faces > 0 && (!faces || (n_vertices > 0 && !vertices))) return PGR_ERR_INVALID_ARGUMENT;
    const size_t n = grid_points(grid);
    mesh_sdf_kernel<<<(uint32_t)((n + SDF_THREADS - 1) / SDF_THREADS), SDF_THREADS, 0, as_stream(stream_v)>>>(
        mesh_grid(grid), vertices, n_vertices, faces, n_faces, sdf, winding);
    return launch_status("mesh_sdf launch");
}

int32_t pgr_sdf_sample(const PgrGrid* grid, const float* sdf, int64_t n_points, const float* points, float* values,
                       float* gradients, void* stream_v) {
    if (!grid_ok(grid) || !sdf || n_points < 0 || n_points > ((int64_t)1 << 38)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_points > 0 && (!points || !values)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_points == 0) return PGR_OK;
    sdf_sample_kernel<<<(uint32_t)((n_points + 255) / 256), 256, 0, as_stream(stream_v)>>>(
        mesh_grid(grid), sdf, (long long)n_points, points, values, gradients);
    return launch_status("sdf_sample launch");
}

int32_t pgr_sdf_sweep(int32_t n_bodies, const PgrSdfBody* bodies, int32_t n_jobs, const PgrSweepJob* jobs, float tol,
                      float max_travel, int32_t max_steps, uint64_t* out, void* stream_v) {
    if (n_bodies < 0 || n_jobs < 0 || max_steps < 0 || !(tol >= 0.f) || !(max_travel >= 0.f)) return PGR_ERR_INVALID_ARGUMENT;
    if ((n_bodies > 0 && !bodies) || (n_jobs > 0 && (!jobs || !out))) return PGR_ERR_INVALID_ARGUMENT;
    for (int32_t b = 0; b < n_bodies; ++b)
        if (bodies[b].n_shell < 0 || (bodies[b].n_shell > 0 && !bodies[b].shell)) return PGR_ERR_INVALID_ARGUMENT;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrSweepJob& j = jobs[k];
        if (j.mover < 0 || j.mover >= n_bodies || j.target < PGR_SWEEP_PLANE || j.target >= n_bodies || j.target == j.mover)
            return PGR_ERR_INVALID_ARGUMENT;
        if (!unit_vector(j.dir)) return PGR_ERR_INVALID_ARGUMENT;
        if (j.target == PGR_SWEEP_PLANE) {
            if (!unit_vector(j.plane) || !std::isfinite(j.plane[3])) return PGR_ERR_INVALID_ARGUMENT;
        } else if (!grid_ok(&bodies[j.target].grid) || !bodies[j.target].sdf) {
            return PGR_ERR_INVALID_ARGUMENT;
        }
    }
    if (n_jobs == 0) return PGR_OK;
    hipStream_t stream = as_stream(stream_v);
    sdf_sweep_init_kernel<<<(2 * n_jobs + 255) / 256, 256, 0, stream>>>(out, 2 * n_jobs);
    for (int32_t k0 = 0; k0 < n_jobs; k0 += SWEEP_JOBS_PER_LAUNCH) {
        SweepJobTable T{};
        T.count = std::min(SWEEP_JOBS_PER_LAUNCH, n_jobs - k0);
        T.first = k0;
        T.tol = tol;
        T.max_travel = max_travel;
        T.max_steps = max_steps;
        uint32_t blocks = 0;
        for (int32_t k = 0; k < T.count; ++k) {
            const PgrSweepJob& j = jobs[k0 + k];
            const PgrSdfBody& a = bodies[j.mover];
            SweepJobDev& d = T.job[k];
            d.shell = a.shell;
            d.n_shell = a.n_shell;
            std::memcpy(d.Ra, a.R, sizeof(d.Ra));
            std::memcpy(d.ta, a.t, sizeof(d.ta));
            std::memcpy(d.dir, j.dir, sizeof(d.dir));
            d.is_plane = j.target == PGR_SWEEP_PLANE;
            if (d.is_plane) {
                std::memcpy(d.plane, j.plane, sizeof(d.plane));
            } else {
                const PgrSdfBody& b = bodies[j.target];
                d.sdf = b.sdf;
                d.g = mesh_grid(&b.grid);
                std::memcpy(d.Rb, b.R, sizeof(d.Rb));
                std::memcpy(d.tb, b.t, sizeof(d.tb));
            }
            d.block0 = blocks;
            blocks += (uint32_t)(((int64_t)a.n_shell + SWEEP_THREADS - 1) / SWEEP_THREADS);
        }
        if (blocks > 0) sdf_sweep_kernel<<<blocks, SWEEP_THREADS, 0, stream>>>(T, out);
    }
    return launch_status("sdf_sweep launch");
}

// ---- rigid-body drops: field contacts and the batched impulse solver (rigid.hip.h) ------------------------------------------
namespace {
constexpr int32_t RIGID_MAX_WORLDS = 1 << 20;
struct RigidLayout { size_t table, words, halt, rest_count, rows, total; };
RigidLayout rigid_layout(int32_t S, int32_t B) {
    RigidLayout L{};
    if (S < 0 || S > RIGID_MAX_WORLDS || B < 0 || B > RIGID_MAX_BODIES) return L;
    const size_t pairs = (size_t)S * B * B;
    Carver c;
    L.table = c.take(sizeof(RigidTable));
    L.words = c.take(pairs * RIGID_WORDS * sizeof(uint64_t));
    L.halt = c.take((size_t)S * sizeof(int32_t));
    L.rest_count = c.take((size_t)S * sizeof(int32_t));
    L.rows = c.take(pairs * RIGID_WORDS * RIGID_ROW_FIELDS * sizeof(float));
    L.total = c.off;
    return L;
}
bool all_finite(const float* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}
// the checks both rigid entries share; fills the kernels' copies of the table and the parameters
bool rigid_args(const PgrRigidParams* p, int32_t n_types, const PgrRigidType* types, int32_t S, int32_t B, const int32_t* type,
                const float* state, RigidTable& T, RigidParamsDev& P) {
    if (!p || S < 0 || S > RIGID_MAX_WORLDS || B < 0 || B > RIGID_MAX_BODIES || n_types < 0 || n_types > RIGID_MAX_TYPES) return false;
    if (n_types > 0 && !types) return false;
    const bool slots = S > 0 && B > 0;
    if (slots && (!type || !state || n_types == 0)) return false;
    if (!std::isfinite(p->h) || !(p->h > 0.f) || p->iterations <= 0 || !all_finite(p->gravity, 3)) return false;
    if (!unit_vector(p->plane) || !std::isfinite(p->plane[3])) return false;
    for (float v : {p->plane_friction, p->beta, p->slop, p->margin, p->v_sleep, p->w_sleep})
        if (!std::isfinite(v) || v < 0.f) return false;
    for (float v : {p->lin_damp, p->ang_damp})
        if (!std::isfinite(v) || v < 0.f || !(v < 1.f)) return false;
    T = RigidTable{};
    for (int32_t k = 0; k < n_types; ++k) {
        const PgrRigidType& t = types[k];
        if (t.n_shell < 0 || (t.n_shell > 0 && !t.shell)) return false;
        if (B > 1 && (!t.sdf || !grid_ok(&t.grid))) return false;
        if (!std::isfinite(t.mass) || !(t.mass > 0.f) || !std::isfinite(t.friction) || t.friction < 0.f) return false;
        if (!std::isfinite(t.radius) || t.radius < 0.f || !all_finite(t.com, 3) || !all_finite(t.inv_inertia, 9)) return false;
        RigidTypeDev& d = T.t[k];
        if (t.sdf && grid_ok(&t.grid)) {
            d.g = mesh_grid(&t.grid);
            d.sdf = t.sdf;
        }
        d.mass = t.mass;
        d.shell = t.shell;
        d.n_shell = t.n_shell;
        d.friction = t.friction;
        d.radius = t.radius;
        std::memcpy(d.com, t.com, sizeof(d.com));
        std::memcpy(d.iinv, t.inv_inertia, sizeof(d.iinv));
    }
    P = RigidParamsDev{};
    P.h = p->h;
    P.gx = p->gravity[0];
    P.gy = p->gravity[1];
    P.gz = p->gravity[2];
    P.nx = p->plane[0];
    P.ny = p->plane[1];
    P.nz = p->plane[2];
    P.d = p->plane[3];
    P.plane_friction = p->plane_friction;
    P.lin_factor = (float)std::pow(1.0 - (double)p->lin_damp, (double)p->h);
    P.ang_factor = (float)std::pow(1.0 - (double)p->ang_damp, (double)p->h);
    P.beta = p->beta;
    P.slop = p->slop;
    P.margin = p->margin;
    P.v_sleep = p->v_sleep;
    P.w_sleep = p->w_sleep;
    P.iterations = p->iterations;
    P.sleep_steps = p->sleep_steps;
    P.n_types = n_types;
    return true;
}
// the ground of the *_ground entries: NULL is the plane (G.sdf stays NULL)
bool rigid_ground(const PgrRigidGround* ground, RigidGroundDev& G) {
    G = RigidGroundDev{};
    if (!ground) return true;
    if (!ground->sdf || !grid_ok(&ground->grid) || !std::isfinite(ground->friction) || ground->friction < 0.f) return false;
    G.g = mesh_grid(&ground->grid);
    G.sdf = ground->sdf;
    G.friction = ground->friction;
    return true;
}
// one pass of rigid_contacts_kernel over every (world, pair, point block); halt may be NULL
void rigid_launch_contacts(const RigidTable& T, const RigidTypeDev* table, const RigidParamsDev& P, const RigidGroundDev& G,
                           int32_t n_types, int32_t S, int32_t B, const int32_t* type,
                           const float* state, const int32_t* halt, uint64_t* words, hipStream_t stream) {
    int32_t most = 0;
    for (int32_t k = 0; k < n_types; ++k) most = std::max(most, T.t[k].n_shell);
    const uint32_t point_blocks = (uint32_t)(((int64_t)most + RIGID_CONTACT_THREADS - 1) / RIGID_CONTACT_THREADS);
    if (point_blocks == 0) return;
    const dim3 blocks((uint32_t)S, (uint32_t)(B * B), point_blocks);
    if (G.sdf)
        rigid_contacts_kernel<true><<<blocks, RIGID_CONTACT_THREADS, 0, stream>>>(table, P, G, B, type, state, halt, words);
    else
        rigid_contacts_kernel<false><<<blocks, RIGID_CONTACT_THREADS, 0, stream>>>(table, P, G, B, type, state, halt, words);
}
}  // namespace

size_t pgr_rigid_workspace_bytes(int32_t n_worlds, int32_t n_slots) { return rigid_layout(n_worlds, n_slots).total; }

int32_t pgr_rigid_contacts(const PgrRigidParams* params, int32_t n_types, const PgrRigidType* types, int32_t S, int32_t B,
                           const int32_t* type, const float* state, uint64_t* words, void* workspace, size_t workspace_bytes,
                           void* stream_v) {
    return pgr_rigid_contacts_ground(params, nullptr, n_types, types, S, B, type, state, words, workspace, workspace_bytes, stream_v);
}

int32_t pgr_rigid_contacts_ground(const PgrRigidParams* params, const PgrRigidGround* ground, int32_t n_types,
                                  const PgrRigidType* types, int32_t S, int32_t B, const int32_t* type, const float* state,
                                  uint64_t* words, void* workspace, size_t workspace_bytes, void* stream_v) {
    RigidTable T;
    RigidParamsDev P;
    RigidGroundDev G;
    if (!rigid_args(params, n_types, types, S, B, type, state, T, P) || !rigid_ground(ground, G)) return PGR_ERR_INVALID_ARGUMENT;
    if (S == 0 || B == 0) return PGR_OK;
    if (!words || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    const RigidLayout L = rigid_layout(S, B);
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    for (int32_t k = 0; k < n_types; ++k)
        if ((int64_t)T.t[k].n_shell > (int64_t)65535 * RIGID_CONTACT_THREADS) return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = as_stream(stream_v);
    const long long n_words = (long long)S * B * B * RIGID_WORDS;
    RigidTypeDev* table = ws_at<RigidTypeDev>(workspace, L.table);
    rigid_table_kernel<<<1, WAVE, 0, stream>>>(T, table);
    rigid_init_kernel<<<(uint32_t)((n_words + 255) / 256), 256, 0, stream>>>(words, n_words, nullptr, nullptr, nullptr, nullptr, 0);
    rigid_launch_contacts(T, table, P, G, n_types, S, B, type, state, nullptr, words, stream);
    return launch_status("rigid_contacts launch");
}

int32_t pgr_rigid_simulate(const PgrRigidParams* params, int32_t n_types, const PgrRigidType* types, int32_t S, int32_t B,
                           const int32_t* type, float* state, int32_t n_steps, int32_t record_every, float* trajectory,
                           int32_t* rest_step, int32_t* status, void* workspace, size_t workspace_bytes, void* stream_v) {
    return pgr_rigid_simulate_ground(params, nullptr, n_types, types, S, B, type, state, n_steps, record_every, trajectory, rest_step,
                                     status, workspace, workspace_bytes, stream_v);
}

int32_t pgr_rigid_simulate_ground(const PgrRigidParams* params, const PgrRigidGround* ground, int32_t n_types,
                                  const PgrRigidType* types, int32_t S, int32_t B, const int32_t* type, float* state, int32_t n_steps,
                                  int32_t record_every, float* trajectory, int32_t* rest_step, int32_t* status, void* workspace,
                                  size_t workspace_bytes, void* stream_v) {
    RigidTable T;
    RigidParamsDev P;
    RigidGroundDev G;
    if (!rigid_args(params, n_types, types, S, B, type, state, T, P) || !rigid_ground(ground, G)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_steps < 0 || record_every < 1) return PGR_ERR_INVALID_ARGUMENT;
    if (S == 0 || B == 0) return PGR_OK;
    const int32_t n_records = n_steps / record_every;
    if (!rest_step || !status || !workspace || (n_records > 0 && !trajectory)) return PGR_ERR_INVALID_ARGUMENT;
    if (!workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    for (int32_t k = 0; k < n_types; ++k)
        if ((int64_t)T.t[k].n_shell > (int64_t)65535 * RIGID_CONTACT_THREADS) return PGR_ERR_INVALID_ARGUMENT;
    const RigidLayout L = rigid_layout(S, B);
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    uint64_t* words = ws_at<uint64_t>(workspace, L.words);
    int32_t* halt = ws_at<int32_t>(workspace, L.halt);
    int32_t* rest_count = ws_at<int32_t>(workspace, L.rest_count);
    float* rows = ws_at<float>(workspace, L.rows);
    RigidTypeDev* table = ws_at<RigidTypeDev>(workspace, L.table);
    rigid_table_kernel<<<1, WAVE, 0, stream>>>(T, table);
    const long long n_words = (long long)S * B * B * RIGID_WORDS;
    const long long n_init = std::max<long long>(n_words, S);
    rigid_init_kernel<<<(uint32_t)((n_init + 255) / 256), 256, 0, stream>>>(words, n_words, halt, rest_count, rest_step, status, S);
    const uint32_t solve_blocks = (uint32_t)((S + RIGID_SOLVE_THREADS - 1) / RIGID_SOLVE_THREADS);
    for (int32_t k = 0; k < n_steps; ++k) {
        rigid_launch_contacts(T, table, P, G, n_types, S, B, type, state, halt, words, stream);
        const int32_t record = (k + 1) % record_every == 0 ? (k + 1) / record_every - 1 : -1;
        if (G.sdf)
            rigid_solve_kernel<true><<<solve_blocks, RIGID_SOLVE_THREADS, 0, stream>>>(
                table, P, G, S, B, type, state, words, rows, halt, rest_count, k, record, n_records, trajectory, rest_step, status);
        else
            rigid_solve_kernel<false><<<solve_blocks, RIGID_SOLVE_THREADS, 0, stream>>>(
                table, P, G, S, B, type, state, words, rows, halt, rest_count, k, record, n_records, trajectory, rest_step, status);
    }
    return launch_status("rigid_simulate launch");
}
