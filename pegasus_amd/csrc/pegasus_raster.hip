// pegasus_raster.hip -- the rasterizer's share of the C ABI of libpegasus_raster.so (see include/pegasus_raster.h): version,
// status and error strings, forward and backward, object posing, block visibility, frame packing.  The other kernel families
// have a translation unit each (pointcloud.hip, mesh.hip, eval.hip, train.hip; DESIGN.md "Source layout").
// gfx950 only.  Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -shared -fPIC
//
// Pipeline of one batch of views of one scene (all stages enqueued on the caller's stream, no host
// round trip until the end-of-batch status read):
//   per view : pack_camera, preprocess                           (preprocess.hip.h)
//   batch    : bin_count -> tile_scan -> bin_scatter -> work order -> tile_sort, one launch per tier   (tilebin.hip.h, tilesort.hip.h)
//   batch    : composite_wave over every (view, tile, half) work item, longest lists first (composite.hip.h)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "backward.hip.h"
#include "blockcull.hip.h"
#include "compose.hip.h"
#include "composite.hip.h"
#include "host_common.h"
#include "pgr_common.h"
#include "preprocess.hip.h"
#include "tilebin.hip.h"
#include "tilesort.hip.h"

namespace pgr {

// Calls of one or two views (the drop-in GaussianRasterizer: one camera per call) cannot fill the chip; their launches are
// latency-bound and get a few arrangements of their own (fewer, fuller launches).  Results never depend on it.
constexpr int SMALL_BATCH_VIEWS = 2;
#ifndef PGR_PRE_SMALL_SCENE
#define PGR_PRE_SMALL_SCENE 400000
#endif
constexpr int PRE_SMALL_SCENE = PGR_PRE_SMALL_SCENE;   // Gaussians: below this the preprocess spreads a batch's views over gridDim.y ...
constexpr int PRE_VIEW_GROUP = 8;         // ... in groups of this many

// A/B switch for tests and measurements (read per call; results never depend on it)
static bool block_cull_enabled() {
    const char* e = getenv("PGR_BLOCK_CULL");
    return !(e && e[0] == '0');
}


// Does a batch call of this shape run the block test (blockcull.hip.h) inside its preprocess?  Not when it is switched off,
// not for one- and two-view calls (bounding the blocks costs their latency-bound preprocess more than it returns), and not
// when a small scene's views are spread over gridDim.y (split_views_shape: the visibility words hold 32 views).  The one
// place this is decided: forward_batch_impl and pgr_workspace_block_visibility both ask here.
static bool split_views_shape(int n, int n_views) { return n <= PRE_SMALL_SCENE && n_views >= 2 * PRE_VIEW_GROUP; }
static bool call_runs_block_cull(int n, int n_views) {
    return block_cull_enabled() && n_views > SMALL_BATCH_VIEWS && !split_views_shape(n, n_views);
}

static bool records_enabled() {      // PGR_BIN_RECORDS=0: the scatter walk re-evaluates every candidate (A/B, tests)
    const char* e = getenv("PGR_BIN_RECORDS");
    return !(e && e[0] == '0');
}

// layers > 1 (PgrForwardCall::layers): the view is `layers` stacked copies of the tile grid -- per-(tile, layer) lists
static Layout make_layout(int32_t n, int32_t width, int32_t height, int64_t max_instances, int32_t layers = 1) {
    Layout L{};
    const size_t N = (size_t)(n > 0 ? n : 0), I = (size_t)(max_instances > 0 ? max_instances : 0);
    const int gx = (width + TILE - 1) / TILE, gy = (height + TILE - 1) / TILE * (layers > 1 ? layers : 1);
    L.tiles = gx * gy;
    L.grid_x = gx;
    L.grid_y = gy;
    L.n_blocks = (int)((N + PRE_BLOCK - 1) / PRE_BLOCK);
    L.n_chunks = (int)((N + BIN_CHUNK - 1) / BIN_CHUNK);
    Carver c;
    L.splats = c.take(N * 48);
    L.radii = c.take(N * 4);
    L.rects = c.take(N * 8);
    L.crects = c.take(N * 8);
    L.rel = c.take((size_t)L.n_chunks * L.tiles * 4);
    L.ranges = c.take((size_t)L.tiles * 8);
    L.bucket = c.take(I * 8);
    L.alt = c.take(I * 8);
    L.gauss_sorted = c.take(I * 4);
    L.total = c.off;
    L.max_instances = (int64_t)I;
    return L;
}

static int check_scene(const PgrScene* s) {
    if (!s || s->n < 0) return PGR_ERR_INVALID_ARGUMENT;
    if (s->n == 0) return PGR_OK;
    if (!s->means3d || !s->opacities) return PGR_ERR_INVALID_ARGUMENT;
    if ((s->shs == nullptr) == (s->colors_precomp == nullptr)) return PGR_ERR_INVALID_ARGUMENT;
    const bool have_sr = s->scales != nullptr && s->rotations != nullptr;
    if (have_sr == (s->cov3d_precomp != nullptr)) return PGR_ERR_INVALID_ARGUMENT;
    if (s->shs && (s->sh_degree < 0 || s->sh_degree > 3 || s->sh_stride < (s->sh_degree + 1) * (s->sh_degree + 1)))
        return PGR_ERR_INVALID_ARGUMENT;
    if (s->shs_rest && (!s->shs || s->sh_stride < 2)) return PGR_ERR_INVALID_ARGUMENT;   // split layout: dc + at least one more
    return PGR_OK;
}

// Batch header placed in front of the per-view slices.
// The host scratch: the image of the three pointer tables (laid out exactly as in the workspace's `tables`: one H2D copy),
// then the status words read back -- per view [0] listed instances, [1] overflow flag.
struct HostTables { size_t view_table, bin_table, pre_table, tables_bytes, status, total; };

static HostTables host_tables(int n_views) {
    HostTables T{};
    T.bin_table = T.view_table + align_up((size_t)n_views * sizeof(ViewEntry), 16);
    T.pre_table = T.bin_table + align_up((size_t)n_views * sizeof(BinView), 16);
    T.tables_bytes = T.status = T.pre_table + align_up((size_t)n_views * sizeof(PreOut), 16);
    T.total = T.status + (size_t)n_views * 8;
    return T;
}

// Batch header placed in front of the per-view slices.
struct BatchLayout {
    size_t tables, cams, status, tile_counts, order_state, work_order, long_list, tie_inv, vis, obj_u8, views, total;
    int n_groups, vis_words;
    HostTables host;             // offsets inside `tables`
    size_t order_slots;
    size_t seg_cap;              // entries of the segment queue (behind the SORT_TIERS tier queues)
    size_t per_view;
};

static BatchLayout make_batch_layout(const Layout& L, int n_views, size_t n_scene) {
    BatchLayout B{};
    Carver c;
    B.host = host_tables(n_views);
    B.tables = c.take(B.host.tables_bytes);
    B.cams = c.take((size_t)n_views * sizeof(CameraDev));
    B.status = c.take((size_t)n_views * 8);        // per view: [0] listed instances, [1] overflow flag
    B.tile_counts = c.take((size_t)n_views * L.tiles * 8);   // [tile_count u32 | obj_last u32] x views: one memset
    B.order_state = c.take(ORDER_STATE_WORDS * 4);
    // NUM_XCD interleaved streams; each holds the items of its band of tile rows for every view
    B.order_slots = (size_t)NUM_XCD * max_band_rows(L.grid_y) * L.grid_x * ITEMS_PER_TILE * n_views;
    B.work_order = c.take(B.order_slots * 4);
    // the sort queues: one per tier, and the segment queue of the split pre-pass -- a list of n > SORT_WINDOW_MAX keys yields
    // at most n / SEG_HALF + 2 <= n (1 / 4096 + 2 / 15872) = n / 2702 segments, and a view's lists hold max_instances keys
    B.seg_cap = (size_t)n_views * ((size_t)(L.max_instances > 0 ? L.max_instances : 0) / 2702 + 2);
    B.long_list = c.take(((size_t)n_views * L.tiles * SORT_TIERS + B.seg_cap) * sizeof(uint4));
    B.tie_inv = c.take((size_t)n_scene * 4);    // inverse of PgrScene::tie_index (filled only when one is given)
    B.n_groups = (int)((n_scene + WAVE - 1) / WAVE);
    B.vis_words = (n_views + 31) / 32;
    B.vis = c.take((size_t)B.n_groups * B.vis_words * 4);
    B.obj_u8 = c.take(n_scene);                // object ids as bytes (fused semantic pass)
    B.views = c.off;
    B.per_view = align_up(L.total);
    B.total = B.views + (size_t)n_views * B.per_view;
    return B;
}

// One view's share of a workspace: its slice behind the batch header, and its entries of the header's per-view arrays
// (the cameras of a batch are contiguous: the preprocess walks them; so are the status words: one D2H copy per batch).
struct ViewWs {
    CameraDev* cam;       // batch header
    uint32_t* counters;   // batch header: [0] listed instances, [1] overflow flag
    float4* splats;   // [n,3] per-Gaussian records
    uint2 *rects, *crects;
    uint32_t *tile_count, *rel;   // tile_count: batch header
    uint2* ranges;
    uint2* bucket;
    uint64_t* alt;
    uint32_t* gauss_sorted;
    uint32_t* obj_last;   // batch header
};

static ViewWs view_slice(char* ws, const Layout& L, const BatchLayout& B, int n_views, int v) {
    char* const slice = ws + B.views + (size_t)v * B.per_view;
    auto* const tile_counts = ws_at<uint32_t>(ws, B.tile_counts);
    ViewWs w;
    w.cam = ws_at<CameraDev>(ws, B.cams) + v;
    w.counters = ws_at<uint32_t>(ws, B.status) + 2 * v;
    w.splats = ws_at<float4>(slice, L.splats);
    w.rects = ws_at<uint2>(slice, L.rects);
    w.crects = ws_at<uint2>(slice, L.crects);
    w.tile_count = tile_counts + (size_t)v * L.tiles;
    w.rel = ws_at<uint32_t>(slice, L.rel);
    w.ranges = ws_at<uint2>(slice, L.ranges);
    w.bucket = ws_at<uint2>(slice, L.bucket);
    w.alt = ws_at<uint64_t>(slice, L.alt);
    w.gauss_sorted = ws_at<uint32_t>(slice, L.gauss_sorted);
    w.obj_last = tile_counts + (size_t)(n_views + v) * L.tiles;
    return w;
}

static bool camera_ok(const PgrCamera& c) {      // what every entry that packs cameras asks of one
    return c.image_width > 0 && c.image_height > 0 && c.tanfovx > 0.f && c.tanfovy > 0.f && c.viewmatrix && c.projmatrix &&
           c.campos && c.bg;
}

// The launch argument that packs up to CAM_PACK_MAX cameras (pack_camera: preprocess.hip.h).
static CamPack pack_cameras(const PgrCamera* cams, int cnt, bool with_depth_mode) {
    CamPack cp;
    for (int k = 0; k < cnt; ++k) {
        const PgrCamera& c = cams[k];
        cp.view[k] = c.viewmatrix; cp.proj[k] = c.projmatrix; cp.campos[k] = c.campos; cp.bg[k] = c.bg;
        cp.tanfovx[k] = c.tanfovx; cp.tanfovy[k] = c.tanfovy; cp.depth_mode[k] = with_depth_mode ? c.depth_mode : 0;
    }
    return cp;
}

static PgrRecordLayout record_layout(size_t P, int k) {       // one view's frame record (pgr_frame_record_layout)
    PgrRecordLayout R;
    R.off_rgb = 0;
    R.off_depth = (int64_t)align_up(3 * P, 16);
    R.off_masks = R.off_depth + (int64_t)align_up(2 * P, 16);
    R.bytes = R.off_masks + (int64_t)align_up((size_t)((k + 7) / 8) * P, 16);
    return R;
}

static int check_camera(const PgrCamera* cam, const PgrOutputs* out, bool layered = false) {
    if (!cam || !out || !camera_ok(*cam) ||
        // color + depth, or (records-only view) the frame record alone; a layered call writes mask planes only
        (layered ? !out->sem_masks : !((out->color && out->depth) || (out->record && !out->color && !out->depth))) ||
        (cam->depth_mode != PGR_DEPTH_EXPECTED && cam->depth_mode != PGR_DEPTH_NORMALIZED))
        return PGR_ERR_INVALID_ARGUMENT;
    // tile coordinates are packed into 16 bits
    if ((cam->image_width + TILE - 1) / TILE > 0xffff || (cam->image_height + TILE - 1) / TILE > 0xffff)
        return PGR_ERR_INVALID_ARGUMENT;
    return PGR_OK;
}

static int zero_outputs(const PgrOutputs* out, size_t P, hipStream_t stream, int n_masks) {
    const struct { void* p; size_t bytes; const char* what; } fills[] = {
        {out->color, 3 * P * sizeof(float), "memset color"}, {out->depth, P * sizeof(float), "memset depth"},
        {n_masks > 0 ? out->sem_masks : nullptr, (size_t)n_masks * P, "memset masks"},
        {out->record, (size_t)record_layout(P, n_masks).bytes, "memset record"},
        {out->final_T, P * sizeof(float), "memset T"}, {out->n_contrib, P * sizeof(uint32_t), "memset n"},
        {out->sem_color, 3 * P * sizeof(float), "memset sem"}, {out->sem_depth, P * sizeof(float), "memset semd"}};
    for (const auto& f : fills)
        if (f.p && !hip_ok(hipMemsetAsync(f.p, 0, f.bytes, stream), f.what)) return PGR_ERR_LAUNCH_FAILURE;
    return PGR_OK;
}

// The batch header in ONE launch: tile counters | obj_last and the work-order state cleared, the work order invalid, the first
// CAM_PACK_MAX cameras packed, and -- one- and two-view calls -- the pointer tables written from the launch arguments.  A
// single-view call lasts 0.45 ms on the GPU: the H2D copy of its 300 bytes of tables and the camera launch were 10 us of it.
constexpr int HEADER_TABLE_WORDS = 256;
struct HeaderTables { uint32_t w[HEADER_TABLE_WORDS]; };
__global__ __launch_bounds__(256) void batch_header_kernel(uint32_t* __restrict__ zero, size_t n_zero, uint32_t* __restrict__ ff,
                                                           size_t n_ff, CamPack cams, int cam_count, int width, int height,
                                                           CameraDev* __restrict__ cams_out, HeaderTables tables,
                                                           uint32_t* __restrict__ tables_out, int table_words) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_zero; i += stride) gstore(zero + i, 0u);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ff; i += stride) gstore(ff + i, INVALID_ITEM);
    if ((int)blockIdx.x < cam_count && threadIdx.x < 64)
        pack_camera(cams, (int)blockIdx.x, (int)threadIdx.x, width, height, cams_out + blockIdx.x);
    if (blockIdx.x == gridDim.x - 1)
        for (int i = threadIdx.x; i < table_words; i += blockDim.x) gstore(tables_out + i, tables.w[i]);
}

// What a call adds to the plain batch; every field is optional.
struct ForwardOptions {
    hipEvent_t* ev = nullptr;             // PGR_NUM_STAGES+1 events recorded at the stage boundaries (a call with stage_ms)
    // NULL = synchronous call (tables staged from pageable memory, stream synchronised at the end, num_instances
    // filled).  Non-NULL = pinned host memory of host_scratch_bytes(n_views): nothing blocks, the status words land in
    // its tail when the stream reaches them (pgr_batch_status reads them).
    void* host_scratch = nullptr;
    const PgrSemantic* semantic = nullptr;
    const PgrPosedObjects* posed = nullptr;
    const PgrLayers* layers = nullptr;
    hipEvent_t status_event = nullptr;    // recorded behind the tile scan, which stores the status words itself
};

// The whole hot path for a batch of views of ONE scene.  All views share the image size.
static int32_t forward_batch_impl(const PgrScene* scene, int n_views, const PgrCamera* cams, const PgrOutputs* outs,
                                  void* workspace, size_t workspace_bytes, int64_t max_instances,
                                  int64_t* num_instances, hipStream_t stream, const ForwardOptions& opt = {}) {
    hipEvent_t* const ev = opt.ev;
    void* const host_scratch = opt.host_scratch;
    const PgrSemantic* const semantic = opt.semantic;
    const PgrPosedObjects* const posed = opt.posed;
    const PgrLayers* const layers = opt.layers;
    const hipEvent_t status_event = opt.status_event;
    auto mark = [&](int k) { if (ev) (void)hipEventRecord(ev[k], stream); };
    // every argument check happens here, before the first enqueue: an early return below this block would leave work
    // on the stream that still reads the (pageable) table staging of the synchronous path
    // (per-Gaussian arrays of an EMPTY scene may be NULL: torch hands out a null pointer for an empty tensor)
    const bool empty = scene && scene->n == 0;
    if (posed && ((!posed->object_id && !empty) || !posed->poses || posed->k_objects <= 0 ||
                  (scene && (scene->cov3d_precomp || scene->shs_rest))))
        return PGR_ERR_INVALID_ARGUMENT;
    if (semantic && ((!semantic->object_id && !empty) || !semantic->colors || semantic->n_env < 0 || semantic->k_objects <= 0))
        return PGR_ERR_INVALID_ARGUMENT;
    if (layers && (semantic || (!layers->layer_id && !empty) || !layers->mask_colors || layers->n_layers <= 0 || layers->n_layers > 4096))
        return PGR_ERR_INVALID_ARGUMENT;
    if (n_views <= 0 || !cams || !outs) return PGR_ERR_INVALID_ARGUMENT;
    if (num_instances) for (int v = 0; v < n_views; ++v) num_instances[v] = 0;
    if (int rc = check_scene(scene)) return rc;
    if (max_instances < 0 || max_instances > 0x7fffffffLL) return PGR_ERR_INVALID_ARGUMENT;
    const int W = cams[0].image_width, H = cams[0].image_height, N = scene->n;
    for (int v = 0; v < n_views; ++v) {
        if (int rc = check_camera(&cams[v], &outs[v], layers != nullptr)) return rc;
        if (cams[v].image_width != W || cams[v].image_height != H) return PGR_ERR_INVALID_ARGUMENT;
        // a semantic descriptor asks for the objects-only image of EVERY view of the batch
        // (a records-only view takes it as the mask planes of its record instead: no image, but then the colours to
        // threshold against must be there)
        if (semantic && !outs[v].sem_color && !(outs[v].record && !outs[v].color && semantic->mask_colors && !outs[v].sem_depth))
            return PGR_ERR_INVALID_ARGUMENT;
        // masks in the compositor's epilogue need the colours to threshold against
        if (!layers && outs[v].sem_masks && !(semantic && semantic->mask_colors)) return PGR_ERR_INVALID_ARGUMENT;
    }
    const int n_layers = layers ? layers->n_layers : 1;
    if (layers && (size_t)n_layers * ((H + TILE - 1) / TILE) > 0xffffu) return PGR_ERR_INVALID_ARGUMENT;   // 16-bit tile rows
    const size_t P = (size_t)W * H;
    // failure after the first enqueue: the synchronous path drains the stream before its staging memory goes away
    auto fail = [&](int32_t rc) {
        if (!host_scratch) (void)hipStreamSynchronize(stream);
        return rc;
    };

    // N == 0: outputs stay zero-filled, no background (SURVEY.md section 8a "Edge cases")
    if (N == 0) {
        for (int v = 0; v < n_views; ++v)
            if (int rc = zero_outputs(&outs[v], P, stream, layers ? n_layers : (semantic && semantic->mask_colors ? semantic->k_objects : 0))) return rc;
        if (status_event && !hip_ok(hipEventRecord(status_event, stream), "record status event")) return PGR_ERR_LAUNCH_FAILURE;
        return PGR_OK;
    }

    if (!workspace) return PGR_ERR_INVALID_ARGUMENT;
    const Layout L = make_layout(N, W, H, max_instances, n_layers);
    const int layer_tiles = L.tiles / n_layers, layer_rows = L.grid_y / n_layers;
    if (layers && layer_tiles > BIN_LDS_TILES) return PGR_ERR_INVALID_ARGUMENT;     // one layer per LDS pass
    const BatchLayout B = make_batch_layout(L, n_views, (size_t)N);
    if (workspace_bytes < B.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    char* ws = static_cast<char*>(workspace);
    auto* view_table = ws_at<ViewEntry>(ws, B.tables + B.host.view_table);
    auto* bin_table = ws_at<BinView>(ws, B.tables + B.host.bin_table);
    auto* pre_table = ws_at<PreOut>(ws, B.tables + B.host.pre_table);
    auto* cams_dev = ws_at<CameraDev>(ws, B.cams);
    auto* status_dev = ws_at<uint32_t>(ws, B.status);
    auto* order_state = ws_at<uint32_t>(ws, B.order_state);
    auto* sort_queue = ws_at<uint4>(ws, B.long_list);
    auto* work_order = ws_at<uint32_t>(ws, B.work_order);
    std::vector<ViewWs> vw((size_t)n_views);
    std::vector<char> pageable;
    char* hs = static_cast<char*>(host_scratch);
    if (!hs) {
        pageable.resize(B.host.total);
        hs = pageable.data();
    }
    auto* table = ws_at<ViewEntry>(hs, B.host.view_table);
    auto* bins = ws_at<BinView>(hs, B.host.bin_table);
    auto* pres = ws_at<PreOut>(hs, B.host.pre_table);
    auto* h_status = ws_at<uint32_t>(hs, B.host.status);
    bool want_aux = false, want_sem = false;
    // the count walk's verdicts live where the sort's outputs will (alt, gauss_sorted: contiguous, dead until the sort)
    const size_t verdict_room = (L.total - L.alt) / (VERDICT_REGION_WORDS * 4);
    const int verdict_groups = layer_tiles <= BIN_LDS_TILES && records_enabled()
                                   ? (int)std::min<size_t>(verdict_room, (size_t)(N + WAVE - 1) / WAVE) : 0;
    for (int v = 0; v < n_views; ++v) {
        vw[v] = view_slice(ws, L, B, n_views, v);
        ViewEntry& e = table[v];
        memset(&e, 0, sizeof(e));
        e.cam = vw[v].cam; e.ranges = vw[v].ranges; e.gauss_sorted = vw[v].gauss_sorted; e.splats = vw[v].splats;
        e.out = CompOut{outs[v].color, outs[v].depth, outs[v].final_T, outs[v].n_contrib};
        e.counters = vw[v].counters;
        // fused semantic pass: the same walk also accumulates the objects-only image
        e.sem_color = semantic ? outs[v].sem_color : nullptr;
        e.sem_depth = semantic ? outs[v].sem_depth : nullptr;
        e.obj_last = vw[v].obj_last;
        e.sem_masks = (semantic || layers) ? outs[v].sem_masks : nullptr;
        e.record = layers ? nullptr : outs[v].record;
        want_sem = want_sem || e.sem_color || (semantic && e.record);
        want_aux = want_aux || outs[v].final_T || outs[v].n_contrib;
        bins[v] = BinView{vw[v].crects, vw[v].splats, vw[v].tile_count, vw[v].rel, vw[v].ranges,
                          vw[v].counters, vw[v].bucket, vw[v].gauss_sorted, vw[v].alt, vw[v].obj_last,
                          semantic ? semantic->n_env : -1, scene->tie_index,
                          scene->tie_index ? (scene->tie_inv ? scene->tie_inv : ws_at<const uint32_t>(ws, B.tie_inv)) : nullptr,
                          reinterpret_cast<uint2*>(vw[v].alt)};
        // radii and the reference-style 3-sigma rectangles are per-view OUTPUTS: written only when the caller asks for
        // radii (12 N bytes per view the frame path never reads; pgr_workspace_view's `rects` is valid only then)
        pres[v] = PreOut{vw[v].splats, outs[v].radii ? vw[v].rects : nullptr, vw[v].crects, outs[v].radii};
    }
    // the pointer tables: in the header launch's arguments when they are small (one / two views), else one H2D copy
    HeaderTables header_tables;
    int table_words = 0;
    if (n_views <= SMALL_BATCH_VIEWS && B.host.tables_bytes <= sizeof(header_tables)) {
        memcpy(header_tables.w, hs, B.host.tables_bytes);
        table_words = (int)(B.host.tables_bytes / 4);
    } else if (!hip_ok(hipMemcpyAsync(ws + B.tables, hs, B.host.tables_bytes, hipMemcpyHostToDevice, stream), "memcpy tables"))
        return fail(PGR_ERR_LAUNCH_FAILURE);

    // ---- stage 0: batch header (+ cameras) + per-Gaussian preprocess
    mark(0);
    static_assert(ORDER_STATE_WORDS * 4 <= 256, "order state fits its slot");
    {
        const int cnt = std::min(CAM_PACK_MAX, n_views);
        batch_header_kernel<<<256, 256, 0, stream>>>(ws_at<uint32_t>(ws, B.tile_counts), (B.work_order - B.tile_counts) / 4,
            ws_at<uint32_t>(ws, B.work_order), B.order_slots, pack_cameras(cams, cnt, true), cnt, W, H, cams_dev, header_tables,
            ws_at<uint32_t>(ws, B.tables), table_words);
    }
    if (scene->tie_index && !scene->tie_inv)     // (a per-scene constant: pgr_scene_prepare computes it once)
        invert_tie_index_kernel<<<(N + 255) / 256, 256, 0, stream>>>(N, scene->tie_index, ws_at<uint32_t>(ws, B.tie_inv));
    for (int v0 = CAM_PACK_MAX; v0 < n_views; v0 += CAM_PACK_MAX) {
        const int cnt = std::min(CAM_PACK_MAX, n_views - v0);
        pack_camera_kernel<<<cnt, 64, 0, stream>>>(pack_cameras(cams + v0, cnt, true), W, H, cams_dev + v0);
    }
    // which 64-Gaussian blocks can show up in which view: decided by the preprocess waves themselves (conservative;
    // PGR_BLOCK_CULL=0 switches the test off), left in `vis` for the binning walks
    // (one- and two-view calls skip it: bounding the blocks costs their latency-bound preprocess more than the skipped
    // work returns -- 98 -> 88 us for a single view of the 2 M-Gaussian scene)
    // small scene, many views (an objects-only pass, a single object): the batch's views are spread over gridDim.y in groups of
    // PRE_VIEW_GROUP instead of walked by one wave -- 200 k Gaussians are 3 000 waves, a quarter of what the chip holds, and 32
    // views in a row per wave cost 0.31 ms where the arithmetic is 0.1.  Block culling is off there (its words hold 32 views).
    const bool split_views = split_views_shape(N, n_views);
    const int view_groups = split_views ? (n_views + PRE_VIEW_GROUP - 1) / PRE_VIEW_GROUP : 1;
    const int views_per_block = split_views ? PRE_VIEW_GROUP : n_views;
    uint32_t* vis = call_runs_block_cull(N, n_views) ? ws_at<uint32_t>(ws, B.vis) : nullptr;
    // one pass over the Gaussians for the whole batch (scene data read once, per-view outputs written)
    const PosedDev pd{posed ? posed->object_id : nullptr, posed ? posed->poses : nullptr, posed ? posed->k_objects : 0};
    const int deg = scene->shs ? scene->sh_degree : 0;
    const LayerDev ld{layers ? layers->layer_id : nullptr, n_layers};
#define PGR_PRE(D, Pz, Ly, Sp) preprocess_batch_kernel<D, Pz, Ly, Sp><<<dim3(L.n_blocks, view_groups), PRE_BLOCK, 0, stream>>>(*scene, cams_dev, pre_table, n_views, pd, vis, B.vis_words, ld, views_per_block)
#define PGR_PRE_DEG(Pz, Ly, Sp) switch (deg) { case 0: PGR_PRE(0, Pz, Ly, Sp); break; case 1: PGR_PRE(1, Pz, Ly, Sp); break; \
                                               case 2: PGR_PRE(2, Pz, Ly, Sp); break; default: PGR_PRE(3, Pz, Ly, Sp); break; }
    // (the split SH layout -- PgrScene::shs_rest, the single-view render() of a model as stored -- has its own kernels for the
    //  plain and the layered call; a posed call takes the concatenated layout: check above)
    if (layers) {
        if (posed) { PGR_PRE_DEG(true, true, false) } else if (scene->shs_rest) { PGR_PRE_DEG(false, true, true) } else { PGR_PRE_DEG(false, true, false) }
    } else {
        if (posed) { PGR_PRE_DEG(true, false, false) } else if (scene->shs_rest) { PGR_PRE_DEG(false, false, true) } else { PGR_PRE_DEG(false, false, false) }
    }
#undef PGR_PRE_DEG
#undef PGR_PRE
    mark(1);
    // ---- stage 1: per-chunk LDS tile histograms + slice reservation, then the tile scan (device only)
    const int grid_x = (W + TILE - 1) / TILE;
    const bool few_views = n_views <= SMALL_BATCH_VIEWS;
    const size_t lds = bin_lds_bytes(layer_tiles, few_views ? BIN_THREADS_SMALL : BIN_THREADS);
    const BinLayers bl{layers ? layers->layer_id : nullptr, layer_tiles, layer_rows, n_layers};
    if (few_views)
        bin_kernel<false, BIN_THREADS_SMALL><<<dim3(L.n_chunks, n_views), BIN_THREADS_SMALL, lds, stream>>>(
            bin_table, N, grid_x, L.tiles, W, H, vis, B.vis_words, verdict_groups, bl);
    else
        bin_kernel<false, BIN_THREADS><<<dim3(L.n_chunks, n_views), BIN_THREADS, lds, stream>>>(
            bin_table, N, grid_x, L.tiles, W, H, vis, B.vis_words, verdict_groups, bl);
    // tile scan -> ranges; the same pass counts the compositor's work items per (XCD stream, length class) and its last
    // workgroup turns the counts into the streams' write cursors
    tile_scan_kernel<<<n_views, 1024, 0, stream>>>(bin_table, L.tiles, (uint32_t)max_instances, L.grid_x, order_state,
                                                   layers ? 1 : 0, status_event ? h_status : nullptr);
    // early status: the scan wrote the status words into the pinned host scratch itself; whoever waits for this event reads
    // them two thirds of a single-view call before its compositor ends
    if (status_event && !hip_ok(hipEventRecord(status_event, stream), "record status event")) return fail(PGR_ERR_LAUNCH_FAILURE);
    mark(2);
    // ---- stage 2: scatter (depth bits, index) into the tiles' slices
    if (few_views)
        bin_kernel<true, BIN_THREADS_SMALL><<<dim3(L.n_chunks, n_views), BIN_THREADS_SMALL, lds, stream>>>(
            bin_table, N, grid_x, L.tiles, W, H, vis, B.vis_words, verdict_groups, bl);
    else
        bin_kernel<true, BIN_THREADS><<<dim3(L.n_chunks, n_views), BIN_THREADS, lds, stream>>>(
            bin_table, N, grid_x, L.tiles, W, H, vis, B.vis_words, verdict_groups, bl);
    mark(3);
    // ---- stage 3: work order (XCD streams, longest lists first) + per-tile (depth, index) sort
    const dim3 og((L.tiles + 255) / 256, n_views);
    const int items = n_views * L.tiles;
    const size_t qs = (size_t)items;              // queue stride
    const bool merge_long = n_views <= SMALL_BATCH_VIEWS;
    order_scatter_kernel<<<og, 256, 0, stream>>>(view_table, L.tiles, L.grid_x, order_state, work_order, sort_queue,
                                                 (uint32_t)items, merge_long ? 1 : 0, layers ? 1 : 0);
    // a tier's queue and its length word (SortTier, pgr_common.h); the segment queue lies behind the tiers' queues
    const auto queue_of = [&](SortTier tier) { return sort_queue + (size_t)tier * qs; };
    const auto n_queue_of = [&](SortTier tier) { return order_state + ORDER_BINS + tier; };
    uint4* const seg_queue = sort_queue + (size_t)SORT_TIERS * qs;
    uint32_t* const n_seg = order_state + ORDER_SEG_WORD;
    if (!merge_long) {
        // 8193..15872 keys: the windowed sort (two workgroups per CU); longer: the split pre-pass, whose depth segments the
        // 512 x 16 tier's kernel sorts from the segment queue; what either rejects joins the open-ended kernel's queue
        // (one launch: its first workgroups run the split pre-pass, the windowed sort fills the chip beside them)
        const int part_blocks = std::min(items, 1024);          // every third workgroup: 3 x part_blocks in all, two thirds sort
        tile_sort_window_kernel<<<3 * part_blocks, SORT_WINDOW_THREADS, 0, stream>>>(
            bin_table, L.tiles, queue_of(TIER_WINDOW), n_queue_of(TIER_WINDOW), queue_of(TIER_OPEN), n_queue_of(TIER_OPEN),
            (uint32_t)part_blocks, queue_of(TIER_SPLIT), n_queue_of(TIER_SPLIT), seg_queue, n_seg, (uint32_t)B.seg_cap);
    }
    // the open-ended kernel: every long list of a one- / two-view call; in a batch only what the two kernels above rejected
    // (piled-up depths: rare) -- a handful of workgroups then, 512 of them cost 20 us to find an empty queue
    tile_sort_long_kernel<1024, 16, true><<<merge_long ? std::min(items, 512) : 32, 1024, 0, stream>>>(
        bin_table, L.tiles, queue_of(TIER_OPEN), n_queue_of(TIER_OPEN));
    if (!merge_long) {
        // 4097..8192 keys: 512 threads x 16 keys over 3584 buckets = 80 KiB, TWO workgroups per CU (round 5: the position-owned
        // ranking needs no index image, so the bucket count is free; 1024 x 8 over 8192 buckets = 96 KiB held a CU alone);
        // the same launch sorts the split pre-pass's segments behind its own lists
        tile_sort_long_kernel<512, 16, false, SORT_T2_BUCKETS, 4, true><<<std::min(items, 2048), 512, 0, stream>>>(
            bin_table, L.tiles, queue_of(TIER_8K), n_queue_of(TIER_8K), seg_queue, n_seg, (uint32_t)B.seg_cap);
        tile_sort_long_kernel<512, 8, false><<<std::min(items, 2048), 512, 0, stream>>>(
            bin_table, L.tiles, queue_of(TIER_4K), n_queue_of(TIER_4K));
    }
    tile_sort_kernel<<<items, SORT_THREADS, 0, stream>>>(bin_table, L.tiles, queue_of(TIER_SHORT), n_queue_of(TIER_SHORT));
    mark(4);
    // ---- stage 4: compositing of every (view, tile, quarter) work item in ONE launch; with `semantic` the same
    // walk also produces the objects-only semantic image
    const uint32_t items_per_view = ITEMS_PER_TILE * (uint32_t)L.tiles;
    const uint32_t slots = (uint32_t)B.order_slots;
    SemanticDev sd{nullptr, nullptr, nullptr, 0, 0, nullptr, 0.0f, layer_tiles};
    if (want_sem) {
        const uint8_t* ids_u8 = semantic->object_id_u8;      // (a per-scene constant: pgr_scene_prepare packs it once)
        if (!ids_u8 && semantic->k_objects <= 255 && semantic->n_env < N) {
            auto* dst = ws_at<uint8_t>(ws, B.obj_u8);
            const int n_obj = N - semantic->n_env;
            pack_object_ids_kernel<<<(n_obj + 255) / 256, 256, 0, stream>>>(semantic->object_id, semantic->n_env, N, dst);
            ids_u8 = dst;
        }
        sd = SemanticDev{semantic->object_id, ids_u8, semantic->colors, semantic->n_env, semantic->k_objects,
                         semantic->mask_colors, semantic->mask_threshold, layer_tiles};
    }
    if (layers) {
        sd.mask_colors = layers->mask_colors; sd.mask_thr = layers->mask_threshold; sd.k = n_layers;
        // empty (layer, tile) lists have no work item: their pixels hold the background's verdict
        layer_mask_fill_kernel<<<dim3(LAYER_FILL_BLOCKS, n_layers, n_views), 256, 0, stream>>>(
            view_table, layers->mask_colors, layers->mask_threshold, P, layers->layer_id, N);
        launch_composite<false, false, true>(slots, stream, view_table, items_per_view, work_order, sd);
    } else if (want_aux && want_sem)
        launch_composite<true, true>(slots, stream, view_table, items_per_view, work_order, sd);
    else if (want_aux)
        launch_composite<true, false>(slots, stream, view_table, items_per_view, work_order, sd);
    else if (want_sem)
        launch_composite<false, true>(slots, stream, view_table, items_per_view, work_order, sd);
    else
        launch_composite<false, false>(slots, stream, view_table, items_per_view, work_order, sd);
    mark(5);
    if (int32_t rc = launch_status("kernel launch")) return fail(rc);

    if (status_event) return PGR_OK;       // the status words reached the host behind the scan
    // the only host read of the batch: instance counts + overflow flags, after everything is enqueued
    if (!hip_ok(hipMemcpyAsync(h_status, status_dev, (size_t)n_views * 8, hipMemcpyDeviceToHost, stream), "memcpy status"))
        return fail(PGR_ERR_LAUNCH_FAILURE);
    if (host_scratch) return PGR_OK;       // asynchronous: the caller synchronises and calls pgr_batch_status
    if (!hip_ok(hipStreamSynchronize(stream), "sync at batch end")) return PGR_ERR_LAUNCH_FAILURE;
    bool overflow = false;
    for (int v = 0; v < n_views; ++v) {
        if (num_instances) num_instances[v] = (int64_t)h_status[2 * v];
        overflow = overflow || h_status[2 * v + 1];
    }
    return overflow ? PGR_ERR_INSTANCE_OVERFLOW : PGR_OK;
}

// The batched backward's scratch: the gradient rows [n_views, n, GRAD_ROW], then the BwdViewDev table.
struct BackwardScratch { size_t rows_bytes, table, total; };

static BackwardScratch backward_scratch(int32_t n, int32_t n_views) {
    const size_t rows_bytes = (size_t)n_views * (size_t)n * GRAD_ROW * sizeof(float), table = align_up(rows_bytes);
    return {rows_bytes, table, table + align_up((size_t)n_views * sizeof(BwdViewDev))};
}

// What the backward's checks leave behind for its launches (all zero for an empty scene, which launches nothing).
struct BackwardPlan { char* ws; Layout L; BatchLayout B; float* rows; BwdViewDev* table; };

// The backward after its checks: the per-view table into `table` from the launch arguments (no host staging that
// would have to outlive the call), `rows` [n_views, n, GRAD_ROW] cleared, the walk of every (view, tile, quarter) item of the
// forward's work order, then one thread per Gaussian over the views.  One view runs the kernels' ONE instances.
static int32_t backward_impl(const PgrScene* scene, int n_views, const PgrBackwardView* views,
                             const float* const* grad_alpha, char* ws, const Layout& L, const BatchLayout& B,
                             const PgrGradOutputs* grads, float* rows, BwdViewDev* table, hipStream_t stream) {
    const int N = scene->n;
    const CameraDev* cams_dev = ws_at<const CameraDev>(ws, B.cams);
    for (int v0 = 0; v0 < n_views; v0 += BWD_TABLE_CHUNK) {
        const int cnt = std::min(BWD_TABLE_CHUNK, n_views - v0);
        BwdTableChunk chunk;
        memset(&chunk, 0, sizeof(chunk));
        for (int k = 0; k < cnt; ++k) {
            const int v = v0 + k;
            const ViewWs vw = view_slice(ws, L, B, n_views, v);
            const PgrBackwardView& bv = views[v];
            chunk.v[k] = BwdViewDev{vw.ranges, vw.gauss_sorted, vw.splats, vw.counters, bv.grad_color, bv.grad_depth,
                                    bv.final_T, bv.n_contrib, bv.radii, rows + (size_t)v * N * GRAD_ROW,
                                    grad_alpha ? grad_alpha[v] : nullptr};
        }
        backward_table_kernel<<<1, 64, 0, stream>>>(chunk, cnt, table + v0);
    }
    if (!hip_ok(hipMemsetAsync(rows, 0, backward_scratch(N, n_views).rows_bytes, stream), "memset grad rows"))
        return PGR_ERR_LAUNCH_FAILURE;
    bool any_alpha = false;
    for (int v = 0; grad_alpha && v < n_views; ++v) any_alpha = any_alpha || grad_alpha[v];
    // (the instance without the alpha term when there is no dL/dalpha: backward.hip.h, composite_backward_block)
    const bool one = n_views == 1;
    auto* walk = any_alpha ? (one ? composite_backward_batch_kernel<true, true> : composite_backward_batch_kernel<true, false>)
                           : (one ? composite_backward_batch_kernel<false, true> : composite_backward_batch_kernel<false, false>);
    walk<<<4u * (uint32_t)B.order_slots, WAVE, 0, stream>>>(table, cams_dev, (uint32_t)n_views, ITEMS_PER_TILE * (uint32_t)L.tiles,
                                                          ws_at<const uint32_t>(ws, B.work_order));
    const GradOut go{grads->means2d, grads->means3d, grads->opacities, grads->colors, grads->shs, grads->cov3d,
                     grads->scales, grads->rotations};
    constexpr decltype(&preprocess_backward_batch_kernel<0, false>) pres[4][2] = {
        {preprocess_backward_batch_kernel<0, false>, preprocess_backward_batch_kernel<0, true>},
        {preprocess_backward_batch_kernel<1, false>, preprocess_backward_batch_kernel<1, true>},
        {preprocess_backward_batch_kernel<2, false>, preprocess_backward_batch_kernel<2, true>},
        {preprocess_backward_batch_kernel<3, false>, preprocess_backward_batch_kernel<3, true>}};
    auto* pre = pres[scene->shs ? scene->sh_degree : 0][one];
    pre<<<(N + 255) / 256, 256, 0, stream>>>(*scene, table, cams_dev, n_views, go);
    return launch_status("backward launch");
}

// The camera kernels behind a finished backward_impl: `table` and the packed cameras as it left them, the outputs of up to
// BWD_TABLE_CHUNK views per finishing launch (kernel arguments).  An empty scene writes zeros.
static size_t camera_scratch_bytes(int32_t n, int32_t n_views) {
    return align_up((size_t)n_views * (size_t)((n + CAM_BLOCK - 1) / CAM_BLOCK) * CAM_GRAD * sizeof(float) + 1);
}

static int32_t camera_backward_impl(const PgrScene* scene, int n_views, const PgrCameraGrad* cg, const BwdViewDev* table,
                                    const CameraDev* cams_dev, float* partials, hipStream_t stream) {
    const int N = scene->n;
    if (N == 0) {
        for (int v = 0; v < n_views; ++v) {
            const std::pair<float*, size_t> outs[3] = {{cg[v].viewmatrix, 16}, {cg[v].projmatrix, 16}, {cg[v].campos, 3}};
            for (const auto& o : outs)
                if (o.first && !hip_ok(hipMemsetAsync(o.first, 0, o.second * sizeof(float), stream), "memset camera grad"))
                    return PGR_ERR_LAUNCH_FAILURE;
        }
        return PGR_OK;
    }
    const int blocks = (N + CAM_BLOCK - 1) / CAM_BLOCK;
    const bool one = n_views == 1;
    constexpr decltype(&camera_backward_kernel<0, false>) cks[4][2] = {
        {camera_backward_kernel<0, false>, camera_backward_kernel<0, true>},
        {camera_backward_kernel<1, false>, camera_backward_kernel<1, true>},
        {camera_backward_kernel<2, false>, camera_backward_kernel<2, true>},
        {camera_backward_kernel<3, false>, camera_backward_kernel<3, true>}};
    cks[scene->shs ? scene->sh_degree : 0][one]<<<blocks, CAM_BLOCK, 0, stream>>>(*scene, table, cams_dev, n_views, partials);
    for (int v0 = 0; v0 < n_views; v0 += BWD_TABLE_CHUNK) {
        const int cnt = std::min(BWD_TABLE_CHUNK, n_views - v0);
        CamGradChunk chunk;
        memset(&chunk, 0, sizeof(chunk));
        for (int k = 0; k < cnt; ++k) {
            chunk.view[k] = cg[v0 + k].viewmatrix;
            chunk.proj[k] = cg[v0 + k].projmatrix;
            chunk.campos[k] = cg[v0 + k].campos;
        }
        camera_grad_finish_kernel<<<cnt, CAM_BLOCK, 0, stream>>>(partials, blocks, v0, chunk);
    }
    return launch_status("camera backward launch");
}

// pgr_pose_objects' workspace, per launch of POSE_JOBS_PER_LAUNCH jobs: the centroid partials, then the jobs' poses.
constexpr size_t POSE_PART_BYTES = align_up((size_t)POSE_JOBS_PER_LAUNCH * POSE_REDUCE_BLOCKS * 3 * sizeof(double));
constexpr size_t POSE_LAUNCH_BYTES = POSE_PART_BYTES + align_up((size_t)POSE_JOBS_PER_LAUNCH * sizeof(ObjectPoseDev));

}  // namespace pgr

using namespace pgr;

extern "C" {

int32_t pgr_abi_version(void) { return PGR_ABI_VERSION; }
#ifndef PGR_SOURCE_HASH
#define PGR_SOURCE_HASH "unstamped"      // pegasus_amd/build.py passes the hash of the sources it compiled
#endif
const char* pgr_version(void) { return "pegasus_raster 0.9 (gfx950) src " PGR_SOURCE_HASH; }

const char* pgr_status_string(int32_t status) {
    switch (status) {
        case PGR_OK: return "ok";
        case PGR_ERR_INVALID_ARGUMENT: return "invalid argument";
        case PGR_ERR_WORKSPACE_TOO_SMALL: return "workspace too small";
        case PGR_ERR_INSTANCE_OVERFLOW: return "instance buffer overflow";
        case PGR_ERR_LAUNCH_FAILURE: return "HIP launch failure";
        case PGR_ERR_NO_DEVICE: return "no HIP device";
        default: return "unknown status";
    }
}

const char* pgr_last_hip_error(void) { return g_hip_error; }

size_t pgr_batch_workspace_bytes(int32_t n, int32_t width, int32_t height, int64_t max_instances, int32_t n_views) {
    if (n < 0 || width <= 0 || height <= 0 || max_instances < 0 || max_instances > 0x7fffffffLL || n_views <= 0)
        return 0;
    return make_batch_layout(make_layout(n, width, height, max_instances), n_views, (size_t)n).total;
}

size_t pgr_workspace_bytes(int32_t n, int32_t width, int32_t height, int64_t max_instances) {
    return pgr_batch_workspace_bytes(n, width, height, max_instances, 1);
}

int32_t pgr_workspace_view(void* workspace, size_t workspace_bytes, int32_t n, int32_t width, int32_t height,
                           int64_t max_instances, int32_t n_views, int32_t view_index, PgrWorkspaceView* v) {
    if (!workspace || !v || n < 0 || width <= 0 || height <= 0 || max_instances < 0 || n_views <= 0 ||
        view_index < 0 || view_index >= n_views)
        return PGR_ERR_INVALID_ARGUMENT;
    const Layout L = make_layout(n, width, height, max_instances);
    const BatchLayout B = make_batch_layout(L, n_views, (size_t)n);
    if (workspace_bytes < B.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    const ViewWs w = view_slice(static_cast<char*>(workspace), L, B, n_views, view_index);
    v->splats = reinterpret_cast<const float*>(w.splats);
    v->rects = reinterpret_cast<const uint16_t*>(w.rects);
    v->gauss_sorted = w.gauss_sorted;
    v->ranges = reinterpret_cast<const uint32_t*>(w.ranges);
    v->num_instances = w.counters;
    return PGR_OK;
}

// Host only, launches nothing: where a batch call of this shape leaves its visibility words (NULL = it runs no block test).
int32_t pgr_workspace_block_visibility(void* workspace, size_t workspace_bytes, int32_t n, int32_t width, int32_t height,
                                       int64_t max_instances, int32_t n_views, const uint32_t** vis_words,
                                       int32_t* words_per_block) {
    if (!workspace || !vis_words || !words_per_block || n < 0 || width <= 0 || height <= 0 || max_instances < 0 ||
        n_views <= 0)
        return PGR_ERR_INVALID_ARGUMENT;
    const Layout L = make_layout(n, width, height, max_instances);
    const BatchLayout B = make_batch_layout(L, n_views, (size_t)n);
    if (workspace_bytes < B.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    *words_per_block = B.vis_words;
    *vis_words = n > 0 && call_runs_block_cull(n, n_views)
                     ? ws_at<const uint32_t>(workspace, B.vis) : nullptr;
    return PGR_OK;
}

size_t pgr_host_scratch_bytes(int32_t n_views) { return n_views > 0 ? host_tables(n_views).total : 0; }

// The synchronous call with stage_ms: PGR_NUM_STAGES + 1 events around forward_batch_impl, their elapsed times read afterwards.
static int32_t forward_profiled(const PgrForwardCall* c, ForwardOptions opt, hipStream_t stream) {
    hipEvent_t ev[PGR_NUM_STAGES + 1];
    for (auto& e : ev)
        if (!hip_ok(hipEventCreate(&e), "hipEventCreate")) return PGR_ERR_LAUNCH_FAILURE;
    for (int k = 0; k < PGR_NUM_STAGES; ++k) c->stage_ms[k] = 0.f;
    opt.ev = ev;
    int32_t rc = forward_batch_impl(c->scene, c->n_views, c->cameras, c->outs, c->workspace, c->workspace_bytes,
                                    c->max_instances_per_view, c->num_instances, stream, opt);
    if (rc == PGR_OK && c->scene->n > 0) {
        for (int k = 0; rc == PGR_OK && k < PGR_NUM_STAGES; ++k)
            if (!hip_ok(hipEventElapsedTime(&c->stage_ms[k], ev[k], ev[k + 1]), "hipEventElapsedTime"))
                rc = PGR_ERR_LAUNCH_FAILURE;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    return rc;
}

// forward_batch_impl behind the checks of what goes with a synchronous and with an asynchronous call.  An empty scene
// launches nothing: the asynchronous call's status words (all zero) are written here.
int32_t pgr_forward(const PgrForwardCall* c, void* stream_v) {
    if (!c) return PGR_ERR_INVALID_ARGUMENT;
    if (c->host_scratch ? (c->num_instances || c->stage_ms) : (c->posed || c->layers || c->status_event))
        return PGR_ERR_INVALID_ARGUMENT;
    if (c->status_event && c->layers) return PGR_ERR_INVALID_ARGUMENT;
    if (c->host_scratch) {
        if (c->n_views <= 0 || c->host_scratch_bytes < host_tables(c->n_views).total) return PGR_ERR_INVALID_ARGUMENT;
        if (c->scene && c->scene->n == 0) memset(c->host_scratch, 0, host_tables(c->n_views).total);
    }
    ForwardOptions opt;
    opt.host_scratch = c->host_scratch;
    opt.semantic = c->semantic;
    opt.posed = c->posed;
    opt.layers = c->layers;
    opt.status_event = static_cast<hipEvent_t>(c->status_event);
    hipStream_t stream = as_stream(stream_v);
    if (c->stage_ms) return forward_profiled(c, opt, stream);
    return forward_batch_impl(c->scene, c->n_views, c->cameras, c->outs, c->workspace, c->workspace_bytes,
                              c->max_instances_per_view, c->num_instances, stream, opt);
}

size_t pgr_layers_workspace_bytes(int32_t n, int32_t width, int32_t height, int64_t max_instances, int32_t n_views,
                                  int32_t n_layers) {
    if (n < 0 || width <= 0 || height <= 0 || max_instances < 0 || max_instances > 0x7fffffffLL || n_views <= 0 ||
        n_layers <= 0 || n_layers > 4096)
        return 0;
    return make_batch_layout(make_layout(n, width, height, max_instances, n_layers), n_views, (size_t)n).total;
}

size_t pgr_scene_cache_bytes(int32_t n) { return n < 0 ? 0 : align_up((size_t)n * 4) + align_up((size_t)n); }

int32_t pgr_scene_prepare(const PgrScene* scene, const PgrSemantic* semantic, void* cache, size_t cache_bytes,
                          const uint32_t** tie_inv, const uint8_t** object_id_u8, void* stream_v) {
    if (!scene || scene->n < 0 || !tie_inv || !object_id_u8) return PGR_ERR_INVALID_ARGUMENT;
    *tie_inv = nullptr;
    *object_id_u8 = nullptr;
    const int N = scene->n;
    if (N == 0) return PGR_OK;
    if (!cache) return PGR_ERR_INVALID_ARGUMENT;
    if (cache_bytes < pgr_scene_cache_bytes(N)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = as_stream(stream_v);
    char* c = static_cast<char*>(cache);
    if (scene->tie_index) {
        auto* inv = reinterpret_cast<uint32_t*>(c);
        invert_tie_index_kernel<<<(N + 255) / 256, 256, 0, stream>>>(N, scene->tie_index, inv);
        *tie_inv = inv;
    }
    if (semantic && semantic->object_id && semantic->k_objects > 0 && semantic->k_objects <= 255 && semantic->n_env >= 0 &&
        semantic->n_env < N) {
        auto* ids = ws_at<uint8_t>(c, align_up((size_t)N * 4));
        const int n_obj = N - semantic->n_env;
        pack_object_ids_kernel<<<(n_obj + 255) / 256, 256, 0, stream>>>(semantic->object_id, semantic->n_env, N, ids);
        *object_id_u8 = ids;
    }
    return launch_status("scene_prepare launch");
}

int32_t pgr_batch_status(const void* host_scratch, int32_t n_views, int64_t* num_instances) {
    if (!host_scratch || n_views <= 0) return PGR_ERR_INVALID_ARGUMENT;
    const uint32_t* st = ws_at<uint32_t>(host_scratch, host_tables(n_views).status);
    bool overflow = false;
    for (int v = 0; v < n_views; ++v) {
        if (num_instances) num_instances[v] = (int64_t)st[2 * v];
        overflow = overflow || st[2 * v + 1];
    }
    return overflow ? PGR_ERR_INSTANCE_OVERFLOW : PGR_OK;
}

size_t pgr_backward_batch_scratch_bytes(int32_t n, int32_t n_views) {
    return (n < 0 || n_views <= 0) ? 0 : backward_scratch(n, n_views).total;
}

size_t pgr_camera_grad_scratch_bytes(int32_t n, int32_t n_views) {
    return (n < 0 || n_views <= 0) ? 0 : camera_scratch_bytes(n, n_views);
}

// The backward's checks and layouts: every check before the first enqueue.
static int32_t backward_plan(const PgrBackwardCall& c, BackwardPlan* p) {
    const PgrScene* scene = c.scene;
    if (c.camera_grads && (!scene || scene->n < 0 || c.n_views <= 0 || !c.camera_scratch ||
                           c.camera_scratch_bytes < camera_scratch_bytes(scene->n, c.n_views)))
        return PGR_ERR_INVALID_ARGUMENT;
    if (int rc = check_scene(scene)) return rc;
    if (scene->shs_rest) return PGR_ERR_INVALID_ARGUMENT;      // the SH gradient is one [n,sh_stride,3] array
    if (c.n_views <= 0 || !c.cameras || !c.views || !c.grads) return PGR_ERR_INVALID_ARGUMENT;
    if (c.max_instances_per_view < 0 || c.max_instances_per_view > 0x7fffffffLL) return PGR_ERR_INVALID_ARGUMENT;
    const int N = scene->n, W = c.cameras[0].image_width, H = c.cameras[0].image_height;
    if (W <= 0 || H <= 0) return PGR_ERR_INVALID_ARGUMENT;
    for (int v = 0; v < c.n_views; ++v) {
        if (c.cameras[v].image_width != W || c.cameras[v].image_height != H) return PGR_ERR_INVALID_ARGUMENT;
        if (!c.views[v].grad_color || !c.views[v].final_T || !c.views[v].n_contrib) return PGR_ERR_INVALID_ARGUMENT;
        if (N > 0 && !c.views[v].radii) return PGR_ERR_INVALID_ARGUMENT;
    }
    if (N == 0) return PGR_OK;
    const BackwardScratch S = backward_scratch(N, c.n_views);
    if (!c.workspace || !c.scratch || c.scratch_bytes < S.total) return PGR_ERR_INVALID_ARGUMENT;
    p->L = make_layout(N, W, H, c.max_instances_per_view);
    p->B = make_batch_layout(p->L, c.n_views, (size_t)N);
    if (c.workspace_bytes < p->B.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    p->ws = static_cast<char*>(c.workspace);
    p->rows = static_cast<float*>(c.scratch);
    p->table = ws_at<BwdViewDev>(c.scratch, S.table);
    return PGR_OK;
}

// The plan, the scene backward, then (with camera_grads) the camera kernels.
int32_t pgr_backward(const PgrBackwardCall* c, void* stream_v) {
    if (!c) return PGR_ERR_INVALID_ARGUMENT;
    BackwardPlan p{};
    if (int rc = backward_plan(*c, &p)) return rc;
    hipStream_t stream = as_stream(stream_v);
    if (c->scene->n > 0)
        if (int32_t rc = backward_impl(c->scene, c->n_views, c->views, c->grad_alpha, p.ws, p.L, p.B, c->grads, p.rows, p.table,
                                       stream))
            return rc;
    if (!c->camera_grads) return PGR_OK;
    return camera_backward_impl(c->scene, c->n_views, c->camera_grads, p.table,
                                ws_at<const CameraDev>(p.ws, p.B.cams), static_cast<float*>(c->camera_scratch), stream);
}

int32_t pgr_compose_object(int32_t n, const float* xyz, const float* rot, const float* f_rest, int32_t n_rest,
                           int32_t in_rest_stride, const PgrObjectPose* pose, float* out_xyz, float* out_rot,
                           float* out_rest, int32_t out_rest_stride, void* stream_v) {
    static_assert(sizeof(PgrObjectPose) == sizeof(ObjectPoseDev), "pose layout");
    if (n < 0 || !pose || (n > 0 && (!xyz || !out_xyz)) || (n_rest != 0 && n_rest != 3 && n_rest != 8 && n_rest != 15) ||
        (f_rest && n_rest > 0 && (in_rest_stride < 3 * n_rest || out_rest_stride < 3 * n_rest)))
        return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    ObjectPoseDev P;
    memcpy(&P, pose, sizeof(P));
    compose_object_kernel<<<(n + 255) / 256, 256, 0, as_stream(stream_v)>>>(
        n, xyz, rot, f_rest, n_rest, in_rest_stride, P, out_xyz, out_rot, out_rest, out_rest_stride);
    return launch_status("compose_object launch");
}

// one wave that watches both of its clocks for spin_us microseconds: s_memtime ticks once per SHADER cycle, s_memrealtime
// at a constant 100 MHz (MI355X_MICROARCH.md "Per-instruction cycle constants"), so ticks[0] / ticks[1] x 100 MHz is the
// clock the chip ran at while whatever else was resident ran beside it; ticks[2], ticks[3] = the 100 MHz counter at the
// start and at the end (two probes on two streams can be checked for having overlapped)
__global__ void clock_probe_kernel(unsigned long long* __restrict__ ticks, uint32_t spin_us) {
    const unsigned long long r0 = wall_clock64();
    const unsigned long long c0 = __builtin_readcyclecounter();
    unsigned long long r1 = r0;
    while (r1 - r0 < (unsigned long long)spin_us * 100ull) {
        __builtin_amdgcn_s_sleep(8);
        r1 = wall_clock64();
    }
    const unsigned long long c1 = __builtin_readcyclecounter();
    if (threadIdx.x == 0) { ticks[0] = c1 - c0; ticks[1] = r1 - r0; ticks[2] = r0; ticks[3] = r1; }
}

int32_t pgr_clock_probe(uint64_t* ticks, uint32_t spin_us, void* stream_v) {
    if (!ticks || spin_us > 1000000u) return PGR_ERR_INVALID_ARGUMENT;
    clock_probe_kernel<<<1, WAVE, 0, as_stream(stream_v)>>>(reinterpret_cast<unsigned long long*>(ticks), spin_us);
    return launch_status("clock_probe launch");
}

size_t pgr_pose_objects_workspace_bytes(int32_t n_jobs) {
    if (n_jobs <= 0) return 0;
    return ((size_t)n_jobs + POSE_JOBS_PER_LAUNCH - 1) / POSE_JOBS_PER_LAUNCH * POSE_LAUNCH_BYTES;
}

int32_t pgr_pose_objects(int32_t n_jobs, const PgrPoseJob* jobs, const double* sh_dirs, const double* sh_pinv,
                         void* workspace, size_t workspace_bytes, void* stream_v) {
    hipStream_t stream = as_stream(stream_v);
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return PGR_OK;
    for (int k = 0; k < n_jobs; ++k) {
        const PgrPoseJob& j = jobs[k];
        if (j.n < 0 || (j.n > 0 && (!j.src || !j.dst)) || j.kind < PGR_POSE_XYZ || j.kind > PGR_POSE_SH ||
            (j.kind == PGR_POSE_SH && ((j.n_rest != 3 && j.n_rest != 8 && j.n_rest != 15) || !sh_dirs || !sh_pinv)))
            return PGR_ERR_INVALID_ARGUMENT;
    }
    if (!workspace || workspace_bytes < pgr_pose_objects_workspace_bytes(n_jobs)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    for (int k0 = 0, launch = 0; k0 < n_jobs; k0 += POSE_JOBS_PER_LAUNCH, ++launch) {
        PoseJobTable T{};
        T.count = std::min(POSE_JOBS_PER_LAUNCH, n_jobs - k0);
        uint32_t blocks = 0;
        bool reduce = false;
        for (int k = 0; k < T.count; ++k) {
            const PgrPoseJob& j = jobs[k0 + k];
            T.job[k] = PoseJobDev{j.src, j.dst, j.R, j.t, j.n, j.kind, j.n_rest, j.about_origin,
                                  j.R_row_stride > 0 ? j.R_row_stride : 3, j.t_stride > 0 ? j.t_stride : 1, blocks};
            blocks += (uint32_t)((j.n + 255) / 256);
            reduce = reduce || (j.kind == PGR_POSE_XYZ && !j.about_origin && j.R && j.n > 0);
        }
        auto* partial = ws_at<double>(workspace, (size_t)launch * POSE_LAUNCH_BYTES);
        auto* poses = ws_at<ObjectPoseDev>(workspace, (size_t)launch * POSE_LAUNCH_BYTES + POSE_PART_BYTES);
        if (reduce) pose_reduce_kernel<<<dim3(POSE_REDUCE_BLOCKS, T.count), 256, 0, stream>>>(T, partial);
        pose_prepare_kernel<<<T.count, 128, 0, stream>>>(T, partial, sh_dirs, sh_pinv, poses);
        if (blocks) pose_apply_kernel<<<blocks, 256, 0, stream>>>(T, poses);
    }
    return launch_status("pose_objects launch");
}

size_t pgr_block_visibility_workspace_bytes(int32_t n, int32_t n_views) {
    if (n < 0 || n_views <= 0) return 0;
    return align_up((size_t)n_views * sizeof(CameraDev)) + align_up((size_t)((n + WAVE - 1) / WAVE) * sizeof(BlockBounds) + 1);
}

int32_t pgr_block_visibility(const PgrScene* scene, int32_t n_views, const PgrCamera* cams, void* workspace,
                             size_t workspace_bytes, uint32_t* vis_words, void* stream_v) {
    hipStream_t stream = as_stream(stream_v);
    if (int rc = check_scene(scene)) return rc;
    if (n_views <= 0 || !cams) return PGR_ERR_INVALID_ARGUMENT;
    if (scene->n == 0) return PGR_OK;
    if (!workspace || !vis_words) return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < pgr_block_visibility_workspace_bytes(scene->n, n_views)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    const int W = cams[0].image_width, H = cams[0].image_height;
    for (int v = 0; v < n_views; ++v)
        if (cams[v].image_width != W || cams[v].image_height != H || !camera_ok(cams[v])) return PGR_ERR_INVALID_ARGUMENT;
    char* ws = static_cast<char*>(workspace);
    auto* cams_dev = reinterpret_cast<CameraDev*>(ws);
    auto* bounds = ws_at<BlockBounds>(ws, align_up((size_t)n_views * sizeof(CameraDev)));
    for (int v0 = 0; v0 < n_views; v0 += CAM_PACK_MAX) {
        const int cnt = std::min(CAM_PACK_MAX, n_views - v0);
        pack_camera_kernel<<<cnt, 64, 0, stream>>>(pack_cameras(cams + v0, cnt, false), W, H, cams_dev + v0);
    }
    const int groups = (scene->n + WAVE - 1) / WAVE, words = (n_views + 31) / 32;
    block_bounds_kernel<<<(groups + 3) / 4, 256, 0, stream>>>(*scene, nullptr, bounds, groups);
    block_cull_kernel<<<dim3((groups + 7) / 8, words), 256, 0, stream>>>(bounds, groups, cams_dev, n_views, words, vis_words);
    return launch_status("block_visibility launch");
}

int32_t pgr_mark_visible(int32_t n, const float* means3d, const float* viewmatrix, uint8_t* present, void* stream_v) {
    if (n < 0 || (n > 0 && (!means3d || !viewmatrix || !present))) return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    mark_visible_kernel<<<(n + 255) / 256, 256, 0, as_stream(stream_v)>>>(n, means3d, viewmatrix, present);
    return launch_status("mark_visible launch");
}

int32_t pgr_color_masks(const float* img_chw, int32_t n_images, int32_t width, int32_t height, const float* colors_k3,
                        int32_t k, float threshold, uint8_t* masks_khw, void* stream_v) {
    if (!img_chw || n_images < 0 || n_images > 65535 || width <= 0 || height <= 0 || k < 0 ||
        (k > 0 && (!colors_k3 || !masks_khw)))
        return PGR_ERR_INVALID_ARGUMENT;
    if (k == 0 || n_images == 0) return PGR_OK;
    const size_t P = (size_t)width * height;
    color_masks_kernel<<<dim3((unsigned)((P + 255) / 256), n_images), 256, 0, as_stream(stream_v)>>>(
        img_chw, P, colors_k3, k, threshold, masks_khw);
    return launch_status("color_masks launch");
}

int32_t pgr_quantize_frame(const float* img_chw, const float* depth_hw, int32_t width, int32_t height,
                           uint8_t* rgb_hwc, uint16_t* depth_mm_hw, void* stream_v) {
    if (width <= 0 || height <= 0 || ((img_chw == nullptr) != (rgb_hwc == nullptr)) ||
        ((depth_hw == nullptr) != (depth_mm_hw == nullptr)))
        return PGR_ERR_INVALID_ARGUMENT;
    const size_t P = (size_t)width * height;
    quantize_kernel<<<(unsigned)((P + 255) / 256), 256, 0, as_stream(stream_v)>>>(img_chw, depth_hw, P, rgb_hwc, depth_mm_hw);
    return launch_status("quantize launch");
}

int32_t pgr_pack_frames(const float* color_b3hw, const float* depth_bhw, const uint8_t* masks_bkhw, int32_t n_images,
                        int32_t k, int32_t width, int32_t height, uint8_t* rgb_bhwc, uint16_t* depth_mm_bhw,
                        uint8_t* mask_bits_bhwj, void* stream_v) {
    if (n_images < 0 || n_images > 65535 || width <= 0 || height <= 0 || k < 0 ||
        ((color_b3hw == nullptr) != (rgb_bhwc == nullptr)) || ((depth_bhw == nullptr) != (depth_mm_bhw == nullptr)) ||
        ((masks_bkhw == nullptr) != (mask_bits_bhwj == nullptr)) || (masks_bkhw && k == 0))
        return PGR_ERR_INVALID_ARGUMENT;
    if (n_images == 0) return PGR_OK;
    const size_t P = (size_t)width * height;
    pack_frames_kernel<<<dim3((unsigned)((P + 255) / 256), n_images), 256, 0, as_stream(stream_v)>>>(
        color_b3hw, depth_bhw, masks_bkhw, P, k, rgb_bhwc, depth_mm_bhw, mask_bits_bhwj);
    return launch_status("pack_frames launch");
}

int32_t pgr_frame_record_layout(int32_t width, int32_t height, int32_t k, PgrRecordLayout* layout) {
    if (!layout || width <= 0 || height <= 0 || k < 0) return PGR_ERR_INVALID_ARGUMENT;
    *layout = record_layout((size_t)width * height, k);
    return PGR_OK;
}

int32_t pgr_pack_records(const float* color_b3hw, const float* depth_bhw, const uint8_t* masks_bkhw, int32_t n_images,
                         int32_t k, int32_t width, int32_t height, uint8_t* records, int64_t record_stride,
                         void* stream_v) {
    PgrRecordLayout L;
    if (pgr_frame_record_layout(width, height, k, &L) != PGR_OK || n_images < 0 || n_images > 65535 || !records ||
        record_stride < L.bytes || (record_stride & 15) || (masks_bkhw && k == 0))
        return PGR_ERR_INVALID_ARGUMENT;
    if (n_images == 0) return PGR_OK;
    const size_t P = (size_t)width * height;
    pack_records_kernel<<<dim3((unsigned)((P + 255) / 256), n_images), 256, 0, as_stream(stream_v)>>>(
        color_b3hw, depth_bhw, masks_bkhw, P, k, records, (size_t)record_stride, (size_t)L.off_depth, (size_t)L.off_masks);
    return launch_status("pack_records launch");
}

}  // extern "C"
