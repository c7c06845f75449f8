// pegasus_raster.hip -- C ABI of libpegasus_raster.so (see include/pegasus_raster.h).
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
#include "cocoeval.hip.h"
#include "cocorle.hip.h"
#include "knn.hip.h"
#include "mesh.hip.h"
#include "meshattr.hip.h"
#include "meshraster.hip.h"
#include "meshsdf.hip.h"
#include "obb.hip.h"
#include "compose.hip.h"
#include "composite.hip.h"
#include "decimate.hip.h"
#include "pgr_common.h"
#include "plane.hip.h"
#include "poseerr.hip.h"
#include "preprocess.hip.h"
#include "radius.hip.h"
#include "registration.hip.h"
#include "tilebin.hip.h"
#include "tilesort.hip.h"
#include "train.hip.h"

namespace pgr {

static thread_local char g_hip_error[256] = "";

static bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    snprintf(g_hip_error, sizeof(g_hip_error), "%s: %s", what, hipGetErrorString(e));
    return false;
}

static constexpr size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Hands out consecutive slices of a buffer, each aligned to 256 B; a slice of zero bytes still takes one unit.  So no layout
// is empty, and the layout functions that check their sizing arguments themselves return one whose total is 0 for "refused".
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += align_up(bytes ? bytes : 1); return o; }
};

// What the evaluation entries (masks, COCO scores) ask of a workspace pointer: their kernels read and write it in 16-byte and
// 8-byte elements at the carved offsets.  And the most workgroups one launch of theirs may have: grid.x is 31 bits.
static bool workspace_aligned_16(const void* workspace) { return reinterpret_cast<uintptr_t>(workspace) % 16 == 0; }
constexpr int64_t MAX_GRID_BLOCKS = 0x7fffffff;

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
    auto* const tile_counts = reinterpret_cast<uint32_t*>(ws + B.tile_counts);
    ViewWs w;
    w.cam = reinterpret_cast<CameraDev*>(ws + B.cams) + v;
    w.counters = reinterpret_cast<uint32_t*>(ws + B.status) + 2 * v;
    w.splats = reinterpret_cast<float4*>(slice + L.splats);
    w.rects = reinterpret_cast<uint2*>(slice + L.rects);
    w.crects = reinterpret_cast<uint2*>(slice + L.crects);
    w.tile_count = tile_counts + (size_t)v * L.tiles;
    w.rel = reinterpret_cast<uint32_t*>(slice + L.rel);
    w.ranges = reinterpret_cast<uint2*>(slice + L.ranges);
    w.bucket = reinterpret_cast<uint2*>(slice + L.bucket);
    w.alt = reinterpret_cast<uint64_t*>(slice + L.alt);
    w.gauss_sorted = reinterpret_cast<uint32_t*>(slice + L.gauss_sorted);
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
    auto* view_table = reinterpret_cast<ViewEntry*>(ws + B.tables + B.host.view_table);
    auto* bin_table = reinterpret_cast<BinView*>(ws + B.tables + B.host.bin_table);
    auto* pre_table = reinterpret_cast<PreOut*>(ws + B.tables + B.host.pre_table);
    auto* cams_dev = reinterpret_cast<CameraDev*>(ws + B.cams);
    auto* status_dev = reinterpret_cast<uint32_t*>(ws + B.status);
    auto* order_state = reinterpret_cast<uint32_t*>(ws + B.order_state);
    auto* sort_queue = reinterpret_cast<uint4*>(ws + B.long_list);
    auto* work_order = reinterpret_cast<uint32_t*>(ws + B.work_order);
    std::vector<ViewWs> vw((size_t)n_views);
    std::vector<char> pageable;
    char* hs = static_cast<char*>(host_scratch);
    if (!hs) {
        pageable.resize(B.host.total);
        hs = pageable.data();
    }
    auto* table = reinterpret_cast<ViewEntry*>(hs + B.host.view_table);
    auto* bins = reinterpret_cast<BinView*>(hs + B.host.bin_table);
    auto* pres = reinterpret_cast<PreOut*>(hs + B.host.pre_table);
    auto* h_status = reinterpret_cast<uint32_t*>(hs + B.host.status);
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
                          scene->tie_index ? (scene->tie_inv ? scene->tie_inv : reinterpret_cast<const uint32_t*>(ws + B.tie_inv)) : nullptr,
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
        batch_header_kernel<<<256, 256, 0, stream>>>(
            reinterpret_cast<uint32_t*>(ws + B.tile_counts), (B.work_order - B.tile_counts) / 4,
            reinterpret_cast<uint32_t*>(ws + B.work_order), B.order_slots, pack_cameras(cams, cnt, true), cnt, W, H, cams_dev, header_tables,
            reinterpret_cast<uint32_t*>(ws + B.tables), table_words);
    }
    if (scene->tie_index && !scene->tie_inv)     // (a per-scene constant: pgr_scene_prepare computes it once)
        invert_tie_index_kernel<<<(N + 255) / 256, 256, 0, stream>>>(N, scene->tie_index,
                                                                      reinterpret_cast<uint32_t*>(ws + B.tie_inv));
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
    uint32_t* vis = call_runs_block_cull(N, n_views) ? reinterpret_cast<uint32_t*>(ws + B.vis) : nullptr;
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
            auto* dst = reinterpret_cast<uint8_t*>(ws + B.obj_u8);
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
    if (!hip_ok(hipGetLastError(), "kernel launch")) return fail(PGR_ERR_LAUNCH_FAILURE);

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
    const CameraDev* cams_dev = reinterpret_cast<const CameraDev*>(ws + B.cams);
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
                                                          reinterpret_cast<const uint32_t*>(ws + B.work_order));
    const GradOut go{grads->means2d, grads->means3d, grads->opacities, grads->colors, grads->shs, grads->cov3d,
                     grads->scales, grads->rotations};
    constexpr decltype(&preprocess_backward_batch_kernel<0, false>) pres[4][2] = {
        {preprocess_backward_batch_kernel<0, false>, preprocess_backward_batch_kernel<0, true>},
        {preprocess_backward_batch_kernel<1, false>, preprocess_backward_batch_kernel<1, true>},
        {preprocess_backward_batch_kernel<2, false>, preprocess_backward_batch_kernel<2, true>},
        {preprocess_backward_batch_kernel<3, false>, preprocess_backward_batch_kernel<3, true>}};
    auto* pre = pres[scene->shs ? scene->sh_degree : 0][one];
    pre<<<(N + 255) / 256, 256, 0, stream>>>(*scene, table, cams_dev, n_views, go);
    return hip_ok(hipGetLastError(), "backward launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    return hip_ok(hipGetLastError(), "camera backward launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
                     ? reinterpret_cast<const uint32_t*>(static_cast<char*>(workspace) + B.vis) : nullptr;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* c = static_cast<char*>(cache);
    if (scene->tie_index) {
        auto* inv = reinterpret_cast<uint32_t*>(c);
        invert_tie_index_kernel<<<(N + 255) / 256, 256, 0, stream>>>(N, scene->tie_index, inv);
        *tie_inv = inv;
    }
    if (semantic && semantic->object_id && semantic->k_objects > 0 && semantic->k_objects <= 255 && semantic->n_env >= 0 &&
        semantic->n_env < N) {
        auto* ids = reinterpret_cast<uint8_t*>(c + align_up((size_t)N * 4));
        const int n_obj = N - semantic->n_env;
        pack_object_ids_kernel<<<(n_obj + 255) / 256, 256, 0, stream>>>(semantic->object_id, semantic->n_env, N, ids);
        *object_id_u8 = ids;
    }
    return hip_ok(hipGetLastError(), "scene_prepare launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

int32_t pgr_batch_status(const void* host_scratch, int32_t n_views, int64_t* num_instances) {
    if (!host_scratch || n_views <= 0) return PGR_ERR_INVALID_ARGUMENT;
    const uint32_t* st = reinterpret_cast<const uint32_t*>(static_cast<const char*>(host_scratch) + host_tables(n_views).status);
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
    p->table = reinterpret_cast<BwdViewDev*>(static_cast<char*>(c.scratch) + S.table);
    return PGR_OK;
}

// The plan, the scene backward, then (with camera_grads) the camera kernels.
int32_t pgr_backward(const PgrBackwardCall* c, void* stream_v) {
    if (!c) return PGR_ERR_INVALID_ARGUMENT;
    BackwardPlan p{};
    if (int rc = backward_plan(*c, &p)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (c->scene->n > 0)
        if (int32_t rc = backward_impl(c->scene, c->n_views, c->views, c->grad_alpha, p.ws, p.L, p.B, c->grads, p.rows, p.table,
                                       stream))
            return rc;
    if (!c->camera_grads) return PGR_OK;
    return camera_backward_impl(c->scene, c->n_views, c->camera_grads, p.table,
                                reinterpret_cast<const CameraDev*>(p.ws + p.B.cams), static_cast<float*>(c->camera_scratch),
                                stream);
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
    compose_object_kernel<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream_v)>>>(
        n, xyz, rot, f_rest, n_rest, in_rest_stride, P, out_xyz, out_rot, out_rest, out_rest_stride);
    return hip_ok(hipGetLastError(), "compose_object launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    clock_probe_kernel<<<1, WAVE, 0, static_cast<hipStream_t>(stream_v)>>>(reinterpret_cast<unsigned long long*>(ticks), spin_us);
    return hip_ok(hipGetLastError(), "clock_probe launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

size_t pgr_pose_objects_workspace_bytes(int32_t n_jobs) {
    if (n_jobs <= 0) return 0;
    return ((size_t)n_jobs + POSE_JOBS_PER_LAUNCH - 1) / POSE_JOBS_PER_LAUNCH * POSE_LAUNCH_BYTES;
}

int32_t pgr_pose_objects(int32_t n_jobs, const PgrPoseJob* jobs, const double* sh_dirs, const double* sh_pinv,
                         void* workspace, size_t workspace_bytes, void* stream_v) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return PGR_OK;
    for (int k = 0; k < n_jobs; ++k) {
        const PgrPoseJob& j = jobs[k];
        if (j.n < 0 || (j.n > 0 && (!j.src || !j.dst)) || j.kind < PGR_POSE_XYZ || j.kind > PGR_POSE_SH ||
            (j.kind == PGR_POSE_SH && ((j.n_rest != 3 && j.n_rest != 8 && j.n_rest != 15) || !sh_dirs || !sh_pinv)))
            return PGR_ERR_INVALID_ARGUMENT;
    }
    if (!workspace || workspace_bytes < pgr_pose_objects_workspace_bytes(n_jobs)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    char* ws = static_cast<char*>(workspace);
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
        auto* partial = reinterpret_cast<double*>(ws + (size_t)launch * POSE_LAUNCH_BYTES);
        auto* poses = reinterpret_cast<ObjectPoseDev*>(ws + (size_t)launch * POSE_LAUNCH_BYTES + POSE_PART_BYTES);
        if (reduce) pose_reduce_kernel<<<dim3(POSE_REDUCE_BLOCKS, T.count), 256, 0, stream>>>(T, partial);
        pose_prepare_kernel<<<T.count, 128, 0, stream>>>(T, partial, sh_dirs, sh_pinv, poses);
        if (blocks) pose_apply_kernel<<<blocks, 256, 0, stream>>>(T, poses);
    }
    return hip_ok(hipGetLastError(), "pose_objects launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

size_t pgr_block_visibility_workspace_bytes(int32_t n, int32_t n_views) {
    if (n < 0 || n_views <= 0) return 0;
    return align_up((size_t)n_views * sizeof(CameraDev)) + align_up((size_t)((n + WAVE - 1) / WAVE) * sizeof(BlockBounds) + 1);
}

int32_t pgr_block_visibility(const PgrScene* scene, int32_t n_views, const PgrCamera* cams, void* workspace,
                             size_t workspace_bytes, uint32_t* vis_words, void* stream_v) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
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
    auto* bounds = reinterpret_cast<BlockBounds*>(ws + align_up((size_t)n_views * sizeof(CameraDev)));
    for (int v0 = 0; v0 < n_views; v0 += CAM_PACK_MAX) {
        const int cnt = std::min(CAM_PACK_MAX, n_views - v0);
        pack_camera_kernel<<<cnt, 64, 0, stream>>>(pack_cameras(cams + v0, cnt, false), W, H, cams_dev + v0);
    }
    const int groups = (scene->n + WAVE - 1) / WAVE, words = (n_views + 31) / 32;
    block_bounds_kernel<<<(groups + 3) / 4, 256, 0, stream>>>(*scene, nullptr, bounds, groups);
    block_cull_kernel<<<dim3((groups + 7) / 8, words), 256, 0, stream>>>(bounds, groups, cams_dev, n_views, words, vis_words);
    return hip_ok(hipGetLastError(), "block_visibility launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

int32_t pgr_mark_visible(int32_t n, const float* means3d, const float* viewmatrix, uint8_t* present, void* stream_v) {
    if (n < 0 || (n > 0 && (!means3d || !viewmatrix || !present))) return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    mark_visible_kernel<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream_v)>>>(n, means3d, viewmatrix,
                                                                                         present);
    return hip_ok(hipGetLastError(), "mark_visible launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

int32_t pgr_color_masks(const float* img_chw, int32_t n_images, int32_t width, int32_t height, const float* colors_k3,
                        int32_t k, float threshold, uint8_t* masks_khw, void* stream_v) {
    if (!img_chw || n_images < 0 || n_images > 65535 || width <= 0 || height <= 0 || k < 0 ||
        (k > 0 && (!colors_k3 || !masks_khw)))
        return PGR_ERR_INVALID_ARGUMENT;
    if (k == 0 || n_images == 0) return PGR_OK;
    const size_t P = (size_t)width * height;
    color_masks_kernel<<<dim3((unsigned)((P + 255) / 256), n_images), 256, 0, static_cast<hipStream_t>(stream_v)>>>(
        img_chw, P, colors_k3, k, threshold, masks_khw);
    return hip_ok(hipGetLastError(), "color_masks launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

int32_t pgr_quantize_frame(const float* img_chw, const float* depth_hw, int32_t width, int32_t height,
                           uint8_t* rgb_hwc, uint16_t* depth_mm_hw, void* stream_v) {
    if (width <= 0 || height <= 0 || ((img_chw == nullptr) != (rgb_hwc == nullptr)) ||
        ((depth_hw == nullptr) != (depth_mm_hw == nullptr)))
        return PGR_ERR_INVALID_ARGUMENT;
    const size_t P = (size_t)width * height;
    quantize_kernel<<<(unsigned)((P + 255) / 256), 256, 0, static_cast<hipStream_t>(stream_v)>>>(
        img_chw, depth_hw, P, rgb_hwc, depth_mm_hw);
    return hip_ok(hipGetLastError(), "quantize launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    pack_frames_kernel<<<dim3((unsigned)((P + 255) / 256), n_images), 256, 0, static_cast<hipStream_t>(stream_v)>>>(
        color_b3hw, depth_bhw, masks_bkhw, P, k, rgb_bhwc, depth_mm_bhw, mask_bits_bhwj);
    return hip_ok(hipGetLastError(), "pack_frames launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    pack_records_kernel<<<dim3((unsigned)((P + 255) / 256), n_images), 256, 0, static_cast<hipStream_t>(stream_v)>>>(
        color_b3hw, depth_bhw, masks_bkhw, P, k, records, (size_t)record_stride, (size_t)L.off_depth, (size_t)L.off_masks);
    return hip_ok(hipGetLastError(), "pack_records launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

}  // extern "C"

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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* ws = static_cast<char*>(workspace);
    auto* grid = reinterpret_cast<KnnGrid*>(ws + K.grid);
    auto* count = reinterpret_cast<uint32_t*>(ws + K.count);
    auto* start = reinterpret_cast<uint32_t*>(ws + K.start);
    auto* sorted = reinterpret_cast<float4*>(ws + K.sorted);
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
    return hip_ok(hipGetLastError(), "knn launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
}  // namespace

size_t pgr_radius_count_workspace_bytes(int32_t n) { return n < 0 ? 0 : radius_layout(n).total; }

int32_t pgr_radius_count(int32_t n, const float* xyz, double radius, int32_t cap, int32_t* counts, void* workspace,
                         size_t workspace_bytes, void* stream_v) {
    if (n < 0 || cap < 1 || !std::isfinite(radius) || !(radius > 0.0)) return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    if (!xyz || !counts || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    const RadiusLayout R = radius_layout(n);
    if (workspace_bytes < R.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* ws = static_cast<char*>(workspace);
    auto* total = reinterpret_cast<uint32_t*>(ws + R.total_word);
    auto* slots = reinterpret_cast<RadiusSlot*>(ws + R.slots);
    auto* begin = reinterpret_cast<uint32_t*>(ws + R.begin);
    auto* point_slot = reinterpret_cast<uint32_t*>(ws + R.point_slot);
    auto* sorted = reinterpret_cast<float4*>(ws + R.sorted);
    // the running total and the table lie one behind the other: one memset
    if (!hip_ok(hipMemsetAsync(total, 0, R.begin - R.total_word, stream), "memset radius table")) return PGR_ERR_LAUNCH_FAILURE;
    const double inv_h = 1.0 / (radius * RADIUS_CELL_MARGIN), r2 = radius * radius;
    const uint32_t mask = (uint32_t)(R.n_slots - 1);
    const int blocks = (n + RADIUS_BLOCK - 1) / RADIUS_BLOCK;
    radius_insert_kernel<<<blocks, RADIUS_BLOCK, 0, stream>>>(n, xyz, inv_h, slots, mask, point_slot);
    radius_ranges_kernel<<<(unsigned)(R.n_slots / RADIUS_BLOCK), RADIUS_BLOCK, 0, stream>>>(slots, begin, total);
    radius_scatter_kernel<<<blocks, RADIUS_BLOCK, 0, stream>>>(n, xyz, point_slot, begin, sorted);
    radius_count_kernel<<<blocks, RADIUS_BLOCK, 0, stream>>>(n, sorted, slots, begin, mask, inv_h, r2, cap, counts);
    return hip_ok(hipGetLastError(), "radius count launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

// ---- registration: correspondences, ICP sums, normals by radius (registration.hip.h) --------------------------------------
namespace {
struct RadiusGrid { uint32_t* total; RadiusSlot* slots; uint32_t* begin; uint32_t* point_slot; float4* sorted; uint32_t mask; };
RadiusGrid radius_grid(const RadiusLayout& R, void* workspace) {
    char* ws = static_cast<char*>(workspace);
    return RadiusGrid{reinterpret_cast<uint32_t*>(ws + R.total_word), reinterpret_cast<RadiusSlot*>(ws + R.slots),
                      reinterpret_cast<uint32_t*>(ws + R.begin), reinterpret_cast<uint32_t*>(ws + R.point_slot),
                      reinterpret_cast<float4*>(ws + R.sorted), (uint32_t)(R.n_slots - 1)};
}
// files the n points of `xyz` into the grid (the first three kernels of pgr_radius_count); afterwards begin[] holds the ends
bool radius_grid_build(int32_t n, const float* xyz, double inv_h, const RadiusLayout& R, const RadiusGrid& G, hipStream_t stream) {
    if (!hip_ok(hipMemsetAsync(G.total, 0, R.begin - R.total_word, stream), "memset radius table")) return false;
    const int blocks = (n + RADIUS_BLOCK - 1) / RADIUS_BLOCK;
    radius_insert_kernel<<<blocks, RADIUS_BLOCK, 0, stream>>>(n, xyz, inv_h, G.slots, G.mask, G.point_slot);
    radius_ranges_kernel<<<(unsigned)(R.n_slots / RADIUS_BLOCK), RADIUS_BLOCK, 0, stream>>>(G.slots, G.begin, G.total);
    radius_scatter_kernel<<<blocks, RADIUS_BLOCK, 0, stream>>>(n, xyz, G.point_slot, G.begin, G.sorted);
    return true;
}
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (!radius_grid_build(n_target, target, 1.0 / (max_distance * RADIUS_CELL_MARGIN), R, radius_grid(R, workspace), stream))
        return PGR_ERR_LAUNCH_FAILURE;
    return hip_ok(hipGetLastError(), "nn grid launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* ws = static_cast<char*>(workspace);
    auto* posed = reinterpret_cast<float*>(ws + L.posed);
    const RadiusLayout R = radius_layout(n_source);
    const RadiusGrid G = radius_grid(R, ws + L.grid);
    registration_pose_kernel<<<reg_blocks(n_source), REG_BLOCK, 0, stream>>>(n_source, source, P, posed);
    if (!radius_grid_build(n_source, posed, 1.0 / (max_distance * RADIUS_CELL_MARGIN), R, G, stream)) return PGR_ERR_LAUNCH_FAILURE;
    registration_order_kernel<<<reg_blocks(n_source), REG_BLOCK, 0, stream>>>(n_source, G.sorted, order);
    return hip_ok(hipGetLastError(), "nn source order launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    registration_correspond_kernel<<<reg_blocks(n_source), REG_BLOCK, 0, static_cast<hipStream_t>(stream_v)>>>(
        n_source, source, order, P, n_target, G.sorted, G.slots, G.begin, G.mask, 1.0 / (max_distance * RADIUS_CELL_MARGIN),
        max_distance * max_distance, index, d2);
    return hip_ok(hipGetLastError(), "nn correspond launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

size_t pgr_icp_sums_workspace_bytes(int32_t n_source) {
    return n_source < 0 ? 0 : align_up((size_t)std::max(reg_blocks(n_source), 1) * REG_SUMS * sizeof(double));
}

int32_t pgr_icp_sums(int32_t n_source, const float* source, const double* transformation, const int32_t* index,
                     const double* d2, int32_t n_target, const float* target, const double* target_normals, double* sums,
                     void* workspace, size_t workspace_bytes, void* stream_v) {
    RegPose P;
    if (n_source < 0 || n_target < 0 || !reg_pose(transformation, P) || !sums) return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (n_source == 0 || n_target == 0)                          // nothing corresponds: every sum is 0
        return hip_ok(hipMemsetAsync(sums, 0, REG_SUMS * sizeof(double), stream), "memset icp sums") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
    if (!source || !index || !d2 || !target || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < pgr_icp_sums_workspace_bytes(n_source)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    auto* partials = static_cast<double*>(workspace);
    const int32_t blocks = reg_blocks(n_source);
    registration_sums_kernel<<<blocks, REG_BLOCK, 0, stream>>>(n_source, source, P, index, d2, n_target, target, target_normals,
                                                               partials);
    registration_sums_final_kernel<<<1, REG_FINAL_BLOCK, 0, stream>>>(blocks, partials, sums);
    return hip_ok(hipGetLastError(), "icp sums launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

size_t pgr_radius_normals_workspace_bytes(int32_t n) { return n < 0 ? 0 : radius_layout(n).total; }

int32_t pgr_radius_normals(int32_t n, const float* xyz, double radius, double* normals, int32_t* counts, void* workspace,
                           size_t workspace_bytes, void* stream_v) {
    if (n < 0 || !distance_ok(radius)) return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    if (!xyz || !normals || !counts || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    const RadiusLayout R = radius_layout(n);
    if (workspace_bytes < R.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const RadiusGrid G = radius_grid(R, workspace);
    const double inv_h = 1.0 / (radius * RADIUS_CELL_MARGIN);
    if (!radius_grid_build(n, xyz, inv_h, R, G, stream)) return PGR_ERR_LAUNCH_FAILURE;
    registration_normals_kernel<<<reg_blocks(n), REG_BLOCK, 0, stream>>>(n, G.sorted, G.slots, G.begin, G.mask, inv_h,
                                                                        radius * radius, normals, counts);
    return hip_ok(hipGetLastError(), "radius normals launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (n == 0) {                                                // no row is inside [0, 0): every hypothesis is invalid
        if (!hip_ok(hipMemsetAsync(planes, 0, (size_t)n_hyp * 4 * sizeof(double), stream), "memset planes") ||
            !hip_ok(hipMemsetAsync(valid, 0, (size_t)n_hyp, stream), "memset plane validity"))
            return PGR_ERR_LAUNCH_FAILURE;
        return PGR_OK;
    }
    plane_hypotheses_kernel<<<plane_blocks(n_hyp, PLANE_BLOCK), PLANE_BLOCK, 0, stream>>>(n, xyz, n_hyp, triples, planes, valid);
    return hip_ok(hipGetLastError(), "plane hypotheses launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

size_t pgr_plane_score_workspace_bytes(int32_t n, int32_t n_hyp) {
    return n < 0 || n_hyp < 0 ? 0 : plane_score_layout(n, n_hyp).total;
}

int32_t pgr_plane_score(int32_t n, const float* xyz, int32_t n_hyp, const double* planes, double threshold, int32_t* counts,
                        double* sumsq, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (n < 0 || n_hyp < 0 || !distance_ok(threshold)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_hyp == 0) return PGR_OK;
    if (!counts || !sumsq) return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (n == 0) {                                                // no point: every score is 0
        if (!hip_ok(hipMemsetAsync(counts, 0, (size_t)n_hyp * sizeof(int32_t), stream), "memset plane counts") ||
            !hip_ok(hipMemsetAsync(sumsq, 0, (size_t)n_hyp * sizeof(double), stream), "memset plane sums"))
            return PGR_ERR_LAUNCH_FAILURE;
        return PGR_OK;
    }
    if (!xyz || !planes || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    const PlaneScoreLayout L = plane_score_layout(n, n_hyp);
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    char* ws = static_cast<char*>(workspace);
    auto* part_sumsq = reinterpret_cast<double*>(ws + L.sumsq);
    auto* part_count = reinterpret_cast<int32_t*>(ws + L.count);
    // few tiles: the batches of hypotheses are spread over gridDim.y (at most PLANE_SCORE_MIN_BLOCKS groups)
    const int32_t batches = plane_blocks(n_hyp, PLANE_HYP_BATCH);
    const int32_t wanted = std::min(batches, (PLANE_SCORE_MIN_BLOCKS + L.blocks - 1) / L.blocks);
    const int32_t per_group = (batches + wanted - 1) / wanted;
    const dim3 grid((unsigned)L.blocks, (unsigned)((batches + per_group - 1) / per_group));
    plane_score_kernel<<<grid, PLANE_BLOCK, 0, stream>>>(n, xyz, n_hyp, planes, threshold, per_group, part_sumsq, part_count);
    if (!hip_ok(hipGetLastError(), "plane score launch")) return PGR_ERR_LAUNCH_FAILURE;     // (no second pass over nothing)
    plane_score_final_kernel<<<plane_blocks(n_hyp, PLANE_BLOCK), PLANE_BLOCK, 0, stream>>>(L.blocks, n_hyp, part_sumsq, part_count,
                                                                                        counts, sumsq);
    return hip_ok(hipGetLastError(), "plane score final launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (n == 0)                                                  // no point: every sum is 0
        return hip_ok(hipMemsetAsync(sums, 0, PLANE_SUM_TERMS * sizeof(double), stream), "memset plane sums") ? PGR_OK
                                                                                                                 : PGR_ERR_LAUNCH_FAILURE;
    if (!xyz || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < pgr_plane_inliers_workspace_bytes(n)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    auto* partials = static_cast<double*>(workspace);
    const int32_t blocks = plane_blocks(n, PLANE_BLOCK);
    plane_inliers_kernel<<<blocks, PLANE_BLOCK, 0, stream>>>(n, xyz, P, threshold, mask, partials);
    if (!hip_ok(hipGetLastError(), "plane inliers launch")) return PGR_ERR_LAUNCH_FAILURE;
    plane_inliers_final_kernel<<<1, PLANE_FINAL_BLOCK, 0, stream>>>(blocks, partials, sums);
    return hip_ok(hipGetLastError(), "plane inliers final launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

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
}  // namespace

int32_t pgr_tsdf_integrate(const PgrGrid* grid, int32_t n_views, const PgrCamera* cameras, const float* depth,
                           const float* final_T, float truncation, float alpha_min, float* sdf, void* stream_v) {
    if (!grid_ok(grid) || n_views < 1 || n_views > TSDF_MAX_VIEWS || !cameras || !depth || !final_T || !sdf)
        return PGR_ERR_INVALID_ARGUMENT;
    if (!(truncation > 0.f) || !std::isfinite(truncation) || std::isnan(alpha_min)) return PGR_ERR_INVALID_ARGUMENT;
    const int32_t W = cameras[0].image_width, H = cameras[0].image_height;
    if (W <= 0 || H <= 0 || (int64_t)W * H > (int64_t)1 << 28) return PGR_ERR_INVALID_ARGUMENT;
    TsdfArgs a{};
    for (int32_t v = 0; v < n_views; ++v) {
        const PgrCamera& c = cameras[v];
        if (c.image_width != W || c.image_height != H || !c.viewmatrix || !(c.tanfovx > 0.f) || !(c.tanfovy > 0.f))
            return PGR_ERR_INVALID_ARGUMENT;
        a.view[v] = c.viewmatrix;
        a.fx[v] = (float)((double)W / (2.0 * (double)c.tanfovx));
        a.fy[v] = (float)((double)H / (2.0 * (double)c.tanfovy));
    }
    a.g = mesh_grid(grid);
    a.n_views = n_views;
    a.width = W;
    a.height = H;
    a.cx = (float)(W - 1) * 0.5f;
    a.cy = (float)(H - 1) * 0.5f;
    a.truncation = truncation;
    a.alpha_min = alpha_min;
    a.depth = depth;
    a.final_T = final_T;
    a.sdf = sdf;
    const dim3 block(TSDF_BX, TSDF_BY, TSDF_BZ);
    const dim3 blocks((grid->nx + TSDF_BX - 1) / TSDF_BX, (grid->ny + TSDF_BY - 1) / TSDF_BY, (grid->nz + TSDF_BZ - 1) / TSDF_BZ);
    tsdf_integrate_kernel<<<blocks, block, 0, static_cast<hipStream_t>(stream_v)>>>(a);
    return hip_ok(hipGetLastError(), "tsdf_integrate launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* ws = static_cast<char*>(workspace);
    auto* tile_tot = reinterpret_cast<long long*>(ws + M.tile_tot);
    march_count_kernel<<<M.tiles, MARCH_THREADS, 0, stream>>>(mesh_grid(grid), sdf, n, reinterpret_cast<uint8_t*>(ws + M.mask),
                                                              reinterpret_cast<uint8_t*>(ws + M.ntri), tile_tot);
    auto* tile_off = reinterpret_cast<long long*>(ws + M.tile_off);
    march_scan_kernel<<<1, MARCH_SCAN_THREADS, 0, stream>>>(tile_tot, M.tiles, tile_off, reinterpret_cast<long long*>(counts));
    march_vbase_kernel<<<M.tiles, MARCH_THREADS, 0, stream>>>(n, reinterpret_cast<uint8_t*>(ws + M.mask), tile_off,
                                                              reinterpret_cast<int32_t*>(ws + M.vbase));
    return hip_ok(hipGetLastError(), "march_count launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

int32_t pgr_march_emit(const PgrGrid* grid, const float* sdf, const void* workspace, size_t workspace_bytes, float* vertices,
                       int32_t* faces, void* stream_v) {
    if (!grid_ok(grid) || !sdf || !workspace || !vertices || !faces) return PGR_ERR_INVALID_ARGUMENT;
    const size_t n = grid_points(grid);
    const MarchLayout M = march_layout(n);
    if (workspace_bytes < M.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const char* ws = static_cast<const char*>(workspace);
    const auto* mask = reinterpret_cast<const uint8_t*>(ws + M.mask);
    const auto* tile_off = reinterpret_cast<const long long*>(ws + M.tile_off);
    const auto* vbase = reinterpret_cast<const int32_t*>(ws + M.vbase);
    march_vertices_kernel<<<(unsigned)((n + MARCH_THREADS - 1) / MARCH_THREADS), MARCH_THREADS, 0, stream>>>(
        mesh_grid(grid), sdf, n, mask, vbase, vertices);
    march_faces_kernel<<<M.tiles, MARCH_THREADS, 0, stream>>>(mesh_grid(grid), sdf, n, mask,
                                                              reinterpret_cast<const uint8_t*>(ws + M.ntri), tile_off, vbase,
                                                              faces);
    return hip_ok(hipGetLastError(), "march_emit launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const size_t plane = (size_t)width * height, total = plane * (size_t)n_slots;
    if (!hip_ok(hipMemsetAsync(out, 0xFF, total * sizeof(Pix), stream), what) ||
        !hip_ok(hipMemsetAsync(straddle_count, 0, sizeof(int32_t), stream), what))
        return PGR_ERR_LAUNCH_FAILURE;
    char* ws = static_cast<char*>(workspace);
    auto* qctr = reinterpret_cast<unsigned long long*>(ws + L.qctr);
    auto* queue = reinterpret_cast<MeshQueueEntry*>(ws + L.queue);
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
    return hip_ok(hipGetLastError(), what) ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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

int32_t pgr_mesh_shade(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t n_jobs,
                       const PgrMeshJob* jobs, int32_t width, int32_t height, float near_z, const uint64_t* keys,
                       int32_t n_slots, const PgrMeshShade* shade, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (n_jobs > MESHV_MAX_JOBS || !keys || !shade || std::isnan(shade->ambient) || reinterpret_cast<uintptr_t>(keys) % sizeof(uint64_t) ||
        reinterpret_cast<uintptr_t>(workspace) % alignof(MeshShadeJobDev) ||
        !mesh_call_ok(vertices, n_vertices, faces, n_faces, n_jobs, jobs, width, height, near_z, n_slots))
        return PGR_ERR_INVALID_ARGUMENT;
    const size_t need = pgr_mesh_shade_workspace_bytes(n_jobs, jobs);
    if (n_jobs > 0 && (!need || !workspace || workspace_bytes < need)) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    auto* table = static_cast<MeshShadeJobDev*>(workspace);
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
    mesh_shade_kernel<<<grid, MESHS_THREADS, 0, stream>>>(A);
    return hip_ok(hipGetLastError(), "mesh_shade launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
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
    return hip_ok(hipGetLastError(), "bop_gt_info launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
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
    return hip_ok(hipGetLastError(), "pose_errors launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

size_t pgr_pose_adi_workspace_bytes(int32_t n_jobs, const PgrPoseErrorJob* jobs) { return adi_layout(n_jobs, jobs).total; }

int32_t pgr_pose_adi(const float* vertices, int64_t n_vertices, int32_t n_jobs, const PgrPoseErrorJob* jobs, float* adi,
                     void* workspace, size_t workspace_bytes, void* stream_v) {
    if (!pose_vertices_ok(vertices, n_vertices, n_jobs, jobs) || (n_jobs > 0 && !adi)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return PGR_OK;
    const AdiLayout L = adi_layout(n_jobs, jobs);
    if (!L.total) return PGR_ERR_INVALID_ARGUMENT;
    if (!workspace || workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    auto* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + L.partials);
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
    return hip_ok(hipGetLastError(), "pose_adi launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
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
    return hip_ok(hipGetLastError(), "obb_candidates launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
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
    return hip_ok(hipGetLastError(), "point_diameter launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* ws = static_cast<char*>(workspace);
    auto* planes = reinterpret_cast<uint32_t*>(ws + L.planes);
    auto* columns = reinterpret_cast<RleColumn*>(ws + L.columns);
    rle_planes_kernel<<<(unsigned)L.plane_blocks, RLE_THREADS, 0, stream>>>(masks, width, height, L.S, L.Wp, L.col_tiles,
                                                                            L.row_groups, planes);
    rle_columns_kernel<<<(unsigned)L.column_blocks, RLE_THREADS, 0, stream>>>(planes, width, height, L.S, L.Wp, L.col_blocks,
                                                                              columns);
    rle_scan_kernel<<<(unsigned)n_masks, RLE_THREADS, 0, stream>>>(columns, width, height, stats);
    return hip_ok(hipGetLastError(), "mask_rle_count launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    const char* ws = static_cast<const char*>(workspace);
    rle_emit_kernel<<<(unsigned)L.column_blocks, RLE_THREADS, 0, static_cast<hipStream_t>(stream_v)>>>(
        reinterpret_cast<const uint32_t*>(ws + L.planes), reinterpret_cast<const RleColumn*>(ws + L.columns), width, height, L.S,
        L.Wp, L.col_blocks, reinterpret_cast<const long long*>(offsets), counts, (long long)total);
    return hip_ok(hipGetLastError(), "mask_rle_emit launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

int32_t pgr_mask_rle_decode(const int32_t* counts, const int64_t* offsets, int32_t n_masks, int32_t width, int32_t height,
                            uint8_t* masks, void* stream_v) {
    if (!counts || !offsets || !masks || !rle_shape_ok(n_masks, width, height)) return PGR_ERR_INVALID_ARGUMENT;
    const int64_t HW = (int64_t)width * height;
    const int64_t slice = std::max<int64_t>(RLE_DECODE_MIN_SLICE, (HW + RLE_DECODE_MAX_SLICES - 1) / RLE_DECODE_MAX_SLICES);
    const int64_t slices = (HW + slice - 1) / slice;
    if ((int64_t)n_masks * slices > MAX_GRID_BLOCKS) return PGR_ERR_INVALID_ARGUMENT;
    rle_decode_kernel<<<(unsigned)(n_masks * slices), RLE_THREADS, 0, static_cast<hipStream_t>(stream_v)>>>(
        counts, reinterpret_cast<const long long*>(offsets), width, height, (int)slices, (int)slice, masks);
    return hip_ok(hipGetLastError(), "mask_rle_decode launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

int32_t pgr_mask_overlap(const uint8_t* a, int32_t n_a, const uint8_t* b, int32_t n_b, int32_t width, int32_t height,
                         int32_t* inter, int32_t* area_a, int32_t* area_b, void* stream_v) {
    if (!a || !b || !inter || !area_a || !area_b || !rle_shape_ok(n_a, width, height) || !rle_shape_ok(n_b, width, height))
        return PGR_ERR_INVALID_ARGUMENT;
    const size_t HW = (size_t)width * height;
    const int64_t chunks = (int64_t)((HW + OVERLAP_CHUNK - 1) / OVERLAP_CHUNK);
    const int64_t pairs = (int64_t)n_a * n_b;
    if (pairs > MAX_GRID_BLOCKS || pairs * chunks > MAX_GRID_BLOCKS) return PGR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (!hip_ok(hipMemsetAsync(inter, 0, (size_t)pairs * sizeof(int32_t), stream), "mask_overlap clear") ||
        !hip_ok(hipMemsetAsync(area_a, 0, (size_t)n_a * sizeof(int32_t), stream), "mask_overlap clear") ||
        !hip_ok(hipMemsetAsync(area_b, 0, (size_t)n_b * sizeof(int32_t), stream), "mask_overlap clear"))
        return PGR_ERR_LAUNCH_FAILURE;
    mask_overlap_kernel<<<(unsigned)(pairs * chunks), RLE_THREADS, 0, stream>>>(a, n_a, b, n_b, HW, (int)chunks, inter, area_a,
                                                                               area_b);
    return hip_ok(hipGetLastError(), "mask_overlap launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* ws = static_cast<char*>(workspace);
    auto* groups_dev = reinterpret_cast<PgrCocoGroup*>(ws + L.groups);
    auto* dt_ends = reinterpret_cast<int32_t*>(ws + L.dt_ends);
    auto* gt_ends = reinterpret_cast<int32_t*>(ws + L.gt_ends);
    auto* gt_cover = reinterpret_cast<int32_t*>(ws + L.gt_cover);
    auto* dt_cover = reinterpret_cast<int32_t*>(ws + L.dt_cover);
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
    return hip_ok(hipGetLastError(), "rle_iou launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    auto* groups_dev = reinterpret_cast<PgrCocoGroup*>(static_cast<char*>(workspace) + L.groups);
    if (!coco_groups_upload(groups_dev, groups, n_groups, stream)) return PGR_ERR_LAUNCH_FAILURE;
    coco_box_iou_kernel<<<(unsigned)n_groups, COCO_THREADS, 0, stream>>>(groups_dev, dt_boxes, gt_boxes, gt_crowd, iou);
    return hip_ok(hipGetLastError(), "box_iou launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* ws = static_cast<char*>(workspace);
    auto* groups_dev = reinterpret_cast<PgrCocoGroup*>(ws + L.groups);
    auto* order = reinterpret_cast<int32_t*>(ws + L.order);
    if (!coco_groups_upload(groups_dev, groups, n_groups, stream)) return PGR_ERR_LAUNCH_FAILURE;
    coco_match_kernel<<<(unsigned)n_groups, WAVE, 0, stream>>>(groups_dev, P, iou, dt_area, gt_area, gt_flag, gt_crowd, (long long)n_dt,
                                                              (long long)n_gt, order, dt_match, dt_ignore, gt_match, gt_ignore);
    return hip_ok(hipGetLastError(), "coco_match launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    char* ws = static_cast<char*>(workspace);
    auto* ws_tp = reinterpret_cast<int32_t*>(ws + L.tp);
    auto* ws_idx = reinterpret_cast<int32_t*>(ws + L.idx);
    auto* ws_pr = reinterpret_cast<double*>(ws + L.pr);
    coco_accumulate_kernel<<<(unsigned)(n_cat * n_area * n_max_dets), COCO_THREADS, 0, static_cast<hipStream_t>(stream_v)>>>(
        P, reinterpret_cast<const long long*>(perm), reinterpret_cast<const long long*>(seg_start), (long long)n_dt, rank, dt_match,
        dt_ignore, npig, rec_thrs, dt_scores, ws_tp, ws_idx, ws_pr, precision, scores, recall);
    return hip_ok(hipGetLastError(), "coco_accumulate launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

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
                             nullptr, workspace, static_cast<hipStream_t>(stream_v));
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
                             grad_alpha, workspace, static_cast<hipStream_t>(stream_v));
}

namespace {
int32_t image_loss_launch(const LossLayout& L, const float* x, const float* y, const float* mask, const float* bg,
                          const float* alpha, int32_t height, int32_t width, double lambda_dssim, double lambda_alpha,
                          float* out3, float* out_a, float* grad, float* grad_alpha, void* workspace,
                          hipStream_t stream) {
    char* ws = static_cast<char*>(workspace);
    auto* A = reinterpret_cast<float*>(ws + L.a);
    auto* B = reinterpret_cast<float*>(ws + L.b);
    auto* Cm = reinterpret_cast<float*>(ws + L.c);
    auto* partial = reinterpret_cast<double*>(ws + L.partial);
    const LossWindow win = ssim_window();
    const dim3 grid(L.tiles_x, L.tiles_y, 3);
    const int n_blocks = 3 * L.tiles_x * L.tiles_y;
    const double n_values = 3.0 * (double)height * (double)width;
    const double n_pix = (double)height * (double)width;
    auto* partial_a = alpha ? reinterpret_cast<double*>(ws + L.partial_a) : nullptr;
    loss_ssim_kernel<<<grid, 256, 0, stream>>>(x, y, height, width, win, A, B, Cm, partial, mask, bg, alpha,
                                               (float)(lambda_alpha / n_pix), grad_alpha, partial_a);
    if (grad)
        loss_grad_kernel<<<grid, 256, 0, stream>>>(x, y, height, width, win, A, B, Cm, (float)(-lambda_dssim / n_values),
                                                   (float)((1.0 - lambda_dssim) / n_values), grad, mask, bg);
    loss_reduce_kernel<<<1, 256, 0, stream>>>(partial, n_blocks, 1.0 / n_values, lambda_dssim, out3, partial_a,
                                              L.tiles_x * L.tiles_y, 1.0 / n_pix, lambda_alpha, out_a);
    return hip_ok(hipGetLastError(), "image loss launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    adam_step_kernel<<<(unsigned)blocks, 256, 0, static_cast<hipStream_t>(stream_v)>>>(a);
    return hip_ok(hipGetLastError(), "adam launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

int32_t pgr_densify_stats(int32_t n, const float* viewspace_grad, int32_t grad_stride, const int32_t* radii,
                          float* grad_accum, float* denom, float* max_radii2d, void* stream_v) {
    if (n < 0 || grad_stride < 2) return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    if (!viewspace_grad || !radii || !grad_accum || !denom || !max_radii2d) return PGR_ERR_INVALID_ARGUMENT;
    densify_stats_kernel<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream_v)>>>(
        n, viewspace_grad, grad_stride, radii, grad_accum, denom, max_radii2d);
    return hip_ok(hipGetLastError(), "densify stats launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (!hip_ok(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), stream), "memset cluster counts")) return PGR_ERR_LAUNCH_FAILURE;
    if (n_vertices == 0) return PGR_OK;                                     // (no vertex: no cluster, and no face can be kept)
    char* ws = static_cast<char*>(workspace);
    const DecSortBuffers S{{reinterpret_cast<uint64_t*>(ws + D.key_a), reinterpret_cast<uint64_t*>(ws + D.key_b)},
                           {reinterpret_cast<uint32_t*>(ws + D.val_a), reinterpret_cast<uint32_t*>(ws + D.val_b)},
                           reinterpret_cast<uint32_t*>(ws + D.hist)};
    auto* flag = reinterpret_cast<uint32_t*>(ws + D.flag);
    auto* number = reinterpret_cast<uint32_t*>(ws + D.number);
    auto* block_tot = reinterpret_cast<uint32_t*>(ws + D.block_tot);
    auto* cluster_of_vertex = reinterpret_cast<int32_t*>(ws + D.cluster_of_vertex);
    auto* tri = reinterpret_cast<int32_t*>(ws + D.tri);
    auto* rank = reinterpret_cast<uint32_t*>(ws + D.rank);
    const uint32_t V = (uint32_t)n_vertices, F = (uint32_t)n_faces;
    const DecGrid g{{lo_x, lo_y, lo_z}, voxel};

    dec_vertex_key_kernel<<<dec_blocks(V), DEC_BLOCK, 0, stream>>>(V, vertices, g, S.key[0], S.val[0]);
    int at = dec_sort(V, 60, S, stream);
    dec_key_heads_kernel<<<dec_blocks(V), DEC_BLOCK, 0, stream>>>(V, S.key[at], flag);
    dec_flag_scan(V, flag, block_tot, number, stream);
    dec_cluster_write_kernel<<<dec_blocks(V), DEC_BLOCK, 0, stream>>>(
        V, S.key[at], S.val[at], number, cluster_of_vertex, reinterpret_cast<uint32_t*>(ws + D.order),
        reinterpret_cast<uint32_t*>(ws + D.start), reinterpret_cast<uint64_t*>(ws + D.cluster_key),
        reinterpret_cast<long long*>(counts));
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
        dec_face_heads_kernel<<<dec_blocks(F), DEC_BLOCK, 0, stream>>>(F, tri, S.val[at], reinterpret_cast<uint32_t*>(ws + D.perm),
                                                                       flag);
        dec_flag_scan(F, flag, block_tot, rank, stream);
        dec_face_total_kernel<<<1, 1, 0, stream>>>(F, rank, reinterpret_cast<long long*>(counts));
    }
    return hip_ok(hipGetLastError(), "mesh_cluster_count launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    char* ws = static_cast<char*>(workspace);
    const DecSortBuffers S{{reinterpret_cast<uint64_t*>(ws + D.key_a), reinterpret_cast<uint64_t*>(ws + D.key_b)},
                           {reinterpret_cast<uint32_t*>(ws + D.val_a), reinterpret_cast<uint32_t*>(ws + D.val_b)},
                           reinterpret_cast<uint32_t*>(ws + D.hist)};
    const auto* cov = reinterpret_cast<const int32_t*>(ws + D.cluster_of_vertex);
    auto* corner_begin = reinterpret_cast<uint32_t*>(ws + D.corner_begin);
    auto* corner_end = reinterpret_cast<uint32_t*>(ws + D.corner_end);
    const uint32_t V = (uint32_t)n_vertices, F = (uint32_t)n_faces;
    if (!hip_ok(hipMemcpyAsync(cluster_of_vertex, cov, (size_t)V * sizeof(int32_t), hipMemcpyDeviceToDevice, stream),
                "memcpy cluster_of_vertex"))
        return PGR_ERR_LAUNCH_FAILURE;
    if (n_out_faces > 0)
        dec_face_emit_kernel<<<dec_blocks(F), DEC_BLOCK, 0, stream>>>(F, reinterpret_cast<const int32_t*>(ws + D.tri),
                                                                      reinterpret_cast<const uint32_t*>(ws + D.perm),
                                                                      reinterpret_cast<const uint32_t*>(ws + D.rank), n_out_faces,
                                                                      out_faces);
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
        a.order = reinterpret_cast<const uint32_t*>(ws + D.order);
        a.start = reinterpret_cast<const uint32_t*>(ws + D.start);
        a.cluster_key = reinterpret_cast<const uint64_t*>(ws + D.cluster_key);
        a.corner = S.val[at];
        a.corner_begin = corner_begin;
        a.corner_end = corner_end;
        a.n_clusters = n_clusters;
        a.quadric = quadric ? 1 : 0;
        a.out = out_vertices;
        a.used_quadric = used_quadric;
        dec_position_kernel<<<(unsigned)((n_clusters + DEC_WAVES - 1) / DEC_WAVES), DEC_BLOCK, 0, stream>>>(a);
    }
    return hip_ok(hipGetLastError(), "mesh_cluster_emit launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    auto* sums = static_cast<long long*>(workspace);
    if (!hip_ok(hipMemsetAsync(sums, 0, pgr_mesh_vertex_normals_workspace_bytes(n_vertices), stream), "memset normal sums"))
        return PGR_ERR_LAUNCH_FAILURE;
    if (n_faces > 0)
        vertex_normals_accumulate_kernel<<<attr_blocks(n_faces), MESHATTR_THREADS, 0, stream>>>(n_vertices, vertices, n_faces, faces,
                                                                                               sums);
    vertex_normals_finalize_kernel<<<attr_blocks(n_vertices), MESHATTR_THREADS, 0, stream>>>(n_vertices, sums, normals);
    return hip_ok(hipGetLastError(), "mesh_vertex_normals launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

int32_t pgr_mesh_vertex_colors(int32_t n_vertices, const float* vertices, const float* normals, int32_t n_views,
                               const PgrCamera* cameras, const float* color, const float* depth, const float* final_T,
                               float depth_tol, float alpha_min, float cos_min, const float* fill, float* colors, int32_t* seen,
                               void* stream_v) {
    if (n_vertices < 0 || n_views < 1 || n_views > TSDF_MAX_VIEWS || !cameras || !color || !depth || !final_T || !fill)
        return PGR_ERR_INVALID_ARGUMENT;
    if (!(alpha_min > 0.f) || !(depth_tol >= 0.f) || std::isnan(cos_min)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_vertices > 0 && (!vertices || !colors)) return PGR_ERR_INVALID_ARGUMENT;
    const int32_t W = cameras[0].image_width, H = cameras[0].image_height;
    if (W <= 0 || H <= 0 || (int64_t)W * H > (int64_t)1 << 28) return PGR_ERR_INVALID_ARGUMENT;
    VertexColorArgs a{};
    for (int32_t v = 0; v < n_views; ++v) {
        const PgrCamera& c = cameras[v];
        if (c.image_width != W || c.image_height != H || !c.viewmatrix || !c.campos || !(c.tanfovx > 0.f) || !(c.tanfovy > 0.f))
            return PGR_ERR_INVALID_ARGUMENT;
        a.view[v] = c.viewmatrix;
        a.campos[v] = c.campos;
        a.fx[v] = (float)((double)W / (2.0 * (double)c.tanfovx));
        a.fy[v] = (float)((double)H / (2.0 * (double)c.tanfovy));
    }
    if (n_vertices == 0) return PGR_OK;
    a.n_vertices = n_vertices;
    a.n_views = n_views;
    a.width = W;
    a.height = H;
    a.cx = (float)(W - 1) * 0.5f;
    a.cy = (float)(H - 1) * 0.5f;
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
    vertex_colors_kernel<<<attr_blocks(n_vertices), MESHATTR_THREADS, 0, static_cast<hipStream_t>(stream_v)>>>(a);
    return hip_ok(hipGetLastError(), "mesh_vertex_colors launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    mesh_sdf_kernel<<<(uint32_t)((n + SDF_THREADS - 1) / SDF_THREADS), SDF_THREADS, 0, static_cast<hipStream_t>(stream_v)>>>(
        mesh_grid(grid), vertices, n_vertices, faces, n_faces, sdf, winding);
    return hip_ok(hipGetLastError(), "mesh_sdf launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}

int32_t pgr_sdf_sample(const PgrGrid* grid, const float* sdf, int64_t n_points, const float* points, float* values,
                       float* gradients, void* stream_v) {
    if (!grid_ok(grid) || !sdf || n_points < 0 || n_points > ((int64_t)1 << 38)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_points > 0 && (!points || !values)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_points == 0) return PGR_OK;
    sdf_sample_kernel<<<(uint32_t)((n_points + 255) / 256), 256, 0, static_cast<hipStream_t>(stream_v)>>>(
        mesh_grid(grid), sdf, (long long)n_points, points, values, gradients);
    return hip_ok(hipGetLastError(), "sdf_sample launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
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
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
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
    return hip_ok(hipGetLastError(), "sdf_sweep launch") ? PGR_OK : PGR_ERR_LAUNCH_FAILURE;
}
