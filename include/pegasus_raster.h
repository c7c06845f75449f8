/*
 * pegasus_raster.h -- C ABI of libpegasus_raster.so, the MI355X (gfx950) Gaussian-splatting
 * rasterizer that replaces PEGASUS's CUDA extension `diff_gaussian_rasterization._C`.
 *
 * What each entry point replaces.  The reference binds its rasterizer through a PyTorch C++
 * extension that lives in an absent, un-pinned submodule
 * (/root/reference/.gitmodules:1-3 ; installed by /root/reference/setup.sh:19), so the
 * citations are to the reference's CALL SITES of that extension's Python surface:
 *
 *   pgr_forward            <- _C.rasterize_gaussians(...) behind GaussianRasterizer.forward;
 *                             reached from render(): /root/reference/src/gs/render.py:16,57,86,118,
 *                             /root/reference/pegasus.py:271
 *   pgr_mark_visible       <- _C.mark_visible behind GaussianRasterizer.markVisible
 *   pgr_color_masks        <- the colour-distance masks /root/reference/src/gs/render.py:60-63,89-93
 *   pgr_quantize_frame     <- (img*255).astype(uint8), (depth*1000).astype(uint16):
 *                             /root/reference/pegasus.py:347,355
 *   pgr_pack_records       <- the same casts for a whole batch + the K masks as bit planes, ONE record per frame: what the
 *                             writer threads of /root/reference/pegasus.py:346-358 consume / what the gather to the root
 *                             rank carries
 *   pgr_forward + PgrLayers <- render_silhouette_mask, /root/reference/src/gs/render.py:36-65 (every object rendered
 *                             ALONE and thresholded), for all objects and a batch of cameras in one pipeline pass
 *   pgr_backward           <- _C.rasterize_gaussians_backward(...), training only: /root/reference/src/gs/gs_training.py:7,46
 *
 * Conventions
 *   - Every pointer in PgrScene / PgrCamera / PgrOutputs is a DEVICE address of a contiguous
 *     array (fp32 / int32) in the layouts PEGASUS's GaussianModel getters produce
 *     (/root/reference/src/gs/gaussian_model.py:105-128).  The caller (torch) owns all memory.
 *   - The library never allocates or frees device memory and never touches the default stream:
 *     all work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - Re-entrant, no global state.  One call = one stream = one workspace.
 *   - Environment switches for A/B measurements and tests, read per call; results NEVER depend on them:
 *     PGR_BLOCK_CULL=0 (no per-block view culling), PGR_BIN_RECORDS=0 (the scatter walk of the binning evaluates the
 *     tight-list predicate itself instead of reading the count walk's verdicts).
 *   - Return value: 0 = enqueued; negative = PgrStatus.  pgr_status_string() names a code.
 */
#ifndef PEGASUS_RASTER_H
#define PEGASUS_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGR_ABI_VERSION 4
#define PGR_TILE_SIZE 16

typedef enum PgrStatus {
    PGR_OK = 0,
    PGR_ERR_INVALID_ARGUMENT = -1,   /* NULL / inconsistent pointers, bad sizes, bad sh_degree */
    PGR_ERR_WORKSPACE_TOO_SMALL = -2,/* workspace_bytes < pgr_workspace_bytes(...) */
    PGR_ERR_INSTANCE_OVERFLOW = -3,  /* listed instances > max_instances; *num_instances holds the need */
    PGR_ERR_LAUNCH_FAILURE = -4,     /* a HIP call failed; see pgr_last_hip_error */
    PGR_ERR_NO_DEVICE = -5
} PgrStatus;

/* One merged point cloud (environment first, then objects), activated values. */
typedef struct PgrScene {
    int32_t n;                   /* Gaussians */
    const float *means3d;        /* [n,3]  get_xyz */
    const float *opacities;      /* [n]    get_opacity (sigmoid applied) */
    const float *scales;         /* [n,3]  get_scaling (exp applied)      -- or NULL with cov3d_precomp */
    const float *rotations;      /* [n,4]  get_rotation (w,x,y,z), unit   -- or NULL with cov3d_precomp */
    const float *cov3d_precomp;  /* [n,6]  (xx,xy,xz,yy,yz,zz)            -- or NULL */
    const float *shs;            /* [n,sh_stride,3] get_features          -- or NULL with colors_precomp */
    const float *colors_precomp; /* [n,3]                                 -- or NULL */
    int32_t sh_degree;           /* active degree 0..3 */
    int32_t sh_stride;           /* coefficients stored per Gaussian, >= (sh_degree+1)^2 */
    float scale_modifier;
    const int32_t *tie_index;    /* [n] a permutation of 0..n-1, or NULL = the position itself.  The per-tile order is
                                    (depth, index): where two depths are EXACTLY equal the smaller tie_index comes
                                    first.  A scene stored in another order than the caller's (FrameRenderer's Morton
                                    layout) passes the caller's indices here and renders the caller's image bit for bit. */
    const uint32_t *tie_inv;     /* [n] inverse permutation of tie_index (tie_inv[tie_index[i]] = i), or NULL = the library
                                    rebuilds it in its workspace on every call.  A per-SCENE constant: pgr_scene_prepare
                                    computes it once into caller-owned memory. */
    const float *shs_rest;       /* optional: [n,sh_stride-1,3] -- the SH coefficients as PEGASUS's model STORES them, in two
                                    tensors: `shs` is then _features_dc [n,1,3] (coefficient 0 only) and this is
                                    _features_rest (coefficients 1 .. sh_stride-1).  Saves the caller the torch.cat of
                                    get_features (/root/reference/src/gs/gaussian_model.py:118-121: 768 MB moved per
                                    render() of a freshly merged 2 M-Gaussian scene).  Same coefficients, same arithmetic:
                                    results are bit-identical.  pgr_forward without PgrPosedObjects only (with poses, and
                                    in pgr_backward -- whose SH gradient is one [n,sh_stride,3] array --
                                    PGR_ERR_INVALID_ARGUMENT). */
} PgrScene;

/* The depth image's blend rule.  The reference's rasterizer is the absent fork `depth-diff-gaussian-rasterization`
 * (/root/reference/setup.sh:19); the widely used fork of that name writes the un-normalised expected depth, which the
 * in-tree evidence is consistent with (/root/reference/pegasus.py:355 scales it to millimetres as is) -- but the rule
 * itself is unverified (SURVEY.md section 8a "Depth variant"), so it is a switch:
 *   PGR_DEPTH_EXPECTED    depth = sum_i T_i alpha_i z_i                      (default; no background term)
 *   PGR_DEPTH_NORMALIZED  depth = sum_i T_i alpha_i z_i / (1 - T_final)      (sum_i T_i alpha_i = 1 - T_final; 0 where
 *                                                                             nothing was blended) */
typedef enum PgrDepthMode { PGR_DEPTH_EXPECTED = 0, PGR_DEPTH_NORMALIZED = 1 } PgrDepthMode;

/* The fields of GaussianRasterizationSettings that describe one view.  Scalars are host values;
 * the four small tensors stay on the device exactly as PEGASUS's Camera holds them. */
typedef struct PgrCamera {
    int32_t image_width, image_height;
    float tanfovx, tanfovy;
    const float *viewmatrix;     /* device [16], world_view_transform (transposed storage) */
    const float *projmatrix;     /* device [16], full_proj_transform  (transposed storage) */
    const float *campos;         /* device [3] */
    const float *bg;             /* device [3] */
    int32_t depth_mode;          /* PgrDepthMode; applies to depth and sem_depth of this view */
} PgrCamera;

typedef struct PgrOutputs {
    float *color;                /* [3,H,W]  required, except: a layered call writes no image; a RECORDS-ONLY view passes
                                    color = depth = NULL with `record` set and receives the frame record alone (round 6:
                                    a rank of a view-sharded job ships 3.84 MB per 800x800 frame and has no reader for the
                                    25.6 MB of fp32 / mask planes beside it) */
    float *depth;                /* [1,H,W]  required (same exceptions; NULL exactly when color is): sum_i T_i alpha_i z_i, no
                                    bg term; PgrCamera::depth_mode selects the normalised form */
    int32_t *radii;              /* [n]      optional (NULL); a view pgr_backward is to differentiate needs it */
    float *final_T;              /* [H,W]    optional (NULL) */
    uint32_t *n_contrib;         /* [H,W]    optional (NULL) */
    float *sem_color;            /* [3,H,W]  the objects-only semantic render: REQUIRED on every view of a call that
                                    passes a PgrSemantic (PGR_ERR_INVALID_ARGUMENT otherwise), ignored without one.  A
                                    records-only view (color == NULL, record set) may pass NULL when the descriptor carries
                                    mask_colors: the semantic image then exists only as the record's mask planes */
    float *sem_depth;            /* [1,H,W]  optional, only with sem_color */
    uint8_t *sem_masks;          /* [K,H,W]  optional: the K colour-distance masks of the semantic image
                                    (pgr_color_masks of sem_color against PgrSemantic::mask_colors, bit for bit), written by
                                    the compositor's epilogue from the pixel it holds in registers -- needs
                                    PgrSemantic::mask_colors.  In a LAYERED call (PgrForwardCall::layers) the one output:
                                    [n_layers,H,W], plane k = layer k's image against mask_colors[k]. */
    uint8_t *record;             /* optional: this view's FRAME RECORD (PgrRecordLayout below: uint8 rgb | uint16 depth mm |
                                    mask bit planes, pgr_frame_record_layout(width, height, K) bytes), written by the
                                    compositor's epilogue from the pixel it holds in registers -- bit for bit what
                                    pgr_pack_records makes of color / depth / sem_masks, without the pass that re-reads them.
                                    K = the semantic descriptor's k_objects when it carries mask_colors, else 0 (no mask
                                    section).  What leaves the GPU for a finished frame (gather to the root rank, writers). */
} PgrOutputs;

/* Fused semantic pass: PEGASUS renders the objects alone, painted in flat semantic colours, to derive masks
 * (/root/reference/src/gs/render.py:68-97, colours from pegasus.py:230-232).  With this descriptor the batch
 * call also writes that image (outs[v].sem_color) from the SAME per-tile lists -- the objects-only list of a
 * tile is the scene's list minus the environment entries -- instead of a second preprocess/bin/sort/composite. */
typedef struct PgrSemantic {
    const int32_t *object_id;    /* device [n]: 0 = environment, k = object k (1..k_objects) */
    const float *colors;         /* device [k_objects,3]: the rgb each object's Gaussians carry =
                                    max(C0 * RGB2SH(c_k) + 0.5, 0), evaluated in fp32 in that order */
    int32_t n_env;               /* Gaussians [0, n_env) are the environment */
    int32_t k_objects;
    const uint8_t *object_id_u8; /* device [n - n_env]: object_id[n_env + j] as a byte, or NULL = the library packs it in
                                    its workspace on every call (k_objects <= 255).  Per-scene constant: pgr_scene_prepare */
    const float *mask_colors;    /* device [k_objects,3]: the colours the masks are thresholded against (the c_k of
                                    /root/reference/src/gs/render.py:60-63,89-93), or NULL = no sem_masks output */
    float mask_threshold;        /* L2 distance, the reference's 0.1 */
} PgrSemantic;                   /* checked before anything is enqueued: object_id (unless the scene is empty), colors non-NULL,
                                    n_env >= 0, k_objects > 0, outs[v].sem_color non-NULL for every view, mask_colors
                                    non-NULL if any view passes sem_masks */

/* Device pointers to one view's share of a workspace -- its slice and, for num_instances, its two status words in the
 * batch header -- for stage-level parity tests and for backward. */
typedef struct PgrWorkspaceView {
    const float *splats;         /* [n,12] per-Gaussian record: x, y, conic A, B, C, opacity, B/C, B/A, r, g, b, depth
                                    (defined only for Gaussians with a non-empty rectangle) */
    const uint16_t *rects;       /* [n,4] tile rectangle minx,miny,maxx,maxy (max exclusive); zeros = culled.
                                    Written only for views rendered WITH a radii output. */
    const uint32_t *gauss_sorted;/* [num_instances] Gaussian index, tile-major, (depth, index) ascending per tile */
    const uint32_t *ranges;      /* [tiles,2] start,end into gauss_sorted */
    const uint32_t *num_instances; /* [0] listed instances, [1] overflow flag: the words the forward of this view wrote */
} PgrWorkspaceView;

int32_t pgr_abi_version(void);
const char *pgr_version(void);
const char *pgr_status_string(int32_t status);
/* Text of the last HIP error seen by THIS thread inside the library (thread-local, read-only use). */
const char *pgr_last_hip_error(void);

/* Bytes of workspace needed to render one view of `n` Gaussians at width x height with room for
 * `max_instances` (Gaussian,tile) pairs. */
size_t pgr_workspace_bytes(int32_t n, int32_t width, int32_t height, int64_t max_instances);
/* Same for a batch of `n_views` views in flight at once. */
size_t pgr_batch_workspace_bytes(int32_t n, int32_t width, int32_t height, int64_t max_instances_per_view,
                                 int32_t n_views);

/* Pinned host memory an asynchronous pgr_forward call stages its tables in and receives its status words in. */
size_t pgr_host_scratch_bytes(int32_t n_views);

/* Dynamic scenes: per-view rigid poses of the scene's objects, applied INSIDE the preprocess instead of composing a
 * posed copy of the scene per time step (reference: update_object_pose + deepcopy + merge per frame,
 * /root/reference/pegasus.py:254-264,387-390; /root/reference/src/gs/pegasus_setup.py:160-226).  A Gaussian with
 * object_id k > 0 is placed by poses[view][k-1] with the arithmetic of pgr_compose_object (position, orientation);
 * its view-dependent colour is its own SH evaluated in the object's frame (direction R^T d) -- the function the
 * band-rotated coefficients of a composed copy represent.  A batch of time steps then runs like a batch of cameras.
 * Needs scales + rotations (no cov3d_precomp). */
#define PGR_POSE_STRIDE 20
typedef struct PgrPosedObjects {
    const int32_t *object_id;   /* [n] device; 0 = not posed (environment) */
    const float *poses;         /* [n_views, k_objects, PGR_POSE_STRIDE] device:
                                   R[9] row-major, t[3], center[3], q[4] = R as unit quaternion (w,x,y,z), pad */
    int32_t k_objects;
} PgrPosedObjects;

/* Per-SCENE constants the batch calls would otherwise rebuild on every call (round 3: invert_tie_index_kernel and
 * pack_object_ids_kernel, 24 us + 76 MB of traffic per batch of the 2 M-Gaussian scene): the inverse of
 * PgrScene::tie_index and the object ids of the object Gaussians as bytes.  Enqueues the work on `stream`, writes into
 * caller-owned `cache` (device, pgr_scene_cache_bytes(n) bytes) and returns the two device pointers to put into
 * PgrScene::tie_inv / PgrSemantic::object_id_u8 (NULL where the input is absent: scene->tie_index == NULL, semantic ==
 * NULL, or k_objects > 255).  Valid until the scene's tie_index / object ids change. */
size_t pgr_scene_cache_bytes(int32_t n);
int32_t pgr_scene_prepare(const PgrScene *scene, const PgrSemantic *semantic, void *cache, size_t cache_bytes,
                          const uint32_t **tie_inv, const uint8_t **object_id_u8, void *stream);

/* Layered render = silhouette masks (/root/reference/src/gs/render.py:36-65: every object rendered ALONE over an empty
 * environment and thresholded against its semantic colour -- the reference does one deepcopy + merge + render per object
 * and camera).  One pipeline pass renders n_layers images per view: a Gaussian with layer_id k > 0 is composited into
 * image k only (per-(tile, layer) lists: the binning treats the n_layers images as one image of n_layers x grid_y tile
 * rows; projection, lists and blending of a layer are those of rendering its Gaussians alone), and the compositor's
 * epilogue writes outs[v].sem_masks[k-1] = || pixel - mask_colors[k-1] ||_2 <= mask_threshold.  No colour image is
 * written (outs[v].color / depth may be NULL).  layer_id must be non-decreasing along the scene (PEGASUS merges object
 * after object); Gaussians with layer_id 0 are dropped.  Goes with PgrForwardCall::posed or without.
 * EMPTY LAYERS: the plane of a layer no Gaussian carries is all 0, whatever the background -- the reference never renders
 * an object that is not in gs_object_list and leaves its mask column 0 (/root/reference/src/gs/render.py:44-63); an
 * empty scene (n == 0) is the same rule for every layer.  A layer WITH Gaussians of which none reaches a pixel holds the
 * background's verdict || bg - mask_colors[k-1] ||_2 <= mask_threshold there, as a render of that object alone would. */
typedef struct PgrLayers {
    const int32_t *layer_id;     /* device [n] */
    int32_t n_layers;
    const float *mask_colors;    /* device [n_layers,3] */
    float mask_threshold;
} PgrLayers;
size_t pgr_layers_workspace_bytes(int32_t n, int32_t width, int32_t height, int64_t max_instances_per_view,
                                  int32_t n_views, int32_t n_layers);

/* The stages PgrForwardCall::stage_ms times (bench / rocprof only): HIP events on `stream` at the stage boundaries (each
 * stage runs for all views before the next starts), elapsed milliseconds of each stage for the whole batch, in PgrStage
 * order. */
#define PGR_NUM_STAGES 5
typedef enum PgrStage {
    PGR_STAGE_PREPROCESS = 0,  /* camera pack + per-Gaussian projection / EWA / SH */
    PGR_STAGE_BIN_COUNT = 1,   /* per-chunk tile histograms, slice reservation, tile scan */
    PGR_STAGE_BIN_SCATTER = 2, /* (depth, index) pairs into the tiles' slices */
    PGR_STAGE_TILE_SORT = 3,   /* work order + per-tile (depth, index) sort */
    PGR_STAGE_COMPOSITE = 4    /* front-to-back alpha compositing of all views; with a PgrSemantic the same
                                  walk also accumulates the objects-only semantic image */
} PgrStage;

/* THE forward: render `n_views` views of ONE scene (the per-frame loop of /root/reference/pegasus.py:254-325 calls render()
 * once per camera over the same merged cloud; this is that loop as one call, and one view is a batch of one).  `cameras`
 * and `outs` are HOST arrays of n_views entries; all views share the image size.  The batch is what fills an MI355X: the
 * compositing of every (view, tile) list is one launch, ordered longest list first, so no view waits on its own slowest
 * tile.  `workspace`: device, pgr_batch_workspace_bytes (a layered call: pgr_layers_workspace_bytes) for
 * `max_instances_per_view` (Gaussian, tile) pairs per view.
 *
 * SYNCHRONOUS (host_scratch NULL): everything is enqueued on `stream` and the call synchronises it once, at its end, to
 * read the instance counts and overflow flags (the reference synchronises mid-pipeline to read num_rendered, SURVEY.md
 * section 2a), so that an overflow is returned as PGR_ERR_INSTANCE_OVERFLOW instead of as an image.  `num_instances` (host,
 * n_views entries) receives the counts.  With `stage_ms` the call also times its stages (PgrStage above).
 *
 * ASYNCHRONOUS (host_scratch non-NULL): enqueues and returns without synchronising.  `host_scratch` is PINNED host memory
 * of pgr_host_scratch_bytes(n_views) in which the library stages its pointer tables and receives the status words; it must
 * stay untouched until `stream` has passed the call.  After synchronising, pgr_batch_status(host_scratch, n_views,
 * num_instances) returns PGR_OK or PGR_ERR_INSTANCE_OVERFLOW (frames of an overflowed batch are not valid: the rest of the
 * call did nothing; re-run with a larger capacity).  Two batches can run concurrently on two streams with two workspaces.
 * With `status_event` (a hipEvent_t) the status words reach the host EARLY: they are final once the tile scan has run -- a
 * third into a single-view call -- so the scan stores them into `host_scratch` itself (which must therefore be
 * device-accessible at its host address: hipHostMalloc memory, what torch's pin_memory() hands out) and the event is
 * recorded on `stream` right behind it.  After hipEventSynchronize(status_event), pgr_batch_status is valid while scatter,
 * sort and compositor still run: the caller of a single view (PEGASUS's render(), /root/reference/src/gs/render.py:17-24 --
 * the upstream rasterizer blocks on its own instance count in the middle of every call the same way) returns to its host
 * code without leaving the GPU idle; the outputs are complete in STREAM order, as for every asynchronous call.
 *
 * PGR_ERR_INVALID_ARGUMENT before anything is enqueued: call NULL; a synchronous call with posed, layers or status_event;
 * an asynchronous one with num_instances or stage_ms, or with host_scratch_bytes below pgr_host_scratch_bytes(n_views);
 * status_event with layers; layers with semantic; and what the descriptors above say of themselves. */
typedef struct PgrForwardCall {
    const PgrScene *scene;
    int32_t n_views;
    const PgrCamera *cameras;
    const PgrOutputs *outs;
    void *workspace;
    size_t workspace_bytes;
    int64_t max_instances_per_view;
    const PgrSemantic *semantic;         /* optional: the fused objects-only semantic image */
    const PgrPosedObjects *posed;        /* optional, asynchronous only: per-view object poses */
    const PgrLayers *layers;             /* optional, asynchronous only: a layered call */
    void *host_scratch;                  /* NULL = synchronous */
    size_t host_scratch_bytes;
    int64_t *num_instances;              /* optional, synchronous only */
    float *stage_ms;                     /* optional, synchronous only: [PGR_NUM_STAGES] */
    void *status_event;                  /* optional, asynchronous only, not with layers */
} PgrForwardCall;
int32_t pgr_forward(const PgrForwardCall *call, void *stream);
int32_t pgr_batch_status(const void *host_scratch, int32_t n_views, int64_t *num_instances);

/* Conservative block visibility (pegasus_amd/csrc/blockcull.hip.h): bit (v % 32) of
 * vis_words[g * ceil(n_views / 32) + v / 32] is CLEAR only if none of the Gaussians [64 g, 64 g + 64) can get a
 * non-zero radius in view v (all behind the near plane, or all tile rectangles empty) -- the test the batch entry
 * points run internally to skip whole waves in the per-Gaussian stages (switch: environment PGR_BLOCK_CULL=0; outputs
 * never depend on it).  A block-granular, many-view relative of markVisible; exposed for the parity tests.
 * vis_words: device [ceil(n / 64) * ceil(n_views / 32)]. */
size_t pgr_block_visibility_workspace_bytes(int32_t n, int32_t n_views);
int32_t pgr_block_visibility(const PgrScene *scene, int32_t n_views, const PgrCamera *cameras, void *workspace,
                             size_t workspace_bytes, uint32_t *vis_words, void *stream);

/* Fill `view` with device pointers into view `view_index` of a workspace laid out for
 * (n,width,height,max_instances,n_views). */
int32_t pgr_workspace_view(void *workspace, size_t workspace_bytes, int32_t n, int32_t width, int32_t height,
                           int64_t max_instances, int32_t n_views, int32_t view_index, PgrWorkspaceView *view);

/* Where a batch call of that shape (not a layered one) leaves its block-visibility words in its workspace: *vis_words is
 * the device pointer of [ceil(n / 64) * *words_per_block] words in pgr_block_visibility's layout, or NULL when such a call
 * runs no block test (environment PGR_BLOCK_CULL=0, one- and two-view calls, a small scene whose views are spread over the
 * grid) -- decided by the function the forward call itself asks.  Host only: launches nothing, reads no device memory. */
int32_t pgr_workspace_block_visibility(void *workspace, size_t workspace_bytes, int32_t n, int32_t width,
                                       int32_t height, int64_t max_instances, int32_t n_views,
                                       const uint32_t **vis_words, int32_t *words_per_block);

/* Rigid pose of one object, host struct (copied into the launch).  R row-major, q = R as a unit quaternion
 * (w,x,y,z), D1/D2/D3 = real-SH band rotation matrices (row-major, c' = D c) for the rasterizer's basis. */
typedef struct PgrObjectPose {
    float R[9];
    float t[3];
    float center[3];
    float q[4];
    float D1[9], D2[25], D3[49];
} PgrObjectPose;

/* Scene composition (replaces GaussianModel.apply_transformation + merge_gaussians,
 * /root/reference/src/gs/gaussian_model.py:482-546,584-591, called per frame at pegasus.py:255-264,387-390):
 *   out_xyz[i]  = R (xyz[i] - center) + center + t
 *   out_rot[i]  = q (x) normalise(rot[i])                    (skipped when rot or out_rot is NULL)
 *   out_rest[i] = band-wise D_l * f_rest[i]                  (n_rest in {0,3,8,15} coefficients of 3 floats)
 * Input rows of f_rest are in_rest_stride floats apart, output rows out_rest_stride floats apart, so the output can
 * point INTO a merged [N,16,3] feature tensor (base + 3 floats, stride 48).  In-place operation is allowed. */
int32_t pgr_compose_object(int32_t n, const float *xyz, const float *rot, const float *f_rest, int32_t n_rest,
                           int32_t in_rest_stride, const PgrObjectPose *pose, float *out_xyz, float *out_rot,
                           float *out_rest, int32_t out_rest_stride, void *stream);

/* The pose calls of a whole frame (round 6).  PEGASUS re-poses every object between two frames of a dynamic sequence with
 * three calls per object -- apply_transformation_on_xyz(T), apply_rotation_on_splats(R), apply_rotation_on_sh(R):
 * /root/reference/src/gs/pegasus_setup.py:195-208 -> /root/reference/src/gs/gaussian_model.py:482-546 -- each handed a
 * rotation / translation that already lives on the device.  One JOB per (object, array); R and t stay DEVICE pointers (no
 * host round trip, unlike PgrObjectPose), the cloud's mean, the quaternion of R and the SH band matrices are derived on the
 * device:
 *   PGR_POSE_XYZ   dst[i] = R (src[i] - c) + c + t,  c = the mean of src (about_origin = 0) or 0      src, dst [n,3]
 *   PGR_POSE_ROT   dst[i] = quat(R) (x) normalise(src[i])                              (w,x,y,z)       src, dst [n,4]
 *   PGR_POSE_SH    dst[i] = band-wise D_l(R) src[i],  D_l = pinv(B_l) B_l(R^T d_k)                     src, dst [n,n_rest,3]
 * R = NULL: identity (PGR_POSE_XYZ then writes src + t in float32, a bit-for-bit copy without t; an identity MATRIX handed over as
 * R is multiplied like any other: 0 * Inf is NaN there, here and in pgr_compose_object); t = NULL: zero.  R and t may point INTO a 4x4 transform (strides below): PEGASUS builds T on the device and
 * hands its corner and last column over.  src == dst is allowed.  Jobs of one call must not depend on each other.
 * sh_dirs [61,3] / sh_pinv [15,61]: device fp64 tables of the SH sample directions and the three bands' pseudo-inverses
 * (pegasus_amd/sh_rotation.py builds them for the rasterizer's basis; needed only if a job is PGR_POSE_SH).
 * workspace: pgr_pose_objects_workspace_bytes(n_jobs) bytes of device memory. */
typedef enum PgrPoseKind { PGR_POSE_XYZ = 0, PGR_POSE_ROT = 1, PGR_POSE_SH = 2 } PgrPoseKind;
typedef struct PgrPoseJob {
    const float *src;
    float *dst;
    const float *R;              /* device, row-major: R[r][c] at R[r * R_row_stride + c] */
    const float *t;              /* device: t[c] at t[c * t_stride] */
    int32_t n;
    int32_t kind;                /* PgrPoseKind */
    int32_t n_rest;              /* PGR_POSE_SH: coefficients per Gaussian, 3, 8 or 15 */
    int32_t about_origin;        /* PGR_POSE_XYZ */
    int32_t R_row_stride;        /* floats between the rows of R: 3 = a contiguous 3x3, 4 = the corner of a 4x4 */
    int32_t t_stride;            /* floats between the components of t: 1 = contiguous, 4 = the last column of a 4x4 */
} PgrPoseJob;
size_t pgr_pose_objects_workspace_bytes(int32_t n_jobs);
int32_t pgr_pose_objects(int32_t n_jobs, const PgrPoseJob *jobs, const double *sh_dirs, const double *sh_pinv,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Measurement aid (bench.py's roofline.issue_model; replaces nothing of the reference): ONE wave that reads its two clocks
 * around a sleep loop of spin_us microseconds (0: no loop, a time stamp) -- ticks[0] = shader cycles (s_memtime), ticks[1] =
 * 100 MHz ticks (s_memrealtime), ticks[2] / ticks[3] = the 100 MHz counter at its start / end -- so ticks[0] / ticks[1] x
 * 100 MHz is the shader clock under whatever runs beside it on other streams, and stamps taken on the measured stream show
 * whether the two really overlapped.  `ticks`: device uint64[4]. */
int32_t pgr_clock_probe(uint64_t *ticks, uint32_t spin_us, void *stream);

/* Mean squared distance to the 3 nearest neighbours of every point (replaces simple_knn._C.distCUDA2 of the reference's
 * second absent submodule: GaussianModel.create_from_pcd, /root/reference/src/gs/gaussian_model.py:25,147).  Exact
 * 3-NN over a device-built uniform grid; with fewer than 4 points the missing neighbours count as FLT_MAX, as upstream.
 * `xyz` [n,3] and `out` [n] are device pointers; workspace of pgr_knn_workspace_bytes(n) bytes. */
size_t pgr_knn_workspace_bytes(int32_t n);
int32_t pgr_knn_mean_dist2(int32_t n, const float *xyz, float *out, void *workspace, size_t workspace_bytes,
                           void *stream);

/* How many points lie within `radius` of every point, the point itself included (open3d's remove_radius_outlier, which
 * keeps point i iff counts[i] > nb_points: the reference's load_ply(clean_pcd=True) and denoise_point_cloud,
 * /root/reference/src/gs/gaussian_model.py:238-247,633-651).  Point j counts for point i iff
 * ((dx*dx) + dy*dy) + dz*dz < radius*radius, evaluated in float64 with every operation rounded on its own (the float32
 * coordinates widened exactly, radius*radius rounded once) and compared STRICTLY.  Counting stops at `cap` hits:
 * counts[i] = min(count_i, cap); cap = n gives exact counts, cap = nb_points + 1 is all the filter needs.  A sparse grid with
 * cells of about `radius` is built on the device, in storage proportional to n wherever the points lie.  Results are exact
 * integers, identical from run to run.  The caller's contract, which the entry cannot check: every coordinate is finite and
 * |x| / radius < 2^30.  `xyz` [n,3] and `counts` [n] are device pointers; workspace (16-byte aligned) of
 * pgr_radius_count_workspace_bytes(n) bytes (0 for n < 0).  n == 0 returns PGR_OK without a launch. */
size_t pgr_radius_count_workspace_bytes(int32_t n);
int32_t pgr_radius_count(int32_t n, const float *xyz, double radius, int32_t cap, int32_t *counts, void *workspace,
                         size_t workspace_bytes, void *stream);

/* Rigid registration of a source cloud to a target cloud (open3d's evaluate_registration / registration_icp, which the
 * reference's marker alignment refines with: /root/reference/submodules/aruco-estimator/aruco_estimator/utils.py:82-98;
 * pegasus_amd/registration.py drives these entries; DESIGN.md section 17 holds the rules).  Points are float32 [n,3] device
 * arrays.  A `transformation` is a HOST pointer to a row-major float64 4x4 whose upper 3x4 is read and handed to the kernel
 * by value; a value that is not finite is PGR_ERR_INVALID_ARGUMENT.  The posed source point is s' = R s + t in float64, each
 * coordinate ((r0*x + r1*y) + r2*z) + t with every operation rounded on its own.  The caller's contract, which the entries
 * cannot check: every target coordinate and every s' is finite with |x| / max_distance < 2^30.  Every argument check comes
 * before any launch; a count of 0 returns PGR_OK without a launch; workspaces are 16-byte aligned.
 *
 * pgr_nn_grid_build files the target into pgr_radius_count's sparse grid with cells of max_distance * 1.0001, in a
 * caller-owned workspace of pgr_nn_grid_build_workspace_bytes(n_target) bytes (0 for a negative count) that later calls read
 * with the same n_target and max_distance, for as long as the target stays where it is.
 *
 * pgr_nn_correspond: for every source point the target of smallest d2 = ((dx*dx) + dy*dy) + dz*dz (dx = q.x - s'.x, float64,
 * every operation rounded on its own), among equal d2 the lowest target index, accepted iff d2 < max_distance * max_distance
 * (rounded once, compared STRICTLY): `index` int32 [n_source] (-1: none) and `d2` float64 [n_source] (0 where none), exact and
 * identical from run to run.  `order` (device int32 [n_source], may be NULL = row order) is a permutation of the source rows:
 * lane i works on point order[i]; it changes no result.  n_target == 0: every index is -1 and `grid` is not read.
 *
 * pgr_nn_source_order writes such a permutation: the source rows in the order of the grid cells their s' fall into (a grid of
 * the source's own, in the workspace); pgr_nn_source_order_workspace_bytes(n_source) bytes.
 *
 * pgr_icp_sums: one pass over the source given `index` and `d2` as pgr_nn_correspond wrote them (an index outside
 * [0, n_target) counts as none), reduced in a fixed order without floating-point atomics, so equal inputs give equal bytes.
 * `sums` is device float64 [PGR_ICP_SUMS].  With q the correspondent, n its row of `target_normals` (device float64
 * [n_target,3]; NULL: the first 27 sums are 0), r = (s' - q) . n and J = [s' x n, n]:
 *   [0,21) the upper triangle of sum J^T J, row by row    [21,27) sum J^T r    [27] the count    [28] sum d2
 *   [29,32) sum s'    [32,35) sum q    [35,44) sum s' q^T, row by row    [44] sum |s'|^2    [45,48) 0
 * (point-to-plane reads [0,32), point-to-point [16,48)).  Workspace: pgr_icp_sums_workspace_bytes(n_source) bytes.
 *
 * pgr_radius_normals (open3d's estimate_normals(KDTreeSearchParamRadius(radius)): /root/reference/src/gs/ao_test.py:21): for
 * every point the float64 covariance of the points within `radius` of it -- pgr_radius_count's strict test, the point itself
 * included -- and of it the unit eigenvector of the smallest eigenvalue, signed so that its component of largest magnitude is
 * positive; (0,0,1) with fewer than 3 neighbours.  `normals` float64 [n,3], `counts` int32 [n] (exact).  The neighbour sums
 * run in grid order, so the normals may differ in their last bits from run to run; the counts may not.  Workspace:
 * pgr_radius_normals_workspace_bytes(n) bytes; the contract on the coordinates is pgr_radius_count's. */
#define PGR_ICP_SUMS 48
size_t pgr_nn_grid_build_workspace_bytes(int32_t n_target);
int32_t pgr_nn_grid_build(int32_t n_target, const float *target, double max_distance, void *workspace, size_t workspace_bytes,
                          void *stream);
size_t pgr_nn_source_order_workspace_bytes(int32_t n_source);
int32_t pgr_nn_source_order(int32_t n_source, const float *source, const double *transformation, double max_distance,
                            int32_t *order, void *workspace, size_t workspace_bytes, void *stream);
int32_t pgr_nn_correspond(int32_t n_source, const float *source, const int32_t *order, const double *transformation,
                          int32_t n_target, double max_distance, const void *grid, size_t grid_bytes, int32_t *index,
                          double *d2, void *stream);
size_t pgr_icp_sums_workspace_bytes(int32_t n_source);
int32_t pgr_icp_sums(int32_t n_source, const float *source, const double *transformation, const int32_t *index,
                     const double *d2, int32_t n_target, const float *target, const double *target_normals, double *sums,
                     void *workspace, size_t workspace_bytes, void *stream);
size_t pgr_radius_normals_workspace_bytes(int32_t n);
int32_t pgr_radius_normals(int32_t n, const float *xyz, double radius, double *normals, int32_t *counts, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Object meshes from a trained model's rendered views (pegasus_amd/mesh.py; replaces the open3d alpha shape of the
 * reference's reconstruction step).  A regular grid: point (i,j,k) sits at origin + voxel*(i,j,k); a field over it is
 * float32 [nz,ny,nx], x fastest.  Every axis holds 2 .. 1024 points.  Results are identical from run to run. */
typedef struct PgrGrid {
    int32_t nx, ny, nz;
    float origin[3];
    float voxel;
} PgrGrid;

/* TSDF fusion with space carving.  `depth` (PGR_DEPTH_NORMALIZED) and `final_T` are device [n_views,H,W], all views of
 * one size (cameras[v].image_width/height), n_views 1..256; each camera's viewmatrix and tanfovx/y place its view (the
 * other PgrCamera fields are not read).  Per grid point p and view v in order, in float32:
 *   (x,y,z) = viewmatrix_v . p; skipped when z <= 0.2 (the renderer's near cull)
 *   pixel = floor((x/z) * W/(2 tanfovx) + (W-1)/2 + 0.5), likewise y; skipped outside the image
 *   1 - final_T < alpha_min: carved (sdf = +1); else d = depth - z, skipped when d < -truncation,
 *   else s += min(d, truncation) / truncation, w += 1
 * sdf = carved ? +1 : (w == 0 ? -1 : s / w); the outermost layer of points is +1, so the surface closes.  Positive is
 * outside.  `sdf` is device [nz,ny,nx].  A NaN depth counts like +inf, as an observation at the full truncation (NaN <
 * -truncation is false and min is fminf); the depth of a carving pixel is never read. */
int32_t pgr_tsdf_integrate(const PgrGrid *grid, int32_t n_views, const PgrCamera *cameras, const float *depth,
                           const float *final_T, float truncation, float alpha_min, float *sdf, void *stream);

/* The environment as a distance field (pegasus_amd/environment.py; the rule stands at the top of
 * pegasus_amd/csrc/envfield.hip.h and in DESIGN.md section 25): a signed distance field over the whole grid from a carved
 * volume, which is +-1 a few voxels from the surface and useless for sphere tracing.  `tsdf`, `sdf` and `dist2` (may be NULL)
 * are device [nz,ny,nx]; `sdf` must not be `tsdf`.  inside(p) <=> tsdf(p) < 0 (a NaN is outside).  dist2(p) is the exact squared
 * distance, in voxels, to the nearest grid point of the other sign, -1 where there is none.  A point with a 6-neighbour of the
 * other sign (taken in the order -x, +x, -y, +y, -z, +z) is a band point: beta = min a / (a + b), a = |tsdf(p)|, b = |tsdf(n)|
 * (1 for a value that is not finite), where pgr_march_emit puts its vertex on that edge.  sdf = s voxel beta for a band point,
 * s voxel (sqrtf((float)dist2) - 0.5f) for other points, s voxel (float)(nx + ny + nz) without a point of the other sign; s = -1
 * inside, +1 outside.  float32, every operation rounded on its own; integer minima only: two runs give equal bytes.  The field
 * differs from the distance to the surface by less than a voxel and is not 1-Lipschitz.  Workspace:
 * pgr_sdf_from_tsdf_workspace_bytes(nx, ny, nz) device bytes (0 for a bad grid; host-only), 16-byte aligned.  Invalid
 * (PGR_ERR_INVALID_ARGUMENT, before any launch): a bad grid, a NULL tsdf, sdf or workspace, sdf == tsdf, a workspace that is too
 * small or not aligned. */
size_t pgr_sdf_from_tsdf_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int32_t pgr_sdf_from_tsdf(const PgrGrid *grid, const float *tsdf, float *sdf, int32_t *dist2, void *workspace,
                          size_t workspace_bytes, void *stream);

/* Marching tetrahedra over `sdf` (inside: sdf < 0).  Every cell splits into the 6 tetrahedra around its
 * (0,0,0)-(1,1,1) diagonal; the mesh is closed and manifold, its triangles face positive sdf.  Each grid point owns the
 * edges +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z (in that order) and emits one vertex per crossed edge, at
 * pa + t (pb - pa), t = fa / (fa - fb), a = the owner.  Vertices come in (point, edge) order, faces in (cell,
 * tetrahedron, triangle) order.  Workspace: pgr_march_workspace_bytes(nx, ny, nz) device bytes (0 for a bad grid),
 * host-only.
 * pgr_march_count writes the vertex and face totals to device int64 counts[2]; the caller reads them, allocates
 * vertices float32 [V,3] and faces int32 [F,3] (V < 2^31), and calls pgr_march_emit with the same grid, sdf and
 * workspace, which it reads only. */
size_t pgr_march_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int32_t pgr_march_count(const PgrGrid *grid, const float *sdf, void *workspace, size_t workspace_bytes, int64_t *counts,
                        void *stream);
int32_t pgr_march_emit(const PgrGrid *grid, const float *sdf, const void *workspace, size_t workspace_bytes,
                       float *vertices, int32_t *faces, void *stream);

/* Depth images of triangle meshes at given poses: the depth renderer of the BOP toolkit (its renderer.render_object(...)
 * ['depth']), for ground-truth masks, scene_gt_info and VSD (pegasus_amd/mesh_render.py).  One call renders n_jobs jobs.  A
 * job is one mesh at one pose into one canvas: the mesh is a range of the shared device arrays `vertices` (float32
 * [n_vertices,3]) and `faces` (int32 [n_faces,3], indices relative to the mesh's vertex_first); R (row-major 3x3) and t take a
 * model point to the camera in the model's units; fx, fy, cx, cy project it; `slot` names the canvas.  All canvases are
 * width x height, each 1..8192; `depth` is device float32 [n_slots,height,width] and receives the camera z of the nearest
 * surface, 0 where nothing is hit.  Jobs that share a slot render into the same canvas.  The exact rules (float32 operation
 * order, the sample point (i + 0.5, j + 0.5), the 1/256-pixel snap, int64 edge functions with a top-left fill rule, no
 * back-face culling, perspective-correct depth, integer atomic min) are pinned at the top of
 * pegasus_amd/csrc/meshraster.hip.h; two runs give equal bytes.  near > 0: faces wholly nearer are dropped; faces that straddle
 * it are dropped whole and counted in the device int32 *straddle_count (there is no clipping).
 * `jobs` is a host array.  Workspace: pgr_mesh_depth_workspace_bytes(n_jobs, jobs) device bytes; host-only, 0 for bad
 * arguments (n_jobs <= 0, NULL jobs, a negative range, more than 2^22 faces in one job). */
typedef struct PgrMeshJob {
    int32_t vertex_first, vertex_count;
    int32_t face_first, face_count;
    float R[9];
    float t[3];
    float fx, fy, cx, cy;
    int32_t slot;
} PgrMeshJob;
size_t pgr_mesh_depth_workspace_bytes(int32_t n_jobs, const PgrMeshJob *jobs);
int32_t pgr_mesh_depth(const float *vertices, int64_t n_vertices, const int32_t *faces, int64_t n_faces, int32_t n_jobs,
                       const PgrMeshJob *jobs, int32_t width, int32_t height, float near_z, float *depth, int32_t n_slots,
                       int32_t *straddle_count, void *workspace, size_t workspace_bytes, void *stream);

/* Shaded object meshes: the toolkit's renderer.render_object(...)['rgb'] and the dense maps only a mesh gives (model
 * coordinates, face ids, normals), in two passes (pegasus_amd/mesh_render.py render / Renderer / vis_object_poses).
 *
 * pgr_mesh_visibility is pgr_mesh_depth with a 64-bit canvas element: same jobs, same rules, same workspace layout, but
 * `keys` (device uint64 [n_slots,height,width], 8-byte aligned) receives per pixel
 *     key = (uint64)float_bits(z) << 32 | (uint32)(job_index_in_call << 22 | face_index_in_job)
 * of the nearest surface, combined by one 64-bit integer atomic min: on equal depth bits the lower job index wins, then the
 * lower face index; 0 where nothing is hit.  The high word equals what pgr_mesh_depth writes for the same call, bit for bit;
 * two runs give equal bytes.  At most 2^22 faces per job and PGR_MESH_VISIBILITY_MAX_JOBS jobs per call: beyond these the
 * workspace functions return 0 and the entries PGR_ERR_INVALID_ARGUMENT (callers chunk).
 *
 * pgr_mesh_shade resolves `keys` of a pgr_mesh_visibility call with the same vertices, faces, jobs, size and near_z: one
 * lane per pixel redoes the winning face's setup and writes every output of PgrMeshShade whose pointer is non-NULL.  The
 * rule, all float32 without contraction, correctly rounded division and square root (pinned above mesh_shade_kernel in
 * pegasus_amd/csrc/meshraster.hip.h and restated in tests/mesh_shade_reference.py, which the outputs equal bit for bit):
 *   weights   la = (float)E_bc w_a, lb = (float)E_ca w_b, lc = (float)E_ab w_c, den = (la + lb) + lc; an attribute A is
 *             ((la A_a + lb A_b) + lc A_c) / den, its values swapped with b and c when the face was flipped
 *   depth     the key's high word, 0 where empty;   face_id, job_id: -1 where empty
 *   xyz       the attribute rule on the model vertices, 0 where empty;   P = R xyz + t,   L = (light - P) / |light - P|
 *   normal    camera frame, unit, 0 where empty.  normals == NULL (flat): cross(P_b - P_a, P_c - P_a) normalised, negated when
 *             dot(n, P) > 0.  Else (smooth): the attribute rule on `normals` [n_vertices,3], rotated by R, normalised.  A zero
 *             or non-finite length gives normal 0 and diffuse 0
 *   rgb       min(ambient + max(dot(L, n), 0), 1) * colour; colour is the attribute rule on `colors` [n_vertices,3] in [0,1],
 *             or, when colors == NULL, row k of the HOST array surf_colors [n_jobs,3] (NULL: 0.5 grey); empty pixels get bg
 * A key that names no face of the call is treated as empty.  Workspace (the device-side job table):
 * pgr_mesh_shade_workspace_bytes(n_jobs, jobs), host-only, 0 for bad arguments.  Neither entry allocates or synchronises. */
#define PGR_MESH_VISIBILITY_MAX_JOBS 1024
typedef struct PgrMeshShade {
    const float *normals;      /* device float32 [n_vertices,3] or NULL: flat shading */
    const float *colors;       /* device float32 [n_vertices,3] or NULL: surf_colors */
    const float *surf_colors;  /* HOST float32 [n_jobs,3] or NULL: 0.5 */
    float light[3];            /* camera frame; the toolkit's default is the camera centre (0,0,0) */
    float ambient;             /* the toolkit's default is 0.5 */
    float bg[3];
    float *depth;              /* outputs, device, each may be NULL: float32 [n_slots,height,width] */
    int32_t *face_id;          /* int32 [n_slots,height,width] */
    int32_t *job_id;           /* int32 [n_slots,height,width] */
    float *xyz;                /* float32 [n_slots,height,width,3] */
    float *normal;             /* float32 [n_slots,height,width,3] */
    float *rgb;                /* float32 [n_slots,height,width,3] */
} PgrMeshShade;
size_t pgr_mesh_visibility_workspace_bytes(int32_t n_jobs, const PgrMeshJob *jobs);
int32_t pgr_mesh_visibility(const float *vertices, int64_t n_vertices, const int32_t *faces, int64_t n_faces, int32_t n_jobs,
                            const PgrMeshJob *jobs, int32_t width, int32_t height, float near_z, uint64_t *keys,
                            int32_t n_slots, int32_t *straddle_count, void *workspace, size_t workspace_bytes, void *stream);
size_t pgr_mesh_shade_workspace_bytes(int32_t n_jobs, const PgrMeshJob *jobs);
int32_t pgr_mesh_shade(const float *vertices, int64_t n_vertices, const int32_t *faces, int64_t n_faces, int32_t n_jobs,
                       const PgrMeshJob *jobs, int32_t width, int32_t height, float near_z, const uint64_t *keys,
                       int32_t n_slots, const PgrMeshShade *shade, void *workspace, size_t workspace_bytes, void *stream);

/* Textured object models (BOP's obj_NNNNNN.ply with texture coordinates and a PNG beside it; the toolkit's renderers draw them
 * with texture2D(u_texture, v_texcoord)).  pgr_mesh_shade_textured takes every argument of pgr_mesh_shade, resolves the same
 * `keys`, and reads the colour of a textured job from its texture.  Rule (pinned above mesh_shade_kernel in
 * pegasus_amd/csrc/meshraster.hip.h, restated in tests/mesh_texture_reference.py, which the outputs equal bit for bit; float32,
 * no contraction, correctly rounded division):
 *   uv        the attribute rule of pgr_mesh_shade on corner_uv[face][a, b, c] (b's and c's values swapped when the face was
 *             flipped): perspective-correct.  The optional output `uv` receives it for every covered pixel, 0 where empty
 *   texture   width x height texels of 3 bytes (RGB), rows tightly packed, at `offset` bytes into `texels`; stored row 0 is the
 *             image's top row and v = 0 is its BOTTOM row (stored row = height - 1 - j); clamp to edge:
 *             clamp(x, n) = x >= 0 ? (x < n ? (int)x : n - 1) : 0, so a NaN gives index 0
 *   nearest   i = clamp(floorf(u * width), width), j = clamp(floorf(v * height), height), colour = (float)texel / 255.0f
 *   bilinear  x = u * width - 0.5f, x0 = floorf(x), fx = x - x0 (0 when that is a NaN), i0 = clamp(x0), i1 = clamp(x0 + 1); y
 *             alike; top = (1 - fx) c00 + fx c10, bot = (1 - fx) c01 + fx c11, colour = (1 - fy) top + fy bot
 *   rgb       light_w * colour, light_w as in pgr_mesh_shade.  A job whose job_texture is -1 is untextured: it follows
 *             pgr_mesh_shade's colour rule, and every output of it equals pgr_mesh_shade's bit for bit
 * No alignment is asked of `texels` or of an offset.  Workspace (the job table and one texture row per job):
 * pgr_mesh_shade_textured_workspace_bytes(n_jobs, jobs), host-only, 0 for bad arguments; 8-byte aligned.  Invalid
 * (PGR_ERR_INVALID_ARGUMENT, before any launch): whatever pgr_mesh_shade refuses, a NULL `textures`, n_textures < 0, a NULL
 * table with n_textures > 0, a NULL job_texture, a job_texture outside [-1, n_textures), a texture side outside 1..8192, an
 * offset plus 3 width height beyond texel_bytes, an unknown filter, and a NULL corner_uv or texels when a job is textured. */
#define PGR_TEXTURE_NEAREST 0
#define PGR_TEXTURE_BILINEAR 1
typedef struct PgrMeshTexture {
    int64_t offset;            /* bytes from `texels` to the texture's top-left texel */
    int32_t width, height;     /* texels, each 1..8192 */
} PgrMeshTexture;
typedef struct PgrMeshTextures {
    const float *corner_uv;          /* device float32 [n_faces,3,2]: (u, v) per face corner in the order of `faces`; NULL: no uv */
    const uint8_t *texels;           /* device uint8: every texture, RGB */
    int64_t texel_bytes;
    int32_t n_textures;
    const PgrMeshTexture *textures;  /* HOST [n_textures] */
    const int32_t *job_texture;      /* HOST int32 [n_jobs]: a texture index, or -1 for an untextured job */
    int32_t filter;                  /* PGR_TEXTURE_NEAREST or PGR_TEXTURE_BILINEAR */
    float *uv;                       /* output, device float32 [n_slots,height,width,2], may be NULL */
} PgrMeshTextures;
size_t pgr_mesh_shade_textured_workspace_bytes(int32_t n_jobs, const PgrMeshJob *jobs);
int32_t pgr_mesh_shade_textured(const float *vertices, int64_t n_vertices, const int32_t *faces, int64_t n_faces, int32_t n_jobs,
                                const PgrMeshJob *jobs, int32_t width, int32_t height, float near_z, const uint64_t *keys,
                                int32_t n_slots, const PgrMeshShade *shade, const PgrMeshTextures *textures, void *workspace,
                                size_t workspace_bytes, void *stream);

/* BOP ground truth of n_jobs (object, image) pairs from depth canvases, the sequence of the toolkit's
 * scripts/calc_gt_info.py:117-177.  Job k reads canvas `slot` of `canvases` [n_slots,canvas_height,canvas_width] (as
 * pgr_mesh_depth leaves it) and image `frame` of `scene_depth` [n_frames,height,width] (same unit, 0 = missing); the image
 * window sits at (margin_x, margin_y) inside the canvas (the toolkit renders a 3x canvas: margins = the image size, cx + margin_x,
 * cy + margin_y).  fx, fy, cx, cy are the image's own K in float64: the distance images are computed in float64 as
 * misc.depth_im_to_dist_im_fast does, rounded to float32, compared in float32:
 *   visib = (dist_model - dist_test <= delta or dist_test == 0) and dist_model > 0        (visibility.py, mode bop19)
 * Outputs: `mask` and `mask_visib` uint8 [n_jobs,height,width] (0/1), and `stats` int32 [n_jobs,11]: px_count_all (whole
 * canvas), px_count_valid, px_count_visib, then min x, min y, max x, max y of the silhouette over the canvas and of the visible
 * mask, in image coordinates (INT32_MAX / INT32_MIN when empty).
 * The two shapes at which the launch changes path (tests/gt_info_cases.py is built around them): jobs go to the device
 * PGR_GT_INFO_JOBS_PER_LAUNCH at a time, and a canvas of more than PGR_GT_INFO_BLOCKS_X * 256 pixels is walked by a
 * grid-stride loop. */
#define PGR_GT_INFO_JOBS_PER_LAUNCH 64  /* jobs per kernel launch (one job table per launch) */
#define PGR_GT_INFO_BLOCKS_X 512        /* workgroups of 256 pixels per job, at most */
typedef struct PgrGtInfoJob {
    int32_t slot, frame;
    double fx, fy, cx, cy;
} PgrGtInfoJob;
int32_t pgr_bop_gt_info(const float *canvases, int32_t n_slots, int32_t canvas_width, int32_t canvas_height, int32_t margin_x,
                        int32_t margin_y, const float *scene_depth, int32_t n_frames, int32_t width, int32_t height,
                        int32_t n_jobs, const PgrGtInfoJob *jobs, float delta, uint8_t *mask, uint8_t *mask_visib,
                        int32_t *stats, void *stream);

/* The BOP pose errors of n_jobs (estimate, ground truth) pairs: the toolkit's pose_error.mssd, mspd, add, proj, re and te
 * (bop_toolkit_lib/pose_error.py) in one call.  A job names its object's model points as a range of the shared device array
 * `vertices` (float32 [n_vertices,3], what mesh_render.MeshSet uploads) and the object's symmetry transforms as a range of
 * the device array `syms` (float64 [n_syms,12]: R row-major, then t; what misc.get_symmetry_transformations returns, the
 * identity first), the two poses in float64 and the intrinsics (no skew).  `errors` is device float32 [n_jobs,6]: mssd, mspd,
 * add, proj, re (degrees), te; `re_te` (device float64 [n_jobs,2], may be NULL) receives re and te unrounded.  Ground truth
 * and symmetry are composed in float64 on the device and rounded to float32 once, the per-vertex arithmetic is float32; the
 * exact rules are pinned at the top of pegasus_amd/csrc/poseerr.hip.h.  est == gt gives mssd = mspd = add = proj = 0 exactly;
 * two runs give equal bytes (integer atomic min, fixed-order sums).  `jobs` is a host array.  PGR_ERR_INVALID_ARGUMENT before
 * anything is enqueued: a NULL array with n_jobs > 0, a vertex or symmetry range that leaves its array, vertex_count <= 0,
 * sym_count <= 0.  n_jobs == 0: PGR_OK, no launch.  PGR_POSE_SYM_CHUNK symmetries of a job share one workgroup. */
#define PGR_POSE_ERRORS 6
#define PGR_POSE_SYM_CHUNK 4
typedef struct PgrPoseErrorJob {
    int32_t vertex_first, vertex_count;
    int32_t sym_first, sym_count;
    double R_est[9], t_est[3];   /* model to camera, row-major */
    double R_gt[9], t_gt[3];
    double fx, fy, cx, cy;       /* rounded to float32 for the projection */
} PgrPoseErrorJob;
int32_t pgr_pose_errors(const float *vertices, int64_t n_vertices, const double *syms, int64_t n_syms, int32_t n_jobs,
                        const PgrPoseErrorJob *jobs, float *errors, double *re_te, void *stream);

/* ADI (ADD-S) of n_jobs pairs: the toolkit's pose_error.adi, the mean over the ground-truth-posed model points of the
 * distance to the nearest estimate-posed model point.  Exact brute-force search in float32 in the model's frame (only the
 * queries are transformed, by R_est^T R_gt and R_est^T (t_gt - t_est) composed in float64 on the host and rounded once; rules
 * in pegasus_amd/csrc/poseerr.hip.h).  `adi` is device float32 [n_jobs].  est == gt gives 0 exactly; two runs give equal
 * bytes.  The jobs' symmetry ranges and intrinsics are not read.  Workspace: pgr_pose_adi_workspace_bytes(n_jobs, jobs)
 * device bytes (host-only; 0 for n_jobs <= 0, NULL jobs or a vertex_count <= 0).  Argument checks as pgr_pose_errors makes
 * them for the vertices; PGR_ERR_WORKSPACE_TOO_SMALL for a workspace below the query. */
size_t pgr_pose_adi_workspace_bytes(int32_t n_jobs, const PgrPoseErrorJob *jobs);
int32_t pgr_pose_adi(const float *vertices, int64_t n_vertices, int32_t n_jobs, const PgrPoseErrorJob *jobs, float *adi,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Minimal oriented bounding boxes by open3d's rule (OrientedBoundingBox::CreateFromPointsMinimal: one candidate box per
 * triangle, normally the convex hull's) for n_jobs jobs in one call (pegasus_amd/obb.py; rules in
 * pegasus_amd/csrc/obb.hip.h and DESIGN.md section 16).  A job is a range of the device array `points` (float32
 * [n_points,3]) and a range of the device array `triangles` (int32 [n_triangles,3], indices relative to the job's
 * point_first).  Triangle (i0,i1,i2) spans the frame a = p[i0], u = p[i1]-a, w = u x (p[i2]-a), v = w x u, normalised, all in
 * float64; its candidate is the box of all the job's points in that frame.  Outputs (device): `volumes` float64
 * [n_triangles] (written for every triangle of every job, not finite for a degenerate triangle or a job that holds an Inf or
 * NaN point), and per job `best` int32 (the finite volume that is smallest, the lowest index within the job among equal
 * ones, -1 if there is none) and `lohi` float64 [n_jobs,6] (min then max of the chosen candidate's projections; NaN for -1).
 * No float atomics: equal bytes from run to run, for a job alone or in a batch, and however its points are cut.
 * PGR_ERR_INVALID_ARGUMENT before anything is enqueued: NULL arrays that are needed, a negative count, a range that leaves
 * its array, triangles over no points.  The kernels do NOT clamp an index: when `triangles_host` (a host copy of
 * `triangles`, may be NULL) is given, every index of every job is checked against [0, point_count) here; a caller that passes
 * NULL has checked them itself.  n_jobs == 0: PGR_OK, no launch; a job without triangles: best = -1.  `jobs` is a host array.
 * Workspace (16-byte aligned): pgr_obb_candidates_workspace_bytes(n_jobs, jobs) device bytes; host-only, 0 for n_jobs <= 0,
 * NULL jobs, a negative count or triangles over no points.  A job's points go through LDS PGR_OBB_POINT_TILE at a time,
 * its triangles PGR_OBB_TRI_TILE per workgroup (tests/obb_cases.py is built around both). */
#define PGR_OBB_TRI_TILE 256
#define PGR_OBB_POINT_TILE 512
typedef struct PgrObbJob {
    int32_t point_first, point_count;
    int32_t tri_first, tri_count;
} PgrObbJob;
size_t pgr_obb_candidates_workspace_bytes(int32_t n_jobs, const PgrObbJob *jobs);
int32_t pgr_obb_candidates(const float *points, int64_t n_points, const int32_t *triangles, int64_t n_triangles,
                           const int32_t *triangles_host, int32_t n_jobs, const PgrObbJob *jobs, double *volumes,
                           int32_t *best, double *lohi, void *workspace, size_t workspace_bytes, void *stream);

/* The two points of every job's point range that lie farthest apart (the toolkit's misc.calc_pts_diameter, exact brute
 * force): d2(i,j) = fma(dz, dz, fma(dy, dy, dx dx)) of p[j] - p[i] in float64 over i < j.  `pair` device int32 [n_jobs,2]
 * receives the pair of largest d2 (indices within the job, the lexicographically lowest pair among equal ones), `d2` device
 * float64 [n_jobs] its value.  One point: pair (0,0), d2 0; no point: pair (-1,-1), d2 0.  A NaN distance is never chosen.
 * The jobs' triangle ranges are not read.  Equal bytes from run to run and for a job alone or in a batch.  Argument checks
 * as pgr_obb_candidates makes them for the points; workspace (16-byte aligned) of pgr_point_diameter_workspace_bytes device
 * bytes (host-only; 0 for n_jobs <= 0, NULL jobs or a negative count).  Points are walked PGR_DIAMETER_TILE at a time. */
#define PGR_DIAMETER_TILE 256
size_t pgr_point_diameter_workspace_bytes(int32_t n_jobs, const PgrObbJob *jobs);
int32_t pgr_point_diameter(const float *points, int64_t n_points, int32_t n_jobs, const PgrObbJob *jobs, int32_t *pair,
                           double *d2, void *workspace, size_t workspace_bytes, void *stream);

/* Gradients returned by pgr_backward (device pointers, any may be NULL = not wanted). */
typedef struct PgrGradOutputs {
    float *means2d;              /* [n,3] screen-space mean, NDC-scaled (what viewspace_points.grad receives) */
    float *means3d;              /* [n,3] */
    float *opacities;            /* [n]   */
    float *colors;               /* [n,3] wrt colors_precomp (or the SH-evaluated rgb) */
    float *shs;                  /* [n,sh_stride,3] */
    float *cov3d;                /* [n,6] wrt the stored covariance parameters */
    float *scales;               /* [n,3] */
    float *rotations;            /* [n,4] */
} PgrGradOutputs;

/* THE backward (PgrBackwardCall below), of a pgr_forward call without semantic, posed or layers: the gradients of a loss
 * over all n_views images at once; one view is a batch of one (same kernels, same results).  Replaces _C.rasterize_gaussians_backward of the
 * reference's extension (used by training only: /root/reference/src/gs/gs_training.py:7,46).  `workspace` must be exactly
 * as that call left it (same n, image size, max_instances_per_view and n_views) and is only read; `cameras` are the forward's
 * (only the image size is read: the packed cameras live in the workspace).  `views` is a HOST array of n_views entries, one
 * per view: dL/dcolor, optionally dL/ddepth, and the forward's final_T / n_contrib / radii outputs.
 * `grad_alpha`: the gradient of the accumulated opacity alpha = 1 - final_T, a HOST array of n_views device pointers ([1,H,W]
 * each), any of which may be NULL; the whole array may be NULL.  For every blended entry i of a pixel, dalpha/dalpha_i =
 * final_T / (1 - alpha_i), under the colour term's conventions (the 0.99 clamp passes the gradient straight through, the
 * T < 1e-4 stop and n_contrib bound the walk).  NULL reads nothing and adds nothing.
 * Every gradient in `grads` is the SUM over the views, except means2d, which is [n_views, n, 3] view-major: each view's own
 * screen-space gradient (densification gathers its statistics per view).  Two launches do the work: the compositor backward
 * of every (view, tile) list in the forward's interleaved work order, and one thread per Gaussian looping over the views in
 * order (cov3D -> scale / rotation once, on the summed cov3D gradient; no atomics across views).
 * `scratch`: device memory of pgr_backward_batch_scratch_bytes(n, n_views) bytes -- per-view accumulator rows of 48 bytes
 * per Gaussian (48 n n_views: 768 MB for 8 views of 2 M Gaussians) and a small table.
 * PGR_ERR_INVALID_ARGUMENT (before anything is enqueued): call NULL, shs_rest, NULL cameras / views / grads, n_views <= 0, mixed
 * image sizes, a view without grad_color / final_T / n_contrib (or radii, n > 0), scratch NULL or smaller than required; with
 * camera_grads (below): camera_scratch NULL or smaller than pgr_camera_grad_scratch_bytes(n, n_views). */
typedef struct PgrBackwardView {
    const float *grad_color;     /* [3,H,W] required */
    const float *grad_depth;     /* [1,H,W] or NULL */
    const float *final_T;        /* [H,W]   the forward's */
    const uint32_t *n_contrib;   /* [H,W]   the forward's */
    const int32_t *radii;        /* [n]     the forward's (required) */
} PgrBackwardView;
size_t pgr_backward_batch_scratch_bytes(int32_t n, int32_t n_views);
/* Camera gradients: the exact partials of the loss with respect to the 35 camera numbers the forward reads per view --
 * viewmatrix [16] and projmatrix [16] (PgrCamera's transposed storage) and campos [3] -- each treated as an independent
 * input (a caller that ties them together, e.g. through a pose, composes them).  With p = (x, y, z, 1) per Gaussian the
 * view rendered (radii > 0, no overflow): viewmatrix through the view-space position t_r = sum_k p_k vm[4k+r] (depth, the
 * Jacobian, the 1.3 tanfov clamp) and the Jacobian product T = J W; projmatrix through the projected screen position;
 * campos through the SH view direction (0 with colors_precomp).  vm[4k+3] and pm[4k+2] are never read: exactly 0.
 * Discrete decisions (near cull, radius, tile rectangle, sort order) have no gradient.
 * The outputs are WRITTEN (not accumulated), on the stream, by two launches behind the scene backward: one thread per
 * Gaussian over the views, summed per workgroup in a fixed order into `cam_scratch`, then one workgroup per view summing
 * its partials in a fixed order (deterministic; no float atomics). */
typedef struct PgrCameraGrad {   /* device pointers, any NULL = not wanted; WRITTEN, not accumulated */
    float *viewmatrix;           /* [16] same storage as PgrCamera::viewmatrix */
    float *projmatrix;           /* [16] */
    float *campos;               /* [3]  */
} PgrCameraGrad;
/* Device scratch of the camera kernels: 140 bytes per view and 256 Gaussians (0 for n < 0 or n_views <= 0). */
size_t pgr_camera_grad_scratch_bytes(int32_t n, int32_t n_views);

typedef struct PgrBackwardCall {
    const PgrScene *scene;
    int32_t n_views;
    const PgrCamera *cameras;
    const PgrBackwardView *views;
    const float *const *grad_alpha;      /* NULL, or n_views entries, any NULL */
    void *workspace;
    size_t workspace_bytes;
    int64_t max_instances_per_view;
    const PgrGradOutputs *grads;
    void *scratch;                       /* device, pgr_backward_batch_scratch_bytes(n, n_views) */
    size_t scratch_bytes;
    const PgrCameraGrad *camera_grads;   /* NULL = scene gradients only (and no camera launch); else a HOST array of n_views
                                            entries; the scene gradients are the same with it and without */
    void *camera_scratch;                /* device, pgr_camera_grad_scratch_bytes(n, n_views); only with camera_grads */
    size_t camera_scratch_bytes;
} PgrBackwardCall;
int32_t pgr_backward(const PgrBackwardCall *call, void *stream);

/* present[i] = 1 iff Gaussian i passes the near-plane test of `viewmatrix` (device [16]). */
int32_t pgr_mark_visible(int32_t n, const float *means3d, const float *viewmatrix, uint8_t *present,
                         void *stream);

/* masks[b,k,y,x] = || img[b,:,y,x] - colors[k,:] ||_2 <= threshold   (uint8 0/1); img is a contiguous batch of
 * n_images CHW fp32 images, masks the matching [n_images,k,H,W] batch. */
int32_t pgr_color_masks(const float *img_chw, int32_t n_images, int32_t width, int32_t height,
                        const float *colors_k3, int32_t k, float threshold, uint8_t *masks_khw, void *stream);

/* rgb_hwc = uint8(img*255) (wraps, no clamp), depth_mm = uint16(depth*1000). Either pair may be NULL. */
int32_t pgr_quantize_frame(const float *img_chw, const float *depth_hw, int32_t width, int32_t height,
                           uint8_t *rgb_hwc, uint16_t *depth_mm_hw, void *stream);

/* Batch form of pgr_quantize_frame plus the K per-object masks of every frame as bit planes -- one launch turns a
 * finished batch into what leaves the GPU (the writer threads of /root/reference/pegasus.py:346-358, or the gather of
 * finished frames to the root rank):
 *   rgb_bhwc[b]      = uint8(color[b] * 255)   (wraps, no clamp)        color_b3hw  [n_images,3,H,W]
 *   depth_mm_bhw[b]  = uint16(depth[b] * 1000)                          depth_bhw   [n_images,H,W]
 *   mask_bits_bhwj[b,y,x,j] bit (m % 8) = masks[b,m,y,x] != 0, j = m / 8   masks_bkhw  [n_images,k,H,W] of
 *                      pgr_color_masks; ceil(k/8) bytes per pixel (one byte for the usual k <= 8 objects)
 * Each input/output pair may be NULL (both or neither). */
int32_t pgr_pack_frames(const float *color_b3hw, const float *depth_bhw, const uint8_t *masks_bkhw, int32_t n_images,
                        int32_t k, int32_t width, int32_t height, uint8_t *rgb_bhwc, uint16_t *depth_mm_bhw,
                        uint8_t *mask_bits_bhwj, void *stream);

/* One RECORD per frame -- everything that leaves the GPU for a finished frame, contiguous, so that a batch is one buffer
 * for the disk writers and ONE collective for the gather to the root rank (3.84 MB per 800x800
 * frame at K <= 8):
 *   [0, 3P)                       uint8 rgb HWC   = uint8(color * 255)      (wraps, no clamp; pegasus.py:347)
 *   [off_depth, off_depth + 2P)   uint16 depth mm = uint16(depth * 1000)    (pegasus.py:355), little endian
 *   [off_masks, off_masks + J P)  mask bit planes, J = ceil(k / 8) bytes per pixel: bit (m % 8) of byte m / 8 = mask m
 * with P = width x height and the three offsets / the record size rounded up to 16 bytes (pgr_frame_record_layout).
 * records: device uint8, record b at records + b * record_stride (record_stride >= layout.bytes, a multiple of 16). */
typedef struct PgrRecordLayout {
    int64_t off_rgb, off_depth, off_masks, bytes;
} PgrRecordLayout;
int32_t pgr_frame_record_layout(int32_t width, int32_t height, int32_t k, PgrRecordLayout *layout);
int32_t pgr_pack_records(const float *color_b3hw, const float *depth_bhw, const uint8_t *masks_bkhw, int32_t n_images,
                         int32_t k, int32_t width, int32_t height, uint8_t *records, int64_t record_stride, void *stream);

/* ---- COCO annotations of binary masks (pegasus_amd/coco.py; csrc/cocorle.hip.h) -------------------------------------------
 * The BOP toolkit's bop_toolkit_lib/pycoco_utils.py on the device: binary_mask_to_rle, bbox_from_binary_mask,
 * rle_to_binary_mask and the integer parts of compute_ious.  A mask is uint8 [height,width], row-major, masks of a stack
 * follow each other without padding (mask k starts at byte k * height * width: no alignment is asked of it); a pixel is SET
 * when its byte is non-zero.  width and height are 1..8192 each.  Everything is an integer and no result depends on the
 * order of execution.
 *
 * Run-length encoding: pixels in column-major order, p = x * height + y; runs alternate and start with a run of zeros
 * (counts[0] = 0 when pixel 0 is set); an all-zero mask is [H*W], an all-set one [0, H*W]; a run that leaves a column at its
 * bottom and enters the next at its top is ONE run.  n_counts = transitions + 1 + (pixel 0 set).
 *
 * Two calls, as pgr_march_count / pgr_march_emit: the count pass leaves the masks as bit planes and per-column records in
 * `workspace` (pgr_mask_rle_workspace_bytes: about H*W/8 + 16 W bytes per mask; 0 for n_masks <= 0 or a side outside
 * 1..8192; device memory, 16-byte aligned) and writes
 *   stats int32 [n_masks,6] = n_counts, area (set pixels), x_min, y_min, x_max, y_max of the set pixels
 * (INT32_MAX / INT32_MIN extents for an empty mask, as pgr_bop_gt_info writes them; the COCO box is
 * [x_min, y_min, x_max - x_min + 1, y_max - y_min + 1]).  The caller forms offsets int64 [n_masks+1], the exclusive sum of
 * n_counts (device memory), allocates counts int32 [capacity] and calls the emit pass with the SAME workspace, untouched in
 * between (`masks` is not read again): mask k's counts go to counts[offsets[k] .. offsets[k+1]).  `total` is offsets[n_masks]
 * as the caller computed it: capacity < total, total < n_masks or total > n_masks * (H*W + 1) is refused on the host, and no
 * store leaves counts[offsets[k] .. min(offsets[k+1], total)) whatever the device-side offsets hold.  No atomics: two runs
 * give equal bytes.  The tile sizes below are the shapes at which the kernels change path (for tests). */
#define PGR_RLE_WORD_ROWS 32         /* rows per bit-plane word */
#define PGR_RLE_TILE_COLS 256        /* columns per wave of the plane kernel, and per workgroup of the column kernels */
#define PGR_RLE_BLOCK_ROWS 128       /* rows per workgroup of the plane kernel */
#define PGR_RLE_DECODE_CHUNK 256     /* runs a decode workgroup scans at a time */
#define PGR_RLE_DECODE_MIN_SLICE 16384   /* pixels per decode workgroup, at least */
#define PGR_RLE_DECODE_MAX_SLICES 64  /* decode workgroups per mask, at most: beyond, the slices grow */
#define PGR_MASK_OVERLAP_CHUNK 16384 /* pixels per overlap workgroup */
size_t pgr_mask_rle_workspace_bytes(int32_t n_masks, int32_t width, int32_t height);
int32_t pgr_mask_rle_count(const uint8_t *masks, int32_t n_masks, int32_t width, int32_t height, int32_t *stats,
                           void *workspace, size_t workspace_bytes, void *stream);
int32_t pgr_mask_rle_emit(const uint8_t *masks, int32_t n_masks, int32_t width, int32_t height, const int64_t *offsets,
                          int64_t total, int32_t *counts, int64_t capacity, const void *workspace, size_t workspace_bytes,
                          void *stream);
/* rle_to_binary_mask for the list form: masks uint8 [n_masks,height,width] of 0 / 1 from counts int32 (device) and offsets
 * int64 [n_masks+1] (device; mask k's counts are counts[offsets[k] .. offsets[k+1])).  Every pixel is written once.
 * Zero-length runs are legal anywhere.  Negative counts read as 0; pixels behind the last run are 0 and runs beyond H*W are
 * cut -- the toolkit does the same silently, pegasus_amd.coco.rle_decode refuses such lists before it calls. */
int32_t pgr_mask_rle_decode(const int32_t *counts, const int64_t *offsets, int32_t n_masks, int32_t width, int32_t height,
                            uint8_t *masks, void *stream);
/* inter int32 [n_a,n_b] = pixels set in both a[i] and b[j]; area_a int32 [n_a], area_b int32 [n_b] = set pixels; a and b
 * uint8 [n,height,width].  The union is area_a[i] + area_b[j] - inter[i,j].  Integer atomic adds into outputs the call
 * clears first: exact, whatever the order.  n_a, n_b >= 1. */
int32_t pgr_mask_overlap(const uint8_t *a, int32_t n_a, const uint8_t *b, int32_t n_b, int32_t width, int32_t height,
                         int32_t *inter, int32_t *area_a, int32_t *area_b, void *stream);

/* ---- COCO detection / segmentation scores (pegasus_amd/coco_eval.py; csrc/cocoeval.hip.h) --------------------------------
 * pycocotools.COCOeval as the BOP toolkit's scripts/eval_bop22_coco.py runs it, in four device stages that work from run
 * lists and boxes, never from pixels.  pycocotools is not a requirement of this project: parity with it is pinned by the
 * written rule at the top of csrc/cocoeval.hip.h and by hand-worked known answers, not by recorded
 * outputs.  Every result is an integer or a float64 produced by a fixed sequence of IEEE operations; no atomics: two runs
 * give equal bytes.
 *
 * A GROUP is one (image, category): dt_count detections from dt_begin (sorted by -score, stable, cut to maxDets[-1] by the
 * caller) and gt_count ground-truth annotations from gt_begin (file order); its IoU matrix is
 * iou[iou_offset + d * gt_count + g], float64.  The table is HOST memory, read during the call (it is copied into the
 * workspace in stream order, and the call returns when the copy has been made: the one wait of these entries).  Refused on the host with PGR_ERR_INVALID_ARGUMENT: a negative count, a slice outside [0, n_dt) / [0, n_gt) /
 * [0, iou_total), and groups that are not ascending and disjoint in all three (dt_begin, gt_begin and iou_offset of a group
 * are at or behind the previous group's ends): no two groups write one element.  Either count may be 0.
 * Every entry checks its arguments on the host before anything is enqueued; every *_workspace_bytes is host-only and
 * returns 0 for invalid arguments; workspaces are device memory, 16-byte aligned. */
typedef struct PgrCocoGroup {
    int32_t dt_begin, dt_count, gt_begin, gt_count;
    int64_t iou_offset;
} PgrCocoGroup;
#define PGR_COCO_CHUNK 256           /* elements a workgroup scans at a time (runs of a mask, detections of a category) */
#define PGR_COCO_LDS_RUNS 4096       /* GT runs of one group staged in LDS, at most: beyond, they are read from the workspace */
#define PGR_COCO_MAX_LANES 64        /* n_area * n_thr of one call, at most (one lane each) */
#define PGR_COCO_MAX_MAXDETS 8       /* n_max_dets, at most */
/* Mask IoU inside groups from run lists in the layout pgr_mask_rle_emit produces: counts int32 [*_total] and offsets int64
 * [n+1], both device (mask k: counts[offsets[k] .. offsets[k+1])); *_total is the length of the counts array, and no read
 * leaves it whatever the offsets hold.  Negative counts read as 0 and sums beyond H*W are cut, as pgr_mask_rle_decode does;
 * zero-length runs are legal anywhere.  gt_crowd uint8 [n_gt].  Writes dt_area int64 [n_dt], gt_area int64 [n_gt] (set
 * pixels, of every mask, grouped or not), and per group inter int64 = pixels set in both and
 *   iou = inter == 0 ? 0 : inter / (crowd ? area_d : area_d + area_g - inter)      (one float64 division). */
size_t pgr_rle_iou_workspace_bytes(int32_t n_groups, int64_t dt_total, int64_t gt_total);
int32_t pgr_rle_iou(const int32_t *dt_counts, const int64_t *dt_offsets, int32_t n_dt, int64_t dt_total,
                    const int32_t *gt_counts, const int64_t *gt_offsets, int32_t n_gt, int64_t gt_total,
                    const uint8_t *gt_crowd, int32_t width, int32_t height, const PgrCocoGroup *groups, int32_t n_groups,
                    int64_t iou_total, int64_t *inter, double *iou, int64_t *dt_area, int64_t *gt_area, void *workspace,
                    size_t workspace_bytes, void *stream);
/* Box IoU inside groups: boxes float64 [n,4] = x, y, w, h (device).  iw = min(dx+dw, gx+gw) - max(dx, gx), ih likewise,
 * inter = iw*ih if both > 0 else 0, union = dw*dh + gw*gh - inter (dw*dh for a crowd), iou = inter == 0 ? 0 : inter / union:
 * each an IEEE operation of its own, in this order (nothing is contracted into an FMA).  0 where pycocotools divides 0/0. */
size_t pgr_box_iou_workspace_bytes(int32_t n_groups);
int32_t pgr_box_iou(const double *dt_boxes, int32_t n_dt, const double *gt_boxes, int32_t n_gt, const uint8_t *gt_crowd,
                    const PgrCocoGroup *groups, int32_t n_groups, int64_t iou_total, double *iou, void *workspace,
                    size_t workspace_bytes, void *stream);
/* COCOeval.evaluateImg for every group, area range and threshold at once.  iou_thrs [n_thr] and area_rng [n_area,2] = lo, hi
 * are HOST arrays; n_thr * n_area <= PGR_COCO_MAX_LANES.  dt_area, gt_area float64, gt_flag uint8 (the ignore flag: iscrowd,
 * or iscrowd | ignore), gt_crowd uint8: device.  A GT is ignored for range a when gt_flag or area < lo or area > hi.  Writes,
 * for the slices of the groups only (rows of detections and GT in no group keep their bytes):
 *   dt_match int32 [n_area,n_thr,n_dt]   index (into the GT arrays) of the GT the detection is matched to, -1 for none
 *   dt_ignore uint8 [n_area,n_thr,n_dt]  the matched GT's ignore flag; unmatched: area outside [lo, hi]
 *   gt_match int32 [n_area,n_thr,n_gt]   index of the detection matched to the GT (the last one for a crowd), -1 for none
 *   gt_ignore uint8 [n_area,n_gt]
 * Detections are visited in the order of the table, so the first m of a group are matched as if the rest were absent. */
size_t pgr_coco_match_workspace_bytes(int32_t n_groups, int32_t n_gt, int32_t n_area);
int32_t pgr_coco_match(const PgrCocoGroup *groups, int32_t n_groups, int64_t iou_total, const double *iou,
                       const double *dt_area, int32_t n_dt, const double *gt_area, const uint8_t *gt_flag,
                       const uint8_t *gt_crowd, int32_t n_gt, const double *iou_thrs, int32_t n_thr, const double *area_rng,
                       int32_t n_area, int32_t *dt_match, uint8_t *dt_ignore, int32_t *gt_match, uint8_t *gt_ignore,
                       void *workspace, size_t workspace_bytes, void *stream);
/* COCOeval.accumulate.  perm int64 [n_dt]: the detections stably sorted by (category, -score) over images in ascending id;
 * seg_start int64 [n_cat+1]: category k is perm[seg_start[k] .. seg_start[k+1]); rank int32 [n_dt]: the detection's place in
 * its group; npig int32 [n_cat,n_area]: GT of the category not ignored for the range; rec_thrs float64 [n_rec]; dt_scores
 * float64 [n_dt]: all device (entries of perm outside [0, n_dt) are skipped and seg_start is cut to [0, n_dt]).  max_dets
 * int32 [n_max_dets] is a HOST array.  Writes every cell once: precision and scores float64 [n_thr,n_rec,n_cat,n_area,
 * n_max_dets], recall float64 [n_thr,n_cat,n_area,n_max_dets]; -1 where npig == 0. */
size_t pgr_coco_accumulate_workspace_bytes(int32_t n_dt, int32_t n_area, int32_t n_max_dets);
int32_t pgr_coco_accumulate(const int64_t *perm, const int64_t *seg_start, int32_t n_cat, const int32_t *rank,
                            const int32_t *dt_match, const uint8_t *dt_ignore, const double *dt_scores, int32_t n_dt,
                            const int32_t *npig, const int32_t *max_dets, int32_t n_max_dets, const double *rec_thrs,
                            int32_t n_rec, int32_t n_thr, int32_t n_area, double *precision, double *scores, double *recall,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ---- training step (pegasus_amd/train_ops.py) ----------------------------------------------------------------------------
 * Fused 3DGS image loss over x, y [3,H,W] fp32 (x: the render, y: the ground truth):
 *   loss = (1 - lambda) mean|x - y| + lambda (1 - mean SSIM(x, y))
 * SSIM with an 11x11 Gaussian window (sigma 1.5, normalised), one window per channel, zero padding 5, C1 = 0.01^2,
 * C2 = 0.03^2; means over all 3 H W values.  out3 (device, 3 floats) = {loss, mean |x - y|, mean SSIM}; grad (device
 * [3,H,W], may be NULL for the value only) = dloss/dx, with sign(0) = 0 for the L1 term.  Deterministic: the sums run in a
 * fixed order, without atomics.  Accuracy against float64: about 1e-6 of the largest gradient element and 1e-7 in the loss
 * on textured images.  On flat images (a constant background, a render that has converged to it) E[x^2] - mu^2 cancels to
 * about 1e-7 against C2 = 9e-4, as in any float32 SSIM: expect 7e-4 of the largest gradient element and 3e-5 in the mean
 * SSIM (the float32 arithmetic itself, measured by tests/test_train_kernels_gpu.py).  Identical images give exactly 0.
 * workspace >= pgr_image_loss_workspace_bytes(height, width). */
size_t pgr_image_loss_workspace_bytes(int32_t height, int32_t width);
int32_t pgr_image_loss(const float *x, const float *y, int32_t height, int32_t width, double lambda_dssim, float *out3,
                       float *grad, void *workspace, size_t workspace_bytes, void *stream);

/* The image loss against a MASKED target, plus an opacity term (training an object from per-image masks):
 *   y' = y m + bg (1 - m)                                  (formed on the fly; no [3,H,W] target is written)
 *   loss = (1 - lambda) mean|x - y'| + lambda (1 - mean SSIM(x, y')) + lambda_alpha mean|a - m|
 * mask m [H,W] in 0..1, bg [3] (the step's background, device), alpha a [H,W] (the render's 1 - final_T), all device fp32.
 * out4 (device, 4 floats) = {loss, mean |x - y'|, mean SSIM, mean |a - m| (0 without alpha)}; grad = dloss/dx [3,H,W] or
 * NULL; grad_alpha = dloss/da [H,W] or NULL (sign(0) = 0).  mask = NULL is pgr_image_loss (bit for bit, out4[3] = 0).
 * PGR_ERR_INVALID_ARGUMENT before anything is enqueued: a mask without bg, alpha without a mask, lambda_alpha < 0,
 * lambda_alpha > 0 without alpha, grad_alpha without alpha (and pgr_image_loss's own checks).  Deterministic, like
 * pgr_image_loss.  workspace >= pgr_image_loss_masked_workspace_bytes(height, width). */
size_t pgr_image_loss_masked_workspace_bytes(int32_t height, int32_t width);
int32_t pgr_image_loss_masked(const float *x, const float *y, const float *mask, const float *bg, const float *alpha,
                              int32_t height, int32_t width, double lambda_dssim, double lambda_alpha, float *out4,
                              float *grad, float *grad_alpha, void *workspace, size_t workspace_bytes, void *stream);

/* One Adam step over up to PGR_ADAM_MAX_GROUPS parameter groups in one launch, with torch.optim.Adam's single-tensor
 * arithmetic (no weight decay, no amsgrad).  The table is HOST memory, read during the call; every pointer in it is a
 * device fp32 array of n elements.  step is the step count AFTER this update (1 on the first step); the bias corrections
 * are formed on the host in double, as torch forms them.  Groups with n = 0 are skipped. */
#define PGR_ADAM_MAX_GROUPS 16
typedef struct PgrAdamGroup {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t n;
    double lr;
    int64_t step;
} PgrAdamGroup;
int32_t pgr_adam_step(const PgrAdamGroup *groups, int32_t n_groups, double beta1, double beta2, double eps, void *stream);

/* Densification statistics of one render, for every Gaussian i with radii[i] > 0:
 *   grad_accum[i] += || viewspace_grad[i, 0:2] ||,  denom[i] += 1,  max_radii2d[i] = max(max_radii2d[i], radii[i])
 * viewspace_grad: [n, grad_stride] fp32 (the screen-space gradient of render()'s "viewspace_points"). */
int32_t pgr_densify_stats(int32_t n, const float *viewspace_grad, int32_t grad_stride, const int32_t *radii,
                          float *grad_accum, float *denom, float *max_radii2d, void *stream);

/* ---- ground plane by RANSAC (pegasus_amd/alignment.py) --------------------------------------------------------------------
 * The dominant plane of a point cloud (open3d's segment_plane, on which the reference's ReconstructionAlignment.align2plane
 * rests: /root/reference/src/reconstruction/environment_reconstruction.py:53-66; DESIGN.md section 18 holds the rules).
 * `xyz` is a device float32 [n,3]; a plane is four float64 (nx, ny, nz, d).  Every argument check comes before any launch:
 * PGR_ERR_INVALID_ARGUMENT for a needed NULL, a negative count, a workspace that is not 16-byte aligned, a threshold that is
 * not finite and positive or (pgr_plane_inliers) a plane or pivot value that is not finite; PGR_ERR_WORKSPACE_TOO_SMALL
 * otherwise.  A count of 0 returns PGR_OK without a launch (outputs that have rows are set to 0).  The size functions return 0
 * for a negative count.  Results are identical from call to call.  The caller's contract, which the entries cannot check:
 * every coordinate is finite.
 *
 * pgr_plane_hypotheses: the plane through rows (i0, i1, i2) of `triples` (device int32 [n_hyp,3]).  With the points widened
 * exactly to float64 and every operation rounded on its own: e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2 (each component
 * (a*b) - (c*d)), norm = sqrt(((cx*cx) + cy*cy) + cz*cz), nrm = c / norm, d = -(((nx*x0) + ny*y0) + nz*z0).  `planes` float64
 * [n_hyp,4], `valid` uint8 [n_hyp].  A row outside [0, n) is never dereferenced: such a triple, one with two equal rows, a norm
 * of 0 and a norm that is not finite give four zeros and valid = 0.
 *
 * pgr_plane_score: every plane against every point.  dist = |((nx*x + ny*y) + nz*z) + d| in float64, every operation rounded
 * on its own; the point is an inlier iff dist < threshold (STRICTLY).  counts int32 [n_hyp] (exact), sumsq float64 [n_hyp]:
 * the sum of dist*dist over the inliers, in a fixed order without floating-point atomics.  A plane of four zeros scores 0, 0.
 * The points are read once per call; workspace: pgr_plane_score_workspace_bytes(n, n_hyp) bytes, 12 bytes per hypothesis and
 * PGR_PLANE_TILE points.
 *
 * pgr_plane_inliers: one pass under one plane.  `plane` (HOST float64 [4]) and `pivot` (HOST float64 [3]) are read during the
 * call and handed to the kernel by value.  mask (device uint8 [n], may be NULL): 1 for the inliers.  sums (device float64
 * [PGR_PLANE_SUMS]) over the inliers, with q = p - pivot in float64: [0] the count (a sum of ones)  [1,4) sum q  [4,10) the
 * upper triangle of sum q q^T, row by row  [10] sum dist*dist  [11] 0.  A plane of four zeros has no inliers.  Workspace:
 * pgr_plane_inliers_workspace_bytes(n) bytes. */
#define PGR_PLANE_SUMS 12
#define PGR_PLANE_TILE 2048
int32_t pgr_plane_hypotheses(int32_t n, const float *xyz, int32_t n_hyp, const int32_t *triples, double *planes, uint8_t *valid,
                             void *stream);
size_t pgr_plane_score_workspace_bytes(int32_t n, int32_t n_hyp);
int32_t pgr_plane_score(int32_t n, const float *xyz, int32_t n_hyp, const double *planes, double threshold, int32_t *counts,
                        double *sumsq, void *workspace, size_t workspace_bytes, void *stream);
size_t pgr_plane_inliers_workspace_bytes(int32_t n);
int32_t pgr_plane_inliers(int32_t n, const float *xyz, const double *plane, const double *pivot, double threshold,
                          uint8_t *mask, double *sums, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Mesh decimation by vertex clustering (after open3d's TriangleMesh.simplify_vertex_clustering; the rule stands at the top
 * of pegasus_amd/csrc/decimate.hip.h and in DESIGN.md section 19; parity with open3d is not pinned).  `vertices` is a device
 * float32 [n_vertices,3], `faces` a device int32 [n_faces,3]; n_vertices <= 2^30 and 3 n_faces < 2^31.  `voxel` is the cell
 * edge and (lo_x, lo_y, lo_z) the grid's origin: the caller's minimum over the vertices minus voxel / 2.
 *
 * Two calls, as pgr_march_count / pgr_march_emit.  pgr_mesh_cluster_count numbers the occupied cells and the distinct
 * canonical faces and writes device int64 counts[2] = {K, F'}; the caller reads them (its only wait), allocates vertices
 * float64 [K,3], faces int32 [F',3], cluster_of_vertex int32 [n_vertices] and used_quadric uint8 [K], and calls
 * pgr_mesh_cluster_emit once with the same mesh, grid and workspace and with n_clusters = K, n_out_faces = F'.  No row at or
 * past either number is written, whatever the workspace holds.  `contraction` picks the vertex of a cluster: the mean of its
 * vertices, or the minimiser of its faces' plane quadrics where that is well conditioned and lies in the cell (used_quadric =
 * 1), the mean elsewhere.
 *
 * The library allocates nothing: pgr_mesh_cluster_workspace_bytes(n_vertices, n_faces) device bytes (a host-only function; 0
 * for a count out of range), 16-byte aligned.  Every argument check comes before any launch: PGR_ERR_INVALID_ARGUMENT for a
 * needed NULL, a count out of range, a voxel that is not finite and positive, an origin that is not finite, an unknown
 * contraction, n_clusters > n_vertices or n_out_faces > n_faces; PGR_ERR_WORKSPACE_TOO_SMALL otherwise.  n_vertices == 0
 * gives counts {0, 0} and emits nothing.  Both calls run on `stream`, use no floating-point atomic and return the same bytes
 * from call to call.  A face index outside [0, n_vertices) is never dereferenced: the face is dropped and adds nothing to any
 * quadric.  The caller's contract, which the entries cannot check: every coordinate finite and (max - min) / voxel + 1 < 2^20
 * per axis; outside it cell indices clamp to [0, 2^20 - 1], so every access stays in bounds and only the result is wrong. */
#define PGR_CONTRACTION_AVERAGE 0
#define PGR_CONTRACTION_QUADRIC 1
size_t pgr_mesh_cluster_workspace_bytes(int32_t n_vertices, int32_t n_faces);
int32_t pgr_mesh_cluster_count(int32_t n_vertices, const float *vertices, int32_t n_faces, const int32_t *faces, double voxel,
                               double lo_x, double lo_y, double lo_z, void *workspace, size_t workspace_bytes, int64_t *counts,
                               void *stream);
int32_t pgr_mesh_cluster_emit(int32_t n_vertices, const float *vertices, int32_t n_faces, const int32_t *faces, double voxel,
                              double lo_x, double lo_y, double lo_z, int32_t contraction, void *workspace,
                              size_t workspace_bytes, int64_t n_clusters, int64_t n_out_faces, double *out_vertices,
                              int32_t *out_faces, int32_t *cluster_of_vertex, uint8_t *used_quadric, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Per-vertex normals and colours of an extracted mesh (pegasus_amd/mesh.py; the rules stand at the top of
 * pegasus_amd/csrc/meshattr.hip.h and in DESIGN.md section 21).  `vertices` is a device float32 [n_vertices,3], `faces` a
 * device int32 [n_faces,3].  Both entries run on `stream`, allocate nothing, wait for nothing, and return the same bytes from
 * call to call.  Every argument check comes before any launch and gives PGR_ERR_INVALID_ARGUMENT.
 *
 * pgr_mesh_vertex_normals: the unit normals of the faces summed per vertex and normalised (the rule of open3d's
 * compute_vertex_normals), `normals` device float32 [n_vertices,3].  Per face, in float32, each operation rounded on its own:
 *   e1 = b - a, e2 = c - a, m = e1 x e2, len = sqrtf((m.x m.x + m.y m.y) + m.z m.z); the face adds nothing unless 0 < len < inf
 *   q = (int64) rintf((m / len) * 2^30), added to the sums of the face's three vertices with 64-bit integer atomics
 * and per vertex, in float64: s = (double) sum, normal = (float)(s / sqrt((s.x s.x + s.y s.y) + s.z s.z)), 0 where the length
 * is not > 0.  A face with an index outside [0, n_vertices) is never dereferenced and adds nothing.  Workspace:
 * pgr_mesh_vertex_normals_workspace_bytes(n_vertices) = 24 n_vertices device bytes, 8-byte aligned, zeroed by the entry (a
 * host-only function; 0 for n_vertices < 1); a shorter or missing one is an invalid argument.  n_vertices == 0 does nothing;
 * n_faces == 0 writes zeros.
 *
 * pgr_mesh_vertex_colors: every vertex projected into every view, averaged over the views that see it.  `cameras`, `depth`
 * (PGR_DEPTH_NORMALIZED) and `final_T` as pgr_tsdf_integrate takes them (n_views 1..256, all of one size; each camera's
 * viewmatrix, tanfovx/y and campos are read); `color` device float32 [n_views,3,H,W], rendered over a ZERO background;
 * `normals` device float32 [n_vertices,3] or NULL; `fill` HOST float32 [3], read during the call.  Per vertex p (normal n) and
 * view in order, in float32:
 *   (x,y,z) = viewmatrix . p; skipped when z <= 0.2
 *   pixel = floor((x/z) * W/(2 tanfovx) + (W-1)/2 + 0.5), likewise y; skipped outside the image
 *   alpha = 1 - final_T; skipped when alpha < alpha_min; skipped unless |depth - z| <= depth_tol (a NaN depth fails)
 *   with normals: e = campos - p, cs = (n . e) / |e|; skipped unless cs > cos_min; w = cs * cs.  Without: w = 1
 *   acc += w * (color / alpha) per channel, wsum += w, seen += 1
 * colors (device float32 [n_vertices,3]) = clamp(acc / wsum, 0, 1) where seen > 0, else fill; `seen` (device int32
 * [n_vertices], may be NULL) the number of views used.  Invalid: a needed NULL, n_views outside 1..256, views of mixed sizes,
 * alpha_min not > 0, depth_tol negative or NaN, cos_min NaN.  n_vertices == 0 does nothing. */
size_t pgr_mesh_vertex_normals_workspace_bytes(int32_t n_vertices);
int32_t pgr_mesh_vertex_normals(int32_t n_vertices, const float *vertices, int32_t n_faces, const int32_t *faces,
                                float *normals, void *workspace, size_t workspace_bytes, void *stream);
int32_t pgr_mesh_vertex_colors(int32_t n_vertices, const float *vertices, const float *normals, int32_t n_views,
                               const PgrCamera *cameras, const float *color, const float *depth, const float *final_T,
                               float depth_tol, float alpha_min, float cos_min, const float *fill, float *colors,
                               int32_t *seen, void *stream);

/* A texture for a mesh: a per-face atlas baked from the same views (pegasus_amd/mesh.py bake_texture).  The rules are pinned in
 * pegasus_amd/csrc/meshattr.hip.h and restated in tests/mesh_texture_reference.py, which the outputs equal bit for bit.
 * Layout: cell side `cell` = s >= 4 texels, leg L = s - 3, cells = ceil(n_faces / 2), cols = the smallest integer with
 * cols^2 >= cells, rows = ceil(cells / cols); `width` = cols s and `height` = rows s, each at most 8192, must be handed in as
 * such (pegasus_amd.mesh.texture_atlas_layout).  Face f lies in cell f >> 1, half f & 1; the cell's origin is ((c % cols) s,
 * (c / cols) s) from the top-left; texel (i, j) of a cell belongs to half 0 when i + j <= s - 1; in texel-centre coordinates half
 * 0 has its corners at (0.5, 0.5), (0.5 + L, 0.5), (0.5, 0.5 + L) and half 1 is its mirror image through the cell's centre.
 *
 * pgr_mesh_atlas_points: one lane per texel writes `points` and `normals` (device float32 [height*width,3]) and `face_of_texel`
 * (device int32 [height*width]): the owning face, or -1 (with zeros) where the half has no face, a face index is outside
 * [0, n_vertices) or the face normal's length is zero or not finite.  (di, dj) = (i, j) in half 0, (s - 1 - i, s - 1 - j) in half
 * 1; p = (A + (di / L) (B - A)) + (dj / L) (C - A) in float32, every operation rounded on its own; the normal is
 * cross(B - A, C - A) normalised (pgr_mesh_shade's flat rule in the model frame, no flip).  The colours of the points come from
 * pgr_mesh_vertex_colors, unchanged.
 *
 * pgr_mesh_atlas_pack: `colors` (device float32 [height*width,3], in [0,1]) and `seen` (device int32 [height*width]) to
 * `texture` (device uint8 [height,width,3]).  A texel of a face with seen > 0 gets (uint8)rintf(255 c) (a NaN gives 0); the face's
 * other texels get the mean of those, (2 sum + cnt) / (2 cnt) in integers, or, when it has none, row f of `face_fill` (device
 * uint8 [n_faces,3]; NULL: `fill`); texels of no face get `fill` (HOST uint8 [3]).  `face_seen` (device int32 [n_faces], may be
 * NULL) receives cnt.  One wave per cell, integer reductions: two runs give equal bytes.
 * Invalid (PGR_ERR_INVALID_ARGUMENT, before any launch): n_faces < 1, cell < 4, a size that is not the layout's or beyond 8192, a
 * NULL among the pointers not marked optional. */
int32_t pgr_mesh_atlas_points(int32_t n_vertices, const float *vertices, int32_t n_faces, const int32_t *faces, int32_t cell,
                              int32_t width, int32_t height, float *points, float *normals, int32_t *face_of_texel,
                              void *stream);
int32_t pgr_mesh_atlas_pack(int32_t n_faces, int32_t cell, int32_t width, int32_t height, const int32_t *face_of_texel,
                            const float *colors, const int32_t *seen, const uint8_t *face_fill, const uint8_t *fill,
                            uint8_t *texture, int32_t *face_seen, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Collision geometry: signed distance fields of triangle meshes and distance / sweep queries between posed bodies
 * (pegasus_amd/collision.py; the rules stand at the top of pegasus_amd/csrc/meshsdf.hip.h and in DESIGN.md section 22).  All
 * three entries run on `stream`, allocate nothing, wait for nothing, use no floating-point atomic and return the same bytes
 * from call to call.  Every argument check comes before any launch and gives PGR_ERR_INVALID_ARGUMENT.  Positive is outside.
 *
 * pgr_mesh_sdf: `vertices` device float32 [n_vertices,3], `faces` device int32 [n_faces,3], `grid` as above; `sdf` device
 * float32 [nz,ny,nx]: at every grid point the exact distance to the nearest triangle (a zero-area face counts as its segment
 * or point), negative where the generalized winding number (the faces' signed solid angles over 4 pi) is >= 0.5; `winding`
 * (device float32 [nz,ny,nx], may be NULL) receives that number.  n_faces == 0 writes +inf (and winding 0).  A face with an
 * index outside [0, n_vertices) is never dereferenced and adds nothing.  Brute force, points x faces, PGR_SDF_FACE_TILE faces
 * per pass through LDS: meant for collision meshes of a few 10^4 faces.  Invalid: a bad grid, a negative count, a needed NULL.
 *
 * pgr_sdf_sample: `points` device float32 [n_points,3]; `values` device float32 [n_points]: the trilinear field value;
 * `gradients` (device float32 [n_points,3], may be NULL): the analytic derivative of the trilinear cell.  Outside the grid the
 * value is sqrt(r^2 + max(field, 0)^2) with r the distance to the grid's box and the field taken at the clamped point (a lower
 * bound of the distance to the surface while the grid encloses the mesh), the gradient that of the clamped point.
 * n_points == 0 does nothing.
 *
 * pgr_sdf_sweep: `bodies` and `jobs` are HOST tables, read during the call and handed to the kernels by value.  A body is a
 * grid with its field (device, may be NULL for a body that is never a target), shell points (device float32 [n_shell,3], body
 * frame) and a pose (R row-major, t).  A job moves the shell of body `mover` along the unit vector `dir` against body
 * `target`, or against the plane n.x = d (`plane` = n, d; n a unit vector) when target == PGR_SWEEP_PLANE.  Per shell point:
 * phi0, the target's field at the point (pgr_sdf_sample's rule in the target's frame; n.x - d for the plane), and s, the free
 * travel by sphere tracing: the point steps by the sampled field while field > tol, s < max_travel and fewer than max_steps
 * steps were taken (closed form for the plane).  out (device uint64 [n_jobs,2]): word 0 the minimum of phi0, word 1 the
 * minimum of s over the job's points, each as (order-preserving bits of the float) << 32 | point index: bits ^ 0x80000000
 * for a float with a clear sign bit, ~bits otherwise.  Equal floats resolve to the lowest index; a job whose mover has no shell
 * points keeps all bits set.  Invalid: a needed NULL, a negative count, a job naming a body outside the table or itself, a
 * target without a field or with a bad grid, a direction or plane normal that is not finite and of unit length within 1e-4,
 * tol or max_travel that is NaN or negative, max_steps < 0.  n_jobs == 0 does nothing. */
#define PGR_SDF_FACE_TILE 256
#define PGR_SWEEP_PLANE (-1)
typedef struct PgrSdfBody {
    PgrGrid grid;
    const float *sdf;
    const float *shell;
    int32_t n_shell;
    float R[9];
    float t[3];
} PgrSdfBody;
typedef struct PgrSweepJob {
    int32_t mover, target;
    float dir[3];
    float plane[4];
} PgrSweepJob;
int32_t pgr_mesh_sdf(int32_t n_vertices, const float *vertices, int32_t n_faces, const int32_t *faces, const PgrGrid *grid,
                     float *sdf, float *winding, void *stream);
int32_t pgr_sdf_sample(const PgrGrid *grid, const float *sdf, int64_t n_points, const float *points, float *values,
                       float *gradients, void *stream);
int32_t pgr_sdf_sweep(int32_t n_bodies, const PgrSdfBody *bodies, int32_t n_jobs, const PgrSweepJob *jobs, float tol,
                      float max_travel, int32_t max_steps, uint64_t *out, void *stream);

/* ---- Rigid-body drops (pegasus_amd/dynamics.py; the rule stands at the top of pegasus_amd/csrc/rigid.hip.h and in DESIGN.md
 * section 24): S independent worlds of B <= PGR_RIGID_MAX_BODIES slots fall onto the plane n.x = d and onto each other.
 * Contacts come from the bodies' distance fields and shell points (pgr_mesh_sdf, pgr_sdf_sample's rule), a sequential-impulse
 * solver with friction steps them.  Both entries run on `stream`, allocate nothing, wait for nothing, use no floating-point
 * atomic and return the same bytes from call to call.  Every argument check comes before any launch and gives
 * PGR_ERR_INVALID_ARGUMENT.
 *
 * `types` is a HOST table of n_types <= PGR_RIGID_MAX_TYPES body types, read during the call and handed to the kernels by
 * value: geometry as in PgrSdfBody (shell points in the mesh frame), mass, centre of mass `com` (mesh frame), inverse inertia
 * about it (mesh frame, row-major), friction, and the bounding radius max |shell - com|.  `type` is device int32 [S,B]: the
 * type of every slot; a value outside [0, n_types) is an empty slot.  `state` is device float32 [S,B,PGR_RIGID_STATE]: centre
 * of mass x, unit quaternion q (x, y, z, w), v, omega, all in the world.
 *
 * pgr_rigid_contacts: `words` device uint64 [S, B*B, PGR_RIGID_WORDS].  Pair slot a*B + b is mover a against target b, slot
 * a*B + a mover a against the plane.  Word 0 is the minimum of the field value over the mover's shell points with value <=
 * params->margin, words 1..6 the minima of +x, -x, +y, -y, +z, -z of (point - x_a) over the same points, each packed as in
 * pgr_sdf_sweep; a pair without such a point (or out of bounding-sphere range, or with an empty slot) keeps all bits set.
 *
 * pgr_rigid_simulate: advances `state` by n_steps steps in place and enqueues all of them.  After every record_every-th step
 * the mesh-frame pose (t = x - R com, q) of every slot goes to `trajectory`, device float32 [S, n_steps / record_every, B, 7]
 * (may be NULL when that count is 0).  rest_step (device int32 [S]): the step at which the world fell asleep, -1 if never.
 * status (device int32 [S]): 1 where a state stopped being finite; such a world stays at its last finite state.  Both entries
 * take a `workspace` of pgr_rigid_workspace_bytes(S, B) bytes (0: arguments refused), 16-byte aligned.
 *
 * Invalid: a needed NULL, S < 0 or > 2^20, B < 0 or > PGR_RIGID_MAX_BODIES, n_types < 0 or > PGR_RIGID_MAX_TYPES (or 0 while
 * there are slots), a type with n_shell < 0, a missing shell, a field that is missing or has a bad grid while B > 1, a mass,
 * friction or radius that is not finite, mass <= 0, friction or radius < 0, a com or inertia entry that is not finite; h or
 * iterations <= 0 or not finite, a plane normal that is not of unit length within 1e-4, any other parameter that is not finite,
 * damping outside [0, 1), beta, slop, margin or a sleep threshold < 0, n_steps < 0, record_every < 1, a workspace that is too
 * small (PGR_ERR_WORKSPACE_TOO_SMALL).  S == 0 or B == 0 (and n_steps == 0) do nothing. */
#define PGR_RIGID_MAX_BODIES 8
#define PGR_RIGID_MAX_TYPES 16
#define PGR_RIGID_WORDS 7
#define PGR_RIGID_STATE 13
typedef struct PgrRigidType {
    PgrGrid grid;
    const float *sdf;
    const float *shell;
    int32_t n_shell;
    float mass;
    float com[3];
    float inv_inertia[9];
    float friction;
    float radius;
} PgrRigidType;
typedef struct PgrRigidParams {
    float h;
    float gravity[3];
    float plane[4];
    float plane_friction;
    float lin_damp, ang_damp;
    int32_t iterations;
    float beta, slop, margin;
    float v_sleep, w_sleep;
    int32_t sleep_steps;
} PgrRigidParams;
size_t pgr_rigid_workspace_bytes(int32_t n_worlds, int32_t n_slots);
int32_t pgr_rigid_contacts(const PgrRigidParams *params, int32_t n_types, const PgrRigidType *types, int32_t n_worlds,
                           int32_t n_slots, const int32_t *type, const float *state, uint64_t *words, void *workspace,
                           size_t workspace_bytes, void *stream);
int32_t pgr_rigid_simulate(const PgrRigidParams *params, int32_t n_types, const PgrRigidType *types, int32_t n_worlds,
                           int32_t n_slots, const int32_t *type, float *state, int32_t n_steps, int32_t record_every,
                           float *trajectory, int32_t *rest_step, int32_t *status, void *workspace, size_t workspace_bytes,
                           void *stream);
/* The same two entries with the ground as a static field in world coordinates (pgr_sdf_from_tsdf writes one): with `ground`
 * NULL they give the bytes of the entries above.  With a ground, pair slot a*B + a holds mover a against the field instead of
 * the plane: no contacts where (field at x_a) - radius_a - 2 ground voxels > margin; per shell point the value and gradient by
 * pgr_sdf_sample's rule at the world point (outside rule included), the unit gradient as the normal (a point whose gradient is
 * shorter than 1e-6 is no candidate); the ground's friction in place of plane_friction; the rows are the plane's rows and the
 * ground does not move.  params->plane is checked as before and not used.  Also invalid: a ground with a NULL field or a bad
 * grid, a friction that is negative or not finite. */
typedef struct PgrRigidGround {
    PgrGrid grid;
    const float *sdf;
    float friction;
} PgrRigidGround;
int32_t pgr_rigid_contacts_ground(const PgrRigidParams *params, const PgrRigidGround *ground, int32_t n_types,
                                  const PgrRigidType *types, int32_t n_worlds, int32_t n_slots, const int32_t *type,
                                  const float *state, uint64_t *words, void *workspace, size_t workspace_bytes, void *stream);
int32_t pgr_rigid_simulate_ground(const PgrRigidParams *params, const PgrRigidGround *ground, int32_t n_types,
                                  const PgrRigidType *types, int32_t n_worlds, int32_t n_slots, const int32_t *type, float *state,
                                  int32_t n_steps, int32_t record_every, float *trajectory, int32_t *rest_step, int32_t *status,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ---- PNG files of device images (pegasus_amd/png.py; csrc/png.hip.h, csrc/png_codes.h) ----------------------------------
 * bop_dataset.encode_png on the device: deflate, checksums and chunk framing of a batch of images that lie in device memory.
 * THE FILE.  A file is the PNG signature, IHDR, ONE IDAT, IEND.  Colour type / bit depth are 0/8 (kind 0, gray8), 2/8 (kind 1,
 * rgb8) and 0/16 (kind 2, gray16: little-endian 16-bit storage, written as big-endian samples); no interlace; every row has
 * filter type 0.  The IDAT payload is one zlib stream: the header 78 01, deflate data, the big-endian Adler-32 of the filtered
 * raw stream (height rows of 1 + row_bytes bytes).  The raw stream is cut into segments of PGR_PNG_SEGMENT_BYTES; one workgroup
 * encodes one segment independently of all others and no match reaches in front of its segment.  A segment becomes ONE deflate
 * block of the cheapest of three forms -- stored, fixed Huffman, dynamic Huffman, by the bytes the segment takes, ties to the
 * earlier in that order.  A Huffman-coded segment that is not the file's last is followed by an empty stored block (000, pad to
 * a byte, 00 00 FF FF) so that segments join at byte boundaries, as pigz joins its blocks; a stored block ends on a byte
 * boundary by itself and is followed by nothing.  The last block carries BFINAL and is padded to a byte.  So a segment never
 * takes more than its raw length + 5 bytes and a file never more than 63 + raw_bytes + 5 * n_segments (pgr_png_max_bytes).
 * Tokens: level 0 codes literals only.  Level 1 gives every position candidates from a hash table of the 3-byte strings at
 * earlier positions of the segment (filled one sub-block of PGR_PNG_SUBBLOCK positions after the other, the highest position
 * of a bucket wins: an integer maximum, so the table does not depend on the order of execution; a position sees the sub-blocks
 * in front of its own) and from the fixed distances 1, 2, 3, 6 and 1 + row_bytes; a candidate is extended to at most 258 bytes
 * inside the segment, the longest wins, ties go to the smaller distance, a match has at least 3 bytes; the parse is greedy from
 * the segment's first byte.  Code lengths are length-limited (15, and 7 for the code-length alphabet) by the one builder behind
 * pgr_png_code_lengths; codes are canonical (RFC 1951 3.2.2); runs of zero code lengths are sent as symbols 17 / 18, symbol 16 is not used.
 * Everything is integer work and every shared update is an integer atomic whose result does not depend on order: two runs give
 * equal bytes.  Nothing of a file is computed on the host.
 *
 * A job names one image where it lies: `pixels` (device) is the first sample of the first row, row y starts row_stride bytes
 * behind row y - 1 and pixel x pixel_stride bytes behind pixel x - 1 (>= 1, 3, 2 bytes for kind 0, 1, 2; row_stride >=
 * (width - 1) * pixel_stride + that), so a view into a frame record or a plane of a stack is read without a copy.  width and
 * height are 1..16384.  `scale` is 1 or 255 (kind 0 only): the sample is multiplied by it, which writes a 0/1 mask as 0/255.
 *
 * Two calls, as pgr_mask_rle_count / pgr_mask_rle_emit.  pgr_png_encode compresses every segment into `workspace`
 * (pgr_png_workspace_bytes: about the raw bytes of the jobs; 0 for n_jobs <= 0 or a job outside the domain above; device
 * memory, 16-byte aligned), combines the checksums and writes sizes int64 [n_jobs] (device), the bytes of each file.  The caller
 * forms offsets int64 [n_jobs + 1] (device), the exclusive sum of the sizes, allocates files uint8 [capacity] and calls
 * pgr_png_emit with the SAME jobs and workspace, untouched in between: file k goes to files[offsets[k] .. offsets[k+1]).
 * `total` is offsets[n_jobs] as the caller computed it; capacity < total is refused on the host and no store leaves
 * files[offsets[k] .. min(offsets[k+1], total)) whatever the device-side offsets hold.  level is 0 or 1.  The job table is
 * copied to the device before the call returns. */
#define PGR_PNG_SEGMENT_BYTES 8192   /* raw bytes per segment (one workgroup, one deflate block) */
#define PGR_PNG_SUBBLOCK 512         /* positions per hash sub-block */
#define PGR_PNG_GRAY8 0
#define PGR_PNG_RGB8 1
#define PGR_PNG_GRAY16 2
typedef struct PgrPngJob {
    const void *pixels;
    int32_t width, height;
    int32_t kind;
    int64_t row_stride;
    int32_t pixel_stride;
    int32_t scale;
} PgrPngJob;
size_t pgr_png_workspace_bytes(int32_t n_jobs, const PgrPngJob *jobs);
int32_t pgr_png_encode(const PgrPngJob *jobs, int32_t n_jobs, int32_t level, int64_t *sizes, void *workspace,
                       size_t workspace_bytes, void *stream);
int32_t pgr_png_emit(const PgrPngJob *jobs, int32_t n_jobs, const int64_t *offsets, int64_t total, uint8_t *files,
                     int64_t capacity, const void *workspace, size_t workspace_bytes, void *stream);
/* 63 + raw_bytes + 5 * n_segments: what no file of that shape exceeds; 0 outside the domain.  Host only. */
int64_t pgr_png_max_bytes(int32_t width, int32_t height, int32_t kind);
/* The code builder of the encoder on host arrays (the same __host__ __device__ function, csrc/png_codes.h): lengths uint8 [n]
 * of a prefix code for the symbols with freq != 0, none longer than `limit`, 0 for unused symbols; a single used symbol gets
 * length 1, two or more get a COMPLETE code (Kraft sum exactly 1) that costs no more than giving every used symbol
 * ceil(log2(used)) bits.  n is 1..288, limit 1..15 with n <= 2^limit, every freq <= 2^22.  Host only. */
int32_t pgr_png_code_lengths(const uint32_t *freq, int32_t n, int32_t limit, uint8_t *lengths);

/* ---- JPEG files of device images (pegasus_amd/jpeg.py; csrc/jpeg.hip.h) ----------------------------
 * Baseline sequential JPEG (8-bit, Huffman, one interleaved scan) of a batch of images that lie in device memory: SOI, APP0
 * JFIF 1.01, DQT, SOF0, DHT, DRI, SOS, entropy data, EOI.  Gray images have one component; RGB images become full-range YCbCr
 * at 4:4:4 or 4:2:0.  Quantisation tables follow the IJG rule on the Annex K tables (pgr_jpeg_quant_tables), the Huffman
 * tables are built per file on the device from the file's own symbol counts with the builder behind pgr_png_code_lengths
 * (limit 16), restart intervals are PGR_JPEG_RESTART_MCUS MCUs.  The arithmetic is integer throughout and written out at the
 * top of csrc/jpeg.hip.h: two runs give equal bytes, and tests/jpeg_reference.py restates it in NumPy.
 *
 * A job names one image where it lies, as a PgrPngJob does: kind PGR_JPEG_GRAY8 (pixel_stride >= 1) or PGR_JPEG_RGB8 (three
 * adjacent bytes R, G, B; pixel_stride >= 3), row_stride >= (width - 1) * pixel_stride + that, width and height 1..16384,
 * quality 1..100, subsampling PGR_JPEG_444 or PGR_JPEG_420 (gray: PGR_JPEG_444 only).
 *
 * Two calls with PNG's contract.  pgr_jpeg_encode transforms, counts, builds the tables and sizes every interval into
 * `workspace` (pgr_jpeg_workspace_bytes: two bytes a coefficient and small records; 0 for n_jobs <= 0 or a job outside the
 * domain; device memory, 16-byte aligned) and writes sizes int64 [n_jobs] (device).  The caller forms offsets int64 [n_jobs + 1]
 * (device), their exclusive sum, and calls pgr_jpeg_emit with the SAME jobs and workspace: file k goes to files[offsets[k] ..
 * offsets[k+1]).  capacity < total is refused on the host and no store leaves files[offsets[k] .. min(offsets[k+1], total))
 * whatever the device-side offsets hold.  Every misuse is PGR_ERR_INVALID_ARGUMENT before any launch. */
#define PGR_JPEG_RESTART_MCUS 16     /* MCUs per restart interval (one workgroup), whatever the width */
#define PGR_JPEG_GRAY8 0
#define PGR_JPEG_RGB8 1
#define PGR_JPEG_444 0
#define PGR_JPEG_420 1
typedef struct PgrJpegJob {
    const void *pixels;
    int32_t width, height;
    int32_t kind;
    int64_t row_stride;
    int32_t pixel_stride;
    int32_t quality;
    int32_t subsampling;
} PgrJpegJob;
size_t pgr_jpeg_workspace_bytes(int32_t n_jobs, const PgrJpegJob *jobs);
int32_t pgr_jpeg_encode(const PgrJpegJob *jobs, int32_t n_jobs, int64_t *sizes, void *workspace, size_t workspace_bytes,
                        void *stream);
int32_t pgr_jpeg_emit(const PgrJpegJob *jobs, int32_t n_jobs, const int64_t *offsets, int64_t total, uint8_t *files,
                      int64_t capacity, const void *workspace, size_t workspace_bytes, void *stream);
/* What no file of that shape exceeds: the longest header (330 bytes gray, 613 colour), 418 bytes a block (1665 bits, every
 * byte stuffed) and 2 bytes a restart interval; 0 outside the domain.  Host only. */
int64_t pgr_jpeg_max_bytes(int32_t width, int32_t height, int32_t kind, int32_t subsampling);
/* The IJG rule: s = 5000 / q below 50, else 200 - 2 q; Q = clamp((base * s + 50) / 100, 1, 255), integer division, on the
 * Annex K tables.  lum and chroma are uint8 [64] in natural (row-major) order.  Host only. */
int32_t pgr_jpeg_quant_tables(int32_t quality, uint8_t *lum, uint8_t *chroma);

/* ---- Undistortion of COLMAP projects (pegasus_amd/undistort.py; csrc/undistort.hip.h) --------------
 * The camera models, their inverse, the remap of images to a pinhole camera and the box pyramid, all in float64; the rule is
 * written out at the top of csrc/undistort.hip.h.  A camera is a COLMAP model id with its parameters in COLMAP's order (host
 * memory): 0 SIMPLE_PINHOLE, 1 PINHOLE, 2 SIMPLE_RADIAL, 3 RADIAL, 4 OPENCV, 5 OPENCV_FISHEYE, 6 FULL_OPENCV; every other id, a
 * parameter that is not finite or a focal length of 0 is PGR_ERR_INVALID_ARGUMENT.  Pixel (x, y) has its centre at (x + 0.5,
 * y + 0.5).
 *
 * pgr_undistort_points: xy double [n,2] (device) image points -> uv double [n,2] normalised points, ok uint8 [n] (may be NULL).
 * A point the inverse does not reach is NaN, NaN with ok 0.  pgr_distort_points is the forward direction, uv -> xy.
 *
 * A PgrUndistortJob names a source and a destination image where they lie (device, uint8, `channels` = 1, 3 or 4 interleaved,
 * row y starts stride bytes behind row y - 1, stride >= width * channels, sides 1..32768), the source camera and the output
 * pinhole fx, fy, cx, cy.  pgr_undistort_images fills every destination pixel: bilinear from the source where the four taps
 * lie inside it, 0 elsewhere.  Jobs are grouped by model and channel count, a launch takes 16 of a group.
 * pgr_image_box_downscale reads only the images of a job: dst = factor x factor integer box means of src, (sum + f f / 2) /
 * (f f); factor is 2, 4 or 8 and dst_width * factor <= src_width, dst_height * factor <= src_height.
 * n = 0 / n_jobs = 0 is PGR_OK without a launch; the tables are read before the call returns. */
typedef struct PgrUndistortJob {
    const void *src;
    int32_t src_width, src_height;
    int32_t channels;
    int32_t model;
    int64_t src_stride;
    void *dst;
    int32_t dst_width, dst_height;
    int64_t dst_stride;
    double params[12];
    double pinhole[4];
} PgrUndistortJob;
int32_t pgr_undistort_points(int32_t model, const double *params, int64_t n, const double *xy, double *uv, uint8_t *ok,
                             void *stream);
int32_t pgr_distort_points(int32_t model, const double *params, int64_t n, const double *uv, double *xy, void *stream);
int32_t pgr_undistort_images(const PgrUndistortJob *jobs, int32_t n_jobs, void *stream);
int32_t pgr_image_box_downscale(const PgrUndistortJob *jobs, int32_t n_jobs, int32_t factor, void *stream);


#ifdef __cplusplus
}
#endif
#endif /* PEGASUS_RASTER_H */
