"""ctypes binding of libpegasus_raster.so (include/pegasus_raster.h).

There is NO fallback: if the library is missing or fails to load, every rasterizer entry point
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported here.)
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import os

# PGR_LIB: an alternative build of the library (stats / timing / variant builds of the measurement scripts load theirs
# from build_variants/ instead of overwriting the product .so)
LIB_PATH = Path(os.environ.get("PGR_LIB") or Path(__file__).resolve().parent / "csrc" / "libpegasus_raster.so")

PGR_ABI_VERSION = 4          # include/pegasus_raster.h PGR_ABI_VERSION
PGR_OK = 0
PGR_ERR_INVALID_ARGUMENT = -1
PGR_ERR_WORKSPACE_TOO_SMALL = -2
PGR_ERR_INSTANCE_OVERFLOW = -3
PGR_ERR_LAUNCH_FAILURE = -4
PGR_NUM_STAGES = 5
STAGE_NAMES = ("preprocess", "bin_count", "bin_scatter", "tile_sort", "composite")


class PgrScene(C.Structure):
    _fields_ = [
        ("n", C.c_int32),
        ("means3d", C.c_void_p), ("opacities", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p),
        ("cov3d_precomp", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
        ("sh_degree", C.c_int32), ("sh_stride", C.c_int32), ("scale_modifier", C.c_float),
        ("tie_index", C.c_void_p), ("tie_inv", C.c_void_p), ("shs_rest", C.c_void_p),
    ]


class PgrCamera(C.Structure):
    _fields_ = [
        ("image_width", C.c_int32), ("image_height", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
        ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p), ("bg", C.c_void_p),
        ("depth_mode", C.c_int32),
    ]


class PgrOutputs(C.Structure):
    _fields_ = [("color", C.c_void_p), ("depth", C.c_void_p), ("radii", C.c_void_p), ("final_T", C.c_void_p),
                ("n_contrib", C.c_void_p), ("sem_color", C.c_void_p), ("sem_depth", C.c_void_p),
                ("sem_masks", C.c_void_p), ("record", C.c_void_p)]


class PgrSemantic(C.Structure):
    _fields_ = [("object_id", C.c_void_p), ("colors", C.c_void_p), ("n_env", C.c_int32), ("k_objects", C.c_int32),
                ("object_id_u8", C.c_void_p), ("mask_colors", C.c_void_p), ("mask_threshold", C.c_float)]


class PgrLayers(C.Structure):
    _fields_ = [("layer_id", C.c_void_p), ("n_layers", C.c_int32), ("mask_colors", C.c_void_p),
                ("mask_threshold", C.c_float)]


class PgrRecordLayout(C.Structure):
    _fields_ = [("off_rgb", C.c_int64), ("off_depth", C.c_int64), ("off_masks", C.c_int64), ("bytes", C.c_int64)]


PGR_DEPTH_EXPECTED = 0
PGR_DEPTH_NORMALIZED = 1


class PgrPosedObjects(C.Structure):
    _fields_ = [("object_id", C.c_void_p), ("poses", C.c_void_p), ("k_objects", C.c_int32)]


PGR_POSE_STRIDE = 20


class PgrObjectPose(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("center", C.c_float * 3), ("q", C.c_float * 4),
                ("D1", C.c_float * 9), ("D2", C.c_float * 25), ("D3", C.c_float * 49)]


class PgrPoseJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p), ("n", C.c_int32),
                ("kind", C.c_int32), ("n_rest", C.c_int32), ("about_origin", C.c_int32), ("R_row_stride", C.c_int32),
                ("t_stride", C.c_int32)]


PGR_POSE_XYZ, PGR_POSE_ROT, PGR_POSE_SH = 0, 1, 2


class PgrGradOutputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("means2d", "means3d", "opacities", "colors", "shs", "cov3d", "scales",
                                          "rotations")]


class PgrBackwardView(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("grad_color", "grad_depth", "final_T", "n_contrib", "radii")]


class PgrCameraGrad(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("viewmatrix", "projmatrix", "campos")]


class PgrForwardCall(C.Structure):
    """One pgr_forward call.  The pointer fields keep what is assigned to them alive as long as the struct."""
    _fields_ = [("scene", C.POINTER(PgrScene)), ("n_views", C.c_int32), ("cameras", C.POINTER(PgrCamera)),
                ("outs", C.POINTER(PgrOutputs)), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("max_instances_per_view", C.c_int64), ("semantic", C.POINTER(PgrSemantic)),
                ("posed", C.POINTER(PgrPosedObjects)), ("layers", C.POINTER(PgrLayers)), ("host_scratch", C.c_void_p),
                ("host_scratch_bytes", C.c_size_t), ("num_instances", C.POINTER(C.c_int64)),
                ("stage_ms", C.POINTER(C.c_float)), ("status_event", C.c_void_p)]


class PgrBackwardCall(C.Structure):
    """One pgr_backward call."""
    _fields_ = [("scene", C.POINTER(PgrScene)), ("n_views", C.c_int32), ("cameras", C.POINTER(PgrCamera)),
                ("views", C.POINTER(PgrBackwardView)), ("grad_alpha", C.POINTER(C.c_void_p)), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("max_instances_per_view", C.c_int64), ("grads", C.POINTER(PgrGradOutputs)),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("camera_grads", C.POINTER(PgrCameraGrad)),
                ("camera_scratch", C.c_void_p), ("camera_scratch_bytes", C.c_size_t)]


class PgrWorkspaceView(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("splats", "rects", "gauss_sorted", "ranges", "num_instances")]


class PgrAdamGroup(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("n", C.c_int64), ("lr", C.c_double), ("step", C.c_int64)]


PGR_ADAM_MAX_GROUPS = 16


class PgrGrid(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_float * 3), ("voxel", C.c_float)]


class PgrMeshJob(C.Structure):
    _fields_ = [("vertex_first", C.c_int32), ("vertex_count", C.c_int32), ("face_first", C.c_int32), ("face_count", C.c_int32),
                ("R", C.c_float * 9), ("t", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("slot", C.c_int32)]


class PgrMeshShade(C.Structure):
    _fields_ = [("normals", C.c_void_p), ("colors", C.c_void_p), ("surf_colors", C.POINTER(C.c_float)),
                ("light", C.c_float * 3), ("ambient", C.c_float), ("bg", C.c_float * 3), ("depth", C.c_void_p),
                ("face_id", C.c_void_p), ("job_id", C.c_void_p), ("xyz", C.c_void_p), ("normal", C.c_void_p),
                ("rgb", C.c_void_p)]


PGR_MESH_VISIBILITY_MAX_JOBS = 1024      # include/pegasus_raster.h


class PgrMeshTexture(C.Structure):
    _fields_ = [("offset", C.c_int64), ("width", C.c_int32), ("height", C.c_int32)]


class PgrMeshTextures(C.Structure):
    _fields_ = [("corner_uv", C.c_void_p), ("texels", C.c_void_p), ("texel_bytes", C.c_int64), ("n_textures", C.c_int32),
                ("textures", C.POINTER(PgrMeshTexture)), ("job_texture", C.POINTER(C.c_int32)), ("filter", C.c_int32),
                ("uv", C.c_void_p)]


PGR_TEXTURE_NEAREST, PGR_TEXTURE_BILINEAR = 0, 1


class PgrGtInfoJob(C.Structure):
    _fields_ = [("slot", C.c_int32), ("frame", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double)]


PGR_GT_INFO_STATS = 11
# include/pegasus_raster.h: jobs per launch and workgroups per job of pgr_bop_gt_info (tests/test_gt_info_host.py holds them
# against it)
PGR_GT_INFO_JOBS_PER_LAUNCH, PGR_GT_INFO_BLOCKS_X = 64, 512


class PgrPoseErrorJob(C.Structure):
    _fields_ = [("vertex_first", C.c_int32), ("vertex_count", C.c_int32), ("sym_first", C.c_int32), ("sym_count", C.c_int32),
                ("R_est", C.c_double * 9), ("t_est", C.c_double * 3), ("R_gt", C.c_double * 9), ("t_gt", C.c_double * 3),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


PGR_POSE_ERRORS = 6          # mssd, mspd, add, proj, re, te
PGR_POSE_SYM_CHUNK = 4       # include/pegasus_raster.h PGR_POSE_SYM_CHUNK


class PgrObbJob(C.Structure):
    _fields_ = [("point_first", C.c_int32), ("point_count", C.c_int32), ("tri_first", C.c_int32), ("tri_count", C.c_int32)]


# include/pegasus_raster.h: the tiles of the box and diameter kernels (tests/obb_cases.py is built around them)
PGR_OBB_TRI_TILE, PGR_OBB_POINT_TILE, PGR_DIAMETER_TILE = 256, 512, 256
# include/pegasus_raster.h: the shapes at which the mask kernels change path (tests/test_coco_host.py holds them against it)
PGR_RLE_WORD_ROWS, PGR_RLE_TILE_COLS, PGR_RLE_BLOCK_ROWS = 32, 256, 128
PGR_RLE_DECODE_CHUNK, PGR_RLE_DECODE_MIN_SLICE, PGR_RLE_DECODE_MAX_SLICES, PGR_MASK_OVERLAP_CHUNK = 256, 16384, 64, 16384
PGR_MASK_STATS = 6           # n_counts, area, x_min, y_min, x_max, y_max
# include/pegasus_raster.h: the shapes at which the COCO score kernels change path, and their limits
PGR_COCO_CHUNK, PGR_COCO_LDS_RUNS, PGR_COCO_MAX_LANES, PGR_COCO_MAX_MAXDETS = 256, 4096, 64, 8
# include/pegasus_raster.h: the sums of pgr_plane_inliers and the points of one workgroup of pgr_plane_score
PGR_PLANE_SUMS, PGR_PLANE_TILE = 12, 2048


class PgrSdfBody(C.Structure):
    _fields_ = [("grid", PgrGrid), ("sdf", C.c_void_p), ("shell", C.c_void_p), ("n_shell", C.c_int32), ("R", C.c_float * 9),
                ("t", C.c_float * 3)]


class PgrSweepJob(C.Structure):
    _fields_ = [("mover", C.c_int32), ("target", C.c_int32), ("dir", C.c_float * 3), ("plane", C.c_float * 4)]


# include/pegasus_raster.h: the faces of one pass of pgr_mesh_sdf through LDS (tests/collision_cases.py is built around it) and
# the target index that names the plane
PGR_SDF_FACE_TILE, PGR_SWEEP_PLANE = 256, -1


class PgrRigidType(C.Structure):
    _fields_ = [("grid", PgrGrid), ("sdf", C.c_void_p), ("shell", C.c_void_p), ("n_shell", C.c_int32), ("mass", C.c_float),
                ("com", C.c_float * 3), ("inv_inertia", C.c_float * 9), ("friction", C.c_float), ("radius", C.c_float)]


class PgrRigidParams(C.Structure):
    _fields_ = [("h", C.c_float), ("gravity", C.c_float * 3), ("plane", C.c_float * 4), ("plane_friction", C.c_float),
                ("lin_damp", C.c_float), ("ang_damp", C.c_float), ("iterations", C.c_int32), ("beta", C.c_float),
                ("slop", C.c_float), ("margin", C.c_float), ("v_sleep", C.c_float), ("w_sleep", C.c_float),
                ("sleep_steps", C.c_int32)]


class PgrRigidGround(C.Structure):
    _fields_ = [("grid", PgrGrid), ("sdf", C.c_void_p), ("friction", C.c_float)]


# include/pegasus_raster.h: the slots of a world, the types of a table, the words of a pair, the floats of a body's state
PGR_RIGID_MAX_BODIES, PGR_RIGID_MAX_TYPES, PGR_RIGID_WORDS, PGR_RIGID_STATE = 8, 16, 7, 13


class PgrCocoGroup(C.Structure):
    _fields_ = [("dt_begin", C.c_int32), ("dt_count", C.c_int32), ("gt_begin", C.c_int32), ("gt_count", C.c_int32),
                ("iou_offset", C.c_int64)]


class PgrPngJob(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("kind", C.c_int32),
                ("row_stride", C.c_int64), ("pixel_stride", C.c_int32), ("scale", C.c_int32)]


# include/pegasus_raster.h: the raw bytes of one deflate segment, the positions of one hash sub-block, the image kinds
PGR_PNG_SEGMENT_BYTES, PGR_PNG_SUBBLOCK = 8192, 512
PGR_PNG_GRAY8, PGR_PNG_RGB8, PGR_PNG_GRAY16 = 0, 1, 2


class PgrJpegJob(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("kind", C.c_int32),
                ("row_stride", C.c_int64), ("pixel_stride", C.c_int32), ("quality", C.c_int32), ("subsampling", C.c_int32)]


# include/pegasus_raster.h: the MCUs of one restart interval, the image kinds, the chroma subsamplings
PGR_JPEG_RESTART_MCUS = 16
PGR_JPEG_GRAY8, PGR_JPEG_RGB8 = 0, 1
PGR_JPEG_444, PGR_JPEG_420 = 0, 1


class PgrUndistortJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_width", C.c_int32), ("src_height", C.c_int32), ("channels", C.c_int32),
                ("model", C.c_int32), ("src_stride", C.c_int64), ("dst", C.c_void_p), ("dst_width", C.c_int32),
                ("dst_height", C.c_int32), ("dst_stride", C.c_int64), ("params", C.c_double * 12), ("pinhole", C.c_double * 4)]


# every symbol include/pegasus_raster.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "pgr_abi_version": (C.c_int32, []),
    "pgr_version": (C.c_char_p, []),
    "pgr_status_string": (C.c_char_p, [C.c_int32]),
    "pgr_last_hip_error": (C.c_char_p, []),
    "pgr_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "pgr_forward": (C.c_int32, [C.POINTER(PgrForwardCall), C.c_void_p]),
    "pgr_batch_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "pgr_host_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_batch_status": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    "pgr_scene_cache_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_scene_prepare": (C.c_int32, [C.POINTER(PgrScene), C.POINTER(PgrSemantic), C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]),
    "pgr_layers_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "pgr_frame_record_layout": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(PgrRecordLayout)]),
    "pgr_pack_records": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_int64, C.c_void_p]),
    "pgr_workspace_view": (C.c_int32, [C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                       C.c_int32, C.c_int32, C.POINTER(PgrWorkspaceView)]),
    "pgr_workspace_block_visibility": (C.c_int32, [C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                                   C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "pgr_backward": (C.c_int32, [C.POINTER(PgrBackwardCall), C.c_void_p]),
    "pgr_backward_batch_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "pgr_camera_grad_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "pgr_compose_object": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                       C.POINTER(PgrObjectPose), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p]),
    "pgr_clock_probe": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "pgr_pose_objects_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_pose_objects": (C.c_int32, [C.c_int32, C.POINTER(PgrPoseJob), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "pgr_block_visibility_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "pgr_block_visibility": (C.c_int32, [C.POINTER(PgrScene), C.c_int32, C.POINTER(PgrCamera), C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_void_p]),
    "pgr_mark_visible": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_color_masks": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                    C.c_void_p, C.c_void_p]),
    "pgr_knn_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_knn_mean_dist2": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_radius_count_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_radius_count": (C.c_int32, [C.c_int32, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "pgr_nn_grid_build_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_nn_grid_build": (C.c_int32, [C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_nn_source_order_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_nn_source_order": (C.c_int32, [C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p]),
    "pgr_nn_correspond": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_double,
                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_icp_sums_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_icp_sums": (C.c_int32, [C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_radius_normals_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_radius_normals": (C.c_int32, [C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p]),
    "pgr_plane_hypotheses": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_plane_score_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "pgr_plane_score": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_plane_inliers_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_plane_inliers": (C.c_int32, [C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_quantize_frame": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "pgr_pack_frames": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_image_loss_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "pgr_image_loss": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_image_loss_masked_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "pgr_image_loss_masked": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_adam_step": (C.c_int32, [C.POINTER(PgrAdamGroup), C.c_int32, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "pgr_densify_stats": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "pgr_tsdf_integrate": (C.c_int32, [C.POINTER(PgrGrid), C.c_int32, C.POINTER(PgrCamera), C.c_void_p, C.c_void_p,
                                       C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "pgr_sdf_from_tsdf_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "pgr_sdf_from_tsdf": (C.c_int32, [C.POINTER(PgrGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_march_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "pgr_march_count": (C.c_int32, [C.POINTER(PgrGrid), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pgr_march_emit": (C.c_int32, [C.POINTER(PgrGrid), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "pgr_mesh_depth_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(PgrMeshJob)]),
    "pgr_mesh_depth": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(PgrMeshJob), C.c_int32,
                                   C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    "pgr_mesh_visibility_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(PgrMeshJob)]),
    "pgr_mesh_visibility": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(PgrMeshJob),
                                        C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p]),
    "pgr_mesh_shade_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(PgrMeshJob)]),
    "pgr_mesh_shade": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(PgrMeshJob), C.c_int32,
                                   C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.POINTER(PgrMeshShade), C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    "pgr_mesh_shade_textured_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(PgrMeshJob)]),
    "pgr_mesh_shade_textured": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(PgrMeshJob),
                                            C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.POINTER(PgrMeshShade),
                                            C.POINTER(PgrMeshTextures), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_bop_gt_info": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                    C.c_int32, C.c_int32, C.c_int32, C.POINTER(PgrGtInfoJob), C.c_float, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_pose_errors": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(PgrPoseErrorJob),
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_pose_adi_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(PgrPoseErrorJob)]),
    "pgr_pose_adi": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(PgrPoseErrorJob), C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    "pgr_obb_candidates_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(PgrObbJob)]),
    "pgr_obb_candidates": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                       C.POINTER(PgrObbJob), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p]),
    "pgr_point_diameter_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(PgrObbJob)]),
    "pgr_point_diameter": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(PgrObbJob), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_mask_rle_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "pgr_mask_rle_count": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p]),
    "pgr_mask_rle_emit": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_mask_rle_decode": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "pgr_mask_overlap": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_rle_iou_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int64]),
    "pgr_rle_iou": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                C.c_void_p, C.c_int32, C.c_int32, C.POINTER(PgrCocoGroup), C.c_int32, C.c_int64, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_box_iou_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_box_iou": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(PgrCocoGroup), C.c_int32,
                                C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_coco_match_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "pgr_coco_match": (C.c_int32, [C.POINTER(PgrCocoGroup), C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int32,
                                   C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_coco_accumulate_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "pgr_coco_accumulate": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "pgr_mesh_cluster_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "pgr_mesh_cluster_count": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                           C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pgr_mesh_cluster_emit": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                          C.c_double, C.c_int32, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_mesh_vertex_normals_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "pgr_mesh_vertex_normals": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p]),
    "pgr_mesh_vertex_colors": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(PgrCamera), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float),
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_mesh_atlas_points": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_mesh_atlas_pack": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_uint8), C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_mesh_sdf": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(PgrGrid), C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "pgr_sdf_sample": (C.c_int32, [C.POINTER(PgrGrid), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_sdf_sweep": (C.c_int32, [C.c_int32, C.POINTER(PgrSdfBody), C.c_int32, C.POINTER(PgrSweepJob), C.c_float, C.c_float,
                                  C.c_int32, C.c_void_p, C.c_void_p]),
    "pgr_rigid_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "pgr_rigid_contacts": (C.c_int32, [C.POINTER(PgrRigidParams), C.c_int32, C.POINTER(PgrRigidType), C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_rigid_simulate": (C.c_int32, [C.POINTER(PgrRigidParams), C.c_int32, C.POINTER(PgrRigidType), C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_rigid_contacts_ground": (C.c_int32, [C.POINTER(PgrRigidParams), C.POINTER(PgrRigidGround), C.c_int32,
                                              C.POINTER(PgrRigidType), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_rigid_simulate_ground": (C.c_int32, [C.POINTER(PgrRigidParams), C.POINTER(PgrRigidGround), C.c_int32,
                                              C.POINTER(PgrRigidType), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_png_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(PgrPngJob)]),
    "pgr_png_encode": (C.c_int32, [C.POINTER(PgrPngJob), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_png_emit": (C.c_int32, [C.POINTER(PgrPngJob), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    "pgr_png_max_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "pgr_png_code_lengths": (C.c_int32, [C.POINTER(C.c_uint32), C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "pgr_jpeg_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(PgrJpegJob)]),
    "pgr_jpeg_encode": (C.c_int32, [C.POINTER(PgrJpegJob), C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pgr_jpeg_emit": (C.c_int32, [C.POINTER(PgrJpegJob), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    "pgr_jpeg_max_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "pgr_jpeg_quant_tables": (C.c_int32, [C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "pgr_undistort_points": (C.c_int32, [C.c_int32, C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "pgr_distort_points": (C.c_int32, [C.c_int32, C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgr_undistort_images": (C.c_int32, [C.POINTER(PgrUndistortJob), C.c_int32, C.c_void_p]),
    "pgr_image_box_downscale": (C.c_int32, [C.POINTER(PgrUndistortJob), C.c_int32, C.c_int32, C.c_void_p]),
}

_lib = None


class RasterizerLibraryError(RuntimeError):
    pass


def lib():
    """Loads the HIP library (once).  Raises RasterizerLibraryError if it is not built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RasterizerLibraryError(
                f"{LIB_PATH} is missing: build it with `python -m pegasus_amd.build` "
                "(there is no CPU fallback for the rasterizer)")
        # torch FIRST: its wheel bundles its own libamdhip64 / libhsa-runtime64, and the library's DT_NEEDED entries name the
        # same sonames -- loaded behind torch it binds to torch's runtime (one HIP runtime in the process, the one that owns
        # the tensors it is handed); loaded in front of it the system's runtime comes in as a SECOND one and every HIP call
        # of the library fails with "no ROCm-capable device is detected" (build() followed by smoke() in one process did)
        import torch  # noqa: F401
        try:
            handle = C.CDLL(str(LIB_PATH))
        except OSError as e:
            raise RasterizerLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        # the ABI version first, binding only that symbol: a stale or variant build (PGR_LIB) then fails with the
        # version message, not with an AttributeError on whichever newer entry point it lacks
        try:
            ver_fn = handle.pgr_abi_version
        except AttributeError as e:
            raise RasterizerLibraryError(f"{LIB_PATH} does not export pgr_abi_version: not a pegasus_raster library") from e
        ver_fn.restype, ver_fn.argtypes = C.c_int32, []
        if ver_fn() != PGR_ABI_VERSION:
            raise RasterizerLibraryError(f"{LIB_PATH}: ABI version {ver_fn()} but this package binds version "
                                         f"{PGR_ABI_VERSION}; rebuild with `python -m pegasus_amd.build`")
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise RasterizerLibraryError(f"{LIB_PATH} does not export {name} (include/pegasus_raster.h)") from e
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def ptr(t):
    """A tensor's address as the pointer argument the ABI takes; None (NULL) for None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device) -> C.c_void_p:
    """torch's CURRENT stream on ``device`` as the stream argument the ABI takes.  Ask at every call, never keep the answer:
    callers switch streams between calls."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def enqueue(name: str, device, *args) -> int:
    """THE way the package calls an entry point that takes a stream: with ``device`` current, on torch's current stream of
    ``device`` at the time of the call, which goes behind ``args``.  Returns the raw status: callers that handle one
    themselves (instance overflow) use this, all others ``call``."""
    import torch
    with torch.cuda.device(device):
        return getattr(lib(), name)(*args, stream_ptr(device))


def call(name: str, device, *args):
    """``enqueue`` whose status other than PGR_OK raises, naming the entry."""
    check(enqueue(name, device, *args), name)


def workspace(entry: str, device, *size_args):
    """THE way the package sizes and allocates the workspace of ``entry``: a fresh uint8 tensor on ``device`` of exactly
    ``<entry>_workspace_bytes(*size_args)`` bytes.  A size of 0 is that function refusing its arguments and raises.  (Callers
    with a policy of their own -- a cached buffer, slack bytes, a memory estimate -- ask the size function themselves.)"""
    import torch
    nbytes = int(getattr(lib(), f"{entry}_workspace_bytes")(*size_args))
    if nbytes == 0:
        raise ValueError(f"{entry}_workspace_bytes rejected its arguments: {size_args!r}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def check(status: int, what: str = "pegasus_raster"):
    if status == PGR_OK:
        return
    L = lib()
    msg = f"{what}: {L.pgr_status_string(status).decode()} ({status})"
    if status == PGR_ERR_LAUNCH_FAILURE:
        msg += f" [{L.pgr_last_hip_error().decode()}]"
    if status == PGR_ERR_INVALID_ARGUMENT:
        raise ValueError(msg)
    raise RuntimeError(msg)
