"""ctypes loader for libstitching_amd.so (C ABI: include/stitching_amd.h).

There is NO CPU fallback: if the HIP library is missing or cannot be loaded the import of
the hot path fails loudly.  Nothing here (or anywhere in stitching_amd) touches oracle/.
"""
import ctypes as C
import os

from .stitching_error import StitchingError

_HERE = os.path.dirname(os.path.abspath(__file__))
# STITCHING_AMD_LIB: another build of the same library (A/B runs of kernel variants on one GPU box: tools/gpu_ab_lib.sh)
LIB_PATH = os.environ.get("STITCHING_AMD_LIB") or os.path.join(_HERE, "libstitching_amd.so")

# constants of include/stitching_amd.h
STX_OK = 0
WARP_PLANE, WARP_AFFINE, WARP_CYLINDRICAL, WARP_SPHERICAL = 0, 1, 2, 3
# cv.PyRotationWarper(name, scale): name -> STX_WARP_* id
WARP_TYPE_IDS = {"plane": 0, "affine": 1, "cylindrical": 2, "spherical": 3, "fisheye": 4, "stereographic": 5,
                 "compressedPlaneA2B1": 6, "compressedPlaneA1.5B1": 7, "compressedPlanePortraitA2B1": 8,
                 "compressedPlanePortraitA1.5B1": 9, "paniniA2B1": 10, "paniniA1.5B1": 11, "paniniPortraitA2B1": 12,
                 "paniniPortraitA1.5B1": 13, "mercator": 14, "transverseMercator": 15}
INTER_NEAREST, INTER_LINEAR = 0, 1
BORDER_CONSTANT, BORDER_REFLECT = 0, 2
BLEND_NO, BLEND_FEATHER, BLEND_MULTIBAND = 0, 1, 2
U8, S16, F32 = 0, 1, 2
TRIG_MODES = {"exact": 0, "glibc": 1, "glibc-nofma": 2}
REMAP_MODES = {"q15": 0, "float": 1, "float-fma": 2}
PYRDOWN_MODES = {"scalar": 0, "simd-v": 1, "simd-hv": 3, "simd-v-fma": 5, "simd-hv-fma": 7}
GAIN_MAP_BOUNDED = 1
# STX_EXPOSURE_*: the cv.detail ExposureCompensator ids of the estimating compensators
EXPOSURE_KINDS = {"gain": 1, "gain_blocks": 2, "channel": 3, "channel_blocks": 4}
# STX_SEAM_*: the seam finders with a device implementation
# STX_EXPOSURE_SOLVER_*: where the gain systems of ExposureEstimator are solved
EXPOSURE_SOLVERS = {"host": 0, "device": 1}
# the device LU of csrc/stx_solve.hip: pivots per blocked step, and the largest system it takes (8 n^2 bytes of device memory: 2 GiB)
LU_NB, LU_MAX_N = 32, 16384
# STX_TRACK_*: the limits of ExposureTracker (lattice stride, images, tile jobs of 32 x 32 lattice points)
TRACK_STRIDE_MAX, TRACK_IMAGES_MAX, TRACK_TILES_MAX = 64, 1024, 65536
SEAM_KINDS = {"no": 0, "voronoi": 1}
# STX_COLOR_SEAM_MAX_*: the limits of ColorSeamEstimator (seam length: u32 accumulators; cross extent: accumulator rows in LDS)
COLOR_SEAM_MAX_LENGTH, COLOR_SEAM_MAX_CROSS = 16384, 4096
# STX_FEATURES_MAX_*: the limits of FeatureEstimator (image side: (response, y, x) is one 64-bit key; levels; features per image)
FEATURES_MAX_SIDE, FEATURES_MAX_LEVELS, FEATURES_MAX_FEATURES = 32767, 16, 65536
# STX_MATCH_MAX_*: the limits of MatchEstimator (features per image: 16-bit train indices; RANSAC hypotheses per pair)
MATCH_MAX_FEATURES, MATCH_MAX_ITERS = 65536, 4096
# STX_MATCH_MODEL_*: the geometric model of MatchEstimator's RANSAC
MATCH_MODELS = {"homography": 0, "affine_partial": 1, "affine_full": 2}
# STX_RAY_MAX_*: the limits of CameraSolver's ray adjustment (cameras; matches on an edge: the union of both directions)
RAY_MAX_CAMERAS, RAY_MAX_MATCHES = 1024, 131072
CONTRIB_U8_BINARY = 1
STRIP_MASK_BITS = 2

# STX_INGEST_*: the pixel formats, matrices and ranges of stx_ingest, and the largest side of a frame
INGEST_FORMATS = {None: 0, "bgr": 1, "rgb": 2, "bgra": 3, "rgba": 4, "gray": 5, "nv12": 6, "i420": 7}
INGEST_MATRICES = {"bt601": 0, "bt709": 1}
INGEST_RANGES = {"limited": 0, "full": 1}
INGEST_MAX_SIDE = 32768
# STX_LENS_CELL, STX_RECTIFY_*: the spacing of a lens map's nodes, the borders of stx_rectify and the largest side of a frame
LENS_CELL = 16
RECTIFY_BORDERS = {"constant": 0, "replicate": 1}
RECTIFY_MAX_SIDE = 16384


class ForeignFrame(C.Structure):
    """stx_foreign_frame: up to three planes of foreign device memory, pitches in bytes."""
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_longlong * 3), ("w", C.c_int), ("h", C.c_int), ("channels", C.c_int),
                ("elem", C.c_int), ("format", C.c_int)]


class EmitItem(C.Structure):
    """stx_emit_item: a source image, an optional alpha image, a format and an optional target of up to three planes."""
    _fields_ = [("src", C.c_void_p), ("alpha", C.c_void_p), ("format", C.c_int), ("has_target", C.c_int), ("plane", C.c_void_p * 3),
                ("pitch", C.c_longlong * 3)]


WARP_FRESH_ROIS = 1

_i, _f, _d, _u, _z = C.c_int, C.c_float, C.c_double, C.c_uint, C.c_size_t
_vp, _vpp = C.c_void_p, C.POINTER(C.c_void_p)
_fp, _ip, _dp, _llp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_longlong)
_ubp, _zp = C.POINTER(C.c_ubyte), C.POINTER(C.c_size_t)

# every export of include/stitching_amd.h and include/stitching_amd_debug.h, declared once: name -> argtypes ([]: takes nothing).
# All return int but stx_last_error (const char*).
PROTOTYPES = {
    "stx_version": [],
    "stx_last_error": [],
    "stx_set_trig_mode": [_i],
    "stx_get_trig_mode": [],
    "stx_set_remap_mode": [_i],
    "stx_get_remap_mode": [],
    "stx_set_pyrdown_mode": [_i, _i],
    "stx_get_pyrdown_mode": [_ip],
    "stx_device_count": [_ip],
    "stx_ctx_create": [_i, _vpp],
    "stx_ctx_destroy": [_vp],
    "stx_ctx_sync": [_vp],
    "stx_host_alloc": [_z, _vpp],
    "stx_host_free": [_vp],
    "stx_buf_from_host": [_vp, _vp, _z, _i, _i, _i, _i, _vpp],
    "stx_buf_from_host_async": [_vp, _vp, _z, _i, _i, _i, _i, _vpp],
    "stx_buf_alloc": [_vp, _i, _i, _i, _i, _vpp],
    "stx_buf_to_host": [_vp, _vp, _z],
    "stx_buf_to_host_async": [_vp, _vp, _z],
    "stx_buf_view": [_vp, _i, _i, _i, _i, _vpp],
    "stx_buf_with_validity": [_vp, _vp, _vpp],
    "stx_buf_validity": [_vp, _vpp],
    "stx_buf_info": [_vp, C.POINTER(C.c_int64)],
    "stx_buf_device_ptr": [_vp, _vpp],
    "stx_buf_free": [_vp],
    "stx_warp_roi": [_vp, _i, _f, _fp, _fp, _i, _i, _ip],
    "stx_warp_rois": [_vp, _i, _f, _i, _fp, _fp, _ip, _ip],
    "stx_warp": [_vp, _i, _f, _fp, _fp, _vp, _i, _i, _vpp, _ip],
    "stx_warp_image_and_mask": [_vp, _i, _f, _fp, _fp, _vp, _vpp, _vpp, _ip],
    "stx_warp_batch": [_vp, _i, _f, _i, _fp, _fp, _vpp, _ip, _vpp, _ip, _i, _vpp, _vpp, _ip, _vpp],
    "stx_warp_tables_free": [_vp],
    "stx_warp_mask": [_vp, _i, _f, _fp, _fp, _i, _i, _vpp, _ip],
    "stx_gain_apply": [_vp, _vp, _fp],
    "stx_block_gain_apply_batch": [_vp, _i, _vpp, _vpp, _ip, _ip],
    "stx_resize_linear_exact": [_vp, _vp, _i, _i, _vpp],
    "stx_resize_linear_exact_batch": [_vp, _i, _vpp, _ip, _vpp],
    "stx_mask_shrink_batch": [_vp, _i, _vpp, _ip, _vpp],
    "stx_seam_mask_resize": [_vp, _vp, _vp, _vpp],
    "stx_seam_mask_resize_batch": [_vp, _i, _vpp, _vpp, _vpp],
    "stx_seam_mask_resize_batch_sub": [_vp, _i, _vpp, _vpp, _ip, _vpp],
    "stx_timelapse_frame": [_vp, _vp, _i, _i, _ip, _vpp],
    "stx_result_roi": [_i, _ip, _ip, _ip],
    "stx_blend_create": [_vp, _i, _i, _f, _ip, _vpp],
    "stx_blend_num_bands": [_vp, _ip],
    "stx_blend_feed": [_vp, _vp, _vp, _i, _i],
    "stx_blend_finish": [_vp, _vpp, _vpp],
    "stx_blend_finish_ex": [_vp, _vpp, _vpp, _vpp],
    "stx_blend_destroy": [_vp],
    "stx_blend_keep_weights": [_vp, _vpp],
    "stx_blend_use_weights": [_vp, _vp, _ip],
    "stx_mb_weights_free": [_vp],
    "stx_blend_set_band": [_vp, _i, _i],
    "stx_blend_feed_ex": [_vp, _vp, _vp, _i, _i, _i],
    "stx_blend_contrib_rect": [_vp, _i, _i, _i, _i, _i, _i, _ip, _zp],
    "stx_blend_export_contrib": [_vp, _i, _i, _i, _vpp, _ip],
    "stx_blend_export_contribs": [_vp, _i, _ip, _ip, _ip, _vpp, _ip],
    "stx_blend_build": [_vp],
    "stx_blend_feed_contrib_ex": [_vp, _i, _ip, _vp, _i],
    "stx_buf_flags": [_vp, _ip],
    "stx_strip_rect": [_vp, _i, _i, _i, _i, _i, _i, _ip, _zp],
    "stx_view_rect": [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _ip],
    "stx_strip_pack": [_vp, _vp, _vp, _i, _i, _vpp],
    "stx_strip_pack_batch_ex": [_vp, _i, _vpp, _vpp, _ip, _ip, _i, _vpp],
    "stx_strip_bytes": [_i, _i, _i, _zp],
    "stx_strip_unpack": [_vp, _i, _i, _i, _vpp, _vpp],
    "stx_blend_feed_strips": [_vp, _i, _vpp, _ip, _ip, _ip, _ip, _ip, _i],
    "stx_comm_unique_id": [_ubp],
    "stx_comm_create": [_vp, _i, _i, _ubp, _vpp],
    "stx_comm_exchange_begin_on": [_vp, _vp, _i, _ip, _ip, _vpp, _zp],
    "stx_comm_exchange_end_on": [_vp, _vp],
    "stx_comm_info": [_vp, _ip],
    "stx_comm_destroy": [_vp],
    "stx_prof_enable": [_vp, _i],
    "stx_prof_reset": [_vp],
    "stx_prof_count": [_vp, _ip],
    "stx_prof_get": [_vp, _i, C.c_char_p, _i, C.POINTER(C.c_int64), _dp, _dp],
    "stx_mark": [_vp, _i],
    "stx_mark_elapsed_ms": [_vp, _i, _i, _dp],
    "stx_exposure_stats": [_vp, _i, _i, _vpp, _vpp, _ip, _i, _llp, _ip, _llp, _dp],
    "stx_exposure_solve": [_i, _i, _ip, _dp, _ubp, _dp],
    "stx_set_exposure_solver": [_i],
    "stx_get_exposure_solver": [],
    "stx_exposure_feed_ex": [_vp, _i, _i, _vpp, _vpp, _ip, _i, _i, _i, _dp, _llp, _dp],
    "stx_exposure_solve_device": [_vp, _i, _i, _ip, _dp, _ubp, _dp, _dp],
    "stx_lu_solve_device": [_vp, _i, _dp, _dp, _dp, _dp],
    "stx_exposure_track_create": [_vp, _i, _ip, _vpp, _i, _vpp],
    "stx_exposure_track_pairs": [_vp, _ip, _ip, _llp],
    "stx_exposure_track_measure": [_vp, _vpp],
    "stx_exposure_track_collect": [_vp, _llp],
    "stx_exposure_track_info": [_vp, _dp],
    "stx_exposure_track_free": [_vp],
    "stx_gain_maps_scale": [_vp, _i, _vpp, _fp, _i, _vpp],
    "stx_seam_find": [_vp, _i, _i, _ip, _ip, _vpp, _vpp, _dp],
    "stx_seam_schedule": [_i, _ip, _ip, _ip, _ip, _ip],
    "stx_color_seam_find": [_vp, _i, _ip, _ip, _vpp, _vpp, _vpp, _dp],
    "stx_crop_lir": [_vp, _vp, _ip, _ip, _dp],
    "stx_features_detect": [_vp, _i, _vpp, _vpp, _i, _i, _i, _ip, _ip, _ip, _ip, C.POINTER(C.c_byte), _ip, _ip, _llp, _ubp, _dp],
    "stx_match_features": [_vp, _i, _vpp, _ip, _vpp, _ip, _i, _i, _i, _d, _u, _ip, _ip, _ubp, _ip, _dp, _dp],
    "stx_match_features_model": [_vp, _i, _vpp, _ip, _vpp, _ip, _i, _i, _i, _d, _u, _i, _ip, _ip, _ubp, _ip, _dp, _dp],
    "stx_ray_problem_create": [_vp, _i, _ip, _llp, _dp, _vpp],
    "stx_ray_problem_eval": [_vp, _i, _dp, _dp, _dp],
    "stx_affine_problem_eval": [_vp, _i, _dp, _dp, _dp],
    "stx_reproj_problem_eval": [_vp, _i, _dp, _dp, _dp],
    "stx_ray_problem_free": [_vp],
    "stx_ingest": [_vp, _i, C.POINTER(ForeignFrame), _i, _i, _vp, _i, _vpp],
    "stx_emit": [_vp, _i, C.POINTER(EmitItem), _i, _i, _vp, _i, _vpp],
    "stx_lens_map_create": [_vp, _i, _i, _i, _i, _i, _i, _ip, _vpp],
    "stx_lens_map_free": [_vp],
    "stx_rectify": [_vp, _i, _vpp, _vpp, _i, _i, _vpp, _vpp],
    "stx_warp_lens_batch": [_vp, _i, _f, _i, _fp, _fp, _vpp, _vpp, _ip, _vpp, _ip, _vpp],
    # include/stitching_amd_debug.h: test hooks, never called by the package's classes
    "stx_debug_warp_maps": [_vp, _i, _f, _fp, _fp, _i, _i, _i, _ip, _vpp, _vpp, _ip],
    "stx_debug_feather_dist_cap": [],
    "stx_debug_blend_replayed": [_vp, _ip],
    "stx_debug_warp_table_launches": [_vp, _ip],
    "stx_debug_blend_uploads": [_vp, _ip],
    "stx_debug_blend_mask_stored": [_vp, _ip],
    "stx_debug_seam_resize_paths": [_vp, _ip],
}
EXPORTS = tuple(PROTOTYPES)

_lib = None


def build_hint():
    return "build it with `make -C stitching_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`"


def lib():
    """Load the shared library once and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: the HIP back end is not built ({build_hint()}). "
                          "stitching_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, argtypes in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.argtypes = argtypes
        fn.restype = C.c_char_p if name == "stx_last_error" else C.c_int
    _lib = L
    return L


def check(rc):
    """C status -> reference error convention (StitchingError; stitching/stitching_error.py:1-2)."""
    if rc != STX_OK:
        msg = lib().stx_last_error()
        raise StitchingError(f"stitching_amd [{rc}]: {msg.decode(errors='replace') if msg else 'unknown error'}")
