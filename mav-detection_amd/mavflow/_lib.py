"""ctypes binding of libmavflow.so (include/mavflow.h).  No CPU fallback: if the library or a GPU is missing the
product path raises."""
from __future__ import annotations

import ctypes as C
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(HERE, "libmavflow.so")          # the one library the product loads; no environment override

MAV_OK, MAV_ERR_ARG, MAV_ERR_HIP, MAV_ERR_OOM, MAV_ERR_STATE = 0, -1, -2, -3, -4


class MavflowError(RuntimeError):
    """HIP / device failure inside libmavflow (the counterpart of cv2.error at the flow-operator seam)."""


class FbParams(C.Structure):
    _fields_ = [("pyr_scale", C.c_double), ("levels", C.c_int), ("winsize", C.c_int), ("iterations", C.c_int),
                ("poly_n", C.c_int), ("poly_sigma", C.c_double), ("flags", C.c_int)]


class FoeParams(C.Structure):
    _fields_ = [("n_pairs", C.c_int), ("mag_threshold", C.c_double), ("ransac_threshold", C.c_double)]


class ThrParams(C.Structure):
    _fields_ = [("fixed_deg", C.c_double), ("fixed_min_mag", C.c_double), ("dyn_min_mag", C.c_double),
                ("dyn_a", C.c_double), ("dyn_b", C.c_double), ("dyn_c", C.c_double)]


class GfttParams(C.Structure):
    """mav_gftt_params: cv2.goodFeaturesToTrack's maxCorners, qualityLevel, minDistance, blockSize."""
    _fields_ = [("max_corners", C.c_int), ("quality_level", C.c_double), ("min_distance", C.c_double), ("block_size", C.c_int)]


class LkParams(C.Structure):
    """mav_lk_params: cv2.calcOpticalFlowPyrLK's winSize, maxLevel, criteria (count, epsilon), minEigThreshold."""
    _fields_ = [("win_w", C.c_int), ("win_h", C.c_int), ("max_level", C.c_int), ("max_count", C.c_int), ("epsilon", C.c_double),
                ("min_eig_threshold", C.c_double)]


LK_MAX_POINTS, LK_MAX_WIN, LK_MAX_LEVEL, LK_HIST_BINS, GFTT_MAX_CANDIDATES = 65536, 33, 7, 104, 262144


class CornerScore(C.Structure):
    """mav_corner_score: cv2.goodFeaturesToTrack's useHarrisDetector and k."""
    _fields_ = [("use_harris", C.c_int), ("k", C.c_double)]


class Result(C.Structure):
    _fields_ = [("box", C.c_int32 * 4), ("foe", C.c_double * 2)]


RESULT_DTYPE = np.dtype([("box", np.int32, (4,)), ("foe", np.float64, (2,))])
assert RESULT_DTYPE.itemsize == C.sizeof(Result) == 32

class MotionResult(C.Structure):
    """mav_motion_result: one item of mav_global_motion."""
    _fields_ = [("max_mag", C.c_float), ("max_row", C.c_int32), ("max_col", C.c_int32), ("reserved", C.c_int32),
                ("window", C.c_int64 * 6), ("opt_score", C.c_int64), ("opt_window", C.c_int32 * 4)]


MOTION_DTYPE = np.dtype([("max_mag", np.float32), ("max_row", np.int32), ("max_col", np.int32), ("reserved", np.int32),
                         ("window", np.int64, (6,)), ("opt_score", np.int64), ("opt_window", np.int32, (4,))])
assert MOTION_DTYPE.itemsize == C.sizeof(MotionResult) == 88
HOMOGRAPHY_MAX_PAIRS = 65536


class CcParams(C.Structure):
    """mav_cc_params: connectivity (4 | 8), min_area (>= 1), max_blobs (1 .. CC_MAX_BLOBS)."""
    _fields_ = [("connectivity", C.c_int), ("min_area", C.c_int), ("max_blobs", C.c_int)]


class CcCounts(C.Structure):
    _fields_ = [("n_components", C.c_int32), ("n_blobs", C.c_int32)]


class Blob(C.Structure):
    """mav_blob: one connected component (x, y, w, h as cv2's CC_STAT_LEFT / TOP / WIDTH / HEIGHT; integer coordinate sums)."""
    _fields_ = [("label", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("area", C.c_int32),
                ("sum_x", C.c_int64), ("sum_y", C.c_int64)]


CC_COUNTS_DTYPE = np.dtype([("n_components", np.int32), ("n_blobs", np.int32)])
BLOB_DTYPE = np.dtype([("label", np.int32), ("x", np.int32), ("y", np.int32), ("w", np.int32), ("h", np.int32), ("area", np.int32),
                       ("sum_x", np.int64), ("sum_y", np.int64)])
assert BLOB_DTYPE.itemsize == C.sizeof(Blob) == 40 and CC_COUNTS_DTYPE.itemsize == C.sizeof(CcCounts) == 8
CC_TILE_W, CC_TILE_H, CC_MAX_BLOBS = 64, 16, 65535      # MAV_CC_TILE_W / _H (the first pass's tile), MAV_CC_MAX_BLOBS


class RocParams(C.Structure):
    """mav_roc_params: the two threshold lists of a sweep (host arrays, copied by each call)."""
    _fields_ = [("n_angles", C.c_int), ("n_mags", C.c_int), ("angles", C.POINTER(C.c_double)), ("mags", C.POINTER(C.c_double))]


ROC_MAX_ANGLES, ROC_MAX_MAGS = 64, 16                    # MAV_ROC_MAX_ANGLES / MAV_ROC_MAX_MAGS


def roc_table_words(ka: int, km: int) -> int:
    """MAV_ROC_TABLE_WORDS: pos, neg, then (tp, fp) per (angle, magnitude) cell."""
    return 2 + 2 * int(ka) * int(km)


def roc_params(angles, mags):
    """(RocParams, angles, mags): the lists as contiguous float64 arrays (which the struct points into: keep them alive with it).
    The library checks them (strictly increasing, finite, >= 0, 1 .. 64 angles and 1 .. 16 magnitudes)."""
    a = np.ascontiguousarray(np.asarray(angles, np.float64).reshape(-1))
    m = np.ascontiguousarray(np.asarray(mags, np.float64).reshape(-1))
    p = RocParams(a.size, m.size, a.ctypes.data_as(C.POINTER(C.c_double)), m.ctypes.data_as(C.POINTER(C.c_double)))
    return p, a, m


def roc_expand(table: np.ndarray, ka: int, km: int) -> np.ndarray:
    """(B, words) int64 tables -> (B, ka, km, 4) = pos, neg, tp, fp per cell, as tpr_fpr_counts orders them."""
    table = np.asarray(table, np.int64).reshape(-1, roc_table_words(ka, km))
    out = np.empty((table.shape[0], ka, km, 4), np.int64)
    out[..., 0] = table[:, 0, None, None]
    out[..., 1] = table[:, 1, None, None]
    out[..., 2:] = table[:, 2:].reshape(-1, ka, km, 2)
    return out

class HistoryParams(C.Structure):
    """mav_history_params: ring length (3 .. 64), element depth (DEPTH_32F / DEPTH_64F), flags (HISTORY_AXES_XY)."""
    _fields_ = [("length", C.c_int), ("depth", C.c_int), ("flags", C.c_int)]


HISTORY_MAX_LENGTH = 64                                  # MAV_HISTORY_MAX_LENGTH
HISTORY_AXES_XY = 1                                      # MAV_HISTORY_AXES_XY
HISTORY_OUT_REFERENCE, HISTORY_OUT_FLOW_F32 = 0, 1       # MAV_HISTORY_OUT_*
HISTORY_AXES = {"reference": 0, "xy": HISTORY_AXES_XY}
HISTORY_OUTS = {"reference": (HISTORY_OUT_REFERENCE, np.dtype(np.float64)), "flow": (HISTORY_OUT_FLOW_F32, np.dtype(np.float32))}


def history_schedule(length: int, index: int) -> list:
    """mav_history_schedule: the ring slots a push at `index` walks, in order (Detector.get_history's loop, detector.py:376-385)."""
    slots, n = (C.c_int * HISTORY_MAX_LENGTH)(), C.c_int()
    check(load().mav_history_schedule(int(length), int(index), slots, C.byref(n)))
    return list(slots[:n.value])


# every symbol include/mavflow.h declares (tests check the library exports each of them)
EXPORTS = [
    "mav_fb_defaults", "mav_foe_defaults", "mav_thr_defaults", "mav_create", "mav_destroy", "mav_last_error",
    "mav_device_count", "mav_set_option", "mav_num_layers", "mav_layer_dims", "mav_farneback", "mav_derotate",
    "mav_foe_dense", "mav_ransac", "mav_bgr2gray", "mav_phi_mask", "mav_bbox", "mav_window_max", "mav_tpr_fpr_counts", "mav_process_batch",
    "mav_farneback_dev", "mav_process_batch_dev", "mav_sync", "mav_stream", "mav_dev_alloc", "mav_dev_free",
    "mav_memcpy_h2d", "mav_memcpy_d2h", "mav_host_alloc", "mav_host_free", "mav_upload_async", "mav_upload_fence", "mav_timer_start", "mav_timer_stop", "mav_profile_enable", "mav_profile_get", "mav_profile_busy",
    "mav_comm_unique_id", "mav_comm_init", "mav_comm_destroy", "mav_allgather_results", "mav_stage_blur_resize",
    "mav_stage_polyexp", "mav_stage_update_matrices", "mav_stage_blur_iter",
    "mav_analyze_pyramid", "mav_pyramid_levels", "mav_pyramid_dims", "mav_optimize_window", "mav_stage_pyramid_level",
    "mav_detect", "mav_detect_dev", "mav_last_flow_dev", "mav_foe_dense_f32", "mav_phi_mask_f32", "mav_stage_coefficients",
    "mav_stage_phi_mask", "mav_last_masks_tpr_fpr", "mav_get_option", "mav_schedule_info", "mav_stage_blur_resize_two_pass",
    "mav_membw_probe", "mav_runtime_info", "mav_upload_async_unordered", "mav_mem_info", "mav_profile_intervals",
    "mav_upload_gather", "mav_download_async", "mav_marker_create", "mav_marker_record", "mav_marker_wait", "mav_marker_destroy",
    "mav_tpr_fpr_counts_dev", "mav_bgr2gray_dev", "mav_png_unfilter", "mav_comm_count",
    "mav_marker_query", "mav_frame_step_dev", "mav_frame_step_post", "mav_frame_step_wait", "mav_worker_drain", "mav_worker_wait_enqueued",
    "mav_farneback_init", "mav_farneback_init_dev", "mav_stage_update_matrices_from", "mav_stage_initial_flow",
    "mav_farneback_ex", "mav_farneback_ex_dev", "mav_stage_blur_resize_ex", "mav_schedule_info_ex",
    "mav_render", "mav_render_dev", "mav_last_render", "mav_flow_to_color", "mav_colormap_jet",
    "mav_overlay", "mav_overlay_dev", "mav_last_overlay",
    "mav_png_bound", "mav_png_encode", "mav_png_encode_dev", "mav_last_render_png", "mav_last_overlay_png",
    "mav_gftt_defaults", "mav_lk_defaults", "mav_good_features", "mav_good_features_dev", "mav_lk_track", "mav_lk_track_dev",
    "mav_lk_last_iterations", "mav_lk_level_dims", "mav_stage_lk_pyramid", "mav_stage_lk_scharr", "mav_stage_min_eigen",
    "mav_good_features_ex", "mav_good_features_ex_dev", "mav_lk_track_ex_dev", "mav_gftt_last_pick", "mav_stage_corner_pick",
    "mav_set_window", "mav_get_window",
    "mav_lk_track_err", "mav_lk_track_err_dev", "mav_corner_score_defaults", "mav_good_features_score", "mav_good_features_score_dev",
    "mav_stage_corner_response",
    "mav_find_homography", "mav_find_homography_dev", "mav_flow_homography", "mav_flow_homography_dev", "mav_global_motion",
    "mav_global_motion_dev", "mav_global_motion_step_dev", "mav_last_global_motion_render", "mav_global_motion_batch",
    "mav_global_motion_batch_dev",
    "mav_cc_defaults", "mav_components", "mav_components_dev", "mav_last_masks_components",
    "mav_roc_sweep", "mav_roc_sweep_dev", "mav_last_roc_sweep", "mav_roc_arm",
    "mav_history_defaults", "mav_history_schedule", "mav_history_create", "mav_history_destroy", "mav_history_reset", "mav_history_info",
    "mav_history_push", "mav_history_push_dev", "mav_stage_remap_linear",
]

# Frame depths of the _ex entry points (cv2's depth codes) by numpy dtype.  uint8 frames keep going through the u8 symbols.
DEPTH_8U, DEPTH_16U, DEPTH_32F = 0, 2, 5
DEPTH_64F = 6                                   # the flow history's fields and ring only: never a frame depth
HISTORY_DEPTHS = {np.dtype(np.float32): DEPTH_32F, np.dtype(np.float64): DEPTH_64F}
DEPTHS = {np.dtype(np.uint8): DEPTH_8U, np.dtype(np.uint16): DEPTH_16U, np.dtype(np.float32): DEPTH_32F}

OPTFLOW_USE_INITIAL_FLOW = 4                    # FbParams.flags bit (cv2.OPTFLOW_USE_INITIAL_FLOW): see Context.farneback(initial_flow=);
#                                                 and a `flags` bit of Context.lk_track_err (the starting positions come in next_pts)
OPTFLOW_LK_GET_MIN_EIGENVALS = 8                # cv2.OPTFLOW_LK_GET_MIN_EIGENVALS: Context.lk_track_err's err is the minimum eigenvalue
# cv2.OPTFLOW_FARNEBACK_GAUSSIAN.  Not an FbParams.flags bit (mav_create refuses it): the window belongs to the context --
# Context(window="gaussian") / Context.set_window; mavflow.farneback translates a cv2 argument list that carries the bit.
OPTFLOW_FARNEBACK_GAUSSIAN = 256
WINDOW_BOX, WINDOW_GAUSSIAN = 0, 1
WINDOWS = {"box": WINDOW_BOX, "gaussian": WINDOW_GAUSSIAN}

GATHER_ORDERED, GATHER_SOURCES_HELD = 1, 2      # mav_upload_gather flags
STEP_MAX_GATHER = 4


# every symbol include/mavflow_shapes.h declares (EXPORTS above lists include/mavflow.h alone)
SHAPES_EXPORTS = ("mav_shapes_scratch_bytes", "mav_draw_shapes", "mav_draw_shapes_dev", "mav_shapes_form", "mav_add_saturate",
                  "mav_add_saturate_dev", "mav_bytes_form", "mav_shapes_from_blobs_dev", "mav_mosaic", "mav_mosaic_dev", "mav_motion_pictures_dev")


# every symbol include/mavflow_png_decode.h declares
PNG_DECODE_EXPORTS = ("mav_png_decode_scratch_bytes", "mav_png_decode_dev", "mav_png_decode", "mav_png_inflate_host")
PNG_OUT = {"samples": 0, "bgr": 1, "gray": 2}                      # MAV_PNG_OUT_*
PNG_DECODE_MAX_COUNT = 1024
PNG_ERRORS = ("OK", "HEADER", "TRUNCATED", "BLOCK_TYPE", "STORED_LEN", "CODE_LENGTHS", "SYMBOL", "DISTANCE", "OVERFLOW", "SHORT", "ADLER", "FILTER")
# mav_png_status, 48 bytes
PNG_STATUS_DTYPE = np.dtype([("code", "<i4"), ("adler_stream", "<u4"), ("adler_computed", "<u4"), ("blocks", "<u4", (3,)), ("consumed", "<u8"),
                             ("produced", "<u8"), ("max_length", "<u4"), ("max_distance", "<u4")])


# every symbol include/mavflow_jpeg.h declares
JPEG_EXPORTS = ("mav_jpeg_parse", "mav_jpeg_decode_scratch_bytes", "mav_jpeg_decode_dev", "mav_jpeg_decode", "mav_jpeg_decode_host")
JPEG_OUT = {"samples": 0, "bgr": 1, "gray": 2}                     # MAV_JPEG_OUT_*
JPEG_MAX_COUNT = 1024
JPEG_ERRORS = ("OK", "TRUNCATED", "CODE", "COEF_INDEX", "RESTART", "UNSUPPORTED")     # MAV_JPEG_E_*
# mav_jpeg_status, 40 bytes
JPEG_STATUS_DTYPE = np.dtype([("code", "<i4"), ("intervals", "<u4"), ("consumed", "<u8"), ("mcus", "<u4"), ("nonzero", "<u4"), ("zrl", "<u4"),
                              ("stuffed", "<u4"), ("max_code_len", "<u4"), ("pad", "<u4")])
_JPEG_COMPONENT = np.dtype([("id", "u1"), ("h", "u1"), ("v", "u1"), ("tq", "u1"), ("td", "u1"), ("ta", "u1"), ("pad", "u1", (2,))])
_JPEG_HUFFMAN = np.dtype([("counts", "u1", (16,)), ("values", "u1", (256,))])
# mav_jpeg_info, 2512 bytes
JPEG_INFO_DTYPE = np.dtype([("W", "<i4"), ("H", "<i4"), ("components", "<i4"), ("restart_interval", "<i4"), ("entropy_offset", "<u8"),
                            ("entropy_bytes", "<u8"), ("comp", _JPEG_COMPONENT, (4,)), ("quant_defined", "u1", (4,)), ("dc_defined", "u1", (4,)),
                            ("ac_defined", "u1", (4,)), ("pad", "u1", (4,)), ("quant", "u1", (4, 64)), ("dc", _JPEG_HUFFMAN, (4,)),
                            ("ac", _JPEG_HUFFMAN, (4,))])


class Gather(C.Structure):
    _fields_ = [("src_host", C.POINTER(C.c_void_p)), ("count", C.c_int), ("bytes_each", C.c_size_t), ("dst_dev", C.c_void_p)]


class FrameStep(C.Structure):
    """mav_frame_step (include/mavflow.h): one iteration of the reference's loop as one call."""
    _fields_ = [("n", C.c_int),
                ("wait_before", C.POINTER(C.c_void_p)), ("n_wait_before", C.c_int),
                ("par_host", C.c_void_p), ("par_dev", C.c_void_p), ("par_bytes", C.c_size_t),
                ("gather", Gather * STEP_MAX_GATHER), ("n_gather", C.c_int),
                ("bgr_dev", C.c_void_p), ("n_bgr", C.c_int), ("gray_dev", C.c_void_p),
                ("compute_flow", C.c_int), ("prev_dev", C.c_void_p), ("next_dev", C.c_void_p), ("flow_dev", C.c_void_p),
                ("record_after_flow", C.POINTER(C.c_void_p)), ("n_record_after_flow", C.c_int),
                ("detect", C.c_int),
                ("off_samples", C.c_size_t), ("off_omega", C.c_size_t), ("off_dt", C.c_size_t), ("off_frame0", C.c_size_t),
                ("has_omega", C.c_int), ("has_frame0", C.c_int),
                ("sky_dev", C.c_void_p), ("gt_dev", C.c_void_p), ("gt_images", C.c_int),
                ("foe", FoeParams), ("thr", ThrParams),
                ("mask_fixed_dev", C.c_void_p), ("mask_dyn_dev", C.c_void_p), ("out_dev", C.c_void_p),
                ("off_counts_fixed", C.c_size_t), ("off_counts_dyn", C.c_size_t),
                ("out_host", C.c_void_p), ("out_bytes", C.c_size_t), ("record_done", C.c_void_p),
                ("cc", CcParams), ("off_cc_counts", C.c_size_t), ("off_cc_blobs", C.c_size_t)]

_lib = None


def load(path: str | None = None) -> C.CDLL:
    """Load libmavflow.so (built in-tree by `make -C mav-detection_amd/csrc` / __graft_entry__.build()).
    path: an explicit other build of the same ABI, given by a diagnostic tool BEFORE anything else loads the library
    (tools/phase_stamps.py and its -DMAV_STAMPS build); the product never passes one."""
    global _lib
    if _lib is not None:
        if path is not None and os.path.abspath(path) != _lib._name:
            raise RuntimeError(f"libmavflow is already loaded from {_lib._name}")
        return _lib
    so = os.path.abspath(path) if path is not None else SO_PATH
    if not os.path.exists(so):
        raise ImportError(f"{so} is missing: build it with __graft_entry__.build(); there is no CPU fallback")
    lib = C.CDLL(so)
    lib.mav_last_error.restype = C.c_char_p
    lib.mav_stream.restype = C.c_void_p
    lib.mav_last_flow_dev.restype = C.c_void_p
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("mav_last_error", "mav_stream", "mav_fb_defaults", "mav_foe_defaults", "mav_thr_defaults", "mav_last_flow_dev", "mav_png_bound",
                        "mav_gftt_defaults", "mav_lk_defaults", "mav_corner_score_defaults", "mav_cc_defaults", "mav_history_defaults"):
            fn.restype = C.c_int
    lib.mav_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(FbParams)]
    lib.mav_destroy.argtypes = [C.c_void_p]
    lib.mav_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    lib.mav_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_long)]
    lib.mav_schedule_info.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    lib.mav_set_window.argtypes = [C.c_void_p, C.c_int]
    lib.mav_get_window.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.mav_runtime_info.argtypes = [C.c_char_p, C.c_size_t]
    lib.mav_membw_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    lib.mav_num_layers.argtypes = [C.c_void_p]
    lib.mav_mem_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_size_t)] * 4
    lib.mav_layer_dims.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    vp = C.c_void_p
    lib.mav_farneback.argtypes = [vp, vp, vp, C.c_int, vp]
    lib.mav_farneback_dev.argtypes = [vp, vp, vp, C.c_int, vp]
    lib.mav_farneback_init.argtypes = [vp, vp, vp, C.c_int, vp, vp]
    lib.mav_farneback_init_dev.argtypes = [vp, vp, vp, C.c_int, vp, vp]
    lib.mav_derotate.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    lib.mav_foe_dense.argtypes = [vp, vp, vp, C.c_int, C.POINTER(FoeParams), vp]
    lib.mav_ransac.argtypes = [vp, vp, C.c_int, C.c_double, vp]
    lib.mav_bgr2gray.argtypes = [vp, vp, C.c_int, vp]
    lib.mav_phi_mask.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(ThrParams), vp, vp, vp, vp]
    lib.mav_bbox.argtypes = [vp, vp, C.c_int, vp]
    lib.mav_window_max.argtypes = [vp, vp, C.c_int, vp]
    lib.mav_tpr_fpr_counts.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
    lib.mav_last_masks_tpr_fpr.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    lib.mav_analyze_pyramid.argtypes = [vp, vp, C.c_int, C.c_double, vp]
    lib.mav_pyramid_levels.argtypes = [vp, C.c_double]
    lib.mav_pyramid_dims.argtypes = [vp, C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mav_optimize_window.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    lib.mav_stage_pyramid_level.argtypes = [vp, vp, C.c_double, C.c_int, vp]
    # ctx, prev, next, samples, omega, dt, frame0, sky, batch, foe params, thr params, flow, phi, mask_fixed, mask_dyn, results
    pb = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(FoeParams), C.POINTER(ThrParams), vp, vp, vp, vp, vp]
    lib.mav_process_batch.argtypes = pb
    lib.mav_process_batch_dev.argtypes = pb
    # ctx, flow, samples, omega, dt, frame0, sky, batch, foe params, thr params, phi, mask_fixed, mask_dyn, results
    dt_ = [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(FoeParams), C.POINTER(ThrParams), vp, vp, vp, vp]
    lib.mav_detect.argtypes = dt_
    lib.mav_detect_dev.argtypes = dt_
    lib.mav_last_flow_dev.argtypes = [vp]
    lib.mav_foe_dense_f32.argtypes = [vp, vp, vp, C.c_int, C.POINTER(FoeParams), vp]
    lib.mav_phi_mask_f32.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(ThrParams), vp, vp, vp, vp]
    lib.mav_stage_coefficients.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.mav_stage_phi_mask.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(ThrParams), vp, vp, vp, vp]
    lib.mav_sync.argtypes = [vp]
    lib.mav_stream.argtypes = [vp]
    lib.mav_dev_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.mav_dev_free.argtypes = [vp, vp]
    lib.mav_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    lib.mav_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    lib.mav_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.mav_host_free.argtypes = [vp, vp]
    lib.mav_upload_async.argtypes = [vp, vp, vp, C.c_size_t]
    lib.mav_upload_async_unordered.argtypes = [vp, vp, vp, C.c_size_t]
    lib.mav_upload_fence.argtypes = [vp]
    lib.mav_upload_gather.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.c_size_t, C.c_int]
    lib.mav_download_async.argtypes = [vp, vp, vp, C.c_size_t]
    lib.mav_marker_create.argtypes = [vp, C.POINTER(vp)]
    lib.mav_marker_record.argtypes = [vp, vp]
    lib.mav_marker_wait.argtypes = [vp, vp]
    lib.mav_marker_destroy.argtypes = [vp, vp]
    lib.mav_marker_query.argtypes = [vp, vp, C.POINTER(C.c_int)]
    lib.mav_frame_step_dev.argtypes = [vp, C.POINTER(FrameStep)]
    lib.mav_frame_step_post.argtypes = [vp, C.POINTER(FrameStep), C.POINTER(C.c_uint64)]
    lib.mav_frame_step_wait.argtypes = [vp, C.c_uint64, vp]
    lib.mav_worker_drain.argtypes = [vp]
    lib.mav_worker_wait_enqueued.argtypes = [vp, C.c_uint64]
    lib.mav_tpr_fpr_counts_dev.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]
    lib.mav_bgr2gray_dev.argtypes = [vp, vp, C.c_int, vp]
    lib.mav_png_unfilter.argtypes = [vp, C.c_int, C.c_size_t, C.c_int, vp]
    lib.mav_timer_start.argtypes = [vp]
    lib.mav_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    lib.mav_profile_enable.argtypes = [vp, C.c_int]
    lib.mav_profile_get.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_long)]
    lib.mav_profile_busy.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double)]
    lib.mav_profile_intervals.argtypes = [vp, C.POINTER(C.c_int), vp, vp, vp, vp]
    lib.mav_comm_unique_id.argtypes = [vp]
    lib.mav_comm_init.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.mav_comm_destroy.argtypes = [vp]
    lib.mav_comm_count.argtypes = [vp, C.POINTER(C.c_int)]
    lib.mav_allgather_results.argtypes = [vp, vp, vp, C.c_size_t, vp]
    lib.mav_stage_blur_resize.argtypes = [vp, vp, C.c_int, vp]
    lib.mav_stage_blur_resize_two_pass.argtypes = [vp, vp, C.c_int, vp]
    lib.mav_stage_polyexp.argtypes = [vp, vp, C.c_int, vp]
    lib.mav_stage_update_matrices.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    lib.mav_stage_blur_iter.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    lib.mav_stage_update_matrices_from.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    lib.mav_stage_initial_flow.argtypes = [vp, vp, C.c_int, vp]
    lib.mav_farneback_ex.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
    lib.mav_farneback_ex_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
    lib.mav_stage_blur_resize_ex.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.mav_schedule_info_ex.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    # ctx, flow, foe, omega, dt, frame0, sky, batch, thr params, img_result, img_flow, img_phi
    rn = [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(ThrParams), vp, vp, vp]
    lib.mav_render.argtypes = rn
    lib.mav_render_dev.argtypes = rn
    lib.mav_last_render.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.mav_flow_to_color.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    lib.mav_colormap_jet.argtypes = [vp, vp, C.c_size_t, vp]
    # ctx, frames, mask_fixed, foe, foe_gt, batch, radius, overlay, written
    lib.mav_overlay.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    lib.mav_overlay_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    lib.mav_last_overlay.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
    lib.mav_png_bound.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.mav_png_bound.restype = C.c_size_t
    lib.mav_png_encode.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp]
    lib.mav_png_encode_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp]
    lib.mav_last_render_png.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp]
    lib.mav_last_overlay_png.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp]
    lib.mav_gftt_defaults.argtypes = [C.POINTER(GfttParams)]
    lib.mav_lk_defaults.argtypes = [C.POINTER(LkParams)]
    lib.mav_good_features.argtypes = [vp, vp, C.POINTER(GfttParams), vp, C.POINTER(C.c_int)]
    lib.mav_good_features_dev.argtypes = [vp, vp, C.POINTER(GfttParams), vp, C.POINTER(C.c_int)]
    # ctx, prev, next, pts, n, params, next_pts, status
    lib.mav_lk_track.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(LkParams), vp, vp]
    lib.mav_lk_track_dev.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(LkParams), vp, vp]
    lib.mav_lk_last_iterations.argtypes = [vp, vp]
    lib.mav_lk_level_dims.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mav_stage_lk_pyramid.argtypes = [vp, vp, C.c_int, vp]
    lib.mav_stage_lk_scharr.argtypes = [vp, vp, C.c_int, vp]
    lib.mav_stage_min_eigen.argtypes = [vp, vp, C.c_int, vp]
    # ctx, gray, mask, params, corners, count
    lib.mav_good_features_ex.argtypes = [vp, vp, vp, C.POINTER(GfttParams), vp, C.POINTER(C.c_int)]
    lib.mav_good_features_ex_dev.argtypes = [vp, vp, vp, C.POINTER(GfttParams), vp, vp]
    # ctx, prev, next, pts, n_max, n_dev, params, next_pts, status
    lib.mav_lk_track_ex_dev.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.POINTER(LkParams), vp, vp]
    lib.mav_gftt_last_pick.argtypes = [vp, vp]
    lib.mav_stage_corner_pick.argtypes = [vp, vp, C.c_int, C.POINTER(GfttParams), vp, C.POINTER(C.c_int)]
    # ctx, prev, next, pts, n, params, flags, next_pts, status, err
    lib.mav_lk_track_err.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(LkParams), C.c_int, vp, vp, vp]
    # ctx, prev, next, pts, n_max, n_dev, params, flags, next_pts, status, err
    lib.mav_lk_track_err_dev.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.POINTER(LkParams), C.c_int, vp, vp, vp]
    lib.mav_corner_score_defaults.argtypes = [C.POINTER(CornerScore)]
    lib.mav_good_features_score.argtypes = [vp, vp, vp, C.POINTER(GfttParams), C.POINTER(CornerScore), vp, C.POINTER(C.c_int)]
    lib.mav_good_features_score_dev.argtypes = [vp, vp, vp, C.POINTER(GfttParams), C.POINTER(CornerScore), vp, vp]
    lib.mav_stage_corner_response.argtypes = [vp, vp, C.c_int, C.POINTER(CornerScore), vp]
    # ctx, src, dst, n, batch, H, ok
    lib.mav_find_homography.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
    lib.mav_find_homography_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
    # ctx, flow, coords, n, batch, H, ok (, pairs_dst)
    lib.mav_flow_homography.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    lib.mav_flow_homography_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
    # ctx, flow, M, batch, scale, optimize, warped, mag, gray, results
    gm = [vp, vp, vp, C.c_int, C.c_double, C.c_int, vp, vp, vp, vp]
    lib.mav_global_motion.argtypes = gm
    lib.mav_global_motion_dev.argtypes = gm
    # ctx, flow, coords, n, batch, scale, optimize, H, ok, gray, results
    lib.mav_global_motion_step_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, vp, vp]
    lib.mav_last_global_motion_render.argtypes = [vp, C.c_int, vp, vp]
    # ctx, prev, next, coords, n, batch, scale, optimize, flow, H, ok, gray, results
    gmb = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, vp, vp, vp]
    lib.mav_global_motion_batch.argtypes = gmb
    lib.mav_global_motion_batch_dev.argtypes = gmb
    lib.mav_cc_defaults.argtypes = [C.POINTER(CcParams)]
    lib.mav_cc_defaults.restype = None
    lib.mav_components.argtypes = [vp, vp, C.c_int, C.POINTER(CcParams), vp, vp, vp]
    lib.mav_components_dev.argtypes = [vp, vp, C.c_int, C.POINTER(CcParams), vp, vp, vp]
    lib.mav_last_masks_components.argtypes = [vp, C.c_int, C.c_int, C.POINTER(CcParams), vp, vp, vp]
    rp = C.POINTER(RocParams)
    lib.mav_roc_sweep.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(ThrParams), rp, vp]
    lib.mav_roc_sweep_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(ThrParams), rp, vp]
    lib.mav_last_roc_sweep.argtypes = [vp, vp, C.c_int, C.c_int, rp, vp]
    lib.mav_roc_arm.argtypes = [vp, rp, C.c_size_t]
    lib.mav_history_defaults.argtypes = [C.POINTER(HistoryParams)]
    lib.mav_history_defaults.restype = None
    lib.mav_history_schedule.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mav_history_create.argtypes = [vp, C.POINTER(HistoryParams), C.POINTER(C.c_void_p)]
    lib.mav_history_destroy.argtypes = [vp, vp]
    lib.mav_history_reset.argtypes = [vp, vp]
    lib.mav_history_info.argtypes = [vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_size_t)]
    # ctx, history, flow, flow_depth, count, out_form, out
    lib.mav_history_push.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.mav_history_push_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.mav_stage_remap_linear.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    # include/mavflow_shapes.h (SHAPES_EXPORTS; the methods are mavflow.shapes')
    i = C.c_int
    lib.mav_shapes_scratch_bytes.restype, lib.mav_shapes_scratch_bytes.argtypes = C.c_size_t, [i, i, i]
    lib.mav_draw_shapes.argtypes = [vp, vp, i, i, vp, i]                          # ctx, img, channels, batch, shapes, n
    lib.mav_draw_shapes_dev.argtypes = [vp, vp, i, i, vp, i, vp, vp]              # ctx, img, channels, batch, shapes, n_max, n_dev, scratch
    lib.mav_shapes_form.argtypes = [vp, i, i]                                     # shapes, n, channels
    for fn in (lib.mav_add_saturate, lib.mav_add_saturate_dev):                   # ctx, a, b, channels, batch, dst
        fn.argtypes = [vp, vp, vp, i, i, vp]
    lib.mav_bytes_form.argtypes = [C.c_size_t, vp, vp, vp]                        # n, a, b, dst
    lib.mav_shapes_from_blobs_dev.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp]    # ctx, blobs, counts, batch, max_blobs, thickness, colour, out, n_out
    for fn in (lib.mav_mosaic, lib.mav_mosaic_dev):                               # ctx, tiles, tile_channels, rows, cols, batch, out
        fn.argtypes = [vp, vp, vp, i, i, i, vp]
    lib.mav_motion_pictures_dev.argtypes = [vp, vp, i, vp, vp, vp, vp]            # ctx, flow, batch, field, img_flow, img_warped, img_global
    # include/mavflow_png_decode.h (PNG_DECODE_EXPORTS)
    lib.mav_png_decode_scratch_bytes.restype, lib.mav_png_decode_scratch_bytes.argtypes = C.c_size_t, [i, i, i, i]     # W, H, channels, count
    # ctx, streams, index, count, W, H, channels, out_format, out, status[, scratch]
    lib.mav_png_decode_dev.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp]
    lib.mav_png_decode.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp]
    lib.mav_png_inflate_host.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp]                                          # z, n, raw, raw_bytes, status
    for fn in (lib.mav_png_decode_dev, lib.mav_png_decode, lib.mav_png_inflate_host):
        fn.restype = C.c_int
    # include/mavflow_jpeg.h (JPEG_EXPORTS)
    lib.mav_jpeg_parse.argtypes = [vp, C.c_size_t, vp]                                                               # file, n, info
    lib.mav_jpeg_decode_scratch_bytes.restype, lib.mav_jpeg_decode_scratch_bytes.argtypes = C.c_size_t, [i, i, i, i]   # W, H, components, count
    # ctx, files, index, info, count, W, H, out_format, out, status[, scratch]
    lib.mav_jpeg_decode_dev.argtypes = [vp, vp, vp, vp, i, i, i, i, vp, vp, vp]
    lib.mav_jpeg_decode.argtypes = [vp, vp, vp, vp, i, i, i, i, vp, vp]
    lib.mav_jpeg_decode_host.argtypes = [vp, C.c_size_t, vp, i, vp, vp]                                              # file, n, info, out_format, out, status
    for fn in (lib.mav_jpeg_parse, lib.mav_jpeg_decode_dev, lib.mav_jpeg_decode, lib.mav_jpeg_decode_host):
        fn.restype = C.c_int
    _lib = lib
    return lib


def jpeg_info(data):
    """(info, None) -- mav_jpeg_parse's answer as a (1,) array of JPEG_INFO_DTYPE -- or (None, the parser's reason) for a file it refuses"""
    lib = load()
    raw = np.frombuffer(bytes(data) + b"\0", np.uint8)
    info = np.zeros(1, JPEG_INFO_DTYPE)
    rc = lib.mav_jpeg_parse(raw.ctypes.data, len(data), info.ctypes.data)
    if rc == MAV_OK:
        return info, None
    why = lib.mav_last_error().decode("utf-8", "replace")
    name = JPEG_ERRORS[rc] if 0 < rc < len(JPEG_ERRORS) else str(rc)
    return None, f"MAV_JPEG_E_{name} ({rc}): {why}"


def jpeg_parse(data) -> dict:
    """mav_jpeg_parse as a dict: W, H, components [(id, h, v, tq, td, ta)], quant {id: (64,) u8 in natural order}, dc / ac {id: (counts (16,),
    values (sum,))}, restart_interval, entropy_offset, entropy_bytes.  ValueError with the parser's reason for a file it refuses."""
    info, why = jpeg_info(data)
    if info is None:
        raise ValueError(f"jpeg_parse(): {why}")
    r = info[0]
    n = int(r["components"])

    def tables(kind):
        return {t: (r[kind][t]["counts"].copy(), r[kind][t]["values"][:int(r[kind][t]["counts"].sum())].copy())
                for t in range(4) if r[kind + "_defined"][t]}
    return {"W": int(r["W"]), "H": int(r["H"]),
            "components": [tuple(int(r["comp"][c][k]) for k in ("id", "h", "v", "tq", "td", "ta")) for c in range(n)],
            "quant": {t: r["quant"][t].copy() for t in range(4) if r["quant_defined"][t]}, "dc": tables("dc"), "ac": tables("ac"),
            "restart_interval": int(r["restart_interval"]), "entropy_offset": int(r["entropy_offset"]), "entropy_bytes": int(r["entropy_bytes"])}


def jpeg_decode_host(data, out: str = "bgr", return_status: bool = False):
    """mav_jpeg_decode_host: one baseline JPEG file decoded on the host by the source the device runs -> (H, W, 3) BGR, (H, W) gray or
    the samples (H, W[, 3]); None for a file the parser or the decoder refuses (return_status=True: (array or None, status record or
    the parser's reason))."""
    if out not in JPEG_OUT:
        raise ValueError(f"jpeg_decode_host(): out must be one of {sorted(JPEG_OUT)}, got {out!r}")
    info, why = jpeg_info(data)
    if info is None:
        return (None, why) if return_status else None
    comps = int(info["components"][0])
    oc = {"samples": comps, "bgr": 3, "gray": 1}[out]
    raw = np.frombuffer(bytes(data) + b"\0", np.uint8)
    img = np.empty((int(info["H"][0]), int(info["W"][0]), oc), np.uint8)
    status = np.zeros(1, JPEG_STATUS_DTYPE)
    check(load().mav_jpeg_decode_host(raw.ctypes.data, len(data), info.ctypes.data, JPEG_OUT[out], img.ctypes.data, status.ctypes.data))
    if oc == 1:
        img = img[..., 0]
    if return_status:
        return img, status[0]
    return img if status["code"][0] == 0 else None


def loaded() -> bool:
    """True when libmavflow.so is loaded, or loads now (it is built in-tree); False where there is no library to load"""
    try:
        load()
        return True
    except (ImportError, OSError):
        return False


def check(rc: int) -> None:
    """Map an error code to the exception the reference raises at that seam."""
    if rc == MAV_OK:
        return
    msg = load().mav_last_error().decode("utf-8", "replace")
    if rc == MAV_ERR_ARG:
        raise ValueError(msg)
    if rc == MAV_ERR_OOM:
        raise MemoryError(msg)
    raise MavflowError(f"[{rc}] {msg}")


def fb_defaults(levels: int | None = None) -> FbParams:
    p = FbParams()
    load().mav_fb_defaults(C.byref(p))
    if levels is not None:
        p.levels = levels
    return p


def foe_defaults() -> FoeParams:
    p = FoeParams()
    load().mav_foe_defaults(C.byref(p))
    return p


def thr_defaults() -> ThrParams:
    p = ThrParams()
    load().mav_thr_defaults(C.byref(p))
    return p


def cc_defaults(**kw) -> CcParams:
    """mav_cc_defaults (8, 1, 256) with the given fields replaced: connectivity, min_area, max_blobs."""
    p = CcParams()
    load().mav_cc_defaults(C.byref(p))
    for k, v in kw.items():
        if k not in dict(CcParams._fields_):
            raise ValueError(f"unknown connected-components parameter {k!r}")
        setattr(p, k, int(v))
    return p


def gftt_defaults(**kw) -> GfttParams:
    """cv2.goodFeaturesToTrack's parameters, the reference's values by default; keywords: the struct's fields or cv2's names."""
    p = GfttParams()
    load().mav_gftt_defaults(C.byref(p))
    names = {"maxCorners": "max_corners", "qualityLevel": "quality_level", "minDistance": "min_distance", "blockSize": "block_size"}
    for k, v in kw.items():
        k = names.get(k, k)
        if k not in dict(GfttParams._fields_):
            raise TypeError(f"good_features: unknown parameter {k!r}")
        setattr(p, k, v)
    return p


def corner_score(useHarrisDetector=False, k=0.04) -> CornerScore:
    """cv2.goodFeaturesToTrack's useHarrisDetector / k as a mav_corner_score."""
    s = CornerScore()
    load().mav_corner_score_defaults(C.byref(s))
    s.use_harris, s.k = int(bool(useHarrisDetector)), float(k)
    return s


def lk_defaults(**kw) -> LkParams:
    """cv2.calcOpticalFlowPyrLK's parameters, the reference's values by default; keywords: the struct's fields, or cv2's winSize = (w, h),
    maxLevel, criteria = (type, count, epsilon), minEigThreshold."""
    p = LkParams()
    load().mav_lk_defaults(C.byref(p))
    names = {"maxLevel": "max_level", "minEigThreshold": "min_eig_threshold"}
    for k, v in kw.items():
        if k == "winSize":
            p.win_w, p.win_h = int(v[0]), int(v[1])
        elif k == "criteria":                    # (TERM_CRITERIA_COUNT = 1 | TERM_CRITERIA_EPS = 2, count, epsilon)
            if int(v[0]) & 1:
                p.max_count = int(v[1])
            if int(v[0]) & 2:
                p.epsilon = float(v[2])
        else:
            k = names.get(k, k)
            if k not in dict(LkParams._fields_):
                raise TypeError(f"lk_track: unknown parameter {k!r}")
            setattr(p, k, v)
    return p


def _depth_of(dtype, name="frames") -> int:
    """MAV_DEPTH_* code of a frame dtype; ValueError naming the accepted dtypes for any other."""
    d = DEPTHS.get(np.dtype(dtype))
    if d is None:
        raise ValueError(f"{name}: expected uint8, uint16 or float32 frames (float64 is narrowed to float32), got {np.dtype(dtype)}")
    return d


def _window_code(window) -> int:
    """"box" / "gaussian", or a MAV_WINDOW_* code as it is (the library range-checks it); anything else is a ValueError like every
    bad argument."""
    if isinstance(window, str) and window in WINDOWS:
        return WINDOWS[window]
    if isinstance(window, (int, np.integer)) and not isinstance(window, bool):
        return int(window)
    raise ValueError(f"window must be 'box' or 'gaussian', got {window!r}")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _arr(a, dtype, shape=None, name="array"):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
    return a


class _PinnedPool:
    """Page-locked host memory for the arrays the host-pointer entry points hand back.  A fresh numpy array is pageable and
    untouched: a 16.6 MB flow field costs ~4000 first-touch page faults plus the runtime's staging copy, more than the GPU
    needs to compute it.  Results are therefore written into page-locked blocks (PCIe rate, no faults) that return to this
    pool when the last numpy array or view over them is garbage-collected.
    Module-level: a block lent out survives the context that allocated it."""

    CAP_BYTES = 2 << 30                                  # idle blocks kept for re-use: at most this much page-locked memory in all

    def __init__(self):
        self.free = {}                                   # nbytes -> [ptr, ...]
        self.idle_bytes = 0
        self.stamp = {}                                  # nbytes -> tick of the last use of that size (least recently used goes first)
        self.tick = 0
        # A block that is the TARGET of a device -> host copy still enqueued (a retired DeviceArray, pipeline.py) must not be lent out
        # again before that copy has landed, even if every array over it has been dropped: guard[ptr] = the marker recorded behind
        # the copy; a returning block whose marker has not fired waits in `pending` (checked with mav_marker_query, never blocking).
        self.guard = {}                                  # ptr -> marker object (has .done())
        self.pending = []                                # [(marker, nbytes, ptr), ...]

    def guard_until(self, arr: np.ndarray, marker) -> None:
        """`arr` (from empty()) is being written by a copy that completes when `marker.done()`: keep its block out of circulation until then."""
        base = arr
        while isinstance(getattr(base, "base", None), np.ndarray):
            base = base.base
        self.guard[base.ctypes.data] = marker

    def _reap(self) -> None:
        if self.pending:
            still = []
            for marker, nbytes, ptr in self.pending:
                if marker.done():
                    self._shelve(nbytes, ptr)
                else:
                    still.append((marker, nbytes, ptr))
            self.pending = still

    def empty(self, ctx: "Context", shape, dtype) -> np.ndarray:
        import weakref
        dtype = np.dtype(dtype)
        nbytes = max(1, int(np.prod(shape)) * dtype.itemsize)
        self.tick += 1
        self.stamp[nbytes] = self.tick
        self._reap()
        lst = self.free.get(nbytes)
        if lst:
            ptr = lst.pop()
            self.idle_bytes -= nbytes
        else:
            p = C.c_void_p()
            check(ctx.lib.mav_host_alloc(ctx._h, nbytes, C.byref(p)))
            ptr = p.value
        # the finalizer hangs on the ctypes object that OWNS the memory in numpy's eyes: every array or view derived from it
        # (numpy collapses view chains onto the owner) keeps it alive, so the block returns only when the last of them is gone
        owner = (C.c_uint8 * nbytes).from_address(ptr)
        weakref.finalize(owner, self._give, nbytes, ptr).atexit = False      # at interpreter exit the OS reclaims; no HIP calls then
        return np.ctypeslib.as_array(owner).view(dtype)[:int(np.prod(shape))].reshape(shape)

    def _give(self, nbytes, ptr):
        """A block comes back (the last array over it is gone) -- to the shelf, or, while a copy into it is still enqueued, to `pending`."""
        marker = self.guard.pop(ptr, None)
        if marker is not None and not marker.done():
            self.pending.append((marker, nbytes, ptr))
            return
        self._shelve(nbytes, ptr)

    def _shelve(self, nbytes, ptr):
        """At most 4 idle blocks per size and CAP_BYTES idle in all: a long-running caller with changing batch
        sizes (a 64-pair 1080p flow block is 1 GB) must not pile up page-locked memory -- blocks of the least recently used sizes
        are released first, then the returning block itself if it alone exceeds the cap."""
        lst = self.free.setdefault(nbytes, [])
        if len(lst) >= 4 or nbytes > self.CAP_BYTES:
            load().mav_host_free(None, ptr)
            return
        lst.append(ptr)
        self.idle_bytes += nbytes
        for size in sorted(self.free, key=lambda k: self.stamp.get(k, 0)):
            while self.idle_bytes > self.CAP_BYTES and self.free[size] and not (size == nbytes and len(self.free[size]) == 1):
                load().mav_host_free(None, self.free[size].pop())
                self.idle_bytes -= size
        if self.idle_bytes > self.CAP_BYTES:             # only this block's own size is left
            load().mav_host_free(None, lst.pop())
            self.idle_bytes -= nbytes


_pinned = _PinnedPool()


class DeviceBuffer:
    """A hipMalloc'd buffer owned through the C-ABI (bench / multi-GPU path)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        check(ctx.lib.mav_dev_alloc(ctx._h, self.nbytes, C.byref(p)))      # (an allocation touches no stream: no need to drain the worker)
        self.ptr = p.value

    def upload(self, a: np.ndarray):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        check(self.ctx.lib.mav_memcpy_h2d(self.ctx.h, self.ptr, _ptr(a), a.nbytes))
        return self

    def download(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        check(self.ctx.lib.mav_memcpy_d2h(self.ctx.h, _ptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.mav_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


def _dev_ptr(p) -> int:
    """A device pointer: an int, or an object with a .ptr (DeviceBuffer, pipeline.DeviceArray)."""
    return int(getattr(p, "ptr", p))


class FlowHistory:
    """One mav_history of a context (Context.flow_history): a ring of the last `length` flow fields on the device and, per push, every
    pixel's accumulated displacement along its trajectory through them (the reference's Detector.get_history, detector.py:365-388)."""

    def __init__(self, ctx: "Context", length: int = 20, dtype=np.float32, axes: str = "reference"):
        if np.dtype(dtype) not in HISTORY_DEPTHS:
            raise ValueError(f"flow_history: dtype must be float32 or float64, got {np.dtype(dtype)}")
        if axes not in HISTORY_AXES:
            raise ValueError(f"flow_history: axes must be 'reference' or 'xy', got {axes!r}")
        self.ctx, self.length, self.dtype, self.axes = ctx, int(length), np.dtype(dtype), axes
        p = HistoryParams(self.length, HISTORY_DEPTHS[self.dtype], HISTORY_AXES[axes])
        h = C.c_void_p()
        check(ctx.lib.mav_history_create(ctx.h, C.byref(p), C.byref(h)))
        self._h = h

    def _info(self):
        i, n, b = C.c_int(), C.c_long(), C.c_size_t()
        check(self.ctx.lib.mav_history_info(self.ctx.h, self._h, C.byref(i), C.byref(n), C.byref(b)))
        return i.value, n.value, b.value

    @property
    def index(self) -> int:
        """The slot the next field goes to (the reference's history_index)."""
        return self._info()[0]

    @property
    def pushes(self) -> int:
        return self._info()[1]

    @property
    def ring_bytes(self) -> int:
        return self._info()[2]

    @staticmethod
    def _out_form(out: str):
        if out not in HISTORY_OUTS:
            raise ValueError(f"push: out must be 'reference' or 'flow', got {out!r}")
        return HISTORY_OUTS[out]

    def push(self, flow, out: str = "reference") -> np.ndarray:
        """Store the field(s) and return the accumulated displacement(s).  flow: (H, W, 2) -> (H, W, 2), or (n, H, W, 2) -> (n, H, W, 2),
        float32 or (into a float64 ring) float64; a host array, or a device handle with .ptr / .shape / .dtype (pipeline.DeviceArray)
        of this context, which is read where it is.  out="reference": float64 (r - y, c - x), the reference's return value;
        out="flow": float32 (c - x, r - y), the (u, v) layout Context.detect takes."""
        form, odt = self._out_form(out)
        ctx = self.ctx
        on_dev = hasattr(flow, "ptr") and getattr(flow, "on_device", True) and getattr(flow, "ctx", ctx) is ctx
        if on_dev and getattr(flow, "_deferred", None) is not None:        # a flow the flow stage has not enqueued yet
            flow._deferred.flush()
        a = flow if on_dev else np.asarray(flow)
        shape, dt = tuple(a.shape), np.dtype(a.dtype)
        if dt not in HISTORY_DEPTHS:
            raise ValueError(f"push: expected a float32 or float64 field, got {dt}")
        single = len(shape) == 3
        if (shape[1:] if not single else shape) != (ctx.H, ctx.W, 2) or len(shape) not in (3, 4) or (not single and shape[0] < 1):
            raise ValueError(f"push: expected ({ctx.H}, {ctx.W}, 2) or (n, {ctx.H}, {ctx.W}, 2), got {shape}")
        n = 1 if single else shape[0]
        res = np.empty((n, ctx.H, ctx.W, 2), odt)
        if on_dev:
            buf = ctx.alloc(res.nbytes)
            try:
                check(ctx.lib.mav_history_push_dev(ctx.h, self._h, flow.ptr, HISTORY_DEPTHS[dt], n, form, buf.ptr))
                res = buf.download(odt, res.shape)
            finally:
                buf.free()
        else:
            a = np.ascontiguousarray(a)
            check(ctx.lib.mav_history_push(ctx.h, self._h, _ptr(a), HISTORY_DEPTHS[dt], n, form, _ptr(res)))
        return res[0] if single else res

    def push_enqueue(self, flow_ptr, out_ptr, count: int = 1, dtype=np.float32, out: str = "reference") -> None:
        """mav_history_push_dev: enqueue only, device pointers (ints, or objects with a .ptr); `count` fields of `dtype` at flow_ptr,
        `count` results in the `out` form at out_ptr."""
        form, _ = self._out_form(out)
        if np.dtype(dtype) not in HISTORY_DEPTHS:
            raise ValueError(f"push_enqueue: dtype must be float32 or float64, got {np.dtype(dtype)}")
        check(self.ctx.lib.mav_history_push_dev(self.ctx.h, self._h, _dev_ptr(flow_ptr), HISTORY_DEPTHS[np.dtype(dtype)], int(count), form,
                                                _dev_ptr(out_ptr)))

    def reset(self) -> None:
        """Zero ring, index 0 (enqueue only)."""
        check(self.ctx.lib.mav_history_reset(self.ctx.h, self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) and self.ctx.alive:
            check(self.ctx.lib.mav_history_destroy(self.ctx.h, self._h))
        self._h = None                     # (a closed context has freed the ring already)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One mav_ctx: (device, W, H, max_batch, Farneback parameters).

    The methods of the headers beside include/mavflow.h are attached by the module that binds each header, when it is imported:
    mavflow.shapes adds draw_shapes, draw_blob_boxes, add_saturate, mosaic, motion_pictures_enqueue and their *_enqueue twins (as
    mavflow.vis, mavflow.warp, mavflow.resize and the others add theirs).  Import that module before calling them on a Context."""

    def __init__(self, W: int, H: int, max_batch: int = 1, fb: FbParams | None = None, device: int = 0, window="box"):
        self.lib = load()
        self.W, self.H, self.max_batch = int(W), int(H), int(max_batch)
        self.fb = fb if fb is not None else fb_defaults()
        h = C.c_void_p()
        check(self.lib.mav_create(C.byref(h), device, self.W, self.H, self.max_batch, C.byref(self.fb)))
        self._h = h
        self._posted = False                  # steps have been posted to the context's worker thread since the last drain
        if window not in ("box", WINDOW_BOX):
            try:
                self.set_window(window)
            except Exception:
                self.close()
                raise

    # A context is single-threaded.  Once a step has been posted (post_step) the library's worker thread is that thread until it has
    # enqueued everything posted; `h` -- what every other call of this binding passes as the context -- therefore drains the worker
    # first.  post_step / wait_step use the raw handle.
    @property
    def h(self):
        if self._posted:
            self.drain()
        return self._h

    @h.setter
    def h(self, v):
        self._h = v

    @property
    def alive(self) -> bool:
        """Not closed (asks nothing of the worker thread, unlike `h`)."""
        return bool(self._h)

    def post_step(self, step: "FrameStep") -> int:
        """mav_frame_step_post: hand one loop iteration to the context's worker thread; returns its ticket at once.  The caller keeps
        the step's host buffers alive until wait_step(ticket, marker) has returned."""
        t = C.c_uint64()
        check(self.lib.mav_frame_step_post(self._h, C.byref(step), C.byref(t)))
        self._posted = True
        return t.value

    def wait_step(self, ticket: int, marker=None) -> None:
        """The step has been enqueued and, with its record_done marker given, has finished on the device; raises what the step raised."""
        check(self.lib.mav_frame_step_wait(self._h, ticket, marker))

    def drain(self) -> None:
        """Every posted step has been enqueued (mav_worker_drain); raises the first failure among them."""
        self._posted = False
        check(self.lib.mav_worker_drain(self._h))

    def close(self):
        if getattr(self, "_h", None):
            for p in getattr(self, "_pinned", []):
                self.lib.mav_host_free(self._h, p)
            self._pinned = []
            self.lib.mav_destroy(self._h)            # (the worker finishes the step in hand, drops what is still queued, joins)
            self._h = None
            self._posted = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- introspection ---------------------------------------------------------------------------------------
    def set_option(self, name: str, value: int):
        check(self.lib.mav_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_long()
        check(self.lib.mav_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def set_window(self, window) -> None:
        """The sweeps' window: "box" (cv2's default) or "gaussian" (cv2.OPTFLOW_FARNEBACK_GAUSSIAN), or the MAV_WINDOW_* code
        (mav_set_window: drains the context first).  Every call that computes flow follows it from then on."""
        check(self.lib.mav_set_window(self.h, _window_code(window)))

    @property
    def window(self) -> str:
        v = C.c_int()
        check(self.lib.mav_get_window(self.h, C.byref(v)))
        return {code: name for name, code in WINDOWS.items()}[v.value]

    def membw_probe(self, bytes_per_buffer: int, reps: int = 20) -> float:
        """GB/s of a plain 3-reads-1-write streaming kernel over four buffers of that size (calibration for bench.py's roofline)."""
        g = C.c_double()
        check(self.lib.mav_membw_probe(self.h, int(bytes_per_buffer), int(reps), C.byref(g)))
        return g.value

    def schedule_info(self, batch: int, dtype=None) -> dict:
        """The schedule a call of `batch` pairs takes with the options in effect (every option, group split, per-layer plan).
        dtype: the frames' dtype (uint8 / uint16 / float32) -- the per-layer blur form depends on it; None = uint8 (mav_schedule_info)."""
        import json
        buf = C.create_string_buffer(8192)
        if dtype is None:
            check(self.lib.mav_schedule_info(self.h, int(batch), buf, len(buf)))
        else:
            check(self.lib.mav_schedule_info_ex(self.h, int(batch), _depth_of(dtype), buf, len(buf)))
        info = json.loads(buf.value.decode())
        info.setdefault("window", "box")      # the library's line names the window of a Gaussian context only
        return info

    def mem_info(self) -> dict:
        """Device memory in bytes: free / total of the GPU, what this context holds in all, and its Farneback workspace alone
        (0 until a call computes flow)."""
        v = [C.c_size_t() for _ in range(4)]
        check(self.lib.mav_mem_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("dev_free", "dev_total", "ctx_bytes", "workspace_bytes"), (x.value for x in v)))

    def num_layers(self) -> int:
        return self.lib.mav_num_layers(self.h)

    def layer_dims(self, k: int):
        w, h, ks, sg = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        check(self.lib.mav_layer_dims(self.h, k, C.addressof(w), C.addressof(h), C.addressof(ks), C.addressof(sg)))
        return w.value, h.value, sg.value, ks.value

    def sync(self):
        check(self.lib.mav_sync(self.h))

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def pinned_like(self, a: np.ndarray) -> np.ndarray:
        """A page-locked host copy of `a` (numpy view over hipHostMalloc memory; freed with the context)."""
        p = C.c_void_p()
        check(self.lib.mav_host_alloc(self.h, a.nbytes, C.byref(p)))
        self._pinned = getattr(self, "_pinned", []) + [p.value]
        out = np.ctypeslib.as_array((C.c_uint8 * a.nbytes).from_address(p.value)).view(a.dtype).reshape(a.shape)
        out[...] = a
        return out

    def upload_async(self, dst: DeviceBuffer, src: np.ndarray, ordered: bool = True):
        """Copy on the copy stream.  ordered (default): behind everything enqueued on the compute stream so far (safe for a buffer
        set an earlier batch may still read); ordered=False: no wait -- for a destination no enqueued work touches."""
        fn = self.lib.mav_upload_async if ordered else self.lib.mav_upload_async_unordered
        check(fn(self.h, dst.ptr, _ptr(src), src.nbytes))

    def upload_fence(self):
        check(self.lib.mav_upload_fence(self.h))

    # -- host-array entry points -----------------------------------------------------------------------------
    def _imgs(self, a, name):
        a = np.asarray(a)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1:] != (self.H, self.W):
            raise ValueError(f"{name}: expected (batch, {self.H}, {self.W}) u8, got {a.shape}")
        if a.dtype != np.uint8:
            raise ValueError(f"{name}: expected uint8, got {a.dtype}")
        return np.ascontiguousarray(a)

    def _frames(self, a, name):
        """Frames of the Farneback entry points: (batch, H, W) uint8, uint16 or float32, C-contiguous; float64 is rounded to float32
        on the host (cv2's convertTo(CV_32F)).  Any other dtype is a ValueError."""
        a = np.asarray(a)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1:] != (self.H, self.W):
            raise ValueError(f"{name}: expected (batch, {self.H}, {self.W}) frames, got {a.shape}")
        if a.dtype == np.float64:
            a = a.astype(np.float32)
        _depth_of(a.dtype, name)
        return np.ascontiguousarray(a)

    def _flows(self, a, B, name):
        """(H, W, 2) for a batch of one, or (B, H, W, 2): float32, C-contiguous."""
        a = np.asarray(a)
        if a.ndim == 3 and B == 1:
            a = a[None]
        if a.shape != (B, self.H, self.W, 2):
            raise ValueError(f"{name}: expected ({B}, {self.H}, {self.W}, 2) float32, got {a.shape}")
        if a.dtype != np.float32:
            raise ValueError(f"{name}: expected float32, got {a.dtype}")
        return np.ascontiguousarray(a)

    def farneback(self, prev, nxt, initial_flow=None) -> np.ndarray:
        """cv2.calcOpticalFlowFarneback for a batch of pairs -> (B, H, W, 2) float32.  initial_flow: None starts every pair from zero;
        an (H, W, 2) field (one pair) or (B, H, W, 2) fields are the starting flow of each pair, as cv2 takes `flow` with
        OPTFLOW_USE_INITIAL_FLOW set (mav_farneback_init).  Frames: uint8, uint16 or float32 (float64 is narrowed on the host, as
        cv2's convertTo does), prev and next of ONE dtype -- unlike cv2, which converts each frame on its own; no rescaling."""
        prev, nxt = np.asarray(prev), np.asarray(nxt)
        if prev.dtype != nxt.dtype:
            raise ValueError(f"prev and next differ in dtype ({prev.dtype} vs {nxt.dtype})")
        prev, nxt = self._frames(prev, "prev"), self._frames(nxt, "next")
        if prev.shape != nxt.shape:
            raise ValueError("prev and next differ in shape")
        B = prev.shape[0]
        init = None if initial_flow is None else self._flows(initial_flow, B, "initial_flow")
        flow = _pinned.empty(self, (B, self.H, self.W, 2), np.float32)
        if prev.dtype != np.uint8:
            check(self.lib.mav_farneback_ex(self.h, _ptr(prev), _ptr(nxt), DEPTHS[prev.dtype], B, None if init is None else _ptr(init),
                                            _ptr(flow)))
        elif init is None:
            check(self.lib.mav_farneback(self.h, _ptr(prev), _ptr(nxt), B, _ptr(flow)))
        else:
            check(self.lib.mav_farneback_init(self.h, _ptr(prev), _ptr(nxt), B, _ptr(init), _ptr(flow)))
        return flow

    def farneback_chain(self, frames, initial_flow=None) -> np.ndarray:
        """cv2's video idiom over a run of frames (n + 1, H, W) u8 -> (n, H, W, 2) float32:
            flow = calcOpticalFlowFarneback(f[i], f[i + 1], flow, ..., flags | OPTFLOW_USE_INITIAL_FLOW)
        pair i starts from pair i - 1's flow, pair 0 from initial_flow ((H, W, 2) float32) or from zero when it is None.  The run is
        uploaded once, the n one-pair calls keep their input and output flow on the device, and one download brings all n back."""
        frames = self._frames(frames, "frames")
        n = frames.shape[0] - 1
        if n < 1:
            raise ValueError("a chain needs at least two frames")
        init = None if initial_flow is None else self._flows(initial_flow, 1, "initial_flow")
        fbytes, px = self.H * self.W * 2 * 4, self.H * self.W * frames.itemsize
        d_frames = self.alloc(frames.nbytes).upload(frames)
        d_flow = self.alloc(n * fbytes)
        depth = DEPTHS[frames.dtype]

        def run(i, f_init, f_out):                    # pair (frame i, frame i + 1): u8 through the u8 symbols, as before
            a, b = d_frames.ptr + i * px, d_frames.ptr + (i + 1) * px
            if depth != DEPTH_8U:
                check(self.lib.mav_farneback_ex_dev(self.h, a, b, depth, 1, f_init, f_out))
            elif f_init is None:
                check(self.lib.mav_farneback_dev(self.h, a, b, 1, f_out))
            else:
                check(self.lib.mav_farneback_init_dev(self.h, a, b, 1, f_init, f_out))
        try:
            if init is None:                          # zero start: the flags = 0 call (bit-identical to an all-zero initial flow)
                run(0, None, d_flow.ptr)
            else:
                check(self.lib.mav_memcpy_h2d(self.h, d_flow.ptr, _ptr(init), fbytes))
                run(0, d_flow.ptr, d_flow.ptr)
            for i in range(1, n):
                run(i, d_flow.ptr + (i - 1) * fbytes, d_flow.ptr + i * fbytes)
            return d_flow.download(np.float32, (n, self.H, self.W, 2))
        finally:
            self.sync()
            d_flow.free()
            d_frames.free()

    def farneback_sequence(self, frames) -> np.ndarray:
        """Flow of every consecutive pair of a run of frames (n + 1, H, W) u8 -> (n, H, W, 2) float32.  The two batches handed to
        the library are views of the one array (next = prev + one frame), which it recognises: the run is uploaded once and every
        frame is blurred and expanded once instead of twice.  Same flow, bit for bit, as farneback(frames[:-1], frames[1:]) on
        separate copies."""
        frames = self._frames(frames, "frames")
        if frames.shape[0] < 2:
            raise ValueError("a sequence needs at least two frames")
        return self.farneback(frames[:-1], frames[1:])

    def derotate(self, flow, omega, dt) -> np.ndarray:
        flow = np.asarray(flow, np.float32)
        flow = flow[None] if flow.ndim == 3 else flow
        B = flow.shape[0]
        flow = _arr(flow, np.float32, (B, self.H, self.W, 2), "flow")
        omega = _arr(np.asarray(omega, np.float64).reshape(B, 3), np.float64)
        dt = _arr(np.asarray(dt, np.float64).reshape(B), np.float64)
        out = np.empty((B, self.H, self.W, 2), np.float64)
        check(self.lib.mav_derotate(self.h, _ptr(flow), _ptr(omega), _ptr(dt), B, _ptr(out)))
        return out

    def foe_dense(self, flow, samples, params: FoeParams | None = None) -> np.ndarray:
        """get_FOE_dense + ransac.  The arithmetic follows the array's dtype as numpy's does in the reference: a float32
        field (frame index 0, never derotated) has its |flow2| gate evaluated in float32, anything else runs in double."""
        flow = np.asarray(flow)
        f32 = flow.dtype == np.float32
        if not f32:
            flow = np.asarray(flow, np.float64)
        flow = flow[None] if flow.ndim == 3 else flow
        B = flow.shape[0]
        p = params or foe_defaults()
        flow = _arr(flow, flow.dtype, (B, self.H, self.W, 2), "flow")
        samples = _arr(np.asarray(samples).reshape(B, 2 * p.n_pairs, 2), np.uint32)
        foe = np.empty((B, 2), np.float64)
        fn = self.lib.mav_foe_dense_f32 if f32 else self.lib.mav_foe_dense
        check(fn(self.h, _ptr(flow), _ptr(samples), B, C.byref(p), _ptr(foe)))
        return foe

    def ransac(self, estimates, ransac_threshold: float = 30.0):
        est = _arr(np.asarray(estimates, np.float64).reshape(-1, 2), np.float64)
        foe = np.empty(2, np.float64)
        check(self.lib.mav_ransac(self.h, _ptr(est) if est.shape[0] else None, est.shape[0], float(ransac_threshold), _ptr(foe)))
        return (float(foe[0]), float(foe[1]))

    def bgr2gray(self, bgr) -> np.ndarray:
        a = np.asarray(bgr)
        a = a[None] if a.ndim == 3 else a
        a = _arr(a, np.uint8, (a.shape[0], self.H, self.W, 3), "bgr")
        gray = np.empty((a.shape[0], self.H, self.W), np.uint8)
        check(self.lib.mav_bgr2gray(self.h, _ptr(a), a.shape[0], _ptr(gray)))
        return gray

    def phi_mask(self, flow, foe, sky=None, params: ThrParams | None = None, want_phi=True):
        """get_phi + the threshold block.  dtype in = dtype of the arithmetic and of phi, as in the reference: float32 flow
        (frame index 0) -> float32 phi, float64 flow -> float64 phi."""
        flow = np.asarray(flow)
        f32 = flow.dtype == np.float32
        ft = np.float32 if f32 else np.float64
        flow = np.asarray(flow, ft)
        flow = flow[None] if flow.ndim == 3 else flow
        B = flow.shape[0]
        flow = _arr(flow, ft, (B, self.H, self.W, 2), "flow")
        foe = _arr(np.asarray(foe, np.float64).reshape(B, 2), np.float64)
        sky = None if sky is None else _arr(np.asarray(sky).reshape(B, self.H, self.W).astype(np.uint8), np.uint8)
        p = params or thr_defaults()
        phi = np.empty((B, self.H, self.W), ft) if want_phi else None
        mf = np.empty((B, self.H, self.W), np.uint8)
        md = np.empty((B, self.H, self.W), np.uint8)
        mx = np.empty(B, ft) if want_phi else None      # max(phi) needs the exact path, like phi itself
        fn = self.lib.mav_phi_mask_f32 if f32 else self.lib.mav_phi_mask
        check(fn(self.h, _ptr(flow), _ptr(foe), _ptr(sky), B, C.byref(p), _ptr(phi), _ptr(mf), _ptr(md), _ptr(mx)))
        return phi, mf.view(np.bool_), md.view(np.bool_), mx

    def bbox(self, img) -> np.ndarray:
        img = self._imgs(img, "img")
        box = np.empty((img.shape[0], 4), np.int32)
        check(self.lib.mav_bbox(self.h, _ptr(img), img.shape[0], _ptr(box)))
        return box

    def window_max(self, img) -> np.ndarray:
        img = self._imgs(img, "img")
        out = np.empty((img.shape[0], 3), np.int64)
        check(self.lib.mav_window_max(self.h, _ptr(img), img.shape[0], _ptr(out)))
        return out

    def pyramid_dims(self, scale: float = 1.5):
        """[(w, h)] of every level of im_helpers.pyramid for this frame size."""
        n = self.lib.mav_pyramid_levels(self.h, scale)
        if n < 0:
            check(n)
        dims = []
        for l in range(n):
            w, h = C.c_int(), C.c_int()
            check(self.lib.mav_pyramid_dims(self.h, scale, l, C.byref(w), C.byref(h)))
            dims.append((w.value, h.value))
        return dims

    def analyze_pyramid(self, img, scale: float = 1.5) -> np.ndarray:
        """(batch, 6) int64: score, x, y, level, argmax_row, argmax_col (detector.py:280-312, all levels)."""
        img = self._imgs(img, "img")
        out = np.empty((img.shape[0], 6), np.int64)
        check(self.lib.mav_analyze_pyramid(self.h, _ptr(img), img.shape[0], scale, _ptr(out)))
        return out

    def pyramid_level(self, img, level: int, scale: float = 1.5) -> np.ndarray:
        img = self._imgs(img, "img")
        w, h = C.c_int(), C.c_int()
        check(self.lib.mav_pyramid_dims(self.h, scale, level, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value), np.uint8)
        check(self.lib.mav_stage_pyramid_level(self.h, _ptr(img[:1]), scale, level, _ptr(out)))
        return out

    def optimize_window(self, img, windows):
        """Detector.optimize_window (detector.py:314-358): windows (batch, 4) = x, y, w, h -> (scores int64, windows int32)."""
        img = self._imgs(img, "img")
        B = img.shape[0]
        win = _arr(np.asarray(windows).reshape(B, 4), np.int32)
        score = np.empty(B, np.int64)
        out = np.empty((B, 4), np.int32)
        check(self.lib.mav_optimize_window(self.h, _ptr(img), B, _ptr(win), _ptr(score), _ptr(out)))
        return score, out

    def tpr_fpr_counts(self, gt, mask, mask_value: int = 255) -> np.ndarray:
        """(batch, 4) = positives, negatives, true positives, false positives of calculate_tpr_fpr(gt, mask_value * mask)."""
        gt = self._imgs(gt, "gt")
        mask = self._imgs(np.asarray(mask).astype(np.uint8), "mask")
        out = np.empty((gt.shape[0], 4), np.int64)
        check(self.lib.mav_tpr_fpr_counts(self.h, _ptr(gt), _ptr(mask), int(mask_value), gt.shape[0], _ptr(out)))
        return out

    # -- blob detections: connected components of masks (include/mavflow.h: mav_components) ----------------------
    @staticmethod
    def _cc_result(B, p, labels, counts, table):
        """The call's arrays as the dict the three forms return: the table trimmed per image to min(n_blobs, max_blobs) records."""
        out = dict(n_components=counts["n_components"].copy(), n_blobs=counts["n_blobs"].copy(),
                   blobs=[table[b, :min(int(counts["n_blobs"][b]), p.max_blobs)] for b in range(B)])
        if labels is not None:
            out["labels"] = labels
        return out

    def components(self, mask, connectivity: int = 8, min_area: int = 1, max_blobs: int = 256, labels: bool = False) -> dict:
        """Connected components of (batch, H, W) masks (bool or u8; any non-zero byte is set): n_components, n_blobs (batch) int32,
        blobs = per image the records (BLOB_DTYPE) of the first min(n_blobs, max_blobs) components with area >= min_area in label
        order, and with labels=True the (batch, H, W) int32 label image, numbered as scipy.ndimage.label does (not as cv2 does)."""
        mask = np.asarray(mask)
        mask = self._imgs(mask.view(np.uint8) if mask.dtype == np.bool_ else mask, "mask")
        B = mask.shape[0]
        p = cc_defaults(connectivity=connectivity, min_area=min_area, max_blobs=max_blobs)
        lab = np.empty((B, self.H, self.W), np.int32) if labels else None
        counts, table = np.empty(B, CC_COUNTS_DTYPE), np.empty((B, max(1, p.max_blobs)), BLOB_DTYPE)
        check(self.lib.mav_components(self.h, _ptr(mask), B, C.byref(p), _ptr(lab), _ptr(counts), _ptr(table)))
        return self._cc_result(B, p, lab, counts, table)

    def components_last(self, batch: int, which: str = "fixed", connectivity: int = 8, min_area: int = 1, max_blobs: int = 256,
                        labels: bool = False) -> dict:
        """components() of the fixed or dynamic mask the most recent detect / process_batch / phi_mask call left on the device."""
        if which not in ("fixed", "dynamic"):
            raise ValueError(f"which must be 'fixed' or 'dynamic', got {which!r}")
        B = int(batch)
        p = cc_defaults(connectivity=connectivity, min_area=min_area, max_blobs=max_blobs)
        lab = np.empty((B, self.H, self.W), np.int32) if labels else None
        counts, table = np.empty(max(B, 1), CC_COUNTS_DTYPE), np.empty((max(B, 1), max(1, p.max_blobs)), BLOB_DTYPE)
        check(self.lib.mav_last_masks_components(self.h, int(which == "dynamic"), B, C.byref(p), _ptr(lab), _ptr(counts), _ptr(table)))
        return self._cc_result(B, p, lab, counts, table)

    def components_dev(self, mask_ptr, batch: int, counts_ptr, blobs_ptr, labels_ptr=None, connectivity: int = 8, min_area: int = 1,
                       max_blobs: int = 256) -> None:
        """mav_components_dev: enqueue only, device pointers (ints, or objects with a .ptr such as DeviceBuffer / DeviceArray);
        counts (batch) CC_COUNTS_DTYPE, blobs (batch, max_blobs) BLOB_DTYPE, labels (batch, H, W) int32 or None."""
        p = cc_defaults(connectivity=connectivity, min_area=min_area, max_blobs=max_blobs)
        raw = [getattr(x, "ptr", x) for x in (mask_ptr, labels_ptr, counts_ptr, blobs_ptr)]
        check(self.lib.mav_components_dev(self.h, raw[0], int(batch), C.byref(p), raw[1], raw[2], raw[3]))

    def _detect_args(self, B, samples, omega, dt, frame0, sky, fp):
        samples = _arr(np.asarray(samples).reshape(B, 2 * fp.n_pairs, 2), np.uint32)
        omega = None if omega is None else _arr(np.asarray(omega, np.float64).reshape(B, 3), np.float64)
        dt = None if dt is None else _arr(np.asarray(dt, np.float64).reshape(B), np.float64)
        frame0 = None if frame0 is None else _arr(np.asarray(frame0).reshape(B).astype(np.uint8), np.uint8)
        sky = None if sky is None else _arr(np.asarray(sky).reshape(B, self.H, self.W).astype(np.uint8), np.uint8)
        return samples, omega, dt, frame0, sky

    def last_masks_tpr_fpr(self, gt, mask_value: int = 255):
        """calculate_tpr_fpr counts of BOTH masks of the most recent detect / process_batch / phi_mask call, taken where they
        still are (on the device): ((batch, 4) fixed, (batch, 4) dynamic) = positives, negatives, true / false positives."""
        gt = self._imgs(gt, "gt")
        B = gt.shape[0]
        cf, cd = np.empty((B, 4), np.int64), np.empty((B, 4), np.int64)
        check(self.lib.mav_last_masks_tpr_fpr(self.h, _ptr(gt), int(mask_value), B, _ptr(cf), _ptr(cd)))
        return cf, cd

    def process_batch(self, prev, nxt, samples, omega=None, dt=None, sky=None, foe_params=None, thr_params=None,
                      want_flow=True, want_phi=False, want_masks=True, frame0=None):
        """Fused loop body of Processor.run_detection (processor.py:305-341) for a batch of pairs.  frame0: per-pair flags of
        the reference's frame index 0 (no derotation, float32 arithmetic; detector.py:80-81)."""
        prev, nxt = self._imgs(prev, "prev"), self._imgs(nxt, "next")
        B = prev.shape[0]
        fp = foe_params or foe_defaults()
        tp = thr_params or thr_defaults()
        samples, omega, dt, frame0, sky = self._detect_args(B, samples, omega, dt, frame0, sky, fp)
        flow = _pinned.empty(self, (B, self.H, self.W, 2), np.float32) if want_flow else None
        phi = _pinned.empty(self, (B, self.H, self.W), np.float64) if want_phi else None
        mf = _pinned.empty(self, (B, self.H, self.W), np.uint8) if want_masks else None
        md = _pinned.empty(self, (B, self.H, self.W), np.uint8) if want_masks else None
        res = np.empty(B, RESULT_DTYPE)
        check(self.lib.mav_process_batch(self.h, _ptr(prev), _ptr(nxt), _ptr(samples), _ptr(omega), _ptr(dt), _ptr(frame0), _ptr(sky),
                                         B, C.byref(fp), C.byref(tp), _ptr(flow), _ptr(phi), _ptr(mf), _ptr(md), _ptr(res)))
        return dict(flow=flow, phi=phi, mask_fixed=None if mf is None else mf.view(np.bool_),
                    mask_dyn=None if md is None else md.view(np.bool_), results=res)

    def detect(self, flow, samples, omega=None, dt=None, sky=None, foe_params=None, thr_params=None, want_phi=False,
               want_masks=True, frame0=None):
        """processor.py:305-341 from the reference's own flow seam: a float32 (B, H, W, 2) field (Dataset.get_flow_uv) in,
        derotation -> FoE -> phi -> masks -> box on the device, masks and records out.
        The field must BE float32 (what .flo files and Farneback give): the reference evaluates a float64 field in float64 from the
        start, which this fused call does not do -- such input goes through derotate / foe_dense / phi_mask (the float64 kernels),
        as Processor.run_detection does by itself."""
        flow = np.asarray(flow)
        if flow.dtype != np.float32:
            raise TypeError(f"detect() takes a float32 flow field, got {flow.dtype}: narrowing would change FoE and masks against the "
                            "reference; use derotate / foe_dense / phi_mask for float64 fields")
        flow = flow[None] if flow.ndim == 3 else flow
        B = flow.shape[0]
        flow = _arr(flow, np.float32, (B, self.H, self.W, 2), "flow")
        fp = foe_params or foe_defaults()
        tp = thr_params or thr_defaults()
        samples, omega, dt, frame0, sky = self._detect_args(B, samples, omega, dt, frame0, sky, fp)
        phi = _pinned.empty(self, (B, self.H, self.W), np.float64) if want_phi else None
        mf = _pinned.empty(self, (B, self.H, self.W), np.uint8) if want_masks else None
        md = _pinned.empty(self, (B, self.H, self.W), np.uint8) if want_masks else None
        res = np.empty(B, RESULT_DTYPE)
        check(self.lib.mav_detect(self.h, _ptr(flow), _ptr(samples), _ptr(omega), _ptr(dt), _ptr(frame0), _ptr(sky), B,
                                  C.byref(fp), C.byref(tp), _ptr(phi), _ptr(mf), _ptr(md), _ptr(res)))
        return dict(phi=phi, mask_fixed=None if mf is None else mf.view(np.bool_),
                    mask_dyn=None if md is None else md.view(np.bool_), results=res)

    # -- result images (processor.py:364-374) ---------------------------------------------------------------
    IMAGES = ("result", "flow", "phi")

    def _image_outs(self, B, images):
        bad = set(images) - set(self.IMAGES)
        if bad:
            raise ValueError(f"unknown image(s) {sorted(bad)}; choose from {self.IMAGES}")
        return {k: (np.empty((B, self.H, self.W, 3), np.uint8) if k in images else None) for k in self.IMAGES}

    def render(self, flow, foe, omega=None, dt=None, sky=None, thr_params=None, frame0=None, images=IMAGES):
        """The three images Processor.run_detection writes per frame, as (B, H, W, 3) u8 BGR arrays: "result" (to_rgb of
        255 * the fixed mask), "flow" (get_flow_vis of the derotated flow), "phi" (apply_colormap of to_rgb(phi, 180)).
        flow: float32 (B, H, W, 2) as for detect(); foe (B, 2); omega / dt / sky / frame0 as for detect()."""
        flow = np.asarray(flow)
        if flow.dtype != np.float32:
            raise TypeError(f"render() takes a float32 flow field, got {flow.dtype}")
        flow = flow[None] if flow.ndim == 3 else flow
        B = flow.shape[0]
        flow = _arr(flow, np.float32, (B, self.H, self.W, 2), "flow")
        foe = _arr(np.asarray(foe, np.float64).reshape(B, 2), np.float64)
        omega = None if omega is None else _arr(np.asarray(omega, np.float64).reshape(B, 3), np.float64)
        dt = None if dt is None else _arr(np.asarray(dt, np.float64).reshape(B), np.float64)
        frame0 = None if frame0 is None else _arr(np.asarray(frame0).reshape(B).astype(np.uint8), np.uint8)
        sky = None if sky is None else _arr(np.asarray(sky).reshape(B, self.H, self.W).astype(np.uint8), np.uint8)
        tp = thr_params or thr_defaults()
        out = self._image_outs(B, images)
        check(self.lib.mav_render(self.h, _ptr(flow), _ptr(foe), _ptr(omega), _ptr(dt), _ptr(frame0), _ptr(sky), B, C.byref(tp),
                                  _ptr(out["result"]), _ptr(out["flow"]), _ptr(out["phi"])))
        return {k: v for k, v in out.items() if v is not None}

    def render_dev(self, flow_ptr, foe_ptr, batch, result_ptr=None, flow_img_ptr=None, phi_img_ptr=None, omega_ptr=None, dt_ptr=None,
                   frame0_ptr=None, sky_ptr=None, thr_params=None):
        """mav_render_dev: enqueue only, device pointers."""
        tp = thr_params or thr_defaults()
        check(self.lib.mav_render_dev(self.h, flow_ptr, foe_ptr, omega_ptr, dt_ptr, frame0_ptr, sky_ptr, batch, C.byref(tp), result_ptr,
                                      flow_img_ptr, phi_img_ptr))

    def render_last(self, batch: int, images=IMAGES):
        """render() of what the most recent detect / process_batch(_dev) / frame step left on the device (flow, FoE, sky,
        derotation, thresholds): nothing but the images crosses PCIe."""
        out = self._image_outs(batch, images)
        check(self.lib.mav_last_render(self.h, int(batch), _ptr(out["result"]), _ptr(out["flow"]), _ptr(out["phi"])))
        return {k: v for k, v in out.items() if v is not None}

    # -- threshold sweep (include/mavflow.h: mav_roc_sweep) ------------------------------------------------------
    def _roc_gt(self, gt, B):
        """(gt array (gt_images, H, W) u8, gt_images): one image per pair, or one 2-D image shared by every pair"""
        gt = np.asarray(gt)
        shared = gt.ndim == 2
        gt = self._imgs(gt, "gt")
        if not shared and gt.shape[0] != B:
            raise ValueError(f"gt: {gt.shape[0]} images for {B} pairs (a 2-D image is shared by every pair)")
        return gt, (1 if shared else B)

    def roc_sweep(self, flow, foe, gt, angles, mags, omega=None, dt=None, sky=None, frame0=None, thr_params=None) -> dict:
        """The fixed mask's TPR / FPR counts at every (angle, magnitude) pair in one pass: counts (B, Ka, Km, 4) int64 = pos, neg, tp,
        fp, where counts[b, i, j] is tpr_fpr_counts(gt, fixed mask at fixed_deg = angles[i], fixed_min_mag = mags[j])[b].  flow / foe /
        omega / dt / sky / frame0 as for render(); gt (B, H, W) u8, or (H, W) = one image shared by every pair."""
        flow = np.asarray(flow)
        if flow.dtype != np.float32:
            raise TypeError(f"roc_sweep() takes a float32 flow field, got {flow.dtype}")
        flow = flow[None] if flow.ndim == 3 else flow
        B = flow.shape[0]
        flow = _arr(flow, np.float32, (B, self.H, self.W, 2), "flow")
        foe = _arr(np.asarray(foe, np.float64).reshape(B, 2), np.float64)
        omega = None if omega is None else _arr(np.asarray(omega, np.float64).reshape(B, 3), np.float64)
        dt = None if dt is None else _arr(np.asarray(dt, np.float64).reshape(B), np.float64)
        frame0 = None if frame0 is None else _arr(np.asarray(frame0).reshape(B).astype(np.uint8), np.uint8)
        sky = None if sky is None else _arr(np.asarray(sky).reshape(B, self.H, self.W).astype(np.uint8), np.uint8)
        gt, gt_images = self._roc_gt(gt, B)
        tp = thr_params or thr_defaults()
        p, a, m = roc_params(angles, mags)
        table = np.empty((B, roc_table_words(a.size, m.size)), np.int64)
        check(self.lib.mav_roc_sweep(self.h, _ptr(flow), _ptr(foe), _ptr(omega), _ptr(dt), _ptr(frame0), _ptr(sky), _ptr(gt), gt_images, B,
                                     C.byref(tp), C.byref(p), _ptr(table)))
        return dict(counts=roc_expand(table, a.size, m.size), angles=a, mags=m)

    def roc_sweep_last(self, batch: int, gt, angles, mags) -> dict:
        """roc_sweep() of what the most recent detect / process_batch(_dev) / frame step left on the device (flow, FoE, sky,
        derotation): only the ground truth goes up and the tables come down."""
        B = int(batch)
        gt, gt_images = self._roc_gt(gt, B)
        p, a, m = roc_params(angles, mags)
        table = np.empty((max(B, 1), roc_table_words(a.size, m.size)), np.int64)
        check(self.lib.mav_last_roc_sweep(self.h, _ptr(gt), gt_images, B, C.byref(p), _ptr(table)))
        return dict(counts=roc_expand(table[:B], a.size, m.size), angles=a, mags=m)

    def roc_sweep_dev(self, flow_ptr, foe_ptr, gt_ptr, gt_images: int, batch: int, angles, mags, table_ptr, omega_ptr=None, dt_ptr=None,
                      frame0_ptr=None, sky_ptr=None, thr_params=None) -> None:
        """mav_roc_sweep_dev: enqueue only, device pointers (ints, or objects with a .ptr); table (batch, roc_table_words) int64."""
        tp = thr_params or thr_defaults()
        p, a, m = roc_params(angles, mags)
        raw = [getattr(x, "ptr", x) for x in (flow_ptr, foe_ptr, omega_ptr, dt_ptr, frame0_ptr, sky_ptr, gt_ptr, table_ptr)]
        check(self.lib.mav_roc_sweep_dev(self.h, *raw[:7], int(gt_images), int(batch), C.byref(tp), C.byref(p), raw[7]))

    def roc_arm(self, angles, mags=None, off_table: int = 0) -> None:
        """mav_roc_arm: while armed, every frame step with a ground truth also writes its pairs' sweep tables at out_dev + off_table.
        roc_arm(None) disarms.  The state is the context's, one for all its users: roc_state is what this binding last armed
        (angles bytes, mags bytes, off_table; None = disarmed), by which the pipelines that share a context see whose it is."""
        if angles is None:
            check(self.lib.mav_roc_arm(self.h, None, 0))
            self.roc_state = None
            return
        p, a, m = roc_params(angles, mags)
        check(self.lib.mav_roc_arm(self.h, C.byref(p), int(off_table)))
        self.roc_state = (a.tobytes(), m.tobytes(), int(off_table))

    roc_state = None

    def flow_history(self, length: int = 20, dtype=np.float32, axes: str = "reference") -> FlowHistory:
        """A flow history on this context (mav_history_create): ring of `length` fields (3 .. 64) of `dtype` (float32 / float64), zeroed;
        axes="reference" keeps the reference's channel order (the flow's x component is added to the row), "xy" the geometric one."""
        return FlowHistory(self, length, dtype, axes)

    def stage_remap_linear(self, src, map_x, map_y) -> np.ndarray:
        """mav_stage_remap_linear: cv2.remap(src, map_x, map_y, INTER_LINEAR) as the library restates it, of one (H, W, 2) float32 or
        float64 field at (H, W) float32 maps -> (H, W, 2) float64."""
        src = np.ascontiguousarray(src)
        if src.dtype not in HISTORY_DEPTHS or src.shape != (self.H, self.W, 2):
            raise ValueError(f"stage_remap_linear: expected ({self.H}, {self.W}, 2) float32 or float64, got {src.shape} {src.dtype}")
        mx, my = _arr(map_x, np.float32, (self.H, self.W), "map_x"), _arr(map_y, np.float32, (self.H, self.W), "map_y")
        out = np.empty((self.H, self.W, 2), np.float64)
        check(self.lib.mav_stage_remap_linear(self.h, _ptr(src), HISTORY_DEPTHS[src.dtype], _ptr(mx), _ptr(my), _ptr(out)))
        return out

    def flow_to_color(self, flow) -> np.ndarray:
        """flow_vis.flow_to_color(flow, convert_to_bgr=True) of (B, H, W, 2) fields in their own float type -> (B, H, W, 3) u8."""
        flow = np.asarray(flow)
        f64 = flow.dtype != np.float32
        ft = np.float64 if f64 else np.float32
        flow = flow[None] if flow.ndim == 3 else flow
        B = flow.shape[0]
        flow = _arr(flow, ft, (B, self.H, self.W, 2), "flow")
        out = np.empty((B, self.H, self.W, 3), np.uint8)
        check(self.lib.mav_flow_to_color(self.h, _ptr(flow), int(f64), B, _ptr(out)))
        return out

    # -- global-motion subtraction (detector.py:119-202) ----------------------------------------------------------------------------
    def find_homography(self, src, dst):
        """The fit of cv2.findHomography(src, dst) with method 0 as include/mavflow.h describes it (not pinned against cv2): src, dst
        (n, 2) or (batch, n, 2) (x, y) -> (H (batch, 3, 3) float64 with H[2, 2] == 1, ok (batch) int32).  ok == 0: the pairs do not
        determine a homography, H is zero."""
        src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
        if src.ndim == 2:
            src, dst = src[None], dst[None]
        if src.ndim != 3 or src.shape[2] != 2 or src.shape != dst.shape:
            raise ValueError(f"find_homography: expected two (batch, n, 2) arrays, got {src.shape} and {dst.shape}")
        B, n = src.shape[:2]
        src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
        H, ok = np.empty((B, 3, 3), np.float64), np.empty(B, np.int32)
        check(self.lib.mav_find_homography(self.h, _ptr(src), _ptr(dst), n, B, _ptr(H), _ptr(ok)))
        return H, ok

    @staticmethod
    def _coords(coords) -> np.ndarray:
        c = np.asarray(coords)
        if c.ndim != 2 or c.shape[1] != 2 or not np.issubdtype(c.dtype, np.integer):
            raise ValueError(f"coords: expected (n, 2) integers (x, y), got {c.dtype} {c.shape}")
        return np.ascontiguousarray(c, dtype=np.int32)

    def flow_homography(self, flow, coords, want_pairs: bool = False):
        """Detector.get_transformation_matrix for HOMOGRAPHY (detector.py:126-139): the pairs coords -> coords + flow[y, x] of
        float32 fields (B, H, W, 2), then find_homography.  -> (H, ok), and with want_pairs the (B, n, 2) float64 coords_new."""
        flow = np.asarray(flow)
        flow = flow[None] if flow.ndim == 3 else flow
        flow = self._flows(flow, flow.shape[0], "flow")
        coords = self._coords(coords)
        B, n = flow.shape[0], coords.shape[0]
        H, ok = np.empty((B, 3, 3), np.float64), np.empty(B, np.int32)
        pairs = np.empty((B, n, 2), np.float64) if want_pairs else None
        check(self.lib.mav_flow_homography(self.h, _ptr(flow), _ptr(coords), n, B, _ptr(H), _ptr(ok), _ptr(pairs)))
        return (H, ok, pairs) if want_pairs else (H, ok)

    MOTION_OUTPUTS = ("warped", "mag", "gray")

    def global_motion(self, flow, M, optimize: bool = False, outputs=("gray",), scale: float = 1.5) -> dict:
        """Detector.flow_vec_subtract without its renderings (detector.py:164-192) for float32 fields (B, H, W, 2) and matrices M
        (B, 2 or 3, 3) float64 (rows 0 and 1 are read): dict(results = (B,) MOTION_DTYPE records, and of `outputs` "warped" (B, H, W, 2)
        float32, "mag" (B, H, W) float32, "gray" (B, H, W) u8 -- one channel of cluster_vis)."""
        bad = set(outputs) - set(self.MOTION_OUTPUTS)
        if bad:
            raise ValueError(f"unknown output(s) {sorted(bad)}; choose from {self.MOTION_OUTPUTS}")
        flow = np.asarray(flow)
        flow = flow[None] if flow.ndim == 3 else flow
        B = flow.shape[0]
        flow = self._flows(flow, B, "flow")
        M = np.asarray(M, np.float64)
        M = M[None] if M.ndim == 2 else M
        if M.ndim != 3 or M.shape[0] != B or M.shape[1] not in (2, 3) or M.shape[2] != 3:
            raise ValueError(f"M: expected ({B}, 2 or 3, 3) float64, got {M.shape}")
        M6 = np.ascontiguousarray(M[:, :2, :])
        res = np.empty(B, MOTION_DTYPE)
        out = dict(warped=np.empty((B, self.H, self.W, 2), np.float32) if "warped" in outputs else None,
                   mag=np.empty((B, self.H, self.W), np.float32) if "mag" in outputs else None,
                   gray=np.empty((B, self.H, self.W), np.uint8) if "gray" in outputs else None)
        check(self.lib.mav_global_motion(self.h, _ptr(flow), _ptr(M6), B, scale, int(bool(optimize)), _ptr(out["warped"]), _ptr(out["mag"]),
                                         _ptr(out["gray"]), _ptr(res)))
        got = {k: v for k, v in out.items() if v is not None}
        got["results"] = res
        return got

    def global_motion_step(self, flow_ptr, coords, batch: int, results_ptr, optimize: bool = False, H_ptr=None, ok_ptr=None, gray_ptr=None,
                           scale: float = 1.5):
        """mav_global_motion_step_dev: gather, fit, subtract and window search of device-resident flow, enqueue only.  coords: host
        (n, 2) integers; the other arguments are device pointers (results: batch MOTION_DTYPE records)."""
        coords = self._coords(coords)
        check(self.lib.mav_global_motion_step_dev(self.h, flow_ptr, _ptr(coords), coords.shape[0], int(batch), scale, int(bool(optimize)),
                                                  H_ptr, ok_ptr, gray_ptr, results_ptr))

    MOTION_BATCH_OUTPUTS = ("flow", "gray")

    def global_motion_batch(self, prev, nxt, coords, optimize: bool = False, outputs=(), scale: float = 1.5) -> dict:
        """processor.py:286-303 for a batch of u8 frame pairs (B, H, W) as one call (mav_global_motion_batch): Farneback, the pairs at
        coords (n, 2) integers (x, y), the homography fit, the subtraction, the normalised image and the window search.  Views of one
        run of frames (prev = f[:-1], nxt = f[1:]) are recognised as in farneback_sequence.  -> dict(results = (B,) MOTION_DTYPE
        records -- all zero for an item whose fit failed --, H (B, 3, 3) float64, ok (B,) int32, and of `outputs` "flow" (B, H, W, 2)
        float32 and "gray" (B, H, W) u8)."""
        bad = set(outputs) - set(self.MOTION_BATCH_OUTPUTS)
        if bad:
            raise ValueError(f"unknown output(s) {sorted(bad)}; choose from {self.MOTION_BATCH_OUTPUTS}")
        prev, nxt = self._imgs(prev, "prev"), self._imgs(nxt, "next")
        if prev.shape != nxt.shape:
            raise ValueError("prev and next differ in shape")
        coords = self._coords(coords)
        B = prev.shape[0]
        got = dict(results=np.empty(B, MOTION_DTYPE), H=np.empty((B, 3, 3), np.float64), ok=np.empty(B, np.int32))
        flow = np.empty((B, self.H, self.W, 2), np.float32) if "flow" in outputs else None
        gray = np.empty((B, self.H, self.W), np.uint8) if "gray" in outputs else None
        check(self.lib.mav_global_motion_batch(self.h, _ptr(prev), _ptr(nxt), _ptr(coords), coords.shape[0], B, scale, int(bool(optimize)),
                                               _ptr(flow), _ptr(got["H"]), _ptr(got["ok"]), _ptr(gray), _ptr(got["results"])))
        if flow is not None:
            got["flow"] = flow
        if gray is not None:
            got["gray"] = gray
        return got

    def global_motion_batch_dev(self, prev_ptr, next_ptr, coords, batch: int, results_ptr, optimize: bool = False, flow_ptr=None, H_ptr=None,
                                ok_ptr=None, gray_ptr=None, scale: float = 1.5):
        """mav_global_motion_batch_dev: the same for device-resident frames, enqueue only.  coords: host (n, 2) integers; the other
        arguments are device pointers (flow_ptr None: the context's own flow buffer, last_flow() reads it)."""
        coords = self._coords(coords)
        check(self.lib.mav_global_motion_batch_dev(self.h, prev_ptr, next_ptr, _ptr(coords), coords.shape[0], int(batch), scale,
                                                   int(bool(optimize)), flow_ptr, H_ptr, ok_ptr, gray_ptr, results_ptr))

    MOTION_IMAGES = ("warped", "global")

    def render_last_global_motion(self, batch: int, images=MOTION_IMAGES) -> dict:
        """get_flow_vis of flow_uv_warped ("warped") and of global_motion ("global") for the most recent global_motion /
        global_motion_step / global_motion_batch call, from its resident flow and matrix: (batch, H, W, 3) u8 BGR each."""
        bad = set(images) - set(self.MOTION_IMAGES)
        if bad:
            raise ValueError(f"unknown image(s) {sorted(bad)}; choose from {self.MOTION_IMAGES}")
        out = {k: (np.empty((batch, self.H, self.W, 3), np.uint8) if k in images else None) for k in self.MOTION_IMAGES}
        check(self.lib.mav_last_global_motion_render(self.h, int(batch), _ptr(out["warped"]), _ptr(out["global"])))
        return {k: v for k, v in out.items() if v is not None}

    def colormap_jet(self, gray) -> np.ndarray:
        """cv2.applyColorMap(gray, COLORMAP_JET) of a u8 array of any shape -> shape + (3,) BGR."""
        g = np.ascontiguousarray(gray, np.uint8)
        out = np.empty(g.shape + (3,), np.uint8)
        check(self.lib.mav_colormap_jet(self.h, _ptr(g), g.size, _ptr(out)))
        return out

    # -- the processed.mp4 frame (processor.py:376-392) ------------------------------------------------------
    OVERLAY_RADIUS = 10                                 # what the reference's loop draws (draw_FoE's default)

    def _bgr_frames(self, frames) -> np.ndarray:
        a = np.asarray(frames)
        a = a[None] if a.ndim == 3 else a
        if a.ndim != 4 or a.shape[1:] != (self.H, self.W, 3) or a.dtype != np.uint8:
            raise ValueError(f"frames: expected (batch, {self.H}, {self.W}, 3) uint8, got {a.shape} {a.dtype}")
        return np.ascontiguousarray(a)

    @staticmethod
    def _foes(foe, B: int, name: str) -> np.ndarray:
        """(B, 2) float64 of FoE tuples as draw_FoE takes them: one (x, y) for a batch of one, or B of them.  A coordinate that IS the
        np.nan object draws nothing in the reference (-> inf: not drawn, as |v| > 1e9); any other NaN goes on to the library, which
        refuses it (ValueError, as int(nan) raises)."""
        rows = [foe] if np.ndim(foe) == 1 else list(foe)
        if len(rows) != B or any(len(r) != 2 for r in rows):
            raise ValueError(f"{name}: expected {B} (x, y) pairs")
        return np.array([[np.inf if v is np.nan else float(v) for v in r] for r in rows], np.float64).reshape(B, 2)

    def overlay(self, frames, masks, foe, foe_gt, radius: int = OVERLAY_RADIUS):
        """The frame the reference's loop writes to processed.mp4 (processor.py:376-392): FoE discs (foe green, foe_gt white over it)
        on the BGR frame, the fixed mask painted (150, 0, 150), blended 0.2 / 0.8 -> (overlay (B, H, W, 3) u8, written (B,) bool: the
        reference writes the frame, np.sum(result_img) > 0).  frames (B, H, W, 3) u8, masks (B, H, W), foe / foe_gt (x, y) per pair.
        The frames are not modified."""
        frames = self._bgr_frames(frames)
        B = frames.shape[0]
        masks = self._imgs(np.asarray(masks).astype(np.uint8), "masks")
        if masks.shape[0] != B:
            raise ValueError(f"masks: {masks.shape[0]} for {B} frames")
        fo, gt = self._foes(foe, B, "foe"), self._foes(foe_gt, B, "foe_gt")
        out = _pinned.empty(self, frames.shape, np.uint8)
        wr = np.empty(B, np.uint8)
        check(self.lib.mav_overlay(self.h, _ptr(frames), _ptr(masks), _ptr(fo), _ptr(gt), B, int(radius), _ptr(out), _ptr(wr)))
        return out, wr.view(np.bool_)

    def overlay_last(self, frames, foe_gt, radius: int = OVERLAY_RADIUS):
        """overlay() with the fixed masks and dense FoEs that the most recent detect / process_batch(_dev) / frame step left on the device:
        the frames go up, the overlays come back, the masks stay put."""
        frames = self._bgr_frames(frames)
        B = frames.shape[0]
        gt = self._foes(foe_gt, B, "foe_gt")
        out = _pinned.empty(self, frames.shape, np.uint8)
        wr = np.empty(B, np.uint8)
        check(self.lib.mav_last_overlay(self.h, _ptr(frames), _ptr(gt), B, int(radius), _ptr(out), _ptr(wr)))
        return out, wr.view(np.bool_)

    def overlay_dev(self, frames_ptr, mask_ptr, foe_ptr, foe_gt_ptr, batch: int, overlay_ptr, written_ptr, radius: int = OVERLAY_RADIUS):
        """mav_overlay_dev: enqueue only, device pointers."""
        check(self.lib.mav_overlay_dev(self.h, frames_ptr, mask_ptr, foe_ptr, foe_gt_ptr, int(batch), int(radius), overlay_ptr, written_ptr))

    # -- PNG files encoded on the device -----------------------------------------------------------------------
    def _png_out(self, count: int, channels: int):
        """(stream buffer of count x mav_png_bound bytes, index (count, 2) uint64).  The buffer is kept between calls (grow-only): it
        is virtual memory until written, and the pages the streams really take are then touched once."""
        need = self.lib.mav_png_bound(self.W, self.H, channels) * count
        buf = getattr(self, "_png_buf", None)
        if buf is None or buf.size < need:
            buf = self._png_buf = np.empty(need, np.uint8)
        return buf[:need], np.empty((count, 2), np.uint64)

    def _png_files(self, out, index, channels: int, wrap: bool = True):
        """the files of the streams in `out` -- or, wrap=False, (W, H, channels, stream bytes) tuples for frame_source.png_wrap, for a
        caller that adds the chunk framing (two CRC passes over the stream) somewhere else, e.g. on its writer threads"""
        from .frame_source import png_wrap
        streams = [out[int(o):int(o) + int(n)].tobytes() for o, n in index]
        return [png_wrap(self.W, self.H, channels, z) if wrap else (self.W, self.H, channels, z) for z in streams]

    def png_encode(self, imgs) -> list:
        """Complete PNG files (bytes) of 8-bit images, deflated on the device: (H, W) / (H, W, 1) gray, (H, W, 3) BGR, (H, W, 4) BGRA, or a
        batch of them with one more leading axis (a 3-d array whose last axis is 1, 3 or 4 long is ONE image).  Any PNG reader decodes
        them to exactly the pixels frame_source.encode_png's files hold; the bytes differ (Sub filter, run-length matches)."""
        a = np.asarray(imgs)
        if a.dtype != np.uint8:
            raise TypeError(f"png_encode() takes uint8 images, got {a.dtype}")
        if a.ndim == 2:
            a = a[None, :, :, None]
        elif a.ndim == 3:
            a = a[None] if a.shape == (self.H, self.W, a.shape[2]) and a.shape[2] in (1, 3, 4) else a[..., None]
        if a.ndim != 4 or a.shape[1:3] != (self.H, self.W) or a.shape[0] < 1:
            raise ValueError(f"png_encode(): expected (batch, {self.H}, {self.W}[, channels]) images, got {np.shape(imgs)}")
        count, ch = a.shape[0], a.shape[3]
        if ch not in (1, 3, 4):
            raise ValueError(f"png_encode(): channels must be 1, 3 or 4, got {ch}")
        a = np.ascontiguousarray(a)
        out, index = self._png_out(count, ch)
        check(self.lib.mav_png_encode(self.h, _ptr(a), count, ch, _ptr(out), out.size, _ptr(index)))
        return self._png_files(out, index, ch)

    def render_last_png(self, batch: int, images=IMAGES, wrap: bool = True) -> dict:
        """render_last() as PNG files: {name: [bytes per pair]}; rendered and deflated on the device, only the files' data comes back.
        wrap=False: png_wrap's argument tuples instead of files (see _png_files)."""
        bad = set(images) - set(self.IMAGES)
        if bad:
            raise ValueError(f"unknown image(s) {sorted(bad)}; choose from {self.IMAGES}")
        names = [k for k in self.IMAGES if k in images]
        out, index = self._png_out(max(1, len(names)) * int(batch), 3)
        check(self.lib.mav_last_render_png(self.h, int(batch), int("result" in names), int("flow" in names), int("phi" in names), _ptr(out),
                                           out.size, _ptr(index)))
        files = self._png_files(out, index, 3, wrap) if names else []
        return {k: files[j * batch:(j + 1) * batch] for j, k in enumerate(names)}

    def overlay_last_png(self, frames, foe_gt, radius: int = OVERLAY_RADIUS, wrap: bool = True):
        """overlay_last() as PNG files: ([bytes per pair], written (B,) bool).  wrap=False: as render_last_png."""
        frames = self._bgr_frames(frames)
        B = frames.shape[0]
        gt = self._foes(foe_gt, B, "foe_gt")
        out, index = self._png_out(B, 3)
        wr = np.empty(B, np.uint8)
        check(self.lib.mav_last_overlay_png(self.h, _ptr(frames), _ptr(gt), B, int(radius), _ptr(out), out.size, _ptr(index), _ptr(wr)))
        return self._png_files(out, index, 3, wrap), wr.view(np.bool_)

    # -- PNG decode on the device (include/mavflow_png_decode.h) --------------------------------------------------
    @staticmethod
    def _png_streams(files, verify_crc: bool = False):
        """(W, H, channels, streams u8, index (n, 2) u64) of PNG files that all hold device-eligible images of one size and colour
        type: the IDAT bodies of each file joined into its zlib stream, the streams packed back to back.  ValueError names the file."""
        from . import frame_source
        shape, parts, index, at = None, [], [], 0
        for k, data in enumerate(files):
            try:
                ihdr, _, _, spans = frame_source.png_chunks(data, "all" if verify_crc else "small")
            except (ValueError, struct.error) as e:
                raise ValueError(f"png_decode(): file {k}: {e}") from None
            if not frame_source.device_eligible(ihdr):
                raise ValueError(f"png_decode(): file {k} is not one the device decodes (depth {ihdr[2]}, colour type {ihdr[3]}, "
                                 f"interlace {ihdr[6]}): frame_source.decode_png reads it")
            this = (ihdr[0], ihdr[1], frame_source._CHANNELS[ihdr[3]])
            if shape is None:
                shape = this
            elif this != shape:
                raise ValueError(f"png_decode(): file {k} is {this[0]} x {this[1]} x {this[2]}, file 0 is {shape[0]} x {shape[1]} x {shape[2]}")
            n = sum(length for _, length in spans)
            parts += [data[o:o + length] for o, length in spans]
            index.append((at, n))
            at += n
        if shape is None:
            raise ValueError("png_decode(): no files")
        if len(index) > PNG_DECODE_MAX_COUNT:
            raise ValueError(f"png_decode(): {len(index)} files in one call, at most {PNG_DECODE_MAX_COUNT}")
        streams = np.frombuffer(b"".join(parts) + b"\0", np.uint8)
        return shape[0], shape[1], shape[2], streams, np.array(index, np.uint64).reshape(-1, 2)

    @staticmethod
    def _png_raise(status, what="png_decode()"):
        bad = np.flatnonzero(status["code"] != 0)
        if bad.size:
            k = int(bad[0])
            code = int(status["code"][k])
            name = PNG_ERRORS[code] if 0 <= code < len(PNG_ERRORS) else str(code)
            raise ValueError(f"{what}: file {k}: MAV_PNG_E_{name} ({code}) after {int(status['consumed'][k])} bytes of its stream"
                             + (f"; files {bad.tolist()} failed" if bad.size > 1 else ""))

    def png_decode(self, files, out: str = "bgr", verify_crc: bool = False, return_status: bool = False):
        """PNG files (bytes) of ONE size and colour type, 8-bit, not interlaced -> (n, H, W, 3) BGR as cv2.imread returns them
        (out="bgr"), (n, H, W) gray as cvtColor(BGR2GRAY) of that (out="gray"), or the files' own samples (n, H, W[, channels])
        (out="samples").  The compressed streams go up; inflate, Adler-32, un-filtering and conversion run on the device.  The size is
        the files' own, not the context's.  verify_crc: the IDAT CRC is checked on the host as well (the small chunks' always are).
        ValueError names the first file the decoder refused and its MAV_PNG_E_* code; return_status=True returns (array, statuses)
        instead and raises nothing for them (a refused image is all zero)."""
        if out not in PNG_OUT:
            raise ValueError(f"png_decode(): out must be one of {sorted(PNG_OUT)}, got {out!r}")
        W, H, ch, streams, index = self._png_streams(list(files), verify_crc)
        return self.png_decode_streams(streams, index, W, H, ch, out, return_status)

    def png_decode_streams(self, streams, index, W: int, H: int, channels: int, out: str = "samples", return_status: bool = False):
        """mav_png_decode on zlib streams: streams u8, index (n, 2) u64 of (offset, size) -> as png_decode."""
        streams = np.ascontiguousarray(streams, np.uint8)
        index = np.ascontiguousarray(index, np.uint64).reshape(-1, 2)
        n = index.shape[0]
        if n and int((index[:, 0] + index[:, 1]).max()) > streams.size:
            raise ValueError("png_decode_streams(): a stream ends past the buffer")
        if streams.size == 0:
            streams = np.zeros(1, np.uint8)
        oc = {"samples": int(channels), "bgr": 3, "gray": 1}[out]
        img = np.empty((n, int(H), int(W), oc), np.uint8)
        status = np.zeros(n, PNG_STATUS_DTYPE)
        check(self.lib.mav_png_decode(self.h, _ptr(streams), _ptr(index), n, int(W), int(H), int(channels), PNG_OUT[out], _ptr(img), _ptr(status)))
        if oc == 1:
            img = img[..., 0]
        if return_status:
            return img, status
        self._png_raise(status)
        return img

    def png_decode_dev(self, streams_ptr, index_ptr, count: int, W: int, H: int, channels: int, out: str, out_ptr, status_ptr, scratch_ptr) -> None:
        """mav_png_decode_dev: device pointers, enqueue only.  scratch: png_decode_scratch_bytes(W, H, channels, count) bytes."""
        check(self.lib.mav_png_decode_dev(self.h, _dev_ptr(streams_ptr), _dev_ptr(index_ptr), int(count), int(W), int(H), int(channels), PNG_OUT[out],
                                          _dev_ptr(out_ptr), _dev_ptr(status_ptr), _dev_ptr(scratch_ptr)))

    def png_decode_scratch_bytes(self, W: int, H: int, channels: int, count: int) -> int:
        return int(self.lib.mav_png_decode_scratch_bytes(int(W), int(H), int(channels), int(count)))

    def png_decode_to_device(self, files, out: str = "bgr", verify_crc: bool = False):
        """png_decode with the frames LEFT on the device: (DeviceBuffer of (n, H, W[, c]) u8, shape).  The statuses are checked (one
        synchronisation, 48 bytes per file come back); the caller frees the buffer."""
        W, H, ch, streams, index = self._png_streams(list(files), verify_crc)
        n = index.shape[0]
        oc = {"samples": ch, "bgr": 3, "gray": 1}[out]
        d_out = self.alloc(n * H * W * oc)
        bufs = []
        try:
            bufs = [self.alloc(streams.nbytes).upload(streams), self.alloc(index.nbytes).upload(index), self.alloc(n * PNG_STATUS_DTYPE.itemsize),
                    self.alloc(self.png_decode_scratch_bytes(W, H, ch, n))]
            self.png_decode_dev(bufs[0], bufs[1], n, W, H, ch, out, d_out, bufs[2], bufs[3])
            self._png_raise(bufs[2].download(PNG_STATUS_DTYPE, (n,)))      # (a stream-ordered copy and the call's one synchronisation)
        except Exception:
            self.sync()
            d_out.free()
            raise
        finally:
            self.sync()
            for b in bufs:
                b.free()
        return d_out, ((n, H, W) if oc == 1 else (n, H, W, oc))

    def farneback_png(self, files) -> np.ndarray:
        """Flow of every consecutive pair of n + 1 PNG files of the context's size -> (n, H, W, 2) float32, with no pixel crossing
        PCIe: the files are decoded to ONE gray block on the device and mav_farneback_dev reads frames 0 .. n - 1 as `prev` and
        1 .. n as `next` (the frame-sequence layout).  Byte for byte farneback(gray[:-1], gray[1:]) of the decoded frames."""
        files = list(files)
        n = len(files) - 1
        if n < 1:
            raise ValueError("farneback_png(): a sequence needs at least two files")
        if n > self.max_batch:
            raise ValueError(f"farneback_png(): {n} pairs on a context of max_batch {self.max_batch}")
        d_gray, shape = self.png_decode_to_device(files, "gray")
        d_flow = None
        try:
            if shape[1:] != (self.H, self.W):
                raise ValueError(f"farneback_png(): the files are {shape[2]} x {shape[1]}, the context is {self.W} x {self.H}")
            d_flow = self.alloc(n * self.H * self.W * 8)
            check(self.lib.mav_farneback_dev(self.h, d_gray.ptr, d_gray.ptr + self.W * self.H, n, d_flow.ptr))
            return d_flow.download(np.float32, (n, self.H, self.W, 2))
        finally:
            self.sync()
            d_gray.free()
            if d_flow is not None:
                d_flow.free()

    # -- JPEG decode on the device (include/mavflow_jpeg.h) --------------------------------------------------------
    @staticmethod
    def _jpeg_pack(files):
        """(W, H, components, files u8, index (n, 2) u64, infos (n,) JPEG_INFO_DTYPE) of baseline JPEG files of one size and component
        count, packed back to back as they are.  ValueError names the file and carries the parser's reason."""
        shape, index, infos, at = None, [], [], 0
        for k, data in enumerate(files):
            info, why = jpeg_info(data)
            if info is None:
                raise ValueError(f"jpeg_decode(): file {k}: {why}")
            this = (int(info["W"][0]), int(info["H"][0]), int(info["components"][0]))
            if shape is None:
                shape = this
            elif this != shape:
                raise ValueError(f"jpeg_decode(): file {k} is {this[0]} x {this[1]} x {this[2]}, file 0 is {shape[0]} x {shape[1]} x {shape[2]}")
            infos.append(info)
            index.append((at, len(data)))
            at += len(data)
        if shape is None:
            raise ValueError("jpeg_decode(): no files")
        if len(index) > JPEG_MAX_COUNT:
            raise ValueError(f"jpeg_decode(): {len(index)} files in one call, at most {JPEG_MAX_COUNT}")
        packed = np.frombuffer(b"".join(bytes(f) for f in files) + b"\0", np.uint8)
        return shape[0], shape[1], shape[2], packed, np.array(index, np.uint64).reshape(-1, 2), np.concatenate(infos)

    @staticmethod
    def _jpeg_raise(status, what="jpeg_decode()"):
        bad = np.flatnonzero(status["code"] != 0)
        if bad.size:
            k = int(bad[0])
            code = int(status["code"][k])
            name = JPEG_ERRORS[code] if 0 <= code < len(JPEG_ERRORS) else str(code)
            raise ValueError(f"{what}: file {k}: MAV_JPEG_E_{name} ({code}) after {int(status['consumed'][k])} bytes of its entropy segment"
                             + (f"; files {bad.tolist()} failed" if bad.size > 1 else ""))

    def jpeg_decode(self, files, out: str = "bgr", return_status: bool = False):
        """Baseline JPEG files (bytes) of ONE size and component count -> (n, H, W, 3) BGR as cv2.imread returns them (out="bgr"),
        (n, H, W) gray as cvtColor(BGR2GRAY) of that (out="gray"; not IMREAD_GRAYSCALE), or the upsampled Y, Cb, Cr (n, H, W[, 3])
        (out="samples").  The files go up as they are; restart-marker search, Huffman decoding, IDCT, upsampling and conversion run on
        the device.  The size is the files' own, not the context's.  ValueError names the first file the parser or the decoder
        refused; return_status=True returns (array, statuses) instead and raises nothing for the decoder's verdicts (a refused image
        is all zero)."""
        if out not in JPEG_OUT:
            raise ValueError(f"jpeg_decode(): out must be one of {sorted(JPEG_OUT)}, got {out!r}")
        W, H, comps, packed, index, infos = self._jpeg_pack(list(files))
        return self.jpeg_decode_packed(packed, index, infos, W, H, out, return_status)

    def jpeg_decode_packed(self, packed, index, infos, W: int, H: int, out: str = "bgr", return_status: bool = False):
        """mav_jpeg_decode on files packed in one array: packed u8, index (n, 2) u64 of (offset, size), infos (n,) JPEG_INFO_DTYPE."""
        packed = np.ascontiguousarray(packed, np.uint8)
        index = np.ascontiguousarray(index, np.uint64).reshape(-1, 2)
        infos = np.ascontiguousarray(infos, JPEG_INFO_DTYPE).reshape(-1)
        n = index.shape[0]
        if n != infos.shape[0] or n < 1:
            raise ValueError(f"jpeg_decode_packed(): {n} index rows, {infos.shape[0]} infos")
        if int((index[:, 0] + index[:, 1]).max()) > packed.size:
            raise ValueError("jpeg_decode_packed(): a file ends past the buffer")
        comps = 3 if int(infos["components"][0]) == 3 else 1
        oc = {"samples": comps, "bgr": 3, "gray": 1}[out]
        img = np.empty((n, int(H), int(W), oc), np.uint8)
        status = np.zeros(n, JPEG_STATUS_DTYPE)
        check(self.lib.mav_jpeg_decode(self.h, _ptr(packed), _ptr(index), _ptr(infos), n, int(W), int(H), JPEG_OUT[out], _ptr(img), _ptr(status)))
        if oc == 1:
            img = img[..., 0]
        if return_status:
            return img, status
        self._jpeg_raise(status)
        return img

    def jpeg_decode_dev(self, files_ptr, index_ptr, info_ptr, count: int, W: int, H: int, out: str, out_ptr, status_ptr, scratch_ptr) -> None:
        """mav_jpeg_decode_dev: device pointers, enqueue only.  scratch: jpeg_decode_scratch_bytes(W, H, components, count) bytes."""
        check(self.lib.mav_jpeg_decode_dev(self.h, _dev_ptr(files_ptr), _dev_ptr(index_ptr), _dev_ptr(info_ptr), int(count), int(W), int(H),
                                           JPEG_OUT[out], _dev_ptr(out_ptr), _dev_ptr(status_ptr), _dev_ptr(scratch_ptr)))

    def jpeg_decode_scratch_bytes(self, W: int, H: int, components: int, count: int) -> int:
        return int(self.lib.mav_jpeg_decode_scratch_bytes(int(W), int(H), int(components), int(count)))

    def jpeg_decode_to_device(self, files, out: str = "bgr", return_status: bool = False):
        """jpeg_decode with the frames LEFT on the device: (DeviceBuffer of (n, H, W[, c]) u8, shape[, statuses]).  The statuses are
        checked (one synchronisation, 40 bytes per file come back) unless they are returned; the caller frees the buffer."""
        W, H, comps, packed, index, infos = self._jpeg_pack(list(files))
        n = index.shape[0]
        oc = {"samples": comps, "bgr": 3, "gray": 1}[out]
        d_out = self.alloc(n * H * W * oc)
        bufs = []
        try:
            bufs = [self.alloc(packed.nbytes).upload(packed), self.alloc(index.nbytes).upload(index), self.alloc(infos.nbytes).upload(infos),
                    self.alloc(n * JPEG_STATUS_DTYPE.itemsize), self.alloc(self.jpeg_decode_scratch_bytes(W, H, comps, n))]
            self.jpeg_decode_dev(bufs[0], bufs[1], bufs[2], n, W, H, out, d_out, bufs[3], bufs[4])
            status = bufs[3].download(JPEG_STATUS_DTYPE, (n,))         # (a stream-ordered copy and the call's one synchronisation)
            if not return_status:
                self._jpeg_raise(status)
        except Exception:
            self.sync()
            d_out.free()
            raise
        finally:
            self.sync()
            for b in bufs:
                b.free()
        shape = (n, H, W) if oc == 1 else (n, H, W, oc)
        return (d_out, shape, status) if return_status else (d_out, shape)

    def farneback_jpeg(self, files) -> np.ndarray:
        """farneback_png for JPEG files: the flow of every consecutive pair of n + 1 baseline JPEG files of the context's size ->
        (n, H, W, 2) float32.  The files are decoded to ONE gray block on the device, where mav_farneback_dev reads frames 0 .. n - 1
        as `prev` and 1 .. n as `next`.  Byte for byte farneback(gray[:-1], gray[1:]) of the decoded frames."""
        files = list(files)
        n = len(files) - 1
        if n < 1:
            raise ValueError("farneback_jpeg(): a sequence needs at least two files")
        if n > self.max_batch:
            raise ValueError(f"farneback_jpeg(): {n} pairs on a context of max_batch {self.max_batch}")
        d_gray, shape = self.jpeg_decode_to_device(files, "gray")
        d_flow = None
        try:
            if shape[1:] != (self.H, self.W):
                raise ValueError(f"farneback_jpeg(): the files are {shape[2]} x {shape[1]}, the context is {self.W} x {self.H}")
            d_flow = self.alloc(n * self.H * self.W * 8)
            check(self.lib.mav_farneback_dev(self.h, d_gray.ptr, d_gray.ptr + self.W * self.H, n, d_flow.ptr))
            return d_flow.download(np.float32, (n, self.H, self.W, 2))
        finally:
            self.sync()
            d_gray.free()
            if d_flow is not None:
                d_flow.free()

    # -- device-pointer path (bench, multi-GPU) --------------------------------------------------------------
    def process_batch_dev(self, prev_ptr, next_ptr, samples_ptr, batch, results_ptr, flow_ptr=None, omega_ptr=None,
                          dt_ptr=None, sky_ptr=None, phi_ptr=None, mf_ptr=None, md_ptr=None, foe_params=None,
                          thr_params=None, frame0_ptr=None):
        fp = foe_params or foe_defaults()
        tp = thr_params or thr_defaults()
        check(self.lib.mav_process_batch_dev(self.h, prev_ptr, next_ptr, samples_ptr, omega_ptr, dt_ptr, frame0_ptr, sky_ptr, batch,
                                             C.byref(fp), C.byref(tp), flow_ptr, phi_ptr, mf_ptr, md_ptr, results_ptr))

    def last_flow(self, pair: int) -> np.ndarray:
        """Flow field (H, W, 2) float32 of pair `pair` of the most recent process_batch_dev / farneback_dev call, downloaded
        from wherever that call wrote it (the caller's buffer or the context's workspace)."""
        p = self.lib.mav_last_flow_dev(self.h)
        if not p:
            raise ValueError("no flow has been computed on this context yet")
        if not 0 <= pair < self.max_batch:
            raise ValueError(f"pair {pair} outside [0, {self.max_batch})")
        out = np.empty((self.H, self.W, 2), np.float32)
        check(self.lib.mav_memcpy_d2h(self.h, _ptr(out), p + pair * out.nbytes, out.nbytes))
        return out

    def farneback_dev(self, prev_ptr, next_ptr, batch, flow_ptr, flow_init_ptr=None, depth=None):
        """Enqueue only.  flow_init_ptr: None = zero start (mav_farneback_dev); a device pointer (it may equal flow_ptr) = the pairs'
        initial flow (mav_farneback_init_dev).  depth: the frames' dtype (uint8 / uint16 / float32) or a MAV_DEPTH_* code; None =
        uint8.  Any depth but uint8 goes through mav_farneback_ex_dev."""
        if depth is not None:
            d = depth if isinstance(depth, int) and not isinstance(depth, bool) else _depth_of(depth)
            if d != DEPTH_8U:
                check(self.lib.mav_farneback_ex_dev(self.h, prev_ptr, next_ptr, d, batch, flow_init_ptr, flow_ptr))
                return
        if flow_init_ptr is None:
            check(self.lib.mav_farneback_dev(self.h, prev_ptr, next_ptr, batch, flow_ptr))
        else:
            check(self.lib.mav_farneback_init_dev(self.h, prev_ptr, next_ptr, batch, flow_init_ptr, flow_ptr))

    # -- multi-GPU record exchange (RCCL through the library, on the context's stream) ------------------------
    def comm_unique_id(self) -> np.ndarray:
        """A fresh ncclUniqueId (128 bytes, uint8) -- rank 0 creates it, every rank passes the same bytes to comm_init."""
        uid = np.zeros(128, np.uint8)
        check(self.lib.mav_comm_unique_id(_ptr(uid)))
        return uid

    def comm_init(self, uid, rank: int, nranks: int):
        uid = np.ascontiguousarray(np.asarray(uid, np.uint8).reshape(128))
        comm = C.c_void_p()
        check(self.lib.mav_comm_init(self.h, _ptr(uid), int(rank), int(nranks), C.byref(comm)))
        return comm

    def allgather(self, comm, local_ptr, bytes_per_rank: int, all_ptr):
        """ncclAllGather of bytes_per_rank bytes from every rank, enqueued on the context's stream (no host sync)."""
        check(self.lib.mav_allgather_results(self.h, comm, local_ptr, int(bytes_per_rank), all_ptr))

    def comm_count(self, comm) -> int:
        n = C.c_int()
        check(self.lib.mav_comm_count(comm, C.byref(n)))
        return n.value

    def comm_destroy(self, comm):
        check(self.lib.mav_comm_destroy(comm))

    def timer_start(self):
        check(self.lib.mav_timer_start(self.h))

    def timer_stop(self) -> float:
        ms = C.c_float()
        check(self.lib.mav_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def profile_enable(self, on=True):
        check(self.lib.mav_profile_enable(self.h, int(on)))

    def profile_get(self) -> dict:
        n = C.c_int(32)
        names = (C.c_char_p * 32)()
        ms = (C.c_double * 32)()
        cnt = (C.c_long * 32)()
        check(self.lib.mav_profile_get(self.h, C.byref(n), names, ms, cnt))
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n.value)}

    def profile_intervals(self):
        """(class index, stream, t0 ms, t1 ms) arrays of every profiled launch / run since profile_enable; class names in
        profile_get()'s order."""
        n = C.c_int(0)
        check(self.lib.mav_profile_intervals(self.h, C.byref(n), None, None, None, None))
        k, st = np.empty(n.value, np.int32), np.empty(n.value, np.int32)
        t0, t1 = np.empty(n.value, np.float32), np.empty(n.value, np.float32)
        check(self.lib.mav_profile_intervals(self.h, C.byref(n), _ptr(k), _ptr(st), _ptr(t0), _ptr(t1)))
        return k[:n.value], st[:n.value], t0[:n.value], t1[:n.value]

    def profile_busy(self, *names: str) -> float:
        """ms during which at least one launch of the named kernel classes was running (union of the launches' intervals)."""
        out = C.c_double()
        check(self.lib.mav_profile_busy(self.h, ",".join(names).encode(), C.byref(out)))
        return out.value

    # -- sparse optical flow ---------------------------------------------------------------------------------
    def _gray1(self, a, name):
        return None if a is None else _arr(np.asarray(a), np.uint8, (self.H, self.W), name)

    def _mask1(self, mask):
        """cv2's mask: an (H, W) uint8 array (non-zero = the pixel takes part) or None; ValueError for any other shape or dtype."""
        if mask is None:
            return None
        mask = np.asarray(mask)
        if mask.dtype != np.uint8 or mask.shape != (self.H, self.W):
            raise ValueError(f"mask: expected a uint8 array of shape {(self.H, self.W)}, got {mask.dtype} {mask.shape}")
        return np.ascontiguousarray(mask)

    def good_features(self, gray, mask=None, useHarrisDetector=False, k=0.04, **params) -> np.ndarray:
        """cv2.goodFeaturesToTrack(gray, mask=mask, useHarrisDetector=..., k=..., **params) on one (H, W) uint8 frame -> (n, 2) float32
        corners (x, y), strongest first.  gray None: the context's resident frame (the `nxt` of the last lk_track, or the last frame
        given here).  useHarrisDetector: the Harris response with `k` as the score (mav_good_features_score)."""
        p = gftt_defaults(**params)
        gray, mask = self._gray1(gray, "gray"), self._mask1(mask)
        out = np.empty((max(int(p.max_corners), 1), 2), np.float32)
        n = C.c_int()
        if useHarrisDetector:
            sc = corner_score(True, k)
            check(self.lib.mav_good_features_score(self.h, _ptr(gray), _ptr(mask), C.byref(p), C.byref(sc), _ptr(out), C.byref(n)))
        elif mask is None:
            check(self.lib.mav_good_features(self.h, _ptr(gray), C.byref(p), _ptr(out), C.byref(n)))
        else:
            check(self.lib.mav_good_features_ex(self.h, _ptr(gray), _ptr(mask), C.byref(p), _ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def good_features_enqueue(self, gray_ptr, corners_ptr, count_ptr, mask_ptr=None, useHarrisDetector=False, k=0.04, **params):
        """mav_good_features_ex_dev: device pointers in and out, enqueue only.  gray_ptr None: the resident frame.  corners_ptr:
        max_corners x 2 float32, count_ptr: one int32 (the corner count, or -(candidates) when they overflow the buffer).
        useHarrisDetector: mav_good_features_score_dev with the Harris response and `k`."""
        p = gftt_defaults(**params)
        if useHarrisDetector:
            sc = corner_score(True, k)
            check(self.lib.mav_good_features_score_dev(self.h, gray_ptr, mask_ptr, C.byref(p), C.byref(sc), corners_ptr, count_ptr))
        else:
            check(self.lib.mav_good_features_ex_dev(self.h, gray_ptr, mask_ptr, C.byref(p), corners_ptr, count_ptr))

    def lk_track_enqueue(self, prev_ptr, next_ptr, pts_ptr, n_max: int, n_ptr, next_pts_ptr, status_ptr, **params):
        """mav_lk_track_ex_dev: mav_lk_track_dev for up to n_max points whose count is the int32 at the device pointer n_ptr."""
        check(self.lib.mav_lk_track_ex_dev(self.h, prev_ptr, next_ptr, pts_ptr, int(n_max), n_ptr, C.byref(lk_defaults(**params)), next_pts_ptr,
                                           status_ptr))

    def gftt_last_pick(self):
        """(chunks, rounds) of the most recent corner pick on the device."""
        st = np.zeros(2, np.uint32)
        check(self.lib.mav_gftt_last_pick(self.h, _ptr(st)))
        return int(st[0]), int(st[1])

    def stage_corner_pick(self, keys, **params) -> np.ndarray:
        """The device sort and pick on host candidate keys (value bits << 32 | linear index, uint64, any order) -> (n, 2) float32."""
        p = gftt_defaults(**params)
        keys = _arr(np.asarray(keys, np.uint64).reshape(-1), np.uint64)
        out = np.empty((max(int(p.max_corners), 1), 2), np.float32)
        n = C.c_int()
        check(self.lib.mav_stage_corner_pick(self.h, _ptr(keys) if len(keys) else None, len(keys), C.byref(p), _ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def lk_track(self, prev, nxt, pts, **params):
        """cv2.calcOpticalFlowPyrLK(prev, nxt, pts, None, **params) -> (next_pts (n, 2) float32, status (n,) uint8).  prev None: the
        resident frame.  `nxt` becomes the resident frame."""
        p = lk_defaults(**params)
        prev, nxt = self._gray1(prev, "prev"), self._gray1(nxt, "nxt")
        pts = _arr(np.asarray(pts, np.float32).reshape(-1, 2), np.float32)
        n = pts.shape[0]
        out, status = np.empty((n, 2), np.float32), np.empty(n, np.uint8)
        check(self.lib.mav_lk_track(self.h, _ptr(prev), _ptr(nxt), _ptr(pts) if n else None, n, C.byref(p), _ptr(out) if n else None,
                                    _ptr(status) if n else None))
        return out, status

    def lk_track_err(self, prev, nxt, pts, next_pts=None, flags=0, **params):
        """cv2.calcOpticalFlowPyrLK(prev, nxt, pts, next_pts, flags=flags, **params) as cv2's Python call runs it, err always computed
        -> (next_pts (n, 2) float32, status (n,) uint8, err (n,) float32).  flags: 0 or an OR of OPTFLOW_USE_INITIAL_FLOW (the
        starting positions are `next_pts`, which is not written) and OPTFLOW_LK_GET_MIN_EIGENVALS (err is level 0's minimum
        eigenvalue).  With err comes cv2's final bounds test: a point whose last position leaves the bounds ends with status 0, where
        lk_track keeps it at 1.  prev None: the resident frame; `nxt` becomes the resident frame."""
        p = lk_defaults(**params)
        prev, nxt = self._gray1(prev, "prev"), self._gray1(nxt, "nxt")
        pts = _arr(np.asarray(pts, np.float32).reshape(-1, 2), np.float32)
        n = pts.shape[0]
        out = np.empty((n, 2), np.float32)
        if int(flags) & OPTFLOW_USE_INITIAL_FLOW:
            if next_pts is None:
                raise ValueError("lk_track_err: OPTFLOW_USE_INITIAL_FLOW needs the starting positions in next_pts")
            out[:] = _arr(np.asarray(next_pts, np.float32).reshape(-1, 2), np.float32, (n, 2), "next_pts")
        status, err = np.empty(n, np.uint8), np.empty(n, np.float32)
        check(self.lib.mav_lk_track_err(self.h, _ptr(prev), _ptr(nxt), _ptr(pts) if n else None, n, C.byref(p), int(flags),
                                        _ptr(out) if n else None, _ptr(status) if n else None, _ptr(err) if n else None))
        return out, status, err

    def lk_track_err_enqueue(self, prev_ptr, next_ptr, pts_ptr, n_max: int, n_ptr, next_pts_ptr, status_ptr, err_ptr, flags=0, **params):
        """mav_lk_track_err_dev: device pointers, enqueue only.  n_ptr: the int32 point count on the device, or None (n_max points
        run).  next_pts_ptr is read first under OPTFLOW_USE_INITIAL_FLOW and may equal pts_ptr; err_ptr may be None."""
        check(self.lib.mav_lk_track_err_dev(self.h, prev_ptr, next_ptr, pts_ptr, int(n_max), n_ptr, C.byref(lk_defaults(**params)), int(flags),
                                            next_pts_ptr, status_ptr, err_ptr))

    def lk_track_dev(self, prev_ptr, next_ptr, pts_ptr, n: int, next_pts_ptr, status_ptr, **params):
        """mav_lk_track_dev: device pointers, enqueue only."""
        check(self.lib.mav_lk_track_dev(self.h, prev_ptr, next_ptr, pts_ptr, int(n), C.byref(lk_defaults(**params)), next_pts_ptr, status_ptr))

    def good_features_dev(self, gray_ptr, **params) -> np.ndarray:
        """mav_good_features_dev: a device frame (None: the resident one) -> host corners; synchronises once, to bring them back."""
        p = gftt_defaults(**params)
        out = np.empty((max(int(p.max_corners), 1), 2), np.float32)
        n = C.c_int()
        check(self.lib.mav_good_features_dev(self.h, gray_ptr, C.byref(p), _ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def lk_last_iterations(self) -> np.ndarray:
        """Iterations per (point, level) of the latest track call as a histogram (LK_HIST_BINS bins, the last = more)."""
        h = np.empty(LK_HIST_BINS, np.uint32)
        check(self.lib.mav_lk_last_iterations(self.h, _ptr(h)))
        return h

    def lk_level_dims(self, level: int):
        w, h = C.c_int(), C.c_int()
        check(self.lib.mav_lk_level_dims(self.h, int(level), C.byref(w), C.byref(h)))
        return w.value, h.value

    def stage_lk_pyramid(self, img, level: int) -> np.ndarray:
        w, h = self.lk_level_dims(level)
        out = np.empty((h, w), np.uint8)
        check(self.lib.mav_stage_lk_pyramid(self.h, _ptr(self._gray1(img, "img")), int(level), _ptr(out)))
        return out

    def stage_lk_scharr(self, img, level: int) -> np.ndarray:
        w, h = self.lk_level_dims(level)
        out = np.empty((h, w, 2), np.int16)
        check(self.lib.mav_stage_lk_scharr(self.h, _ptr(self._gray1(img, "img")), int(level), _ptr(out)))
        return out

    def stage_min_eigen(self, img, block_size: int = 7) -> np.ndarray:
        out = np.empty((self.H, self.W), np.float32)
        check(self.lib.mav_stage_min_eigen(self.h, _ptr(self._gray1(img, "img")), int(block_size), _ptr(out)))
        return out

    def stage_corner_response(self, img, block_size: int = 7, useHarrisDetector=False, k=0.04) -> np.ndarray:
        """The corner score map (H, W) float32: the Harris response, or stage_min_eigen's bytes without useHarrisDetector."""
        out = np.empty((self.H, self.W), np.float32)
        sc = corner_score(useHarrisDetector, k)
        check(self.lib.mav_stage_corner_response(self.h, _ptr(self._gray1(img, "img")), int(block_size), C.byref(sc), _ptr(out)))
        return out

    # -- stage hooks (parity tests) --------------------------------------------------------------------------
    def stage_phi_mask(self, flow32, foe, omega=None, dt=None, sky=None, params: ThrParams | None = None, want_phi=False):
        """The phi / mask / box stage of the fused path (float32 flow, double arithmetic, screen on unless phi is wanted)
        with a caller-supplied FoE."""
        flow = np.asarray(flow32, np.float32)
        flow = flow[None] if flow.ndim == 3 else flow
        B = flow.shape[0]
        flow = _arr(flow, np.float32, (B, self.H, self.W, 2), "flow")
        foe = _arr(np.asarray(foe, np.float64).reshape(B, 2), np.float64)
        omega = None if omega is None else _arr(np.asarray(omega, np.float64).reshape(B, 3), np.float64)
        dt = None if dt is None else _arr(np.asarray(dt, np.float64).reshape(B), np.float64)
        sky = None if sky is None else _arr(np.asarray(sky).reshape(B, self.H, self.W).astype(np.uint8), np.uint8)
        p = params or thr_defaults()
        phi = np.empty((B, self.H, self.W), np.float64) if want_phi else None
        mf = np.empty((B, self.H, self.W), np.uint8)
        md = np.empty((B, self.H, self.W), np.uint8)
        box = np.empty((B, 4), np.int32)
        check(self.lib.mav_stage_phi_mask(self.h, _ptr(flow), _ptr(foe), _ptr(omega), _ptr(dt), _ptr(sky), B, C.byref(p), _ptr(phi),
                                          _ptr(mf), _ptr(md), _ptr(box)))
        return phi, mf.view(np.bool_), md.view(np.bool_), box

    def stage_coefficients(self, k: int = -1):
        """The constants the flow kernels use: dict(g, xg, xxg (poly_n + 1 each, centre first), ig = [ig11, ig03, ig33, ig55],
        blur = layer k's Gaussian taps when k >= 0)."""
        n = self.fb.poly_n
        g, xg, xxg = (np.empty(n + 1, np.float32) for _ in range(3))
        ig = np.empty(4, np.float32)
        blur = np.empty(self.layer_dims(k)[3], np.float32) if k >= 0 else None
        check(self.lib.mav_stage_coefficients(self.h, k, _ptr(g), _ptr(xg), _ptr(xxg), _ptr(ig), _ptr(blur)))
        return dict(g=g, xg=xg, xxg=xxg, ig=ig, blur=blur)

    def stage_blur_resize(self, img, k, two_pass=False):
        """Layer image k of one frame (uint8, uint16 or float32; float64 is narrowed on the host)."""
        img = np.asarray(img)
        if img.dtype == np.float64:
            img = img.astype(np.float32)
        depth = _depth_of(img.dtype, "img")
        img = _arr(img, img.dtype, (self.H, self.W), "img")
        w, h, _, _ = self.layer_dims(k)
        out = np.empty((h, w), np.float32)
        if depth != DEPTH_8U:
            check(self.lib.mav_stage_blur_resize_ex(self.h, _ptr(img), depth, k, int(bool(two_pass)), _ptr(out)))
            return out
        fn = self.lib.mav_stage_blur_resize_two_pass if two_pass else self.lib.mav_stage_blur_resize
        check(fn(self.h, _ptr(img), k, _ptr(out)))
        return out

    def stage_polyexp(self, I, k):
        w, h, _, _ = self.layer_dims(k)
        I = _arr(I, np.float32, (h, w), "I")
        R = np.empty((5, h, w), np.float32)
        check(self.lib.mav_stage_polyexp(self.h, _ptr(I), k, _ptr(R)))
        return R

    def stage_update_matrices(self, R0, R1, flow, k):
        w, h, _, _ = self.layer_dims(k)
        R0 = _arr(R0, np.float32, (5, h, w), "R0"); R1 = _arr(R1, np.float32, (5, h, w), "R1")
        flow = _arr(flow, np.float32, (h, w, 2), "flow")
        M = np.empty((5, h, w), np.float32)
        check(self.lib.mav_stage_update_matrices(self.h, _ptr(R0), _ptr(R1), _ptr(flow), k, _ptr(M)))
        return M

    def stage_update_matrices_from(self, R0, R1, flow_coarse, k):
        """The initial M of layer k from the coarser layer's flow (upsampled inside the kernel), or from zero when flow_coarse is None."""
        w, h, _, _ = self.layer_dims(k)
        R0 = _arr(R0, np.float32, (5, h, w), "R0"); R1 = _arr(R1, np.float32, (5, h, w), "R1")
        if flow_coarse is not None:
            pw, ph = (self.layer_dims(k + 1)[:2] if k + 1 < self.num_layers() else np.shape(flow_coarse)[1::-1])
            flow_coarse = _arr(flow_coarse, np.float32, (ph, pw, 2), "flow_coarse")
        M = np.empty((5, h, w), np.float32)
        check(self.lib.mav_stage_update_matrices_from(self.h, _ptr(R0), _ptr(R1), _ptr(flow_coarse), k, _ptr(M)))
        return M

    def stage_initial_flow(self, flow0, k):
        """Layer k's initial flow from a frame-size field: resize(INTER_AREA), times pyr_scale^k."""
        flow0 = _arr(flow0, np.float32, (self.H, self.W, 2), "flow0")
        w, h, _, _ = self.layer_dims(k)
        out = np.empty((h, w, 2), np.float32)
        check(self.lib.mav_stage_initial_flow(self.h, _ptr(flow0), k, _ptr(out)))
        return out

    def stage_blur_iter(self, R0, R1, M, k, update=True):
        w, h, _, _ = self.layer_dims(k)
        R0 = _arr(R0, np.float32, (5, h, w), "R0"); R1 = _arr(R1, np.float32, (5, h, w), "R1")
        M = _arr(M, np.float32, (5, h, w), "M")
        flow = np.empty((h, w, 2), np.float32)
        Mo = np.empty((5, h, w), np.float32)
        check(self.lib.mav_stage_blur_iter(self.h, _ptr(R0), _ptr(R1), _ptr(M), k, int(bool(update)), _ptr(flow), _ptr(Mo)))
        return flow, (Mo if update else None)


def runtime_info() -> dict:
    """HIP version of the build, HIP runtime / driver versions of this process, RCCL version once loaded (mav_runtime_info)."""
    import json
    buf = C.create_string_buffer(512)
    check(load().mav_runtime_info(buf, len(buf)))
    return json.loads(buf.value.decode())


def device_count() -> int:
    return load().mav_device_count()


# include/mavflow_truth.h (Context.gt_flow, .radial_error_hist, .radial_error_accumulator): a binding module of its own, attached here so
# that every Context has the methods
from . import _truth  # noqa: E402,F401


# include/mavflow_validation.h (Context.gt_stats, .gt_stats_enqueue): likewise
from . import _validation  # noqa: E402,F401


# include/mavflow_cluster.h (Context.kmeans, .kmeans_enqueue, .kmeans_workspace_bytes, .kmeans_paint): likewise
from . import clustering  # noqa: E402,F401


# include/mavflow_warp.h (Context.remap, .warp_flow, .warp_affine, .warp_perspective, .warp_method and their *_enqueue twins): likewise
from . import warp  # noqa: E402,F401


# include/mavflow_affine.h (Context.estimate_affine, .flow_affine, their *_enqueue twins and .estimate_affine_workspace_bytes): likewise
from . import affine  # noqa: E402,F401

# include/mavflow_fundamental.h (Context.find_fundamental, .flow_fundamental, .epipolar_residual, their *_enqueue twins and
# .find_fundamental_workspace_bytes): likewise
from . import fundamental  # noqa: E402,F401

# include/mavflow_essential.h (Context.find_essential, .flow_essential, their *_enqueue twins and .find_essential_workspace_bytes):
# likewise
from . import essential  # noqa: E402,F401
