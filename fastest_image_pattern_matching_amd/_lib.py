"""ctypes binding of libfpm_hip.so (include/fpm.h).

The shared library is built in-tree by ``csrc/Makefile`` (``__graft_entry__.build()`` or ``make -C
fastest_image_pattern_matching_amd/csrc``).  There is no CPU fallback: if the library is missing or no gfx950
device is present, loading / context creation raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfpm_hip.so")
CSRC = os.path.join(_HERE, "csrc")

FPM_OK = 0
FPM_E_INVALID_ARG = -1
FPM_E_NOT_LEARNED = -2
FPM_E_SIZE = -3
FPM_E_DEVICE = -4
FPM_E_CAPACITY = -5
FPM_E_INTERNAL = -6

# pixel formats of the device-memory entries (include/fpm.h FPM_FMT_*)
(FMT_GRAY8, FMT_BGR8, FMT_RGB8, FMT_BGRA8, FMT_RGBA8, FMT_BGR8_PLANAR, FMT_RGB8_PLANAR) = range(7)
FMT_COUNT = 7

(K_PYR, K_TOP_WARP, K_TOP_NCC, K_TOP_NMS, K_CAND_INIT, K_ROI_TABLES, K_ROI_WARP, K_ROI_CORR, K_ROI_EVAL, K_ROI_SMALL,
 K_CAND_STEP, K_TOP_MAP, K_NOT, K_PATCH, K_COMPARE, K_LEARN) = range(16)
# profiling index -> kernel (include/fpm.h FPM_K_*); top_ncc is k_top_mma (matrix-core top layer) where it applies, else
# k_ncc_tile for templates up to 128 x 64; top_map = k_top_map, the matrix-core form's fallback (full maps for the jobs
# its lists left); bitwise_not = k_bitwise_not, 255 - source over the staged level 0 (Params.bitwise_not); patch_warp =
# the match patches' launch (k_patch_warp, or k_warp under FPM_PATCH_FORM_WARP), never part of a search; patch_compare =
# k_patch_compare, the launches of last_compare / compare_at (one, two when normalising), never part of a search either
KERNEL_NAMES = ["pyr_down", "top_warp", "top_ncc", "top_nms", "cand_init", "roi_tables", "roi_warp", "roi_corr",
                "roi_eval", "roi_small", "cand_step", "top_map", "bitwise_not", "patch_warp", "patch_compare"]
# KERNEL_NAMES holds the kernels of searches, patches and comparisons, and keeps its 15 entries (tests/test_gpu_compare.py
# pins the count).  The learn entries' kernel has its profiling index past them: tmpl_prep = k_tmpl_prep, the one launch of
# learn_device / learn_at / learn_hit over all template levels, never part of a search.  PROFILE_NAMES names every
# FPM_K_* index.
LEARN_KERNEL_NAME = "tmpl_prep"
PROFILE_NAMES = KERNEL_NAMES + [LEARN_KERNEL_NAME]
# fpm_set_patch_form
PATCH_FORM_TILED, PATCH_FORM_WARP = 0, 1
# fpm_last_compare / fpm_compare_at flags
COMPARE_NORMALIZE = 1
KERNEL_SYMBOLS = {"pyr_down": ["k_pyr_down_s", "k_pyr_down"], "top_warp": ["k_warp"],
                  "top_ncc": ["k_top_mma", "k_ncc_tile", "k_ncc_map"],
                  "top_nms": ["k_nms_greedy", "k_nms"], "cand_init": ["k_cand_init"], "roi_tables": ["k_roi_tables"],
                  "roi_warp": ["k_roi_warp3", "k_roi_warp"], "roi_corr": ["k_roi_corr"], "roi_eval": ["k_roi_eval"],
                  "roi_small": ["k_roi_small"], "cand_step": ["k_cand_step"], "top_map": ["k_top_map"],
                  "bitwise_not": ["k_bitwise_not"], "patch_warp": ["k_patch_warp"],
                  "patch_compare": ["k_patch_compare"], "tmpl_prep": ["k_tmpl_prep"]}
# fpm_model_profile's `which`: the variation model's kernels have no FPM_K_* index
MODEL_TRAIN, MODEL_PREPARE, MODEL_INSPECT = 0, 1, 2
MODEL_KERNEL_SYMBOLS = ["k_model_accum", "k_model_prepare", "k_model_inspect"]
MODEL_MAX_SAMPLES = 65535
# fpm_align_*: the call flag of fpm_align_last beside COMPARE_NORMALIZE, the result flags, the rectangle's caps; the kernel
# has no FPM_K_* index (fpm_align_profile)
ALIGN_ADOPT = 2
ALIGN_SINGULAR, ALIGN_STEP_CLAMPED, ALIGN_KEPT_START = 1, 2, 4
ALIGN_MAX_AREA, ALIGN_MAX_SIDE, ALIGN_MAX_ITERS, ALIGN_MAX_STEP = 1 << 20, 4096, 8, 1024.0
ALIGN_KERNEL_SYMBOL = "k_patch_align"
# fpm_blobs_host: the summary's flag and the capacity rules
BLOBS_TRUNCATED = 1
BLOBS_MAX_CAP, BLOBS_MAX_SLOTS = 65536, 1 << 22
# fpm_blobs_profile's `which`: the labelling kernels have no FPM_K_* index
BLOB_TILE, BLOB_MERGE, BLOB_FLATTEN, BLOB_SLOTS, BLOB_FEATURES = 0, 1, 2, 3, 4
BLOB_KERNEL_SYMBOLS = ["k_blob_tile", "k_blob_merge", "k_blob_flatten", "k_blob_slots", "k_blob_features"]
# fpm_last_calipers / fpm_calipers_at: the summary's flags and the caps; the kernel has no FPM_K_* index
# (fpm_caliper_profile)
CALIPER_TRUNCATED, CALIPER_OUTSIDE = 1, 2
CALIPER_MAX_LENGTH, CALIPER_MAX_WIDTH, CALIPER_MAX_HALF = 1024, 256, 16
CALIPER_MAX_CALS, CALIPER_MAX_CAP, CALIPER_MAX_SLOTS = 64, 64, 1 << 22
CALIPER_KERNEL_SYMBOL = "k_caliper"
# gray-value tools (fpm_hist_derive / fpm_last_histogram / fpm_last_segment ..): flags, the Otsu threshold value, the
# caps, and fpm_gray_profile's `which`
HIST_EMPTY, HIST_FLAT, GRAY_OUTSIDE = 1, 2, 4
SEG_OTSU = -1
GRAY_MAX_RECTS, GRAY_MAX_JOBS = 64, 65536
GRAY_HIST, GRAY_THRESHOLD = 0, 1
GRAY_KERNEL_SYMBOLS = ["k_patch_hist", "k_patch_threshold"]
# sub-pattern locators (fpm_locate_host / fpm_locate_derive / fpm_last_locate / fpm_locate_at): flags and caps
LOCATE_EDGE_X, LOCATE_EDGE_Y, LOCATE_FLAT, LOCATE_OUTSIDE = 1, 2, 4, 8
LOCATE_MAX_SIDE, LOCATE_MAX_RADIUS, LOCATE_MAX_FEATURES, LOCATE_MAX_JOBS = 128, 16, 64, 65536
LOCATE_KERNEL_SYMBOL = "k_patch_locate"
# edge probes (fpm_probe_* / fpm_last_probes / fpm_probes_at / fpm_fit_*): select rules, flags and caps; the kernel has
# no FPM_K_* index (fpm_probe_profile)
PROBE_NEAREST, PROBE_STRONGEST, PROBE_FIRST, PROBE_LAST = 0, 1, 2, 3
PROBE_OUTSIDE = 1
PROBE_MIN_LENGTH, PROBE_MAX_LENGTH, PROBE_MAX_WIDTH, PROBE_MAX_HALF = 4, 64, 16, 8
PROBE_MAX, PROBE_MAX_SLOTS = 4096, 1 << 22
PROBE_KERNEL_SYMBOL = "k_probe"
FIT_NOT_CONVERGED, FIT_COLLINEAR, FIT_TRIM_STARVED = 1, 2, 4


class Params(C.Structure):
    """fpm_params — the 7 TemplateMatcher setters + hidden range members (TemplateMatcher.h:22-28, 88-89), then the
    MFC tool's fast mode and bitwise-not switches (MatchToolDlg.cpp:936, :788)."""

    _fields_ = [
        ("max_pos", C.c_int32),
        ("min_reduce_area", C.c_int32),
        ("max_overlap", C.c_double),
        ("score", C.c_double),
        ("tolerance_angle", C.c_double),
        ("use_simd", C.c_int32),
        ("subpixel", C.c_int32),
        ("tolerance_range", C.c_int32),
        ("semantics", C.c_int32),
        ("tolerance", C.c_double * 4),
        ("top_angle_step", C.c_double),
        ("stop_layer", C.c_int32),
        ("bitwise_not", C.c_int32),
    ]


class Result(C.Structure):
    """fpm_result — POD-identical to s_SingleTargetMatch (DataStructures.h:97-115)."""

    _fields_ = [(n, C.c_double) for n in (
        "lt_x", "lt_y", "rt_x", "rt_y", "rb_x", "rb_y", "lb_x", "lb_y", "cx", "cy", "angle", "score")]


class Candidate(C.Structure):
    """fpm_candidate — one top-layer candidate (s_MatchParameter, DataStructures.h:58-94) and its refinement."""

    _fields_ = [("top_score", C.c_double), ("x", C.c_double), ("y", C.c_double), ("score", C.c_double),
                ("angle", C.c_double), ("angle_index", C.c_int32), ("peak_rank", C.c_int32), ("source", C.c_int32),
                ("kept", C.c_int32)]


class PatchRect(C.Structure):
    """fpm_patch_rect — a patch's rectangle in template coordinates."""

    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class CompareStats(C.Structure):
    """fpm_compare_stats — one hit against the template (fpm_last_compare / fpm_compare_at)."""

    _fields_ = [("n", C.c_int64), ("sum_i", C.c_int64), ("sum_ii", C.c_int64), ("sum_t", C.c_int64),
                ("sum_tt", C.c_int64), ("sum_it", C.c_int64), ("sum_abs", C.c_int64),
                ("n_over", C.c_int32), ("max_abs", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("x1", C.c_int32), ("y1", C.c_int32),
                ("zncc", C.c_double), ("gain", C.c_double), ("offset", C.c_double)]


class InspectStats(C.Structure):
    """fpm_inspect_stats — one hit against the variation model (fpm_last_inspect / fpm_inspect_at)."""

    _fields_ = [("n", C.c_int64), ("sum_excess", C.c_int64),
                ("n_low", C.c_int32), ("n_high", C.c_int32), ("max_excess", C.c_int32), ("x0", C.c_int32),
                ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
                ("gain", C.c_double), ("offset", C.c_double)]


class AlignSums(C.Structure):
    """fpm_align_sums -- the exact sums of one Gauss-Newton step of a hit's pose (fpm_align_sums_at)."""

    _fields_ = [(n, C.c_int64) for n in ("n_used", "h_xx", "h_xy", "h_yy", "h_xt", "h_yt", "h_tt", "g_x", "g_y", "g_t",
                                         "ssd")]


class AlignResult(C.Structure):
    """fpm_align_result -- one hit's aligned pose (fpm_align_at / fpm_align_last)."""

    _fields_ = [("lt_x", C.c_float), ("lt_y", C.c_float), ("angle", C.c_double), ("ssd_start", C.c_int64),
                ("ssd", C.c_int64), ("n_used", C.c_int64), ("evals", C.c_int32), ("best_eval", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class Blob(C.Structure):
    """fpm_blob -- one connected component of an excess image (fpm_blobs_host)."""

    _fields_ = [(n, C.c_int32) for n in ("hit", "seed", "area", "x0", "y0", "x1", "y1", "max_value")] + \
               [(n, C.c_int64) for n in ("sum_value", "sum_x", "sum_y")]


class BlobSummary(C.Structure):
    """fpm_blob_summary -- one image's counts (fpm_blobs_host)."""

    _fields_ = [("fg_pixels", C.c_int64)] + \
               [(n, C.c_int32) for n in ("n_components", "n_blobs", "n_returned", "largest_area", "flags", "reserved")]


class Caliper(C.Structure):
    """fpm_caliper -- one caliper, drawn on the taught image (fpm_last_calipers / fpm_calipers_at)."""

    _fields_ = [("cx", C.c_double), ("cy", C.c_double), ("phi", C.c_double)] + \
               [(n, C.c_int32) for n in ("length", "width", "half", "contrast", "polarity", "reserved")]


class EdgeRaw(C.Structure):
    """fpm_edge_raw -- the four exact integers of one edge (fpm_caliper_edges_host)."""

    _fields_ = [(n, C.c_int32) for n in ("index", "d_prev", "d", "d_next")]


class Edge(C.Structure):
    """fpm_edge -- one edge: the raw integers and what fpm_caliper_derive makes of them."""

    _fields_ = [(n, C.c_int32) for n in ("index", "d_prev", "d", "d_next")] + \
               [(n, C.c_double) for n in ("t", "contrast", "tx", "ty", "sx", "sy")]


class CaliperSummary(C.Structure):
    """fpm_caliper_summary -- one (hit, caliper): counts, flags and the sampling pose."""

    _fields_ = [(n, C.c_int32) for n in ("n_edges", "n_returned", "strongest", "flags")] + \
               [("lt_x", C.c_float), ("lt_y", C.c_float), ("angle", C.c_double)]


class HistStats(C.Structure):
    """fpm_hist_stats -- what fpm_hist_derive makes of one 256-bin histogram."""

    _fields_ = [(n, C.c_int64) for n in ("n", "sum", "sum_sq")] + \
               [(n, C.c_int32) for n in ("min", "max", "median", "otsu")] + \
               [("mean", C.c_double), ("stddev", C.c_double), ("flags", C.c_int32), ("reserved", C.c_int32)]


class SegmentInfo(C.Structure):
    """fpm_segment_info -- one hit of fpm_last_segment / fpm_segment_at: used pixels, the threshold used, flags."""

    _fields_ = [("n", C.c_int64), ("threshold", C.c_int32), ("flags", C.c_int32)]


class Feature(C.Structure):
    """fpm_feature -- a region of the template to find again on a hit, with its search radii."""

    _fields_ = [(n, C.c_int32) for n in ("x", "y", "w", "h", "rx", "ry")] + [("reserved", C.c_int32 * 2)]


class LocateRaw(C.Structure):
    """fpm_locate_raw -- what k_patch_locate writes per (hit, feature): the peak and the integer sums around it."""

    _fields_ = [(n, C.c_int32) for n in ("dx", "dy", "flags", "reserved")] + \
               [(n, C.c_int64) for n in ("n", "sum_t", "sum_tt")] + \
               [(n, C.c_int32 * 9) for n in ("s_i", "s_ii", "s_it")] + \
               [(n, C.c_int32) for n in ("c_i", "c_ii", "c_it")]


class LocateResult(C.Structure):
    """fpm_locate_result -- what fpm_locate_derive makes of one raw record."""

    _fields_ = [(n, C.c_int32) for n in ("dx", "dy", "flags", "reserved")] + \
               [(n, C.c_double) for n in ("score", "score_nominal", "ox", "oy", "tx", "ty", "sx", "sy")]


class Probe(C.Structure):
    """fpm_probe -- one edge probe: the nominal edge point and the scan direction, template frame."""

    _fields_ = [("x", C.c_double), ("y", C.c_double), ("phi", C.c_double)]


class ProbeParams(C.Structure):
    """fpm_probe_params -- the size and rules all probes of a call share."""

    _fields_ = [(n, C.c_int32) for n in ("length", "width", "half", "contrast", "polarity", "select")] + \
               [("reserved", C.c_int32 * 2)]


class ProbeRaw(C.Structure):
    """fpm_probe_raw -- what k_probe writes per (hit, probe): the selected edge's integers, the count, the flags."""

    _fields_ = [(n, C.c_int32) for n in ("index", "n_edges", "d_prev", "d", "d_next", "flags")]


class ProbeResult(C.Structure):
    """fpm_probe_result -- what fpm_probe_derive makes of one raw record."""

    _fields_ = [(n, C.c_int32) for n in ("index", "n_edges", "d", "flags")] + \
               [(n, C.c_double) for n in ("dev", "contrast", "tx", "ty", "sx", "sy")]


class ProbeSummary(C.Structure):
    """fpm_probe_summary -- one hit: counts, the deviation sums and the hit's pose."""

    _fields_ = [(n, C.c_int32) for n in ("n_found", "n_missing", "n_ambiguous", "n_outside", "worst", "reserved")] + \
               [(n, C.c_double) for n in ("sum_dev", "sum_dev_sq", "max_abs_dev")] + \
               [("lt_x", C.c_float), ("lt_y", C.c_float), ("angle", C.c_double)]


class LineFit(C.Structure):
    """fpm_line_fit -- fpm_fit_line's result."""

    _fields_ = [(n, C.c_double) for n in ("angle", "px", "py", "rms", "max_resid")] + \
               [("n_used", C.c_int32), ("flags", C.c_int32)]


class CircleFit(C.Structure):
    """fpm_circle_fit -- fpm_fit_circle's result."""

    _fields_ = [(n, C.c_double) for n in ("cx", "cy", "r", "rms", "max_resid")] + \
               [("n_used", C.c_int32), ("flags", C.c_int32)]


class RoiRecord(C.Structure):
    """fpm_roi_record — what the search keeps of one refinement ROI's 7x7 map."""

    _fields_ = [("score", C.c_float), ("mx", C.c_int32), ("my", C.c_int32), ("on_border", C.c_int32),
                ("vec", C.c_float * 9)]


class Peak(C.Structure):
    """fpm_peak — one top-layer peak (fpm_op_peaks)."""

    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("score", C.c_float)]


PEAKS_STATS_CALL, PEAKS_STATS_JOB = 8, 4   # FPM_PEAKS_STATS_CALL / _JOB
PEAKS_RAN_BLOCKS, PEAKS_RAN_NMS, PEAKS_RAN_FAST, PEAKS_RAN_GREEDY = 1, 2, 4, 8   # stats[0] of fpm_op_peaks
TOP_MAPS_STATS = 8   # FPM_TOP_MAPS_STATS
TOP_FUSED_STATS = 10  # FPM_TOP_FUSED_STATS
TOP_FORM_EXACT16, TOP_FORM_EXACT14, TOP_FORM_SMALL, TOP_FORM_LARGE = 0, 1, 2, 3   # stats[5] of fpm_op_top_maps

# every symbol include/fpm.h declares, with (restype, argtypes)
_P = C.c_void_p
_U8P = C.POINTER(C.c_uint8)
SIGNATURES = {
    "fpm_params_default": (None, [C.POINTER(Params)]),
    "fpm_abi_version": (C.c_int, []),
    "fpm_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "fpm_destroy": (C.c_int, [_P]),
    "fpm_last_error": (C.c_char_p, [_P]),
    "fpm_set_params": (C.c_int, [_P, C.POINTER(Params)]),
    "fpm_get_params": (C.c_int, [_P, C.POINTER(Params)]),
    "fpm_learn": (C.c_int, [_P, _U8P, C.c_int32, C.c_int32, C.c_size_t]),
    "fpm_clear_pattern": (C.c_int, [_P]),
    "fpm_is_learned": (C.c_int, [_P]),
    "fpm_match": (C.c_int, [_P, _U8P, C.c_int32, C.c_int32, C.c_size_t, C.POINTER(Result), C.c_int32,
                            C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "fpm_stage_sources": (C.c_int, [_P, C.POINTER(_U8P), C.c_int32, C.c_int32, C.c_int32, C.c_size_t]),
    "fpm_stage_sources_device": (C.c_int, [_P, C.POINTER(_P), C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.c_size_t,
                                           C.c_int32, _P]),
    "fpm_match_device": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_size_t, C.c_size_t, C.c_int32, _P,
                                   C.POINTER(Result), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "fpm_match_staged": (C.c_int, [_P, C.POINTER(Result), C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_match_staged_launch": (C.c_int, [_P]),
    "fpm_match_staged_finish": (C.c_int, [_P, C.POINTER(Result), C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_op_pyr_down": (C.c_int, [_P, _U8P, C.c_int32, C.c_int32, C.c_size_t, _U8P, C.c_size_t]),
    "fpm_op_pyr_down2": (C.c_int, [_P, _U8P, C.c_int32, C.c_int32, C.c_size_t, _U8P, C.c_size_t, _U8P, C.c_size_t,
                                   C.c_int32, C.c_int32]),
    "fpm_op_bitwise_not": (C.c_int, [_P, _U8P, C.c_int32, C.c_int32, C.c_size_t, _U8P, C.c_size_t]),
    "fpm_op_to_gray": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32, _U8P,
                                 C.c_size_t]),
    "fpm_op_warp_affine": (C.c_int, [_P, _U8P, C.c_int32, C.c_int32, C.c_size_t, C.POINTER(C.c_double), _U8P,
                                     C.c_int32, C.c_int32, C.c_size_t, C.c_int32]),
    "fpm_op_ncc_map": (C.c_int, [_P, _U8P, C.c_int32, C.c_int32, C.c_size_t, C.c_int32, C.c_int32,
                                 C.POINTER(C.c_float)]),
    "fpm_op_refine": (C.c_int, [_P, C.POINTER(_U8P), C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.c_int32,
                                C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.POINTER(RoiRecord), _U8P, C.POINTER(C.c_int32)]),
    "fpm_op_peaks": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                               C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                               C.c_int32, C.c_int32, C.c_uint32, C.POINTER(Peak), C.POINTER(C.c_int32),
                               C.POINTER(C.c_int32)]),
    "fpm_op_top_maps": (C.c_int, [_P, C.c_int32, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32,
                                  C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int32)]),
    "fpm_op_top_fused": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_float),
                                   C.c_int64, C.POINTER(Peak), C.POINTER(C.c_int32), C.POINTER(Peak),
                                   C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int32)]),
    "fpm_op_overlap_filter": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_int32, C.c_double,
                                        C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "fpm_template_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "fpm_template_level": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int32), _U8P, C.c_size_t]),
    "fpm_set_angle_shard": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "fpm_get_angle_shard": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "fpm_last_candidates": (C.c_int, [_P, C.c_int32, C.POINTER(Candidate), C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_last_results": (C.c_int, [_P, C.POINTER(Result), C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_patch_matrix": (C.c_int, [C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_double, C.c_int32, C.c_int32,
                                   C.POINTER(C.c_double)]),
    "fpm_last_patches": (C.c_int, [_P, C.POINTER(PatchRect), C.c_int32, _U8P, C.c_size_t, C.c_size_t, C.c_int32,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "fpm_last_patches_device": (C.c_int, [_P, C.POINTER(PatchRect), C.c_int32, _P, C.c_size_t, C.c_size_t, C.c_int32,
                                          C.POINTER(C.c_int32), _P]),
    "fpm_patches_at": (C.c_int, [_P, C.POINTER(PatchRect), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                 C.POINTER(C.c_double), C.c_int32, _U8P, C.c_size_t, C.c_size_t,
                                 C.POINTER(C.c_double)]),
    "fpm_set_patch_form": (C.c_int, [_P, C.c_int32]),
    "fpm_last_compare": (C.c_int, [_P, C.POINTER(PatchRect), C.c_int32, C.c_int32, C.c_int32, C.POINTER(CompareStats),
                                   C.c_int32, C.POINTER(C.c_int32), _U8P, C.c_size_t, C.c_size_t]),
    "fpm_compare_at": (C.c_int, [_P, C.POINTER(PatchRect), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                 C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_int32, C.POINTER(CompareStats), _U8P,
                                 C.c_size_t, C.c_size_t]),
    "fpm_compare_derive": (C.c_int, [C.c_int64] * 6 + [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                       C.POINTER(C.c_double), _U8P]),
    "fpm_learn_device": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_size_t, C.c_size_t, C.c_int32, _P]),
    "fpm_learn_at": (C.c_int, [_P, C.POINTER(PatchRect), C.c_int32, C.c_float, C.c_float, C.c_double]),
    "fpm_learn_hit": (C.c_int, [_P, C.POINTER(PatchRect), C.c_int32, C.c_int32]),
    "fpm_learn_derive": (C.c_int, [C.c_int64] * 3 + [C.POINTER(C.c_double)] * 3 + [C.POINTER(C.c_int32)]),
    "fpm_template_operands": (C.c_int, [_P, C.POINTER(C.c_int8), C.POINTER(C.c_size_t), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_size_t)]),
    "fpm_model_clear": (C.c_int, [_P]),
    "fpm_model_set_chunk": (C.c_int, [_P, C.c_int32]),
    "fpm_model_train_last": (C.c_int, [_P, C.POINTER(PatchRect), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_model_train_at": (C.c_int, [_P, C.POINTER(PatchRect), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                     C.POINTER(C.c_double), C.c_int32, C.c_int32]),
    "fpm_model_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(PatchRect)]),
    "fpm_model_sums": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fpm_model_images": (C.c_int, [_P, C.c_int32, C.c_int32, _U8P, _U8P, _U8P, C.c_size_t]),
    "fpm_last_inspect": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(InspectStats), C.c_int32,
                                   C.POINTER(C.c_int32), _U8P, C.c_size_t, C.c_size_t]),
    "fpm_inspect_at": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_int32,
                                 C.c_int32, C.c_int32, C.c_int32, C.POINTER(InspectStats), _U8P, C.c_size_t,
                                 C.c_size_t]),
    "fpm_model_learn": (C.c_int, [_P]),
    "fpm_model_derive": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32] + [C.POINTER(C.c_int32)] * 3),
    "fpm_model_profile": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int64)]),
    "fpm_align_sums_at": (C.c_int, [_P, C.POINTER(PatchRect), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                    C.POINTER(C.c_double), C.c_int32, C.c_int32, C.POINTER(AlignSums)]),
    "fpm_align_at": (C.c_int, [_P, C.POINTER(PatchRect), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                               C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_double, C.c_int32,
                               C.POINTER(AlignResult)]),
    "fpm_align_last": (C.c_int, [_P, C.POINTER(PatchRect), C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                 C.POINTER(AlignResult), C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_align_solve": (C.c_int, [C.POINTER(AlignSums)] + [C.POINTER(C.c_double)] * 3),
    "fpm_align_update": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(PatchRect), C.c_float, C.c_float, C.c_double,
                                   C.c_double, C.c_double, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                   C.POINTER(C.c_double)]),
    "fpm_align_profile": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "fpm_blobs_host": (C.c_int, [_U8P, C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                                 C.POINTER(BlobSummary), C.POINTER(Blob), C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_last_blobs": (C.c_int, [_P] + [C.c_int32] * 7 + [C.POINTER(InspectStats), C.POINTER(BlobSummary), C.POINTER(Blob),
                                                          C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_blobs_at": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)] + [C.c_int32] * 7 +
                     [C.POINTER(InspectStats), C.POINTER(BlobSummary), C.POINTER(Blob), C.c_int32]),
    "fpm_op_blobs": (C.c_int, [_P, _U8P, C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                               C.POINTER(BlobSummary), C.POINTER(Blob), C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_blobs_set_round": (C.c_int, [_P, C.c_int32]),
    "fpm_blobs_profile": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "fpm_caliper_pose": (C.c_int, [C.c_float, C.c_float, C.c_double, C.POINTER(Caliper), C.POINTER(C.c_float),
                                   C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "fpm_caliper_edges_host": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(Caliper), C.c_int32, C.POINTER(EdgeRaw),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "fpm_caliper_derive": (C.c_int, [C.POINTER(Caliper), C.c_float, C.c_float, C.c_double, C.POINTER(EdgeRaw), C.c_int32,
                                     C.POINTER(Edge)]),
    "fpm_calipers_at": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_int32,
                                  C.POINTER(Caliper), C.c_int32, C.c_int32, C.POINTER(CaliperSummary), C.POINTER(Edge),
                                  C.POINTER(C.c_int32), C.c_int32]),
    "fpm_last_calipers": (C.c_int, [_P, C.c_int32, C.POINTER(Caliper), C.c_int32, C.c_int32, C.POINTER(CaliperSummary),
                                    C.POINTER(Edge), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_caliper_profile": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "fpm_mask_set": (C.c_int, [_P, _U8P, C.c_int32, C.c_int32, C.c_size_t]),
    "fpm_mask_set_device": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_size_t, _P]),
    "fpm_mask_clear": (C.c_int, [_P]),
    "fpm_mask_enable": (C.c_int, [_P, C.c_int32]),
    "fpm_mask_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                C.POINTER(C.c_int32)]),
    "fpm_mask_get": (C.c_int, [_P, _U8P, C.c_size_t]),
    "fpm_mask_count": (C.c_int, [_P, C.POINTER(PatchRect), C.POINTER(C.c_int64)]),
    "fpm_hist_derive": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(HistStats)]),
    "fpm_last_histogram": (C.c_int, [_P, C.POINTER(PatchRect), C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.c_int32,
                                     C.POINTER(C.c_int32)]),
    "fpm_histogram_at": (C.c_int, [_P, C.POINTER(PatchRect), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                   C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_uint32)]),
    "fpm_last_segment": (C.c_int, [_P, C.c_int32, C.POINTER(PatchRect), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.POINTER(SegmentInfo), C.POINTER(BlobSummary), C.POINTER(Blob), C.c_int32, C.c_int32,
                                   C.POINTER(C.c_int32), _U8P, C.c_size_t, C.c_size_t]),
    "fpm_segment_at": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_int32,
                                 C.POINTER(PatchRect), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SegmentInfo),
                                 C.POINTER(BlobSummary), C.POINTER(Blob), C.c_int32, _U8P, C.c_size_t, C.c_size_t]),
    "fpm_gray_set_run": (C.c_int, [_P, C.c_int32]),
    "fpm_gray_profile": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "fpm_locate_host": (C.c_int, [_U8P, C.c_size_t, _U8P, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.POINTER(LocateRaw), C.POINTER(C.c_int32)]),
    "fpm_locate_derive": (C.c_int, [C.POINTER(Feature), C.c_float, C.c_float, C.c_double, C.POINTER(LocateRaw),
                                    C.POINTER(LocateResult)]),
    "fpm_locate_at": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_int32,
                                C.POINTER(Feature), C.c_int32, C.POINTER(LocateResult), C.POINTER(LocateRaw),
                                C.POINTER(C.c_int32), C.c_int32]),
    "fpm_last_locate": (C.c_int, [_P, C.c_int32, C.POINTER(Feature), C.c_int32, C.POINTER(LocateResult),
                                  C.POINTER(LocateRaw), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_locate_profile": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "fpm_probe_matrix": (C.c_int, [C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_double, C.POINTER(Probe),
                                   C.POINTER(ProbeParams), C.POINTER(C.c_double)]),
    "fpm_probe_edges_host": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(ProbeParams), C.POINTER(ProbeRaw)]),
    "fpm_probe_derive": (C.c_int, [C.POINTER(Probe), C.POINTER(ProbeParams), C.c_float, C.c_float, C.c_double,
                                   C.POINTER(ProbeRaw), C.c_int32, C.POINTER(ProbeResult)]),
    "fpm_probes_at": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_int32,
                                C.POINTER(Probe), C.c_int32, C.POINTER(ProbeParams), C.POINTER(ProbeSummary),
                                C.POINTER(ProbeResult), C.POINTER(C.c_int32), C.c_int32]),
    "fpm_last_probes": (C.c_int, [_P, C.c_int32, C.POINTER(Probe), C.c_int32, C.POINTER(ProbeParams),
                                  C.POINTER(ProbeSummary), C.POINTER(ProbeResult), C.POINTER(C.c_int32), C.c_int32,
                                  C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_probe_profile": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "fpm_fit_line": (C.c_int, [C.POINTER(C.c_double), C.c_int32, C.c_double, C.POINTER(LineFit)]),
    "fpm_fit_circle": (C.c_int, [C.POINTER(C.c_double), C.c_int32, C.c_double, C.POINTER(CircleFit)]),
    "fpm_merge_candidates": (C.c_int, [C.POINTER(Params), C.c_int32, C.c_int32, C.POINTER(Candidate), C.c_int32,
                                       C.POINTER(Result), C.c_int32, C.POINTER(C.c_int32)]),
    "fpm_search_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.c_int32]),
    "fpm_search_bytes": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "fpm_profile_enable": (C.c_int, [_P, C.c_int32]),
    "fpm_profile_reset": (C.c_int, [_P]),
    "fpm_profile_get": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64)]),
    "fpm_profile_last": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

_lib = None


def build_library(force: bool = False) -> str:
    """Compile libfpm_hip.so in-tree with hipcc for gfx950 (no-op when up to date)."""
    cmd = ["make", "-C", CSRC, "-j8"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"])
    subprocess.check_call(cmd)
    return LIB_PATH


def load(build_if_missing: bool = True) -> C.CDLL:
    """Load libfpm_hip.so; raises if it cannot be built or loaded (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if not build_if_missing:
            raise RuntimeError(f"{LIB_PATH} not built; run make -C {CSRC}")
        build_library()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def hip_runtimes():
    """Paths of the HIP runtime libraries (libamdhip64) mapped into this process.  Device pointers and stream handles
    mean something only inside the runtime that made them, so the device-memory entries need the caller's framework and
    libfpm_hip.so on ONE runtime.  A torch wheel bundles its own libamdhip64 under the system library's soname: imported
    before libfpm_hip.so is loaded, the dynamic linker gives both the same copy; imported after it, the process ends up
    with two runtimes and torch's tensors are foreign to the library."""
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.split(None, 5)[-1].strip() if line.count("/") else ""
                if os.path.basename(path).startswith("libamdhip64.so"):
                    paths.add(os.path.realpath(path))
    except OSError:
        pass
    return sorted(paths)


def u8ptr(a):
    return a.ctypes.data_as(_U8P)
