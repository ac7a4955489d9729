"""ctypes view of the C ABI declared in include/mtgpu.h / include/mt_types.h.

The product path is the HIP library ``libmtgpu.so`` built in-tree by
``csrc/Makefile``.  There is no Python or CPU fallback: if the library is missing
``load_library()`` raises, and every compute entry point of the library itself
fails with MT_ERR_DEVICE when no gfx950 device is usable.
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libmtgpu.so")

LAYOUT_COMPACT8, LAYOUT_AOS40, LAYOUT_ZERO_COPY, LAYOUT_CENTRES = 0, 1, 2, 4
LAYOUT_BOXES = 8                                    # include/mtgpu_pipe_boxes.h
SWEEP_MAX_LEVELS = 16
SWEEP_MAX_THRESHOLDS, SWEEP_MAX_VECTORS = 8, 8      # include/mtgpu_sweep.h
COMPACT_DTYPE = np.dtype([("src_x", "<i2"), ("src_y", "<i2"), ("dst_x", "<i2"), ("dst_y", "<i2")])
MT_OK, MT_ERR_INVALID, MT_ERR_CAPACITY, MT_ERR_DEVICE, MT_ERR_NOMEM, MT_ERR_BUSY, MT_ERR_UNSUPPORTED = 0, 1, 2, 3, 4, 5, 6
# copy-out loops of mtgpu_pack_records_with (include/mtgpu.h)
PACK_SCALAR, PACK_AVX2, PACK_AVX512, PACK_IMPL_MASK, PACK_NT = 1, 2, 3, 15, 16

# AVMotionVector-compatible record (include/mt_types.h: mt_mv; 40 bytes).
MV_DTYPE = np.dtype(
    {
        "names": ["source", "w", "h", "src_x", "src_y", "dst_x", "dst_y", "flags",
                  "motion_x", "motion_y", "motion_scale"],
        "formats": ["<i4", "u1", "u1", "<i2", "<i2", "<i2", "<i2", "<u8", "<i4", "<i4", "<u2"],
        "offsets": [0, 4, 5, 6, 8, 10, 12, 16, 24, 28, 32],
        "itemsize": 40,
    }
)
SEGMENT_DTYPE = np.dtype([("start", "<f8"), ("end", "<f8")])
# mt_blob_box (include/mtgpu_blobs.h): inclusive cell bounds of a frame's largest blob, all 0xFFFF: no blob
BLOB_BOX_DTYPE = np.dtype([("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2")])
# mt_object (include/mtgpu_objects.h): one blob of a frame's list — its cell count (0: no such blob), the smallest
# y * grid_w + x of its cells, its inclusive cell bounds; an empty entry reads {0, 0xFFFFFFFF, 0xFFFF x 4}
OBJECT_DTYPE = np.dtype([("cells", "<u4"), ("first", "<u4"), ("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2")])
OBJECTS_MAX, OBJECT_TABLE_BYTES = 16, 24
# mt_heading (include/mtgpu_headings.h): the motion of one list entry — the belonging records per sector (0 = E,
# clockwise), all belonging records, the heading (HEADING_NONE: every bin is 0), the summed displacement; an empty entry
# reads zeros with heading = HEADING_NONE
HEADING_DTYPE = np.dtype([("n", "<u4", (8,)), ("records", "<u4"), ("heading", "<u4"), ("sum_dx", "<i8"), ("sum_dy", "<i8"),
                          ("reserved", "<u8")])
HEADING_NONE, HEADING_TABLE_BYTES = 0xFFFFFFFF, 56
# mt_gmc_info (include/mtgpu_gmc.h): the applied vector, the modes of the two axes, the counted records, the modes' counts
GMC_INFO_DTYPE = np.dtype([("gx", "<i2"), ("gy", "<i2"), ("mode_x", "<i2"), ("mode_y", "<i2"), ("n_in", "<u4"), ("n_x", "<u4"),
                           ("n_y", "<u4")])
GMC_MAX_SHIFT, GMC_DEFAULT_MAX_SHIFT, GMC_DEFAULT_MIN_SHARE_Q8 = 127, 16, 128
MERGE_PARAMS_DTYPE = np.dtype([("max_gap_sec", "<f8"), ("padding_sec", "<f8"),
                               ("duration", "<f8"), ("min_savings_pct", "<f8")])
MERGE_RESULT_DTYPE = np.dtype([("n_timestamps", "<u8"), ("n_segments", "<u8"),
                               ("time_removed", "<f8"), ("saved_pct", "<f8"),
                               ("do_cut", "<i4"), ("status", "<i4")])


class ScanParamsC(C.Structure):
    _fields_ = [("mv_threshold_sq", C.c_double), ("block_shift", C.c_int32),
                ("clusters_needed", C.c_int32), ("vertical_margin", C.c_int32),
                ("vectors_needed", C.c_uint8), ("_pad", C.c_uint8 * 3),
                ("grid_w", C.c_int32), ("grid_h", C.c_int32)]


class MergeParamsC(C.Structure):
    _fields_ = [("max_gap_sec", C.c_double), ("padding_sec", C.c_double),
                ("duration", C.c_double), ("min_savings_pct", C.c_double)]


class MergeResultC(C.Structure):
    _fields_ = [("n_timestamps", C.c_uint64), ("n_segments", C.c_uint64),
                ("time_removed", C.c_double), ("saved_pct", C.c_double),
                ("do_cut", C.c_int32), ("status", C.c_int32)]


class PlanC(C.Structure):
    _fields_ = [("block_threads", C.c_int32), ("bands", C.c_int32), ("band_rows", C.c_int32),
                ("lds_bytes", C.c_int32), ("counter_bits", C.c_int32), ("device", C.c_int32),
                ("cu_count", C.c_int32), ("chunk_rows", C.c_int32),
                # _pad: mtgpu_plan::early_exit.  It keeps the name it had as padding: MotionScanner.plan and plan_preview
                # list the fields without an underscore, and what they hand the library and return is a recorded surface
                # (tests/golden/scanner_calls.json); early_exit.py reads it.
                ("counter_mode", C.c_int32), ("_pad", C.c_int32)]


class SweepPlanC(C.Structure):
    _fields_ = [("thresholds_per_pass", C.c_int32), ("passes", C.c_int32), ("lds_bytes", C.c_int32),
                ("counter_bits", C.c_int32)]


class ActivityPlanC(C.Structure):
    _fields_ = [("lds_bytes", C.c_int32), ("acc_bits", C.c_int32), ("max_run", C.c_int32), ("workgroup", C.c_int32)]


class ZonesPlanC(C.Structure):
    _fields_ = [("lds_bytes", C.c_int32), ("workgroup", C.c_int32), ("keep_words_per_row", C.c_int32),
                ("keep_words_per_stream", C.c_int32)]


class BlobsPlanC(C.Structure):
    _fields_ = [("lds_bytes", C.c_int32), ("workgroup", C.c_int32), ("keep_words_per_row", C.c_int32),
                ("keep_words_per_stream", C.c_int32)]


class ObjectsPlanC(C.Structure):
    _fields_ = [("lds_bytes", C.c_int32), ("workgroup", C.c_int32), ("keep_words_per_row", C.c_int32),
                ("keep_words_per_stream", C.c_int32)]


class HeadingsPlanC(C.Structure):
    _fields_ = [("lds_bytes", C.c_int32), ("workgroup", C.c_int32), ("keep_words_per_row", C.c_int32),
                ("keep_words_per_stream", C.c_int32)]


class GmcPlanC(C.Structure):
    _fields_ = [("lds_bytes", C.c_int32), ("workgroup", C.c_int32), ("hist_bins", C.c_int32), ("info_bytes", C.c_int32)]


class GmcBlobsPlanC(C.Structure):
    _fields_ = [("lds_bytes", C.c_int32), ("workgroup", C.c_int32), ("keep_words_per_row", C.c_int32),
                ("keep_words_per_stream", C.c_int32), ("hist_bins", C.c_int32), ("info_bytes", C.c_int32)]


class PersistPlanC(C.Structure):
    _fields_ = [("workgroup", C.c_int32), ("frames_per_tile", C.c_int32)]


class TracksPlanC(C.Structure):
    _fields_ = [("workgroup", C.c_int32), ("frames_per_tile", C.c_int32), ("work_words_per_entry", C.c_int32)]


class DirPlanC(C.Structure):
    _fields_ = [("lds_bytes", C.c_int32), ("workgroup", C.c_int32), ("sectors", C.c_int32), ("rose_bytes", C.c_int32)]


class LanesPlanC(C.Structure):
    _fields_ = [("lds_bytes", C.c_int32), ("workgroup", C.c_int32), ("staged", C.c_int32), ("plane_bytes", C.c_int32)]


class CtxStatsC(C.Structure):
    _fields_ = [("staging_device_bytes", C.c_uint64), ("pool_reserved_bytes", C.c_uint64),
                ("pool_reserved_high", C.c_uint64), ("hip_streams", C.c_uint32), ("private_pool", C.c_uint32)]


class PipeStatsC(C.Structure):
    _fields_ = [("pinned_bytes", C.c_uint64), ("device_bytes", C.c_uint64), ("submits", C.c_uint64),
                ("n_buffers", C.c_uint32), ("layout", C.c_int32), ("pin_us", C.c_uint64),
                ("pinned_batches", C.c_uint32), ("hip_streams", C.c_uint32), ("list_bytes", C.c_uint64)]


assert C.sizeof(ScanParamsC) == 32 and C.sizeof(MergeResultC) == 40

# name -> (restype, argtypes): every symbol include/mtgpu.h declares.
ABI = {
    "mtgpu_version": (C.c_char_p, []),
    "mtgpu_last_error": (C.c_char_p, []),
    "mtgpu_device_count": (C.c_int, []),
    "mtgpu_device_pci_address": (C.c_int, [C.c_int, C.c_char_p, C.c_uint64]),
    "mtgpu_params_from_config": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.c_int, C.c_double,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]),
    "mtgpu_create": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.POINTER(C.c_void_p)]),
    "mtgpu_destroy": (None, [C.c_void_p]),
    "mtgpu_get_params": (C.c_int, [C.c_void_p, C.POINTER(ScanParamsC)]),
    "mtgpu_get_stats": (C.c_int, [C.c_void_p, C.POINTER(CtxStatsC)]),
    "mtgpu_trim": (C.c_int, [C.c_void_p]),
    "mtgpu_get_plan": (C.c_int, [C.c_void_p, C.POINTER(PlanC)]),
    "mtgpu_plan_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.c_int, C.POINTER(PlanC)]),
    "mtgpu_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "mtgpu_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "mtgpu_set_slices": (C.c_int, [C.c_void_p, C.c_int]),
    "mtgpu_scan_frames_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                           C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mtgpu_scan_frames_device_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                                   C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mtgpu_scan_centres_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                                            C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtgpu_scan_frames_centres": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                            C.c_void_p]),
    "mtgpu_flags_from_centres_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]),
    "mtgpu_sweep_streams_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                             C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "mtgpu_batch_centres": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mtgpu_pack_records": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "mtgpu_pack_records_with": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]),
    "mtgpu_pack_selected": (C.c_int, []),
    "mtgpu_scan_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_uint32, C.c_void_p]),
    "mtgpu_merge_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(MergeParamsC),
                                       C.c_int, C.c_void_p, C.c_uint64, C.POINTER(MergeResultC)]),
    "mtgpu_merge_timestamps_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(MergeParamsC),
                                                C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "mtgpu_merge_streams_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_uint32, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "mtgpu_pipe_create": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "mtgpu_pipe_create_layout": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int,
                                           C.POINTER(C.c_void_p)]),
    "mtgpu_pipe_destroy": (None, [C.c_void_p]),
    "mtgpu_pipe_acquire": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mtgpu_batch_add_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_double, C.c_uint64]),
    "mtgpu_batch_frames": (C.c_uint32, [C.c_void_p]),
    "mtgpu_pipe_submit": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mtgpu_pipe_collect": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]),
    "mtgpu_pipe_release": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mtgpu_pipe_get_stats": (C.c_int, [C.c_void_p, C.POINTER(PipeStatsC)]),
    "mtgpu_comm_unique_id": (C.c_int, [C.c_void_p]),
    "mtgpu_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "mtgpu_comm_destroy": (None, [C.c_void_p]),
    "mtgpu_gather_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_motion.h declares (the motion scalar; mtgpu.h includes it).
ABI_MOTION = {
    "mtgpu_motion_scores_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "mtgpu_motion_bins_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtgpu_motion_scalar": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_sweep.h declares (the setting sweep; mtgpu.h includes it).
ABI_SWEEP = {
    "mtgpu_scan_sweep_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.c_uint32, C.c_uint32, C.POINTER(SweepPlanC)]),
    "mtgpu_scan_sweep_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_int32), C.c_uint32, C.c_void_p,
                                          C.c_void_p]),
    "mtgpu_scan_frames_sweep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_double),
                                          C.c_uint32, C.POINTER(C.c_int32), C.c_uint32, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_activity.h declares (the activity maps; mtgpu.h includes it).
ABI_ACTIVITY = {
    "mtgpu_activity_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.POINTER(ActivityPlanC)]),
    "mtgpu_activity_map_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "mtgpu_activity_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_zones.h declares (the ignore zones; mtgpu.h includes it).
ABI_ZONES = {
    "mtgpu_zones_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.POINTER(ZonesPlanC)]),
    "mtgpu_scan_zones_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtgpu_scan_frames_zones": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_pipe_zones.h declares (the keep mask of a pipe; mtgpu.h includes it).
ABI_PIPE_ZONES = {
    "mtgpu_pipe_set_keep": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mtgpu_pipe_has_keep": (C.c_int, [C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_blobs.h declares (the motion blobs; mtgpu.h includes it).
ABI_BLOBS = {
    "mtgpu_blobs_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.POINTER(BlobsPlanC)]),
    "mtgpu_scan_blobs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtgpu_scan_frames_blobs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_pipe_blobs.h declares (the blob setting of a pipe; mtgpu.h includes it).
ABI_PIPE_BLOBS = {
    "mtgpu_pipe_set_blobs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int]),
    "mtgpu_pipe_blobs": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
}
MT_PIPE_REPORT_CENTRES, MT_PIPE_REPORT_LARGEST = 0, 1

# name -> (restype, argtypes): every symbol include/mtgpu_gmc.h declares (global-motion compensation; mtgpu.h includes it).
ABI_GMC = {
    "mtgpu_gmc_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.POINTER(GmcPlanC)]),
    "mtgpu_scan_gmc_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtgpu_scan_frames_gmc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_pipe_gmc.h declares (the compensation setting of a pipe; mtgpu.h includes it).
ABI_PIPE_GMC = {
    "mtgpu_pipe_set_gmc": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_int]),
    "mtgpu_pipe_gmc": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
}
MT_PIPE_REPORT_VECTOR = 2

# name -> (restype, argtypes): every symbol include/mtgpu_gmc_blobs.h declares (the compensated blob scan; mtgpu.h includes it).
ABI_GMC_BLOBS = {
    "mtgpu_gmc_blobs_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.POINTER(GmcBlobsPlanC)]),
    "mtgpu_scan_gmc_blobs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                              C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtgpu_scan_frames_gmc_blobs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                              C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_pipe_gmc_blobs.h declares (the compensated blob setting of a pipe; mtgpu.h includes it).
ABI_PIPE_GMC_BLOBS = {
    "mtgpu_pipe_set_gmc_blobs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int]),
    "mtgpu_pipe_gmc_blobs": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_persist.h declares (temporal persistence; mtgpu.h includes it).
ABI_PERSIST = {
    "mtgpu_persist_preview": (C.c_int, [C.POINTER(PersistPlanC)]),
    "mtgpu_persist_flags_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "mtgpu_persist_flags": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
}
PERSIST_NO_DROPOUT_LIMIT = 0xFFFFFFFF

# name -> (restype, argtypes): every symbol include/mtgpu_pipe_boxes.h declares (the boxes of a pipe's batch; mtgpu.h includes it).
ABI_PIPE_BOXES = {
    "mtgpu_batch_boxes": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_dir.h declares (the direction filter; mtgpu.h includes it).
ABI_DIR = {
    "mtgpu_dir_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.POINTER(DirPlanC)]),
    "mtgpu_scan_dir_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "mtgpu_scan_frames_dir": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                        C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
}
DIR_ALL, DIR_SECTORS = 0xFF, 8

# name -> (restype, argtypes): every symbol include/mtgpu_pipe_dir.h declares (the direction setting of a pipe; mtgpu.h includes it).
ABI_PIPE_DIR = {
    "mtgpu_pipe_set_dir": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, C.c_int]),
    "mtgpu_pipe_dir": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
}
MT_PIPE_REPORT_SECTORS = 3

# name -> (restype, argtypes): every symbol include/mtgpu_lanes.h declares (direction planes and flow maps; mtgpu.h includes it).
ABI_LANES = {
    "mtgpu_lanes_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.POINTER(LanesPlanC)]),
    "mtgpu_scan_lanes_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtgpu_scan_frames_lanes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtgpu_flow_map_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mtgpu_flow_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_pipe_lanes.h declares (the direction plane of a pipe; mtgpu.h includes it).
ABI_PIPE_LANES = {
    "mtgpu_pipe_set_plane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "mtgpu_pipe_plane": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_objects.h declares (object lists; mtgpu.h includes it).
ABI_OBJECTS = {
    "mtgpu_objects_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.c_int, C.POINTER(ObjectsPlanC)]),
    "mtgpu_scan_objects_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtgpu_scan_frames_objects": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                            C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/mtgpu_tracks.h declares (object tracks; mtgpu.h includes it).
ABI_TRACKS = {
    "mtgpu_tracks_preview": (C.c_int, [C.c_int, C.POINTER(TracksPlanC)]),
    "mtgpu_track_objects_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtgpu_track_objects": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
}
TRACK_NO_PRED, TRACK_NO_ID = 0xFF, 0xFFFFFFFF
TRACK_WORK_WORDS = 2                                 # mtgpu_tracks_plan.work_words_per_entry: uint32 words of d_work per list entry

# name -> (restype, argtypes): every symbol include/mtgpu_headings.h declares (object headings; mtgpu.h includes it).
ABI_HEADINGS = {
    "mtgpu_headings_preview": (C.c_int, [C.POINTER(ScanParamsC), C.c_int, C.c_int, C.POINTER(HeadingsPlanC)]),
    "mtgpu_scan_headings_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "mtgpu_scan_frames_headings": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                             C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# every table above, in header order: what load_library() binds
ABI_TABLES = (ABI, ABI_MOTION, ABI_SWEEP, ABI_ACTIVITY, ABI_ZONES, ABI_PIPE_ZONES, ABI_BLOBS, ABI_PIPE_BLOBS, ABI_GMC,
              ABI_PIPE_GMC, ABI_GMC_BLOBS, ABI_PIPE_GMC_BLOBS, ABI_PERSIST, ABI_PIPE_BOXES, ABI_DIR, ABI_PIPE_DIR, ABI_LANES,
              ABI_PIPE_LANES, ABI_OBJECTS, ABI_TRACKS, ABI_HEADINGS)

_lib = None


class MtgpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mtgpu error {code}: {msg}")
        self.code = code


def load_library(path=None):
    """Load libmtgpu.so (built by csrc/Makefile).  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # MTGPU_LIBRARY: another build of the same ABI (developers: e.g. a previous build for an interleaved A/B)
    p = path or os.environ.get("MTGPU_LIBRARY") or LIB_PATH
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7 /
    # libhsa-runtime64.so.1 (same SONAMEs as /opt/rocm).  If libmtgpu.so pulled in the
    # system copies first, a later `import torch` would find "No HIP GPUs".  Importing
    # torch first makes both share torch's runtime; without torch the system ROCm is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} not found: build it with `make -C {os.path.join(PKG_DIR, 'csrc')}` "
            "(or __graft_entry__.build()).  There is no fallback path.")
    lib = C.CDLL(p)
    for table in ABI_TABLES:
        for name, (res, args) in table.items():
            fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def check(rc):
    if rc != MT_OK:
        raise MtgpuError(rc, load_library().mtgpu_last_error().decode("utf-8", "replace"))
