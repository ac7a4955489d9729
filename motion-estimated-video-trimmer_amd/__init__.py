"""MI355X-native motion-vector scanner: the hot path of
Vaibhav-20022002/Motion-Estimated-Video-Trimmer (MotionScanner::check_frame + the
gap-bounded segment merge) as hand-written gfx950 HIP kernels behind the C ABI of
include/mtgpu.h.  This package is the thin host-side mirror of the reference's
scanner interface; the compute lives in libmtgpu.so (csrc/)."""
from . import config, mvfile, mvjson
from ._abi import (COMPACT_DTYPE, GMC_INFO_DTYPE, LAYOUT_AOS40, LAYOUT_BOXES, LAYOUT_CENTRES, LAYOUT_COMPACT8, LAYOUT_ZERO_COPY, LIB_PATH, MERGE_PARAMS_DTYPE, MERGE_RESULT_DTYPE, MV_DTYPE, SEGMENT_DTYPE,
                   MtgpuError, load_library)
from .scanner import (FrameBatch, activity_preview, blobs_preview, dir_preview, MergeParams, MotionScanner, ScanParams, ScanPipe, concat_list, filter_frames,
                      frame_skip, gmc_blobs_preview, gmc_preview, lanes_preview, make_chunks, pack_records, persist_preview, plan_preview, results_from_bytes, sweep_preview, zones_preview)

__all__ = ["config", "mvfile", "mvjson", "LIB_PATH", "COMPACT_DTYPE", "LAYOUT_AOS40", "LAYOUT_BOXES", "LAYOUT_CENTRES", "LAYOUT_COMPACT8", "LAYOUT_ZERO_COPY",
           "pack_records", "plan_preview", "MV_DTYPE", "SEGMENT_DTYPE", "MERGE_PARAMS_DTYPE",
           "MERGE_RESULT_DTYPE", "MtgpuError", "load_library", "FrameBatch", "MergeParams",
           "MotionScanner", "ScanParams", "ScanPipe", "concat_list", "filter_frames", "frame_skip", "make_chunks",
           "results_from_bytes", "sweep_preview", "activity_preview", "zones_preview", "blobs_preview", "gmc_preview", "GMC_INFO_DTYPE",
           "gmc_blobs_preview", "persist_preview", "dir_preview", "lanes_preview"]
