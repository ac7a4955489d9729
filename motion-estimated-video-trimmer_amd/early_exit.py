"""The scan's early exit, as the launch plan reports it (include/mtgpu.h, mtgpu_plan::early_exit).

A flags-only scan of 40-byte records may stop reading a frame once a vote has proven its flag (csrc/scan_kernels.hip,
vote_and_prove).  Whether a context takes that exit is a field of its plan: 1 on a plan with one tile of 32-bit counters,
VECTORS_NEEDED >= 1 and CLUSTERS_NEEDED <= 2, unless MTGPU_EARLY_EXIT=0 was set when the context was created.  Launches
that are cut into slices and the centre-count entry points never take it, whatever the plan says.

plan() and preview() return what MotionScanner.plan and scanner.plan_preview return, plus the key `early_exit`.
(MotionScanner's own methods and the keys they return are a recorded surface: tests/golden/scanner_calls.json.)
"""
import ctypes as C

from ._abi import PlanC, check, load_library
from .scanner import MotionScanner, ScanParams, _fields


def _with_key(p: PlanC) -> dict:
    return dict(_fields(p), early_exit=int(p._pad))        # (_abi.PlanC: the field keeps its old name there)


def plan(scanner: MotionScanner) -> dict:
    """The launch plan of a context (mtgpu_get_plan) with `early_exit`."""
    p = PlanC()
    check(load_library().mtgpu_get_plan(scanner._ctx, C.byref(p)))
    return _with_key(p)


def preview(params: ScanParams, lds_bytes: int = 163840, cu_count: int = 256) -> dict:
    """The plan the library would pick (mtgpu_plan_preview) with `early_exit`.  Host arithmetic only: works without a GPU."""
    p = PlanC()
    check(load_library().mtgpu_plan_preview(C.byref(params.to_c()), int(lds_bytes), int(cu_count), C.byref(p)))
    return _with_key(p)
