"""Host-side mirror of the reference's scanner interface for the MV-scan path.

`MotionScanner` keeps the public shape of the reference class
(include/motion_trim/motion_scanner.hpp:113-152: construct, initialize(), scan_range())
but its `check_frame` half runs on the MI355X through the C ABI of include/mtgpu.h.
FFmpeg decode stays on the host and is NOT part of this package: frames arrive as
already-extracted AVMotionVector arrays (`FrameBatch`).

Host logic restated here (cheap, sequential, per call):
  - cfg/grid derivation   -> done inside libmtgpu (mtgpu_params_from_config)
  - scan_range's frame filter (src/motion_scanner.cpp:307-314, 357-371)
  - chunk creation (src/pipeline.cpp:141-142, 163-167)
Everything per-MV or per-timestamp runs in HIP kernels.
"""
import ctypes as C
import weakref
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi, config
from ._abi import (BLOB_BOX_DTYPE, HEADING_DTYPE, OBJECT_DTYPE, BlobsPlanC, COMPACT_DTYPE, DIR_ALL, DirPlanC, LanesPlanC, LAYOUT_AOS40, LAYOUT_BOXES, LAYOUT_CENTRES, LAYOUT_COMPACT8, LAYOUT_ZERO_COPY, MERGE_PARAMS_DTYPE, MERGE_RESULT_DTYPE,
                   GMC_DEFAULT_MAX_SHIFT, GMC_DEFAULT_MIN_SHARE_Q8, GMC_INFO_DTYPE, GmcBlobsPlanC, GmcPlanC,
                   MV_DTYPE, SEGMENT_DTYPE, ActivityPlanC, MergeParamsC, MergeResultC, PersistPlanC, PlanC, ScanParamsC, SweepPlanC, ZonesPlanC, check,
                   load_library)


@dataclass
class ScanParams:
    """mt_scan_params (include/mt_types.h) == MotionScanner::cfg + grid dims."""
    mv_threshold_sq: float
    block_shift: int
    clusters_needed: int
    vertical_margin: int
    vectors_needed: int
    grid_w: int
    grid_h: int

    @classmethod
    def from_config(cls, width: int, height: int, mv_threshold_sq=None, block_size=None,
                    block_shift=None, vectors_needed=None, clusters_needed=None,
                    vertical_mask=None) -> "ScanParams":
        """MotionScanner::initialize() lines 184-199; None -> the env/default getter."""
        lib = load_library()
        c = ScanParamsC()
        check(lib.mtgpu_params_from_config(
            C.byref(c), int(width), int(height),
            config.mv_threshold_sq() if mv_threshold_sq is None else float(mv_threshold_sq),
            config.block_size() if block_size is None else int(block_size),
            config.block_shift() if block_shift is None else int(block_shift),
            config.vectors_needed() if vectors_needed is None else int(vectors_needed),
            config.clusters_needed() if clusters_needed is None else int(clusters_needed),
            config.vertical_mask() if vertical_mask is None else float(vertical_mask)))
        return cls.from_c(c)

    @classmethod
    def from_c(cls, c: ScanParamsC) -> "ScanParams":
        return cls(c.mv_threshold_sq, c.block_shift, c.clusters_needed, c.vertical_margin,
                   c.vectors_needed, c.grid_w, c.grid_h)

    def to_c(self) -> ScanParamsC:
        c = ScanParamsC()
        c.mv_threshold_sq = self.mv_threshold_sq
        c.block_shift = self.block_shift
        c.clusters_needed = self.clusters_needed
        c.vertical_margin = self.vertical_margin
        c.vectors_needed = self.vectors_needed & 0xFF
        c.grid_w = self.grid_w
        c.grid_h = self.grid_h
        return c


@dataclass
class MergeParams:
    """mt_merge_params: MAX_GAP_SEC, PADDING_SEC, duration, MIN_SAVINGS_PCT."""
    duration: float
    max_gap_sec: float = None
    padding_sec: float = None
    min_savings_pct: float = None

    def __post_init__(self):
        if self.max_gap_sec is None:
            self.max_gap_sec = config.max_gap_sec()
        if self.padding_sec is None:
            self.padding_sec = config.padding_sec()
        if self.min_savings_pct is None:
            self.min_savings_pct = config.min_savings_pct()

    def to_c(self) -> MergeParamsC:
        return MergeParamsC(self.max_gap_sec, self.padding_sec, self.duration, self.min_savings_pct)

    def to_record(self) -> np.ndarray:
        return np.array([(self.max_gap_sec, self.padding_sec, self.duration, self.min_savings_pct)],
                        dtype=MERGE_PARAMS_DTYPE)


@dataclass
class FrameBatch:
    """CSR batch of extracted MV side data: frame f owns mv[frame_off[f]:frame_off[f+1]]."""
    mv: np.ndarray                      # MV_DTYPE, packed
    frame_off: np.ndarray               # uint64 [F+1]
    pts: Optional[np.ndarray] = None    # float64 [F], seconds
    has_sd: Optional[np.ndarray] = None  # uint8 [F]; None: side data iff >= 1 record

    @property
    def n_frames(self) -> int:
        return len(self.frame_off) - 1

    @classmethod
    def from_frames(cls, frames: Sequence[Optional[np.ndarray]], pts=None) -> "FrameBatch":
        """frames[i] is an MV_DTYPE array, or None when the frame had no MV side data."""
        counts = [0 if f is None else len(f) for f in frames]
        off = np.zeros(len(frames) + 1, dtype=np.uint64)
        np.cumsum(counts, out=off[1:])
        mv = np.zeros(int(off[-1]), dtype=MV_DTYPE)
        for i, f in enumerate(frames):
            if f is not None and len(f):
                mv[int(off[i]):int(off[i + 1])] = f
        has_sd = np.array([0 if f is None else 1 for f in frames], dtype=np.uint8)
        return cls(mv, off, None if pts is None else np.asarray(pts, dtype=np.float64), has_sd)


def frame_skip(video_fps: float, target_fps: float) -> int:
    """src/motion_scanner.cpp:311-313."""
    return int(video_fps / target_fps) if (target_fps > 0 and target_fps < video_fps) else 1


def filter_frames(frame_pts: Sequence[int], time_base: float, start: float, end: float,
                  skip: int) -> Tuple[List[int], List[float]]:
    """Which decoded frames of one scan_range(start, end) call reach check_frame
    (src/motion_scanner.cpp:314, 357-371).  Returns (indices, pts_seconds)."""
    idx, pts_out = [], []
    count = 0
    for i, p in enumerate(frame_pts):
        count += 1
        if count % skip != 0:
            continue
        pts = float(p) * time_base
        if pts < start:
            continue
        if pts >= end:
            break
        idx.append(i)
        pts_out.append(pts)
    return idx, pts_out


def make_chunks(duration: float, chunk_sec: Optional[float] = None) -> List[Tuple[float, float, int]]:
    """src/pipeline.cpp:163-167: ScanTask{start, end, id}."""
    chunk_sec = config.chunk_duration_sec() if chunk_sec is None else chunk_sec
    out, t, cid = [], 0.0, 0
    while t < duration:
        out.append((t, min(t + chunk_sec, duration), cid))
        cid += 1
        t += chunk_sec
    return out


def concat_list(segments, abs_input_path: str) -> str:
    """The text the reference's cut executor feeds to `ffmpeg -f concat` for a job's segments
    (src/ffmpeg_executor.cpp:38-50): per segment with end > start three lines — file '<path>', inpoint and
    outpoint with two decimals (fmt's {:.2f} == "%.2f").  Convenience for diffing against the reference's cut
    list; the hand-off itself is the segment doubles."""
    out = []
    for s in segments:
        a, b = float(s[0]), float(s[1])
        if b <= a:
            continue
        out.append("file '%s'\ninpoint %.2f\noutpoint %.2f\n" % (abs_input_path, a, b))
    return "".join(out)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dptr(t):
    return None if t is None else t.data_ptr()


def _stream_handle(dev, stream):
    """The hipStream_t of a device call: the caller's handle, or torch's current stream on `dev`."""
    if stream is not None:
        return stream
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def _fields(p) -> dict:
    """A ctypes struct as a dict of its fields (padding, named _..., left out)."""
    return {n: getattr(p, n) for n, *_ in p._fields_ if not n.startswith("_")}


def _preview(symbol, plan_c, params, *ints) -> dict:
    """One mtgpu_*_preview call: (params, ints..., plan out) -> the plan as a dict; params None: the call takes none."""
    p = plan_c()
    head = () if params is None else (C.byref(params.to_c()),)
    check(getattr(load_library(), symbol)(*head, *(int(i) for i in ints), C.byref(p)))
    return _fields(p)


def plan_preview(params: "ScanParams", lds_bytes: int = 163840, cu_count: int = 256) -> dict:
    """The launch plan the library would pick for `params` on a device with that much LDS per
    workgroup and that many CUs (defaults: MI355X).  Host arithmetic only: works without a GPU."""
    return _preview("mtgpu_plan_preview", PlanC, params, lds_bytes, cu_count)


def sweep_preview(params: "ScanParams", n_thresholds: int, n_vectors: int, lds_bytes: int = 163840) -> dict:
    """How a sweep of n_thresholds x n_vectors settings would run on the grid of `params` with that much LDS per
    workgroup (mtgpu_scan_sweep_preview): tiles per launch, launches (= reads of the records), LDS bytes.  Host
    arithmetic only: works without a GPU.  MtgpuError(MT_ERR_UNSUPPORTED) for a grid the sweep has no form for."""
    return _preview("mtgpu_scan_sweep_preview", SweepPlanC, params, lds_bytes, n_thresholds, n_vectors)


def activity_preview(params: "ScanParams", lds_bytes: int = 163840) -> dict:
    """The form the activity map takes on the grid of `params` with that much LDS per workgroup
    (mtgpu_activity_preview): LDS bytes, width of the LDS accumulators (32, 16, or 0 = every frame flushes), the most
    frames a workgroup accumulates before it flushes, lanes.  Host arithmetic only: works without a GPU.
    MtgpuError(MT_ERR_UNSUPPORTED) for a grid the map has no form for."""
    return _preview("mtgpu_activity_preview", ActivityPlanC, params, lds_bytes)


def zones_preview(params: "ScanParams", lds_bytes: int = 163840) -> dict:
    """How the masked scan runs on the grid of `params` with that much LDS per workgroup (mtgpu_zones_preview): LDS
    bytes, lanes, and the sizes of a keep mask: uint64 words per grid row and per stream.  Host arithmetic only: works
    without a GPU.  MtgpuError(MT_ERR_UNSUPPORTED) for a grid the masked scan has no form for."""
    return _preview("mtgpu_zones_preview", ZonesPlanC, params, lds_bytes)


def blobs_preview(params: "ScanParams", lds_bytes: int = 163840) -> dict:
    """How the blob scan runs on the grid of `params` with that much LDS per workgroup (mtgpu_blobs_preview): LDS
    bytes, lanes, and the sizes of a keep mask: uint64 words per grid row and per stream.  Host arithmetic only: works
    without a GPU.  MtgpuError(MT_ERR_UNSUPPORTED) for a grid the blob scan has no form for."""
    return _preview("mtgpu_blobs_preview", BlobsPlanC, params, lds_bytes)


def gmc_preview(params: "ScanParams", lds_bytes: int = 163840) -> dict:
    """How the compensated scan runs on the grid of `params` with that much LDS per workgroup (mtgpu_gmc_preview): LDS
    bytes, lanes, histogram bins per axis, bytes of one GMC_INFO_DTYPE element.  Host arithmetic only: works without a
    GPU.  MtgpuError(MT_ERR_UNSUPPORTED) for a grid the compensated scan has no form for."""
    return _preview("mtgpu_gmc_preview", GmcPlanC, params, lds_bytes)


def gmc_blobs_preview(params: "ScanParams", lds_bytes: int = 163840) -> dict:
    """How the compensated blob scan runs on the grid of `params` with that much LDS per workgroup
    (mtgpu_gmc_blobs_preview): LDS bytes, lanes, the sizes of a keep mask (uint64 words per grid row and per stream),
    histogram bins per axis, bytes of one GMC_INFO_DTYPE element.  Host arithmetic only: works without a GPU.
    MtgpuError(MT_ERR_UNSUPPORTED) for a grid the scan has no form for."""
    return _preview("mtgpu_gmc_blobs_preview", GmcBlobsPlanC, params, lds_bytes)


def dir_preview(params: "ScanParams", lds_bytes: int = 163840) -> dict:
    """How the direction scan runs on the grid of `params` with that much LDS per workgroup (mtgpu_dir_preview): LDS
    bytes, lanes, sectors of a rose (8), bytes of one rose (32).  Host arithmetic only: works without a GPU.
    MtgpuError(MT_ERR_UNSUPPORTED) for a grid the direction scan has no form for."""
    return _preview("mtgpu_dir_preview", DirPlanC, params, lds_bytes)


def lanes_preview(params: "ScanParams", lds_bytes: int = 163840) -> dict:
    """How the plane scan runs on the grid of `params` with that much LDS per workgroup (mtgpu_lanes_preview): LDS bytes,
    lanes, staged (1: the plane's analysed rows are held in LDS, 0: read from memory), bytes of one plane (gw * gh).
    Host arithmetic only: works without a GPU.  MtgpuError(MT_ERR_UNSUPPORTED) for a grid the plane scan has no form
    for."""
    return _preview("mtgpu_lanes_preview", LanesPlanC, params, lds_bytes)


def persist_preview() -> dict:
    """How the persistence pass runs (mtgpu_persist_preview): lanes per workgroup and the frames a workgroup takes per
    step.  Host only: works without a GPU."""
    return _preview("mtgpu_persist_preview", PersistPlanC, None)


ACTIVITY_OUTPUTS = ("active", "centre", "frames")
PERSIST_OUTPUTS = ("flags", "run", "pos")
BLOB_OUTPUTS = ("flags", "centres", "blobs", "largest", "box")
GMC_BLOB_OUTPUTS = BLOB_OUTPUTS + ("info",)
DIR_OUTPUTS = ("flags", "centres", "rose")


# Every named output of the scans: name -> (torch element type, trailing shape on the device, numpy dtype on the host,
# the byte a host array is filled with).  A structured numpy dtype takes the trailing shape into its element; a trailing
# shape of None is the caller's (the grid of an activity map, the k entries of an object list: objects.py).  The *_OUTPUTS tuples above are the public lists of names
# and the order of the library's arguments.
_COUNT = ("int32", (), np.uint32, 0)
_OUTPUTS = {
    "flags": ("uint8", (), np.uint8, 0),
    "centres": _COUNT, "blobs": _COUNT, "largest": _COUNT, "objects": _COUNT, "run": _COUNT, "pos": _COUNT, "frames": _COUNT,
    "rose": ("int32", (8,), np.uint32, 0),
    "box": ("int16", (4,), BLOB_BOX_DTYPE, 0xFF),
    "info": ("int32", (5,), GMC_INFO_DTYPE, 0),
    "list": ("int32", None, OBJECT_DTYPE, 0),
    # object tracks (tracks.py): per list entry, the trailing shape is the caller's k
    "pred": ("uint8", None, np.uint8, 0xFF), "age": ("int32", None, np.uint32, 0), "id": ("int32", None, np.uint32, 0xFF),
    "len": ("int32", None, np.uint32, 0), "track": _COUNT,
    # object headings (headings.py): per list entry; the empty entry's heading word is the library's to write
    "motion": ("int32", None, HEADING_DTYPE, 0), "allowed": _COUNT,
    "active": ("int32", None, np.uint32, 0), "centre": ("int32", None, np.uint32, 0),
}


def _wanted(want, names) -> tuple:
    want = tuple(want)
    for w in want:
        if w not in names:
            raise ValueError(f"want: {w!r} is not one of {names}")
    return want


def _host_outputs(names, n, want=None, grid=()) -> dict:
    """name -> the numpy array of `n` elements the library fills (None for a name left out of `want`)."""
    out = {}
    for name in names:
        _, trail, dtype, fill = _OUTPUTS[name]
        out[name] = None
        if want is None or name in want:
            out[name] = np.empty((n,) + (grid if trail is None else () if np.dtype(dtype).names else trail), dtype=dtype)
            out[name].view(np.uint8)[...] = fill
    return out


def _device_outputs(names, want, out, n, dev, grid=()) -> dict:
    """name -> the torch tensor of `n` elements the library fills: the caller's out[name], checked, or a new one; None
    for a name left out of `want`."""
    import torch
    want = _wanted(want, names)
    res = {}
    for name in names:
        if name not in want:
            res[name] = None
            continue
        elem, trail = _OUTPUTS[name][:2]
        dtype, shape = getattr(torch, elem), (n,) + (grid if trail is None else trail)
        t = (out or {}).get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        assert t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape, name
        res[name] = t
    return res


def _optional(t, n, spec, dev, none_allocates=True, checked=True):
    """One optional output of a tuple-returning device scan: None = allocated, False = not computed (None comes back),
    or a tensor of at least `n` elements to fill.  spec: a name of _OUTPUTS, or (element type, trailing shape).
    none_allocates=False: None is "not computed" too and True allocates.  checked=False: a tensor passes unlooked at."""
    import torch
    elem, trail = (_OUTPUTS[spec] if isinstance(spec, str) else spec)[:2]
    dtype, shape = getattr(torch, elem), (n,) + trail
    if t is False or (t is None and not none_allocates):
        return None
    if t is None or (t is True and not none_allocates):
        return torch.empty(shape, dtype=dtype, device=dev)
    assert not checked or (t.dtype == dtype and t.is_contiguous() and t.numel() >= int(np.prod(shape)))
    return t


def _host_batch(batch, stream_off=None, null_if_empty=False):
    """The arrays of a host batch as the library takes them: ((mv or NULL, frame_off, has_sd or NULL, n frames),
    (stream_off or NULL, n streams), the contiguous arrays themselves).  The pointers keep their arrays alive."""
    mv = np.ascontiguousarray(batch.mv, dtype=MV_DTYPE)
    off = np.ascontiguousarray(batch.frame_off, dtype=np.uint64)
    sd = None if batch.has_sd is None else np.ascontiguousarray(batch.has_sd, dtype=np.uint8)
    soff, ns = None, 0
    if stream_off is not None:
        soff = np.ascontiguousarray(stream_off, dtype=np.uint64)
        ns = max(len(soff) - 1, 0)
    soff_ptr = None if null_if_empty and not len(soff) else _ptr(soff)
    return (_ptr(mv) if len(mv) else None, _ptr(off), _ptr(sd), max(len(off) - 1, 0)), (soff_ptr, ns), (mv, off, sd, soff)


def _sweep_settings(thresholds, vectors):
    """The two HOST arrays of a sweep call as ctypes arrays (at least one element each, so that a count of 0 still
    reaches the library's own check)."""
    th = [float(t) for t in thresholds]
    ve = [int(v) for v in vectors]
    for v in ve:
        if not -2 ** 31 <= v < 2 ** 31:
            raise ValueError(f"vector level {v} does not fit int32")
    return (C.c_double * max(len(th), 1))(*th), len(th), (C.c_int32 * max(len(ve), 1))(*ve), len(ve)


def pack_records(mv: np.ndarray) -> np.ndarray:
    """40-byte AVMotionVector records -> the 8-byte compact records the host dispatcher stages
    (bytes 6..13: src_x, src_y, dst_x, dst_y) through the library's own packer (mtgpu_pack_records)."""
    mv = np.ascontiguousarray(mv, dtype=MV_DTYPE)
    out = np.zeros(len(mv), dtype=COMPACT_DTYPE)
    if len(mv):
        check(load_library().mtgpu_pack_records(_ptr(mv), len(mv), _ptr(out)))
    return out


class MotionScanner:
    """GPU scanner context (one per device; callable from many threads)."""

    def __init__(self, params: ScanParams, device: int = 0):
        self.params = params
        self.device = device
        self._lib = load_library()
        self._ctx = C.c_void_p()
        self._pipes = weakref.WeakSet()    # open ScanPipes of this context: closed before it (include/mtgpu.h)
        c = params.to_c()
        check(self._lib.mtgpu_create(C.byref(c), int(device), C.byref(self._ctx)))

    # -- reference-shaped constructor: MotionScanner(...).initialize()
    @classmethod
    def initialize(cls, width: int, height: int, device: int = 0, **cfg) -> "MotionScanner":
        return cls(ScanParams.from_config(width, height, **cfg), device)

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            # pipes are destroyed before their context (include/mtgpu.h): a pipe that outlives it — e.g. one kept alive
            # by the traceback of a failed test — would otherwise drain streams the context has already destroyed
            for pipe in list(getattr(self, "_pipes", ())):
                pipe.close()
            self._lib.mtgpu_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def plan(self) -> dict:
        p = PlanC()
        check(self._lib.mtgpu_get_plan(self._ctx, C.byref(p)))
        return _fields(p)

    def set_slices(self, slices: int):
        """Workgroups per frame: 0 = automatic (default), or 1 / 2 / 4 / 8.  Never changes results."""
        check(self._lib.mtgpu_set_slices(self._ctx, int(slices)))

    def profile(self, on: bool = True):
        """Launch timing on / off (mtgpu_profile_enable): three events per scan launch, read with profile_read()."""
        check(self._lib.mtgpu_profile_enable(self._ctx, 1 if on else 0))

    def profile_read(self) -> dict:
        """Waits for the profiled launches so far; {"plan_ms", "scan_ms"}: MEAN per launch over "launches" launches."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint32()
        check(self._lib.mtgpu_profile_read(self._ctx, C.byref(a), C.byref(b), C.byref(n)))
        k = max(n.value, 1)
        return {"plan_ms": a.value / k, "scan_ms": b.value / k, "launches": n.value}

    def stats(self) -> dict:
        """What the context holds on the device (mtgpu_get_stats): staging of the host-pointer entry points,
        the scratch pool's reserved bytes now and at its high-water mark."""
        from ._abi import CtxStatsC
        st = CtxStatsC()
        check(self._lib.mtgpu_get_stats(self._ctx, C.byref(st)))
        return _fields(st)

    def trim(self):
        """Hand the scratch pool's unused blocks back to the device (mtgpu_trim)."""
        check(self._lib.mtgpu_trim(self._ctx))

    def _device_batch(self, d_rec, d_off, d_sd, compact, stream):
        """The head of every device scan's argument list — (context, records or NULL, bytes per record, n records,
        frame offsets, has_sd or NULL, n frames) — and the stream handle, from a device-resident batch."""
        import torch
        assert d_rec.is_contiguous() and d_off.is_contiguous() and d_off.dtype == torch.int64
        rec_bytes = 8 if compact else 40
        n_records = (d_rec.numel() * d_rec.element_size()) // rec_bytes
        return (self._ctx, d_rec.data_ptr() if n_records else None, rec_bytes, n_records, d_off.data_ptr(), _dptr(d_sd),
                max(d_off.numel() - 1, 0)), _stream_handle(d_off.device, stream)

    def _hold(self, ws, dev, stream):
        """Keeps a workspace of this call alive: it must outlive the kernel that was just queued, so it is held until an
        event recorded behind the launch on ITS stream has passed (torch's caching allocator knows nothing of a raw
        hipStream_t handed in by the caller, and several launches may be queued back to back)."""
        import torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev) if stream is None else torch.cuda.ExternalStream(stream, device=dev))
        self._held = [(e, w) for e, w in getattr(self, "_held", []) if not e.query()]
        self._held.append((ev, ws))

    # ---------------------------------------------------------------- scan
    def check_frames(self, batch: FrameBatch) -> np.ndarray:
        """check_frame() for every frame of a host batch -> uint8 flags [F]."""
        (mv, off, sd, n), _, _ = _host_batch(batch)
        flags = _host_outputs(("flags",), n)["flags"]
        if n <= 0:
            return flags
        check(self._lib.mtgpu_scan_frames(self._ctx, mv, off, sd, n, _ptr(flags)))
        return flags

    def check_frames_device(self, mv, frame_off, has_sd=None, flags=None, stream=None):
        """Device-resident batch (torch CUDA tensors).  mv: uint8 [n_records*40] (or any
        dtype viewing the packed records), frame_off: int64 [F+1].  Asynchronous on
        `stream` (default: torch's current stream).  Returns the uint8 flags tensor."""
        # (this form and the compact one below run inside bench.py's timed loops: they keep their direct bodies, the
        # shared _device_batch costs them about a microsecond per call — docs/rounds/r29_python_fold.md)
        import torch
        n_frames = frame_off.numel() - 1
        if flags is None:
            flags = torch.empty(max(n_frames, 0), dtype=torch.uint8, device=frame_off.device)
        if n_frames <= 0:
            return flags
        assert mv.is_contiguous() and frame_off.is_contiguous() and flags.is_contiguous()
        assert frame_off.dtype == torch.int64 and flags.dtype == torch.uint8
        n_records = (mv.numel() * mv.element_size()) // 40
        st = torch.cuda.current_stream(frame_off.device).cuda_stream if stream is None else stream
        check(self._lib.mtgpu_scan_frames_device(
            self._ctx, mv.data_ptr() if n_records else None, n_records, frame_off.data_ptr(),
            None if has_sd is None else has_sd.data_ptr(), n_frames, flags.data_ptr(), st))
        return flags

    def check_frames_device_compact(self, rec8, frame_off, has_sd=None, flags=None, stream=None):
        """Device-resident batch of COMPACT records (8 bytes each, see pack_records): rec8 is a
        torch CUDA tensor viewing n_records * 8 bytes.  Otherwise like check_frames_device."""
        import torch
        n_frames = frame_off.numel() - 1
        if flags is None:
            flags = torch.empty(max(n_frames, 0), dtype=torch.uint8, device=frame_off.device)
        if n_frames <= 0:
            return flags
        assert rec8.is_contiguous() and frame_off.is_contiguous() and flags.is_contiguous()
        assert frame_off.dtype == torch.int64 and flags.dtype == torch.uint8
        n_records = (rec8.numel() * rec8.element_size()) // 8
        st = torch.cuda.current_stream(frame_off.device).cuda_stream if stream is None else stream
        check(self._lib.mtgpu_scan_frames_device_compact(
            self._ctx, rec8.data_ptr() if n_records else None, n_records, frame_off.data_ptr(),
            None if has_sd is None else has_sd.data_ptr(), n_frames, flags.data_ptr(), st))
        return flags

    # ------------------------------------------------------- centre counts
    def count_centres(self, batch: FrameBatch) -> Tuple[np.ndarray, np.ndarray]:
        """check_frame() for every frame of a host batch, with the frame's centre count: the `clusters` counter of
        src/motion_scanner.cpp:272-294 without its early return (0 for a frame without side data).
        Returns (flags uint8 [F], centres uint32 [F]); flags == centres >= max(1, clusters_needed)."""
        head, _, _ = _host_batch(batch)
        out = _host_outputs(("flags", "centres"), head[3])
        if head[3] > 0:
            check(self._lib.mtgpu_scan_frames_centres(self._ctx, *head, _ptr(out["flags"]), _ptr(out["centres"])))
        return out["flags"], out["centres"]

    def count_centres_device(self, records, frame_off, has_sd=None, compact=False, flags=None, centres=None,
                             stream=None):
        """Device-resident batch (torch CUDA tensors) -> (flags uint8 [F], centres int32 [F], the bits of the
        library's uint32 counts).  records: the packed 40-byte records, or the 8-byte compact ones with
        compact=True.  flags=False: only the counts are computed (returns (None, centres)).  Asynchronous on
        `stream` (default: torch's current stream)."""
        import torch
        n_frames = frame_off.numel() - 1
        dev, n = frame_off.device, max(n_frames, 0)
        flags = _optional(flags, n, "flags", dev, checked=n_frames > 0)
        if centres is None:
            centres = torch.empty(n, dtype=torch.int32, device=dev)
        if n_frames <= 0:
            return flags, centres
        assert centres.is_contiguous() and centres.dtype == torch.int32 and centres.numel() >= n_frames
        head, st = self._device_batch(records, frame_off, has_sd, compact, stream)
        check(self._lib.mtgpu_scan_centres_device(*head, _dptr(flags), centres.data_ptr(), st))
        return flags, centres

    def flags_from_centres(self, centres, clusters_needed: int, flags=None, stream=None):
        """flags[f] = centres[f] >= max(1, clusters_needed) (src/motion_scanner.cpp:288) on the device: the flags a
        scanner created with that CLUSTERS_NEEDED returns.  centres: int32 CUDA tensor from count_centres_device."""
        import torch
        assert centres.dtype == torch.int32 and centres.is_contiguous()
        n = centres.numel()
        if flags is None:
            flags = torch.empty(n, dtype=torch.uint8, device=centres.device)
        st = _stream_handle(centres.device, stream)
        if n:
            check(self._lib.mtgpu_flags_from_centres_device(self._ctx, centres.data_ptr(), n, int(clusters_needed),
                                                            flags.data_ptr(), st))
        return flags

    def sweep_streams_device(self, centres, pts, stream_off, merge_params, levels, job_semantics=False,
                             seg_cap=64, stream=None):
        """merge_streams_device for several CLUSTERS_NEEDED values from ONE scan's centre counts, in one launch:
        level l is bit for bit what merge_streams_device returns on flags_from_centres(centres, levels[l]).
        centres int32 [F], pts float64 [F], stream_off int64 [S+1], merge_params as for merge_streams_device,
        levels: 1..16 ints.  Returns (segments float64 [L, S, seg_cap, 2], results uint8 [L, S, 40])."""
        import torch
        dev = pts.device
        levels = [int(v) for v in levels]
        n_levels = len(levels)
        n_streams = stream_off.numel() - 1
        n_frames = pts.numel()
        assert centres.dtype == torch.int32 and centres.is_contiguous() and centres.numel() >= n_frames
        ws = torch.empty(2 * max(n_frames, 1) * max(n_levels, 1), dtype=torch.float64, device=dev)
        seg = torch.zeros((n_levels, max(n_streams, 0), seg_cap, 2), dtype=torch.float64, device=dev)
        res = torch.zeros((n_levels, max(n_streams, 0), MERGE_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        c_levels = (C.c_int32 * max(n_levels, 1))(*levels)
        check(self._lib.mtgpu_sweep_streams_device(
            self._ctx, centres.data_ptr(), pts.data_ptr(), stream_off.data_ptr(), max(n_streams, 0), n_frames,
            merge_params.data_ptr(), c_levels, n_levels, 1 if job_semantics else 0, ws.data_ptr(), seg.data_ptr(),
            seg_cap, res.data_ptr(), _stream_handle(dev, stream)))
        self._hold(ws, dev, stream)
        return seg, res

    # ------------------------------------------------------- setting sweep
    def sweep_centres(self, batch: FrameBatch, thresholds, vectors) -> np.ndarray:
        """The centre counts of every frame of a host batch for every (MV_THRESHOLD_SQ, VECTORS_NEEDED) pair, from
        one read of the records per pass (mtgpu_scan_frames_sweep): uint32 [T, V, F], in the caller's order.
        out[t, v] is what count_centres returns through a scanner created with thresholds[t] and vectors[v];
        the scanner's own threshold, vectors and clusters play no part."""
        c_th, n_th, c_ve, n_ve = _sweep_settings(thresholds, vectors)
        head, _, _ = _host_batch(batch)
        out = np.zeros((n_th, n_ve, head[3]), dtype=np.uint32)
        check(self._lib.mtgpu_scan_frames_sweep(self._ctx, *head, c_th, n_th, c_ve, n_ve, _ptr(out) if out.size else None))
        return out

    def sweep_centres_device(self, records, frame_off, has_sd, thresholds, vectors, compact=False, out=None, stream=None):
        """Device-resident batch (torch CUDA tensors) -> int32 [T, V, F] CUDA tensor (the bits of the library's uint32
        counts): out[t, v] is the centres tensor of count_centres_device through a scanner created with
        thresholds[t] and vectors[v], ready for flags_from_centres / sweep_streams_device.  records: the packed
        40-byte records, or the 8-byte compact ones with compact=True.  Asynchronous on `stream` (default: torch's
        current stream)."""
        import torch
        c_th, n_th, c_ve, n_ve = _sweep_settings(thresholds, vectors)
        n_frames = max(frame_off.numel() - 1, 0)
        if out is None:
            out = torch.empty((n_th, n_ve, n_frames), dtype=torch.int32, device=frame_off.device)
        assert out.is_contiguous() and out.dtype == torch.int32 and out.numel() >= n_th * n_ve * n_frames
        head, st = self._device_batch(records, frame_off, has_sd, compact, stream)
        check(self._lib.mtgpu_scan_sweep_device(*head, c_th, n_th, c_ve, n_ve, out.data_ptr(), st))
        return out

    # ------------------------------------------------------- activity maps
    def activity_map(self, batch: FrameBatch, stream_off, min_centres: int = 0, want=ACTIVITY_OUTPUTS):
        """Per-stream activity maps of a host batch (mtgpu_activity_map): (active uint32 [S, gh, gw], centre uint32
        [S, gh, gw], frames uint32 [S]) — per grid cell, the contributing frames of stream s in which the cell was
        active / one of the centres src/motion_scanner.cpp:277-292 counts; frames[s]: the contributing frames.  A
        frame contributes iff it has side data and its centre count is >= min_centres.  stream_off: S + 1 frame
        offsets.  An output left out of `want` is not computed and comes back as None."""
        want = _wanted(want, ACTIVITY_OUTPUTS)
        head, (soff, ns), _ = _host_batch(batch, stream_off, null_if_empty=True)
        out = _host_outputs(ACTIVITY_OUTPUTS, ns, want, (self.params.grid_h, self.params.grid_w))
        check(self._lib.mtgpu_activity_map(self._ctx, *head, soff, ns, int(min_centres), *(_ptr(out[k]) for k in ACTIVITY_OUTPUTS)))
        return tuple(out[k] for k in ACTIVITY_OUTPUTS)

    def activity_map_device(self, d_rec, d_off, d_sd, d_stream_off, min_centres: int = 0, run_frames: int = 0,
                            want=ACTIVITY_OUTPUTS, compact=False, out=None, stream=None):
        """Device-resident batch (torch CUDA tensors) -> (active int32 [S, gh, gw], centre int32 [S, gh, gw], frames
        int32 [S]) CUDA tensors (the bits of the library's uint32 counts; None for an output not in `want`).  d_rec:
        the packed 40-byte records, or the 8-byte compact ones with compact=True; d_off int64 [F + 1]; d_sd uint8 [F]
        or None; d_stream_off int64 [S + 1].  run_frames: work-list entries per workgroup, 0 = the planner chooses;
        the maps do not depend on it.  out: a dict of preallocated tensors by name.  Asynchronous on `stream`
        (default: torch's current stream)."""
        import torch
        ns = max(d_stream_off.numel() - 1, 0)
        res = _device_outputs(ACTIVITY_OUTPUTS, want, out, ns, d_off.device, (self.params.grid_h, self.params.grid_w))
        assert d_stream_off.is_contiguous() and d_stream_off.dtype == torch.int64
        head, st = self._device_batch(d_rec, d_off, d_sd, compact, stream)
        check(self._lib.mtgpu_activity_map_device(*head, d_stream_off.data_ptr(), ns, int(min_centres), int(run_frames),
                                                  *(_dptr(res[k]) for k in ACTIVITY_OUTPUTS), st))
        return tuple(res[k] for k in ACTIVITY_OUTPUTS)

    # -------------------------------------------------------- ignore zones
    def _keep_words(self, keep, n_streams):
        """uint64 [S, gh, W] from a packed mask (zones.pack_keep), one per stream or one for all of them."""
        gh, W = self.params.grid_h, (self.params.grid_w + 63) // 64
        keep = np.ascontiguousarray(keep, dtype=np.uint64)
        if keep.shape == (gh, W):
            keep = np.ascontiguousarray(np.broadcast_to(keep, (n_streams, gh, W)))
        if keep.shape != (n_streams, gh, W):
            raise ValueError(f"keep has shape {keep.shape}, not {(n_streams, gh, W)} (or {(gh, W)} for every stream)")
        return keep

    def _device_keep(self, d_stream_off, d_keep) -> int:
        """The streams of a device keep mask, checked against its stream offsets; 0 without a mask."""
        if d_keep is None:
            return 0
        import torch
        ns = max(d_stream_off.numel() - 1, 0)
        assert d_stream_off.is_contiguous() and d_keep.is_contiguous()
        assert d_stream_off.dtype == torch.int64 and d_keep.dtype == torch.int64
        assert d_keep.numel() == ns * self.params.grid_h * ((self.params.grid_w + 63) // 64)
        return ns

    def scan_zones(self, batch: FrameBatch, stream_off, keep, want_all: bool = False):
        """The centre scan of a host batch under per-stream keep masks (mtgpu_scan_frames_zones): on the analysed rows
        a cell is active iff votes >= vectors_needed (src/motion_scanner.cpp:282) AND its keep bit is set.  stream_off:
        S + 1 frame offsets; keep: uint64 [S, gh, W] from zones.pack_keep (or [gh, W]: the same mask for every stream).
        Returns (flags uint8 [F], centres uint32 [F], centres_all): centres_all is the count without the mask from the
        same votes (uint32 [F]) with want_all=True, else None."""
        head, (soff, ns), _ = _host_batch(batch, stream_off, null_if_empty=True)
        keep = self._keep_words(keep, ns)
        out = _host_outputs(("flags", "centres"), head[3])
        call = _host_outputs(("centres",), head[3])["centres"] if want_all else None
        check(self._lib.mtgpu_scan_frames_zones(self._ctx, *head, soff, ns, _ptr(keep) if keep.size else None,
                                                _ptr(out["flags"]), _ptr(out["centres"]), _ptr(call)))
        return out["flags"], out["centres"], call

    def scan_zones_device(self, d_rec, d_off, d_sd, d_stream_off, d_keep, compact=False, flags=None, centres=None,
                          centres_all=None, stream=None):
        """Device-resident batch (torch CUDA tensors) -> (flags uint8 [F], centres int32 [F], centres_all int32 [F]), the
        bits of the library's uint32 counts.  d_rec: the packed 40-byte records, or the 8-byte compact ones with
        compact=True; d_off int64 [F + 1]; d_sd uint8 [F] or None; d_stream_off int64 [S + 1]; d_keep int64 [S, gh, W]
        (the bits of zones.pack_keep's uint64 words).  flags / centres: None = allocated, False = not computed, or a
        tensor to fill; centres_all: None or False = not computed, True = allocated, or a tensor to fill.
        Asynchronous on `stream` (default: torch's current stream)."""
        import torch
        dev = d_off.device
        n_frames = max(d_off.numel() - 1, 0)
        ns = max(d_stream_off.numel() - 1, 0)
        flags = _optional(flags, n_frames, "flags", dev)
        centres = _optional(centres, n_frames, "centres", dev)
        centres_all = _optional(centres_all, n_frames, "centres", dev, none_allocates=False)
        assert d_stream_off.is_contiguous() and d_keep.is_contiguous()
        assert d_stream_off.dtype == torch.int64 and d_keep.dtype == torch.int64
        assert d_keep.numel() == ns * self.params.grid_h * ((self.params.grid_w + 63) // 64)
        head, st = self._device_batch(d_rec, d_off, d_sd, compact, stream)
        check(self._lib.mtgpu_scan_zones_device(*head, d_stream_off.data_ptr(), ns, d_keep.data_ptr(), _dptr(flags),
                                                _dptr(centres), _dptr(centres_all), st))
        return flags, centres, centres_all

    # -------------------------------------------------------- the direction filter
    def scan_dir(self, batch: FrameBatch, allow: int = DIR_ALL, stream_off=None, allows=None) -> dict:
        """The centre scan of a host batch in which a record votes only if the sector of dst - src is allowed
        (mtgpu_scan_frames_dir; the sectors: direction.SECTOR_NAMES, 0 = E, clockwise on the screen), and every frame's
        rose.  allow: a byte, bit k lets sector k vote (direction.allow_from_names), for every frame; or stream_off
        (S + 1 frame offsets) with allows (S bytes), one byte per stream.  Returns a dict of numpy arrays over the
        frames: flags uint8, centres uint32, rose uint32 [F, 8]: the counting records per sector, whatever is allowed."""
        if (stream_off is None) != (allows is None):
            raise ValueError("stream_off and allows go together: give both or neither")
        head, (soff, ns), _ = _host_batch(batch, stream_off)
        if allows is not None:
            given = np.asarray(allows)
            if given.shape != (ns,) or (ns and (int(given.min()) < 0 or int(given.max()) > 255)):
                raise ValueError(f"allows: {ns} bytes in 0 .. 255 wanted, one per stream")
            allows = np.ascontiguousarray(np.concatenate([given.astype(np.uint8), np.zeros(1, dtype=np.uint8)]))   # never empty
        out = _host_outputs(DIR_OUTPUTS, head[3])
        check(self._lib.mtgpu_scan_frames_dir(self._ctx, *head, soff, ns, _ptr(allows), int(allow),
                                              *(_ptr(out[k]) for k in DIR_OUTPUTS)))
        return out

    def scan_dir_device(self, d_rec, d_off, d_sd, allow: int = DIR_ALL, d_stream_off=None, d_allow=None, compact=False,
                        want=DIR_OUTPUTS, out=None, stream=None) -> dict:
        """Device-resident batch (torch CUDA tensors) -> a dict of CUDA tensors over the frames: flags uint8, centres int32
        and rose int32 [F, 8] (the bits of the library's uint32 counts); None for an output not in `want`.  d_rec: the
        packed 40-byte records, or the 8-byte compact ones with compact=True; d_off int64 [F + 1]; d_sd uint8 [F] or
        None; allow: the byte for every frame, or d_stream_off int64 [S + 1] and d_allow uint8 [S], both or neither.
        out: a dict of preallocated tensors by name.  Asynchronous on `stream` (default: torch's current stream)."""
        import torch
        want = _wanted(want, DIR_OUTPUTS)
        if (d_stream_off is None) != (d_allow is None):
            raise ValueError("d_stream_off and d_allow go together: give both or neither")
        n_frames = max(d_off.numel() - 1, 0)
        res = _device_outputs(DIR_OUTPUTS, want, out, n_frames, d_off.device)
        if n_frames == 0:              # nothing to write (an empty tensor has no address to hand over)
            return res
        ns = 0
        if d_allow is not None:
            ns = max(d_stream_off.numel() - 1, 0)
            assert d_stream_off.is_contiguous() and d_stream_off.dtype == torch.int64
            assert d_allow.is_contiguous() and d_allow.dtype == torch.uint8 and d_allow.numel() >= max(ns, 1)
        head, st = self._device_batch(d_rec, d_off, d_sd, compact, stream)
        check(self._lib.mtgpu_scan_dir_device(*head, _dptr(d_stream_off), ns, _dptr(d_allow), int(allow),
                                              *(_dptr(res[k]) for k in DIR_OUTPUTS), st))
        return res

    # -------------------------------------------------------- direction planes and flow maps
    def _planes(self, planes, n_streams):
        """uint8 [S, gh, gw] (n_streams given) or [gh, gw] (n_streams None: one plane for every frame), contiguous."""
        gh, gw = self.params.grid_h, self.params.grid_w
        planes = np.ascontiguousarray(planes, dtype=np.uint8)
        want = (gh, gw) if n_streams is None else (n_streams, gh, gw)
        if planes.shape != want:
            raise ValueError(f"planes has shape {planes.shape}, not {want}")
        return planes

    def scan_lanes(self, batch: FrameBatch, planes, stream_off=None) -> dict:
        """The centre scan of a host batch in which a record votes only if the allow byte of its destination cell lets
        its sector vote (mtgpu_scan_frames_lanes), and every frame's rose.  planes: uint8 [gh, gw], one plane for every
        frame; or, with stream_off (S + 1 frame offsets), uint8 [S, gh, gw], one plane per stream (lanes.plane_from_rects,
        lanes.plane_from_flow).  Returns a dict of numpy arrays over the frames: flags uint8, centres uint32, rose uint32
        [F, 8]: the counting records per sector, whatever the planes say."""
        head, (soff, ns), _ = _host_batch(batch, stream_off)
        if stream_off is not None and ns == 0:
            raise ValueError("stream_off: at least one stream wanted (or None: one plane for every frame)")
        planes = self._planes(planes, None if stream_off is None else ns)
        out = _host_outputs(DIR_OUTPUTS, head[3])
        check(self._lib.mtgpu_scan_frames_lanes(self._ctx, *head, soff, ns, _ptr(planes), *(_ptr(out[k]) for k in DIR_OUTPUTS)))
        return out

    def scan_lanes_device(self, d_rec, d_off, d_sd, d_planes, d_stream_off=None, compact=False, want=DIR_OUTPUTS, out=None,
                          stream=None) -> dict:
        """Device-resident batch (torch CUDA tensors) -> a dict of CUDA tensors over the frames: flags uint8, centres int32
        and rose int32 [F, 8] (the bits of the library's uint32 counts); None for an output not in `want`.  d_rec: the
        packed 40-byte records, or the 8-byte compact ones with compact=True; d_off int64 [F + 1]; d_sd uint8 [F] or
        None; d_planes uint8: gh x gw bytes, or S x gh x gw with d_stream_off int64 [S + 1] — a contiguous tensor at any
        byte address.  out: a dict of preallocated tensors by name.  Asynchronous on `stream` (default: torch's current
        stream)."""
        import torch
        n_frames = max(d_off.numel() - 1, 0)
        res = _device_outputs(DIR_OUTPUTS, want, out, n_frames, d_off.device)
        if n_frames == 0:              # nothing to write (an empty tensor has no address to hand over)
            return res
        ns = 0
        if d_stream_off is not None:
            ns = max(d_stream_off.numel() - 1, 0)
            assert d_stream_off.is_contiguous() and d_stream_off.dtype == torch.int64 and ns > 0
        assert d_planes.is_contiguous() and d_planes.dtype == torch.uint8
        assert d_planes.numel() == max(ns, 1) * self.params.grid_h * self.params.grid_w
        head, st = self._device_batch(d_rec, d_off, d_sd, compact, stream)
        check(self._lib.mtgpu_scan_lanes_device(*head, _dptr(d_stream_off), ns, d_planes.data_ptr(),
                                                *(_dptr(res[k]) for k in DIR_OUTPUTS), st))
        return res

    def flow_map(self, batch: FrameBatch, stream_off) -> np.ndarray:
        """The flow map of a host batch (mtgpu_flow_map): uint32 [S, 8, gh, gw] — per stream, sector (0 = E, clockwise on
        the screen) and grid cell, the counting records with that sector and destination cell over the stream's frames
        with side data.  stream_off: S + 1 frame offsets.  Maps of successive batches add."""
        head, (soff, ns), _ = _host_batch(batch, stream_off)
        flow = np.zeros((ns, 8, self.params.grid_h, self.params.grid_w), dtype=np.uint32)
        if ns == 0:
            return flow
        check(self._lib.mtgpu_flow_map(self._ctx, *head, soff, ns, _ptr(flow)))
        return flow

    def flow_map_device(self, d_rec, d_off, d_sd, d_stream_off, compact=False, out=None, stream=None):
        """Device-resident batch (torch CUDA tensors) -> the flow map, an int32 [S, 8, gh, gw] CUDA tensor (the bits of the
        library's uint32 counts).  d_rec / d_off / d_sd as scan_lanes_device; d_stream_off int64 [S + 1].  out: a
        preallocated tensor; it is cleared, then counted into.  Asynchronous on `stream` (default: torch's current
        stream)."""
        import torch
        ns = max(d_stream_off.numel() - 1, 0)
        shape = (ns, 8, self.params.grid_h, self.params.grid_w)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=d_off.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == shape
        if ns == 0:
            return out
        assert d_stream_off.is_contiguous() and d_stream_off.dtype == torch.int64
        head, st = self._device_batch(d_rec, d_off, d_sd, compact, stream)
        check(self._lib.mtgpu_flow_map_device(*head, d_stream_off.data_ptr(), ns, out.data_ptr(), st))
        return out

    # -------------------------------------------------------- global-motion compensation
    def scan_gmc(self, batch: FrameBatch, max_shift: int = GMC_DEFAULT_MAX_SHIFT, min_share_q8: int = GMC_DEFAULT_MIN_SHARE_Q8):
        """The centre scan of a host batch on the residuals of each frame's dominant vector (mtgpu_scan_frames_gmc): the
        per-axis mode of the displacements of the records inside the analysed rows, within +-max_shift, is subtracted
        where at least min_share_q8 / 256 of those records agree on it; then src/motion_scanner.cpp:246-292 as
        count_centres runs it.  Returns (flags uint8 [F], centres uint32 [F], info GMC_INFO_DTYPE [F])."""
        head, _, _ = _host_batch(batch)
        out = _host_outputs(("flags", "centres", "info"), head[3])
        check(self._lib.mtgpu_scan_frames_gmc(self._ctx, *head, int(max_shift), int(min_share_q8), *(_ptr(a) for a in out.values())))
        return tuple(out.values())

    def scan_gmc_device(self, d_rec, d_off, d_sd, max_shift: int = GMC_DEFAULT_MAX_SHIFT,
                        min_share_q8: int = GMC_DEFAULT_MIN_SHARE_Q8, compact=False, flags=None, centres=None, info=None,
                        stream=None):
        """Device-resident batch (torch CUDA tensors) -> (flags uint8 [F], centres int32 [F], info int32 [F, 5]): the
        bits of the library's uint32 counts and of its mt_gmc_info elements (info.cpu().numpy().view(GMC_INFO_DTYPE)).
        d_rec: the packed 40-byte records, or the 8-byte compact ones with compact=True; d_off int64 [F + 1]; d_sd uint8
        [F] or None.  flags / centres / info: None = allocated, False = not computed, or a tensor to fill.
        Asynchronous on `stream` (default: torch's current stream)."""
        dev = d_off.device
        n_frames = max(d_off.numel() - 1, 0)
        flags = _optional(flags, n_frames, "flags", dev)
        centres = _optional(centres, n_frames, "centres", dev)
        info = _optional(info, n_frames, "info", dev)
        head, st = self._device_batch(d_rec, d_off, d_sd, compact, stream)
        check(self._lib.mtgpu_scan_gmc_device(*head, int(max_shift), int(min_share_q8), _dptr(flags), _dptr(centres),
                                              _dptr(info), st))
        return flags, centres, info

    # -------------------------------------------------------- motion blobs
    def scan_blobs(self, batch: FrameBatch, min_blob_cells: int = 1, stream_off=None, keep=None) -> dict:
        """The blob scan of a host batch (mtgpu_scan_frames_blobs): the 4-connected components of every frame's centre
        cells (the cells src/motion_scanner.cpp:277-292 counts).  Returns a dict of numpy arrays over the frames:
        flags uint8 (centres >= max(1, clusters_needed) and largest >= max(1, min_blob_cells)), centres uint32, blobs
        uint32 (components), largest uint32 (cells of the largest one), box BLOB_BOX_DTYPE (its inclusive cell bounds,
        all 0xFFFF without a blob).  stream_off / keep: per-stream keep masks as for scan_zones, both or neither."""
        if (stream_off is None) != (keep is None):
            raise ValueError("stream_off and keep go together: give both or neither")
        head, (soff, ns), _ = _host_batch(batch, stream_off)
        if keep is not None:
            keep = self._keep_words(keep, ns)
        out = _host_outputs(BLOB_OUTPUTS, head[3])
        check(self._lib.mtgpu_scan_frames_blobs(self._ctx, *head, soff, ns, _ptr(keep), int(min_blob_cells),
                                                *(_ptr(out[k]) for k in BLOB_OUTPUTS)))
        return out

    def scan_blobs_device(self, d_rec, d_off, d_sd, min_blob_cells: int = 1, d_stream_off=None, d_keep=None, compact=False,
                          want=BLOB_OUTPUTS, out=None, stream=None) -> dict:
        """Device-resident batch (torch CUDA tensors) -> a dict of CUDA tensors over the frames: flags uint8, centres /
        blobs / largest int32 (the bits of the library's uint32 counts), box int16 [F, 4] (the bits of x0, y0, x1, y1;
        all -1 without a blob); None for an output not in `want`.  d_rec: the packed 40-byte records, or the 8-byte
        compact ones with compact=True; d_off int64 [F + 1]; d_sd uint8 [F] or None; d_stream_off int64 [S + 1] and
        d_keep int64 [S, gh, W] (the bits of zones.pack_keep's words), both or neither.  `largest` is ready for
        sweep_streams_device: level L there is flags at min_blob_cells = L.  out: a dict of preallocated tensors by
        name.  Asynchronous on `stream` (default: torch's current stream)."""
        want = _wanted(want, BLOB_OUTPUTS)
        if (d_stream_off is None) != (d_keep is None):
            raise ValueError("d_stream_off and d_keep go together: give both or neither")
        n_frames = max(d_off.numel() - 1, 0)
        res = _device_outputs(BLOB_OUTPUTS, want, out, n_frames, d_off.device)
        if n_frames == 0:              # nothing to write (an empty tensor has no address to hand over)
            return res
        head, st = self._device_batch(d_rec, d_off, d_sd, compact, stream)
        ns = self._device_keep(d_stream_off, d_keep)
        check(self._lib.mtgpu_scan_blobs_device(*head, _dptr(d_stream_off), ns, _dptr(d_keep), int(min_blob_cells),
                                                *(_dptr(res[k]) for k in BLOB_OUTPUTS), st))
        return res

    # -------------------------------------------------------- motion blobs on compensated residuals
    def scan_gmc_blobs(self, batch: FrameBatch, max_shift: int = GMC_DEFAULT_MAX_SHIFT, min_share_q8: int = GMC_DEFAULT_MIN_SHARE_Q8,
                       min_blob_cells: int = 1, stream_off=None, keep=None) -> dict:
        """The compensated blob scan of a host batch (mtgpu_scan_frames_gmc_blobs): each frame's dominant vector is
        estimated as scan_gmc does — under keep masks, from the records in kept cells only — and subtracted; the residual
        vote's centre cells are labelled as scan_blobs does.  Returns a dict of numpy arrays over the frames: the five
        outputs of scan_blobs plus info (GMC_INFO_DTYPE: the applied vector, the modes, the counted records and the
        modes' counts).  stream_off / keep: per-stream keep masks as for scan_zones, both or neither."""
        if (stream_off is None) != (keep is None):
            raise ValueError("stream_off and keep go together: give both or neither")
        head, (soff, ns), _ = _host_batch(batch, stream_off)
        if keep is not None:
            keep = self._keep_words(keep, ns)
        out = _host_outputs(GMC_BLOB_OUTPUTS, head[3])
        check(self._lib.mtgpu_scan_frames_gmc_blobs(self._ctx, *head, soff, ns, _ptr(keep), int(max_shift), int(min_share_q8),
                                                    int(min_blob_cells), *(_ptr(out[k]) for k in GMC_BLOB_OUTPUTS)))
        return out

    def scan_gmc_blobs_device(self, d_rec, d_off, d_sd, max_shift: int = GMC_DEFAULT_MAX_SHIFT,
                              min_share_q8: int = GMC_DEFAULT_MIN_SHARE_Q8, min_blob_cells: int = 1, d_stream_off=None, d_keep=None,
                              compact=False, want=GMC_BLOB_OUTPUTS, out=None, stream=None) -> dict:
        """Device-resident batch (torch CUDA tensors) -> a dict of CUDA tensors over the frames: flags uint8, centres /
        blobs / largest int32, box int16 [F, 4] as scan_blobs_device returns them, info int32 [F, 5] (the bits of the
        library's mt_gmc_info elements: info.cpu().numpy().view(GMC_INFO_DTYPE)); None for an output not in `want`.
        d_rec / d_off / d_sd / d_stream_off / d_keep / compact as for scan_blobs_device.  `largest` is ready for
        sweep_streams_device: level L there is flags at min_blob_cells = L.  out: a dict of preallocated tensors by
        name.  Asynchronous on `stream` (default: torch's current stream)."""
        want = _wanted(want, GMC_BLOB_OUTPUTS)
        if (d_stream_off is None) != (d_keep is None):
            raise ValueError("d_stream_off and d_keep go together: give both or neither")
        n_frames = max(d_off.numel() - 1, 0)
        res = _device_outputs(GMC_BLOB_OUTPUTS, want, out, n_frames, d_off.device)
        if n_frames == 0:              # nothing to write (an empty tensor has no address to hand over)
            return res
        head, st = self._device_batch(d_rec, d_off, d_sd, compact, stream)
        ns = self._device_keep(d_stream_off, d_keep)
        check(self._lib.mtgpu_scan_gmc_blobs_device(*head, _dptr(d_stream_off), ns, _dptr(d_keep), int(max_shift),
                                                    int(min_share_q8), int(min_blob_cells),
                                                    *(_dptr(res[k]) for k in GMC_BLOB_OUTPUTS), st))
        return res

    # -------------------------------------------------------- temporal persistence
    def persist(self, flags, stream_off, has_sd=None, box=None, min_run: int = 1, max_dropout: int = 0, reach: int = 1) -> dict:
        """The runs of motion frames of a host batch (mtgpu_persist_flags, include/mtgpu_persist.h).  flags: uint8 [F]
        from any scan (non-zero: a motion frame); stream_off: [S + 1] frame offsets; has_sd uint8 [F] or None: a quiet
        frame without side data (a key frame) is transparent, it neither breaks a run nor counts as a dropout; box
        BLOB_BOX_DTYPE [F] or None: consecutive motion frames stay in one run only while their largest blobs' boxes lie
        within `reach` cells of each other; max_dropout: the quiet analysed frames a run bridges.  Returns a dict of
        numpy arrays over the frames: flags uint8 (flags != 0 and run >= max(1, min_run)), run uint32 (motion frames in
        the frame's run, 0 on a quiet frame), pos uint32 (1-based place in the run)."""
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        soff = np.ascontiguousarray(stream_off, dtype=np.uint64)
        n, ns = len(fl), max(len(soff) - 1, 0)
        sd = None if has_sd is None else np.ascontiguousarray(has_sd, dtype=np.uint8)
        bx = None if box is None else np.ascontiguousarray(box, dtype=BLOB_BOX_DTYPE)
        if (sd is not None and len(sd) != n) or (bx is not None and len(bx) != n):
            raise ValueError("has_sd and box have one element per frame")
        out = _host_outputs(PERSIST_OUTPUTS, n)
        check(self._lib.mtgpu_persist_flags(self._ctx, _ptr(fl), _ptr(sd), _ptr(bx), n, _ptr(soff) if len(soff) else None, ns,
                                            int(min_run), int(max_dropout), int(reach), *(_ptr(out[k]) for k in PERSIST_OUTPUTS)))
        return out

    def persist_device(self, d_flags, d_stream_off, d_has_sd=None, d_box=None, min_run: int = 1, max_dropout: int = 0,
                       reach: int = 1, want=PERSIST_OUTPUTS, out=None, work=None, stream=None) -> dict:
        """Device-resident batch (torch CUDA tensors) -> a dict of CUDA tensors over the frames: flags uint8, run / pos
        int32 (the bits of the library's uint32 counts); None for an output not in `want`.  d_flags uint8 [F];
        d_stream_off int64 [S + 1]; d_has_sd uint8 [F] or None; d_box int16 [F, 4] as scan_blobs_device returns it, or
        None.  `run` is ready for sweep_streams_device: level L there is flags at min_run = L.  out: a dict of
        preallocated tensors by name; work: int32 [F] workspace of the caller (else one is allocated and held until the
        launch has passed).  No output may share memory with an input.  Asynchronous on `stream` (default: torch's
        current stream)."""
        import torch
        dev = d_flags.device
        n_frames = d_flags.numel()
        res = _device_outputs(PERSIST_OUTPUTS, want, out, n_frames, dev)
        if n_frames == 0:              # nothing to write (an empty tensor has no address to hand over)
            return res
        assert d_flags.dtype == torch.uint8 and d_flags.is_contiguous()
        assert d_stream_off.dtype == torch.int64 and d_stream_off.is_contiguous()
        assert d_has_sd is None or (d_has_sd.dtype == torch.uint8 and d_has_sd.is_contiguous() and d_has_sd.numel() == n_frames)
        assert d_box is None or (d_box.dtype == torch.int16 and d_box.is_contiguous() and tuple(d_box.shape) == (n_frames, 4))
        held = work is None
        if held:
            work = torch.empty(n_frames, dtype=torch.int32, device=dev)
        assert work.dtype == torch.int32 and work.is_contiguous() and work.numel() >= n_frames
        check(self._lib.mtgpu_persist_flags_device(
            self._ctx, d_flags.data_ptr(), _dptr(d_has_sd), _dptr(d_box), n_frames, d_stream_off.data_ptr(),
            max(d_stream_off.numel() - 1, 0), int(min_run), int(max_dropout), int(reach), work.data_ptr(),
            *(_dptr(res[k]) for k in PERSIST_OUTPUTS), _stream_handle(dev, stream)))
        if held:
            self._hold(work, dev, stream)
        return res

    # ------------------------------------------------------- motion scalar
    def motion_scores(self, batch: FrameBatch) -> Tuple[np.ndarray, np.ndarray]:
        """Per-frame motion scores of a host batch (tools/motion_scalar.cpp:68-83 for every frame): the sum of
        sqrt(dx^2 + dy^2) * w * h over the frame's records with motion_scale != 0, and the number of those records.
        Returns (scores float64 [F], terms uint32 [F])."""
        n = batch.n_frames
        if n <= 0:
            return np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.uint32)
        import torch
        dev = torch.device("cuda", self.device)
        _, _, (mv, off, _, _) = _host_batch(batch)
        d_mv = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy()).to(dev)
        d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        scores, terms = self.motion_scores_device(d_mv, d_off)
        torch.cuda.synchronize(dev)
        return scores.cpu().numpy(), terms.cpu().numpy().view(np.uint32)

    def motion_scores_device(self, records, frame_off, scores=None, terms=None, stream=None):
        """Device-resident batch (torch CUDA tensors) -> (scores float64 [F], terms int32 [F], the bits of the library's
        uint32 counts).  records: the packed 40-byte records, frame_off: int64 [F+1].  terms=False: only the scores
        are computed (returns (scores, None)).  Asynchronous on `stream` (default: torch's current stream)."""
        import torch
        n_frames = frame_off.numel() - 1
        dev = frame_off.device
        if scores is None:
            scores = torch.empty(max(n_frames, 0), dtype=torch.float64, device=dev)
        terms = _optional(terms, max(n_frames, 0), _COUNT, dev, checked=n_frames > 0)
        if n_frames <= 0:
            return scores, terms
        assert records.is_contiguous() and frame_off.is_contiguous() and scores.is_contiguous()
        assert frame_off.dtype == torch.int64 and scores.dtype == torch.float64 and scores.numel() >= n_frames
        n_records = (records.numel() * records.element_size()) // 40
        check(self._lib.mtgpu_motion_scores_device(
            self._ctx, records.data_ptr() if n_records else None, n_records, frame_off.data_ptr(), n_frames,
            scores.data_ptr(), _dptr(terms), _stream_handle(dev, stream)))
        return scores, terms

    def motion_bins_device(self, scores, terms, pts, stream_off, n_sec: int, acc=None, bin_terms=None, stream=None):
        """Per-second bins of S streams (tools/motion_scalar.cpp:62-66, :82) from per-frame scores: scores float64 [F],
        terms int32 [F] or None, pts float64 [F] (seconds; negative, NaN and >= n_sec are skipped), stream_off int64
        [S+1].  Returns (acc float64 [S, n_sec], bin_terms int64 [S, n_sec] or None without terms): every bin adds
        its frames' scores in ascending frame order.  Asynchronous on `stream`."""
        import torch
        dev = pts.device
        n_streams = stream_off.numel() - 1
        n_sec = int(n_sec)
        if acc is None:
            acc = torch.empty((max(n_streams, 0), n_sec), dtype=torch.float64, device=dev)
        assert scores.dtype == torch.float64 and pts.dtype == torch.float64 and stream_off.dtype == torch.int64
        assert scores.is_contiguous() and pts.is_contiguous() and stream_off.is_contiguous() and acc.is_contiguous()
        assert acc.dtype == torch.float64 and acc.numel() >= max(n_streams, 0) * n_sec
        assert terms is None or (terms.dtype == torch.int32 and terms.is_contiguous())
        if bin_terms is None and terms is None:          # no counts in, none out
            bin_terms = False
        bin_terms = _optional(bin_terms, max(n_streams, 0), ("int64", (n_sec,)), dev)
        check(self._lib.mtgpu_motion_bins_device(
            self._ctx, scores.data_ptr(), _dptr(terms), pts.data_ptr(), stream_off.data_ptr(), max(n_streams, 0), n_sec,
            acc.data_ptr(), _dptr(bin_terms), _stream_handle(dev, stream)))
        return acc, bin_terms

    def motion_scalar(self, batch: FrameBatch, pts_seconds, n_sec: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """tools/motion_scalar.cpp:61-84 for one stream in host memory: (acc float64 [n_sec], bin_terms uint64 [n_sec]).
        pts_seconds[f]: the frame's timestamp in seconds, None (or negative) = null: the frame is skipped.  n_sec None:
        one more than the largest second that occurs.  A second has a row in the reference tool's output iff
        bin_terms[second] > 0."""
        pts = np.array([-1.0 if p is None else float(p) for p in pts_seconds], dtype=np.float64)
        n = batch.n_frames
        if len(pts) != max(n, 0):
            raise ValueError(f"{len(pts)} timestamps for {n} frames")
        if n_sec is None:
            ok = pts[np.isfinite(pts) & (pts >= 0)]
            n_sec = int(np.floor(ok.max())) + 1 if len(ok) else 1
        n_sec = int(n_sec)
        acc = np.zeros(max(n_sec, 0), dtype=np.float64)
        bin_terms = np.zeros(max(n_sec, 0), dtype=np.uint64)
        (mv, off, _, n), _, _ = _host_batch(batch)
        check(self._lib.mtgpu_motion_scalar(self._ctx, mv, off, _ptr(pts), n, n_sec, _ptr(acc) if n_sec > 0 else None,
                                            _ptr(bin_terms) if n_sec > 0 else None))
        return acc, bin_terms

    def scan_range(self, frame_pts: Sequence[int], frames: Sequence[Optional[np.ndarray]],
                   time_base: float, start: float, end: float, video_fps: float,
                   target_fps: Optional[float] = None) -> List[float]:
        """MotionScanner::scan_range (src/motion_scanner.cpp:297-391) over frames that a
        host decoder already produced for this chunk: `frame_pts[i]` / `frames[i]` are the
        AVFrame::pts and the MV side data (None = no side data) of the i-th frame returned
        after the seek.  Returns the motion timestamps of [start, end)."""
        skip = frame_skip(video_fps, config.target_fps() if target_fps is None else target_fps)
        idx, pts = filter_frames(frame_pts, time_base, start, end, skip)
        if not idx:
            return []
        batch = FrameBatch.from_frames([frames[i] for i in idx], pts)
        flags = self.check_frames(batch)
        return [p for p, f in zip(pts, flags) if f]

    # --------------------------------------------------------------- merge
    def merge_segments(self, timestamps: Iterable[float], mp: MergeParams, job_semantics: bool = False,
                       cap: Optional[int] = None) -> Tuple[np.ndarray, dict]:
        """sort + unique + gap merge + clamp + savings + cut decision on the device
        (src/pipeline.cpp:302-358, 387-388).  Returns (segments, result)."""
        ts = np.ascontiguousarray(np.asarray(list(timestamps) if not isinstance(timestamps, np.ndarray)
                                             else timestamps, dtype=np.float64))
        cap = (len(ts) + 1) if cap is None else cap
        seg = np.zeros(cap, dtype=SEGMENT_DTYPE)
        res = MergeResultC()
        c_mp = mp.to_c()
        check(self._lib.mtgpu_merge_segments(self._ctx, _ptr(ts) if len(ts) else None, len(ts),
                                             C.byref(c_mp), 1 if job_semantics else 0,
                                             _ptr(seg) if cap else None, cap, C.byref(res)))
        return seg[:res.n_segments].copy(), _fields(res)

    def merge_timestamps_device(self, ts, mp: MergeParams, job_semantics: bool = False, seg_cap: int = 64,
                                stream=None):
        """The same merge for ONE stream's pooled timestamps already on the device (1-D float64
        CUDA tensor, any order, duplicates allowed); large lists are sorted / merged by many
        workgroups.  Returns (segments float64 [seg_cap, 2], result uint8 [40]) device tensors;
        asynchronous on `stream` (default: torch's current stream)."""
        import torch
        assert ts.dtype == torch.float64 and ts.is_contiguous()
        dev = ts.device
        seg = torch.zeros((seg_cap, 2), dtype=torch.float64, device=dev)
        res = torch.zeros(MERGE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        c_mp = mp.to_c()
        check(self._lib.mtgpu_merge_timestamps_device(
            self._ctx, ts.data_ptr() if ts.numel() else None, ts.numel(), C.byref(c_mp),
            1 if job_semantics else 0, seg.data_ptr(), seg_cap, res.data_ptr(), _stream_handle(dev, stream)))
        return seg, res

    def merge_streams_device(self, flags, pts, stream_off, merge_params, job_semantics=False,
                             seg_cap=64, stream=None, out=None):
        """Per-stream timestamp pooling + merge without leaving the device.
        flags uint8 [F], pts float64 [F], stream_off int64 [S+1], merge_params: uint8 view of
        S mt_merge_params records (torch tensors on the scanner's device).
        Returns (segments float64 [S, seg_cap, 2], results uint8 [S, 40]).
        `out` = (segments, results, workspace float64 [2F]) reuses caller buffers (no allocation,
        no zero fill: entries past n_segments are then unspecified)."""
        import torch
        dev = pts.device
        n_streams = stream_off.numel() - 1
        n_frames = pts.numel()
        if out is not None:
            seg, res, ws = out
            assert seg.is_contiguous() and res.is_contiguous() and ws.numel() >= 2 * n_frames
            assert tuple(seg.shape) == (n_streams, seg_cap, 2) and res.shape[0] == n_streams
        else:
            ws = torch.empty(2 * max(n_frames, 1), dtype=torch.float64, device=dev)
            seg = torch.zeros((max(n_streams, 0), seg_cap, 2), dtype=torch.float64, device=dev)
            res = torch.zeros((max(n_streams, 0), MERGE_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        if n_streams <= 0:
            return seg, res
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream      # (direct: a timed loop of bench.py)
        check(self._lib.mtgpu_merge_streams_device(
            self._ctx, None if flags is None else flags.data_ptr(), pts.data_ptr(),
            stream_off.data_ptr(), n_streams, merge_params.data_ptr(), 1 if job_semantics else 0,
            ws.data_ptr(), seg.data_ptr(), seg_cap, res.data_ptr(), st))
        if out is None:
            self._hold(ws, dev, stream)
        return seg, res


# what a pipe's drain_centres() can carry per frame (mt_pipe_report), and which of them each scan mode of a pipe takes
_REPORTS = {"centres": _abi.MT_PIPE_REPORT_CENTRES, "largest": _abi.MT_PIPE_REPORT_LARGEST,
            "vector": _abi.MT_PIPE_REPORT_VECTOR, "sectors": _abi.MT_PIPE_REPORT_SECTORS}
_REPORT_NAMES = {code: name for name, code in _REPORTS.items()}
_MODE_REPORTS = {"blobs": ("centres", "largest"), "gmc": ("centres", "vector"), "gmc_blobs": ("centres", "largest", "vector"),
                 "dir": ("centres", "sectors"), "plane": ("centres", "sectors")}


def _report_code(mode, report) -> int:
    names = _MODE_REPORTS[mode]
    if report not in names:
        quoted = [repr(n) for n in names]
        raise ValueError(f"report is {report!r}, not {', '.join(quoted[:-1])} or {quoted[-1]}")
    return _REPORTS[report]


def _report_name(mode, code) -> str:
    """The report a getter of `mode` hands back for the library's code.  A code the mode does not take reads as
    "centres"; under gmc_blobs it is a KeyError (the library answers neither)."""
    name = _REPORT_NAMES.get(code)
    if mode == "gmc_blobs" and name not in _MODE_REPORTS[mode]:
        raise KeyError(code)
    return name if name in _MODE_REPORTS[mode] else "centres"


class ScanPipe:
    """Pinned, multi-buffered host->device scan pipeline (include/mtgpu.h "Host dispatcher"):
    what a decoder thread uses instead of calling check_frame per frame
    (src/motion_scanner.cpp:375-383).  feed() copies a frame's MV side data into pinned
    staging and submits full batches asynchronously; drain() returns every finished
    (pts, flag, tag) in submission order."""

    def __init__(self, scanner: MotionScanner, max_records: int, max_frames: int, n_buffers: int = 3,
                 layout: int = LAYOUT_COMPACT8 | LAYOUT_ZERO_COPY, centres: bool = False, boxes: bool = False):
        """layout: LAYOUT_COMPACT8 (8 of every 40 record bytes are staged) or LAYOUT_AOS40 (records
        staged unchanged), optionally | LAYOUT_ZERO_COPY (the scan reads the pinned staging over
        PCIe itself: no copy commands).  Default: compact + zero-copy.  Results are identical.
        centres=True (or layout | LAYOUT_CENTRES): every batch also carries the frames' centre counts
        (src/motion_scanner.cpp:272-294); read them with drain_centres().
        boxes=True (or layout | LAYOUT_BOXES, include/mtgpu_pipe_boxes.h): every batch submitted under set_blobs or
        set_gmc_blobs also carries the largest blob's box of every frame with a flag; read them with drain_boxes()."""
        self._lib = scanner._lib
        self._scanner = scanner            # keeps the context alive
        self._pipe = C.c_void_p()
        if centres:
            layout = int(layout) | LAYOUT_CENTRES
        if boxes:
            layout = int(layout) | LAYOUT_BOXES
        self._centres = (int(layout) & LAYOUT_CENTRES) != 0
        self._boxes = (int(layout) & LAYOUT_BOXES) != 0
        check(self._lib.mtgpu_pipe_create_layout(scanner._ctx, int(max_records), int(max_frames),
                                                 int(n_buffers), int(layout), C.byref(self._pipe)))
        scanner._pipes.add(self)
        self._cur = None
        self._inflight = 0
        self._done: List[Tuple[float, int, int]] = []
        self._done_centres: List[int] = []          # with LAYOUT_CENTRES: one count per entry of _done
        self._done_boxes: List[Tuple[int, int, int, int]] = []   # with LAYOUT_BOXES: one box per entry of _done
        self._box_error = None                      # the library's refusal of mtgpu_batch_boxes since the last drain

    def close(self):
        if getattr(self, "_pipe", None) and self._pipe.value:
            self._lib.mtgpu_pipe_destroy(self._pipe)
            self._pipe = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_keep(self, keep):
        """Ignore zones on the decode path (mtgpu_pipe_set_keep): from now on every batch of this pipe runs the masked
        scan — on the analysed rows a cell is active iff votes >= vectors_needed (src/motion_scanner.cpp:282) AND its keep
        bit is set.  keep: bool [grid_h, grid_w] (True = analysed), packed uint64 [grid_h, W] words (zones.pack_keep), or
        None: drop the mask, the plain scan again.  Only while no batch is being filled or in flight (call drain()
        first): otherwise MtgpuError(MT_ERR_BUSY) and nothing changes."""
        if keep is None:
            check(self._lib.mtgpu_pipe_set_keep(self._pipe, None))
            return
        p = self._scanner.params
        gh, gw, W = p.grid_h, p.grid_w, (p.grid_w + 63) // 64
        a = np.asarray(keep)
        if a.dtype != np.uint64:
            if a.shape != (gh, gw):
                raise ValueError(f"keep has shape {a.shape}, not {(gh, gw)} (or packed uint64 {(gh, W)})")
            from .zones import pack_keep
            a = pack_keep(a)
        a = np.ascontiguousarray(a, dtype=np.uint64)
        if a.shape != (gh, W):
            raise ValueError(f"packed keep has shape {a.shape}, not {(gh, W)}")
        check(self._lib.mtgpu_pipe_set_keep(self._pipe, _ptr(a)))

    @property
    def has_keep(self) -> bool:
        """True while the pipe's submits run the masked scan (mtgpu_pipe_has_keep)."""
        return self._lib.mtgpu_pipe_has_keep(self._pipe) == 1

    def set_blobs(self, min_blob_cells: int, report: str = "centres"):
        """A minimum blob size on the decode path (mtgpu_pipe_set_blobs): from now on every batch of this pipe runs the
        blob scan — flag = centres >= max(1, clusters_needed) AND largest blob >= min_blob_cells (the centres of
        src/motion_scanner.cpp:272-294, under the keep mask if the pipe has one).  min_blob_cells 0: off, the pipe as it
        was.  report: which count drain_centres() returns, "centres" or "largest" (the staging block has one count
        array; "largest" needs centres=True).  Only while no batch is being filled or in flight (call drain() first):
        otherwise MtgpuError(MT_ERR_BUSY) and nothing changes."""
        check(self._lib.mtgpu_pipe_set_blobs(self._pipe, int(min_blob_cells), _report_code("blobs", report)))

    @property
    def blobs(self) -> Optional[Tuple[int, str]]:
        """None, or (min_blob_cells, report) while the pipe's submits run the blob scan (mtgpu_pipe_blobs)."""
        n, r = C.c_int32(), C.c_int()
        if self._lib.mtgpu_pipe_blobs(self._pipe, C.byref(n), C.byref(r)) != 1:
            return None
        return int(n.value), _report_name("blobs", r.value)

    def set_gmc(self, max_shift: int = _abi.GMC_DEFAULT_MAX_SHIFT, min_share_q8: int = _abi.GMC_DEFAULT_MIN_SHARE_Q8,
                report: str = "centres"):
        """Global-motion compensation on the decode path (mtgpu_pipe_set_gmc): from now on every batch of this pipe is
        scanned against each frame's dominant vector (src/motion_scanner.cpp:246-292 on the residuals); under the keep
        mask, if the pipe has one, the estimate counts only records of kept cells and the active plane is the masked
        one.  report: what drain_centres() returns per frame, "centres" or "vector" — the applied vector packed as
        (uint16)gx | (uint16)gy << 16 (unpack_gmc_vector); "vector" needs centres=True.  Only while no batch is being
        filled or in flight (call drain() first): otherwise MtgpuError(MT_ERR_BUSY) and nothing changes.  Not together
        with set_blobs: MtgpuError(MT_ERR_UNSUPPORTED)."""
        check(self._lib.mtgpu_pipe_set_gmc(self._pipe, 1, int(max_shift), int(min_share_q8), _report_code("gmc", report)))

    def clear_gmc(self):
        """Compensation off (mtgpu_pipe_set_gmc with enable 0): the pipe is the plain or masked pipe it was before."""
        check(self._lib.mtgpu_pipe_set_gmc(self._pipe, 0, 0, 0, 0))

    def gmc(self) -> Optional[Tuple[int, int, str]]:
        """None, or (max_shift, min_share_q8, report) while the pipe's submits run the compensated scan (mtgpu_pipe_gmc)."""
        ms, q8, r = C.c_int32(), C.c_int32(), C.c_int()
        if self._lib.mtgpu_pipe_gmc(self._pipe, C.byref(ms), C.byref(q8), C.byref(r)) != 1:
            return None
        return int(ms.value), int(q8.value), _report_name("gmc", r.value)

    def set_gmc_blobs(self, min_blob_cells: int, max_shift: int = _abi.GMC_DEFAULT_MAX_SHIFT,
                      min_share_q8: int = _abi.GMC_DEFAULT_MIN_SHARE_Q8, report: str = "centres"):
        """The compensated blob scan on the decode path (mtgpu_pipe_set_gmc_blobs), the pipe's third mode: from now on
        every batch runs motion blobs on the residuals of each frame's dominant vector — flag = centres >=
        max(1, clusters_needed) AND largest blob >= min_blob_cells — under the keep mask if the pipe has one.
        min_blob_cells 0: off.  report: what drain_centres() returns per frame, "centres", "largest" or "vector"
        (unpack_gmc_vector); the last two need centres=True.  Only while no batch is being filled or in flight:
        otherwise MtgpuError(MT_ERR_BUSY) and nothing changes.  Not while set_blobs or set_gmc is on, nor they while
        this is: MtgpuError(MT_ERR_INVALID)."""
        check(self._lib.mtgpu_pipe_set_gmc_blobs(self._pipe, int(min_blob_cells), int(max_shift), int(min_share_q8),
                                                 _report_code("gmc_blobs", report)))

    def clear_gmc_blobs(self):
        """The compensated blob scan off (mtgpu_pipe_set_gmc_blobs with min_blob_cells 0): the pipe as it was before."""
        check(self._lib.mtgpu_pipe_set_gmc_blobs(self._pipe, 0, 0, 0, 0))

    def gmc_blobs(self) -> Optional[Tuple[int, int, int, str]]:
        """None, or (min_blob_cells, max_shift, min_share_q8, report) while the pipe's submits run the compensated blob
        scan (mtgpu_pipe_gmc_blobs)."""
        n, ms, q8, r = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int()
        if self._lib.mtgpu_pipe_gmc_blobs(self._pipe, C.byref(n), C.byref(ms), C.byref(q8), C.byref(r)) != 1:
            return None
        return int(n.value), int(ms.value), int(q8.value), _report_name("gmc_blobs", r.value)

    def set_dir(self, allow=_abi.DIR_ALL, report: str = "centres"):
        """The direction filter on the decode path (mtgpu_pipe_set_dir), the pipe's fourth mode: from now on a record of
        every batch votes only if the sector of dst - src is allowed (include/mtgpu_dir.h); under the keep mask, if the
        pipe has one, the rose counts only records of kept cells and the active plane is the masked one.  allow: the
        byte 0 .. 255, or sector names ("E,SE" / ["E", "SE"], direction.allow_from_names).  report: what
        drain_centres() returns per frame, "centres" or "sectors" — the frame's sector word
        (direction.unpack_sector_word); "sectors" needs centres=True.  Only while no batch is being filled or in flight
        (call drain() first): otherwise MtgpuError(MT_ERR_BUSY) and nothing changes.  Not together with set_blobs,
        set_gmc or set_gmc_blobs: MtgpuError(MT_ERR_UNSUPPORTED)."""
        code = _report_code("dir", report)
        if not isinstance(allow, (int, np.integer)):
            from .direction import allow_from_names
            allow = allow_from_names(allow)
        check(self._lib.mtgpu_pipe_set_dir(self._pipe, 1, int(allow), code))

    def clear_dir(self):
        """The direction filter off (mtgpu_pipe_set_dir with enable 0): the pipe is the plain or masked pipe it was before."""
        check(self._lib.mtgpu_pipe_set_dir(self._pipe, 0, 0, 0))

    def dir(self) -> Optional[Tuple[int, str]]:
        """None, or (allow, report) while the pipe's submits run the direction scan (mtgpu_pipe_dir)."""
        a, r = C.c_int32(), C.c_int()
        if self._lib.mtgpu_pipe_dir(self._pipe, C.byref(a), C.byref(r)) != 1:
            return None
        return int(a.value), _report_name("dir", r.value)

    def set_plane(self, plane, report: str = "centres"):
        """A direction plane on the decode path (mtgpu_pipe_set_plane): from now on a record of every batch votes only if
        the allow byte of its DESTINATION CELL has the bit of its sector (include/mtgpu_lanes.h); under the keep mask, if
        the pipe has one, the rose counts only records of kept cells and the active plane is the masked one.  plane:
        uint8 [grid_h, grid_w] (lanes.load_plane / lanes.learn_plane).  report: what drain_centres() returns per frame,
        "centres" or "sectors" — the frame's sector word (direction.unpack_sector_word); "sectors" needs centres=True.
        Only while no batch is being filled or in flight (call drain() first): otherwise MtgpuError(MT_ERR_BUSY) and
        nothing changes.  Not together with set_dir (MtgpuError(MT_ERR_INVALID): one rule at two granularities), nor
        with set_blobs, set_gmc or set_gmc_blobs (MtgpuError(MT_ERR_UNSUPPORTED))."""
        code = _report_code("plane", report)
        p = self._scanner.params
        a = np.asarray(plane)
        if a.dtype != np.uint8:
            raise ValueError(f"plane has dtype {a.dtype}, not uint8")
        if a.shape != (p.grid_h, p.grid_w):
            raise ValueError(f"plane has shape {a.shape}, not {(p.grid_h, p.grid_w)}")
        a = np.ascontiguousarray(a)
        check(self._lib.mtgpu_pipe_set_plane(self._pipe, _ptr(a), code))

    def clear_plane(self):
        """The direction plane off (mtgpu_pipe_set_plane with NULL): the pipe is the plain or masked pipe it was before."""
        check(self._lib.mtgpu_pipe_set_plane(self._pipe, None, 0))

    @property
    def plane(self) -> Optional[Tuple[np.ndarray, str]]:
        """None, or (plane uint8 [grid_h, grid_w], report) while the pipe's submits run the plane scan (mtgpu_pipe_plane)."""
        p = self._scanner.params
        a, r = np.zeros((p.grid_h, p.grid_w), np.uint8), C.c_int()
        if self._lib.mtgpu_pipe_plane(self._pipe, _ptr(a), C.byref(r)) != 1:
            return None
        return a, _report_name("plane", r.value)

    @staticmethod
    def unpack_gmc_vector(word: int) -> Tuple[int, int]:
        """(gx, gy) of a count reported under set_gmc(report="vector"): two signed 16-bit halves."""
        gx, gy = int(word) & 0xFFFF, (int(word) >> 16) & 0xFFFF
        return (gx - 0x10000 if gx >= 0x8000 else gx), (gy - 0x10000 if gy >= 0x8000 else gy)

    def _collect_one(self):
        b, fl, pts, tags, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
        rc = self._lib.mtgpu_pipe_collect(self._pipe, C.byref(b), C.byref(fl), C.byref(pts), C.byref(tags),
                                          C.byref(n))
        if rc != _abi.MT_OK:
            msg = self._lib.mtgpu_last_error().decode("utf-8", "replace")
            if b.value:                         # a failed collect still hands the batch out: give it back
                self._lib.mtgpu_pipe_release(self._pipe, b)
                self._inflight -= 1
            raise _abi.MtgpuError(rc, msg)
        k = n.value
        if k:
            f = np.ctypeslib.as_array(C.cast(fl, C.POINTER(C.c_uint8)), (k,)).copy()
            p = np.ctypeslib.as_array(C.cast(pts, C.POINTER(C.c_double)), (k,)).copy()
            t = np.ctypeslib.as_array(C.cast(tags, C.POINTER(C.c_uint64)), (k,)).copy()
            self._done += list(zip(p.tolist(), f.tolist(), t.tolist()))
            if self._centres:
                cp = C.c_void_p()
                check(self._lib.mtgpu_batch_centres(b, C.byref(cp)))
                self._done_centres += np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_uint32)), (k,)).tolist()
            if self._boxes:
                bp = C.c_void_p()
                rc = self._lib.mtgpu_batch_boxes(b, C.byref(bp))
                if rc == _abi.MT_OK:
                    # four uint16 per frame; specified where the flag is set, the no-blob box everywhere else
                    bx = np.ctypeslib.as_array(C.cast(bp, C.POINTER(C.c_uint16)), (k, 4)).copy()
                    bx[f == 0] = 0xFFFF
                    self._done_boxes += [tuple(r) for r in bx.tolist()]
                else:                           # not a blob submit: drain_boxes() raises this, drain() goes on
                    self._box_error = (rc, self._lib.mtgpu_last_error().decode("utf-8", "replace"))
                    self._done_boxes += [(0xFFFF,) * 4] * k
        check(self._lib.mtgpu_pipe_release(self._pipe, b))
        self._inflight -= 1

    def _acquire(self):
        while True:
            b = C.c_void_p()
            rc = self._lib.mtgpu_pipe_acquire(self._pipe, C.byref(b))
            if rc == _abi.MT_ERR_BUSY:          # back-pressure: finish the oldest batch first
                self._collect_one()
                continue
            check(rc)
            return b

    def _submit(self):
        if self._cur is not None:
            check(self._lib.mtgpu_pipe_submit(self._pipe, self._cur))
            self._cur = None
            self._inflight += 1

    def feed(self, mv: Optional[np.ndarray], pts: float, tag: int = 0):
        """One decoded frame: `mv` is its MV side data (MV_DTYPE array or raw bytes), None when
        the frame has no side data."""
        if mv is None:
            ptr, nbytes, sd = None, 0, 0
        else:
            a = np.ascontiguousarray(mv)
            ptr, nbytes, sd = (a.ctypes.data_as(C.c_void_p) if a.nbytes else None), a.nbytes, 1
        while True:
            if self._cur is None:
                self._cur = self._acquire()
            rc = self._lib.mtgpu_batch_add_frame(self._cur, ptr, nbytes, sd, float(pts), int(tag))
            if rc == _abi.MT_ERR_CAPACITY:      # batch full: ship it, start the next one
                self._submit()
                continue
            check(rc)
            return

    def drain(self) -> List[Tuple[float, int, int]]:
        """Submit the partial batch, wait for everything in flight, return and clear the
        accumulated (pts, flag, tag) list."""
        if self._cur is not None and self._lib.mtgpu_batch_frames(self._cur) > 0:
            self._submit()
        elif self._cur is not None:
            check(self._lib.mtgpu_pipe_release(self._pipe, self._cur))
            self._cur = None
        while self._inflight:
            self._collect_one()
        out, self._done = self._done, []
        self._last_centres, self._done_centres = self._done_centres, []
        self._last_boxes, self._done_boxes = self._done_boxes, []
        self._last_box_error, self._box_error = self._box_error, None
        return out

    def drain_centres(self) -> List[Tuple[float, int, int, int]]:
        """drain() of a pipe created with centres=True: (pts, flag, tag, count) in submission order — the centre count,
        or the largest blob's cell count after set_blobs(n, report="largest")."""
        if not self._centres:
            raise _abi.MtgpuError(_abi.MT_ERR_INVALID, "the pipe was created without centres=True / LAYOUT_CENTRES")
        out = self.drain()
        return [(p, f, t, c) for (p, f, t), c in zip(out, self._last_centres)]

    def drain_boxes(self) -> List[Tuple[float, int, int, Optional[int], Tuple[int, int, int, int]]]:
        """drain() of a pipe created with boxes=True under set_blobs / set_gmc_blobs: (pts, flag, tag, count, (x0, y0, x1,
        y1)) in submission order — count as drain_centres() reports it, None in a pipe without centres=True; the box is
        the largest blob's inclusive cell bounds (mtgpu_scan_blobs_device's `box`) where the flag is set and the no-blob
        box (0xFFFF,) * 4 everywhere else.  MtgpuError(MT_ERR_INVALID), the library's reason, when the pipe has no boxes
        or a drained batch was submitted in a mode that writes none (the results of that drain are dropped)."""
        if not self._boxes:
            raise _abi.MtgpuError(_abi.MT_ERR_INVALID, "the pipe was created without boxes=True / LAYOUT_BOXES")
        out = self.drain()
        if self._last_box_error is not None:
            raise _abi.MtgpuError(*self._last_box_error)
        counts = self._last_centres if self._centres else [None] * len(out)
        return [(p, f, t, c, b) for (p, f, t), c, b in zip(out, counts, self._last_boxes)]


def results_from_bytes(res_bytes: np.ndarray) -> np.ndarray:
    """uint8 [S,40] (host) -> structured mt_merge_result records."""
    return np.ascontiguousarray(res_bytes).view(MERGE_RESULT_DTYPE).reshape(-1)
