"""`python -m mvtrim_amd.tracks FILE [--top K] [--min-blob-cells N] [--min-track 1,2,3,5] [--max-dropout N] [--reach R] [--keep MASK.mtkeep] [--json]`

Object tracks: what "one of the frame's objects has existed for at least L motion frames" keeps of one recording.  An
object scan (`objects`) lists the K largest blobs of every frame; persistence (`persist`) follows one box per frame, the
largest blob, so a parked lorry that sways all day keeps every run alive and hides that the small object beside it has
existed for two frames.  A track links list entries from one motion frame to the next: an entry continues the
lowest-ranked entry of the previous motion frame whose box lies within --reach cells of its own; key frames, which are
never analysed, do not end a track, and --max-dropout quiet frames between two motion frames do not either.  MIN_TRACK
= L keeps a motion frame iff one of its objects belongs to a track that gets at least L frames deep.  FILE is the JSON
that tools/extract_mvs.cpp prints (mvjson.py) or a `.mtmv` container (mvfile.py), loaded as `tune` loads it.

One object scan (objects.scan_device), ONE tracks pass (link_device below) on its flags and lists without a copy to
the host in between, then the existing sweep (sweep_streams_device) merges once per level on `track`: per level the
frames kept, the segments and the seconds kept.  The row of --min-track 1 is the object scan's answer and is always
printed.  Then come the number of tracks and a histogram of their lengths, one count per root.  --keep MASK.mtkeep
applies ignore zones (zones.save_keep / `zones --save-mask`) to the scan.

This module is also the Python layer of include/mtgpu_tracks.h: preview(), link() and link_device() take a
MotionScanner and go through scanner.py's output table, as its own methods do.  (MotionScanner's own methods and the
package's export list are a recorded surface: tests/golden/scanner_calls.json.)

Width, height and duration come from a `.mtmv` header or from --width / --height / --duration.  Everything is computed
by libmtgpu; without a usable device the command fails, there is no CPU path.
"""
import argparse
import json
import sys

import numpy as np

from . import _abi, objects, tune, zones
from ._abi import OBJECT_DTYPE, OBJECTS_MAX, TracksPlanC, check
from .persist import HIST_EDGES, _reach, _u32, levels_with_one
from .scanner import (MergeParams, MotionScanner, ScanParams, results_from_bytes, _device_outputs, _dptr, _host_outputs, _preview, _ptr,
                      _stream_handle, _wanted)

OUTPUTS = ("pred", "age", "id", "len", "track", "flags")     # the order of the library's arguments; "flags" is flags_out
NO_PRED = _abi.TRACK_NO_PRED
NO_ID = _abi.TRACK_NO_ID

MAX_LEVELS = _abi.SWEEP_MAX_LEVELS
DEFAULT_LEVELS = (1, 2, 3, 5)


def preview(k: int = OBJECTS_MAX) -> dict:
    """How the tracks pass runs for `k` list entries per frame (mtgpu_tracks_preview): lanes per workgroup, the frames a
    workgroup takes per step, and the uint32 words of workspace per list entry.  Host only: works without a GPU.
    MtgpuError(MT_ERR_INVALID) for k outside 1 .. 16."""
    return _preview("mtgpu_tracks_preview", TracksPlanC, None, k)


def link(scanner: MotionScanner, flags, lists, stream_off, has_sd=None, min_cells: int = 1, max_dropout: int = 0, reach: int = 1,
         min_track: int = 1, want=OUTPUTS) -> dict:
    """The tracks of a host batch (mtgpu_track_objects, include/mtgpu_tracks.h).  flags: uint8 [F] from any scan (non-zero:
    a motion frame); lists: OBJECT_DTYPE [F, k] as objects.scan returns them (any order is legal); stream_off: [S + 1]
    frame offsets; has_sd uint8 [F] or None: a quiet frame without side data (a key frame) is transparent.  Returns a
    dict of numpy arrays: pred uint8 [F, k] (NO_PRED: none), age / id / len uint32 [F, k] (an absent entry reads age =
    len = 0, id = NO_ID), track uint32 [F] (the longest track among the frame's objects), flags uint8 [F] (flags != 0
    and track >= max(1, min_track)); None for an output not in `want`."""
    want = _wanted(want, OUTPUTS)
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    li = np.ascontiguousarray(lists, dtype=OBJECT_DTYPE)
    soff = np.ascontiguousarray(stream_off, dtype=np.uint64)
    n, ns = len(fl), max(len(soff) - 1, 0)
    if li.ndim != 2 or li.shape[0] != n:
        raise ValueError("lists has one row of k entries per frame")
    k = li.shape[1]
    sd = None if has_sd is None else np.ascontiguousarray(has_sd, dtype=np.uint8)
    if sd is not None and len(sd) != n:
        raise ValueError("has_sd has one element per frame")
    out = _host_outputs(OUTPUTS, n, want, grid=(k,))
    check(scanner._lib.mtgpu_track_objects(scanner._ctx, _ptr(fl), _ptr(sd), _ptr(li), k, n, _ptr(soff) if len(soff) else None, ns,
                                           int(min_cells), int(max_dropout), int(reach), int(min_track), *(_ptr(out[o]) for o in OUTPUTS)))
    return out


def link_device(scanner: MotionScanner, d_flags, d_list, d_stream_off, d_has_sd=None, min_cells: int = 1, max_dropout: int = 0,
                reach: int = 1, min_track: int = 1, want=OUTPUTS, out=None, work=None, stream=None) -> dict:
    """Device-resident batch (torch CUDA tensors) -> a dict of CUDA tensors: pred uint8 [F, k], age / id / len int32
    [F, k] (the bits of the library's uint32 values), track int32 [F], flags uint8 [F]; None for an output not in `want`.
    d_flags uint8 [F]; d_list int32 [F, k, 4] as objects.scan_device returns it; d_stream_off int64 [S + 1]; d_has_sd
    uint8 [F] or None.  `track` is ready for sweep_streams_device: level L there is flags at min_track = L.  out: a dict
    of preallocated tensors by name; work: int32 workspace of the caller, preview(k)["work_words_per_entry"] * F * k
    elements (else one is allocated and held until the launch has passed).  No output may share memory with an input.
    Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    dev = d_flags.device
    n_frames = d_flags.numel()
    assert d_list.dtype == torch.int32 and d_list.is_contiguous() and d_list.dim() == 3 and d_list.shape[0] == n_frames and d_list.shape[2] == 4
    k = int(d_list.shape[1])
    res = _device_outputs(OUTPUTS, want, out, n_frames, dev, grid=(k,))
    if n_frames == 0:              # nothing to write (an empty tensor has no address to hand over)
        return res
    assert d_flags.dtype == torch.uint8 and d_flags.is_contiguous()
    assert d_stream_off.dtype == torch.int64 and d_stream_off.is_contiguous()
    assert d_has_sd is None or (d_has_sd.dtype == torch.uint8 and d_has_sd.is_contiguous() and d_has_sd.numel() == n_frames)
    words = _abi.TRACK_WORK_WORDS * n_frames * max(k, 1)
    held = work is None
    if held:
        work = torch.empty(words, dtype=torch.int32, device=dev)
    assert work.dtype == torch.int32 and work.is_contiguous() and work.numel() >= words
    check(scanner._lib.mtgpu_track_objects_device(
        scanner._ctx, d_flags.data_ptr(), _dptr(d_has_sd), d_list.data_ptr(), k, n_frames, d_stream_off.data_ptr(),
        max(d_stream_off.numel() - 1, 0), int(min_cells), int(max_dropout), int(reach), int(min_track), work.data_ptr(),
        *(_dptr(res[o]) for o in OUTPUTS), _stream_handle(dev, stream)))
    if held:
        scanner._hold(work, dev, stream)
    return res


def _levels(text):
    try:
        v = [int(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--min-track: {text!r} is not a comma-separated list of whole numbers")
    if not 1 <= len(v) <= MAX_LEVELS - 1:
        raise argparse.ArgumentTypeError(f"--min-track: {len(v)} levels, want 1 .. {MAX_LEVELS - 1}")
    if any(not 1 <= x < 2 ** 31 for x in v):
        raise argparse.ArgumentTypeError(f"--min-track: {text!r}: a level is at least 1 and fits int32")
    if len(set(v)) != len(v):
        raise argparse.ArgumentTypeError(f"--min-track: {text!r} names a level twice")
    return v


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.tracks", description=__doc__.splitlines()[2])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    ap.add_argument("--top", type=objects._top, metavar="K", default=OBJECTS_MAX,
                    help=f"list entries per frame, 1 .. {OBJECTS_MAX} (default {OBJECTS_MAX})")
    ap.add_argument("--min-blob-cells", type=objects._cells, metavar="N", default=1,
                    help="an object is a blob of at least N cells (default 1)")
    ap.add_argument("--min-track", type=_levels, metavar="L[,L...]", default=list(DEFAULT_LEVELS),
                    help="the levels: least depth of the longest track among a frame's objects (default 1,2,3,5; 1 is always reported)")
    ap.add_argument("--max-dropout", type=_u32("--max-dropout"), metavar="N", default=0,
                    help="analysed quiet frames between two motion frames that do not end a track (default 0)")
    ap.add_argument("--reach", type=_reach, metavar="R", default=1, help="cells two linked boxes may lie apart (default 1)")
    ap.add_argument("--keep", metavar="MASK.mtkeep", help="ignore zones: a .mtkeep text mask, 1 = analysed")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--duration", type=float, help="seconds")
    ap.add_argument("--block-size", type=int)
    ap.add_argument("--block-shift", type=int)
    ap.add_argument("--vectors-needed", type=int)
    ap.add_argument("--mv-threshold-sq", type=float)
    ap.add_argument("--vertical-mask", type=float)
    ap.add_argument("--max-gap-sec", type=float)
    ap.add_argument("--padding-sec", type=float)
    ap.add_argument("--min-savings-pct", type=float)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", action="store_true", help="one JSON document instead of the table")
    return ap


def histogram(length, pred, age):
    """Track lengths, one count per track (taken from `len` at the roots: present entries without predecessor): {"1":
    tracks of one frame, "2": ..., "3-4": ..., "100+": ...}, in that order."""
    length, pred, age = (np.asarray(a).reshape(-1) for a in (length, pred, age))
    lengths = length.astype(np.int64)[(pred == NO_PRED) & (age == 1)]
    out = {}
    for i, lo in enumerate(HIST_EDGES):
        hi = HIST_EDGES[i + 1] - 1 if i + 1 < len(HIST_EDGES) else None
        label = f"{lo}+" if hi is None else str(lo) if hi == lo else f"{lo}-{hi}"
        out[label] = int(((lengths >= lo) & ((lengths <= hi) if hi is not None else True)).sum())
    return out


def measure(scanner, batch, pts, levels, merge_params, k=OBJECTS_MAX, min_blob_cells=1, max_dropout=0, reach=1, keep=None):
    """One object scan, one tracks pass, then the sweep on `track`.  keep: bool [gh, gw] or None.  Returns a dict."""
    import torch
    dev = torch.device("cuda", scanner.device)
    p = scanner.params
    n = batch.n_frames
    mv = np.ascontiguousarray(batch.mv, dtype=_abi.MV_DTYPE)
    # a frame without records was never analysed: transparent, as a key frame is
    has = np.diff(np.asarray(batch.frame_off).astype(np.int64)) > 0 if batch.has_sd is None else np.asarray(batch.has_sd) != 0
    d_rec = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy()).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(batch.frame_off, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_sd = torch.from_numpy(np.ascontiguousarray(has, dtype=np.uint8)).to(dev)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(dev)
    d_soff = torch.tensor([0, n], dtype=torch.int64, device=dev)
    d_mp = torch.from_numpy(merge_params.to_record().view(np.uint8).copy()).to(dev)
    levels = levels_with_one(levels)
    with torch.cuda.device(dev):
        d_keep = None
        if keep is not None:
            d_keep = torch.from_numpy(zones.pack_keep(keep).view(np.int64).copy()).reshape(1, p.grid_h, -1).to(dev)
        scan = objects.scan_device(scanner, d_rec, d_off, d_sd, k, min_blob_cells, 1, d_soff if keep is not None else None, d_keep,
                                   want=("flags", "list"))
        res = link_device(scanner, scan["flags"], scan["list"], d_soff, d_sd, min_blob_cells, max_dropout, reach, 1,
                          want=("pred", "age", "len", "track"))
        _seg, r8 = scanner.sweep_streams_device(res["track"], d_pts, d_soff, d_mp, levels, seg_cap=1)
        torch.cuda.synchronize(dev)
    track = res["track"].cpu().numpy().view(np.uint32)
    length = res["len"].cpu().numpy().view(np.uint32)
    pred, age = res["pred"].cpu().numpy(), res["age"].cpu().numpy().view(np.uint32)
    rows = []
    for i, lv in enumerate(levels):
        r = results_from_bytes(r8[i].cpu().numpy())[0]
        if int(r["status"]) != _abi.MT_OK:
            raise _abi.MtgpuError(int(r["status"]), "timestamps contain NaN")
        removed = float(r["time_removed"]) if int(r["n_segments"]) else float(merge_params.duration)
        rows.append({"min_track": int(lv), "motion_frames": int((track >= lv).sum()), "frames_kept": int(r["n_timestamps"]),
                     "segments": int(r["n_segments"]), "seconds_kept": float(merge_params.duration) - removed,
                     "saved_pct": float(r["saved_pct"]), "do_cut": int(r["do_cut"])})
    return {"levels": rows, "tracks": int(((pred == NO_PRED) & (age == 1)).sum()), "longest_track": int(track.max()) if n else 0,
            "track_lengths": histogram(length, pred, age)}


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad option: nothing below has run, no device has been touched
    try:
        path = a.file
        batch, pts, hdr = tune.load(path)
        path = a.keep
        keep = None if path is None else zones.load_keep(path)
    except (OSError, ValueError, KeyError) as e:
        print(f"tracks: cannot read {path}: {e}", file=sys.stderr)
        return 1
    width = a.width if a.width is not None else hdr.get("width")
    height = a.height if a.height is not None else hdr.get("height")
    duration = a.duration if a.duration is not None else hdr.get("duration")
    if width is None or height is None or duration is None:
        ap.error("the file carries no width / height / duration: give --width, --height and --duration")
    params = ScanParams.from_config(width, height, block_size=a.block_size, block_shift=a.block_shift,
                                    vectors_needed=a.vectors_needed, mv_threshold_sq=a.mv_threshold_sq,
                                    clusters_needed=1, vertical_mask=a.vertical_mask)
    if keep is not None and keep.shape != (params.grid_h, params.grid_w):
        ap.error(f"--keep: the mask is for a {keep.shape[1]}x{keep.shape[0]} grid, this one is {params.grid_w}x{params.grid_h}")
    mp = MergeParams(duration=float(duration), max_gap_sec=a.max_gap_sec, padding_sec=a.padding_sec,
                     min_savings_pct=a.min_savings_pct)
    try:
        with MotionScanner(params, device=a.device) as s:
            res = measure(s, batch, pts, a.min_track, mp, a.top, a.min_blob_cells, a.max_dropout, a.reach, keep)
    except _abi.MtgpuError as e:
        print(f"tracks: {e}", file=sys.stderr)
        return 1
    if a.json:
        print(json.dumps({"file": a.file, "width": width, "height": height, "grid_w": params.grid_w, "grid_h": params.grid_h,
                          "frames": batch.n_frames, "keep": a.keep, "top": a.top, "min_blob_cells": a.min_blob_cells,
                          "max_dropout": a.max_dropout, "reach": a.reach, **res}))
        return 0
    print(f"# grid {params.grid_w} x {params.grid_h}, {batch.n_frames} frames, {res['tracks']} tracks; the longest is "
          f"{res['longest_track']} motion frames deep; top {a.top}, min_blob_cells {a.min_blob_cells}, max_dropout {a.max_dropout}, "
          f"reach {a.reach}")
    print("min_track motion_frames frames_kept segments seconds_kept saved_pct do_cut")
    for r in res["levels"]:
        print("%-9d %-13d %-11d %-8d %-12.2f %-9.2f %d" % (r["min_track"], r["motion_frames"], r["frames_kept"], r["segments"],
                                                           r["seconds_kept"], r["saved_pct"], r["do_cut"]))
    print("track lengths: " + "  ".join(f"{k}: {v}" for k, v in res["track_lengths"].items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
