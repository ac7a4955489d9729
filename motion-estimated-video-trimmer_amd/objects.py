"""`python -m mvtrim_amd.objects FILE [--top K] [--min-blob-cells N] [--min-objects 1,2,3] [--keep MASK.mtkeep] [--json]`

Object lists: how many objects a frame holds, and what "at least N things of at least M cells" keeps of one recording.
A blob is a 4-connected component of a frame's centre cells (the cells src/motion_scanner.cpp:272-294 counts); an
OBJECT is a blob of at least MIN_BLOB_CELLS cells, and MIN_OBJECTS = L keeps a frame iff it holds at least L objects: a
crowd, two vehicles at a gate.  FILE is the JSON that tools/extract_mvs.cpp prints (mvjson.py) or a `.mtmv` container
(mvfile.py), loaded as `tune` loads it.

One object scan (scan_device below) returns every frame's object count and the list of its K largest
blobs; the existing sweep (sweep_streams_device) then merges once per level on `objects`: per level the frames kept,
the segments and the seconds kept.  The scan itself runs with CLUSTERS_NEEDED 1, as `blobs` does: a level is the only
bar a frame has to pass.  Then come a histogram of objects per frame and one of the listed sizes (every listed blob,
whatever MIN_BLOB_CELLS is).  --keep MASK.mtkeep applies ignore zones (zones.save_keep / `zones --save-mask`) to the
scan.

This module is also the Python layer of include/mtgpu_objects.h: preview(), scan() and scan_device() take a
MotionScanner and go through scanner.py's batch marshaller and output table, as its own methods do; OBJECT_DTYPE is the
list's element.  (MotionScanner's own methods and the package's export list are a recorded surface:
tests/golden/scanner_calls.json.)

Width, height and duration come from a `.mtmv` header or from --width / --height / --duration.  Everything is computed
by libmtgpu; without a usable device the command fails, there is no CPU path.
"""
import argparse
import json
import sys

import numpy as np

from . import _abi, tune, zones
from .blobs import histogram
from ._abi import OBJECT_DTYPE, OBJECTS_MAX, ObjectsPlanC, check
from .scanner import (FrameBatch, MergeParams, MotionScanner, ScanParams, results_from_bytes, _device_outputs, _dptr, _host_batch,
                      _host_outputs, _preview, _ptr, _wanted)

OUTPUTS = ("flags", "centres", "blobs", "objects", "list")     # the order of the library's arguments

MAX_LEVELS = _abi.SWEEP_MAX_LEVELS
DEFAULT_LEVELS = (1, 2, 3)
SIZE_BINS = (1, 2, 4, 8, 16, 32, 64)       # the size histogram's bins begin here: "1", "2-3", "4-7", ..., "64+"


def preview(params: ScanParams, k: int = OBJECTS_MAX, lds_bytes: int = 163840) -> dict:
    """How the object scan runs on the grid of `params` with `k` list entries per frame and that much LDS per workgroup
    (mtgpu_objects_preview): LDS bytes (the blob scan's plus 24 per entry), lanes, and the sizes of a keep mask.  Host
    arithmetic only: works without a GPU.  MtgpuError(MT_ERR_INVALID) for k outside 1 .. 16, MtgpuError(MT_ERR_UNSUPPORTED)
    for a grid the object scan has no form for."""
    return _preview("mtgpu_objects_preview", ObjectsPlanC, params, k, lds_bytes)


def scan(scanner: MotionScanner, batch: FrameBatch, k: int = OBJECTS_MAX, min_blob_cells: int = 1, min_objects: int = 1,
         stream_off=None, keep=None) -> dict:
    """The object scan of a host batch (mtgpu_scan_frames_objects): the k largest blobs of every frame, ranked and boxed.
    Returns a dict of numpy arrays over the frames: flags uint8 (centres >= max(1, clusters_needed) and objects >=
    max(1, min_objects)), centres uint32, blobs uint32, objects uint32 (the blobs of at least min_blob_cells cells,
    listed or not), list OBJECT_DTYPE [F, k] (cells descending, then first ascending; an empty entry reads cells 0,
    first 0xFFFFFFFF, bounds 0xFFFF).  stream_off / keep: per-stream keep masks as for MotionScanner.scan_zones, both or
    neither."""
    if (stream_off is None) != (keep is None):
        raise ValueError("stream_off and keep go together: give both or neither")
    head, (soff, ns), _ = _host_batch(batch, stream_off)
    if keep is not None:
        keep = scanner._keep_words(keep, ns)
    out = _host_outputs(OUTPUTS, head[3], grid=(max(int(k), 0),))
    check(scanner._lib.mtgpu_scan_frames_objects(scanner._ctx, *head, soff, ns, _ptr(keep), int(k), int(min_blob_cells),
                                                 int(min_objects), *(_ptr(out[n]) for n in OUTPUTS)))
    return out


def scan_device(scanner: MotionScanner, d_rec, d_off, d_sd, k: int = OBJECTS_MAX, min_blob_cells: int = 1, min_objects: int = 1,
                d_stream_off=None, d_keep=None, compact=False, want=OUTPUTS, out=None, stream=None) -> dict:
    """Device-resident batch (torch CUDA tensors) -> a dict of CUDA tensors over the frames: flags uint8, centres / blobs
    / objects int32 (the bits of the library's uint32 counts), list int32 [F, k, 4] (the bits of mt_object:
    list.cpu().numpy().view(OBJECT_DTYPE)[..., 0] is [F, k]); None for an output not in `want`.  d_rec / d_off / d_sd /
    d_stream_off / d_keep / compact as for MotionScanner.scan_blobs_device.  `objects` is ready for
    sweep_streams_device: with clusters_needed <= 1, level L there is flags at min_objects = L.  out: a dict of
    preallocated tensors by name.  Asynchronous on `stream` (default: torch's current stream)."""
    want = _wanted(want, OUTPUTS)
    if (d_stream_off is None) != (d_keep is None):
        raise ValueError("d_stream_off and d_keep go together: give both or neither")
    n_frames = max(d_off.numel() - 1, 0)
    res = _device_outputs(OUTPUTS, want, out, n_frames, d_off.device, grid=(max(int(k), 0), 4))
    if n_frames == 0:              # nothing to write (an empty tensor has no address to hand over)
        return res
    head, st = scanner._device_batch(d_rec, d_off, d_sd, compact, stream)
    ns = scanner._device_keep(d_stream_off, d_keep)
    check(scanner._lib.mtgpu_scan_objects_device(*head, _dptr(d_stream_off), ns, _dptr(d_keep), int(k), int(min_blob_cells),
                                                 int(min_objects), *(_dptr(res[n]) for n in OUTPUTS), st))
    return res


def _levels(text):
    try:
        v = [int(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--min-objects: {text!r} is not a comma-separated list of whole numbers")
    if not 1 <= len(v) <= MAX_LEVELS:
        raise argparse.ArgumentTypeError(f"--min-objects: {len(v)} levels, want 1 .. {MAX_LEVELS}")
    if any(not 1 <= x < 2 ** 31 for x in v):
        raise argparse.ArgumentTypeError(f"--min-objects: {text!r}: a level is at least 1 and fits int32")
    if len(set(v)) != len(v):
        raise argparse.ArgumentTypeError(f"--min-objects: {text!r} names a level twice")
    return v


def _top(text):
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--top: {text!r} is not a whole number")
    if not 1 <= k <= _abi.OBJECTS_MAX:
        raise argparse.ArgumentTypeError(f"--top: {k}, want 1 .. {_abi.OBJECTS_MAX}")
    return k


def _cells(text):
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--min-blob-cells: {text!r} is not a whole number")
    if not 1 <= n < 2 ** 31:
        raise argparse.ArgumentTypeError(f"--min-blob-cells: {n}: at least 1 and fits int32")
    return n


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.objects", description=__doc__.splitlines()[2])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    ap.add_argument("--top", type=_top, metavar="K", default=_abi.OBJECTS_MAX,
                    help=f"list entries per frame, 1 .. {_abi.OBJECTS_MAX} (default {_abi.OBJECTS_MAX})")
    ap.add_argument("--min-blob-cells", type=_cells, metavar="N", default=1,
                    help="an object is a blob of at least N cells (default 1)")
    ap.add_argument("--min-objects", type=_levels, metavar="L[,L...]", default=list(DEFAULT_LEVELS),
                    help="the levels: least object counts of a frame (default 1,2,3)")
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


def size_histogram(cells):
    """{"1": listed blobs of one cell, "2-3": ..., "64+": ...}, in that order; entries with cells 0 are no blobs."""
    c = np.asarray(cells).astype(np.int64).reshape(-1)
    c = c[c > 0]
    out = {}
    for i, lo in enumerate(SIZE_BINS):
        hi = SIZE_BINS[i + 1] if i + 1 < len(SIZE_BINS) else None
        name = f"{lo}+" if hi is None else str(lo) if hi == lo + 1 else f"{lo}-{hi - 1}"
        out[name] = int(((c >= lo) & ((c < hi) if hi is not None else True)).sum())
    return out


def measure(scanner, batch, pts, levels, merge_params, k=_abi.OBJECTS_MAX, min_blob_cells=1, keep=None):
    """One object scan, then the sweep on `objects`.  keep: bool [gh, gw] or None.  Returns a dict."""
    import torch
    dev = torch.device("cuda", scanner.device)
    p = scanner.params
    n = batch.n_frames
    mv = np.ascontiguousarray(batch.mv, dtype=_abi.MV_DTYPE)
    d_rec = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy()).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(batch.frame_off, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_sd = None if batch.has_sd is None else torch.from_numpy(np.ascontiguousarray(batch.has_sd, dtype=np.uint8)).to(dev)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(dev)
    d_soff = torch.tensor([0, n], dtype=torch.int64, device=dev)
    d_mp = torch.from_numpy(merge_params.to_record().view(np.uint8).copy()).to(dev)
    with torch.cuda.device(dev):
        d_keep = None
        if keep is not None:
            d_keep = torch.from_numpy(zones.pack_keep(keep).view(np.int64).copy()).reshape(1, p.grid_h, -1).to(dev)
        res = scan_device(scanner, d_rec, d_off, d_sd, k, min_blob_cells, 1, d_soff if keep is not None else None, d_keep,
                                          want=("centres", "blobs", "objects", "list"))
        swept = scanner.sweep_streams_device(res["objects"], d_pts, d_soff, d_mp, levels, seg_cap=1)
        torch.cuda.synchronize(dev)
    objects = res["objects"].cpu().numpy().view(np.uint32)
    listed = res["list"].cpu().numpy().reshape(n, k, 4).view(OBJECT_DTYPE)[..., 0]
    rows = []
    for i, lv in enumerate(levels):
        r = results_from_bytes(swept[1][i].cpu().numpy())[0]
        if int(r["status"]) != _abi.MT_OK:
            raise _abi.MtgpuError(int(r["status"]), "timestamps contain NaN")
        rows.append({"level": int(lv), "motion_frames": int((objects >= lv).sum()), "frames_kept": int(r["n_timestamps"]),
                     "segments": int(r["n_segments"]), "seconds_kept": float(merge_params.duration) - float(r["time_removed"]),
                     "saved_pct": float(r["saved_pct"]), "do_cut": int(r["do_cut"])})
    return {"levels": rows, "objects_per_frame": histogram(objects), "listed_sizes": size_histogram(listed["cells"]),
            "largest_blob": int(listed["cells"].max()) if n else 0,
            "centres": int(res["centres"].cpu().numpy().view(np.uint32).sum(dtype=np.uint64))}


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad option: nothing below has run, no device has been touched
    try:
        path = a.file
        batch, pts, hdr = tune.load(path)
        path = a.keep
        keep = None if path is None else zones.load_keep(path)
    except (OSError, ValueError, KeyError) as e:
        print(f"objects: cannot read {path}: {e}", file=sys.stderr)
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
            res = measure(s, batch, pts, a.min_objects, mp, a.top, a.min_blob_cells, keep)
    except _abi.MtgpuError as e:
        print(f"objects: {e}", file=sys.stderr)
        return 1
    if a.json:
        print(json.dumps({"file": a.file, "width": width, "height": height, "grid_w": params.grid_w, "grid_h": params.grid_h,
                          "frames": batch.n_frames, "keep": a.keep, "top": a.top, "min_blob_cells": a.min_blob_cells, **res}))
        return 0
    print(f"# grid {params.grid_w} x {params.grid_h}, {batch.n_frames} frames, {res['centres']} centres; an object has at least "
          f"{a.min_blob_cells} cells; the largest blob has {res['largest_blob']}")
    print("MIN_OBJECTS motion_frames frames_kept segments seconds_kept saved_pct do_cut")
    for r in res["levels"]:
        print("%-11d %-13d %-11d %-8d %-12.2f %-9.2f %d" % (r["level"], r["motion_frames"], r["frames_kept"], r["segments"],
                                                           r["seconds_kept"], r["saved_pct"], r["do_cut"]))
    print("objects per frame: " + "  ".join(f"{k}: {v}" for k, v in res["objects_per_frame"].items()))
    print(f"sizes of the listed blobs (top {a.top}): " + "  ".join(f"{k}: {v}" for k, v in res["listed_sizes"].items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
