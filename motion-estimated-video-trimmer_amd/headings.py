"""`python -m mvtrim_amd.headings FILE [--top K] [--min-blob-cells N] [--min-objects 1,2,3] [--allow NAMES | --ignore NAMES] [--keep MASK.mtkeep] [--json]`

Object headings: which way each object of a frame moves, and what "at least N objects heading THAT way" keeps of one
recording.  An object is a blob of at least MIN_BLOB_CELLS cells (objects.py); its heading is the sector — E, SE, S, SW,
W, NW, N, NE (direction.py) — in which most of the records that land in its cells point, the lowest sector on a tie, and
"none" when they are all still.  FILE is the JSON that tools/extract_mvs.cpp prints (mvjson.py) or a `.mtmv` container
(mvfile.py), loaded as `tune` loads it.

Two heading scans (scan_device below) — one with every sector allowed, one with the byte of --allow / --ignore — return
per frame the number of listed objects whose heading is allowed; the existing sweep (sweep_streams_device) then merges
once per level on `allowed`: per level the frames kept, the segments and the seconds kept, under all sectors and under
the byte.  The scan itself runs with CLUSTERS_NEEDED 1, as `objects` does.  Then comes a histogram of the headings of
the objects: eight sectors plus "none".  --keep MASK.mtkeep applies ignore zones (zones.save_keep / `zones
--save-mask`) to the scan.

This module is also the Python layer of include/mtgpu_headings.h: preview(), scan() and scan_device() take a
MotionScanner and go through scanner.py's batch marshaller and output table, as its own methods do; HEADING_DTYPE is the
element of `motion`, NO_HEADING the heading of an object whose records are all still, and mean_vector() divides the
summed displacement by the record count on the host.  (MotionScanner's own methods and the package's export list are a
recorded surface: tests/golden/scanner_calls.json.)

Width, height and duration come from a `.mtmv` header or from --width / --height / --duration.  Everything is computed
by libmtgpu; without a usable device the command fails, there is no CPU path.
"""
import argparse
import json
import sys

import numpy as np

from . import _abi, direction, tune, zones
from ._abi import HEADING_DTYPE, OBJECT_DTYPE, OBJECTS_MAX, HeadingsPlanC, check
from .objects import _cells, _levels, _top
from .scanner import (FrameBatch, MergeParams, MotionScanner, ScanParams, results_from_bytes, _device_outputs, _dptr, _host_batch,
                      _host_outputs, _preview, _ptr, _wanted)

OUTPUTS = ("flags", "centres", "blobs", "objects", "list", "motion", "allowed")     # the order of the library's arguments
NO_HEADING = _abi.HEADING_NONE
ALL = direction.ALL
HEADING_WORDS = HEADING_DTYPE.itemsize // 4        # int32 words of one mt_heading on the device

DEFAULT_LEVELS = (1, 2, 3)


def preview(params: ScanParams, k: int = OBJECTS_MAX, lds_bytes: int = 163840) -> dict:
    """How the heading scan runs on the grid of `params` with `k` list entries per frame and that much LDS per workgroup
    (mtgpu_headings_preview): LDS bytes (the object scan's plus 56 per entry), lanes, and the sizes of a keep mask.  Host
    arithmetic only: works without a GPU.  MtgpuError(MT_ERR_INVALID) for k outside 1 .. 16, MtgpuError(MT_ERR_UNSUPPORTED)
    for a grid the heading scan has no form for."""
    return _preview("mtgpu_headings_preview", HeadingsPlanC, params, k, lds_bytes)


def _grid(name, k):
    k = max(int(k), 0)
    return {"list": (k,), "motion": (k,)}.get(name, ())


def scan(scanner: MotionScanner, batch: FrameBatch, k: int = OBJECTS_MAX, min_blob_cells: int = 1, min_objects: int = 1,
         allow: int = ALL, stream_off=None, keep=None) -> dict:
    """The heading scan of a host batch (mtgpu_scan_frames_headings).  Returns a dict of numpy arrays over the frames:
    flags uint8 (centres >= max(1, clusters_needed) and allowed >= max(1, min_objects)), centres / blobs / objects uint32
    and list OBJECT_DTYPE [F, k] as objects.scan returns them, motion HEADING_DTYPE [F, k] (an entry without a blob reads
    zeros with heading NO_HEADING), allowed uint32 (the listed objects of at least min_blob_cells cells whose heading is
    NO_HEADING or has its bit in `allow`).  min_objects is at most k.  stream_off / keep: per-stream keep masks as for
    MotionScanner.scan_zones, both or neither."""
    if (stream_off is None) != (keep is None):
        raise ValueError("stream_off and keep go together: give both or neither")
    head, (soff, ns), _ = _host_batch(batch, stream_off)
    if keep is not None:
        keep = scanner._keep_words(keep, ns)
    out = {}
    for name in OUTPUTS:
        out.update(_host_outputs((name,), head[3], grid=_grid(name, k)))
    check(scanner._lib.mtgpu_scan_frames_headings(scanner._ctx, *head, soff, ns, _ptr(keep), int(k), int(min_blob_cells),
                                                  int(min_objects), int(allow), *(_ptr(out[n]) for n in OUTPUTS)))
    return out


def scan_device(scanner: MotionScanner, d_rec, d_off, d_sd, k: int = OBJECTS_MAX, min_blob_cells: int = 1, min_objects: int = 1,
                allow: int = ALL, d_stream_off=None, d_keep=None, compact=False, want=OUTPUTS, out=None, stream=None) -> dict:
    """Device-resident batch (torch CUDA tensors) -> a dict of CUDA tensors over the frames: flags uint8, centres / blobs
    / objects / allowed int32 (the bits of the library's uint32 counts), list int32 [F, k, 4] (the bits of mt_object),
    motion int32 [F, k, 16] (the bits of mt_heading: motion.cpu().numpy().view(HEADING_DTYPE)[..., 0] is [F, k]); None
    for an output not in `want`.  d_rec / d_off / d_sd / d_stream_off / d_keep / compact as for objects.scan_device.
    `allowed` is ready for sweep_streams_device: with clusters_needed <= 1, level L there is flags at min_objects = L.
    out: a dict of preallocated tensors by name.  Asynchronous on `stream` (default: torch's current stream)."""
    want = _wanted(want, OUTPUTS)
    if (d_stream_off is None) != (d_keep is None):
        raise ValueError("d_stream_off and d_keep go together: give both or neither")
    n_frames = max(d_off.numel() - 1, 0)
    kk = max(int(k), 0)
    res = {}
    for name in OUTPUTS:
        grid = {"list": (kk, 4), "motion": (kk, HEADING_WORDS)}.get(name, ())
        res.update(_device_outputs((name,), (name,) if name in want else (), out, n_frames, d_off.device, grid=grid))
    if n_frames == 0:              # nothing to write (an empty tensor has no address to hand over)
        return res
    head, st = scanner._device_batch(d_rec, d_off, d_sd, compact, stream)
    ns = scanner._device_keep(d_stream_off, d_keep)
    check(scanner._lib.mtgpu_scan_headings_device(*head, _dptr(d_stream_off), ns, _dptr(d_keep), int(k), int(min_blob_cells),
                                                  int(min_objects), int(allow), *(_dptr(res[n]) for n in OUTPUTS), st))
    return res


def mean_vector(motion) -> np.ndarray:
    """HEADING_DTYPE array -> float64 [..., 2]: (sum_dx, sum_dy) / records, the mean displacement of an entry's belonging
    records in pixels per frame; (0, 0) where records is 0."""
    mo = np.asarray(motion)
    n = mo["records"].astype(np.float64)
    out = np.zeros(mo.shape + (2,), dtype=np.float64)
    np.divide(mo["sum_dx"].astype(np.float64), n, out=out[..., 0], where=n > 0)
    np.divide(mo["sum_dy"].astype(np.float64), n, out=out[..., 1], where=n > 0)
    return out


def heading_histogram(cells, heading, min_blob_cells=1) -> dict:
    """{"E": objects heading E, ..., "NE": ..., "none": objects whose records are all still}, in sector order: over the
    listed entries with at least min_blob_cells cells."""
    c, h = np.asarray(cells).reshape(-1), np.asarray(heading).reshape(-1)
    obj = c >= max(1, int(min_blob_cells))
    out = {name: int((obj & (h == s)).sum()) for s, name in enumerate(direction.SECTOR_NAMES)}
    out["none"] = int((obj & (h == NO_HEADING)).sum())
    return out


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.headings", description=__doc__.splitlines()[2])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    ap.add_argument("--top", type=_top, metavar="K", default=OBJECTS_MAX, help=f"list entries per frame, 1 .. {OBJECTS_MAX} (default {OBJECTS_MAX})")
    ap.add_argument("--min-blob-cells", type=_cells, metavar="N", default=1, help="an object is a blob of at least N cells (default 1)")
    ap.add_argument("--min-objects", type=_levels, metavar="L[,L...]", default=list(DEFAULT_LEVELS),
                    help="the levels: least counts of allowed objects of a frame, each at most K (default 1,2,3)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--allow", type=direction._names("--allow"), metavar="E,NE,...", help="the headings an object may have")
    g.add_argument("--ignore", type=direction._names("--ignore"), metavar="W,...", help="the headings an object may not have")
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


def allow_of(args) -> int:
    """The allow byte of parsed options: --allow's, the complement of --ignore's, or every sector."""
    if args.allow is not None:
        return args.allow
    if args.ignore is not None:
        return ALL & ~args.ignore
    return ALL


def measure(scanner, batch, pts, levels, merge_params, allow=ALL, k=OBJECTS_MAX, min_blob_cells=1, keep=None):
    """One heading scan per byte (every sector, then `allow`), then the sweep on `allowed` of each.  keep: bool [gh, gw]
    or None.  Returns a dict."""
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
    tables = {}
    with torch.cuda.device(dev):
        d_keep = None
        if keep is not None:
            d_keep = torch.from_numpy(zones.pack_keep(keep).view(np.int64).copy()).reshape(1, p.grid_h, -1).to(dev)
        for name, byte in (("all", ALL), ("allow", int(allow))):
            res = scan_device(scanner, d_rec, d_off, d_sd, k, min_blob_cells, 1, byte, d_soff if keep is not None else None, d_keep,
                              want=("centres", "list", "motion", "allowed"))
            swept = scanner.sweep_streams_device(res["allowed"], d_pts, d_soff, d_mp, levels, seg_cap=1)
            torch.cuda.synchronize(dev)
            allowed = res["allowed"].cpu().numpy().view(np.uint32)
            rows = []
            for i, lv in enumerate(levels):
                r = results_from_bytes(swept[1][i].cpu().numpy())[0]
                if int(r["status"]) != _abi.MT_OK:
                    raise _abi.MtgpuError(int(r["status"]), "timestamps contain NaN")
                rows.append({"level": int(lv), "motion_frames": int((allowed >= lv).sum()), "frames_kept": int(r["n_timestamps"]),
                             "segments": int(r["n_segments"]), "seconds_kept": float(merge_params.duration) - float(r["time_removed"]),
                             "saved_pct": float(r["saved_pct"]), "do_cut": int(r["do_cut"])})
            tables[name] = rows
    listed = res["list"].cpu().numpy().reshape(n, k, 4).view(OBJECT_DTYPE)[..., 0]
    motion = res["motion"].cpu().numpy().reshape(n, k, HEADING_WORDS).view(HEADING_DTYPE)[..., 0]
    return {"allow": direction.names_from_allow(allow), "levels_all": tables["all"], "levels_allow": tables["allow"],
            "headings": heading_histogram(listed["cells"], motion["heading"], min_blob_cells),
            "records": int(motion["records"].sum(dtype=np.uint64)),
            "centres": int(res["centres"].cpu().numpy().view(np.uint32).sum(dtype=np.uint64))}


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad option: nothing below has run, no device has been touched
    if max(a.min_objects) > a.top:
        ap.error(f"--min-objects: level {max(a.min_objects)} is above --top {a.top}: only listed objects have a heading")
    try:
        path = a.file
        batch, pts, hdr = tune.load(path)
        path = a.keep
        keep = None if path is None else zones.load_keep(path)
    except (OSError, ValueError, KeyError) as e:
        print(f"headings: cannot read {path}: {e}", file=sys.stderr)
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
            res = measure(s, batch, pts, a.min_objects, mp, allow_of(a), a.top, a.min_blob_cells, keep)
    except _abi.MtgpuError as e:
        print(f"headings: {e}", file=sys.stderr)
        return 1
    if a.json:
        print(json.dumps({"file": a.file, "width": width, "height": height, "grid_w": params.grid_w, "grid_h": params.grid_h,
                          "frames": batch.n_frames, "keep": a.keep, "top": a.top, "min_blob_cells": a.min_blob_cells, **res}))
        return 0
    print(f"# grid {params.grid_w} x {params.grid_h}, {batch.n_frames} frames, {res['centres']} centres, {res['records']} records in "
          f"listed objects; an object has at least {a.min_blob_cells} cells")
    for title, rows in (("all", res["levels_all"]), (res["allow"], res["levels_allow"])):
        print(f"headings allowed: {title}")
        print("MIN_OBJECTS motion_frames frames_kept segments seconds_kept saved_pct do_cut")
        for r in rows:
            print("%-11d %-13d %-11d %-8d %-12.2f %-9.2f %d" % (r["level"], r["motion_frames"], r["frames_kept"], r["segments"],
                                                               r["seconds_kept"], r["saved_pct"], r["do_cut"]))
    print(f"object headings (top {a.top}): " + "  ".join(f"{k}: {v}" for k, v in res["headings"].items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
