"""`python -m mvtrim_amd.persist FILE [--min-run 1,2,3,5] [--max-dropout N] [--blobs [--min-blob-cells N] [--reach R]] [--keep MASK.mtkeep] [--json]`

Temporal persistence: what a minimum number of consecutive motion frames keeps of one recording.  Every rule of the scan
is a rule about ONE frame, and the reference pools every frame that passes it (src/motion_scanner.cpp:382-383): one
headlight sweep or one insect on the lens costs a segment of 2 x PADDING_SEC.  MIN_RUN = L keeps a motion frame iff it
belongs to a run of at least L motion frames; key frames, which are never analysed, do not end a run, and --max-dropout
quiet frames between two motion frames do not either.  FILE is the JSON that tools/extract_mvs.cpp prints (mvjson.py)
or a `.mtmv` container (mvfile.py), loaded as `tune` loads it.

One scan — the centre scan, or with --blobs the blob scan (MotionScanner.scan_blobs_device), whose boxes then link the
frames: a run goes on only while the largest blob stays within --reach cells of where it was — then ONE persistence pass
(MotionScanner.persist_device) returns every frame's run length, and the existing sweep (sweep_streams_device) merges
once per level on `run`: per level the frames kept, the segments and the seconds kept.  The row of --min-run 1 is
today's answer and is always printed.  Last comes a histogram of the run lengths, one count per run.
--keep MASK.mtkeep applies ignore zones (zones.save_keep / `zones --save-mask`) to the scan.  --min-blob-cells and
--reach need --blobs.

Width, height and duration come from a `.mtmv` header or from --width / --height / --duration.  Everything is computed
by libmtgpu; without a usable device the command fails, there is no CPU path.
"""
import argparse
import json
import sys

import numpy as np

from . import _abi, tune, zones
from .scanner import MergeParams, MotionScanner, ScanParams, results_from_bytes

MAX_LEVELS = _abi.SWEEP_MAX_LEVELS
DEFAULT_LEVELS = (1, 2, 3, 5)
HIST_EDGES = (1, 2, 3, 5, 10, 30, 100)      # the histogram's bins start here; the last one is open


def _levels(text):
    try:
        v = [int(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--min-run: {text!r} is not a comma-separated list of whole numbers")
    if not 1 <= len(v) <= MAX_LEVELS - 1:
        raise argparse.ArgumentTypeError(f"--min-run: {len(v)} levels, want 1 .. {MAX_LEVELS - 1}")
    if any(not 1 <= x < 2 ** 31 for x in v):
        raise argparse.ArgumentTypeError(f"--min-run: {text!r}: a level is at least 1 and fits int32")
    if len(set(v)) != len(v):
        raise argparse.ArgumentTypeError(f"--min-run: {text!r} names a level twice")
    return v


def _u32(name):
    def parse(text):
        try:
            v = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f"{name}: {text!r} is not a whole number")
        if not 0 <= v <= 0xFFFFFFFF:
            raise argparse.ArgumentTypeError(f"{name}: {v} outside 0 .. 4294967295")
        return v
    return parse


def _reach(text):
    v = _u32("--reach")(text)
    if v > 65535:
        raise argparse.ArgumentTypeError(f"--reach: {v} outside 0 .. 65535")
    return v


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.persist", description=__doc__.splitlines()[2])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    ap.add_argument("--min-run", type=_levels, metavar="L[,L...]", default=list(DEFAULT_LEVELS),
                    help="the levels: least motion frames in a frame's run (default 1,2,3,5; 1 is always reported)")
    ap.add_argument("--max-dropout", type=_u32("--max-dropout"), metavar="N", default=0,
                    help="analysed quiet frames between two motion frames that do not end a run (default 0)")
    ap.add_argument("--blobs", action="store_true",
                    help="scan with the blob scan: the boxes of the largest blobs link the frames of a run")
    ap.add_argument("--min-blob-cells", type=int, metavar="N", help="with --blobs: least cells of a frame's largest blob (default 1)")
    ap.add_argument("--reach", type=_reach, metavar="R", help="with --blobs: cells two consecutive boxes may lie apart (default 1)")
    ap.add_argument("--keep", metavar="MASK.mtkeep", help="ignore zones: a .mtkeep text mask, 1 = analysed")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--duration", type=float, help="seconds")
    ap.add_argument("--block-size", type=int)
    ap.add_argument("--block-shift", type=int)
    ap.add_argument("--vectors-needed", type=int)
    ap.add_argument("--clusters-needed", type=int)
    ap.add_argument("--mv-threshold-sq", type=float)
    ap.add_argument("--vertical-mask", type=float)
    ap.add_argument("--max-gap-sec", type=float)
    ap.add_argument("--padding-sec", type=float)
    ap.add_argument("--min-savings-pct", type=float)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", action="store_true", help="one JSON document instead of the table")
    return ap


def levels_with_one(levels):
    """The levels in the caller's order, with 1 — today's answer — in front when it is not among them."""
    levels = [int(v) for v in levels]
    return levels if 1 in levels else [1] + levels


def histogram(run, pos):
    """Run lengths, one count per run (taken from `run` at pos == 1): {"1": runs of one frame, "2": ..., "3-4": ...,
    "100+": ...}, in that order."""
    lengths = np.asarray(run).astype(np.int64)[np.asarray(pos) == 1]
    out = {}
    for i, lo in enumerate(HIST_EDGES):
        hi = HIST_EDGES[i + 1] - 1 if i + 1 < len(HIST_EDGES) else None
        label = f"{lo}+" if hi is None else str(lo) if hi == lo else f"{lo}-{hi}"
        out[label] = int(((lengths >= lo) & ((lengths <= hi) if hi is not None else True)).sum())
    return out


def measure(scanner, batch, pts, levels, merge_params, max_dropout=0, blob_settings=None, keep=None):
    """One scan, one persistence pass, then the sweep on `run`.  blob_settings: (min_blob_cells, reach) — the scan is then
    the blob scan and its boxes link the frames — or None: the centre scan.  keep: bool [gh, gw] or None.  Returns a
    dict."""
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
        d_box, reach = None, 0
        if blob_settings is not None:
            res = scanner.scan_blobs_device(d_rec, d_off, d_sd, blob_settings[0], d_soff if keep is not None else None, d_keep,
                                            want=("flags", "box"))
            d_flags, d_box, reach = res["flags"], res["box"], blob_settings[1]
        elif keep is not None:
            d_flags, _, _ = scanner.scan_zones_device(d_rec, d_off, d_sd, d_soff, d_keep, centres=False)
        else:
            d_flags, _ = scanner.count_centres_device(d_rec, d_off, d_sd)
        per = scanner.persist_device(d_flags, d_soff, d_sd, d_box, 1, max_dropout, reach, want=("run", "pos"))
        _seg, r8 = scanner.sweep_streams_device(per["run"], d_pts, d_soff, d_mp, levels, seg_cap=1)
        torch.cuda.synchronize(dev)
    run = per["run"].cpu().numpy().view(np.uint32)
    pos = per["pos"].cpu().numpy().view(np.uint32)
    rows = []
    for i, lv in enumerate(levels):
        r = results_from_bytes(r8[i].cpu().numpy())[0]
        if int(r["status"]) != _abi.MT_OK:
            raise _abi.MtgpuError(int(r["status"]), "timestamps contain NaN")
        removed = float(r["time_removed"]) if int(r["n_segments"]) else float(merge_params.duration)
        rows.append({"min_run": int(lv), "motion_frames": int((run >= lv).sum()), "frames_kept": int(r["n_timestamps"]),
                     "segments": int(r["n_segments"]), "seconds_kept": float(merge_params.duration) - removed,
                     "saved_pct": float(r["saved_pct"]), "do_cut": int(r["do_cut"])})
    return {"levels": rows, "runs": int((pos == 1).sum()), "longest_run": int(run.max()) if n else 0, "run_lengths": histogram(run, pos)}


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad option: nothing below has run, no device has been touched
    if not a.blobs and (a.min_blob_cells is not None or a.reach is not None):
        ap.error("--min-blob-cells and --reach belong to --blobs")
    if a.min_blob_cells is not None and a.min_blob_cells < 1:
        ap.error("--min-blob-cells: at least 1")
    settings = (1 if a.min_blob_cells is None else a.min_blob_cells, 1 if a.reach is None else a.reach) if a.blobs else None
    try:
        path = a.file
        batch, pts, hdr = tune.load(path)
        path = a.keep
        keep = None if path is None else zones.load_keep(path)
    except (OSError, ValueError, KeyError) as e:
        print(f"persist: cannot read {path}: {e}", file=sys.stderr)
        return 1
    width = a.width if a.width is not None else hdr.get("width")
    height = a.height if a.height is not None else hdr.get("height")
    duration = a.duration if a.duration is not None else hdr.get("duration")
    if width is None or height is None or duration is None:
        ap.error("the file carries no width / height / duration: give --width, --height and --duration")
    params = ScanParams.from_config(width, height, block_size=a.block_size, block_shift=a.block_shift,
                                    vectors_needed=a.vectors_needed, mv_threshold_sq=a.mv_threshold_sq,
                                    clusters_needed=a.clusters_needed, vertical_mask=a.vertical_mask)
    if keep is not None and keep.shape != (params.grid_h, params.grid_w):
        ap.error(f"--keep: the mask is for a {keep.shape[1]}x{keep.shape[0]} grid, this one is {params.grid_w}x{params.grid_h}")
    mp = MergeParams(duration=float(duration), max_gap_sec=a.max_gap_sec, padding_sec=a.padding_sec,
                     min_savings_pct=a.min_savings_pct)
    try:
        with MotionScanner(params, device=a.device) as s:
            res = measure(s, batch, pts, a.min_run, mp, a.max_dropout, settings, keep)
    except _abi.MtgpuError as e:
        print(f"persist: {e}", file=sys.stderr)
        return 1
    if a.json:
        doc = {"file": a.file, "width": width, "height": height, "grid_w": params.grid_w, "grid_h": params.grid_h,
               "frames": batch.n_frames, "keep": a.keep, "max_dropout": a.max_dropout, "blobs": bool(a.blobs)}
        if settings is not None:
            doc.update({"min_blob_cells": settings[0], "reach": settings[1]})
        print(json.dumps({**doc, **res}))
        return 0
    print(f"# grid {params.grid_w} x {params.grid_h}, {batch.n_frames} frames, {res['runs']} runs; the longest has "
          f"{res['longest_run']} motion frames; max_dropout {a.max_dropout}" +
          (f"; blob scan, min_blob_cells {settings[0]}, reach {settings[1]}" if settings is not None else "; centre scan"))
    print("min_run motion_frames frames_kept segments seconds_kept saved_pct do_cut")
    for r in res["levels"]:
        print("%-7d %-13d %-11d %-8d %-12.2f %-9.2f %d" % (r["min_run"], r["motion_frames"], r["frames_kept"], r["segments"],
                                                         r["seconds_kept"], r["saved_pct"], r["do_cut"]))
    print("run lengths: " + "  ".join(f"{k}: {v}" for k, v in res["run_lengths"].items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
