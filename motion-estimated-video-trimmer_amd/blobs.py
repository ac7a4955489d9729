"""`python -m mvtrim_amd.blobs FILE [--min-blob-cells 1,2,4,8] [--keep MASK.mtkeep] [--gmc [--max-shift N] [--min-share S]] [--json]`

Motion blobs: what a minimum object size keeps of one recording.  The reference counts a "cluster" per cell — an active
cell with an active 4-neighbour (src/motion_scanner.cpp:272-294) — so CLUSTERS_NEEDED = 8 cannot tell one object of
eight cells from four unrelated pairs of rain, foliage or compression noise.  A blob is a 4-connected component of a
frame's centre cells; MIN_BLOB_CELLS = L keeps a frame iff its LARGEST blob has at least L cells.  FILE is the JSON that
tools/extract_mvs.cpp prints (mvjson.py) or a `.mtmv` container (mvfile.py), loaded as `tune` loads it.

One blob scan (MotionScanner.scan_blobs_device) returns every frame's centre count, blob count and largest blob; the
existing sweep (sweep_streams_device) then merges once per level on `largest` and once per level on `centres`: per
level the frames kept and the segments under the object-size rule, and beside them the row of CLUSTERS_NEEDED at the
same level, so that one sees what the object-size rule removes that the cell-count rule keeps.  The scan itself runs
with CLUSTERS_NEEDED 1: a level is the only bar a frame has to pass.  Last comes a histogram of blobs per frame.
--keep MASK.mtkeep applies ignore zones (zones.save_keep / `zones --save-mask`) to the scan.
--gmc runs every row on the compensated blob scan (MotionScanner.scan_gmc_blobs_device): each frame's dominant vector is
estimated — under --keep, from the records in kept cells — and subtracted first, so the blobs are those of the residual
motion; one more line gives the share of compensated frames and the most frequent applied vectors, as `gmc` prints
them.  --max-shift and --min-share are `gmc`'s and need --gmc.

Width, height and duration come from a `.mtmv` header or from --width / --height / --duration.  Everything is computed
by libmtgpu; without a usable device the command fails, there is no CPU path.
"""
import argparse
import json
import sys

import numpy as np

from . import _abi, gmc, tune, zones
from .scanner import MergeParams, MotionScanner, ScanParams, results_from_bytes

MAX_LEVELS = _abi.SWEEP_MAX_LEVELS
DEFAULT_LEVELS = (1, 2, 4, 8)
HIST_LAST = 9                      # the histogram's last bin: HIST_LAST blobs or more


def _levels(text):
    try:
        v = [int(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--min-blob-cells: {text!r} is not a comma-separated list of whole numbers")
    if not 1 <= len(v) <= MAX_LEVELS:
        raise argparse.ArgumentTypeError(f"--min-blob-cells: {len(v)} levels, want 1 .. {MAX_LEVELS}")
    if any(not 1 <= x < 2 ** 31 for x in v):
        raise argparse.ArgumentTypeError(f"--min-blob-cells: {text!r}: a level is at least 1 and fits int32")
    if len(set(v)) != len(v):
        raise argparse.ArgumentTypeError(f"--min-blob-cells: {text!r} names a level twice")
    return v


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.blobs", description=__doc__.splitlines()[2])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    ap.add_argument("--min-blob-cells", type=_levels, metavar="L[,L...]", default=list(DEFAULT_LEVELS),
                    help="the levels: least cell counts of a frame's largest blob (default 1,2,4,8)")
    ap.add_argument("--keep", metavar="MASK.mtkeep", help="ignore zones: a .mtkeep text mask, 1 = analysed")
    ap.add_argument("--gmc", action="store_true",
                    help="blobs of the residual motion: every row comes from the compensated blob scan (scan_gmc_blobs_device)")
    ap.add_argument("--max-shift", type=gmc._max_shift, metavar="N",
                    help=f"with --gmc: largest displacement per axis the estimate looks at, 0 .. 127 (default {_abi.GMC_DEFAULT_MAX_SHIFT})")
    ap.add_argument("--min-share", type=gmc._min_share, metavar="S",
                    help="with --gmc: share of the analysed records that must agree on a mode, 0 .. 1 "
                         f"(default {_abi.GMC_DEFAULT_MIN_SHARE_Q8 / 256.0})")
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


def histogram(blobs):
    """{"0": frames without a blob, "1": ..., "9+": frames with HIST_LAST blobs or more}, in that order."""
    b = np.minimum(np.asarray(blobs).astype(np.int64), HIST_LAST)
    counts = np.bincount(b, minlength=HIST_LAST + 1)
    return {(str(i) if i < HIST_LAST else f"{HIST_LAST}+"): int(counts[i]) for i in range(HIST_LAST + 1)}


def measure(scanner, batch, pts, levels, merge_params, keep=None, gmc_settings=None):
    """One blob scan, then the sweep on `largest` and on `centres`.  keep: bool [gh, gw] or None.  gmc_settings:
    (max_shift, min_share_q8) — the scan is then the compensated blob scan, and the dict also carries `compensated_share`
    (of the frames with side data) and `vectors`: [[gx, gy, frames]], most frequent first, as gmc.measure reports them —
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
    with torch.cuda.device(dev):
        d_keep = None
        if keep is not None:
            d_keep = torch.from_numpy(zones.pack_keep(keep).view(np.int64).copy()).reshape(1, p.grid_h, -1).to(dev)
        if gmc_settings is None:
            res = scanner.scan_blobs_device(d_rec, d_off, d_sd, 1, d_soff if keep is not None else None, d_keep,
                                            want=("centres", "blobs", "largest"))
        else:
            res = scanner.scan_gmc_blobs_device(d_rec, d_off, d_sd, gmc_settings[0], gmc_settings[1], 1,
                                                d_soff if keep is not None else None, d_keep,
                                                want=("centres", "blobs", "largest", "info"))
        by_blob = scanner.sweep_streams_device(res["largest"], d_pts, d_soff, d_mp, levels, seg_cap=1)
        by_cell = scanner.sweep_streams_device(res["centres"], d_pts, d_soff, d_mp, levels, seg_cap=1)
        torch.cuda.synchronize(dev)
    largest = res["largest"].cpu().numpy().view(np.uint32)
    centres = res["centres"].cpu().numpy().view(np.uint32)
    rows = []
    for i, lv in enumerate(levels):
        row = {"level": int(lv)}
        for name, (_seg, r8), counts in (("min_blob_cells", by_blob, largest), ("clusters_needed", by_cell, centres)):
            r = results_from_bytes(r8[i].cpu().numpy())[0]
            if int(r["status"]) != _abi.MT_OK:
                raise _abi.MtgpuError(int(r["status"]), "timestamps contain NaN")
            row[name] = {"motion_frames": int((counts >= lv).sum()), "frames_kept": int(r["n_timestamps"]),
                         "segments": int(r["n_segments"]), "saved_pct": float(r["saved_pct"]), "do_cut": int(r["do_cut"])}
        rows.append(row)
    out = {"levels": rows, "blobs_per_frame": histogram(res["blobs"].cpu().numpy().view(np.uint32)),
           "largest_blob": int(largest.max()) if n else 0, "centres": int(centres.sum(dtype=np.uint64))}
    if gmc_settings is not None:
        inf = res["info"].cpu().numpy().reshape(-1).view(_abi.GMC_INFO_DTYPE)
        has = np.diff(np.asarray(batch.frame_off).astype(np.int64)) > 0 if batch.has_sd is None else np.asarray(batch.has_sd) != 0
        moved = (inf["gx"] != 0) | (inf["gy"] != 0)
        out["compensated_share"] = float(moved.sum()) / float(has.sum()) if has.any() else 0.0
        vec, cnt = np.unique(np.stack([inf["gx"][has], inf["gy"][has]], axis=1), axis=0, return_counts=True) if has.any() else ([], [])
        order = sorted(range(len(cnt)), key=lambda i: (-int(cnt[i]), abs(int(vec[i][0])) + abs(int(vec[i][1])), tuple(vec[i])))
        out["vectors"] = [[int(vec[i][0]), int(vec[i][1]), int(cnt[i])] for i in order[:gmc.TOP_VECTORS]]
    return out


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad option: nothing below has run, no device has been touched
    if not a.gmc and (a.max_shift is not None or a.min_share is not None):
        ap.error("--max-shift and --min-share belong to --gmc")
    settings = None
    if a.gmc:
        settings = (_abi.GMC_DEFAULT_MAX_SHIFT if a.max_shift is None else a.max_shift,
                    _abi.GMC_DEFAULT_MIN_SHARE_Q8 if a.min_share is None else gmc.share_q8(a.min_share))
    try:
        path = a.file
        batch, pts, hdr = tune.load(path)
        path = a.keep
        keep = None if path is None else zones.load_keep(path)
    except (OSError, ValueError, KeyError) as e:
        print(f"blobs: cannot read {path}: {e}", file=sys.stderr)
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
            res = measure(s, batch, pts, a.min_blob_cells, mp, keep, settings)
    except _abi.MtgpuError as e:
        print(f"blobs: {e}", file=sys.stderr)
        return 1
    if a.json:
        doc = {"file": a.file, "width": width, "height": height, "grid_w": params.grid_w, "grid_h": params.grid_h,
               "frames": batch.n_frames, "keep": a.keep}
        if settings is not None:
            doc.update({"max_shift": settings[0], "min_share_q8": settings[1]})
        print(json.dumps({**doc, **res}))
        return 0
    print(f"# grid {params.grid_w} x {params.grid_h}, {batch.n_frames} frames, {res['centres']} centres; the largest blob has "
          f"{res['largest_blob']} cells")
    if settings is not None:
        print(f"# gmc: max_shift {settings[0]}, min_share {settings[1]}/256; {100.0 * res['compensated_share']:.2f}% of the frames with "
              "side data have a non-zero applied vector; most frequent: " +
              "  ".join("(%d, %d): %d" % (gx, gy, cnt) for gx, gy, cnt in res["vectors"]))
    print("level rule            motion_frames frames_kept segments saved_pct do_cut")
    for row in res["levels"]:
        for name, label in (("min_blob_cells", "MIN_BLOB_CELLS"), ("clusters_needed", "CLUSTERS_NEEDED")):
            r = row[name]
            print("%-5d %-15s %-13d %-11d %-8d %-9.2f %d" % (row["level"], label, r["motion_frames"], r["frames_kept"], r["segments"],
                                                           r["saved_pct"], r["do_cut"]))
    print("blobs per frame: " + "  ".join(f"{k}: {v}" for k, v in res["blobs_per_frame"].items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
