"""`python -m mvtrim_amd.zones FILE [--ignore X0,Y0,X1,Y1]... [--ignore-busy SHARE] [--mask-npy PATH] [--mask PATH.mtkeep] [--save-mask PATH] [--json]`

Ignore zones: what the trimmer keeps of one recording when some grid cells are not analysed.  The reference can only
mask full-width strips (VERTICAL_MASK, src/motion_scanner.cpp:237-238, 262); a keep mask removes single cells — a
burnt-in clock, a road at one side, a neighbour's window.  FILE is the JSON that tools/extract_mvs.cpp prints
(mvjson.py) or a `.mtmv` container (mvfile.py), loaded as `tune` loads it.

The mask is the intersection of what the options give: --ignore rectangles (pixels by default, see --unit; a rectangle
ignores every cell its blocks intersect), --ignore-busy SHARE (one activity map first: every cell that was a centre in
more than SHARE of the frames with side data is ignored), --mask-npy (a [grid_h, grid_w] array, non-zero = keep) and
--mask (a `.mtkeep` text file).  --save-mask PATH.mtkeep writes the mask used in the form `mtgpu_scan_file --keep` and
ScanPipe.set_keep(load_keep(PATH)) take: `zones --ignore-busy 0.5 --save-mask cam3.mtkeep`, then
`mtgpu_scan_file --keep cam3.mtkeep` trims with it.
One masked scan (MotionScanner.scan_zones_device) returns every frame's centre count with and without the zones from one
read of the records; the existing merge runs on both.  Printed: frames kept and segments without and with the zones,
and the ignored share of the analysed cells.

Width, height and duration come from a `.mtmv` header or from --width / --height / --duration.  Everything but the mask
arithmetic is computed by libmtgpu; without a usable device the command fails, there is no CPU path.

The helpers below (pack_keep, unpack_keep, save_keep, load_keep, keep_from_rects, keep_from_activity) are pure numpy.
"""
import argparse
import json
import math
import sys

import numpy as np

from . import _abi, tune
from .scanner import MergeParams, MotionScanner, ScanParams, results_from_bytes

UNITS = ("px", "frac", "cell")
MAX_RECTS = 256


# ------------------------------------------------------------------ the mask (numpy only)

def pack_keep(keep):
    """bool [gh, gw] (True = analysed) -> uint64 [gh, W], W = (gw + 63) // 64: cell (x, y) is bit x & 63 of word x >> 6 of
    row y (include/mtgpu_zones.h).  Bits at x >= gw are 0."""
    keep = np.asarray(keep)
    if keep.ndim != 2:
        raise ValueError(f"keep has {keep.ndim} dimensions, want [grid_h, grid_w]")
    gh, gw = keep.shape
    W = (gw + 63) // 64
    bits = np.zeros((gh, W * 64), dtype=np.uint64)
    bits[:, :gw] = keep != 0
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return np.ascontiguousarray((bits.reshape(gh, W, 64) * weights).sum(axis=2, dtype=np.uint64))


def unpack_keep(words, gw):
    """uint64 [gh, W] -> bool [gh, gw]; bits at x >= gw are dropped."""
    words = np.asarray(words, dtype=np.uint64)
    if words.ndim != 2 or words.shape[1] != (gw + 63) // 64:
        raise ValueError(f"words has shape {words.shape}, want [grid_h, {(gw + 63) // 64}]")
    x = np.arange(gw)
    return ((words[:, x >> 6] >> (x & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


MTKEEP_MAGIC = "mtkeep 1"


def save_keep(path, keep):
    """Write a bool [grid_h, grid_w] mask (True = analysed) as a `.mtkeep` text file: line 1 `mtkeep 1`, line 2
    `<grid_w> <grid_h>`, then grid_h lines of grid_w characters, `1` analysed, `0` ignored.  What mtgpu_scan_file --keep
    and load_keep read; plain text, so that a mask can be edited by hand."""
    keep = np.asarray(keep)
    if keep.ndim != 2 or keep.shape[0] < 1 or keep.shape[1] < 1:
        raise ValueError(f"keep has shape {keep.shape}, want [grid_h, grid_w]")
    gh, gw = keep.shape
    rows = ["".join("1" if v else "0" for v in row) for row in (keep != 0)]
    with open(path, "w", encoding="ascii", newline="\n") as f:
        f.write(f"{MTKEEP_MAGIC}\n{gw} {gh}\n" + "\n".join(rows) + "\n")


def load_keep(path, grid=None):
    """Read a `.mtkeep` file -> bool [grid_h, grid_w].  grid: (grid_w, grid_h) the file must match, or None.  ValueError
    names the line of anything else: another first line, a grid that does not match, a short file, a row of another
    length, a character other than 0 / 1, lines behind the last row."""
    with open(path, "r", encoding="ascii", errors="replace", newline="") as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()                                        # the final newline
    lines = [ln[:-1] if ln.endswith("\r") else ln for ln in lines]
    if not lines or lines[0] != MTKEEP_MAGIC:
        raise ValueError(f"{path}: line 1: want '{MTKEEP_MAGIC}'")
    dims = lines[1].split(" ") if len(lines) > 1 else []
    if len(dims) != 2 or not all(d.isascii() and d.isdigit() and len(d) <= 6 for d in dims) or int(dims[0]) < 1 or int(dims[1]) < 1:
        raise ValueError(f"{path}: line 2: want '<grid_w> <grid_h>'")
    gw, gh = int(dims[0]), int(dims[1])
    if grid is not None and (gw, gh) != (int(grid[0]), int(grid[1])):
        raise ValueError(f"{path}: line 2: the mask is for a {gw}x{gh} grid, this one is {int(grid[0])}x{int(grid[1])}")
    keep = np.zeros((gh, gw), dtype=bool)
    for y in range(gh):
        n = 3 + y
        if n > len(lines):
            raise ValueError(f"{path}: line {n}: the file ends after {y} of {gh} rows")
        row = lines[n - 1]
        if len(row) != gw:
            raise ValueError(f"{path}: line {n}: {len(row)} characters, want {gw}")
        for x, ch in enumerate(row):
            if ch not in "01":
                raise ValueError(f"{path}: line {n}: character {x + 1} is neither 0 nor 1")
        keep[y] = np.frombuffer(row.encode("ascii"), dtype=np.uint8) == ord("1")
    if len(lines) > 2 + gh:
        raise ValueError(f"{path}: line {3 + gh}: text behind the last of {gh} rows")
    return keep


def keep_from_rects(params, rects, unit="px", size=None):
    """bool [grid_h, grid_w], True = analysed: everything but the rectangles.  rects: (x0, y0, x1, y1), half-open
    [x0, x1) x [y0, y1).
      unit "px"    pixels: the rectangle ignores every cell its blocks intersect, columns x0 >> shift .. (x1 - 1) >> shift
                   and the rows likewise (src/motion_scanner.cpp:255-256 maps a pixel to its cell the same way)
      unit "frac"  fractions of the picture, `size` = (width, height) in pixels (default: the grid's extent, grid << shift):
                   pixels floor(x0 * width) .. ceil(x1 * width), then as "px"
      unit "cell"  grid cells [x0, x1) x [y0, y1)
    An empty rectangle ignores nothing; a rectangle is clipped to the grid."""
    if unit not in UNITS:
        raise ValueError(f"unit {unit!r} is not one of {UNITS}")
    gw, gh, sh = params.grid_w, params.grid_h, params.block_shift
    keep = np.ones((gh, gw), dtype=bool)
    pw, ph = (gw << sh, gh << sh) if size is None else (int(size[0]), int(size[1]))
    for r in rects:
        x0, y0, x1, y1 = r
        if unit == "frac":
            for v in r:
                if not (math.isfinite(v) and 0.0 <= v <= 1.0):
                    raise ValueError(f"fraction {v!r} is not in [0, 1]")
            x0, y0, x1, y1 = math.floor(x0 * pw), math.floor(y0 * ph), math.ceil(x1 * pw), math.ceil(y1 * ph)
        else:
            for v in r:
                if int(v) != v:
                    raise ValueError(f"{unit} coordinate {v!r} is not an integer")
            x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
        if x1 <= x0 or y1 <= y0:
            continue
        if unit != "cell":                  # first cell .. one past the last cell
            x0, y0, x1, y1 = x0 >> sh, y0 >> sh, ((x1 - 1) >> sh) + 1, ((y1 - 1) >> sh) + 1
        keep[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = False
    return keep


def keep_from_activity(centre_map, frames, share):
    """bool [grid_h, grid_w], True = analysed: a cell is ignored iff it was a centre in MORE than share * frames of the
    `frames` contributing frames of an activity map (MotionScanner.activity_map: centre [gh, gw], frames).  share 1:
    nothing is ignored (a cell is a centre at most once per frame); share 0: every cell that ever was a centre; a cell
    exactly at share * frames is kept."""
    share = float(share)
    if not (math.isfinite(share) and 0.0 <= share <= 1.0):
        raise ValueError(f"share {share!r} is not in [0, 1]")
    centre_map = np.asarray(centre_map)
    if centre_map.ndim != 2:
        raise ValueError(f"centre_map has {centre_map.ndim} dimensions, want [grid_h, grid_w]")
    return ~(centre_map.astype(np.float64) > share * float(int(frames)))


def ignored_share(keep, margin):
    """The share of the analysed cells (rows [margin, gh - margin), every column) that the mask ignores."""
    gh = keep.shape[0]
    rows = keep[min(margin, gh):max(gh - margin, min(margin, gh))]
    return float((~rows).sum()) / rows.size if rows.size else 0.0


# ------------------------------------------------------------------ the command

def _rect(text):
    try:
        v = [float(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--ignore: {text!r} is not X0,Y0,X1,Y1")
    if len(v) != 4 or not all(math.isfinite(x) for x in v):
        raise argparse.ArgumentTypeError(f"--ignore: {text!r} is not four finite numbers X0,Y0,X1,Y1")
    if v[0] < 0 or v[1] < 0 or v[2] < v[0] or v[3] < v[1]:
        raise argparse.ArgumentTypeError(f"--ignore: {text!r}: want 0 <= X0 <= X1 and 0 <= Y0 <= Y1")
    return tuple(v)


def _share(text):
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--ignore-busy: {text!r} is not a number")
    if not text.strip() or not math.isfinite(v) or not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError(f"--ignore-busy: {text!r} is not in [0, 1]")
    return v


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.zones", description=__doc__.splitlines()[2])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    ap.add_argument("--ignore", action="append", type=_rect, metavar="X0,Y0,X1,Y1", default=[],
                    help="ignore the rectangle [X0, X1) x [Y0, Y1) (may be given several times)")
    ap.add_argument("--unit", choices=UNITS, default="px", help="unit of --ignore: pixels (default), fractions of the picture, grid cells")
    ap.add_argument("--ignore-busy", type=_share, metavar="SHARE",
                    help="ignore every cell that is a centre in more than SHARE of the frames with side data (one activity map first)")
    ap.add_argument("--mask-npy", metavar="PATH", help="a [grid_h, grid_w] array, non-zero = keep")
    ap.add_argument("--mask", metavar="PATH.mtkeep", help="a .mtkeep text mask (save_keep / --save-mask), 1 = keep")
    ap.add_argument("--save-mask", metavar="PATH", help="write the mask used: a .mtkeep text file when PATH ends in .mtkeep "
                    "(what mtgpu_scan_file --keep reads), else a bool [grid_h, grid_w] .npy")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--duration", type=float, help="seconds")
    ap.add_argument("--block-size", type=int)
    ap.add_argument("--block-shift", type=int)
    ap.add_argument("--vectors-needed", type=int)
    ap.add_argument("--mv-threshold-sq", type=float)
    ap.add_argument("--clusters-needed", type=int)
    ap.add_argument("--vertical-mask", type=float)
    ap.add_argument("--max-gap-sec", type=float)
    ap.add_argument("--padding-sec", type=float)
    ap.add_argument("--min-savings-pct", type=float)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", action="store_true", help="one JSON document instead of the table")
    return ap


def _check_args(ap, a):
    """Everything the options alone decide; ap.error exits 2."""
    if len(a.ignore) > MAX_RECTS:
        ap.error(f"--ignore: {len(a.ignore)} rectangles, at most {MAX_RECTS}")
    for r in a.ignore:
        if a.unit == "frac":
            if max(r) > 1.0:
                ap.error(f"--ignore: {r} is not inside [0, 1] (--unit frac)")
        elif any(int(v) != v for v in r):
            ap.error(f"--ignore: {r} is not whole numbers (--unit {a.unit})")


def measure(scanner, batch, pts, keep, merge_params, ignore_busy=None):
    """One masked scan with centres_all, then the merge on both.  keep: bool [gh, gw].  Returns (keep used, dict)."""
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
        if ignore_busy is not None:
            _, centre, frames = scanner.activity_map_device(d_rec, d_off, d_sd, d_soff, want=("centre", "frames"))
            torch.cuda.synchronize(dev)
            keep = keep & keep_from_activity(centre[0].cpu().numpy().view(np.uint32),
                                             int(frames.cpu().numpy().view(np.uint32)[0]), ignore_busy)
        d_keep = torch.from_numpy(pack_keep(keep).view(np.int64).copy()).reshape(1, p.grid_h, -1).to(dev)
        flags, centres, call = scanner.scan_zones_device(d_rec, d_off, d_sd, d_soff, d_keep, centres_all=True)
        flags_all = scanner.flags_from_centres(call, p.clusters_needed)
        with_z = scanner.merge_streams_device(flags, d_pts, d_soff, d_mp, seg_cap=1)
        without = scanner.merge_streams_device(flags_all, d_pts, d_soff, d_mp, seg_cap=1)
        torch.cuda.synchronize(dev)
    out = {}
    for name, (_seg, res) in (("without_zones", without), ("with_zones", with_z)):
        r = results_from_bytes(res.cpu().numpy())[0]
        if int(r["status"]) != _abi.MT_OK:
            raise _abi.MtgpuError(int(r["status"]), "timestamps contain NaN")
        out[name] = {"frames_kept": int(r["n_timestamps"]), "segments": int(r["n_segments"]),
                     "saved_pct": float(r["saved_pct"]), "do_cut": int(r["do_cut"])}
    c, ca = centres.cpu().numpy().view(np.uint32), call.cpu().numpy().view(np.uint32)
    out["with_zones"]["centres"] = int(c.sum(dtype=np.uint64))
    out["without_zones"]["centres"] = int(ca.sum(dtype=np.uint64))
    out["with_zones"]["motion_frames"] = int(flags.cpu().numpy().sum())
    out["without_zones"]["motion_frames"] = int(flags_all.cpu().numpy().sum())
    return keep, out


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad option: nothing below has run, no device has been touched
    _check_args(ap, a)
    try:
        path = a.file
        batch, pts, hdr = tune.load(path)
        path = a.mask_npy
        given = None if path is None else np.load(path)
        path = a.mask
        given_text = None if path is None else load_keep(path)
    except (OSError, ValueError, KeyError) as e:
        print(f"zones: cannot read {path}: {e}", file=sys.stderr)
        return 1
    width = a.width if a.width is not None else hdr.get("width")
    height = a.height if a.height is not None else hdr.get("height")
    duration = a.duration if a.duration is not None else hdr.get("duration")
    if width is None or height is None or duration is None:
        ap.error("the file carries no width / height / duration: give --width, --height and --duration")
    params = ScanParams.from_config(width, height, block_size=a.block_size, block_shift=a.block_shift,
                                    vectors_needed=a.vectors_needed, mv_threshold_sq=a.mv_threshold_sq,
                                    clusters_needed=a.clusters_needed, vertical_mask=a.vertical_mask)
    keep = keep_from_rects(params, a.ignore, a.unit, size=(width, height))
    if given is not None:
        if given.shape != keep.shape:
            ap.error(f"--mask-npy: shape {given.shape}, the grid is {keep.shape}")
        keep &= given != 0
    if given_text is not None:
        if given_text.shape != keep.shape:
            ap.error(f"--mask: the mask is for a {given_text.shape[1]}x{given_text.shape[0]} grid, this one is {keep.shape[1]}x{keep.shape[0]}")
        keep &= given_text
    mp = MergeParams(duration=float(duration), max_gap_sec=a.max_gap_sec, padding_sec=a.padding_sec,
                     min_savings_pct=a.min_savings_pct)
    try:
        with MotionScanner(params, device=a.device) as s:
            keep, res = measure(s, batch, pts, keep, mp, a.ignore_busy)
    except _abi.MtgpuError as e:
        print(f"zones: {e}", file=sys.stderr)
        return 1
    if a.save_mask:
        if a.save_mask.endswith(".mtkeep"):
            save_keep(a.save_mask, keep)
        else:
            np.save(a.save_mask, keep)
    share = ignored_share(keep, params.vertical_margin)
    if a.json:
        print(json.dumps({"file": a.file, "width": width, "height": height, "grid_w": params.grid_w, "grid_h": params.grid_h,
                          "frames": batch.n_frames, "ignored_cells": int((~keep).sum()), "ignored_share": share, **res}))
        return 0
    print(f"# grid {params.grid_w} x {params.grid_h}, {batch.n_frames} frames; the zones ignore {100.0 * share:.2f}% of the analysed cells")
    print("zones   motion_frames frames_kept segments saved_pct do_cut centres")
    for name, label in (("without_zones", "without"), ("with_zones", "with")):
        r = res[name]
        print("%-7s %-13d %-11d %-8d %-9.2f %-6d %d" % (label, r["motion_frames"], r["frames_kept"], r["segments"], r["saved_pct"],
                                                      r["do_cut"], r["centres"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
