"""`python -m mvtrim_amd.lanes FILE --learn [--min-records N] [--share S] [--widen W] [--save-plane P]`
`python -m mvtrim_amd.lanes FILE (--plane P | --lane X0,Y0,X1,Y1:NAMES ...) [--invert] [--elsewhere all|none] [--json]`

Direction planes: one allow byte per grid cell, where the direction filter (direction.py) has one for the whole picture.
A two-way road lets the near lane go E and the far lane W; a gate wants arrivals where the pavement beside it wants
everything; W is ordinary on a conveyor and an event anywhere else.  FILE is the JSON that tools/extract_mvs.cpp prints
(mvjson.py) or a `.mtmv` container (mvfile.py), loaded as `tune` loads it.

--learn runs one flow map (MotionScanner.flow_map_device: the counting records per sector and destination cell) and makes
a plane of it: a cell with fewer than --min-records records is left unrestricted; in the others sector k is usual iff it
holds at least --share of the cell's records, widened by --widen sectors to either side.  Printed: one line per grid row,
one glyph per cell — the arrow of the cell's dominant sector, a dot where nothing was learned.  --save-plane writes the
plane as a `.mtdir` text file.

--plane reads such a file; --lane gives rectangles by hand (see --unit), each with the sectors allowed inside it, later
ones over earlier ones, `--elsewhere` in the cells of none.  --invert turns a learned plane into the wrong-way detector:
a restricted cell allows exactly the sectors that are NOT usual there, and a cell without a restriction (byte 0xFF: not
learned, or every direction is usual) gets --elsewhere.  One plane scan (MotionScanner.scan_lanes_device) per row; the
existing merge runs on the flags.  Printed: frames kept, segments and seconds kept under all sectors and under the plane.

Width, height and duration come from a `.mtmv` header or from --width / --height / --duration.  Everything but the plane
arithmetic is computed by libmtgpu; without a usable device the command fails, there is no CPU path.

The helpers below (plane_from_rects, plane_from_flow, learned_from_flow, invert_plane, dominant_sector, save_plane,
load_plane) are pure numpy.
"""
import argparse
import json
import math
import sys
import types

import numpy as np

from . import _abi, tune, zones
from .direction import ALL, SECTOR_NAMES, allow_from_names
from .scanner import MergeParams, MotionScanner, ScanParams, results_from_bytes

UNITS = zones.UNITS
MAX_RECTS = zones.MAX_RECTS
GLYPHS = "→↘↓↙←↖↑↗"      # E, SE, S, SW, W, NW, N, NE as seen on the screen
GLYPH_NONE = "·"
ASCII_GLYPHS, ASCII_NONE = "01234567", "."


# ------------------------------------------------------------------ planes (numpy only)

def _byte(v, what):
    v = int(v)
    if not 0 <= v <= 255:
        raise ValueError(f"{what} {v} outside 0 .. 255")
    return v


def plane_from_rects(gw, gh, rects, elsewhere=ALL, unit="cell", shift=0, size=None):
    """uint8 [gh, gw]: `elsewhere` in every cell, then every rectangle in turn, later ones over earlier ones.  rects:
    ((x0, y0, x1, y1), names) pairs — the rectangle as zones.keep_from_rects takes it (half-open; unit "cell", or "px" /
    "frac" with the grid's block `shift` and the picture's `size`), names as direction.allow_from_names takes them
    ("E,NE", ["W"], "all", "none") or an allow byte."""
    grid = types.SimpleNamespace(grid_w=int(gw), grid_h=int(gh), block_shift=int(shift))
    plane = np.full((int(gh), int(gw)), _byte(elsewhere, "elsewhere"), dtype=np.uint8)
    for rect, names in rects:
        allow = _byte(names, "allow") if isinstance(names, (int, np.integer)) else allow_from_names(names)
        inside = ~zones.keep_from_rects(grid, [tuple(rect)], unit, size)
        plane[inside] = allow
    return plane


def _flow(flow):
    flow = np.asarray(flow)
    if flow.ndim != 3 or flow.shape[0] != 8:
        raise ValueError(f"flow has shape {flow.shape}, want [8, grid_h, grid_w] (one stream of a flow map)")
    return flow.astype(np.int64)


def learned_from_flow(flow, min_records):
    """bool [gh, gw]: the cells that hold at least min_records counting records over all sectors."""
    return _flow(flow).sum(axis=0) >= int(min_records)


def plane_from_flow(flow, min_records=16, share_q8=64, widen=1, elsewhere=ALL):
    """uint8 [gh, gw] from one stream of a flow map (uint32 [8, gh, gw]).  For a cell with T = sum over k of flow[k]:
    T < min_records: the byte is `elsewhere`; else bit k is set iff flow[k] * 256 >= share_q8 * T, and then the sectors
    (k +- j) & 7, j <= widen, are set too.  Integer and exact."""
    flow = _flow(flow)
    share_q8, widen = int(share_q8), int(widen)
    if not 0 <= share_q8 <= 256:
        raise ValueError(f"share_q8 {share_q8} outside 0 .. 256")
    if not 0 <= widen <= 4:
        raise ValueError(f"widen {widen} outside 0 .. 4")
    total = flow.sum(axis=0)
    usual = flow * 256 >= share_q8 * total                       # [8, gh, gw]
    wide = usual.copy()
    for j in range(1, widen + 1):
        wide |= np.roll(usual, j, axis=0) | np.roll(usual, -j, axis=0)
    bits = (wide.astype(np.int64) << np.arange(8).reshape(8, 1, 1)).sum(axis=0)
    return np.where(total >= int(min_records), bits, _byte(elsewhere, "elsewhere")).astype(np.uint8)


def invert_plane(plane, learned, elsewhere=0):
    """uint8 [gh, gw]: byte ^ 0xFF on the learned cells (bool [gh, gw]), `elsewhere` on the others: motion against the
    usual flow of its own cell."""
    plane, learned = np.asarray(plane, dtype=np.uint8), np.asarray(learned).astype(bool)
    if plane.ndim != 2 or learned.shape != plane.shape:
        raise ValueError(f"plane has shape {plane.shape} and learned {learned.shape}: want the same [grid_h, grid_w]")
    return np.where(learned, plane ^ np.uint8(0xFF), np.uint8(_byte(elsewhere, "elsewhere"))).astype(np.uint8)


def dominant_sector(flow, min_records=1):
    """int [gh, gw]: the smallest sector whose count is maximal, -1 where the cell holds fewer than max(1, min_records)
    records."""
    flow = _flow(flow)
    return np.where(flow.sum(axis=0) >= max(1, int(min_records)), flow.argmax(axis=0), -1)


MTDIR_MAGIC = "mtdir 1"
_HEX = "0123456789abcdefABCDEF"


def save_plane(path, plane):
    """Write a uint8 [grid_h, grid_w] plane as a `.mtdir` text file: line 1 `mtdir 1`, line 2 `<grid_w> <grid_h>`, then
    grid_h lines of grid_w two-digit hex bytes, bit k of a byte = sector k may vote (0 = E, clockwise on the screen).
    Plain text, so that a plane can be edited by hand."""
    plane = np.asarray(plane)
    if plane.ndim != 2 or plane.shape[0] < 1 or plane.shape[1] < 1 or plane.dtype != np.uint8:
        raise ValueError(f"plane has shape {plane.shape} and type {plane.dtype}, want uint8 [grid_h, grid_w]")
    gh, gw = plane.shape
    rows = ["".join("%02x" % v for v in row) for row in plane.tolist()]
    with open(path, "w", encoding="ascii", newline="\n") as f:
        f.write(f"{MTDIR_MAGIC}\n{gw} {gh}\n" + "\n".join(rows) + "\n")


def load_plane(path, grid=None):
    """Read a `.mtdir` file -> uint8 [grid_h, grid_w].  grid: (grid_w, grid_h) the file must match, or None.  ValueError
    names the line of anything else: another first line, a grid that does not match, a short file, a line of another
    length, a character that is no hex digit, lines behind the last row."""
    with open(path, "r", encoding="ascii", errors="replace", newline="") as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()                                        # the final newline
    lines = [ln[:-1] if ln.endswith("\r") else ln for ln in lines]
    if not lines or lines[0] != MTDIR_MAGIC:
        raise ValueError(f"{path}: line 1: want '{MTDIR_MAGIC}'")
    dims = lines[1].split(" ") if len(lines) > 1 else []
    if len(dims) != 2 or not all(d.isascii() and d.isdigit() and len(d) <= 6 for d in dims) or int(dims[0]) < 1 or int(dims[1]) < 1:
        raise ValueError(f"{path}: line 2: want '<grid_w> <grid_h>'")
    gw, gh = int(dims[0]), int(dims[1])
    if grid is not None and (gw, gh) != (int(grid[0]), int(grid[1])):
        raise ValueError(f"{path}: line 2: the plane is for a {gw}x{gh} grid, this one is {int(grid[0])}x{int(grid[1])}")
    plane = np.zeros((gh, gw), dtype=np.uint8)
    for y in range(gh):
        n = 3 + y
        if n > len(lines):
            raise ValueError(f"{path}: line {n}: the file ends after {y} of {gh} rows")
        row = lines[n - 1]
        if len(row) != 2 * gw:
            raise ValueError(f"{path}: line {n}: {len(row)} characters, want {2 * gw} ({gw} two-digit hex bytes)")
        for x, ch in enumerate(row):
            if ch not in _HEX:
                raise ValueError(f"{path}: line {n}: character {x + 1} is no hex digit")
        plane[y] = np.frombuffer(bytes.fromhex(row), dtype=np.uint8)
    if len(lines) > 2 + gh:
        raise ValueError(f"{path}: line {3 + gh}: text behind the last of {gh} rows")
    return plane


def glyph_rows(dominant, ascii_only=False):
    """One string per grid row from dominant_sector's array."""
    glyphs, none = (ASCII_GLYPHS, ASCII_NONE) if ascii_only else (GLYPHS, GLYPH_NONE)
    return ["".join(none if k < 0 else glyphs[k] for k in row) for row in np.asarray(dominant).tolist()]


# ------------------------------------------------------------------ the command

def _lane(text):
    rect, sep, names = text.partition(":")
    try:
        v = [float(x) for x in rect.split(",")]
    except ValueError:
        v = []
    if not sep or len(v) != 4 or not all(math.isfinite(x) for x in v):
        raise argparse.ArgumentTypeError(f"--lane: {text!r} is not X0,Y0,X1,Y1:NAMES")
    if v[0] < 0 or v[1] < 0 or v[2] < v[0] or v[3] < v[1]:
        raise argparse.ArgumentTypeError(f"--lane: {text!r}: want 0 <= X0 <= X1 and 0 <= Y0 <= Y1")
    try:
        allow = allow_from_names(names)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"--lane: {e}")
    return tuple(v), allow


def _share(text):
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--share: {text!r} is not a number")
    if not text.strip() or not math.isfinite(v) or not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError(f"--share: {text!r} is not in [0, 1]")
    return v


def _whole(flag, lo, hi):
    def parse(text):
        try:
            v = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f"{flag}: {text!r} is not a whole number")
        if not lo <= v <= hi:
            raise argparse.ArgumentTypeError(f"{flag}: {v} is not in {lo} .. {hi}")
        return v
    return parse


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.lanes", description=__doc__.splitlines()[3])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    ap.add_argument("--learn", action="store_true", help="learn a plane from the recording's flow map and print its dominant sectors")
    ap.add_argument("--min-records", type=_whole("--min-records", 0, 2 ** 31 - 1), default=16, metavar="N",
                    help="--learn: a cell with fewer counting records stays unrestricted (default 16)")
    ap.add_argument("--share", type=_share, default=0.25, metavar="S",
                    help="--learn: a sector is usual in a cell with at least this share of its records (default 0.25)")
    ap.add_argument("--widen", type=_whole("--widen", 0, 4), default=1, metavar="W",
                    help="--learn: the usual sectors and W sectors to either side of each (default 1)")
    ap.add_argument("--save-plane", metavar="P", help="--learn: write the plane as a .mtdir text file")
    ap.add_argument("--plane", metavar="P", help="a .mtdir text plane (save_plane / --save-plane)")
    ap.add_argument("--lane", action="append", type=_lane, metavar="X0,Y0,X1,Y1:NAMES", default=[],
                    help="inside the rectangle [X0, X1) x [Y0, Y1) the sectors NAMES may vote (may be given several times)")
    ap.add_argument("--unit", choices=UNITS, default="px", help="unit of --lane: pixels (default), fractions of the picture, grid cells")
    ap.add_argument("--invert", action="store_true", help="allow what a restricted cell forbids; --elsewhere in the unrestricted ones")
    ap.add_argument("--elsewhere", choices=("all", "none"), help="the sectors of the cells no rectangle covers, and with --invert "
                    "of the unrestricted ones (default: all, with --invert: none)")
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
    if a.learn and (a.plane or a.lane or a.invert or a.elsewhere):
        ap.error("--learn goes without --plane, --lane, --invert and --elsewhere")
    if not a.learn and a.save_plane:
        ap.error("--save-plane goes with --learn")
    if not a.learn and not a.plane and not a.lane:
        ap.error("one of --learn, --plane and --lane is wanted")
    if a.plane and a.lane:
        ap.error("--plane and --lane exclude each other")
    if len(a.lane) > MAX_RECTS:
        ap.error(f"--lane: {len(a.lane)} rectangles, at most {MAX_RECTS}")
    for r, _ in a.lane:
        if a.unit == "frac":
            if max(r) > 1.0:
                ap.error(f"--lane: {r} is not inside [0, 1] (--unit frac)")
        elif any(int(v) != v for v in r):
            ap.error(f"--lane: {r} is not whole numbers (--unit {a.unit})")


def _resident(scanner, batch, pts, merge_params):
    import torch
    dev = torch.device("cuda", scanner.device)
    mv = np.ascontiguousarray(batch.mv, dtype=_abi.MV_DTYPE)
    d = types.SimpleNamespace(dev=dev)
    d.rec = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy()).to(dev)
    d.off = torch.from_numpy(np.ascontiguousarray(batch.frame_off, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d.sd = None if batch.has_sd is None else torch.from_numpy(np.ascontiguousarray(batch.has_sd, dtype=np.uint8)).to(dev)
    d.pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(dev)
    d.soff = torch.tensor([0, batch.n_frames], dtype=torch.int64, device=dev)
    d.mp = torch.from_numpy(merge_params.to_record().view(np.uint8).copy()).to(dev)
    return d


def learn(scanner, batch, pts, merge_params):
    """One flow map of the resident batch: uint32 [8, gh, gw]."""
    import torch
    d = _resident(scanner, batch, pts, merge_params)
    with torch.cuda.device(d.dev):
        flow = scanner.flow_map_device(d.rec, d.off, d.sd, d.soff)
        torch.cuda.synchronize(d.dev)
    return flow.cpu().numpy().view(np.uint32)[0]


def measure(scanner, batch, pts, merge_params, planes):
    """One plane scan per plane of `planes` (uint8 [gh, gw] each) on the resident batch, then the unchanged merge on its
    flags.  Returns one dict per plane."""
    import torch
    d = _resident(scanner, batch, pts, merge_params)
    rows = []
    with torch.cuda.device(d.dev):
        for plane in planes:
            d_plane = torch.from_numpy(np.ascontiguousarray(plane, dtype=np.uint8)).to(d.dev)
            res = scanner.scan_lanes_device(d.rec, d.off, d.sd, d_plane, want=("flags", "centres"))
            _seg, mres = scanner.merge_streams_device(res["flags"], d.pts, d.soff, d.mp, seg_cap=1)
            torch.cuda.synchronize(d.dev)
            r = results_from_bytes(mres.cpu().numpy())[0]
            if int(r["status"]) != _abi.MT_OK:
                raise _abi.MtgpuError(int(r["status"]), "timestamps contain NaN")
            flags = res["flags"].cpu().numpy()
            rows.append({"motion_frames": int(flags.sum()), "frames": np.flatnonzero(flags).tolist(),
                         "frames_kept": int(r["n_timestamps"]), "segments": int(r["n_segments"]),
                         "seconds_kept": float(merge_params.duration) - float(r["time_removed"]), "saved_pct": float(r["saved_pct"]),
                         "do_cut": int(r["do_cut"]), "centres": int(res["centres"].cpu().numpy().view(np.uint32).sum(dtype=np.uint64))})
    return rows


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad option: nothing below has run, no device has been touched
    _check_args(ap, a)
    try:
        path = a.file
        batch, pts, hdr = tune.load(path)
        path = a.plane
        given = None if path is None else load_plane(path)
    except (OSError, ValueError, KeyError) as e:
        print(f"lanes: cannot read {path}: {e}", file=sys.stderr)
        return 1
    width = a.width if a.width is not None else hdr.get("width")
    height = a.height if a.height is not None else hdr.get("height")
    duration = a.duration if a.duration is not None else hdr.get("duration")
    if width is None or height is None or duration is None:
        ap.error("the file carries no width / height / duration: give --width, --height and --duration")
    params = ScanParams.from_config(width, height, block_size=a.block_size, block_shift=a.block_shift,
                                    vectors_needed=a.vectors_needed, mv_threshold_sq=a.mv_threshold_sq,
                                    clusters_needed=a.clusters_needed, vertical_mask=a.vertical_mask)
    gw, gh = params.grid_w, params.grid_h
    mp = MergeParams(duration=float(duration), max_gap_sec=a.max_gap_sec, padding_sec=a.padding_sec,
                     min_savings_pct=a.min_savings_pct)
    if given is not None and given.shape != (gh, gw):
        ap.error(f"--plane: the plane is for a {given.shape[1]}x{given.shape[0]} grid, this one is {gw}x{gh}")
    try:
        with MotionScanner(params, device=a.device) as s:
            if a.learn:
                flow = learn(s, batch, pts, mp)
            else:
                elsewhere = {"all": ALL, "none": 0, None: 0 if a.invert else ALL}[a.elsewhere]
                plane = given if given is not None else plane_from_rects(gw, gh, a.lane, ALL if a.invert else elsewhere, a.unit,
                                                                           params.block_shift, (width, height))
                restricted = int((plane != ALL).sum())          # of the plane as given: what --invert turns round
                if a.invert:
                    plane = invert_plane(plane, plane != ALL, elsewhere)
                rows = measure(s, batch, pts, mp, [np.full((gh, gw), ALL, dtype=np.uint8), plane])
    except _abi.MtgpuError as e:
        print(f"lanes: {e}", file=sys.stderr)
        return 1
    if a.learn:
        plane = plane_from_flow(flow, a.min_records, int(round(a.share * 256)), a.widen, ALL)
        if a.save_plane:
            save_plane(a.save_plane, plane)
        learned = learned_from_flow(flow, a.min_records)
        enc = (getattr(sys.stdout, "encoding", None) or "ascii")
        try:
            (GLYPHS + GLYPH_NONE).encode(enc)
            plain = False
        except (UnicodeEncodeError, LookupError):
            plain = True
        print(f"# grid {gw} x {gh}, {batch.n_frames} frames, {int(flow.sum(dtype=np.uint64))} counting records with a direction, "
              f"{int(learned.sum())} of {gw * gh} cells learned")
        for row in glyph_rows(dominant_sector(flow, a.min_records), plain):
            print(row)
        return 0
    doc = {"file": a.file, "width": width, "height": height, "grid_w": gw, "grid_h": gh, "frames": batch.n_frames,
           "restricted_cells": restricted, "inverted": bool(a.invert), "all": rows[0], "plane": rows[1]}
    if a.json:
        print(json.dumps(doc))
        return 0
    print(f"# grid {gw} x {gh}, {batch.n_frames} frames; {restricted} of {gw * gh} cells restrict a direction"
          + (", inverted" if a.invert else ""))
    print("sectors motion_frames frames_kept segments seconds_kept saved_pct do_cut centres")
    for label, r in (("all", rows[0]), ("plane", rows[1])):
        print("%-7s %-13d %-11d %-8d %-12.3f %-9.2f %-6d %d" % (label, r["motion_frames"], r["frames_kept"], r["segments"],
                                                              r["seconds_kept"], r["saved_pct"], r["do_cut"], r["centres"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
