"""`python -m mvtrim_amd.direction FILE [--allow E,NE,... | --ignore W,...] [--each] [--keep-level N] [--json]`

The direction filter: what the trimmer keeps of one recording when only records that move in some directions may vote.
The reference squares dst - src (src/motion_scanner.cpp:246-251) and loses the sign; a one-way street, a gate or a
conveyor wants it back.  FILE is the JSON that tools/extract_mvs.cpp prints (mvjson.py) or a `.mtmv` container
(mvfile.py), loaded as `tune` loads it.

Sectors are numbered clockwise on the screen (x grows to the right, y downwards): 0 = E, 1 = SE, 2 = S, 3 = SW, 4 = W,
5 = NW, 6 = N, 7 = NE; the rule is in include/mtgpu_dir.h.  --allow names the sectors that may vote, --ignore the ones
that may not; neither: all of them.  One direction scan per mask (MotionScanner.scan_dir_device) returns every frame's
centre count under the mask and its rose; the existing merge runs on the flags.  Printed: the recording's rose — the
counting records per sector, summed over all frames and over the frames the plain scan keeps, as a count and a share —
then frames kept, segments and seconds kept for `all` and for the given mask; with --each one more row per sector k
with the wedge {k - 1, k, k + 1} ignored.  --keep-level N: a frame is kept with at least N centres (default:
max(1, CLUSTERS_NEEDED)).

Width, height and duration come from a `.mtmv` header or from --width / --height / --duration.  Everything but the name
arithmetic is computed by libmtgpu; without a usable device the command fails, there is no CPU path.

The helpers below (sector_of, allow_from_names, names_from_allow, rotate_allow, mirror_allow) are pure numpy.
"""
import argparse
import json
import sys

import numpy as np

from . import _abi, tune
from .scanner import MergeParams, MotionScanner, ScanParams, results_from_bytes

SECTOR_NAMES = ("E", "SE", "S", "SW", "W", "NW", "N", "NE")
ALL = _abi.DIR_ALL


# ------------------------------------------------------------------ sectors and masks (numpy only)

def sector_of(dx, dy):
    """The sector of a displacement (include/mtgpu_dir.h), elementwise: 0 .. 7, and -1 for dx == dy == 0.  Integer and
    exact: E / W where 12 |dy| <= 5 |dx|, S / N where 12 |dx| <= 5 |dy|, a diagonal sector otherwise."""
    dx, dy = np.asarray(dx).astype(np.int64), np.asarray(dy).astype(np.int64)
    ax, ay = np.abs(dx), np.abs(dy)
    ew, sn = 12 * ay <= 5 * ax, 12 * ax <= 5 * ay
    diag = np.where(dx > 0, np.where(dy > 0, 1, 7), np.where(dy > 0, 3, 5))
    k = np.where(ew, np.where(dx > 0, 0, 4), np.where(sn, np.where(dy > 0, 2, 6), diag))
    return np.where((dx == 0) & (dy == 0), -1, k)


def allow_from_names(names):
    """"E,SE" or ["E", "SE"] -> the allow byte with those sectors' bits; "all" -> 0xFF, "" or "none" -> 0."""
    if isinstance(names, str):
        text = names.strip()
        if text.lower() == "all":
            return ALL
        if text == "" or text.lower() == "none":
            return 0
        names = text.split(",")
    allow = 0
    for n in names:
        n = n.strip().upper()
        if n not in SECTOR_NAMES:
            raise ValueError(f"{n!r} is not one of {','.join(SECTOR_NAMES)}")
        allow |= 1 << SECTOR_NAMES.index(n)
    return allow


def names_from_allow(allow):
    """The allow byte -> "E,SE,..." in sector order; 0xFF -> "all", 0 -> "none"."""
    allow = int(allow)
    if not 0 <= allow <= 255:
        raise ValueError(f"allow {allow} outside 0 .. 255")
    if allow == ALL:
        return "all"
    if allow == 0:
        return "none"
    return ",".join(n for k, n in enumerate(SECTOR_NAMES) if (allow >> k) & 1)


def rotate_allow(allow, sectors=2):
    """The byte for the picture turned by `sectors` eighths clockwise: sector k becomes (k + sectors) & 7 (rotl8)."""
    allow, r = int(allow) & 0xFF, int(sectors) & 7
    return ((allow << r) | (allow >> (8 - r))) & 0xFF


def mirror_allow(allow):
    """The byte for the picture mirrored left to right (dx -> -dx): sector k becomes (4 - k) & 7."""
    allow = int(allow) & 0xFF
    return sum(1 << ((4 - k) & 7) for k in range(8) if (allow >> k) & 1)


def wedge(k):
    """The three sectors around k: {k - 1, k, k + 1}."""
    return sum(1 << ((k + j) & 7) for j in (-1, 0, 1))


SECTOR_WORD_MAX_COUNT = (1 << 21) - 1


def sector_word(rose):
    """A frame's rose (eight counts, sector 0 = E first) -> the sector word a pipe reports under
    set_dir(report="sectors") (include/mtgpu_pipe_dir.h): bits 0 .. 7 the present byte (bit k iff n[k] >= 1), bits
    8 .. 10 the smallest k whose count is maximal (0 when every count is 0), bits 11 .. 31 min(that count, 2^21 - 1)."""
    n = [int(v) for v in rose]
    if len(n) != 8 or min(n) < 0:
        raise ValueError("a rose is eight counts >= 0")
    present = sum(1 << k for k in range(8) if n[k] >= 1)
    best = max(n)
    k_star = n.index(best) if best > 0 else 0
    return present | (k_star << 8) | (min(best, SECTOR_WORD_MAX_COUNT) << 11)


def unpack_sector_word(word):
    """The sector word -> (present byte, dominant sector or None, count); a frame without a counting moving record
    (word 0) -> (0, None, 0).  The count saturates at 2^21 - 1."""
    word = int(word)
    if not 0 <= word <= 0xFFFFFFFF:
        raise ValueError(f"sector word {word} outside 32 bits")
    present, count = word & 0xFF, word >> 11
    return present, (((word >> 8) & 7) if count else None), count


# ------------------------------------------------------------------ the command

def _names(flag):
    def parse(text):
        try:
            return allow_from_names(text)
        except ValueError as e:
            raise argparse.ArgumentTypeError(f"{flag}: {e}")
    return parse


def _level(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--keep-level: {text!r} is not a whole number")
    if not 1 <= v < 2 ** 31:
        raise argparse.ArgumentTypeError(f"--keep-level: {v} is not at least 1")
    return v


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.direction", description=__doc__.splitlines()[2])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--allow", type=_names("--allow"), metavar="E,NE,...", help="the sectors whose records may vote")
    g.add_argument("--ignore", type=_names("--ignore"), metavar="W,...", help="the sectors whose records may not vote")
    ap.add_argument("--each", action="store_true", help="one more row per sector k with the wedge {k - 1, k, k + 1} ignored")
    ap.add_argument("--keep-level", type=_level, metavar="N", help="a frame is kept with at least N centres (default: max(1, CLUSTERS_NEEDED))")
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
    ap.add_argument("--json", action="store_true", help="one JSON document instead of the tables")
    return ap


def measure(scanner, batch, pts, merge_params, allows, keep_level=None):
    """One direction scan per byte of `allows` on the resident batch, then the unchanged merge on its flags at
    keep_level.  Returns (rose uint32 [F, 8], kept bool [F] under allow = all, a list of one dict per byte)."""
    import torch
    dev = torch.device("cuda", scanner.device)
    n = batch.n_frames
    level = max(1, scanner.params.clusters_needed) if keep_level is None else int(keep_level)
    mv = np.ascontiguousarray(batch.mv, dtype=_abi.MV_DTYPE)
    d_rec = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy()).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(batch.frame_off, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_sd = None if batch.has_sd is None else torch.from_numpy(np.ascontiguousarray(batch.has_sd, dtype=np.uint8)).to(dev)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(dev)
    d_soff = torch.tensor([0, n], dtype=torch.int64, device=dev)
    d_mp = torch.from_numpy(merge_params.to_record().view(np.uint8).copy()).to(dev)
    rows = []
    with torch.cuda.device(dev):
        plain = scanner.scan_dir_device(d_rec, d_off, d_sd, allow=ALL)
        torch.cuda.synchronize(dev)
        rose = plain["rose"].cpu().numpy().view(np.uint32).reshape(n, 8)
        kept = plain["centres"].cpu().numpy().view(np.uint32) >= level
        for allow in allows:
            res = plain if allow == ALL else scanner.scan_dir_device(d_rec, d_off, d_sd, allow=allow, want=("centres",))
            flags = scanner.flags_from_centres(res["centres"], level)
            _seg, mres = scanner.merge_streams_device(flags, d_pts, d_soff, d_mp, seg_cap=1)
            torch.cuda.synchronize(dev)
            r = results_from_bytes(mres.cpu().numpy())[0]
            if int(r["status"]) != _abi.MT_OK:
                raise _abi.MtgpuError(int(r["status"]), "timestamps contain NaN")
            rows.append({"allow": int(allow), "sectors": names_from_allow(allow), "motion_frames": int(flags.cpu().numpy().sum()),
                         "frames_kept": int(r["n_timestamps"]), "segments": int(r["n_segments"]),
                         "seconds_kept": float(merge_params.duration) - float(r["time_removed"]), "saved_pct": float(r["saved_pct"]),
                         "do_cut": int(r["do_cut"]), "centres": int(res["centres"].cpu().numpy().view(np.uint32).sum(dtype=np.uint64))})
    return rose, kept, rows


def rose_table(rose, kept):
    """Per sector: the counting records of all frames and of the kept ones, each with its share of its total."""
    every = rose.sum(axis=0, dtype=np.uint64)
    inside = rose[kept].sum(axis=0, dtype=np.uint64)
    te, ti = int(every.sum()), int(inside.sum())
    return [{"sector": k, "name": SECTOR_NAMES[k], "records": int(every[k]), "share": int(every[k]) / te if te else 0.0,
             "records_kept": int(inside[k]), "share_kept": int(inside[k]) / ti if ti else 0.0} for k in range(8)]


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad option: nothing below has run, no device has been touched
    mask = a.allow if a.allow is not None else (ALL & ~a.ignore) if a.ignore is not None else None
    try:
        batch, pts, hdr = tune.load(a.file)
    except (OSError, ValueError, KeyError) as e:
        print(f"direction: cannot read {a.file}: {e}", file=sys.stderr)
        return 1
    width = a.width if a.width is not None else hdr.get("width")
    height = a.height if a.height is not None else hdr.get("height")
    duration = a.duration if a.duration is not None else hdr.get("duration")
    if width is None or height is None or duration is None:
        ap.error("the file carries no width / height / duration: give --width, --height and --duration")
    params = ScanParams.from_config(width, height, block_size=a.block_size, block_shift=a.block_shift,
                                    vectors_needed=a.vectors_needed, mv_threshold_sq=a.mv_threshold_sq,
                                    clusters_needed=a.clusters_needed, vertical_mask=a.vertical_mask)
    mp = MergeParams(duration=float(duration), max_gap_sec=a.max_gap_sec, padding_sec=a.padding_sec,
                     min_savings_pct=a.min_savings_pct)
    allows = [ALL] + ([mask] if mask is not None else []) + ([ALL & ~wedge(k) for k in range(8)] if a.each else [])
    try:
        with MotionScanner(params, device=a.device) as s:
            rose, kept, rows = measure(s, batch, pts, mp, allows, a.keep_level)
    except _abi.MtgpuError as e:
        print(f"direction: {e}", file=sys.stderr)
        return 1
    table = rose_table(rose, kept)
    doc = {"file": a.file, "width": width, "height": height, "grid_w": params.grid_w, "grid_h": params.grid_h,
           "frames": batch.n_frames, "keep_level": max(1, params.clusters_needed) if a.keep_level is None else a.keep_level,
           "rose": table, "all": rows[0]}
    rest = rows[1:]
    if mask is not None:
        doc["mask"] = rest.pop(0)
    if a.each:
        doc["each"] = [dict(r, ignored=names_from_allow(wedge(k))) for k, r in enumerate(rest)]
    if a.json:
        print(json.dumps(doc))
        return 0
    print(f"# grid {params.grid_w} x {params.grid_h}, {batch.n_frames} frames, a frame is kept with {doc['keep_level']} centres")
    print("sector records    share  records_kept share_kept")
    for t in table:
        print("%-6s %-10d %-6.3f %-12d %.3f" % (t["name"], t["records"], t["share"], t["records_kept"], t["share_kept"]))
    print("mask                     motion_frames frames_kept segments seconds_kept saved_pct do_cut centres")
    named = [("all", doc["all"])] + ([(doc["mask"]["sectors"], doc["mask"])] if mask is not None else [])
    named += [("ignore " + r["ignored"], r) for r in doc.get("each", [])]
    for label, r in named:
        print("%-24s %-13d %-11d %-8d %-12.3f %-9.2f %-6d %d" % (label, r["motion_frames"], r["frames_kept"], r["segments"],
                                                               r["seconds_kept"], r["saved_pct"], r["do_cut"], r["centres"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
