"""`python -m mvtrim_amd.activity FILE [--min-centres N | --kept] [--vertical-mask M[,M...]] [--npy PREFIX] [--json]`

WHERE in the picture a recording moves: the per-cell activity map of one recording, the number the reference's
VERTICAL_MASK ("for eliminating false positives from timestamps, watermarks, or motion in fixed UI elements",
config/motion_trim.env) has to be chosen on.  FILE is the JSON that tools/extract_mvs.cpp prints (mvjson.py) or a
`.mtmv` container (mvfile.py), loaded as `tune` loads it.  One call (MotionScanner.activity_map_device) counts, for
every grid cell, the frames in which the cell was active and the frames in which it was one of the centres
src/motion_scanner.cpp:277-292 counts, over the frames that contribute: every frame with side data, or with
--min-centres N / --kept only those whose centre count reaches N / max(1, CLUSTERS_NEEDED) (the frames the trimmer
keeps).  The map is taken WITHOUT a vertical mask.  One line per grid row: row, sum of active, sum of centre, the row's
share of all centre counts.

--vertical-mask adds one line per candidate: the margin in rows it means (the float32 product of
mtgpu_params_from_config) and the share of the centre counts that lies in the rows it would drop.  That share is an
ESTIMATE from the unmasked map, not the count a masked scan returns: a mask also removes the dropped rows' cells as
neighbours of the rows next to them.  The exact answer is one scan with that mask.

Width and height come from a `.mtmv` header or from --width / --height (the JSON carries neither).  Everything is
computed by libmtgpu; without a usable device the command fails, there is no CPU path.
"""
import argparse
import json
import math
import sys

import numpy as np

from . import _abi, tune
from .scanner import MotionScanner, ScanParams

ESTIMATE = ("estimate from the unmasked map: the share of centre counts in the rows the mask drops, not the count a "
            "masked scan returns (the exact answer is one scan with that mask)")
MAX_MASKS = 16


def _mask(text):
    v = float(text)
    if not text.strip() or not math.isfinite(v) or v < 0.0:
        raise ValueError(text)
    return v


def _uint32(text):
    v = int(text.strip(), 10)
    if not 0 <= v < 2 ** 32:
        raise argparse.ArgumentTypeError(f"{text!r} is not in [0, 2^32)")
    return v


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.activity", description=__doc__.splitlines()[2])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--min-centres", type=_uint32, default=0, metavar="N",
                   help="only frames whose centre count is >= N contribute (default 0: every frame with side data)")
    g.add_argument("--kept", action="store_true", help="--min-centres max(1, CLUSTERS_NEEDED): the frames the trimmer keeps")
    ap.add_argument("--vertical-mask", metavar="M[,M...]", type=tune._list_of(_mask, "--vertical-mask", 1, MAX_MASKS),
                    help="candidate VERTICAL_MASK values; for each: its margin in rows and an " + ESTIMATE)
    ap.add_argument("--npy", metavar="PREFIX", help="write PREFIX_active.npy and PREFIX_centre.npy (uint32 [grid_h, grid_w])")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--block-size", type=int)
    ap.add_argument("--block-shift", type=int)
    ap.add_argument("--vectors-needed", type=int)
    ap.add_argument("--mv-threshold-sq", type=float)
    ap.add_argument("--clusters-needed", type=int)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", action="store_true", help="one JSON document instead of the table")
    return ap


def measure(scanner, batch, min_centres):
    """(active uint32 [gh, gw], centre uint32 [gh, gw], contributing frames) of the whole batch as one stream."""
    import torch
    dev = torch.device("cuda", scanner.device)
    mv = np.ascontiguousarray(batch.mv, dtype=_abi.MV_DTYPE)
    d_rec = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy()).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(batch.frame_off, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_sd = None if batch.has_sd is None else torch.from_numpy(np.ascontiguousarray(batch.has_sd, dtype=np.uint8)).to(dev)
    d_soff = torch.tensor([0, batch.n_frames], dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        active, centre, frames = scanner.activity_map_device(d_rec, d_off, d_sd, d_soff, min_centres=min_centres)
        torch.cuda.synchronize(dev)
    return (active[0].cpu().numpy().view(np.uint32), centre[0].cpu().numpy().view(np.uint32),
            int(frames.cpu().numpy().view(np.uint32)[0]))


def row_table(active, centre):
    """One dict per grid row: row, active, centre (sums over the row), centre_share (of the map's centre total)."""
    tot = int(centre.sum(dtype=np.uint64))
    return [{"row": y, "active": int(active[y].sum(dtype=np.uint64)), "centre": int(centre[y].sum(dtype=np.uint64)),
             "centre_share": (int(centre[y].sum(dtype=np.uint64)) / tot) if tot else 0.0} for y in range(centre.shape[0])]


def mask_table(centre, margins):
    """margins: [(vertical_mask, margin_rows)] -> one dict per candidate: the share of the centre counts lying in rows
    outside [margin, grid_h - margin)."""
    gh = centre.shape[0]
    tot = int(centre.sum(dtype=np.uint64))
    out = []
    for mask, margin in margins:
        lo, hi = min(margin, gh), max(gh - margin, min(margin, gh))
        kept = int(centre[lo:hi].sum(dtype=np.uint64))
        out.append({"vertical_mask": mask, "margin_rows": margin,
                    "centre_share_dropped": ((tot - kept) / tot) if tot else 0.0, "kind": ESTIMATE})
    return out


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad list: nothing below has run, no device has been touched
    try:
        batch, _pts, hdr = tune.load(a.file)
    except (OSError, ValueError, KeyError) as e:
        print(f"activity: cannot read {a.file}: {e}", file=sys.stderr)
        return 1
    width = a.width if a.width is not None else hdr.get("width")
    height = a.height if a.height is not None else hdr.get("height")
    if width is None or height is None:
        ap.error("the file carries no width / height: give --width and --height")
    cfg = dict(block_size=a.block_size, block_shift=a.block_shift, vectors_needed=a.vectors_needed,
               mv_threshold_sq=a.mv_threshold_sq, clusters_needed=a.clusters_needed)
    params = ScanParams.from_config(width, height, vertical_mask=0.0, **cfg)
    margins = [(v, ScanParams.from_config(width, height, vertical_mask=v, **cfg).vertical_margin)
               for v in (a.vertical_mask or [])]
    min_centres = max(1, params.clusters_needed) if a.kept else a.min_centres
    try:
        with MotionScanner(params, device=a.device) as s:
            active, centre, frames = measure(s, batch, min_centres)
    except _abi.MtgpuError as e:
        print(f"activity: {e}", file=sys.stderr)
        return 1
    if a.npy:
        np.save(a.npy + "_active.npy", active)
        np.save(a.npy + "_centre.npy", centre)
    rows, masks = row_table(active, centre), mask_table(centre, margins)
    if a.json:
        print(json.dumps({"file": a.file, "width": width, "height": height, "grid_w": params.grid_w, "grid_h": params.grid_h,
                          "frames": batch.n_frames, "contributing_frames": frames, "min_centres": min_centres,
                          "rows": rows, "vertical_mask": masks}))
        return 0
    print(f"# {frames} of {batch.n_frames} frames contribute (min_centres {min_centres}); grid {params.grid_w} x {params.grid_h}")
    print("row active centre centre_share")
    for r in rows:
        print("%-3d %-10d %-10d %.6f" % (r["row"], r["active"], r["centre"], r["centre_share"]))
    if masks:
        print("# " + ESTIMATE)
        print("vertical_mask margin_rows centre_share_dropped")
        for r in masks:
            print("%-13g %-11d %.6f" % (r["vertical_mask"], r["margin_rows"], r["centre_share_dropped"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
