"""`python -m mvtrim_amd.tune FILE --mv-threshold-sq 1,4,16 --vectors-needed 1,2,4 --clusters-needed 1,2,4 [--json]`

The sensitivity study the reference's config/motion_trim.env asks its users to make by hand: what MV_THRESHOLD_SQ,
VECTORS_NEEDED and CLUSTERS_NEEDED do to one recording.  FILE is the JSON that tools/extract_mvs.cpp prints (mvjson.py)
or a `.mtmv` container (mvfile.py), loaded as `motion_scalar` loads it.  One sweep call (MotionScanner.sweep_centres_device)
gives every frame's centre count (src/motion_scanner.cpp:272-294) for every (threshold, vectors) pair; one
sweep_streams_device call per pair turns the counts into segments (src/pipeline.cpp:302-358) for every clusters level.
One row per (threshold, vectors, clusters): frames with motion, segments, saved_pct, do_cut.

Width, height and duration come from a `.mtmv` header or from --width / --height / --duration (the JSON carries none of
them).  The merge constants are the reference's defaults (config.py), overridable.  Frames whose timestamp is null are
left out.  Everything is computed by libmtgpu; without a usable device the command fails, there is no CPU path.
"""
import argparse
import json
import sys

import numpy as np

from . import _abi, config, motion_scalar, mvfile
from .scanner import FrameBatch, MergeParams, MotionScanner, ScanParams, results_from_bytes


def _list_of(conv, what, lo, hi):
    def parse(text):
        try:
            vals = [conv(x) for x in text.split(",")]
        except (ValueError, OverflowError):
            raise argparse.ArgumentTypeError(f"{what}: {text!r} is not a comma-separated list of numbers")
        if not lo <= len(vals) <= hi:
            raise argparse.ArgumentTypeError(f"{what}: {len(vals)} values, want {lo} to {hi}")
        return vals
    return parse


def _int32(text):
    v = int(text.strip(), 10)
    if not -2 ** 31 <= v < 2 ** 31:
        raise ValueError(text)
    return v


def _number(text):
    if not text.strip():
        raise ValueError(text)
    return float(text)


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.tune", description=__doc__.splitlines()[2])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    ap.add_argument("--mv-threshold-sq", required=True, metavar="T[,T...]",
                    type=_list_of(_number, "--mv-threshold-sq", 1, _abi.SWEEP_MAX_THRESHOLDS))
    ap.add_argument("--vectors-needed", required=True, metavar="V[,V...]",
                    type=_list_of(_int32, "--vectors-needed", 1, _abi.SWEEP_MAX_VECTORS))
    ap.add_argument("--clusters-needed", required=True, metavar="C[,C...]",
                    type=_list_of(_int32, "--clusters-needed", 1, _abi.SWEEP_MAX_LEVELS))
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--duration", type=float, help="seconds")
    ap.add_argument("--block-size", type=int)
    ap.add_argument("--block-shift", type=int)
    ap.add_argument("--vertical-mask", type=float)
    ap.add_argument("--max-gap-sec", type=float)
    ap.add_argument("--padding-sec", type=float)
    ap.add_argument("--min-savings-pct", type=float)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", action="store_true", help="one JSON document instead of the table")
    return ap


def load(path):
    """(FrameBatch of the frames that have a timestamp, their pts float64 [F], header dict) of FILE."""
    batch, pts = motion_scalar.load(path)
    hdr = {}
    with open(path, "rb") as fh:
        if fh.read(8) == mvfile.MAGIC:
            h = mvfile.read_mtmv(path)[0]
            hdr = {k: (float if k in ("fps", "duration") else int)(h[k]) for k in ("width", "height", "fps", "duration")}
    keep = [i for i, p in enumerate(pts) if p is not None and p >= 0]
    if len(keep) != len(pts):
        frames = []
        for i in keep:
            a, b = int(batch.frame_off[i]), int(batch.frame_off[i + 1])
            frames.append(batch.mv[a:b] if batch.has_sd is None or batch.has_sd[i] else None)
        batch = FrameBatch.from_frames(frames)
    return batch, np.array([pts[i] for i in keep], dtype=np.float64), hdr


def study(scanner, batch, pts, merge_params, thresholds, vectors, clusters):
    """Rows (dicts) in (threshold, vectors, clusters) order: one sweep of the records, then one merge sweep per pair."""
    import torch
    dev = torch.device("cuda", scanner.device)
    n = batch.n_frames
    mv = np.ascontiguousarray(batch.mv, dtype=_abi.MV_DTYPE)
    d_rec = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy()).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(batch.frame_off, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_sd = None if batch.has_sd is None else torch.from_numpy(np.ascontiguousarray(batch.has_sd, dtype=np.uint8)).to(dev)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(dev)
    d_soff = torch.tensor([0, n], dtype=torch.int64, device=dev)
    d_mp = torch.from_numpy(merge_params.to_record().view(np.uint8).copy()).to(dev)
    with torch.cuda.device(dev):
        centres = scanner.sweep_centres_device(d_rec, d_off, d_sd, thresholds, vectors)
        merged = [[scanner.sweep_streams_device(centres[t, v], d_pts, d_soff, d_mp, clusters, seg_cap=1)
                   for v in range(len(vectors))] for t in range(len(thresholds))]
        torch.cuda.synchronize(dev)
    rows = []
    for t, thr in enumerate(thresholds):
        for v, vec in enumerate(vectors):
            res = results_from_bytes(merged[t][v][1].cpu().numpy().reshape(len(clusters), -1))
            for c, need in enumerate(clusters):
                r = res[c]
                if int(r["status"]) != _abi.MT_OK:
                    raise _abi.MtgpuError(int(r["status"]), "timestamps contain NaN")
                rows.append({"mv_threshold_sq": thr, "vectors_needed": vec, "clusters_needed": need,
                             "motion_frames": int(r["n_timestamps"]), "segments": int(r["n_segments"]),
                             "saved_pct": float(r["saved_pct"]), "do_cut": int(r["do_cut"])})
    return rows


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad list: nothing below has run, no device has been touched
    try:
        batch, pts, hdr = load(a.file)
    except (OSError, ValueError, KeyError) as e:
        print(f"tune: cannot read {a.file}: {e}", file=sys.stderr)
        return 1
    width = a.width if a.width is not None else hdr.get("width")
    height = a.height if a.height is not None else hdr.get("height")
    duration = a.duration if a.duration is not None else hdr.get("duration")
    if width is None or height is None or duration is None:
        ap.error("the file carries no width / height / duration: give --width, --height and --duration")
    params = ScanParams.from_config(width, height, block_size=a.block_size, block_shift=a.block_shift,
                                    vertical_mask=a.vertical_mask)
    mp = MergeParams(duration=float(duration), max_gap_sec=a.max_gap_sec, padding_sec=a.padding_sec,
                     min_savings_pct=a.min_savings_pct)
    try:
        with MotionScanner(params, device=a.device) as s:
            rows = study(s, batch, pts, mp, a.mv_threshold_sq, a.vectors_needed, a.clusters_needed)
    except _abi.MtgpuError as e:
        print(f"tune: {e}", file=sys.stderr)
        return 1
    if a.json:
        print(json.dumps({"file": a.file, "width": width, "height": height, "duration": duration, "fps": hdr.get("fps"),
                          "frames": batch.n_frames, "max_gap_sec": mp.max_gap_sec, "padding_sec": mp.padding_sec,
                          "min_savings_pct": mp.min_savings_pct, "rows": rows}))
        return 0
    print("mv_threshold_sq vectors_needed clusters_needed motion_frames segments saved_pct do_cut")
    for r in rows:
        print("%-15s %-14d %-15d %-13d %-8d %-9.2f %d" % ("%g" % r["mv_threshold_sq"], r["vectors_needed"], r["clusters_needed"],
                                                      r["motion_frames"], r["segments"], r["saved_pct"], r["do_cut"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
