"""`python -m mvtrim_amd.gmc FILE [--max-shift N] [--min-share S] [--json]`

Global-motion compensation: what the trimmer keeps of one recording when every frame is scanned against its own
dominant vector.  The reference thresholds each vector's own magnitude (src/motion_scanner.cpp:246-251), so a camera
that moves — a pole in wind, a PTZ tour, a vibrating mount — keeps every frame.  FILE is the JSON that
tools/extract_mvs.cpp prints (mvjson.py) or a `.mtmv` container (mvfile.py), loaded as `tune` loads it.

One plain centre scan (MotionScanner.count_centres_device) and one compensated scan (MotionScanner.scan_gmc_device,
include/mtgpu_gmc.h) of the same resident records; the existing merge runs on both.  Printed: motion frames, frames kept
and segments without and with the compensation, the share of the frames with side data whose applied vector is not
(0, 0), and the most frequent applied vectors.

--max-shift N: the largest displacement per axis the estimate looks at, 0 .. 127 (default 16; 0 switches the compensation
off).  --min-share S: the share of a frame's analysed records that must agree on an axis' mode before it is applied,
0 .. 1 (default 0.5), rounded to 1/256.

Width, height and duration come from a `.mtmv` header or from --width / --height / --duration.  Everything is computed
by libmtgpu; without a usable device the command fails, there is no CPU path.
"""
import argparse
import json
import math
import sys

import numpy as np

from . import _abi, tune
from .scanner import MergeParams, MotionScanner, ScanParams, results_from_bytes

TOP_VECTORS = 8


def _max_shift(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--max-shift: {text!r} is not an integer")
    if not 0 <= v <= _abi.GMC_MAX_SHIFT:
        raise argparse.ArgumentTypeError(f"--max-shift: {text!r} is not in [0, {_abi.GMC_MAX_SHIFT}]")
    return v


def _min_share(text):
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--min-share: {text!r} is not a number")
    if not text.strip() or not math.isfinite(v) or not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError(f"--min-share: {text!r} is not in [0, 1]")
    return v


def share_q8(share):
    """A share in [0, 1] as the library's min_share_q8 in [0, 256], rounded to the nearest 1/256."""
    return int(round(float(share) * 256.0))


def parser():
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.gmc", description=__doc__.splitlines()[2])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    ap.add_argument("--max-shift", type=_max_shift, default=_abi.GMC_DEFAULT_MAX_SHIFT, metavar="N",
                    help="largest displacement per axis the estimate looks at, 0 .. 127 (default %(default)s)")
    ap.add_argument("--min-share", type=_min_share, default=_abi.GMC_DEFAULT_MIN_SHARE_Q8 / 256.0, metavar="S",
                    help="share of the analysed records that must agree on a mode, 0 .. 1 (default %(default)s)")
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


def measure(scanner, batch, pts, merge_params, max_shift=_abi.GMC_DEFAULT_MAX_SHIFT, min_share_q8=_abi.GMC_DEFAULT_MIN_SHARE_Q8):
    """One plain and one compensated scan of the batch, then the merge on both.  Returns a dict: `without_gmc` /
    `with_gmc` (motion_frames, frames_kept, segments, saved_pct, do_cut, centres, kept: the indices of the motion frames),
    `compensated_share` (of the frames with side data) and `vectors`: [[gx, gy, frames]], most frequent first."""
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
        flags0, centres0 = scanner.count_centres_device(d_rec, d_off, d_sd)
        flags1, centres1, info = scanner.scan_gmc_device(d_rec, d_off, d_sd, max_shift, min_share_q8)
        without = scanner.merge_streams_device(flags0, d_pts, d_soff, d_mp, seg_cap=1)
        with_g = scanner.merge_streams_device(flags1, d_pts, d_soff, d_mp, seg_cap=1)
        torch.cuda.synchronize(dev)
    out = {}
    for name, (_seg, res), fl, ce in (("without_gmc", without, flags0, centres0), ("with_gmc", with_g, flags1, centres1)):
        r = results_from_bytes(res.cpu().numpy())[0]
        if int(r["status"]) != _abi.MT_OK:
            raise _abi.MtgpuError(int(r["status"]), "timestamps contain NaN")
        f = fl.cpu().numpy()
        out[name] = {"motion_frames": int(f.sum()), "frames_kept": int(r["n_timestamps"]), "segments": int(r["n_segments"]),
                     "saved_pct": float(r["saved_pct"]), "do_cut": int(r["do_cut"]),
                     "centres": int(ce.cpu().numpy().view(np.uint32).sum(dtype=np.uint64)), "kept": np.flatnonzero(f).tolist()}
    inf = info.cpu().numpy().reshape(-1).view(_abi.GMC_INFO_DTYPE)
    has = np.diff(np.asarray(batch.frame_off).astype(np.int64)) > 0 if batch.has_sd is None else np.asarray(batch.has_sd) != 0
    moved = (inf["gx"] != 0) | (inf["gy"] != 0)
    out["compensated_share"] = float(moved.sum()) / float(has.sum()) if has.any() else 0.0
    vec, cnt = np.unique(np.stack([inf["gx"][has], inf["gy"][has]], axis=1), axis=0, return_counts=True) if has.any() else ([], [])
    order = sorted(range(len(cnt)), key=lambda i: (-int(cnt[i]), abs(int(vec[i][0])) + abs(int(vec[i][1])), tuple(vec[i])))
    out["vectors"] = [[int(vec[i][0]), int(vec[i][1]), int(cnt[i])] for i in order[:TOP_VECTORS]]
    return out


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)           # exits 2 on a bad option: nothing below has run, no device has been touched
    try:
        batch, pts, hdr = tune.load(a.file)
    except (OSError, ValueError, KeyError) as e:
        print(f"gmc: cannot read {a.file}: {e}", file=sys.stderr)
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
    q8 = share_q8(a.min_share)
    try:
        with MotionScanner(params, device=a.device) as s:
            res = measure(s, batch, pts, mp, a.max_shift, q8)
    except _abi.MtgpuError as e:
        print(f"gmc: {e}", file=sys.stderr)
        return 1
    if a.json:
        print(json.dumps({"file": a.file, "width": width, "height": height, "grid_w": params.grid_w, "grid_h": params.grid_h,
                          "frames": batch.n_frames, "max_shift": a.max_shift, "min_share_q8": q8, **res}))
        return 0
    print(f"# grid {params.grid_w} x {params.grid_h}, {batch.n_frames} frames; max_shift {a.max_shift}, min_share {q8}/256; "
          f"{100.0 * res['compensated_share']:.2f}% of the frames with side data have a non-zero applied vector")
    print("gmc     motion_frames frames_kept segments saved_pct do_cut centres")
    for name, label in (("without_gmc", "without"), ("with_gmc", "with")):
        r = res[name]
        print("%-7s %-13d %-11d %-8d %-9.2f %-6d %d" % (label, r["motion_frames"], r["frames_kept"], r["segments"], r["saved_pct"],
                                                      r["do_cut"], r["centres"]))
    print("applied vector  frames")
    for gx, gy, cnt in res["vectors"]:
        print("(%4d, %4d)    %d" % (gx, gy, cnt))
    return 0


if __name__ == "__main__":
    sys.exit(main())
