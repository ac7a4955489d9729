"""`python -m mvtrim_amd.motion_scalar FILE` — the reference's tools/motion_scalar.cpp on the GPU.

FILE is the JSON that tools/extract_mvs.cpp prints (mvjson.py) or a `.mtmv` container (mvfile.py).  Prints what the
reference tool prints on stdout: the line `second,motion_value`, then one `second,%g` row for every second into which
a record with motion_scale != 0 falls (tools/motion_scalar.cpp:61-84, 110-113; `<<` of a double prints %g), sorted by second.  The sums are
computed by libmtgpu (MotionScanner.motion_scalar); without a usable device the command fails, there is no CPU path.
"""
import argparse
import sys

import numpy as np

from . import mvfile, mvjson
from .scanner import FrameBatch, MotionScanner, ScanParams


def load(path):
    """(FrameBatch, pts_seconds list with None for null) of an extract_mvs JSON or a .mtmv file."""
    with open(path, "rb") as fh:
        magic = fh.read(8)
    if magic == mvfile.MAGIC:
        hdr, tab, mv = mvfile.read_mtmv(path)
        frames = mvfile.frames_of(tab, mv)
        # the seconds extract_mvs would have printed: pts * time_base through %.6f (extract_mvs.cpp:122, 137)
        tb = float(hdr["tb_num"]) / float(hdr["tb_den"])
        pts = [float("%.6f" % (int(p) * tb)) for p in tab["pts"]]
    else:
        frames, pts, _ = mvjson.read_json(path)
    return FrameBatch.from_frames(frames), pts


def rows(scanner, batch, pts):
    """[(second, value)] for every second with at least one term, ascending."""
    acc, bin_terms = scanner.motion_scalar(batch, pts)
    return [(int(s), float(acc[s])) for s in np.nonzero(bin_terms)[0]]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mvtrim_amd.motion_scalar", description=__doc__.splitlines()[0])
    ap.add_argument("file", help="extract_mvs JSON or .mtmv")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        batch, pts = load(a.file)
    except (OSError, ValueError, KeyError) as e:
        print(f"motion_scalar: cannot read {a.file}: {e}", file=sys.stderr)
        return 1
    # the scan parameters play no part in this path: any valid block will do
    with MotionScanner(ScanParams.from_config(1920, 1080), device=a.device) as s:
        out = rows(s, batch, pts)
    print("second,motion_value")
    for sec, v in out:
        print("%d,%s" % (sec, "%g" % v))
    return 0


if __name__ == "__main__":
    sys.exit(main())
