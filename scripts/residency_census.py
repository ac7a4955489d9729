#!/usr/bin/env python3
"""How many scan workgroups share a CU, read off launch times alone: 1080p dense8x8 P-frames of equal size (no key
frames: every frame is the same 1.3 MB of records, one workgroup each), scan-kernel time by the library's own profile
events (mean of 20 launches) at 768, 769, 1024 and 1025 frames.  The idea: a chip of 256 CUs with THREE workgroups per CU
has 768 slots, so frame 769 runs alone after the rest and the time steps up after 768; with FOUR per CU (1024 slots) it
steps up after 1024 instead.  Timing only: no workgroup waits for another.
What it shows in fact (docs/rounds/r22_scan_residency.md): the launch is bound by memory bandwidth, not by slots, and
the time steps up after EVERY multiple of the CU count (try --counts 255 256 257 512 513 ...), at any residency.  Two
builds that differ in residency show it as a difference that begins where the smaller one runs out of slots; that, and
the time per launch size against another build (--lib), is what the script is for.
Usage: python scripts/residency_census.py [--lib OTHER/libmtgpu.so ...] [--rounds 5] [--counts N ...]
Every --lib is another build of the library (say, the parent commit's) measured next to the tree's own, round-robin in
one process.  (needs a GPU)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mvtrim_amd as m  # noqa: E402
from mvtrim_amd import scanner as sc  # noqa: E402
from mvtrim_amd import synth  # noqa: E402

COUNTS = (768, 769, 1024, 1025)
LAUNCHES = 20


def scanner_of(path, params):
    """A scanner on another build of the library (the Python layer talks to whatever load_library returns)."""
    if path is None:
        return m.MotionScanner(params, 0)
    lib = C.CDLL(path)
    for name, (res, args) in m._abi.ABI.items():
        if hasattr(lib, name):
            getattr(lib, name).restype = res
            getattr(lib, name).argtypes = args
    orig = sc.load_library
    sc.load_library = lambda: lib
    try:
        return m.MotionScanner(params, 0)
    finally:
        sc.load_library = orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="another libmtgpu.so to measure next to the tree's")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--counts", type=int, nargs="*", default=list(COUNTS))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    distinct = 30
    spec = synth.spec_1080p(seed=1, sub=2)
    spec.gop = 0                                        # P-frames only
    spec.events = synth.scripted_events(spec, distinct)
    mv, off, _, sd = synth.gen_stream(spec, distinct)
    per = np.diff(off.astype(np.int64))
    assert sd.all() and (per == per[0]).all(), "frames of equal size, all with side data"
    params = m.ScanParams.from_config(1920, 1080, **dict(m.config.CODE_DEFAULTS))
    top = max(a.counts)
    reps = (top + distinct - 1) // distinct
    d_mv = torch.from_numpy(mv.view(np.uint8).copy()).to(dev).repeat(reps)[: top * int(per[0]) * 40].contiguous()
    d_off = torch.from_numpy(np.arange(top + 1, dtype=np.int64) * int(per[0])).to(dev)
    d_flags = torch.empty(top, dtype=torch.uint8, device=dev)
    builds = [("tree", scanner_of(None, params))] + [(p, scanner_of(p, params)) for p in a.lib]
    ms = {(name, n): [] for name, _ in builds for n in a.counts}
    for _ in range(a.rounds):
        for name, s in builds:
            for n in a.counts:
                o, f = d_off[: n + 1], d_flags[:n]
                for _ in range(3):
                    s.check_frames_device(d_mv, o, None, f)
                s.profile(True)
                for _ in range(LAUNCHES):
                    s.check_frames_device(d_mv, o, None, f)
                pr = s.profile_read()
                s.profile(False)
                assert pr["launches"] == LAUNCHES
                ms[(name, n)].append(pr["scan_ms"])
    torch.cuda.synchronize()
    for name, s in builds:
        p = s.plan
        print(f"{name}: block={p['block_threads']} counter_bits={p['counter_bits']} lds={p['lds_bytes']} cus={p['cu_count']} "
              f"frame={int(per[0]) * 40} bytes")
        row = {}
        for n in a.counts:
            t = np.array(ms[(name, n)])
            row[n] = float(np.median(t))
            print(f"  {n:5d} frames  scan kernel median {np.median(t) * 1e3:8.1f} us  (min {t.min() * 1e3:8.1f}, max {t.max() * 1e3:8.1f},"
                  f" {a.rounds} x mean of {LAUNCHES})")
        if all(n in row for n in COUNTS):
            print(f"  step 768 -> 769: {(row[769] - row[768]) * 1e3:+7.1f} us    step 1024 -> 1025: {(row[1025] - row[1024]) * 1e3:+7.1f} us")
        print("CENSUS " + json.dumps({"build": name, "scan_ms": {str(n): row[n] for n in a.counts}}))
        s.close()


if __name__ == "__main__":
    main()
