#!/usr/bin/env python3
"""Interleaved A/B of the current libmtgpu.so against a previous build (scripts/libmtgpu_prev.so) in ONE process, for
what ab_prev.py / ab_pan.py do not reach: compact records, grouped small frames, slices (flags compared).
Usage: ab_layouts.py workload params frames {aos40|compact} [slices]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["AB_PAN"] = "0"
import torch  # noqa: E402
import bench  # noqa: E402
import mvtrim_amd as m  # noqa: E402
from mvtrim_amd import scanner as sc  # noqa: E402

wl, pn, frames, layout = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
slices = int(sys.argv[5]) if len(sys.argv) > 5 else 0
dev = torch.device("cuda", 0)
w = bench.build_workload(wl, pn, frames, 60, 1000, dev)
lib = C.CDLL(os.path.join(ROOT, "scripts", "libmtgpu_prev.so"))
for name, (res, args) in m._abi.ABI.items():
    if hasattr(lib, name):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
orig = sc.load_library
sc.load_library = lambda: lib
try:
    other = m.MotionScanner(w["params"], 0)
finally:
    sc.load_library = orig
this = w["scanner"]
if slices:
    this.set_slices(slices)
    other.set_slices(slices)
if layout == "compact":
    rec = m.pack_records(w["mv"])
    d_tile = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    d_rec = d_tile.repeat(w["reps"])[: w["n_records"] * 8].contiguous()
    call = lambda s, fl: s.check_frames_device_compact(d_rec, w["d_off"], None, fl)
    nbytes = 8 * w["n_records"]
else:
    call = lambda s, fl: s.check_frames_device(w["d_mv"], w["d_off"], None, fl)
    nbytes = 40 * w["n_records"]
variants = [("new", this, []), ("prev", other, []), ("new2", this, []), ("prev2", other, [])]
fl = {n: torch.empty(frames, dtype=torch.uint8, device=dev) for n, _, _ in variants}
for r in range(42):
    for name, s, times in variants:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(s, fl[name]); e1.record(); torch.cuda.synchronize()
        if r >= 2:
            times.append(e0.elapsed_time(e1))
assert all(torch.equal(fl["new"], fl[n]) for n in fl), "flags differ between the builds"
print("plan:", this.plan, "slices asked:", slices, "motion frames", int(fl["new"].sum()))
for name, s, times in variants:
    t = np.array(times)
    print(f"{wl} {pn} {frames:6d} {layout:7s} {name:6s} median {np.median(t):.4f} ms  min {t.min():.4f}  {nbytes / np.median(t) / 1e6:7.0f} GB/s")
