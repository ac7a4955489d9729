#!/usr/bin/env python3
"""What the box costs a submit (include/mtgpu_pipe_boxes.h): the blob pipe and the compensated blob (pair) pipe, each with
and without MT_LAYOUT_BOXES, zero-copy and copied staging — eight pipes in ONE process on one context.  A batch of 256
frames (the hot 1080p dense8x8 frames of host_pipeline_rate.py with one object of 6 x 4 cells added to every frame, so
every workgroup takes its kernel's final exit and the boxed forms run their box pass and store) is filled outside the
timed window; timed is mtgpu_pipe_submit -> mtgpu_pipe_collect, `--iters` times per leg and run; three runs, the legs
interleaved (blob zc, blob zc boxed, pair zc, pair zc boxed, blob copied, ...).  frames/s as median (min - max) per leg,
and the boxed leg against its unboxed one.  PCIe-inclusive; never the bench value.  Needs a GPU.  Prints one JSON document; `--out PATH` also writes it to a file
(profiles/pipe_boxes_rate.json is one)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mvtrim_amd as m  # noqa: E402
from mvtrim_amd import _abi, synth  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
ap.add_argument("--out", metavar="PATH", help="write the JSON document here as well")
ap.add_argument("--iters", type=int, default=40, help="timed submits per leg and run")
ap.add_argument("--frames", type=int, default=256, help="frames per batch")
args_ = ap.parse_args()

spec = synth.spec_1080p(seed=9)
spec.events = list(synth.scripted_events(spec, 150)) + [synth.Event(0, 1000, 40, 30, 6, 4, 9, 1)]   # one object in every frame
hot = [np.ascontiguousarray(synth.gen_frame(spec, 1 + i)) for i in range(12)]
F, runs = args_.frames, 3
params = m.ScanParams.from_config(1920, 1080)
s = m.MotionScanner(params, device=0)
lib = s._lib
max_rec = F * max(len(f) for f in hot)
ZC, BX = m.LAYOUT_ZERO_COPY, m.LAYOUT_BOXES
legs = {}
for stag, zc in (("zc", ZC), ("copied", 0)):
    for mode in ("blob", "pair"):
        for btag, bx in (("", 0), ("_boxed", BX)):
            pipe = m.ScanPipe(s, max_rec, F, 1, layout=m.LAYOUT_COMPACT8 | zc | bx)
            if mode == "blob":
                pipe.set_blobs(3)
            else:
                pipe.set_gmc_blobs(3)
            legs[f"{mode}_{stag}{btag}"] = pipe


def one_batch(pipe):
    """Fill a batch outside the timed window, then time submit -> collect.  Returns (seconds, flagged frames)."""
    b = C.c_void_p()
    _abi.check(lib.mtgpu_pipe_acquire(pipe._pipe, C.byref(b)))
    for i in range(F):
        a = hot[i % len(hot)]
        _abi.check(lib.mtgpu_batch_add_frame(b, a.ctypes.data_as(C.c_void_p), a.nbytes, 1, float(i), i))
    out, fl, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
    t0 = time.perf_counter()
    _abi.check(lib.mtgpu_pipe_submit(pipe._pipe, b))
    _abi.check(lib.mtgpu_pipe_collect(pipe._pipe, C.byref(out), C.byref(fl), None, None, C.byref(n)))
    dt = time.perf_counter() - t0
    flagged = int(np.ctypeslib.as_array(C.cast(fl, C.POINTER(C.c_uint8)), (n.value,)).sum())
    if pipe._boxes:
        bp = C.c_void_p()
        _abi.check(lib.mtgpu_batch_boxes(out, C.byref(bp)))
    _abi.check(lib.mtgpu_pipe_release(pipe._pipe, out))
    return dt, flagged


rates = {k: [] for k in legs}
flagged = {}
for name, pipe in legs.items():                       # warm-up: pins the block, loads the kernel
    one_batch(pipe)
for run in range(runs):
    for name, pipe in legs.items():
        total = 0.0
        for _ in range(args_.iters):
            dt, flagged[name] = one_batch(pipe)
            total += dt
        rates[name].append(F * args_.iters / total)
        print(f"run {run} {name:18s} {rates[name][-1]:10.0f} frames/s  ({flagged[name]} of {F} frames flagged)", flush=True)
out = {"what": f"submit -> collect of a prefilled batch of {F} hot 1080p dense8x8 frames ({np.mean([len(f) for f in hot]):.0f} records each), "
               f"compact staging, one batch in flight, {args_.iters} submits per leg and run, {runs} runs, legs interleaved, one process",
       "frames_per_batch": F, "flagged_frames": flagged, "pipes": {}}
for name, v in rates.items():
    q = sorted(v)
    out["pipes"][name] = {"frames_per_s": {"median": q[len(q) // 2], "min": q[0], "max": q[-1], "runs": v}}
for name in list(legs):
    if name.endswith("_boxed"):
        ref = name[:-len("_boxed")]
        out["pipes"][name]["against"] = ref
        out["pipes"][name]["median_vs_against_pct"] = 100.0 * (out["pipes"][name]["frames_per_s"]["median"] /
                                                               out["pipes"][ref]["frames_per_s"]["median"] - 1.0)
        f = out["pipes"][ref]["frames_per_s"]
        out["pipes"][ref]["spread_pct"] = 100.0 * (f["max"] - f["min"]) / f["median"]
for pipe in legs.values():
    pipe.close()
s.close()
print(json.dumps(out))
if args_.out:
    with open(args_.out, "w") as f:
        json.dump(out, f, indent=1)
