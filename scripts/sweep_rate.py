#!/usr/bin/env python3
"""What the setting sweep costs (needs a GPU): mtgpu_scan_sweep_device at 1x1, 4x1, 1x4, 4x4 and 8x8 (thresholds x vector
levels) against mtgpu_scan_centres_device on the same resident buffers, interleaved in one process and timed with the
library's own event triples (mtgpu_profile_enable / mtgpu_profile_read), on the headline batch (1080p dense8x8, 16 384
frames) and the 4K batch.  A sweep of T x V settings replaces T x V contexts and scans (T scans when only the threshold
varies between contexts that each answer one vector level): both products are reported.
    python scripts/sweep_rate.py [--rounds 5] [--steps 10] [--out profiles/sweep_rate.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mvtrim_amd as m  # noqa: E402
import bench  # noqa: E402  (build_workload: the bench's own batches)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--out", default=None, help="also write the table to this JSON file (profiles/sweep_rate.json is one)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
arena = torch.empty(bench.ARENA_BYTES, dtype=torch.uint8, device=dev)

THRESHOLDS = [1.0, 4.0, 16.0, 50.0, 2.0, 9.0, 25.0, 100.0]
VECTORS = [1, 2, 4, 8, 3, 5, 6, 16]
SHAPES = [(1, 1), (4, 1), (1, 4), (4, 4), (8, 8)]


def timed(s, call):
    call()
    s.profile(True)
    for _ in range(a.steps):
        call()
    pr = s.profile_read()
    s.profile(False)
    return pr["scan_ms"] * 1e3, pr["plan_ms"] * 1e3


def summary(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


rows = []
for (wl, pn, frames) in (("1080p_dense8x8", "code_defaults", 16384), ("4k_dense8x8", "code_defaults", 4096)):
    w = bench.build_workload(wl, pn, frames, 60, 1, dev, arena=arena)
    s = w["scanner"]
    n_records = (w["d_mv"].numel() * w["d_mv"].element_size()) // 40
    centres = torch.empty(frames, dtype=torch.int32, device=dev)
    out = torch.empty(8 * 8 * frames, dtype=torch.int32, device=dev)
    calls = {"centres": lambda: s.count_centres_device(w["d_mv"], w["d_off"], None, flags=False, centres=centres)}
    for (t, v) in SHAPES:
        calls["sweep_%dx%d" % (t, v)] = (lambda t=t, v=v: s.sweep_centres_device(w["d_mv"], w["d_off"], None, THRESHOLDS[:t],
                                                                                 VECTORS[:v], out=out[:t * v * frames]))
    got = {k: [] for k in calls}
    for _ in range(a.rounds):                          # interleaved: centres, 1x1, 4x1, ..., centres, ...
        for k, call in calls.items():
            got[k].append(timed(s, call))
    torch.cuda.synchronize()
    row = {"workload": wl, "params": pn, "frames": frames, "records": n_records, "record_bytes": 40 * n_records,
           "plan": s.plan, "steps_per_round": a.steps, "rounds": a.rounds}
    scan = statistics.median(x[0] for x in got["centres"])
    for k, v in got.items():
        row[k + "_scan_us"] = [round(x[0], 1) for x in v]
        row[k + "_plan_us"] = [round(x[1], 1) for x in v]
        row[k + "_scan_us_summary"] = summary([x[0] for x in v])
    for (t, v) in SHAPES:
        k = "sweep_%dx%d" % (t, v)
        med = statistics.median(x[0] for x in got[k])
        row[k + "_plan"] = m.sweep_preview(s.params, t, v)
        row[k + "_over_one_scan"] = round(med / scan, 3)
        row[k + "_over_T_scans"] = round(med / (t * scan), 3)              # one context per threshold
        row[k + "_over_TxV_scans"] = round(med / (t * v * scan), 3)        # one context per setting
        row[k + "_record_GBps"] = round(row[k + "_plan"]["passes"] * 40 * n_records / (med * 1e-6) / 1e9, 1)
    row["centres_record_GBps"] = round(40 * n_records / (scan * 1e-6) / 1e9, 1)
    rows.append(row)
    print(json.dumps(row), flush=True)
    s.close()
    del w
del arena
if a.out:
    json.dump({"what": "scan-phase us per call (library event triples: planning kernels excluded, every pass of a sweep "
                       "included), interleaved in one process: centres = mtgpu_scan_centres_device (counts only) through the "
                       "batch's own context, sweep_TxV = mtgpu_scan_sweep_device with T thresholds and V vector levels on the "
                       "same buffers; *_over_T_scans / *_over_TxV_scans: the sweep's median over T (T x V) times the plain "
                       "scan's median — below 1 the sweep is cheaper than that many contexts; *_record_GBps: passes x 40 N "
                       "bytes over the median",
               "rows": rows}, open(a.out, "w"), indent=1)
