#!/usr/bin/env python3
"""What the motion-scalar path reaches (needs a GPU): mtgpu_motion_scores_device against mtgpu_scan_frames_device on the
same resident buffer, interleaved in one process and timed with HIP events around each group of launches (planning
kernels included on both sides), on the headline batch and the 4K batch; then mtgpu_motion_bins_device on
64 streams x 2048 frames and on one stream of 10^6 frames.
    python scripts/motion_scalar_rate.py [--rounds 5] [--steps 10] [--out motion_scalar_rate.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mvtrim_amd as m  # noqa: E402
import bench  # noqa: E402  (build_workload: the bench's own batches)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--out", default=None, help="also write the table to this JSON file (profiles/motion_scalar_rate.json is one)")
a = ap.parse_args()
dev = torch.device("cuda", 0)


def event_us(call, reps):
    call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def summary(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


arena = torch.empty(bench.ARENA_BYTES, dtype=torch.uint8, device=dev)
rows = []
for (wl, pn, frames) in (("1080p_dense8x8", "code_defaults", 16384), ("4k_dense8x8", "code_defaults", 4096)):
    w = bench.build_workload(wl, pn, frames, 60, 1, dev, arena=arena)
    s = w["scanner"]
    n_records = (w["d_mv"].numel() * w["d_mv"].element_size()) // 40
    scores = torch.empty(frames, dtype=torch.float64, device=dev)
    terms = torch.empty(frames, dtype=torch.int32, device=dev)
    calls = {"scan": lambda: s.check_frames_device(w["d_mv"], w["d_off"], None, w["d_flags"]),
             "scores": lambda: s.motion_scores_device(w["d_mv"], w["d_off"], scores=scores, terms=terms)}
    got = {k: [] for k in calls}
    for _ in range(a.rounds):                          # interleaved: scan, scores, scan, ...
        for k, call in calls.items():
            got[k].append(event_us(call, a.steps))
    torch.cuda.synchronize()
    # every scale of the batch (the generated frames, tiled) a power of two <=> every wave instruction takes the reciprocal path
    sc = w["mv"]["motion_scale"].astype(np.int64)
    pow2 = bool(((sc & (sc - 1)) == 0).all())
    algo = 40 * n_records + (8 + 8 + 4) * frames
    row = {"workload": wl, "params": pn, "frames": frames, "records": n_records, "algorithmic_bytes": algo,
           "steps_per_round": a.steps, "all_scales_power_of_two": pow2,
           "score_sum": float(scores.sum().item()), "terms_sum": int(terms.to(torch.int64).sum().item())}
    for k, v in got.items():
        row[k + "_us"] = [round(x, 1) for x in v]
        row[k + "_us_summary"] = summary(v)
        row[k + "_GBps"] = round(algo / (statistics.median(v) * 1e-6) / 1e9, 1)
    row["scores_over_scan"] = round(statistics.median(got["scores"]) / statistics.median(got["scan"]), 4)
    rows.append(row)
    print(json.dumps(row), flush=True)
    s.close()
    del w
del arena

# ---- the bins: 64 streams x 2048 frames at 30 fps, and one stream of 10^6 frames
s = m.MotionScanner(m.ScanParams.from_config(1920, 1080))
bins = []
for S, per in ((64, 2048), (1, 10 ** 6)):
    n = S * per
    rng = np.random.RandomState(0)
    d_sc = torch.from_numpy(rng.random_sample(n) * 1e6).to(dev)
    d_tm = torch.from_numpy(rng.randint(0, 32400, size=n).astype(np.int32)).to(dev)
    d_pts = torch.from_numpy(np.concatenate([np.arange(per) / 30.0 for _ in range(S)])).to(dev)
    d_soff = torch.from_numpy(np.arange(S + 1, dtype=np.int64) * per).to(dev)
    n_sec = int(per / 30.0) + 1
    acc = torch.empty((S, n_sec), dtype=torch.float64, device=dev)
    bt = torch.empty((S, n_sec), dtype=torch.int64, device=dev)
    v = [event_us(lambda: s.motion_bins_device(d_sc, d_tm, d_pts, d_soff, n_sec, acc=acc, bin_terms=bt), a.steps)
         for _ in range(a.rounds)]
    row = {"streams": S, "frames_per_stream": per, "n_sec": n_sec, "bins_us": [round(x, 1) for x in v],
           "bins_us_summary": summary(v)}
    bins.append(row)
    print(json.dumps(row), flush=True)
s.close()
if a.out:
    json.dump({"what": "HIP-event us per call (planning kernels included), interleaved in one process: scan = "
                       "mtgpu_scan_frames_device, scores = mtgpu_motion_scores_device (scores + terms) on the same buffer; "
                       "GB/s over 40 N + 20 F bytes; bins = mtgpu_motion_bins_device into caller buffers",
               "scores": rows, "bins": bins}, open(a.out, "w"), indent=1)
