#!/usr/bin/env python3
"""What the activity map costs (needs a GPU): mtgpu_scan_centres_device against mtgpu_activity_map_device with the
planner's run_frames and with run_frames = 1 (the naive design: every contributing frame flushes its masks), interleaved
in one process and timed with the library's own events (mtgpu_profile_enable / mtgpu_profile_read: scan-kernel us per
launch), on the headline batch (1080p dense8x8, 16 384 frames, 8 streams), the 4K batch (4096 frames), a sparse batch
(1080p, one vector per 16x16 block, scripted events) and the headline frames with every vector above the threshold
(every analysed cell active in every frame: the most a flush can cost).
    python scripts/activity_rate.py [--rounds 5] [--steps 10] [--out profiles/activity_rate.json] [--markdown]"""
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
ap.add_argument("--streams", type=int, default=8)
ap.add_argument("--out", default=None, help="also write the table to this JSON file (profiles/activity_rate.json is one)")
ap.add_argument("--markdown", action="store_true", help="print the table of DESIGN.md 6")
a = ap.parse_args()
dev = torch.device("cuda", 0)
arena = torch.empty(bench.ARENA_BYTES, dtype=torch.uint8, device=dev)
rows = []


def timed(s, call):
    call()
    s.profile(True)
    for _ in range(a.steps):
        call()
    pr = s.profile_read()
    s.profile(False)
    return pr["scan_ms"] * 1e3


def stat(v):
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
            "rounds_us": [round(x, 1) for x in v]}


for (label, wl, pn, frames, pan) in (("headline", "1080p_dense8x8", "code_defaults", 16384, False),
                                     ("4k", "4k_dense8x8", "code_defaults", 4096, False),
                                     ("sparse", "1080p_dense16", "code_defaults", 16384, False),
                                     ("every cell active", "1080p_dense8x8", "code_defaults", 16384, True)):
    if pan:
        os.environ["AB_PAN"] = "1"
    try:
        w = bench.build_workload(wl, pn, frames, 60, 1, dev, arena=arena)
    finally:
        os.environ.pop("AB_PAN", None)
    s = w["scanner"]
    centres = torch.empty(frames, dtype=torch.int32, device=dev)
    soff = torch.from_numpy((np.arange(a.streams + 1, dtype=np.int64) * frames) // a.streams).to(dev)
    gh, gw = s.params.grid_h, s.params.grid_w
    out = {"active": torch.empty((a.streams, gh, gw), dtype=torch.int32, device=dev),
           "centre": torch.empty((a.streams, gh, gw), dtype=torch.int32, device=dev),
           "frames": torch.empty(a.streams, dtype=torch.int32, device=dev)}
    calls = {"centres": lambda: s.count_centres_device(w["d_mv"], w["d_off"], None, flags=False, centres=centres),
             "map": lambda: s.activity_map_device(w["d_mv"], w["d_off"], None, soff, out=out),
             "map_run1": lambda: s.activity_map_device(w["d_mv"], w["d_off"], None, soff, run_frames=1, out=out)}
    got = {k: [] for k in calls}
    for _ in range(a.rounds):                          # interleaved: centres, map, map_run1, centres, ...
        for k, call in calls.items():
            got[k].append(timed(s, call))
    torch.cuda.synchronize()
    # the two map forms agree with each other and with the scan's counts
    calls["map"]()
    ref = {k: v.clone() for k, v in out.items()}
    calls["map_run1"]()
    calls["centres"]()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(ref[k], out[k])) for k in out)
    cs = centres.to(torch.int64)
    sums = [int(cs[int(soff[i]):int(soff[i + 1])].sum()) for i in range(a.streams)]
    same = same and sums == [int(out["centre"][i].to(torch.int64).sum()) for i in range(a.streams)]
    row = {"batch": label, "workload": wl, "params": pn, "frames": frames, "streams": a.streams, "records": w["n_records"],
           "scan_plan": s.plan, "activity_plan": m.activity_preview(s.params), "steps_per_round": a.steps,
           "maps_agree": same, "active_sum": int(out["active"].to(torch.int64).sum()),
           "centre_sum": int(out["centre"].to(torch.int64).sum())}
    for k, v in got.items():
        row[k] = stat(v)
    row["map_over_centres"] = round(row["map"]["median_us"] / row["centres"]["median_us"], 4)
    row["run1_over_map"] = round(row["map_run1"]["median_us"] / row["map"]["median_us"], 4)
    rows.append(row)
    print(json.dumps(row), flush=True)
    s.close()
    del w
del arena

if a.out:
    json.dump({"what": "scan-kernel us per launch (library events), 10 launches per round, five rounds, the three calls "
                       "interleaved in one process: mtgpu_scan_centres_device (centres only), mtgpu_activity_map_device "
                       "with the planner's run_frames (map) and with run_frames = 1 (map_run1: every contributing frame "
                       "flushes)", "rows": rows}, open(a.out, "w"), indent=1)
if a.markdown:
    print("| batch | frames | acc_bits | centres us (min-max) | map us (min-max) | map, run_frames 1 us (min-max) | map / centres | run 1 / map |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda k: "%.1f (%.1f-%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])      # noqa: E731
        print("| %s | %d | %d | %s | %s | %s | %.3f | %.3f |" % (r["batch"], r["frames"], r["activity_plan"]["acc_bits"],
                                                             f("centres"), f("map"), f("map_run1"), r["map_over_centres"],
                                                             r["run1_over_map"]))
