#!/usr/bin/env python3
"""What the per-cell allow byte and the flow map cost (needs a GPU): mtgpu_scan_dir_device with every sector allowed — the
yardstick, existing code — against mtgpu_scan_lanes_device with a uniform 0xFF plane (the staged form on 1080p: the
plane's analysed rows are copied into LDS per frame) and mtgpu_flow_map_device (one global atomic per counting record
with a sector), on the same resident 1080p batch (dense8x8, 16 384 frames), as 40-byte and as compact records.  The legs
are interleaved in one process and timed with the library's own events (mtgpu_profile_enable / mtgpu_profile_read:
scan-kernel us per launch); three runs by default, the median with min - max per leg.  The script asserts that the
uniform plane returns the direction scan's counts and roses and that the flow map's sums are the roses' sums.
With AB_PAN=1 in the environment bench.build_workload makes the batch vote-heavy (scripts/ab_pan.py's input: every
record above the threshold): there every record pays the byte read, and the flow map an atomic.
    python scripts/lanes_rate.py [--workload 1080p_dense8x8] [--frames N] [--rounds 3] [--steps 10] [--out profiles/lanes_rate.json] [--markdown]"""
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
ap.add_argument("--workload", default="1080p_dense8x8", help="a workload of bench.py")
ap.add_argument("--params", default="code_defaults")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--frames", type=int, default=16384)
ap.add_argument("--reverse", action="store_true", help="run the legs of a round in the opposite order (what the order itself costs)")
ap.add_argument("--out", default=None, help="also write the table to this JSON file (profiles/lanes_rate.json is one)")
ap.add_argument("--markdown", action="store_true", help="print the table of docs/rounds/r25_lanes.md")
a = ap.parse_args()
dev = torch.device("cuda", 0)
rows = []
KINDS = ("dir_all", "lanes_all", "lanes_all_no_rose", "flow_map")


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


w = bench.build_workload(a.workload, a.params, a.frames, 60, 1, dev)
s = w["scanner"]
frames = a.frames
gh, gw = s.params.grid_h, s.params.grid_w
rec8 = m.pack_records(w["mv"])
d_tile = torch.from_numpy(rec8.view(np.uint8).reshape(-1).copy()).to(dev)
d_rec8 = d_tile.repeat(w["reps"])[: w["n_records"] * 8].contiguous()
del d_tile
soff = torch.tensor([0, frames], dtype=torch.int64, device=dev)
plane = torch.full((gh, gw), 0xFF, dtype=torch.uint8, device=dev)
ref = {"centres": torch.empty(frames, dtype=torch.int32, device=dev), "rose": torch.empty((frames, 8), dtype=torch.int32, device=dev)}
got_out = {"centres": torch.empty(frames, dtype=torch.int32, device=dev), "rose": torch.empty((frames, 8), dtype=torch.int32, device=dev)}
flow = torch.empty((1, 8, gh, gw), dtype=torch.int32, device=dev)

for label, d_rec, compact in (("40-byte", w["d_mv"], False), ("compact", d_rec8, True)):
    calls = {"dir_all": lambda: s.scan_dir_device(d_rec, w["d_off"], None, allow=0xFF, compact=compact, want=("centres", "rose"), out=ref),
             "lanes_all": lambda: s.scan_lanes_device(d_rec, w["d_off"], None, plane, compact=compact, want=("centres", "rose"), out=got_out),
             "lanes_all_no_rose": lambda: s.scan_lanes_device(d_rec, w["d_off"], None, plane, compact=compact, want=("centres",),
                                                              out={"centres": got_out["centres"]}),
             "flow_map": lambda: s.flow_map_device(d_rec, w["d_off"], None, soff, compact=compact, out=flow)}
    got = {k: [] for k in calls}
    for _ in range(a.rounds):                          # interleaved: dir_all, lanes_all, lanes_all_no_rose, flow_map, dir_all, ...
        for k in (reversed(list(calls)) if a.reverse else list(calls)):
            got[k].append(timed(s, calls[k]))
    torch.cuda.synchronize()
    calls["dir_all"]()
    calls["lanes_all"]()
    calls["flow_map"]()
    torch.cuda.synchronize()
    assert bool(torch.equal(ref["centres"], got_out["centres"])), "a plane of 0xFF does not return the direction scan's counts"
    assert bool(torch.equal(ref["rose"], got_out["rose"])), "a plane of 0xFF does not return the direction scan's roses"
    rose_sum = [int(x) for x in ref["rose"].to(torch.int64).sum(dim=0).tolist()]
    assert [int(x) for x in flow[0].to(torch.int64).sum(dim=(1, 2)).tolist()] == rose_sum, "the flow map's sums are not the roses' sums"
    row = {"records": label, "workload": a.workload, "params": a.params, "frames": frames, "n_records": w["n_records"],
           "scan_plan": s.plan, "dir_plan": m.dir_preview(s.params), "lanes_plan": m.lanes_preview(s.params),
           "steps_per_round": a.steps, "rounds": a.rounds, "centre_sum": int(ref["centres"].to(torch.int64).sum()), "rose_sum": rose_sum,
           "flow_adds_per_launch": sum(rose_sum), "flow_cells_touched": int((flow != 0).sum())}
    for k, v in got.items():
        row[k] = stat(v)
    for k in KINDS[1:]:
        row[k + "_over_dir_all"] = round(row[k]["median_us"] / row["dir_all"]["median_us"], 4)
    rows.append(row)
    print(json.dumps(row), flush=True)
s.close()

if a.out:
    json.dump({"what": "scan-kernel us per launch (library events), %d launches per run, %d runs, the four legs interleaved in one "
                       "process on one resident batch: mtgpu_scan_dir_device with every sector allowed (dir_all: the yardstick), "
                       "mtgpu_scan_lanes_device with a uniform 0xFF plane with and without the rose output (lanes_all, "
                       "lanes_all_no_rose) and mtgpu_flow_map_device over one stream (flow_map)" % (a.steps, a.rounds), "rows": rows},
              open(a.out, "w"), indent=1)
if a.markdown:
    print("| records | frames | dir, all us (min-max) | lanes, 0xFF plane | lanes, no rose | flow map | lanes / dir | flow / dir |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda k: "%.1f (%.1f-%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])      # noqa: E731
        print("| %s | %d | %s | %s | %s | %s | %.3f | %.3f |" % (
            r["records"], r["frames"], f("dir_all"), f("lanes_all"), f("lanes_all_no_rose"), f("flow_map"),
            r["lanes_all_over_dir_all"], r["flow_map_over_dir_all"]))
