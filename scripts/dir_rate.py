#!/usr/bin/env python3
"""What the direction test and the rose cost (needs a GPU): mtgpu_scan_centres_device — the yardstick, existing code —
and mtgpu_scan_zones_device with an all-ones mask — the sibling with the same kernel form — against
mtgpu_scan_dir_device with every sector allowed, with half of them allowed, and the first again without the rose output,
on the same resident 1080p batch (dense8x8, 16 384 frames), as 40-byte and as compact records.  The legs are interleaved
in one process and timed with the library's own events (mtgpu_profile_enable / mtgpu_profile_read: scan-kernel us per
launch); three runs by default, the median with min - max per leg.  The script asserts that allow = all returns the
yardstick's counts and that the rose does not depend on the allow byte.
    python scripts/dir_rate.py [--rounds 3] [--steps 10] [--out profiles/dir_rate.json] [--markdown]"""
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
from mvtrim_amd import zones  # noqa: E402
import bench  # noqa: E402  (build_workload: the bench's own batches)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--frames", type=int, default=16384)
ap.add_argument("--out", default=None, help="also write the table to this JSON file (profiles/dir_rate.json is one)")
ap.add_argument("--markdown", action="store_true", help="print the table of docs/rounds/r20_direction.md")
a = ap.parse_args()
dev = torch.device("cuda", 0)
rows = []
KINDS = ("centres", "zones_ones", "dir_all", "dir_half", "dir_all_no_rose")
HALF = 0x1B                                            # E, SE, SW, W


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


w = bench.build_workload("1080p_dense8x8", "code_defaults", a.frames, 60, 1, dev)
s = w["scanner"]
frames = a.frames
gh, gw = s.params.grid_h, s.params.grid_w
rec8 = m.pack_records(w["mv"])
d_tile = torch.from_numpy(rec8.view(np.uint8).reshape(-1).copy()).to(dev)
d_rec8 = d_tile.repeat(w["reps"])[: w["n_records"] * 8].contiguous()
del d_tile
soff = torch.tensor([0, frames], dtype=torch.int64, device=dev)
k_ones = torch.from_numpy(zones.pack_keep(np.ones((gh, gw), dtype=bool)).view(np.int64).copy()).reshape(1, gh, -1).to(dev)
ref = torch.empty(frames, dtype=torch.int32, device=dev)
ce = torch.empty(frames, dtype=torch.int32, device=dev)
rose = torch.empty((frames, 8), dtype=torch.int32, device=dev)
rose_half = torch.empty((frames, 8), dtype=torch.int32, device=dev)

for label, d_rec, compact in (("40-byte", w["d_mv"], False), ("compact", d_rec8, True)):
    def direction(allow, out_rose):
        want = ("centres", "rose") if out_rose is not None else ("centres",)
        return lambda: s.scan_dir_device(d_rec, w["d_off"], None, allow=allow, compact=compact, want=want,
                                         out={"centres": ce, "rose": out_rose})
    calls = {"centres": lambda: s.count_centres_device(d_rec, w["d_off"], None, compact=compact, flags=False, centres=ref),
             "zones_ones": lambda: s.scan_zones_device(d_rec, w["d_off"], None, soff, k_ones, compact=compact, flags=False, centres=ce),
             "dir_all": direction(0xFF, rose), "dir_half": direction(HALF, rose_half), "dir_all_no_rose": direction(0xFF, None)}
    got = {k: [] for k in calls}
    for _ in range(a.rounds):                          # interleaved: centres, zones_ones, dir_all, dir_half, ..., centres, ...
        for k, call in calls.items():
            got[k].append(timed(s, call))
    torch.cuda.synchronize()
    calls["centres"]()
    calls["dir_half"]()
    half_sum = int(ce.to(torch.int64).sum())
    calls["dir_all"]()
    torch.cuda.synchronize()
    assert bool(torch.equal(ref, ce)), "allow = all does not return the centre scan's counts"
    assert bool(torch.equal(rose, rose_half)), "the rose depends on the allow byte"
    row = {"records": label, "workload": "1080p_dense8x8", "params": "code_defaults", "frames": frames, "n_records": w["n_records"],
           "scan_plan": s.plan, "dir_plan": m.dir_preview(s.params), "zones_plan": m.zones_preview(s.params),
           "steps_per_round": a.steps, "rounds": a.rounds, "all_is_the_scan": True, "centre_sum": int(ref.to(torch.int64).sum()),
           "centre_sum_half": half_sum, "rose_sum": [int(x) for x in rose.to(torch.int64).sum(dim=0).tolist()]}
    for k, v in got.items():
        row[k] = stat(v)
    for k in KINDS[1:]:
        row[k + "_over_centres"] = round(row[k]["median_us"] / row["centres"]["median_us"], 4)
    row["dir_all_over_zones_ones"] = round(row["dir_all"]["median_us"] / row["zones_ones"]["median_us"], 4)
    row["no_rose_over_dir_all"] = round(row["dir_all_no_rose"]["median_us"] / row["dir_all"]["median_us"], 4)
    rows.append(row)
    print(json.dumps(row), flush=True)
s.close()

if a.out:
    json.dump({"what": "scan-kernel us per launch (library events), %d launches per run, %d runs, the five legs interleaved in one "
                       "process on one resident batch: mtgpu_scan_centres_device (centres: the yardstick), mtgpu_scan_zones_device "
                       "with an all-ones mask (zones_ones) and mtgpu_scan_dir_device with every sector allowed (dir_all), with E, SE, "
                       "SW and W allowed (dir_half), and with every sector allowed and no rose output (dir_all_no_rose)"
                       % (a.steps, a.rounds), "rows": rows}, open(a.out, "w"), indent=1)
if a.markdown:
    print("| records | frames | centres us (min-max) | zones, all-ones | dir, all | dir, half | dir, all, no rose | dir / centres | dir / zones |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda k: "%.1f (%.1f-%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])      # noqa: E731
        print("| %s | %d | %s | %s | %s | %s | %s | %.3f | %.3f |" % (
            r["records"], r["frames"], f("centres"), f("zones_ones"), f("dir_all"), f("dir_half"), f("dir_all_no_rose"),
            r["dir_all_over_centres"], r["dir_all_over_zones_ones"]))
