#!/usr/bin/env python3
"""What a keep mask costs (needs a GPU): mtgpu_scan_centres_device — the yardstick, existing code — against
mtgpu_scan_zones_device with an all-ones mask, with half the cells cleared, with eight different per-stream masks, and
the last again with centres_all, interleaved in one process and timed with the library's own events
(mtgpu_profile_enable / mtgpu_profile_read: scan-kernel us per launch), on the headline batch (1080p dense8x8, 16 384
frames, 8 streams) and the 4K batch (4096 frames).  all-ones against half-cleared is what the mask costs; all-ones
against the yardstick is what the kernel form costs (one LDS atomic per record, no run pre-aggregation).  The script
asserts that the all-ones result equals the yardstick's counts.
    python scripts/zones_rate.py [--rounds 5] [--steps 10] [--out profiles/zones_rate.json] [--markdown]"""
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
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--streams", type=int, default=8)
ap.add_argument("--out", default=None, help="also write the table to this JSON file (profiles/zones_rate.json is one)")
ap.add_argument("--markdown", action="store_true", help="print the table of DESIGN.md 6")
a = ap.parse_args()
dev = torch.device("cuda", 0)
arena = torch.empty(bench.ARENA_BYTES, dtype=torch.uint8, device=dev)
rows = []
KINDS = ("centres", "ones", "half", "eight", "eight_all")


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


def keep_tensor(keeps):
    return torch.from_numpy(np.stack([zones.pack_keep(k) for k in keeps]).view(np.int64).copy()).to(dev)


for (label, wl, pn, frames) in (("headline", "1080p_dense8x8", "code_defaults", 16384), ("4k", "4k_dense8x8", "code_defaults", 4096)):
    w = bench.build_workload(wl, pn, frames, 60, 1, dev, arena=arena)
    s = w["scanner"]
    gh, gw = s.params.grid_h, s.params.grid_w
    rng = np.random.RandomState(17)
    soff = torch.from_numpy((np.arange(a.streams + 1, dtype=np.int64) * frames) // a.streams).to(dev)
    half = rng.rand(gh, gw) >= 0.5
    k_ones = keep_tensor(np.ones((a.streams, gh, gw), dtype=bool))
    k_half = keep_tensor(np.broadcast_to(half, (a.streams, gh, gw)))
    k_eight = keep_tensor(rng.rand(a.streams, gh, gw) >= 0.5)
    ref = torch.empty(frames, dtype=torch.int32, device=dev)
    ce = torch.empty(frames, dtype=torch.int32, device=dev)
    ca = torch.empty(frames, dtype=torch.int32, device=dev)

    def zone(keep, all_=False):
        return lambda: s.scan_zones_device(w["d_mv"], w["d_off"], None, soff, keep, flags=False, centres=ce,
                                           centres_all=ca if all_ else None)
    calls = {"centres": lambda: s.count_centres_device(w["d_mv"], w["d_off"], None, flags=False, centres=ref),
             "ones": zone(k_ones), "half": zone(k_half), "eight": zone(k_eight), "eight_all": zone(k_eight, True)}
    got = {k: [] for k in calls}
    for _ in range(a.rounds):                          # interleaved: centres, ones, half, eight, eight_all, centres, ...
        for k, call in calls.items():
            got[k].append(timed(s, call))
    torch.cuda.synchronize()
    calls["centres"]()
    calls["ones"]()
    torch.cuda.synchronize()
    assert bool(torch.equal(ref, ce)), "the all-ones mask does not return the centre scan's counts"
    ones_sum = int(ce.to(torch.int64).sum())
    calls["eight_all"]()
    torch.cuda.synchronize()
    assert bool(torch.equal(ref, ca)), "centres_all does not return the centre scan's counts"
    row = {"batch": label, "workload": wl, "params": pn, "frames": frames, "streams": a.streams, "records": w["n_records"],
           "scan_plan": s.plan, "zones_plan": m.zones_preview(s.params), "steps_per_round": a.steps, "all_ones_is_the_scan": True,
           "centre_sum": ones_sum, "centre_sum_eight_masks": int(ce.to(torch.int64).sum())}
    for k, v in got.items():
        row[k] = stat(v)
    for k in KINDS[1:]:
        row[k + "_over_centres"] = round(row[k]["median_us"] / row["centres"]["median_us"], 4)
    row["half_over_ones"] = round(row["half"]["median_us"] / row["ones"]["median_us"], 4)
    row["eight_all_over_eight"] = round(row["eight_all"]["median_us"] / row["eight"]["median_us"], 4)
    rows.append(row)
    print(json.dumps(row), flush=True)
    s.close()
    del w
del arena

if a.out:
    json.dump({"what": "scan-kernel us per launch (library events), 10 launches per round, five rounds, the five calls "
                       "interleaved in one process: mtgpu_scan_centres_device (centres: the yardstick) and "
                       "mtgpu_scan_zones_device with an all-ones mask (ones), half the cells cleared (half), eight different "
                       "per-stream masks (eight) and the same with centres_all (eight_all)", "rows": rows}, open(a.out, "w"), indent=1)
if a.markdown:
    print("| batch | frames | centres us (min-max) | all-ones | half cleared | eight masks | eight masks + centres_all | ones / centres | half / ones | all / eight |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda k: "%.1f (%.1f-%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])      # noqa: E731
        print("| %s | %d | %s | %s | %s | %s | %s | %.3f | %.3f | %.3f |" % (
            r["batch"], r["frames"], f("centres"), f("ones"), f("half"), f("eight"), f("eight_all"), r["ones_over_centres"],
            r["half_over_ones"], r["eight_all_over_eight"]))
