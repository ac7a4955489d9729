#!/usr/bin/env python3
"""What the blob scan costs (needs a GPU): mtgpu_scan_centres_device — the yardstick, existing code — against
mtgpu_scan_blobs_device with keep NULL, interleaved on the same device-resident batch in one process and timed with the
library's own events (mtgpu_profile_enable / mtgpu_profile_read: scan-kernel us per launch), on
    baseline    the BASELINE-shaped stream: 1080p dense8x8 of synth.py, 4096 frames — about half of them hold a centre, in one small blob
    pan         the same stream with every record above the threshold: every frame with side data labels one blob of every cell
    serpentine  512 frames of the 4K grid that each hold one thin path of 14 817 cells (tests/blobs_inputs.py's shape)
The script asserts that the blob scan's `centres` equal the yardstick's counts, and reports how many frames labelled.
    python scripts/blobs_rate.py [--rounds 5] [--steps 10] [--out profiles/blobs_rate.json] [--markdown]"""
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
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--out", default=None, help="also write the table to this JSON file")
ap.add_argument("--markdown", action="store_true", help="print the table of docs/rounds/r08_blobs.md")
a = ap.parse_args()
dev = torch.device("cuda", 0)
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


def serpentine_batch(frames):
    """(scanner, d_mv, d_off, records): full rows 6, 8, .. 128 of columns 1 .. 238 joined at alternating ends, one vote
    per cell under VECTORS_NEEDED 1, the same frame `frames` times."""
    p = m.ScanParams.from_config(3840, 2160, vectors_needed=1)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (240, 135, 6)
    cells, right = [], True
    rows_ = list(range(6, 129, 2))
    for i, y in enumerate(rows_):
        cells += [(x, y) for x in range(1, 239)]
        if i + 1 < len(rows_):
            cells.append((238 if right else 1, y + 1))
            right = not right
    c = np.array(cells, dtype=np.int64)
    mv = np.zeros(len(c), dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"] = c[:, 0] * 16 + 8, c[:, 1] * 16 + 8
    mv["src_x"], mv["src_y"] = mv["dst_x"] - 5, mv["dst_y"]
    mv = mv[np.random.RandomState(3).permutation(len(mv))]
    d_mv = torch.from_numpy(mv.view(np.uint8).copy()).to(dev).repeat(frames).contiguous()
    d_off = torch.from_numpy(np.arange(frames + 1, dtype=np.int64) * len(mv)).to(dev)
    return m.MotionScanner(p, device=0), d_mv, d_off, len(mv) * frames


for label in ("baseline", "pan", "serpentine"):
    if label == "serpentine":
        frames = max(a.frames // 8, 1)
        s, d_mv, d_off, n_records = serpentine_batch(frames)
        wl = "4k serpentine"
    else:
        frames = a.frames
        if label == "pan":
            os.environ["AB_PAN"] = "1"
        try:
            w = bench.build_workload("1080p_dense8x8", "code_defaults", frames, 60, 1, dev)
        finally:
            os.environ.pop("AB_PAN", None)
        s, d_mv, d_off, n_records, wl = w["scanner"], w["d_mv"], w["d_off"], w["n_records"], "1080p_dense8x8"
    ref = torch.empty(frames, dtype=torch.int32, device=dev)
    out = {"centres": torch.empty(frames, dtype=torch.int32, device=dev), "blobs": torch.empty(frames, dtype=torch.int32, device=dev),
           "largest": torch.empty(frames, dtype=torch.int32, device=dev), "flags": torch.empty(frames, dtype=torch.uint8, device=dev),
           "box": torch.empty((frames, 4), dtype=torch.int16, device=dev)}
    calls = {"centres": lambda: s.count_centres_device(d_mv, d_off, None, flags=False, centres=ref),
             "blobs": lambda: s.scan_blobs_device(d_mv, d_off, None, 4, out=out)}
    got = {k: [] for k in calls}
    for _ in range(a.rounds):                          # interleaved: centres, blobs, centres, ...
        for k, call in calls.items():
            got[k].append(timed(s, call))
    torch.cuda.synchronize()
    calls["centres"]()
    calls["blobs"]()
    torch.cuda.synchronize()
    assert bool(torch.equal(ref, out["centres"])), "the blob scan does not return the centre scan's counts"
    row = {"batch": label, "workload": wl, "frames": frames, "records": n_records, "scan_plan": s.plan,
           "blobs_plan": m.blobs_preview(s.params), "steps_per_round": a.steps, "centres_are_the_scan": True,
           "frames_that_label": int((out["blobs"] > 0).sum()), "blobs_sum": int(out["blobs"].to(torch.int64).sum()),
           "largest_max": int(out["largest"].max()), "centre_sum": int(ref.to(torch.int64).sum())}
    for k, v in got.items():
        row[k] = stat(v)
    row["blobs_over_centres"] = round(row["blobs"]["median_us"] / row["centres"]["median_us"], 4)
    rows.append(row)
    print(json.dumps(row), flush=True)
    s.close()
    del d_mv, d_off
    if label != "serpentine":
        del w

if a.out:
    json.dump({"what": "scan-kernel us per launch (library events), steps_per_round launches per round, the two calls interleaved "
                       "in one process: mtgpu_scan_centres_device (centres: the yardstick) and mtgpu_scan_blobs_device with keep "
                       "NULL and all five outputs (blobs)", "rows": rows}, open(a.out, "w"), indent=1)
if a.markdown:
    print("| batch | frames | frames that label | centres us (min-max) | blobs us (min-max) | blobs / centres |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        f = lambda k: "%.1f (%.1f-%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])      # noqa: E731
        print("| %s | %d | %d | %s | %s | %.3f |" % (r["batch"], r["frames"], r["frames_that_label"], f("centres"), f("blobs"),
                                                     r["blobs_over_centres"]))
