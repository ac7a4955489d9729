#!/usr/bin/env python3
"""What the compensated blob scan costs (needs a GPU): mtgpu_scan_gmc_blobs_device against its two parents,
mtgpu_scan_gmc_device and mtgpu_scan_blobs_device, on the same resident 1080p dense8x8 batch, in both record layouts, on
the standard synthetic stream and on the pan stream (every record (9, 3): bench.build_workload's AB_PAN input) — the four
rows and the method of scripts/gmc_rate.py: the three calls interleaved in one process, timed with the library's own
events (mtgpu_profile_enable / mtgpu_profile_read: scan-kernel us per launch), median (min-max) of --rounds rounds of
--steps launches.  The script asserts consequences A and B of include/mtgpu_gmc_blobs.h on the batch it measures: at
max_shift 0 the five blob outputs are the blob scan's, and centres and info are the compensated scan's.  There is no pass
mark.

    python scripts/gmc_blobs_rate.py [--frames 4096] [--rounds 3] [--steps 5] [--out profiles/gmc_blobs_rate.json] [--markdown]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4096, help="frames of the resident batch")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--max-shift", type=int, default=16)
ap.add_argument("--min-share-q8", type=int, default=128)
ap.add_argument("--min-blob-cells", type=int, default=8)
ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
ap.add_argument("--markdown", action="store_true", help="print the table of docs/rounds/r13_gmc_blobs.md")
a = ap.parse_args()

import torch  # noqa: E402
import mvtrim_amd as m  # noqa: E402
import bench  # noqa: E402  (build_workload: the bench's own batches)

dev = torch.device("cuda", 0)
FRAMES = a.frames
NAMES = ("flags", "centres", "blobs", "largest", "box")


def build(kind):
    """The 1080p dense8x8 batch of the bench, 60 distinct frames tiled to FRAMES; kind "pan": every record (9, 3)."""
    old = os.environ.pop("AB_PAN", None)
    if kind == "pan":
        os.environ["AB_PAN"] = "1"
    try:
        w = bench.build_workload("1080p_dense8x8", "code_defaults", FRAMES, 60, 1, dev)
    finally:
        os.environ.pop("AB_PAN", None)
        if old is not None:
            os.environ["AB_PAN"] = old
    rec = m.pack_records(w["mv"])
    d_tile = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    w["d_rec8"] = d_tile.repeat(w["reps"])[: w["n_records"] * 8].contiguous()
    return w


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


rows = []
for kind in ("standard", "pan"):
    w = build(kind)
    s = w["scanner"]
    g_ce = torch.empty(FRAMES, dtype=torch.int32, device=dev)
    g_inf = torch.empty((FRAMES, 5), dtype=torch.int32, device=dev)
    for layout, compact, d_rec in (("aos40", False, w["d_mv"]), ("compact8", True, w["d_rec8"])):
        b_out, gb_out = {}, {}

        def gmc_call():
            return s.scan_gmc_device(d_rec, w["d_off"], None, a.max_shift, a.min_share_q8, compact=compact, flags=False, centres=g_ce,
                                     info=g_inf)

        def blobs_call():
            b_out.update(s.scan_blobs_device(d_rec, w["d_off"], None, a.min_blob_cells, compact=compact, out=b_out or None))

        def gmc_blobs_call(ms=a.max_shift):
            gb_out.update(s.scan_gmc_blobs_device(d_rec, w["d_off"], None, ms, a.min_share_q8, a.min_blob_cells, compact=compact,
                                                  out=gb_out or None))
        calls = {"gmc": gmc_call, "blobs": blobs_call, "gmc_blobs": gmc_blobs_call}
        got = {k: [] for k in calls}
        for _ in range(a.rounds):                      # interleaved: gmc, blobs, gmc_blobs, gmc, ...
            for k, call in calls.items():
                got[k].append(timed(s, call))
        torch.cuda.synchronize()
        blobs_call()
        gmc_blobs_call(0)
        torch.cuda.synchronize()
        for k in NAMES:
            assert bool(torch.equal(b_out[k], gb_out[k])), f"A: max_shift 0 does not return the blob scan's {k}"
        gmc_call()
        gmc_blobs_call()
        torch.cuda.synchronize()
        assert bool(torch.equal(g_ce, gb_out["centres"])) and bool(torch.equal(g_inf, gb_out["info"])), "B: centres / info differ"
        info = gb_out["info"].cpu().numpy().reshape(-1).view(m.GMC_INFO_DTYPE)
        ce = gb_out["centres"].cpu().numpy().view(np.uint32)
        row = {"input": kind, "layout": layout, "frames": FRAMES, "records": w["n_records"], "max_shift": a.max_shift,
               "min_share_q8": a.min_share_q8, "min_blob_cells": a.min_blob_cells, "plan": m.gmc_blobs_preview(s.params),
               "steps_per_round": a.steps, "frames_compensated": int(((info["gx"] != 0) | (info["gy"] != 0)).sum()),
               "frames_labelled": int((ce > 0).sum()), "centre_sum": int(ce.sum(dtype=np.uint64)),
               "blob_sum": int(gb_out["blobs"].cpu().numpy().view(np.uint32).sum(dtype=np.uint64)),
               "largest_max": int(gb_out["largest"].cpu().numpy().view(np.uint32).max()), "motion_frames": int(gb_out["flags"].sum())}
        for k, v in got.items():
            row[k] = stat(v)
        row["gmc_blobs_over_gmc"] = round(row["gmc_blobs"]["median_us"] / row["gmc"]["median_us"], 4)
        row["gmc_blobs_over_blobs"] = round(row["gmc_blobs"]["median_us"] / row["blobs"]["median_us"], 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    s.close()
    del w

if a.out:
    json.dump({"what": "scan-kernel us per launch (library events), the three calls interleaved in one process: "
                       "mtgpu_scan_gmc_device (gmc), mtgpu_scan_blobs_device (blobs) and mtgpu_scan_gmc_blobs_device (gmc_blobs)",
               "rows": rows}, open(a.out, "w"), indent=1)
if a.markdown:
    print("| input | layout | frames | gmc us (min-max) | blobs us (min-max) | gmc + blobs us (min-max) | / gmc | / blobs | frames labelled |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda k: "%.1f (%.1f-%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])      # noqa: E731
        print("| %s | %s | %d | %s | %s | %s | %.3f | %.3f | %d |" % (r["input"], r["layout"], r["frames"], f("gmc"), f("blobs"), f("gmc_blobs"),
                                                                     r["gmc_blobs_over_gmc"], r["gmc_blobs_over_blobs"], r["frames_labelled"]))
