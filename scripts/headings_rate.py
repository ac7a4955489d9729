#!/usr/bin/env python3
"""What the heading scan costs (needs a GPU): mtgpu_scan_objects_device — the yardstick, existing code — against
mtgpu_scan_headings_device at k = 1, 4 and 16, keep NULL, all outputs, interleaved on the same device-resident batch in
one process and timed with the library's own HIP events (mtgpu_profile_enable / mtgpu_profile_read: scan-kernel us per
launch), five rounds, median (min - max), for 40-byte and for 8-byte records, on three batches:
    quiet      1080p frames of 8160 records that all lie below the threshold: no frame has a centre, so no workgroup
               streams its records a second time
    bench      1080p dense8x8 of synth.py, the bench's batch — about half of the frames hold a centre, in one small blob
    busy       1080p frames of 8160 records of which 6000 land in one blob of 30 x 20 cells (ten per cell): every frame
               labels, and most records belong to entry 0 — the LDS adds of a wave mostly hit one entry's words
The script asserts consequence A of include/mtgpu_headings.h on every input: centres, blobs, objects and list are the
object scan's, and with every sector allowed so are the flags.
    python scripts/headings_rate.py [--rounds 5] [--steps 10] [--out profiles/headings_rate.json] [--markdown]"""
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
from mvtrim_amd import headings, objects  # noqa: E402
import bench  # noqa: E402  (build_workload: the bench's own batch)

KS = (1, 4, 16)
MIN_BLOB = 4

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--frames", type=int, default=2048)
ap.add_argument("--out", default=None, help="also write the table to this JSON file")
ap.add_argument("--markdown", action="store_true", help="print the table of docs/rounds/r34_headings.md")
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


def grid_frame(busy):
    """One 1080p frame of 8160 records, one per cell of the 120 x 68 grid, shuffled.  quiet: dst - src = (1, 0), below
    the threshold of 16.  busy: the records of 6000 cells are moved into the 30 x 20 cells at (40, 20), ten per cell,
    with dst - src = (6, 0) +- 1."""
    rng = np.random.RandomState(9)
    gx, gy = np.meshgrid(np.arange(120), np.arange(68))
    gx, gy = gx.reshape(-1), gy.reshape(-1)
    dx, dy = np.ones(8160, dtype=np.int64), np.zeros(8160, dtype=np.int64)
    if busy:
        gx[:6000], gy[:6000] = 40 + np.arange(6000) % 30, 20 + (np.arange(6000) // 30) % 20
        dx[:6000], dy[:6000] = 6 + rng.randint(-1, 2, 6000), rng.randint(-1, 2, 6000)
    mv = np.zeros(8160, dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"] = gx * 16 + 8, gy * 16 + 8
    mv["src_x"], mv["src_y"] = mv["dst_x"] - dx, mv["dst_y"] - dy
    return mv[rng.permutation(8160)]


def batches():
    """(label, workload, scanner, host records [N] MV_DTYPE, d_off, frames)"""
    p = m.ScanParams.from_config(1920, 1080, mv_threshold_sq=16.0, vectors_needed=2, clusters_needed=1)
    for label in ("quiet", "busy"):
        frames = max(a.frames // 2, 1)
        mv = np.tile(grid_frame(label == "busy").view(np.uint8), frames).view(m.MV_DTYPE)
        d_off = torch.from_numpy(np.arange(frames + 1, dtype=np.int64) * 8160).to(dev)
        yield label, "1080p grid frame", m.MotionScanner(p, device=0), mv, d_off, frames
    w = bench.build_workload("1080p_dense8x8", "code_defaults", a.frames, 60, 1, dev)
    mv = w["d_mv"].cpu().numpy().view(np.uint8).reshape(-1).view(m.MV_DTYPE)
    yield "bench", "1080p_dense8x8", w["scanner"], mv, w["d_off"], a.frames


for label, wl, s, mv, d_off, frames in batches():
    for compact in (False, True):
        raw = (m.pack_records(mv) if compact else mv).view(np.uint8).reshape(-1)
        d_rec = torch.from_numpy(np.ascontiguousarray(raw)).to(dev)
        words = lambda: torch.empty(frames, dtype=torch.int32, device=dev)      # noqa: E731
        ref = {k: {"centres": words(), "blobs": words(), "objects": words(), "flags": torch.empty(frames, dtype=torch.uint8, device=dev),
                   "list": torch.empty((frames, k, 4), dtype=torch.int32, device=dev)} for k in KS}
        out = {k: dict({n: torch.empty_like(t) for n, t in ref[k].items()}, allowed=words(),
                       motion=torch.empty((frames, k, headings.HEADING_WORDS), dtype=torch.int32, device=dev)) for k in KS}
        calls = {}
        for k in KS:
            calls["objects_k%d" % k] = lambda k=k: objects.scan_device(s, d_rec, d_off, None, k, MIN_BLOB, 1, compact=compact, out=ref[k])
            calls["headings_k%d" % k] = lambda k=k: headings.scan_device(s, d_rec, d_off, None, k, MIN_BLOB, 1, 0xFF, compact=compact, out=out[k])
        got = {n: [] for n in calls}
        for _ in range(a.rounds):                          # interleaved: objects k 1, headings k 1, objects k 4, ...
            for n, call in calls.items():
                got[n].append(timed(s, call))
        torch.cuda.synchronize()
        for call in calls.values():
            call()
        torch.cuda.synchronize()
        for k in KS:                                       # consequence A (and B's flags: every sector is allowed)
            for n in ("centres", "blobs", "objects", "list", "flags"):
                assert bool(torch.equal(ref[k][n], out[k][n])), (label, compact, k, n)
        mo = out[16]["motion"].cpu().numpy().view(headings.HEADING_DTYPE)[..., 0]
        row = {"batch": label, "workload": wl, "rec_bytes": 8 if compact else 40, "frames": frames, "records": int(len(mv)),
               "objects_plan_k16": objects.preview(s.params, 16), "headings_plan_k16": headings.preview(s.params, 16),
               "steps_per_round": a.steps, "consequence_a_holds": True, "frames_that_label": int((ref[16]["blobs"] > 0).sum()),
               "belonging_records_k16": int(mo["records"].sum(dtype=np.uint64))}
        for n, v in got.items():
            row[n] = stat(v)
        for k in KS:
            row["headings_k%d_over_objects" % k] = round(row["headings_k%d" % k]["median_us"] / row["objects_k%d" % k]["median_us"], 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d_rec, ref, out
    s.close()

if a.out:
    json.dump({"what": "scan-kernel us per launch (library HIP events), steps_per_round launches per round, the six calls interleaved "
                       "in one process: mtgpu_scan_objects_device (the yardstick) and mtgpu_scan_headings_device with keep NULL and "
                       "all outputs at k = 1, 4, 16", "rows": rows}, open(a.out, "w"), indent=1)
if a.markdown:
    print("| batch | record | frames that label | " + " | ".join("objects k %d us | headings k %d us (min-max) | ratio" % (k, k) for k in KS) + " |")
    print("|---|---|---|" + "---|---|---|" * len(KS))
    for r in rows:
        f = lambda n: "%.1f (%.1f-%.1f)" % (r[n]["median_us"], r[n]["min_us"], r[n]["max_us"])      # noqa: E731
        print("| %s | %d | %d of %d | " % (r["batch"], r["rec_bytes"], r["frames_that_label"], r["frames"]) +
              " | ".join("%.1f | %s | %.3f" % (r["objects_k%d" % k]["median_us"], f("headings_k%d" % k), r["headings_k%d_over_objects" % k])
                         for k in KS) + " |")
