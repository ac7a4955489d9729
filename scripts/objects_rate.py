#!/usr/bin/env python3
"""What the object scan costs (needs a GPU): mtgpu_scan_blobs_device — the yardstick, existing code — against
mtgpu_scan_objects_device with keep NULL at k = 1, 4 and 16, interleaved on the same device-resident batch in one
process and timed with the library's own events (mtgpu_profile_enable / mtgpu_profile_read: scan-kernel us per launch),
on the three batches of docs/rounds/r08_blobs.md (scripts/blobs_rate.py):
    baseline    1080p dense8x8 of synth.py, 4096 frames — about half of them hold a centre, in one small blob
    pan         the same stream with every record above the threshold: every frame with side data labels one blob of every cell
    serpentine  512 frames of the 4K grid that each hold one thin path of 14 817 cells
The script asserts, at every k, that entry 0 equals the blob scan's largest and box and that centres and blobs are its.
    python scripts/objects_rate.py [--rounds 5] [--steps 10] [--out profiles/objects_rate.json] [--markdown]"""
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
from mvtrim_amd import objects  # noqa: E402
import bench  # noqa: E402  (build_workload: the bench's own batches)

KS = (1, 4, 16)
MIN_BLOB = 4

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--out", default=None, help="also write the table to this JSON file")
ap.add_argument("--markdown", action="store_true", help="print the table of docs/rounds/r31_objects.md")
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
    """(scanner, d_mv, d_off, records): scripts/blobs_rate.py's batch — full rows 6, 8, .. 128 of columns 1 .. 238 joined at
    alternating ends, one vote per cell under VECTORS_NEEDED 1, the same frame `frames` times."""
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
    words = lambda: torch.empty(frames, dtype=torch.int32, device=dev)      # noqa: E731
    ref = {"centres": words(), "blobs": words(), "largest": words(), "flags": torch.empty(frames, dtype=torch.uint8, device=dev),
           "box": torch.empty((frames, 4), dtype=torch.int16, device=dev)}
    out = {k: {"centres": words(), "blobs": words(), "objects": words(), "flags": torch.empty(frames, dtype=torch.uint8, device=dev),
               "list": torch.empty((frames, k, 4), dtype=torch.int32, device=dev)} for k in KS}
    calls = {"blobs": lambda: s.scan_blobs_device(d_mv, d_off, None, MIN_BLOB, out=ref)}
    for k in KS:
        calls["objects_k%d" % k] = lambda k=k: objects.scan_device(s, d_mv, d_off, None, k, MIN_BLOB, 1, out=out[k])
    got = {n: [] for n in calls}
    for _ in range(a.rounds):                          # interleaved: blobs, k 1, k 4, k 16, blobs, ...
        for n, call in calls.items():
            got[n].append(timed(s, call))
    torch.cuda.synchronize()
    for call in calls.values():
        call()
    torch.cuda.synchronize()
    box = ref["box"].cpu().numpy().view(np.uint16)
    for k in KS:
        lst = out[k]["list"].cpu().numpy().view(objects.OBJECT_DTYPE)[..., 0]
        assert bool(torch.equal(ref["centres"], out[k]["centres"])) and bool(torch.equal(ref["blobs"], out[k]["blobs"])), k
        assert np.array_equal(lst["cells"][:, 0], ref["largest"].cpu().numpy().view(np.uint32)), "entry 0 is not the largest blob"
        assert np.array_equal(np.stack([lst[n][:, 0] for n in ("x0", "y0", "x1", "y1")], axis=1), box), "entry 0 is not the blob scan's box"
        assert bool(torch.equal(ref["flags"], out[k]["flags"])), "flags at min_objects 1 are not the blob scan's"
    row = {"batch": label, "workload": wl, "frames": frames, "records": n_records, "blobs_plan": m.blobs_preview(s.params),
           "objects_plan_k16": objects.preview(s.params, 16), "steps_per_round": a.steps, "entry_0_is_the_blob_scan": True,
           "frames_that_label": int((ref["blobs"] > 0).sum()), "blobs_sum": int(ref["blobs"].to(torch.int64).sum()),
           "blobs_max": int(ref["blobs"].max()), "largest_max": int(ref["largest"].max())}
    for n, v in got.items():
        row[n] = stat(v)
    for k in KS:
        row["objects_k%d_over_blobs" % k] = round(row["objects_k%d" % k]["median_us"] / row["blobs"]["median_us"], 4)
    rows.append(row)
    print(json.dumps(row), flush=True)
    s.close()
    del d_mv, d_off, ref, out
    if label != "serpentine":
        del w

if a.out:
    json.dump({"what": "scan-kernel us per launch (library events), steps_per_round launches per round, the four calls interleaved in "
                       "one process: mtgpu_scan_blobs_device with keep NULL and all five outputs (blobs: the yardstick) and "
                       "mtgpu_scan_objects_device with keep NULL and all five outputs at k = 1, 4, 16", "rows": rows},
              open(a.out, "w"), indent=1)
if a.markdown:
    print("| batch | frames | frames that label | blobs us (min-max) | " + " | ".join("k %d us (min-max) | k %d / blobs" % (k, k) for k in KS) + " |")
    print("|---|---|---|---|" + "---|---|" * len(KS))
    for r in rows:
        f = lambda n: "%.1f (%.1f-%.1f)" % (r[n]["median_us"], r[n]["min_us"], r[n]["max_us"])      # noqa: E731
        print("| %s | %d | %d | %s | " % (r["batch"], r["frames"], r["frames_that_label"], f("blobs")) +
              " | ".join("%s | %.3f" % (f("objects_k%d" % k), r["objects_k%d_over_blobs" % k]) for k in KS) + " |")
