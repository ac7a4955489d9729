#!/usr/bin/env python3
"""What the tracks call costs (needs a GPU): mtgpu_track_objects_device at k = 1, 4 and 16 against the unchanged
mtgpu_persist_flags_device on the same flags and the boxes of entry 0 — the kernel with the same launch shape, one
workgroup per stream — on (a) 64 streams x 256 frames and (b) one stream of 16 384 frames.  The calls are interleaved in
one process; a round is the HIP-event time of --steps back-to-back calls; reported in us per call as the median over
the rounds with min and max.  Two list shapes per input: `movers` (up to four wandering objects that come and go: short
tracks, many roots) and `one_track` (entry 0 links every frame to the one before: ONE id for a whole stream, the case in
which every depth update lands on one address).  Consequence A of include/mtgpu_tracks.h is asserted at k = 1 on the way.
Last comes the tracks call as a share of mtgpu_scan_objects_device on the 1080p 4096-frame batch of scripts/objects_rate.py.

    python scripts/tracks_rate.py [--rounds 5] [--steps 20] [--out profiles/tracks_rate.json] [--markdown]"""
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
from mvtrim_amd import objects, tracks  # noqa: E402

KS = (1, 4, 16)
SHAPES = (("64x256", 64, 256), ("1x16384", 1, 16384))
OBJ = objects.OBJECT_DTYPE
EMPTY = (0, 0xFFFFFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF)


def movers_lists(rng, n, k):
    """OBJECT_DTYPE [n, k], ranked as the object scan ranks: up to four objects wander two cells a frame at most, each
    visible in bursts, sizes 2 .. 9."""
    li = np.empty((n, k), dtype=OBJ)
    li[...] = EMPTY
    cells = np.zeros((n, 4), dtype=np.int64)
    boxes = np.zeros((n, 4, 4), dtype=np.int64)
    for o in range(4):
        x = np.clip(20 + 25 * o + np.cumsum(rng.randint(-2, 3, size=n)), 0, 110)
        y = np.clip(10 + 12 * o + np.cumsum(rng.randint(-1, 2, size=n)), 0, 60)
        seen = np.repeat(rng.random_sample(n // 24 + 1) < 0.6, 24)[:n]
        cells[:, o] = np.where(seen, rng.randint(2, 10, size=n), 0)
        boxes[:, o] = np.stack([x, y, x + 3, y + 2], axis=1)
    order = np.argsort(-cells, axis=1, kind="stable")
    for j in range(min(k, 4)):
        pick = order[:, j]
        c = cells[np.arange(n), pick]
        b = boxes[np.arange(n), pick]
        li["cells"][:, j] = c
        li["first"][:, j] = np.where(c > 0, b[:, 1] * 120 + b[:, 0], 0xFFFFFFFF)
        for i, name in enumerate(("x0", "y0", "x1", "y1")):
            li[name][:, j] = np.where(c > 0, b[:, i], 0xFFFF)
    return li


def one_track_lists(n, k):
    li = np.empty((n, k), dtype=OBJ)
    li[...] = EMPTY
    li[:, 0] = (6, 10 * 120 + 10, 10, 10, 12, 11)
    return li


def stat(v):
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
            "rounds_us": [round(x, 1) for x in v]}


def timed(call, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--scan-frames", type=int, default=4096, help="frames of the object-scan batch (0: skip that part)")
    ap.add_argument("--out", default=None, help="also write the table to this JSON file")
    ap.add_argument("--markdown", action="store_true", help="print the table of docs/rounds/r32_tracks.md")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = m.MotionScanner(m.ScanParams.from_config(1920, 1080))
    rng = np.random.RandomState(32)
    rows = []
    for shape, S, per in SHAPES:
        n = S * per
        for kind in ("movers", "one_track"):
            full = np.concatenate([movers_lists(rng, per, 16) if kind == "movers" else one_track_lists(per, 16) for _ in range(S)])
            lists = {k: np.ascontiguousarray(full[:, :k]) for k in KS}         # the list for k is the first k entries of the list for 16
            # a frame is a motion frame where its list holds an object; a key frame every 30
            fl = (lists[16]["cells"][:, 0] > 0).astype(np.uint8)
            sd = np.ones(n, dtype=np.uint8)
            sd[::30] = 0
            fl[::30] = 0
            d_flags, d_sd = torch.from_numpy(fl).to(dev), torch.from_numpy(sd).to(dev)
            d_soff = torch.from_numpy(np.arange(S + 1, dtype=np.int64) * per).to(dev)
            d_list = {k: torch.from_numpy(lists[k].view(np.int32).reshape(n, k, 4).copy()).to(dev) for k in KS}
            d_box = d_list[1][:, 0, 2:].contiguous().view(torch.int16)
            out = {k: {"pred": torch.empty((n, k), dtype=torch.uint8, device=dev), "flags": torch.empty(n, dtype=torch.uint8, device=dev),
                       "track": torch.empty(n, dtype=torch.int32, device=dev),
                       **{o: torch.empty((n, k), dtype=torch.int32, device=dev) for o in ("age", "id", "len")}} for k in KS}
            work = torch.empty(2 * n * 16, dtype=torch.int32, device=dev)
            pout = {"flags": torch.empty(n, dtype=torch.uint8, device=dev), "run": torch.empty(n, dtype=torch.int32, device=dev),
                    "pos": torch.empty(n, dtype=torch.int32, device=dev)}
            pwork = torch.empty(n, dtype=torch.int32, device=dev)
            calls = {"persist": lambda: s.persist_device(d_flags, d_soff, d_sd, d_box, 3, 1, 1, out=pout, work=pwork)}
            for k in KS:
                calls["tracks_k%d" % k] = lambda k=k: tracks.link_device(s, d_flags, d_list[k], d_soff, d_sd, 1, 1, 1, 3, out=out[k], work=work)
            calls["tracks_k16_flags_only"] = lambda: tracks.link_device(s, d_flags, d_list[16], d_soff, d_sd, 1, 1, 1, 3, want=("flags",),
                                                                        out=out[16], work=work)
            calls["tracks_k16_pred_age_id"] = lambda: tracks.link_device(s, d_flags, d_list[16], d_soff, d_sd, 1, 1, 1, 3,
                                                                         want=("pred", "age", "id"), out=out[16], work=work)
            for call in calls.values():                     # warm-up: code objects, first touch of the buffers
                call()
            torch.cuda.synchronize()
            # consequence A at k = 1, on these buffers
            assert torch.equal(out[1]["age"][:, 0], pout["pos"]) and torch.equal(out[1]["len"][:, 0], pout["run"]), "age/len != pos/run at k = 1"
            assert torch.equal(out[1]["track"], pout["run"]) and torch.equal(out[1]["flags"], pout["flags"]), "track/flags_out != run/flags_out at k = 1"
            got = {c: [] for c in calls}
            for _ in range(a.rounds):                       # interleaved: persist, k 1, k 4, k 16, ..., persist, ...
                for c, call in calls.items():
                    got[c].append(timed(call, a.steps))
            roots = int(((out[16]["age"] == 1)).sum().item())
            row = {"shape": shape, "lists": kind, "streams": S, "frames_per_stream": per, "motion_frames": int(fl.sum()), "roots_k16": roots,
                   "longest_track_k16": int(out[16]["track"].max().item()), "steps_per_round": a.steps, "k1_equals_persistence": True}
            for c, v in got.items():
                row[c] = stat(v)
            for k in KS:
                row["tracks_k%d_over_persist" % k] = round(row["tracks_k%d" % k]["median_us"] / row["persist"]["median_us"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    s.close()

    scan_row = None
    if a.scan_frames:
        import bench  # noqa: E402  (build_workload: the bench's own batches)
        w = bench.build_workload("1080p_dense8x8", "code_defaults", a.scan_frames, 60, 1, dev)
        s2, d_mv, d_off, F = w["scanner"], w["d_mv"], w["d_off"], a.scan_frames
        d_soff = torch.tensor([0, F], dtype=torch.int64, device=dev)
        scan_row = {"batch": "baseline", "workload": "1080p_dense8x8", "frames": F, "steps_per_round": a.steps}
        for k in KS:
            sout = {"flags": torch.empty(F, dtype=torch.uint8, device=dev), "list": torch.empty((F, k, 4), dtype=torch.int32, device=dev)}
            tout = {"track": torch.empty(F, dtype=torch.int32, device=dev), "flags": torch.empty(F, dtype=torch.uint8, device=dev)}
            work = torch.empty(2 * F * k, dtype=torch.int32, device=dev)
            calls = {"scan": lambda: objects.scan_device(s2, d_mv, d_off, None, k, 4, 1, want=("flags", "list"), out=sout),
                     "tracks": lambda: tracks.link_device(s2, sout["flags"], sout["list"], d_soff, None, 4, 1, 1, 3, want=("track", "flags"),
                                                          out=tout, work=work)}
            for call in calls.values():
                call()
            torch.cuda.synchronize()
            got = {c: [] for c in calls}
            for _ in range(a.rounds):
                for c, call in calls.items():
                    got[c].append(timed(call, a.steps))
            scan_row["scan_objects_k%d" % k] = stat(got["scan"])
            scan_row["tracks_k%d" % k] = stat(got["tracks"])
            scan_row["tracks_over_scan_k%d" % k] = round(scan_row["tracks_k%d" % k]["median_us"] / scan_row["scan_objects_k%d" % k]["median_us"], 4)
            scan_row["longest_track_k%d" % k] = int(tout["track"].max().item())
        print(json.dumps(scan_row), flush=True)

    doc = {"what": "HIP-event us per call (host submit included: --steps back-to-back calls between two events), median (min - max) over "
                   "--rounds interleaved rounds: mtgpu_persist_flags_device with boxes and all three outputs (persist: the yardstick, "
                   "existing code) and mtgpu_track_objects_device with all six outputs at k = 1, 4, 16, with flags_out alone and with "
                   "pred, age and id alone (no finish kernel, no depth updates) at k = 16; then the tracks call (track and flags_out) "
                   "next to mtgpu_scan_objects_device (flags and list) on one 1080p stream",
           "plan": tracks.preview(16), "rounds": a.rounds, "rows": rows, "object_scan": scan_row}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    if a.markdown:
        f = lambda r, c: "%.1f (%.1f-%.1f)" % (r[c]["median_us"], r[c]["min_us"], r[c]["max_us"])      # noqa: E731
        print("| input | lists | tracks (k 16) | persist us | " + " | ".join("k %d us | k %d / persist" % (k, k) for k in KS) +
              " | k 16 flags only us | k 16 pred, age, id us |")
        print("|---|---|---|---|" + "---|---|" * len(KS) + "---|---|")
        for r in rows:
            print("| %s | %s | %d | %s | " % (r["shape"], r["lists"], r["roots_k16"], f(r, "persist")) +
                  " | ".join("%s | %.2f" % (f(r, "tracks_k%d" % k), r["tracks_k%d_over_persist" % k]) for k in KS) +
                  " | %s | %s |" % (f(r, "tracks_k16_flags_only"), f(r, "tracks_k16_pred_age_id")))
        if scan_row:
            print()
            print("| k | object scan us | tracks us | tracks / scan |")
            print("|---|---|---|---|")
            for k in KS:
                print("| %d | %s | %s | %.4f |" % (k, f(scan_row, "scan_objects_k%d" % k), f(scan_row, "tracks_k%d" % k), scan_row["tracks_over_scan_k%d" % k]))


if __name__ == "__main__":
    main()
