#!/usr/bin/env python3
"""Time of one persistence call (mtgpu_persist_flags_device) next to mtgpu_merge_streams_device on the same flags — the
kernel with the same launch shape, one workgroup per stream — on (a) 64 streams x 864 000 frames (a day at 10 fps each)
and (b) one stream of 2 160 000 frames, with and without boxes.  Three interleaved runs per leg, each the HIP-event time
of REPS back-to-back calls; reported as median (min - max) per call.  Needs a GPU.

  python scripts/persist_rate.py [--out profiles/persist_rate.json] [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mvtrim_amd as m  # noqa: E402

SHAPES = (("64x864000", 64, 864_000), ("1x2160000", 1, 2_160_000))


def stream(rng, n):
    """Bursts of about sixteen motion frames with dropouts inside, a key frame every 30, a box that wanders."""
    fl = (np.repeat(rng.random_sample(n // 16 + 1) < 0.15, 16)[:n] & (rng.random_sample(n) < 0.9)).astype(np.uint8)
    sd = np.ones(n, dtype=np.uint8)
    sd[::30] = 0
    fl[::30] = 0
    x0 = (40 + np.cumsum(rng.randint(-2, 3, size=n))) % 116
    y0 = (30 + np.cumsum(rng.randint(-2, 3, size=n))) % 65
    box = np.stack([x0, y0, x0 + 3, y0 + 2], axis=1).astype(np.int16)
    return fl, sd, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = m.MotionScanner(m.ScanParams.from_config(1920, 1080))
    rng = np.random.RandomState(18)
    rows = []
    for name, S, per in SHAPES:
        fl, sd, box = stream(rng, per)
        n = S * per
        d_flags = torch.from_numpy(np.tile(fl, S)).to(dev)
        d_sd = torch.from_numpy(np.tile(sd, S)).to(dev)
        d_box = torch.from_numpy(np.tile(box, (S, 1))).to(dev)
        d_soff = torch.from_numpy(np.arange(S + 1, dtype=np.int64) * per).to(dev)
        d_pts = torch.from_numpy(np.tile(np.arange(per, dtype=np.float64) / 10.0, S)).to(dev)
        d_mp = torch.from_numpy(np.tile(m.MergeParams(duration=per / 10.0).to_record().view(np.uint8), S).copy()).to(dev)
        out = {"flags": torch.empty(n, dtype=torch.uint8, device=dev), "run": torch.empty(n, dtype=torch.int32, device=dev),
               "pos": torch.empty(n, dtype=torch.int32, device=dev)}
        work = torch.empty(n, dtype=torch.int32, device=dev)
        mout = (torch.zeros((S, 64, 2), dtype=torch.float64, device=dev), torch.zeros((S, 40), dtype=torch.uint8, device=dev),
                torch.empty(2 * n, dtype=torch.float64, device=dev))
        legs = {
            "persist": lambda: s.persist_device(d_flags, d_soff, d_sd, None, 3, 1, 0, out=out, work=work),
            "persist_boxes": lambda: s.persist_device(d_flags, d_soff, d_sd, d_box, 3, 1, 2, out=out, work=work),
            "persist_flags_only": lambda: s.persist_device(d_flags, d_soff, d_sd, None, 3, 1, 0, want=("flags",), out=out, work=work),
            "merge": lambda: s.merge_streams_device(d_flags, d_pts, d_soff, d_mp, False, 64, out=mout),
        }
        for call in legs.values():                      # warm-up: code objects, first touch of the buffers
            call()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(3):                              # three interleaved runs per leg
            for k, call in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.reps)
        runs = int((out["pos"] == 1).sum().item())
        row = {"shape": name, "streams": S, "frames_per_stream": per, "motion_frames": int(d_flags.sum().item()), "runs": runs}
        for k, v in times.items():
            row[k + "_ms"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d_flags, d_sd, d_box, d_pts, out, work, mout
        torch.cuda.empty_cache()
    doc = {"what": "HIP-event time per call of mtgpu_persist_flags_device (all three outputs; with boxes; flags_out alone) and of "
                   "mtgpu_merge_streams_device on the same flags; median (min - max) of three interleaved runs of --reps calls each",
           "plan": m.persist_preview(), "reps": a.reps, "rows": rows}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
