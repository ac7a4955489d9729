#!/usr/bin/env python3
"""Rate of the decode path with a direction plane (mtgpu_scan_file --plane: .mtmv -> pinned zero-copy pipe -> plane scan
-> merge) next to the same path with the scalar direction filter and without either, on the hot 1080p dense8x8 source of
host_pipeline_rate.py (12 frames, cache-resident, presented many times), through a compact zero-copy pipe, 16 workers.
pipe_dir_rate.py's five legs — plain, masked (an all-ones keep mask), direction (--ignore W,NW,SW), direction under the
all-ones mask, direction with --dir-sectors — plus a plane leg (--plane: the upper half of the picture forbids W, NW and
SW, the lower half allows everything; staged in LDS on this grid) and a plane-under-mask leg; three runs each,
interleaved; frames/s as median and min-max, each leg compared with the plain runs' own spread.  Then the kernel time per
submit where the link does not hide it: one context, one pipe, the same batches in six legs, from the event triples of
mtgpu_profile_enable (ScanPipe + MotionScanner.profile).  PCIe-inclusive; never the bench value.  Needs a GPU.  Prints
one JSON document; `--out PATH` also writes it to a file (profiles/pipe_lanes_rate.json is one)."""
import argparse
import contextlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mvtrim_amd as m  # noqa: E402
from mvtrim_amd import lanes, synth, zones  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
ap.add_argument("--out", metavar="PATH", help="write the JSON document here as well")
args_ = ap.parse_args()
exe = os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "mtgpu_scan_file")
hot_n, reps, runs = 12, int(os.environ.get("RATE_REPS", "30000")), 3
workers = min(16, len(os.sched_getaffinity(0)))
IGNORE = "W,NW,SW"
ALLOW = 0xFF & ~(1 << 4 | 1 << 5 | 1 << 3)

spec = synth.spec_1080p(seed=9)
spec.events = synth.scripted_events(spec, 150)
frames = [synth.gen_frame(spec, 1 + i) for i in range(hot_n)]
params = m.ScanParams.from_config(1920, 1080)
ones = np.ones((params.grid_h, params.grid_w), dtype=bool)
plane = np.full((params.grid_h, params.grid_w), 0xFF, dtype=np.uint8)
plane[:params.grid_h // 2] = ALLOW
# name -> (keep mask or None, further arguments)
legs = {"plain": (None, []), "masked": (ones, []), "dir": (None, ["--ignore", IGNORE]), "dir_masked": (ones, ["--ignore", IGNORE]),
        "dir_sectors": (None, ["--ignore", IGNORE, "--dir-sectors"]), "plane": (None, ["--plane", "PLANE"]),
        "plane_masked": (ones, ["--plane", "PLANE"])}
rates = {k: [] for k in legs}
motion = {}
with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as d:
    path = os.path.join(d, "hot.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, spec.tb_den, spec.fps, hot_n / spec.fps, [spec.pts_ticks(i) for i in range(hot_n)],
                        frames, key=[1] * hot_n)
    mask = os.path.join(d, "ones.mtkeep")
    zones.save_keep(mask, ones)
    plane_path = os.path.join(d, "half.mtdir")
    lanes.save_plane(plane_path, plane)
    env = dict(os.environ, CHUNK_DURATION_SEC="10", TARGET_FPS="0", MTGPU_STAGING="compact8_zc")
    env.pop("MTGPU_BATCH_MB", None)
    for k in ("VECTORS_NEEDED", "CLUSTERS_NEEDED", "MV_THRESHOLD_SQ", "BLOCK_SIZE", "BLOCK_SHIFT", "VERTICAL_MASK"):
        env.pop(k, None)
    for run in range(runs):
        for name, (keep, more) in legs.items():
            args = [exe, path, "--threads", str(workers), "--repeat", str(reps)] + (["--keep", mask] if keep is not None else []) + \
                [plane_path if a == "PLANE" else a for a in more]
            r = json.loads(subprocess.run(args, check=True, capture_output=True, text=True, env=env, timeout=300).stdout)
            rate = hot_n * reps / max(r["scan_work_us"] * 1e-6, 1e-9)
            rates[name].append(rate)
            motion[name] = r["motion_frames"]
            print(f"run {run} {name:11s} {rate:9.0f} frames/s  ({r['motion_frames']} motion frames)", flush=True)

# ---- kernel time per submit: the same batches in four legs, from the event triples
kernel = {}
scanner = m.MotionScanner(params, device=0)
try:
    recs = sum(len(f) for f in frames)
    with contextlib.closing(m.ScanPipe(scanner, recs + 64, hot_n, 2, layout=m.LAYOUT_COMPACT8 | m.LAYOUT_ZERO_COPY)) as pipe:
        for name, keep, on in (("plain", None, None), ("masked", ones, None), ("dir", None, "dir"), ("dir_masked", ones, "dir"),
                               ("plane", None, "plane"), ("plane_masked", ones, "plane")):
            pipe.set_keep(keep)
            pipe.clear_dir()
            pipe.clear_plane()
            if on == "dir":
                pipe.set_dir(ALLOW)
            elif on == "plane":
                pipe.set_plane(plane)
            for timed in (False, True):                   # one warm-up pass, then 50 submits of the 12-frame batch
                scanner.profile(timed)
                if timed:
                    scanner.profile_read()
                for _ in range(50 if timed else 5):
                    for i, f in enumerate(frames):
                        pipe.feed(f, float(i), tag=i)
                    pipe.drain()
                if timed:
                    r = scanner.profile_read()
                    kernel[name] = {"launches": r["launches"], "scan_us_per_submit": 1e3 * r["scan_ms"],
                                    "plan_us_per_submit": 1e3 * r["plan_ms"]}   # profile_read: means per launch
            scanner.profile(False)
finally:
    scanner.close()

recs = float(np.mean([len(f) for f in frames]))
out = {"what": f"mtgpu_scan_file on a {hot_n}-frame 1080p dense8x8 stream (static camera) repeated {reps}x ({hot_n * reps} frames, "
               f"cache-resident), {workers} workers, compact zero-copy staging, default batch size; rate from 'all workers "
               "initialised' to the last result; seven legs, three runs each, interleaved",
       "frames": hot_n * reps, "workers": workers, "records_per_frame": recs,
       "arguments": {k: v[1] + (["--keep", "<all ones>"] if v[0] is not None else []) for k, v in legs.items()},
       "plane": "upper half 0x%02x, lower half 0xff; staged %d" % (ALLOW, m.lanes_preview(params)["staged"]), "motion_frames": motion, "legs": {}, "kernel_time_per_submit": kernel}
for name, v in rates.items():
    s = sorted(v)
    out["legs"][name] = {"frames_per_s": {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "runs": v},
                         "pcie_GBps_median": s[len(s) // 2] * (8 * recs + 10) / 1e9}
f = out["legs"]["plain"]["frames_per_s"]
out["plain_spread_pct"] = 100.0 * (f["max"] - f["min"]) / f["median"]
for name in legs:
    if name != "plain":
        g = out["legs"][name]["frames_per_s"]
        out["legs"][name]["median_vs_plain_pct"] = 100.0 * (g["median"] / f["median"] - 1.0)
        out["legs"][name]["within_plain_spread"] = bool(f["min"] <= g["median"] <= f["max"])
print(json.dumps(out))
if args_.out:
    with open(args_.out, "w") as fh:
        json.dump(out, fh, indent=1)
