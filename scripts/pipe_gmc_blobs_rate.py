#!/usr/bin/env python3
"""Rate of the decode path with the compensated blob scan (mtgpu_scan_file --gmc-blobs: .mtmv -> pinned zero-copy pipe
-> motion blobs on compensated residuals -> merge) next to the same path under each of its two halves and without
either, on the two sources of scripts/pipe_gmc_rate.py: the hot 1080p dense8x8 source (12 frames, cache-resident,
presented many times) and the same source with synth.StreamSpec(shake=5), through a compact zero-copy pipe, 16 workers.
The legs of pipe_gmc_rate.py — plain, masked (an all-ones keep mask), compensated (--gmc), compensated under the mask,
--gmc-vectors — plus the blob pipe (--min-blob-cells 3), the pair (--gmc-blobs 3), the pair under the mask and the pair's
sweep (--sweep-gmc-blobs, a pipe with MT_LAYOUT_CENTRES); three runs each, interleaved; frames/s as median and min-max,
each leg compared with the plain runs' own spread.  Then the kernel time per submit where the link does not hide it: one
context, one pipe, the same batches under plain, blobs, compensation and the pair, with and without the all-ones mask,
from the event triples of mtgpu_profile_enable (ScanPipe + MotionScanner.profile).  PCIe-inclusive; never the bench
value.  Needs a GPU.  Prints one JSON document; `--out PATH` also writes it to a file
(profiles/pipe_gmc_blobs_rate.json is one)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mvtrim_amd as m  # noqa: E402
from mvtrim_amd import synth, zones  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
ap.add_argument("--out", metavar="PATH", help="write the JSON document here as well")
args_ = ap.parse_args()
exe = os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "mtgpu_scan_file")
hot_n, reps, runs = 12, int(os.environ.get("RATE_REPS", "30000")), 3
workers = min(16, len(os.sched_getaffinity(0)))


def source(shake):
    spec = synth.spec_1080p(seed=9)
    spec.events = synth.scripted_events(spec, 150)
    spec.shake = shake
    return spec, [synth.gen_frame(spec, 1 + i) for i in range(hot_n)]


sources = {"hot": source(0), "shake": source(5)}
params = m.ScanParams.from_config(1920, 1080)
ones = np.ones((params.grid_h, params.grid_w), dtype=bool)
# name -> (keep mask or None, further arguments)
pipes = {"plain": (None, []), "masked": (ones, []), "gmc": (None, ["--gmc"]), "gmc_masked": (ones, ["--gmc"]),
         "gmc_vectors": (None, ["--gmc-vectors"]), "blobs": (None, ["--min-blob-cells", "3"]), "pair": (None, ["--gmc-blobs", "3"]),
         "pair_masked": (ones, ["--gmc-blobs", "3"]), "pair_sweep": (None, ["--sweep-gmc-blobs", "3,8"])}
rates = {src: {k: [] for k in pipes} for src in sources}
motion = {src: {} for src in sources}
with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as d:
    paths = {}
    for src, (spec, frames) in sources.items():
        paths[src] = os.path.join(d, src + ".mtmv")
        m.mvfile.write_mtmv(paths[src], 1920, 1080, 1, spec.tb_den, spec.fps, hot_n / spec.fps,
                            [spec.pts_ticks(i) for i in range(hot_n)], frames, key=[1] * hot_n)
    mask = os.path.join(d, "ones.mtkeep")
    zones.save_keep(mask, ones)
    env = dict(os.environ, CHUNK_DURATION_SEC="10", TARGET_FPS="0", MTGPU_STAGING="compact8_zc")
    env.pop("MTGPU_BATCH_MB", None)
    for k in ("VECTORS_NEEDED", "CLUSTERS_NEEDED", "MV_THRESHOLD_SQ", "BLOCK_SIZE", "BLOCK_SHIFT", "VERTICAL_MASK"):
        env.pop(k, None)
    for run in range(runs):
        for src in sources:
            for name, (keep, more) in pipes.items():
                args = [exe, paths[src], "--threads", str(workers), "--repeat", str(reps)] + (["--keep", mask] if keep is not None else []) + more
                r = json.loads(subprocess.run(args, check=True, capture_output=True, text=True, env=env, timeout=300).stdout)
                rate = hot_n * reps / max(r["scan_work_us"] * 1e-6, 1e-9)
                rates[src][name].append(rate)
                motion[src][name] = r["motion_frames"]
                print(f"run {run} {src:5s} {name:11s} {rate:9.0f} frames/s  ({r['motion_frames']} motion frames)", flush=True)

# ---- kernel time per submit: the same batches with and without the mask, from the event triples
import contextlib  # noqa: E402

kernel = {}
scanner = m.MotionScanner(params, device=0)
try:
    for src, (spec, frames) in sources.items():
        recs = sum(len(f) for f in frames)
        with contextlib.closing(m.ScanPipe(scanner, recs + 64, hot_n, 2, layout=m.LAYOUT_COMPACT8 | m.LAYOUT_ZERO_COPY)) as pipe:
            for name, keep, mode in (("plain", None, None), ("masked", ones, None), ("blobs", None, "blobs"), ("blobs_masked", ones, "blobs"),
                                     ("gmc", None, "gmc"), ("gmc_masked", ones, "gmc"), ("pair", None, "pair"), ("pair_masked", ones, "pair")):
                pipe.set_keep(keep)
                pipe.clear_gmc_blobs()
                pipe.clear_gmc()
                pipe.set_blobs(0)
                if mode == "gmc":
                    pipe.set_gmc()
                elif mode == "blobs":
                    pipe.set_blobs(3)
                elif mode == "pair":
                    pipe.set_gmc_blobs(3)
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
                        kernel.setdefault(src, {})[name] = {"launches": r["launches"], "scan_us_per_submit": 1e3 * r["scan_ms"],
                                                            "plan_us_per_submit": 1e3 * r["plan_ms"]}   # profile_read: means per launch
                scanner.profile(False)
finally:
    scanner.close()

out = {"what": f"mtgpu_scan_file on a {hot_n}-frame 1080p dense8x8 stream (hot: static camera; shake: synth shake 5) repeated {reps}x "
               f"({hot_n * reps} frames, cache-resident), {workers} workers, compact zero-copy staging, default batch size; rate from "
               f"'all workers initialised' to the last result; {len(pipes)} pipes, three runs each, interleaved",
       "frames": hot_n * reps, "workers": workers, "arguments": {k: v[1] + (["--keep", "<all ones>"] if v[0] is not None else []) for k, v in pipes.items()},
       "motion_frames": motion, "sources": {}, "kernel_time_per_submit": kernel}
for src, (spec, frames) in sources.items():
    recs = float(np.mean([len(f) for f in frames]))
    o = {"records_per_frame": recs, "pipes": {}}
    for name, v in rates[src].items():
        s = sorted(v)
        o["pipes"][name] = {"frames_per_s": {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "runs": v},
                            "pcie_GBps_median": s[len(s) // 2] * (8 * recs + 10) / 1e9}
    f = o["pipes"]["plain"]["frames_per_s"]
    o["plain_spread_pct"] = 100.0 * (f["max"] - f["min"]) / f["median"]
    for name in pipes:
        if name != "plain":
            o["pipes"][name]["median_vs_plain_pct"] = 100.0 * (o["pipes"][name]["frames_per_s"]["median"] / f["median"] - 1.0)
    out["sources"][src] = o
print(json.dumps(out))
if args_.out:
    with open(args_.out, "w") as f:
        json.dump(out, f, indent=1)
