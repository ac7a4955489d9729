#!/usr/bin/env python3
"""Rate of the decode path with a minimum blob size (mtgpu_scan_file --min-blob-cells / --sweep-blobs: .mtmv -> pinned
zero-copy pipe -> blob scan -> merge) next to the same path without one: the hot 1080p dense8x8 source of
host_pipeline_rate.py (12 frames, cache-resident, presented many times) through a compact zero-copy pipe, 16 workers.
Five pipes — plain, masked (an all-ones keep mask), blobs reporting centres (--min-blob-cells 3), plain with centre
counts (--centres), blobs reporting the largest blob (--min-blob-cells 3 --sweep-blobs 3) — three runs each, interleaved
(plain, masked, blobs_centres, plain_counts, blobs_largest, plain, ...); frames/s as median and min-max.  The last two
legs make mtgpu_scan_file do host work the first three do not: a pipe with MT_LAYOUT_CENTRES, one {pts, count} appended
per frame under a mutex inside the timed window, and 360 000 pairs sorted and printed after it (--sweep-blobs also runs
one more merge, after the window).  So blobs_largest is compared with plain_counts, which does the same host work with
the plain kernel, and the other legs with plain.  PCIe-inclusive; never the bench value.  Needs a GPU.  Prints one JSON document;
`--out PATH` also writes it to a file (profiles/pipe_blobs_rate.json is one)."""
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
spec = synth.spec_1080p(seed=9)
spec.events = synth.scripted_events(spec, 150)
hot_n, reps, runs = 12, int(os.environ.get("RATE_REPS", "30000")), 3
workers = min(16, len(os.sched_getaffinity(0)))
frames = [synth.gen_frame(spec, 1 + i) for i in range(hot_n)]
params = m.ScanParams.from_config(1920, 1080)
ones = np.ones((params.grid_h, params.grid_w), dtype=bool)
# name -> (keep mask or None, further arguments)
pipes = {"plain": (None, []), "masked": (ones, []), "blobs_centres": (None, ["--min-blob-cells", "3"]),
         "plain_counts": (None, ["--centres"]), "blobs_largest": (None, ["--min-blob-cells", "3", "--sweep-blobs", "3"])}
against = {"masked": "plain", "blobs_centres": "plain", "plain_counts": "plain", "blobs_largest": "plain_counts"}
rates = {k: [] for k in pipes}
motion = {}
with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as d:
    path = os.path.join(d, "hot.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, spec.tb_den, spec.fps, hot_n / spec.fps,
                        [spec.pts_ticks(i) for i in range(hot_n)], frames, key=[1] * hot_n)
    files = {}
    for name, (keep, _) in pipes.items():
        if keep is not None:
            files[name] = os.path.join(d, name + ".mtkeep")
            zones.save_keep(files[name], keep)
    env = dict(os.environ, CHUNK_DURATION_SEC="10", TARGET_FPS="0", MTGPU_STAGING="compact8_zc")
    env.pop("MTGPU_BATCH_MB", None)
    for k in ("VECTORS_NEEDED", "CLUSTERS_NEEDED", "MV_THRESHOLD_SQ", "BLOCK_SIZE", "BLOCK_SHIFT", "VERTICAL_MASK"):
        env.pop(k, None)
    for run in range(runs):
        for name, (_, more) in pipes.items():
            args = [exe, path, "--threads", str(workers), "--repeat", str(reps)] + (["--keep", files[name]] if name in files else []) + more
            r = json.loads(subprocess.run(args, check=True, capture_output=True, text=True, env=env, timeout=300).stdout)
            rate = hot_n * reps / max(r["scan_work_us"] * 1e-6, 1e-9)
            rates[name].append(rate)
            motion[name] = r["motion_frames"]
            print(f"run {run} {name:13s} {rate:9.0f} frames/s  ({r['motion_frames']} motion frames; copy {r['copy_us'] / 1e6:.2f} + submit "
                  f"{r['submit_us'] / 1e6:.2f} + wait {r['wait_us'] / 1e6:.2f} s summed over {workers} workers)", flush=True)
recs = float(np.mean([len(f) for f in frames]))
out = {"what": f"mtgpu_scan_file on a {hot_n}-frame 1080p dense8x8 stream repeated {reps}x ({hot_n * reps} frames, cache-resident), "
               f"{workers} workers, compact zero-copy staging, default batch size; rate from 'all workers initialised' to the last "
               "result; five pipes, three runs each, interleaved; the legs with per-frame counts (plain_counts, blobs_largest) also "
               "append, sort and print one pair per frame",
       "frames": hot_n * reps, "workers": workers, "records_per_frame": recs, "arguments": {k: v[1] + (["--keep", "<all ones>"] if v[0] is not None else []) for k, v in pipes.items()},
       "motion_frames": motion, "pipes": {}}
for name, v in rates.items():
    s = sorted(v)
    out["pipes"][name] = {"frames_per_s": {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "runs": v},
                          "pcie_GBps_median": s[len(s) // 2] * (8 * recs + 10) / 1e9}
for name in ("plain", "plain_counts"):
    f = out["pipes"][name]["frames_per_s"]
    out[name + "_spread_pct"] = 100.0 * (f["max"] - f["min"]) / f["median"]
for name, ref in against.items():
    out["pipes"][name]["against"] = ref
    out["pipes"][name]["median_vs_against_pct"] = 100.0 * (out["pipes"][name]["frames_per_s"]["median"] /
                                                           out["pipes"][ref]["frames_per_s"]["median"] - 1.0)
print(json.dumps(out))
if args_.out:
    with open(args_.out, "w") as f:
        json.dump(out, f, indent=1)
