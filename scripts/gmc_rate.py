#!/usr/bin/env python3
"""What global-motion compensation costs (needs a GPU): mtgpu_scan_centres_device — the yardstick, existing code —
against mtgpu_scan_gmc_device on the same resident 1080p dense8x8 batch, in both record layouts, on the standard
synthetic stream and on a pan stream (every record (9, 3): bench.build_workload's AB_PAN input, the one
scripts/ab_pan.py measures the scan on).  Interleaved in one process and timed with the library's own events
(mtgpu_profile_enable / mtgpu_profile_read: scan-kernel us per launch), as scripts/zones_rate.py does.  The script
asserts that max_shift 0 returns the yardstick's counts, that every frame of the pan stream is compensated and that its
centre counts drop below a tenth.  There is no pass mark.

    python scripts/gmc_rate.py [--frames 4096] [--rounds 3] [--steps 5] [--out profiles/gmc_rate.json] [--markdown]

A variant of the kernel is another build of the library, compared by running this script once per build
(MTGPU_LIBRARY=<path>, the loader's developer switch):
    make -C motion-estimated-video-trimmer_amd/csrc ../libmtgpu_naive.so OUT=../libmtgpu_naive.so EXTRA=-DMTGPU_GMC_NAIVE_HIST
(one LDS atomic per lane and record instead of the wave-aggregated add).  The rows name the library by its path
relative to the repository.

    python scripts/gmc_rate.py --pmc [--frames 1024] [--library PATH ...]
runs, per library and layout, one child process of this script under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` (a
counter pass of its own, no trace domain other than --kernel-trace) that launches the compensated scan four times on the pan batch, and prints
the fetched bytes of gmc_frames_kernel per launch next to the batch's record bytes: 2x = both passes come from HBM,
1x = the second pass hits in L2 / MALL."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=None, help="frames of the resident batch (default 4096; --pmc: 1024)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--max-shift", type=int, default=16)
ap.add_argument("--min-share-q8", type=int, default=128)
ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
ap.add_argument("--markdown", action="store_true", help="print the table of docs/rounds/r10_gmc.md")
ap.add_argument("--pmc", action="store_true", help="the fetched-bytes leg (see above)")
ap.add_argument("--library", action="append", default=[], help="--pmc: a build of the library to measure (default: the tree's)")
ap.add_argument("--pmc-child", nargs=2, metavar=("LAYOUT", "INPUT"), help="internal: what rocprofv3 profiles")
a = ap.parse_args()


def library_label(path):
    """How a row names the library it measured: "tree" for the tree's own build, else the path relative to the
    repository (the basename for a library outside it) — never an absolute path of the measuring machine."""
    if not path:
        return "tree"
    rel = os.path.relpath(os.path.realpath(path), os.path.realpath(ROOT))
    return os.path.basename(path) if rel.startswith("..") else rel.replace(os.sep, "/")


def pmc_leg():
    """One rocprofv3 child per (library, layout); no GPU work in this process."""
    import csv
    import glob
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    frames = a.frames or 1024
    rows = []
    for lib in (a.library or [None]):
        for layout in ("aos40", "compact8"):
            with tempfile.TemporaryDirectory() as tmp:
                env = dict(os.environ, TMPDIR=tmp)
                if lib:
                    env["MTGPU_LIBRARY"] = os.path.abspath(lib)
                cmd = [exe, "--kernel-trace", "--pmc", "FETCH_SIZE", "-f", "csv", "-d", os.path.join(tmp, "out"), "--", sys.executable,
                       os.path.abspath(__file__), "--pmc-child", layout, "pan", "--frames", str(frames), "--max-shift", str(a.max_shift),
                       "--min-share-q8", str(a.min_share_q8)]
                r = subprocess.run(cmd, cwd=tmp, env=env, capture_output=True, text=True, timeout=280)
                if r.returncode != 0:
                    raise SystemExit(f"rocprofv3 child exited {r.returncode}: {(r.stderr or '')[-400:]}")
                rec_bytes = int([ln for ln in r.stdout.splitlines() if ln.startswith("record_bytes ")][-1].split()[1])
                total, launches = 0.0, 0
                for path in glob.glob(os.path.join(tmp, "out", "**", "*_counter_collection.csv"), recursive=True):
                    with open(path, newline="") as fh:
                        for row in csv.DictReader(fh):
                            if row.get("Counter_Name") == "FETCH_SIZE" and "gmc_frames_kernel" in row.get("Kernel_Name", ""):
                                total += float(row["Counter_Value"])
                                launches += 1
                if not launches:
                    raise SystemExit("no gmc_frames_kernel dispatch in the counter output")
                # gfx950: the counter's unit is KB and wide coalesced streaming reads are reported at half their bytes
                # (bench.pmc_bytes); both figures are printed
                kb = total / launches
                row = {"library": library_label(lib), "layout": layout, "frames": frames, "launches": launches, "record_bytes": rec_bytes,
                       "FETCH_SIZE_KB_raw": round(kb, 1), "fetched_over_records_raw": round(kb * 1024.0 / rec_bytes, 3),
                       "fetched_over_records_x2": round(kb * 2048.0 / rec_bytes, 3)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        json.dump({"what": "FETCH_SIZE of gmc_frames_kernel per launch on the pan batch, one rocprofv3 counter pass per row",
                   "rows": rows}, open(a.out, "w"), indent=1)


if a.pmc:
    pmc_leg()
    sys.exit(0)

import torch  # noqa: E402
import mvtrim_amd as m  # noqa: E402
import bench  # noqa: E402  (build_workload: the bench's own batches)

dev = torch.device("cuda", 0)
FRAMES = a.frames or 4096


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


if a.pmc_child:
    layout, kind = a.pmc_child
    w = build(kind)
    s = w["scanner"]
    compact = layout == "compact8"
    d_rec = w["d_rec8"] if compact else w["d_mv"]
    ce = torch.empty(FRAMES, dtype=torch.int32, device=dev)
    for _ in range(4):
        s.scan_gmc_device(d_rec, w["d_off"], None, a.max_shift, a.min_share_q8, compact=compact, flags=False, centres=ce, info=False)
    torch.cuda.synchronize()
    print("record_bytes", w["n_records"] * (8 if compact else 40), flush=True)
    s.close()
    sys.exit(0)


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
    ref = torch.empty(FRAMES, dtype=torch.int32, device=dev)
    ce = torch.empty(FRAMES, dtype=torch.int32, device=dev)
    inf = torch.empty((FRAMES, 5), dtype=torch.int32, device=dev)
    for layout, compact, d_rec in (("aos40", False, w["d_mv"]), ("compact8", True, w["d_rec8"])):
        def centres():
            return s.count_centres_device(d_rec, w["d_off"], None, compact=compact, flags=False, centres=ref)

        def gmc_call(ms=a.max_shift):
            return s.scan_gmc_device(d_rec, w["d_off"], None, ms, a.min_share_q8, compact=compact, flags=False, centres=ce, info=inf)
        calls = {"centres": centres, "gmc": gmc_call}
        got = {k: [] for k in calls}
        for _ in range(a.rounds):                      # interleaved: centres, gmc, centres, ...
            for k, call in calls.items():
                got[k].append(timed(s, call))
        torch.cuda.synchronize()
        centres()
        gmc_call(0)
        torch.cuda.synchronize()
        assert bool(torch.equal(ref, ce)), "max_shift 0 does not return the centre scan's counts"
        plain_sum = int(ref.to(torch.int64).sum())
        gmc_call()
        torch.cuda.synchronize()
        info = inf.cpu().numpy().reshape(-1).view(m.GMC_INFO_DTYPE)
        row = {"input": kind, "layout": layout, "frames": FRAMES, "records": w["n_records"], "library": library_label(os.environ.get("MTGPU_LIBRARY")),
               "max_shift": a.max_shift, "min_share_q8": a.min_share_q8, "gmc_plan": m.gmc_preview(s.params), "steps_per_round": a.steps,
               "centre_sum_plain": plain_sum, "centre_sum_gmc": int(ce.to(torch.int64).sum()),
               "frames_compensated": int(((info["gx"] != 0) | (info["gy"] != 0)).sum())}
        if kind == "pan":
            # the generator lets an event's rectangle drift with its motion: by the last of the 60 distinct frames the
            # pan has left the 8 leftmost of the 118 centre columns to the background, whose residual is then (-9, -3)
            with_sd = int((info["n_in"] > 0).sum())
            assert row["frames_compensated"] == with_sd and row["centre_sum_gmc"] < plain_sum // 10, row
        for k, v in got.items():
            row[k] = stat(v)
        row["gmc_over_centres"] = round(row["gmc"]["median_us"] / row["centres"]["median_us"], 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    s.close()
    del w

if a.out:
    json.dump({"what": "scan-kernel us per launch (library events), the two calls interleaved in one process: "
                       "mtgpu_scan_centres_device (centres: the yardstick) and mtgpu_scan_gmc_device (gmc)", "rows": rows},
              open(a.out, "w"), indent=1)
if a.markdown:
    print("| input | layout | frames | centres us (min-max) | gmc us (min-max) | gmc / centres | frames compensated |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda k: "%.1f (%.1f-%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])      # noqa: E731
        print("| %s | %s | %d | %s | %s | %.3f | %d |" % (r["input"], r["layout"], r["frames"], f("centres"), f("gmc"),
                                                        r["gmc_over_centres"], r["frames_compensated"]))
