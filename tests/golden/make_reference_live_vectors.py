#!/usr/bin/env python3
"""Generates tests/golden/reference_live_vectors.json by RUNNING THE REFERENCE ITSELF on the inputs of the tests that
used to call its binaries only where they were built (tests/test_reference_host.py::test_live_against_reference_binary,
::test_what_the_reference_would_choose_on_this_machine_vs_the_cpu_budget, tests/test_formats.py::
test_motion_scalar_live_reference_tool).  Those tests now replay this fixture everywhere, and still run the binaries
live where `make -C oracle ref` has built them.

  config / queue / memo   the seeded random inputs of the live host test (random.Random(7)) and the answers of
                          oracle/_ref/ref_host_probe to them
  sizing                  `ref_host_probe sizing` (the reference's detect_cpu_limit / calculate_parallel_streams) under
                          several PARALLEL_STREAMS values, with the CPU facts of the machine it ran on
  motion_scalar           stdout of oracle/_ref/motion_scalar for the 320x240 stream of the motion_scalar test

Run where the reference tree is present:
    make -C oracle ref && python tests/golden/make_reference_live_vectors.py
The fixture is data: inputs and the reference's printed answers.
"""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import mvtrim_amd as m  # noqa: E402
from mvtrim_amd import synth  # noqa: E402

PROBE = os.path.join(ROOT, "oracle", "_ref", "ref_host_probe")
SCALAR = os.path.join(ROOT, "oracle", "_ref", "motion_scalar")
GETTER_NAMES = ["mv_threshold_sq", "block_size", "block_shift", "vectors_needed", "clusters_needed", "vertical_mask",
                "max_gap_sec", "padding_sec", "chunk_duration_sec", "target_fps", "min_savings_pct", "parallel_streams",
                "threads_per_stream"]
CONFIG_VARS = [k.upper() for k in GETTER_NAMES]
SIZING_PARALLEL_STREAMS = [None, "0", "3", "64", "abc"]


def run(exe, args, env=None, stdin=None):
    e = {"PATH": os.environ.get("PATH", "")}
    e.update(env or {})
    out = subprocess.run([exe] + args, env=e, input=stdin, capture_output=True, text=True, check=True)
    return out.stdout.splitlines()


def _random_env(rng):
    pool = ["3", "4.75", "-2", " 9", "0x1F", "1e1", "12abc", "0.0625", "255", "256", ".5", "1e-3", "7."]
    return {v: rng.choice(pool) for v in rng.sample(CONFIG_VARS, rng.randrange(1, len(CONFIG_VARS)))}


def live_inputs():
    """(config envs, queue scripts, memo scripts): the draws the live host test made, in its order."""
    rng = random.Random(7)
    envs = [_random_env(rng) for _ in range(40)]
    queues = []
    for _ in range(10):
        ops, tid = [], 0
        for _ in range(200):
            c = rng.random()
            if c < 0.35:
                ops.append(f"tpush {rng.uniform(0, 9e4)!r} {rng.uniform(0, 9e4)!r} {tid}")
                tid += 1
            elif c < 0.6:
                ops.append("tpop")
            elif c < 0.75:
                n = rng.randrange(0, 6)
                ops.append(("radd %d %s" % (n, " ".join(repr(rng.uniform(-1, 1e5)) for _ in range(n)))).strip())
            elif c < 0.8:
                ops.append("rextract")
            elif c < 0.9:
                n = rng.randrange(0, 4)
                ops.append(("jpush %d %d %s" % (rng.randrange(64), n, " ".join(repr(rng.uniform(0, 1e4))
                                                                             for _ in range(2 * n)))).strip())
            else:
                ops.append(rng.choice(["jpop", "jdone", "jempty", "tfinish", "jfinish"]))
        ops += ["tfinish", "tpop", "jfinish", "jpop", "rextract"]
        queues.append(ops)
    pool = ["3", "4.75", "abc", "", " 9", "0x1F", "1e400", "300", "-1", "12abc", "99999999999"]
    memos = []
    for _ in range(20):
        ops = []
        for _ in range(40):
            c = rng.random()
            name = rng.choice(GETTER_NAMES)
            if c < 0.5:
                ops.append(f"get {name}")
            elif c < 0.9:
                ops.append(f"set {name.upper()} {rng.choice(pool)}")
            else:
                ops.append(f"unset {name.upper()}")
        memos.append(ops)
    return envs, queues, memos


def motion_scalar_stream():
    """The 320x240 stream of tests/test_formats.py::test_motion_scalar_live_reference_tool: (spec, frames, pts)."""
    spec = synth.StreamSpec(width=320, height=240, block=16, sub=1, fps=30.0, gop=10, seed=9, salt_p=0.05)
    spec.events = [synth.Event(3, 40, 4, 3, 5, 4, 11, -7)]
    frames = [synth.gen_frame(spec, i) for i in range(70)]
    pts = [spec.pts_seconds(i) for i in range(70)]
    return spec, frames, pts


def machine_facts():
    """What the reference's detect_cpu_limit() reads (src/system.cpp:107-163), as found where the sizing answers were
    recorded: the cgroup CPU quota rounded up (None: no quota) and the cgroup cpuset's CPU count (None: no file)."""
    def read(path):
        try:
            return open(path).read().strip()
        except OSError:
            return None
    quota = None
    q = read("/sys/fs/cgroup/cpu.max")
    if q and q.split()[0] != "max":
        quota = -(-int(q.split()[0]) // int(q.split()[1]))
    elif read("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") and int(read("/sys/fs/cgroup/cpu/cpu.cfs_quota_us")) > 0:
        quota = -(-int(read("/sys/fs/cgroup/cpu/cpu.cfs_quota_us")) // int(read("/sys/fs/cgroup/cpu/cpu.cfs_period_us")))
    cpus = read("/sys/fs/cgroup/cpuset.cpus.effective") or read("/sys/fs/cgroup/cpuset/cpuset.cpus")
    count = None
    if cpus:
        count = 0
        for part in cpus.split(","):
            lo, _, hi = part.partition("-")
            count += int(hi or lo) - int(lo) + 1
    return {"cgroup_quota_cpus": quota, "cgroup_cpuset_cpus": count, "hardware_concurrency": os.cpu_count()}


def main():
    for exe in (PROBE, SCALAR):
        if not os.path.exists(exe):
            raise SystemExit(f"{exe} missing: run `make -C oracle ref` where the reference tree is present")
    if run(PROBE, ["sizing"])[0] == "unavailable":
        raise SystemExit("ref_host_probe was built without the reference's system.cpp")
    envs, queues, memos = live_inputs()
    spec, frames, pts = motion_scalar_stream()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mv.json")
        m.mvjson.write_json(path, frames, pts, (1, spec.tb_den))
        out = subprocess.run([SCALAR, path], check=True, capture_output=True, text=True).stdout
    rows = sorted([int(a), b] for a, b in (ln.split(",") for ln in out.strip().splitlines()[1:]))
    doc = {
        "source": "oracle/_ref/ref_host_probe and oracle/_ref/motion_scalar (the reference's own code, make -C oracle "
                  "ref) run on the inputs below; generator: tests/golden/make_reference_live_vectors.py",
        "layout": run(PROBE, ["layout"]),
        "config": [{"env": e, "answers": run(PROBE, ["config"], e)} for e in envs],
        "queue": [{"script": ops, "answers": run(PROBE, ["queue"], stdin="\n".join(ops) + "\n")} for ops in queues],
        "memo": [{"script": ops, "answers": run(PROBE, ["memo"], stdin="\n".join(ops) + "\n")} for ops in memos],
        "sizing": {"machine": machine_facts(),
                   "cases": [{"parallel_streams": ps,
                              "answers": run(PROBE, ["sizing"], {} if ps is None else {"PARALLEL_STREAMS": ps})}
                             for ps in SIZING_PARALLEL_STREAMS]},
        "motion_scalar": {"csv_header": out.splitlines()[0], "rows": rows},
    }
    dst = os.path.join(HERE, "reference_live_vectors.json")
    with open(dst, "w") as f:
        json.dump(doc, f, indent=1)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
