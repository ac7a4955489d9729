"""The host layer's answers to every combination of scan modes, as a fixture: tests/cpp/mode_matrix_probe.cpp (its head
comment has the case encodings and the line formats) run on a GPU against one commit's csrc/host/mtgpu_host.hpp and
library.

    python tests/host_mode_matrix.py --record --commit <id> --probe <mode_matrix_probe built against that commit>

writes tests/golden/host_mode_matrix.json: GpuMotionScanner::initialize over the whole product of its settings (`scanner
full`) and run_scan_pipeline over every case with at most three fields off their defaults (`pipeline 3`: the whole product
of its sixteen axes is tens of thousands of threaded runs).  The fixture is recorded from the commit BEFORE a change to
that code, never from the change itself; tests/test_scan_request_host.py and tests/test_gpu_host_mode_matrix.py only
compare.  Each distinct sentence and each distinct pipe state is stored once, and the fixture holds one index per case, in the
order in which scanner_cases() and pipeline_cases(3) below — the probe's own loops — list the cases.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "host_mode_matrix.json")
PROBE_SRC = os.path.join(HERE, "cpp", "mode_matrix_probe.cpp")
ALL_OFF = "blobs=0:0:0 gmc=0:0:0:0 pair=0:0:0:0:0 dir=0:0:0 plane=0:0"      # behind "keep=<0/1> "


def build_probe(exe, pkg):
    """The probe against this tree's host header and library."""
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(pkg, "csrc", "host"), "-o", exe, PROBE_SRC, "-L" + pkg, "-lmtgpu", "-lpthread",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run_probe(exe, *args, timeout=300):
    """-> (grid, {"S": {case: (answer, state)}, "P": {case: (rc, frames_scanned, error)}, "Q": {(x, y): (answer, state)}})"""
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    grid, rows = None, {"S": {}, "P": {}, "Q": {}}
    for line in out.stdout.splitlines():
        kind, _, rest = line.partition(" ")
        if kind == "grid":
            grid = tuple(int(v) for v in rest.split())
            continue
        f = rest.split("\t")
        case = tuple(int(v) for v in f[0].split())
        rows[kind][case] = (int(f[1]), int(f[2]), f[3]) if kind == "P" else (f[1], f[2])
    return grid, rows


def combos(axes, most):
    """mode_matrix_probe.cpp's combos(): every assignment of the axes with at most `most` of them off their default (the
    first value), the first axis outermost; most < 0: the whole product."""
    out, cur = [], [a[0] for a in axes]

    def go(i, used):
        if i == len(axes):
            out.append(tuple(cur))
            return
        for k, v in enumerate(axes[i]):
            if k and 0 <= most == used:
                break
            cur[i] = v
            go(i + 1, used + (1 if k else 0))
        cur[i] = axes[i][0]
    go(0, 0)
    return out


SCANNER_AXES = [[0, 1], [0, 3], [0, 1], [-1, 4], [0, 1], [0, 3], [0, 1, 2], [-1, 0x5B], [0, 1], [0, 1, 2], [0, 1, 2], [-1]]
PIPELINE_AXES = [[0, 1], [0, 1, 2], [0, 3], [0, 1, 2], [-2, 4, 200], [0, 1], [0, 3, -5], [0, 1, 2], [-2, 0x5B, 300], [0, 1], [0, 1, 2],
                 [0, 1, 2], [0, 3, -7], [-1, 2, 70000], [0, 1], [0]]


def scanner_cases(most=-1):
    """The probe's `scanner` cases, in its order."""
    return combos(SCANNER_AXES, most) + [(kc, mb, 0, -1, 0, pair, 0, -1, 0, 0, 0, reach)
                                         for kc in (0, 1) for reach in (2, 70000) for mb in (0, 3) for pair in (0, 3)]


def pipeline_cases(most):
    """The probe's `pipeline` cases, in its order."""
    return combos(PIPELINE_AXES, most) + [(kc, 0, -1, 0, -1, 0, -1, 0, -1, 0, 0, 0, -1, -1, 0, bits)
                                          for bits in range(128) if bin(bits).count("1") <= 2 for kc in (0, 1)]


def load():
    """-> (grid, scanner {case: (answer, state)}, pipeline {case: (rc, frames_scanned, error)}) of the fixture.  The
    fixture holds the answers alone, in the order of scanner_cases() and pipeline_cases(3); a pipeline run that gave no
    error returned 0 and scanned the clip's three frames, every other one returned 1 and scanned none."""
    with open(FIXTURE) as f:
        doc = json.load(f)
    s, st = doc["sentences"], doc["states"]
    sc, pc = scanner_cases(), pipeline_cases(3)
    assert len(sc) == len(doc["scanner_answers"]) == len(doc["scanner_states"]) and len(pc) == len(doc["pipeline_answers"])
    scanner = {c: (s[a], st[b]) for c, a, b in zip(sc, doc["scanner_answers"], doc["scanner_states"])}
    pipeline = {c: ((0, 3, "-") if s[a] == "-" else (1, 0, s[a])) for c, a in zip(pc, doc["pipeline_answers"])}
    return tuple(doc["grid"]), scanner, pipeline


def off_default(case, defaults):
    return sum(1 for v, d in zip(case, defaults) if v != d)


PIPELINE_DEFAULT = (0, 0, 0, 0, -2, 0, 0, 0, -2, 0, 0, 0, 0, -1, 0, 0)


def wrapped(name, numbers, per_line=128):
    rows = [", ".join(str(v) for v in numbers[i:i + per_line]) for i in range(0, len(numbers), per_line)]
    return '"%s": [\n' % name + ",\n".join(rows) + "\n]"


def write_fixture(head, sentences, states, scanner, pipeline):
    """scanner: [(answer, state)] in scanner_cases() order; pipeline: [(rc, frames_scanned, error)] in pipeline_cases(3) order."""
    assert all(v[:2] == ((0, 3) if v[2] == "-" else (1, 0)) for v in pipeline)       # what load() puts back
    si, sti = {t: i for i, t in enumerate(sentences)}, {t: i for i, t in enumerate(states)}
    with open(FIXTURE, "w") as f:
        f.write("{\n" + "".join('"%s": %s,\n' % (k, json.dumps(v)) for k, v in sorted(head.items())))
        for name, texts in (("sentences", sentences), ("states", states)):
            f.write('"%s": [\n' % name + ",\n".join(json.dumps(t) for t in texts) + "\n],\n")
        f.write(wrapped("scanner_answers", [si[v[0]] for v in scanner]) + ",\n" + wrapped("scanner_states", [sti[v[1]] for v in scanner]) + ",\n" +
                wrapped("pipeline_answers", [si[v[2]] for v in pipeline]) + "\n}\n")


def record(commit, probe):
    grid, a = run_probe(probe, "scanner", "full", timeout=600)
    grid_p, b = run_probe(probe, "pipeline", 3, timeout=900)
    assert grid == grid_p and list(a["S"]) == scanner_cases() and list(b["P"]) == pipeline_cases(3)
    sentences = sorted({v[0] for v in a["S"].values()} | {v[2] for v in b["P"].values()})
    states = sorted({v[1] for v in a["S"].values()})
    write_fixture({"recorded_from": commit, "grid": list(grid),
                   "how": "python tests/host_mode_matrix.py --record --commit <id> --probe <tests/cpp/mode_matrix_probe.cpp built against "
                          "that commit's mtgpu_host.hpp and libmtgpu.so>, on the GPU"}, sentences, states, list(a["S"].values()), list(b["P"].values()))
    print("recorded", len(a["S"]), "scanner and", len(b["P"]), "pipeline cases,", len(sentences), "sentences,", len(states), "states, from", commit)


if __name__ == "__main__":
    if "--record" not in sys.argv or "--commit" not in sys.argv or "--probe" not in sys.argv:
        raise SystemExit(__doc__)
    record(sys.argv[sys.argv.index("--commit") + 1], sys.argv[sys.argv.index("--probe") + 1])
