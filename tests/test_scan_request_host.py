"""CPU tier: csrc/host/scan_request.hpp against tests/golden/host_mode_matrix.json — what GpuMotionScanner::initialize and
run_scan_pipeline answered on a GPU at the commit before their "not together" ladders became the two pure functions of
that header (tests/host_mode_matrix.py).  A stand-alone program (tests/cpp/scan_request_replay.cpp: the header alone, no
library, built with the address and undefined-behaviour sanitizers) takes every recorded case through resolve_scanner /
resolve_pipeline; the error text — the FIRST one where several rules are broken — and, where the parent's initialize()
succeeded, the mode and settings its pipe then carried must be the recorded ones."""
import os
import subprocess

import pytest

import host_mode_matrix as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "csrc", "host")


@pytest.fixture(scope="module")
def golden():
    return hm.load()


@pytest.fixture(scope="module")
def replayed(tmp_path_factory, golden):
    exe = str(tmp_path_factory.mktemp("scan_request") / "scan_request_replay")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "scan_request_replay.cpp")])
    grid, scanner, pipeline = golden
    text = "".join("S " + " ".join(map(str, c)) + "\n" for c in scanner) + "".join("P " + " ".join(map(str, c)) + "\n" for c in pipeline)
    out = subprocess.run([exe, str(grid[0]), str(grid[1])], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
    got = {"S": {}, "P": {}}
    for line in out.stdout.splitlines():
        f = line[2:].split("\t")
        got[line[0]][tuple(int(v) for v in f[0].split())] = (f[1], f[2])
    return got


def test_the_header_stands_alone(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "scan_request.hpp"\nint main() { return mtgpu_host::resolve_scanner(mtgpu_host::ScannerAsk()).error.empty() ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           str(src)])
    text = open(os.path.join(HOST, "scan_request.hpp")).read()
    assert "hip_runtime" not in text and '#include "mtgpu_host.hpp"' not in text


def test_the_fixture_is_the_whole_scanner_product_and_the_pipeline_triples(golden):
    _, scanner, pipeline = golden
    assert len(scanner) == 2 ** 8 * 3 ** 3 + 16 and len(pipeline) > 2000
    assert max(hm.off_default(c, hm.PIPELINE_DEFAULT) for c in pipeline if c[2] != -1) == 3
    assert {v[0] for v in scanner.values()} >= {"ok"} and len({v[0] for v in scanner.values()}) > 20
    assert len({v[2] for v in pipeline.values()}) > 25


def test_resolve_scanner_answers_every_recorded_combination(golden, replayed):
    _, scanner, _ = golden
    assert sorted(replayed["S"]) == sorted(scanner)
    wrong = [(c, replayed["S"][c], want) for c, want in scanner.items()
             if replayed["S"][c][0] != want[0] or (want[0] == "ok" and replayed["S"][c][1] != want[1])]
    assert not wrong, (len(wrong), wrong[:5])


def test_resolve_pipeline_answers_every_recorded_combination(golden, replayed):
    _, _, pipeline = golden
    assert sorted(replayed["P"]) == sorted(pipeline)
    wrong = [(c, replayed["P"][c], want) for c, want in pipeline.items() if replayed["P"][c][0] != want[2]]
    assert not wrong, (len(wrong), wrong[:5])
    for c, (rc, frames, error) in pipeline.items():
        assert (rc, frames) == ((0, 3) if error == "-" else (1, 0)), (c, rc, frames, error)


def test_the_derived_booleans_follow_the_fields(golden, replayed):
    """gmc_on pair_on pair_largest report_largest dir_on plane_on persist_on keep_centres of every accepted case without
    options: each is the field it stands for, and keep_centres is any of the things that take the pipe's one count array."""
    _, _, pipeline = golden
    n = 0
    for c, (rc, _, _) in pipeline.items():
        if rc == 0 and c[15] == 0:
            got = tuple(int(v) for v in replayed["P"][c][1].split())
            want = (c[4] >= 0, c[6] > 0 or c[7] == 1, c[7] == 1, c[3] == 1, c[8] >= 0, c[10] == 1, c[12] > 1 or c[14] == 1,
                    bool(c[0] or c[1] or c[3] or c[5] or c[7] or c[9]))
            assert got == tuple(int(v) for v in want), (c, got, want)
            n += 1
    assert n > 200
