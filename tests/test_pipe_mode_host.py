"""CPU tier: the tables of csrc/pipe_mode.h against tests/golden/pipe_mode_matrix.json, the answers a GPU gave at the
commit before the pipe's modes became one value (tests/pipe_mode_matrix.py).  A stand-alone program (tests/cpp/
pipe_mode_tables.cpp: the header alone, no HIP, no library, built with the address and undefined-behaviour sanitizers)
prints the 20 refusals, the busy sentences and the report rungs; each must be, character for character, what the recorded
case that reaches it answered."""
import json
import os
import subprocess

import pytest

from mvtrim_amd import _abi

import pipe_mode_matrix as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "csrc")
MODE_NO = {x: i + 1 for i, x in enumerate(pm.MODES)}          # pipe_mode's values; 0 is the plain scan (the keep mask's slot)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pipe_mode") / "pipe_mode_tables")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "pipe_mode_tables.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    rows = {"refusal": {}, "busy": {}, "report": {}}
    for line in out.stdout.splitlines():
        kind, *f = line.split("\t")
        if kind == "refusal":
            rows[kind][int(f[0]), int(f[1])] = (int(f[2]), f[3])
        elif kind == "busy":
            rows[kind][int(f[0]), f[1]] = f[2]
        else:
            rows[kind][int(f[0]), int(f[1]), int(f[2])] = (int(f[3]), f[4])
    return rows


@pytest.fixture(scope="module")
def golden():
    with open(pm.FIXTURE) as f:
        return pm.unpack(json.load(f))


def test_the_twenty_refusals_are_the_recorded_ones(tables, golden):
    assert len(tables["refusal"]) == 20
    for x in pm.MODES:
        for y in pm.MODES:
            if x != y:
                on_x, on_y, off_y = golden[f"a/{x}/{y}"]
                assert on_x["rc"] == 0 and on_y["rc"] != 0 and off_y["rc"] == 0
                assert tables["refusal"][MODE_NO[x], MODE_NO[y]] == (on_y["rc"], on_y["error"]), (x, y)
                assert on_y["state"] == on_x["state"] == off_y["state"]       # a refusal and a foreign off form leave x alone


def test_the_busy_sentences_are_the_recorded_ones(tables, golden):
    assert len(tables["busy"]) == 12
    for x in pm.MODES + ["keep"]:
        for busy, state in (("fill", "being filled"), ("flight", "in flight")):
            for form in ("on", "off"):
                refused = golden[f"e/{x}/{busy}/{form}"][0 if form == "on" else 1]
                assert refused["rc"] == _abi.MT_ERR_BUSY
                assert refused["error"] == tables["busy"][MODE_NO.get(x, 0), state], (x, busy, form)


def test_the_report_rungs_are_the_recorded_ones(tables, golden):
    assert len(tables["report"]) == 5 * 2 * 7
    for x in pm.MODES:
        for pipe in "cn":
            for r in range(-1, 6):
                got = golden[f"c/{x}/{pipe}/{r}"][0]
                code, text = tables["report"][MODE_NO[x], int(pipe == "c"), r]
                assert (got["rc"], got["error"]) == (code, text), (x, pipe, r)
