"""GPU tier (`-m gpu`): GpuMotionScanner::initialize and run_scan_pipeline against tests/golden/host_mode_matrix.json, their
answers at the commit before csrc/host/scan_request.hpp (tests/host_mode_matrix.py; tests/cpp/mode_matrix_probe.cpp has
the encodings).  The probe is built against this tree and replays every case with at most two settings off their
defaults, and the 36 ordered "the previous video ran X, this video asks Y" pairs on one pooled backend."""
import os

import pytest

import mvtrim_amd as m

import host_mode_matrix as hm

pytestmark = pytest.mark.gpu

PKG = os.path.dirname(m.LIB_PATH)
CENTRES, LARGEST = 0, 1


@pytest.fixture(scope="module")
def golden():
    return hm.load()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return hm.build_probe(str(tmp_path_factory.mktemp("mode_matrix") / "mode_matrix_probe"), PKG)


def test_initialize_answers_the_singles_and_pairs_as_the_parent_did_and_leaves_nothing_behind(golden, probe):
    """Same answer, and after a success the same mode, settings and mask on the pipe.  After a FAILED initialize() the pipe
    here carries no mode and no mask, which is what the parent's comments promised and its undo lists did not do.  In the
    fixture 3 097 of the 6 882 failed cases leave a mode on the pooled pipe: the blob setting where compensation was refused
    behind it ("compensation and blobs are not together yet", 1 728; "report_vector needs set_gmc", 864), the blob or the
    compensation setting where the keep mask's size was refused behind them (504), and the previous case's blob setting
    where a persist rung answered ahead of the pipe (1).  The last lines count them."""
    grid, scanner, _ = golden
    got_grid, rows = hm.run_probe(probe, "scanner", 2)
    assert got_grid == grid and len(rows["S"]) > 100
    for c, (answer, state) in rows["S"].items():
        want = scanner[c]
        assert answer == want[0], (c, answer, want)
        assert state == (want[1] if answer == "ok" else "keep=0 " + hm.ALL_OFF), (c, answer, state)
    failed = [v for v in scanner.values() if v[0] != "ok"]
    stale = [v for v in failed if v[1] != "keep=0 " + hm.ALL_OFF]
    assert (len(stale), len(failed)) == PARENT_LEFT_BEHIND, (len(stale), len(failed))


PARENT_LEFT_BEHIND = (3097, 6882)


def test_run_scan_pipeline_answers_the_singles_and_pairs_as_the_parent_did(golden, probe):
    grid, _, pipeline = golden
    _, rows = hm.run_probe(probe, "pipeline", 2)
    assert len(rows["P"]) > 300
    wrong = [(c, got, pipeline[c]) for c, got in rows["P"].items() if got != pipeline[c]]
    assert not wrong, (len(wrong), wrong[:5])


def asks(mode, masked):
    """mode_matrix_probe.cpp's asks(): the scanner case of each of the six things a video can ask."""
    c = [1, 0, 0, -1, 0, 0, CENTRES, -1, 0, 0, 1 if masked else 0, -1]
    if mode == 1:
        c[1], c[2] = 3, 1
    if mode == 2:
        c[3], c[4] = 4, 1
    if mode == 3:
        c[5], c[6] = 3, LARGEST
    if mode == 4:
        c[7], c[8] = 0x5B, 1
    if mode == 5:
        c[9], c[8] = 1, 1
    return tuple(c)


def test_a_pooled_pipe_carries_exactly_this_videos_mode_and_mask_whatever_the_previous_one_ran(golden, probe):
    """What the order of initialize()'s off and on calls was for: 6 x 6 ordered pairs on ONE backend, the previous video
    with or without a mask.  initialize() succeeds and the pipe's state is that of the same request on a fresh pipe."""
    _, scanner, _ = golden
    _, rows = hm.run_probe(probe, "pooled")
    assert sorted(rows["Q"]) == [(x, y) for x in range(6) for y in range(6)]
    for (x, y), (answer, state) in rows["Q"].items():
        alone = scanner[asks(y, y % 2 == 1)]
        assert alone[0] == "ok" and answer == "ok" and state == alone[1], (x, y, answer, state, alone)
    assert len({v[1] for v in rows["Q"].values()}) == 6
