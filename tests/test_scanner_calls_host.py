"""CPU tier: scanner.py hands the library what it handed it before the wrappers were folded onto shared helpers, and
returns what it returned.  tests/golden/scanner_calls.json was recorded by tests/scanner_calls.py from the scanner.py of
the commit before the fold (docs/rounds/r29_python_fold.md); every case is replayed here on the tree's own file."""
import json

import pytest

import mvtrim_amd as m

import scanner_calls as sc


@pytest.fixture(scope="module")
def golden():
    with open(sc.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def traced():
    return sc.trace(sc.load_scanner())


def test_the_golden_lists_exactly_the_cases_of_the_script(golden):
    assert list(golden["cases"]) == [c[0] for c in sc.cases()]
    assert len(set(golden["cases"])) == len(golden["cases"]) > 700
    assert sorted(set(golden["cases"].values())) == list(range(len(golden["outcomes"])))


def test_every_call_and_every_return_is_the_recorded_one(golden, traced):
    _, outcomes = traced
    wrong = [cid for cid, i in golden["cases"].items() if outcomes[cid] != golden["outcomes"][i]]
    first = wrong[0] if wrong else None
    assert not wrong, (len(wrong), wrong[:20], first and outcomes[first], first and golden["outcomes"][golden["cases"][first]])


def test_the_recorded_cases_reach_the_library_and_its_refusals(golden):
    """The fixture is not vacuous: it holds calls of every scan symbol the wrappers use, returns and every kind of refusal."""
    outcomes = golden["outcomes"]
    symbols = {c[0] for o in outcomes for c in o["calls"]}
    assert len(symbols) >= 50 and {"mtgpu_scan_frames_device", "mtgpu_scan_blobs_device", "mtgpu_pipe_set_plane"} <= symbols
    raised = {o["raises"][0] for o in outcomes if "raises" in o}
    assert {"ValueError", "AssertionError"} <= raised
    sentences = " | ".join(o["raises"][1] for o in outcomes if "raises" in o)
    for words in ("go together", "keep has shape", "planes has shape", "bytes in 0 .. 255", "is not one of", "one element per frame",
                  "timestamps for", "does not fit int32", "report is", "plane has dtype", "packed keep has shape"):
        assert words in sentences, words


def test_every_public_signature_is_the_recorded_one(golden, traced):
    signatures, _ = traced
    assert signatures == golden["signatures"]


def test_every_exported_name_is_still_exported(golden):
    assert sorted(m.__all__) == golden["all"]
    assert [n for n in golden["all"] if not hasattr(m, n)] == []
