"""GPU tier (`-m gpu`): the pipe's mode setters against tests/golden/pipe_mode_matrix.json, the answers of the commit
before the modes became one value (tests/pipe_mode_matrix.py: the cases, and how the fixture was recorded).  Every case
is replayed on this build's library and everything is compared: return code, mtgpu_last_error(), and what the five
getters and mtgpu_pipe_has_keep say afterwards.  There is no update path here."""
import json

import pytest

import mvtrim_amd as m

import pipe_lanes_inputs as pl
import pipe_mode_matrix as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(pm.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed(gpu_scanner_factory):
    return pm.answers(m, gpu_scanner_factory(pl.shapes_case()[0]))


def test_the_fixture_holds_exactly_the_tables_cases(golden):
    assert golden["recorded_from"] == "77f0180"
    assert sorted(golden["answers"]) == sorted(c[0] for c in pm.cases())
    assert len(set(golden["sentences"])) == len(golden["sentences"])


def test_every_setter_answers_and_leaves_what_the_parent_did(golden, replayed):
    want = pm.unpack(golden)
    wrong = {k: (replayed[k], want[k]) for k in want if replayed[k] != want[k]}
    assert not wrong, (len(wrong), sorted(wrong)[:10], next(iter(wrong.values())))


def test_the_cases_reach_every_refusal_and_every_busy_word(golden):
    """The table is only as good as its reach: the second step of each of the 20 ordered pairs is a refusal, the six busy
    sentences are there in both states, and so are the three reports that need MT_LAYOUT_CENTRES."""
    want, s = pm.unpack(golden), golden["sentences"]
    refusals = [want[f"a/{x}/{y}"][1] for x in pm.MODES for y in pm.MODES if x != y]
    assert len(refusals) == 20 and all(r["rc"] != 0 and r["error"].startswith("this pipe runs the ") for r in refusals)
    assert sum(t.startswith("a batch of this pipe is being filled") for t in s) == 6
    assert sum(t.startswith("a batch of this pipe is in flight") for t in s) == 6
    assert sum(" needs a pipe with MT_LAYOUT_CENTRES" in t for t in s) == 3
