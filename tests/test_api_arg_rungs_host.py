"""CPU tier: the order and the text of the argument ladders of the derived scans' entry points (csrc/mtgpu_api.hip over
csrc/api_common.h) against tests/golden/api_arg_rungs.json.

tests/api_arg_rungs.py holds the table of calls — every `_device` and host form of sweep, activity, zones, blobs, gmc,
gmc_blobs and dir with a NULL context and one or two broken rungs — and its recorder, which wrote the fixture from a
build of the commit the fixture names.  This test only compares: which rung answers first, and the text it answers with,
are part of the ABI's observable behaviour.  A deliberate change to a ladder records the fixture anew from the commit
that makes it; nothing here can update it.
"""
import json

import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import api_arg_rungs as rungs

GOLDEN = json.load(open(rungs.FIXTURE))


def test_fixture_covers_the_table():
    assert sorted(GOLDEN["answers"]) == sorted(rungs.TABLE) and len(GOLDEN["recorded_from"]) >= 7
    for entry in rungs.TABLE:
        assert sorted(GOLDEN["answers"][entry]) == sorted(case for case, _ in rungs.cases_of(entry)), entry
    # every form of seven features; the pairs are what shows an order
    assert len(rungs.TABLE) == 14 and sum("+" in case for e in rungs.TABLE for case, _ in rungs.cases_of(e)) > 500


@pytest.mark.parametrize("entry", sorted(rungs.TABLE))
def test_ladder_answers_as_recorded(entry):
    got, want = rungs.answers(m.load_library(), entry), GOLDEN["answers"][entry]
    bad = {case: {"want": want[case], "got": got[case]} for case in want if got[case] != want[case]}
    assert not bad, f"{entry}: {len(bad)} of {len(want)} answers moved: {json.dumps(dict(list(bad.items())[:6]), indent=1)}"
    assert all(rc == _abi.MT_ERR_INVALID and text for rc, text in got.values()), entry
