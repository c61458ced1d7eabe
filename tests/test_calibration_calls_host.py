"""The call transcript of cyclistsocialforce_amd/calibration.py against the one recorded before the module was split into layers
(tests/golden/calibration_calls.json, tests/calibration_calls_common.py; no GPU, no library): the sequence and the arguments of every
engine call, every returned error, trajectory and downhill-simplex result to the last bit, and for every refusal the exception type,
the full message and whether an engine had been made.  Equality, entry by entry."""
import json
import os

import pytest

import calibration_calls_common as cc

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["interaction " + name for name in cc.INTERACTION] + ["simplex", "simplex auxfuncs"]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "calibration_calls.json")) as f:
        return json.load(f)


def _as_recorded(log):
    return json.loads(json.dumps(log))                            # (tuples become lists, as in the file)


def _compare(got, want):
    for at, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"entry {at}: {g!r} where {w!r} was recorded"
    assert len(got) == len(want)


def test_every_recorded_case_is_run(recorded):
    assert sorted(recorded) == sorted(CASES + ["refusals"])
    assert [e[1] for e in recorded["refusals"]] == list(cc.REFUSALS)


@pytest.mark.parametrize("case", CASES)
def test_calls_and_results_are_the_recorded_ones(recorded, case):
    if case.startswith("interaction "):
        got = cc.interaction_case(case[len("interaction "):])
    else:
        got = cc.simplex_case(case.endswith("auxfuncs"))
    _compare(_as_recorded(got), recorded[case])


def test_every_refusal_is_the_recorded_one(recorded):
    _compare(_as_recorded(cc.refusal_case()), recorded["refusals"])
