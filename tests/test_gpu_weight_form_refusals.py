"""What the few-rows exports and the two halves of the decode step answer to every way of saying a weight form -- the returned
status of each case of tests/weight_form_refusal_cases.py against tests/golden/weight_form_refusals.json, recorded with the library of
the commit named inside it.  The form is decided once at the C boundary; whatever carries it below must accept and refuse what
that library accepted and refused.  A status that moves is a changed check: find it.  The fixture is never re-recorded by this
file.

Every pointer of a case is a device allocation sized for the largest accepted call (the case file asserts it), so a call that is
wrongly accepted computes into scratch.

The host half (no GPU) checks that the fixture lists exactly the cases and that it cannot be satisfied by refusing everything."""
import json

import pytest
import torch

import weight_form_refusal_cases as W


@pytest.fixture(scope="module")
def fixture():
    f = json.loads(W.FIXTURE.read_text())
    assert len(f["recorded_at_commit"]) == 40
    return f["status"]


@pytest.mark.gpu
def test_every_status_is_the_recorded_one(fixture):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    got = W.run_all()
    moved = {k: (got.get(k), fixture.get(k)) for k in sorted(set(got) | set(fixture)) if got.get(k) != fixture.get(k)}
    assert not moved, f"{len(moved)} of {len(got)} statuses changed (got, recorded): {dict(list(moved.items())[:12])}"


# ------------------------------------------------------------------------------------------------------------- host: the case list
def test_fixture_lists_exactly_the_cases(fixture):
    assert sorted(fixture) == sorted(W.case_ids())
    W.largest_call_fits()


def test_fixture_holds_accepted_and_refused_calls(fixture):
    """Per export and per half of the step: the nominal call of every form is accepted, and something is refused"""
    for ex in W.ROWS_EXPORTS:
        assert fixture[f"{ex}-nominal"] == 0 and fixture[f"{ex}-pair"] == 0 and fixture[f"{ex}-bias-res-f32"] == 0, ex
        assert fixture[f"{ex}-M65"] == -1 and fixture[f"{ex}-flags4"] == -1 and fixture[f"{ex}-pair-bias"] == -1, ex
        assert fixture[f"{ex}-M64"] == (-1 if ex == "w8" else 0), ex                 # (u2tok_gemm_rows_w8 keeps its 16 rows)
    assert fixture["w8-null-S"] == fixture["w4-null-S"] == -1
    assert fixture["rows-K96"] == 0 and fixture["w8-K96"] == -1 and fixture["w8-K192"] == 0 and fixture["w4-K192"] == -1
    for half, batched in W.HALVES:
        tag = half + ("-batched" if batched else "")
        for wform, name, want in ((0, "none", 0), (0, "all", 0), (2, "all", 0), (2, "none", -1), (0, "scale_o", -1), (2, "scale_o", -1),
                                  (1, "none", -1), (1, "all", -1), (3, "all", -1)):
            assert fixture[f"{tag}-wform{wform}-{name}"] == want, (tag, wform, name)
        assert fixture[f"{tag}-elem-I64"] == 0 and fixture[f"{tag}-e4m3-I64"] == 0 and fixture[f"{tag}-e2m1-I64"] == -1, tag
        assert fixture[f"{tag}-e4m3-I32"] == -1 and fixture[f"{tag}-e2m1-B16"] == 0 and fixture[f"{tag}-e2m1-B65"] == -1, tag
    assert set(fixture.values()) <= {0, -1, -3}
