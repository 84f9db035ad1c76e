"""What the dry runs of csrc/pipeline.hip ANSWER (no GPU): u2tok_tokenizer_workspace_bytes, u2tok_vit_workspace_bytes and
u2tok_spp_workspace_bytes for both builds, at default options and with kmajor_b = 0, over the configs of
tests/pipeline_cases.py (workspace_configs: the GPU cases' configs, the benchmark's sizes, every boolean flipped, 0 / 1 / 7 / 8
layers, the three attention types at B = 1 and 2, ViT depths and geometries, both poolings, and the configs the argument checks
refuse) against tests/golden/pipeline_workspace.json, recorded with the library of the commit named inside it.  A forward is
written once and sized by running it dry, so an answer that moves is an arena request that changed size or order, or an argument
check that moved.  Every answer is compared equal; the fixture is never re-recorded by this file."""
import json

import pipeline_cases as P


def test_workspace_answers_are_the_recorded_ones():
    f = json.loads(P.WS_FIXTURE.read_text())
    assert len(f["recorded_at_commit"]) == 40
    want, got = f["bytes"], P.workspace_answers()
    assert sorted(want) == sorted(P.workspace_ids()) == sorted(got)
    moved = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not moved, f"{len(moved)} of {len(want)} answers changed (now, recorded): {moved}"


def test_fixture_holds_accepted_and_refused_answers_of_every_export():
    want = json.loads(P.WS_FIXTURE.read_text())["bytes"]
    cfgs = P.workspace_configs()
    for elem in P.DTYPES:
        for options in P.WS_OPTIONS:
            tag = f"{elem}-{P._opt_tag(options)}-"
            for export in ("tokenizer", "vit", "spp"):
                answers = {cid: want[tag + cid] for cid, (ex, _) in cfgs.items() if ex == export}
                assert any(v > 0 for v in answers.values()) and any(v == 0 for v in answers.values()), (tag, export)
                # the refused configs are the ones named so, and no other
                assert {cid for cid, v in answers.items() if v == 0} == {cid for cid in answers if "-refused-" in cid}, (tag, export)
