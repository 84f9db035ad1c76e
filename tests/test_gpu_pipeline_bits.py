"""The three module forwards of csrc/pipeline.hip (ViT tower, pooling projector, u2Tokenizer), BIT FOR BIT and LAUNCH FOR LAUNCH:
the SHA-256 of every output's bytes and the launch records of u2tok_profile_collect2 (count, flops and bytes per category) of
every case of tests/pipeline_cases.py against tests/golden/pipeline_bits.json, recorded once with the library of the commit named
inside it -- before pipeline.hip's forwards became stage functions over named weight records.  The parity tests hold these
forwards to a tolerance against the oracle; a stage wired to a neighbouring weight of the same shape, a launch that moved or went
missing, a buffer carved elsewhere can pass there.  Here every case compares equal, with no allowance: the kernels involved have
no atomics and the recording was byte-identical between two processes.  The fixture is never re-recorded by this file.

The host half (no GPU) checks that the fixture lists exactly the cases, and that the tokenizer inputs can expose a mis-wired stage:
exchanging two rows of v_token changes the float64 oracle's output."""
import json

import pytest
import torch

import pipeline_cases as P


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


@pytest.fixture(scope="module")
def fixture():
    f = json.loads(P.FIXTURE.read_text())
    assert len(f["recorded_at_commit"]) == 40
    return f["cases"]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(P.specs()))
@pytest.mark.parametrize("elem", list(P.DTYPES))
def test_output_bits_and_launch_records(ops, fixture, elem, cid):
    got, want = P.run_case(ops, elem, cid), fixture[f"{elem}-{cid}"]
    moved = sorted(k for k in set(got["sha"]) | set(want["sha"]) if got["sha"].get(k) != want["sha"].get(k))
    assert not moved, f"outputs changed bits: {moved}"
    assert got["profile"] == want["profile"], "the launches changed: per category " + str(got["profile"]) + " against " + str(want["profile"])


# ------------------------------------------------------------------------------------------------------------- host: the cases
def test_fixture_lists_exactly_the_cases():
    cases = json.loads(P.FIXTURE.read_text())["cases"]
    assert sorted(cases) == sorted(P.case_ids()) and len(set(P.case_ids())) == len(P.case_ids())
    for cid, rec in cases.items():
        assert rec["sha"] and all(len(v) == 64 for v in rec["sha"].values()), cid
        assert sorted(rec["profile"]) == ["bytes", "count", "flops"] and all(len(v) == P.NCAT for v in rec["profile"].values()), cid
        assert sum(rec["profile"]["count"]) > 0, cid
    # what the case list promises: the ten shared cases, both tap cases, three options on three cases, the shapes and the ViT grid
    ids = list(P.specs())
    assert all(f"tok-{n}" in ids for n in P.TOKENIZER_CASES) and len(P.TOKENIZER_CASES) == 10
    assert len([i for i in ids if i.startswith("taps-")]) == 2 and len([i for i in ids if i.endswith("0") and i.startswith("tok-")]) == 9
    assert len([i for i in ids if i.startswith("vit-")]) == 6 and len([i for i in ids if i.startswith("spp-")]) == len(P.SPP_CASES)
    c = P.TOK_CONFIGS
    assert c["d40_1l"]["E"] // c["d40_1l"]["heads"] == 40 and c["e256_8l"]["layers"] == 8 and c["e256_7l"]["layers"] == 7
    assert {k: v for k, v in c["e256_8l"].items() if k != "layers"} == {k: v for k, v in c["e256_7l"].items() if k != "layers"}


@pytest.mark.parametrize("name", list(P.TOK_CONFIGS))
def test_inputs_expose_a_miswired_stage(name):
    """Two rows of v_token exchanged (another chunk and another token position): the float64 oracle's output moves, so data that
    reaches a stage in the wrong order, or a stage that ignores its input, cannot give the recorded bits by accident."""
    from helpers import module_sd, tok_cfg
    from oracle import u2_oracle as O
    c = P.TOK_CONFIGS[name]
    sd = {k: v.double() for k, v in module_sd(P._mk_tok(c), "u2tokenizer.", c["seed"], lively=c.get("lively", False)).items()}
    v, t = P.tokenizer_inputs(c)
    v, t = v.double(), t.double()
    a, b = P.swapped_rows(c)
    assert a != b and a[1] != b[1] and a[2] != b[2] and not torch.equal(v[a], v[b])
    v2 = v.clone()
    v2[a], v2[b] = v[b], v[a]
    with torch.no_grad():
        out, _ = O.tokenizer_forward(sd, "u2tokenizer", v, t, tok_cfg(c))
        out2, _ = O.tokenizer_forward(sd, "u2tokenizer", v2, t, tok_cfg(c))
    assert torch.isfinite(out).all() and torch.isfinite(out2).all()
    assert not torch.equal(out, out2), name
