"""The decoder layers' host routes, BIT FOR BIT: every case of tests/decoder_route_cases.py -- prefill, continued prefill, decode
steps and training on two-layer Qwen3, Llama and Phi-3 decoders, under every route switch -- against
tests/golden/decoder_route_bits.json (the e2m1 decode step's cases: decoder_route_bits_fp4.json, recorded likewise at the commit
that brought that form; the FP8 KV cache's, the whole-stack step's and the head's: decoder_route_bits_cache.json, recorded before
those routes were folded onto one cache-kind rule), recorded once (twice, with equal results) with the Python of the commit named inside it on
this build of the library, before prefill.py's routes were rewritten around one switch table, one admission function and one
descriptor cache.  Per case: the SHA-256 of each call's last hidden state, of every layer's cached keys and values, of the
training cases' output and gradients, and the deltas of the route counters.  The kernels and their order did not change, so a
digest that moves is a changed launch sequence or operand: find it.  The fixture is never re-recorded by this file.

The host half (no GPU) checks that the fixture lists exactly the cases, that every case took the route it is about, and that the
seeded inputs are not degenerate."""
import json

import pytest
import torch

import decoder_route_cases as C


@pytest.fixture(scope="module")
def fixture():
    cases = {}
    for path, ids in C.FIXTURES.items():
        f = json.loads(path.read_text())
        assert len(f["recorded_at_commit"]) == 40 and sorted(f["cases"]) == sorted(ids) == sorted(C.case_ids(path))
        cases.update(f["cases"])
    return cases


ALL_GROUPS = {**C.GROUPS, **C.FP4_GROUPS, **C.CACHE_GROUPS}


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(ALL_GROUPS))
def test_route_bits(fixture, group):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops
    ops.device_check()
    bad = {}
    for cid in ALL_GROUPS[group]:
        got, want = C.run_case(cid), fixture[cid]
        moved = sorted(k for k in set(got["digests"]) | set(want["digests"]) if got["digests"].get(k) != want["digests"].get(k))
        if moved or got["stats"] != want["stats"]:
            bad[cid] = (moved, got["stats"], want["stats"])
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------- host: cases and inputs
def test_fixture_lists_exactly_the_cases(fixture):
    assert sorted(fixture) == sorted(C.ALL_CASES) == sorted(c for g in ALL_GROUPS.values() for c in g)
    for cid, want in C.FP4_COUNTERS.items():                  # the e2m1 cases: the form each layer ran in, exactly
        got = {k: v for k, v in fixture[cid]["stats"].items() if k.startswith(("w4_stats.", "w8_stats."))}
        assert got == want, (cid, got)
    for cid, want in C.CACHE_COUNTERS.items():                # the mixed cache ran layer by layer; the head at every step
        assert fixture[cid]["stats"] == want, (cid, fixture[cid]["stats"])
    for cid, c in C.CACHE_CASES.items():                      # an e4m3 layer is pinned as what it holds: codes and scales
        d = fixture[cid]["digests"]
        kv8 = any(c["flags"].get(k) for k in ("kv8", "kv8_continued", "stack_kv8"))
        assert [f"key_scales{i}" in d and f"value_scales{i}" in d for i in range(2)] == [kv8, kv8 and not c.get("mixed")], cid
    for cid, c in C.ALL_CASES.items():
        f = fixture[cid]
        for counter in c["expect"]:                       # the route the case is about was taken when it was recorded
            assert f["stats"].get(counter, 0) > 0, (cid, counter)
        want = {"out", "grad.x"} if c["train"] else \
            {k for k, on in (("prefill", c["cache"] != "stock"), ("chunk", c["chunk"])) if on} | {f"step{t}" for t in range(c["steps"])}
        if c["cache"] is not None:
            want |= {f"{n}{i}" for n in ("keys", "values") for i in range(2)}
        assert want <= set(f["digests"]), (cid, want - set(f["digests"]))
        assert len(set(f["digests"].values())) == len(f["digests"]), cid     # no two tensors of a case alike
    # the training cases carry gradients: all of layer 0, or the adapters'
    assert sum(k.startswith("grad.layers.0.") for k in fixture["r-Q-train"]["digests"]) == 11
    assert sum(k.startswith("grad.layers.0.") for k in fixture["s-P-train-phi3"]["digests"]) == 6
    t = fixture["t-Q-train-lora"]["digests"]
    assert sum(".lora_A." in k for k in t) == sum(".lora_B." in k for k in t) == 10


def test_inputs_are_what_the_cases_promise():
    assert C.S0 % 64 not in (0, C.S0) and C.S0 > 64                    # two key tiles, the second ragged
    for cid, c in C.ALL_CASES.items():
        x = C.embeds(c, "x_prefill", c["S"])
        assert x.shape[0] == c["B"] and x.std() > 0.3 and (c["B"] == 1 or not torch.equal(x[0], x[1]))
        for b, p in enumerate(c["left"] or ()):                        # pads where the case says, and not in every sequence
            m = C.mask(c, c["S"] + 3)
            assert (m[b, :p] == 0).all() and (m[b, p:] == 1).all()
        for b, p in enumerate(c["right"] or ()):
            m = C.mask(c, c["S"])
            assert (m[b, :c["S"] - p] == 1).all() and (m[b, c["S"] - p:] == 0).all()
        for pads in (c["left"], c["right"]):
            assert pads is None or (min(pads) == 0 and max(pads) > 0), cid
        if c["model"] == "P":                                           # both sides of the window
            assert c["S"] in (12, 24) and 12 < C.WINDOW < 24
    c = C.CASES["q-Q-lora-merged-and-disabled"]
    m = C.wrap(C.build_model("Q"), c)
    from u2tokenizer_amd.lora import LoRALinear, adapter_of, base_only_of
    wrappers = {n: w for n, w in m.model.layers[0].named_modules() if isinstance(w, LoRALinear)}
    assert sorted(n.rsplit(".", 1)[-1] for n in wrappers) == sorted(C.LORA_TARGETS)
    for n, w in wrappers.items():
        A, B = w.lora_A["default"].weight, w.lora_B["default"].weight
        assert A.dtype == B.dtype == torch.float32 and A.shape[0] == 16 and A.abs().min() > 0 and B.abs().min() > 0
        off = n.rsplit(".", 1)[-1] in c["off"]
        assert (adapter_of(w) is None) == off and (base_only_of(w) is not None) == off
    p = C.wrap(C.build_model("P"), C.CASES["p-P-lora-packed-qkv"])
    assert adapter_of(p.model.layers[1].self_attn.qkv_proj) is not None and type(p.model.layers[1].mlp.gate_up_proj) is torch.nn.Linear
