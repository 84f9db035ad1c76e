"""GPU: u2tok_sample_warp (csrc/sample.hip) through ops.sample_warp and FusedSamplingWarper against the float64 reference of
tests/sampling_cases.py.

Acceptance rule (sampling_cases.check): a token whose float64 ascending cumulative mass lies within 1e-5 of 1 - top_p is undecided and
may go either way; the reference alone must show at most 4 such tokens per row (asserted, not skipped); EVERY other element of the
output equals the reference bit for bit, kept values and -inf alike.  Top-k-only calls have no undecided tokens and also equal
transformers' TopKLogitsWarper on the GPU bit for bit."""
import math

import pytest
import torch

import sampling_cases as SC

pytestmark = pytest.mark.gpu
D = "cuda:0"
NEG = -math.inf


@pytest.fixture(scope="module")
def ops():
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    return _ops


def _run(ops, x, params, **kw):
    T, k, p, mk = params
    return ops.sample_warp(x.to(D), T, k, p, mk, **kw)


# ------------------------------------------------------------------------------------------------ random logits
@pytest.mark.parametrize("bf16_values", [False, True], ids=["fp32", "bf16vals"])
@pytest.mark.parametrize("rows,V", SC.SHAPES, ids=[f"{r}x{v}" for r, v in SC.SHAPES])
def test_random_logits(ops, rows, V, bf16_values):
    x = SC.logits(rows, V, seed=0, bf16_values=bf16_values)
    xg = x.to(D)
    for name, prm in SC.PARAMS.items():
        out = ops.sample_warp(xg, *prm)
        n = SC.check(out, x, prm, what=f"{rows}x{V} {name}")
        if prm[2] == 1.0:     # top-k only: exact, and what the stock warper gives on the GPU, ties included
            assert n == 0
            want, _ = SC.stock(xg, *prm)
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), name


def test_temperature_is_one_correctly_rounded_division(ops):
    """kept values are fp32(x / T) bit for bit: the IEEE division, which is what `scores / T` gives on the CPU.  (On the GPU torch
    divides a tensor by a Python scalar as a multiplication by the fp32 reciprocal, which can land one ulp away; the warper's
    definition is the division.)"""
    x = SC.logits(3, 4097, seed=2)
    for T in (0.7, 0.2, 1.3, 3.0):
        out = ops.sample_warp(x.to(D), T, 0, 0.9, 1)
        kept = out > NEG
        assert kept.any() and torch.equal(out[kept].cpu().view(torch.int32), (x / T)[kept.cpu()].view(torch.int32)), T
        by_reciprocal = (x.to(D) / T)[kept].view(torch.int32)
        assert int((out[kept].view(torch.int32) - by_reciprocal).abs().max()) <= 1, T


# ------------------------------------------------------------------------------------------------ hard rows
def _hard_rows(V):
    g = torch.Generator().manual_seed(V)
    base = torch.randn(V, generator=g)
    rows = {}
    r = base.clone(); r[V // 3] = 12.0
    rows["dominant"] = (r, (1.0, 0, 0.9, 1))                       # one token above top_p: exactly one kept
    rows["uniform"] = (torch.full((V,), 0.25), (1.0, 0, 0.9005, 1))   # all equal: the highest indices (boundary between two tokens)
    r = base.clone() - 6.0; r[torch.randperm(V, generator=g)[:40]] = 1.5
    rows["tie group"] = (r, (1.0, 0, 0.6, 1))                      # 40 equal values carry ~all the mass: the boundary falls inside
    r = torch.full((V,), NEG); r[1], r[V // 2], r[V - 1] = 0.5, 1.5, 1.0
    rows["-inf but 3"] = (r, (0.7, 0, 0.9, 1))
    r = base.clone().abs().neg() - 1.0; r[3], r[7], r[11], r[20] = 2.0, 1.0, 0.0, -0.0
    rows["signed zeros at k"] = (r, (1.0, 3, 1.0, 1))              # k-th largest is +0.0; -0.0 ties with it: 4 kept
    r = base.clone().abs().neg() - 1.0; r[3], r[7], r[11], r[20] = 2.0, 1.0, -0.0, 0.0
    rows["signed zeros at k, then p"] = (r, (1.0, 3, 0.99, 1))
    r = torch.full((V,), -1e4); r[torch.randperm(V, generator=g)[:7]] = 1e4
    rows["+-1e4"] = (r, (1.0, 0, 0.9, 1))                          # masses of exactly 0 below
    rows["+-1e4, T"] = (r, (0.7, 50, 0.5, 1))
    rows["k >= V"] = (base * 3, (1.0, V + 5, 0.9, 1))
    rows["k == V"] = (base * 3, (0.7, V, 1.0, 1))
    r = base.clone(); r[V // 3] = 14.0
    rows["min_keep 3, dominant"] = (r, (1.0, 0, 0.9, 3))
    rows["tiny top_p"] = (base * 3, (0.7, 0, 1e-6, 2))             # only min_keep survive
    rows["tiny top_p, k"] = (base * 3, (1.0, 5, 1e-6, 4))
    return rows


@pytest.mark.parametrize("V", [65, 1000])
def test_hard_rows(ops, V):
    for name, (r, prm) in _hard_rows(V).items():
        x = torch.stack([r, r.flip(0), r])          # (the same row three times, once reversed: other indices, the same values)
        out = _run(ops, x, prm)
        SC.check(out, x, prm, what=f"V={V} {name}")
        kept = (out[0] > NEG).nonzero().flatten().tolist()
        ref = (SC.reference(x, *prm)[0][0] > NEG).nonzero().flatten().tolist()
        if name == "dominant":
            assert kept == [V // 3]
        elif name == "uniform":
            assert len(ref) >= 2 and kept == list(range(V - len(ref), V))      # the count of the reference, the highest indices
        elif name == "tie group":
            ties = (r == 1.5).nonzero().flatten().tolist()
            assert 0 < len(ref) < 40 and kept == ties[-len(ref):]
        elif name == "-inf but 3":
            assert set(kept) <= {1, V // 2, V - 1} and len(kept) >= 1
        elif name == "signed zeros at k":
            assert kept == [3, 7, 11, 20] and math.copysign(1.0, out[0, 20].item()) == -1.0
        elif name == "min_keep 3, dominant":
            assert len(kept) == 3
        elif name == "tiny top_p":
            assert len(kept) == 2
        elif name == "tiny top_p, k":
            assert len(kept) == 4
        elif name.startswith("k >= V"):
            assert len(kept) == len(ref)


# ------------------------------------------------------------------------------------------------ layout and determinism
def test_leading_dimensions_aliasing_stream_and_repeat(ops):
    rows, V, pad = 5, 1000, 24
    prm = SC.PARAMS["T0.7_p0.9"]
    x = SC.logits(rows, V, seed=3)
    big_in = torch.full((rows, V + pad), 777.0, device=D)
    big_in[:, :V] = x.to(D)
    big_out = torch.full((rows, V + 2 * pad), -555.0, device=D)
    out = ops.sample_warp(big_in[:, :V], *prm, out=big_out[:, :V])
    assert out.data_ptr() == big_out.data_ptr()
    SC.check(big_out[:, :V], x, prm, what="ld > V")
    assert (big_out[:, V:] == -555.0).all() and (big_in[:, V:] == 777.0).all() and torch.equal(big_in[:, :V].cpu(), x)
    first = big_out[:, :V].clone()
    # in place
    ops.sample_warp(big_in[:, :V], *prm, out=big_in[:, :V])
    assert torch.equal(big_in[:, :V], first) and (big_in[:, V:] == 777.0).all()
    # on a side stream
    xg = x.to(D)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        side = ops.sample_warp(xg, *prm)
    s.synchronize()
    assert torch.equal(side, first)
    # the same call twice: the same bits (also at the large vocabulary, where every histogram is shared by 16 waves)
    y = SC.logits(16, 151936, seed=0, bf16_values=True).to(D)
    for p2 in (SC.PARAMS["p0.9"], SC.PARAMS["T1.3_k50_p0.95_keep2"]):
        a, b = ops.sample_warp(y, *p2), ops.sample_warp(y, *p2)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_wrapper_refuses_what_the_kernel_does_not_take(ops):
    x = torch.zeros(2, 8, device=D)
    for bad in (x.half(), x[:, ::2], x[0], torch.zeros(2, 1, device=D)):
        with pytest.raises(RuntimeError):
            ops.sample_warp(bad, 1.0, 0, 0.9, 1)
    for kw in (dict(temperature=0.0), dict(top_p=0.0), dict(top_p=1.5), dict(min_keep=0), dict(top_k=-1)):
        with pytest.raises(RuntimeError):
            ops.sample_warp(x, **kw)


def test_a_nan_stays_in_its_row(ops):
    prm = SC.PARAMS["k50_p0.9"]
    x = SC.logits(3, 1000, seed=4)
    x[1, 17] = math.nan
    out = _run(ops, x, prm)
    torch.cuda.synchronize()
    SC.check(out[[0, 2]], x[[0, 2]], prm, what="rows next to a NaN row")
    x[1] = NEG                                     # a row of nothing but -inf; another with +inf
    x[2, 5] = math.inf
    out = _run(ops, x, SC.PARAMS["T0.7_p0.9"])
    torch.cuda.synchronize()
    SC.check(out[[0]], x[[0]], SC.PARAMS["T0.7_p0.9"], what="row next to -inf / +inf rows")


# ------------------------------------------------------------------------------------------------ FusedSamplingWarper / generate
def test_fused_warper_runs_the_kernel_on_gpu_scores(ops):
    from u2tokenizer_amd import sampling
    x = SC.logits(3, 4097, seed=5)
    _, procs = SC.stock(x, 0.7, 50, 0.9)
    f = sampling.fuse_warpers(procs)[0]
    n = dict(sampling.stats)
    out = f(None, x.to(D))
    assert sampling.stats["fused"] == n["fused"] + 1 and sampling.stats["stock"] == n["stock"]
    SC.check(out, x, (0.7, 50, 0.9, 1), what="FusedSamplingWarper")
    f(None, x.to(D).bfloat16())                    # not fp32: the stock warpers
    assert sampling.stats["stock"] == n["stock"] + 1


def _lm(**switches):
    from u2tokenizer_amd import language_model as LM, synth
    cfg = LM.u2Qwen3Config(vocab_size=512, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, max_position_embeddings=512,
                           num_attention_heads=4, num_key_value_heads=2, head_dim=128, tie_word_embeddings=False, pad_token_id=0,
                           bos_token_id=1, eos_token_id=None)
    for k, v in switches.items():
        setattr(cfg, k, v)
    m = LM.u2Qwen3ForCausalLM(cfg)
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m.to(torch.bfloat16).to(D).eval()


def test_generate_samples_through_the_fused_warper(ops, monkeypatch):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopPLogitsWarper
    from u2tokenizer_amd import prefill, sampling
    new = 8
    m = _lm(u2_fused_sampling=True)
    ids = torch.randint(3, 512, (2, 12), generator=torch.Generator().manual_seed(5)).to(D)
    kw = dict(do_sample=True, top_p=0.9, temperature=0.7, max_new_tokens=new, output_logits=True, output_scores=True,
              return_dict_in_generate=True)
    draws = []
    real = torch.multinomial
    monkeypatch.setattr(torch, "multinomial", lambda *a, **k: (draws.append(1), real(*a, **k))[1])
    seen = []
    real_get = type(m)._get_logits_processor
    monkeypatch.setattr(type(m), "_get_logits_processor", lambda self, *a, **k: (seen.append(real_get(self, *a, **k)), seen[-1])[1])

    n, d = dict(sampling.stats), dict(prefill.stats)
    torch.manual_seed(11)
    g = m.generate(None, ids, **kw)
    assert sampling.stats["fused"] == n["fused"] + new and sampling.stats["stock"] == n["stock"]
    layers = m.config.num_hidden_layers
    assert prefill.stats["prefill"] == d["prefill"] + layers and prefill.stats["decode"] == d["decode"] + (new - 1) * layers
    assert len(draws) == new and [type(p) for p in seen[-1]] == [sampling.FusedSamplingWarper]
    f = seen[-1][0]      # (generate may add its own default top_k to the caller's arguments: the reference takes what the warper holds)
    assert (f.temperature, f.top_p, f.min_tokens_to_keep) == (0.7, 0.9, 1)
    prm, stock_types = (f.temperature, f.top_k, f.top_p, f.min_tokens_to_keep), [type(p) for p in f.stock]
    assert len(g.scores) == new and len(g.logits) == new
    for t in range(new):
        logits, scores = g.logits[t].float().cpu(), g.scores[t]
        assert scores.dtype == torch.float32
        SC.check(scores, logits, prm, what=f"step {t}")
        picked = scores.gather(1, g.sequences[:, t - new if g.sequences.shape[1] > new else t][:, None])
        assert torch.isfinite(picked).all(), t

    # the switch off: the stock objects, the fused counter untouched, one draw per step as before
    m.config.u2_fused_sampling = False
    n, before = dict(sampling.stats), len(draws)
    torch.manual_seed(11)
    g2 = m.generate(None, ids, **kw)
    assert [type(p) for p in seen[-1]] == stock_types and TemperatureLogitsWarper in stock_types and TopPLogitsWarper in stock_types
    assert sampling.stats == n and len(draws) == before + new
