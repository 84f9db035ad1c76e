"""CPU: the sampling warper's host side (u2tokenizer_amd/sampling.py) -- which processor lists `fuse_warpers` rewrites and which it
leaves alone, the `config.u2_fused_sampling` switch in `_get_logits_processor`, the CPU fallback of FusedSamplingWarper -- the float64
reference of tests/sampling_cases.py against the stock transformers warpers, and the argument guards of u2tok_sample_warp in both
builds of the library (no launch: every call returns before it)."""
import ctypes as C
import math

import pytest
import torch
from transformers import GenerationConfig
from transformers.generation.logits_process import (LogitsProcessorList, MinLengthLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                    TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper)

import sampling_cases as SC
from u2tokenizer_amd import _lib, language_model as LM, sampling
from u2tokenizer_amd.sampling import FusedSamplingWarper, fuse_warpers


def _T(t=0.7):
    return TemperatureLogitsWarper(t)


def _K(k=50, **kw):
    return TopKLogitsWarper(top_k=k, **kw)


def _P(p=0.9, **kw):
    return TopPLogitsWarper(top_p=p, **kw)


# ------------------------------------------------------------------------------------------------ fuse_warpers
@pytest.mark.parametrize("run,want", [
    ((_T, _K, _P), (0.7, 50, 0.9)), ((_T, _P), (0.7, 0, 0.9)), ((_T, _K), (0.7, 50, 1.0)), ((_K, _P), (1.0, 50, 0.9)),
    ((_K,), (1.0, 50, 1.0)), ((_P,), (1.0, 0, 0.9))])
def test_every_accepted_run_becomes_one_fused_warper(run, want):
    head, tail = RepetitionPenaltyLogitsProcessor(1.1), MinLengthLogitsProcessor(1, 2)
    stock = [f() for f in run]
    out = fuse_warpers(LogitsProcessorList([head] + stock + [tail]))
    assert isinstance(out, LogitsProcessorList) and len(out) == 3
    assert out[0] is head and out[2] is tail                      # outside the run: the same objects, in place
    f = out[1]
    assert type(f) is FusedSamplingWarper and (f.temperature, f.top_k, f.top_p) == want and f.min_tokens_to_keep == 1
    assert len(f.stock) == len(stock) and all(a is b for a, b in zip(f.stock, stock))
    assert fuse_warpers(stock)[0].top_p == want[2]                # a plain list is taken too


class _MyTopP(TopPLogitsWarper):
    pass


class _MyTemp(TemperatureLogitsWarper):
    pass


@pytest.mark.parametrize("name,procs", [
    ("wrong order", lambda: [_P(), _K()]),
    ("temperature last", lambda: [_P(), _T()]),
    ("top-k before temperature", lambda: [_K(), _T(), _P()]),
    ("subclass of top-p", lambda: [_T(), _MyTopP(top_p=0.9)]),
    ("subclass of temperature", lambda: [_MyTemp(0.7), _P()]),
    ("filter value", lambda: [_T(), _P(filter_value=-1e4)]),
    ("filter value of top-k", lambda: [_K(filter_value=0.0), _P()]),
    ("processor in between", lambda: [_T(), RepetitionPenaltyLogitsProcessor(1.1), _P()]),
    ("lone temperature", lambda: [_T()]),
    ("two top-p", lambda: [_P(), _P(0.5)]),
    ("different floors", lambda: [_K(min_tokens_to_keep=1), _P(min_tokens_to_keep=2)]),
    ("nothing to fuse", lambda: [RepetitionPenaltyLogitsProcessor(1.1)]),
    ("empty", lambda: []),
])
def test_every_other_list_is_left_as_it_is(name, procs):
    lst = LogitsProcessorList(procs())
    before = list(lst)
    out = fuse_warpers(lst)
    assert out is lst and len(out) == len(before) and all(a is b for a, b in zip(out, before)), name


def test_beam_floor_and_repr():
    f = fuse_warpers([_K(5, min_tokens_to_keep=2), _P(min_tokens_to_keep=2)])[0]
    assert (f.top_k, f.min_tokens_to_keep) == (5, 2) and "top_p=0.9" in repr(f)
    for bad in (dict(temperature=0.0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(min_tokens_to_keep=0)):
        with pytest.raises(ValueError):
            FusedSamplingWarper(**bad)


def _tiny(switch=None):
    cfg = LM.u2Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                           num_key_value_heads=2, head_dim=16, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    if switch is not None:
        cfg.u2_fused_sampling = switch
    return LM.u2Qwen3ForCausalLM(cfg).eval()


def _processors(m, **kw):
    gc = GenerationConfig(do_sample=True, pad_token_id=0, bos_token_id=1, eos_token_id=2, **kw)
    m._prepare_special_tokens(gc, False, device=torch.device("cpu"))
    return m._get_logits_processor(generation_config=gc, input_ids_seq_length=3, encoder_input_ids=None,
                                   prefix_allowed_tokens_fn=None, logits_processor=LogitsProcessorList(), device="cpu")


@pytest.mark.parametrize("switch", [None, False])
def test_switch_off_returns_what_transformers_returns(switch):
    m = _tiny(switch)
    assert not getattr(m.config, "u2_fused_sampling", False)      # the default is off
    procs = _processors(m, top_p=0.9, temperature=0.7)
    assert [type(p) for p in procs] == [TemperatureLogitsWarper, TopPLogitsWarper]
    assert not any(isinstance(p, FusedSamplingWarper) for p in procs)


def test_switch_on_fuses_the_callers_sampling_arguments():
    m = _tiny(True)
    procs = _processors(m, top_p=0.9, temperature=0.7)
    assert len(procs) == 1 and type(procs[0]) is FusedSamplingWarper
    f = procs[0]
    assert (f.temperature, f.top_k, f.top_p, f.min_tokens_to_keep) == (0.7, 0, 0.9, 1)
    assert [type(p) for p in f.stock] == [TemperatureLogitsWarper, TopPLogitsWarper]
    # other processors of the list stay where they are
    procs = _processors(m, top_p=0.9, temperature=0.7, top_k=50, repetition_penalty=1.2)
    assert [type(p) for p in procs] == [RepetitionPenaltyLogitsProcessor, FusedSamplingWarper] and procs[1].top_k == 50
    # greedy / lone temperature: nothing to fuse
    assert [type(p) for p in _processors(m, temperature=0.7)] == [TemperatureLogitsWarper]


def test_beam_sampling_keeps_two():
    f = _processors(_tiny(True), top_p=0.9, temperature=0.7, num_beams=2)
    f = [p for p in f if isinstance(p, FusedSamplingWarper)]
    assert len(f) == 1 and f[0].min_tokens_to_keep == 2


def test_cpu_scores_take_the_stock_warpers():
    x = SC.logits(3, 65, seed=1)
    want, procs = SC.stock(x, 0.7, 5, 0.9)
    f = fuse_warpers(procs)[0]
    n = dict(sampling.stats)
    got = f(None, x)
    assert torch.equal(got, want)
    assert sampling.stats["stock"] == n["stock"] + 1 and sampling.stats["fused"] == n["fused"]
    got = f(None, x.bfloat16())                                  # (any dtype: the stock warpers decide)
    assert got.dtype == torch.bfloat16 and sampling.stats["stock"] == n["stock"] + 2


def test_generate_on_the_cpu_with_the_switch_on_samples_as_with_it_off():
    """fp32 model on the CPU: the fused warper falls back to the stock ones, so the sampled ids are those of the stock list."""
    m = _tiny(True)
    ids = torch.tensor([[5, 6, 7]])
    kw = dict(do_sample=True, top_p=0.9, temperature=0.7, max_new_tokens=4, pad_token_id=0)
    n = dict(sampling.stats)
    torch.manual_seed(3)
    a = m.generate(None, ids, **kw)
    assert sampling.stats["stock"] == n["stock"] + 4 and sampling.stats["fused"] == n["fused"]
    m.config.u2_fused_sampling = False
    torch.manual_seed(3)
    b = m.generate(None, ids, **kw)
    assert torch.equal(a, b) and sampling.stats["stock"] == n["stock"] + 4


# ------------------------------------------------------------------------------------------------ the reference against stock
HOST_PARAMS = [(0.7, 0, 0.9, 1), (1.0, 50, 0.9, 1), (0.2, 0, 0.7, 1), (1.3, 50, 0.95, 2), (1.0, 5, 1.0, 1)]


@pytest.mark.parametrize("V", [8, 65, 1000, 32064])
@pytest.mark.parametrize("rows", [1, 3, 16])
def test_reference_equals_the_stock_warpers_on_fp32_logits(rows, V):
    """Without ties the stable float64 reference and transformers' fp32 warpers keep the same tokens: bit-equal outputs."""
    for seed in (0, 1):
        x = SC.logits(rows, V, seed)
        for prm in HOST_PARAMS:
            ref, _ = SC.reference(x, *prm)
            want, _ = SC.stock(x, *prm)
            assert torch.equal(ref.view(torch.int32), want.view(torch.int32)), (rows, V, seed, prm)


def test_reference_equals_the_stock_warpers_at_the_qwen3_vocabulary():
    x = SC.logits(3, 151936, 0)
    for prm in HOST_PARAMS[:2]:
        assert torch.equal(SC.reference(x, *prm)[0], SC.stock(x, *prm)[0]), prm


@pytest.mark.parametrize("V", [65, 1000, 32064])
def test_reference_on_tied_logits_keeps_what_stock_keeps_up_to_the_members(V):
    """bf16-valued logits tie everywhere: which of the equal logits at the nucleus boundary stock keeps follows torch.sort's unstable
    order; the count per row and the kept values (sorted) are the same."""
    for seed in (0, 1):
        x = SC.logits(16, V, seed, bf16_values=True)
        for prm in HOST_PARAMS:
            ref, _ = SC.reference(x, *prm)
            want, _ = SC.stock(x, *prm)
            assert torch.equal((ref > -math.inf).sum(-1), (want > -math.inf).sum(-1)), (V, seed, prm)
            assert torch.equal(ref.sort(-1).values, want.sort(-1).values), (V, seed, prm)


def test_reference_tie_rule_keeps_the_highest_indices():
    x = torch.zeros(1, 10)
    out, cum = SC.reference(x, top_p=0.35)           # masses 0.1 each: ranks above < 0.35 -> 4 tokens, the highest indices
    assert (out[0] > -math.inf).nonzero().flatten().tolist() == [6, 7, 8, 9]
    assert int(SC.undecided(x, cum, 0.35).sum()) == 0


# ------------------------------------------------------------------------------------------------ argument guards (no launch)
@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


def test_sample_warp_rejects_bad_arguments(lib):
    ERR_ARG, ERR_WS = -1, -3
    P = 1 << 20       # an aligned address that is never dereferenced
    rows, V = 3, 1000
    need = lib.u2tok_sample_warp_workspace_bytes(rows, V)
    assert need > 0 and need % 256 == 0 and need <= rows * 256 * 16          # O(rows x bins)
    assert lib.u2tok_sample_warp_workspace_bytes(0, V) == 0 and lib.u2tok_sample_warp_workspace_bytes(rows, 1) == 0
    # logits, ld_in, out, ld_out, rows, V, temperature, top_k, top_p, min_keep, workspace, workspace_bytes, stream
    args = [P, V, P + (1 << 16), V, rows, V, 0.7, 50, 0.9, 1, P + (1 << 18), need, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.u2tok_sample_warp(*a)

    for i in (0, 2, 10):                                         # null pointers first
        assert call(**{f"a{i}": None}) == ERR_ARG, i
    assert call(a4=0) == ERR_ARG and call(a4=-1) == ERR_ARG      # rows < 1
    assert call(a5=1, a1=1, a3=1) == ERR_ARG                     # V < 2
    assert call(a6=0.0) == ERR_ARG and call(a6=-1.0) == ERR_ARG and call(a6=math.nan) == ERR_ARG
    assert call(a8=0.0) == ERR_ARG and call(a8=1.0001) == ERR_ARG and call(a8=-0.5) == ERR_ARG and call(a8=math.nan) == ERR_ARG
    assert call(a9=0) == ERR_ARG                                 # min_keep < 1
    assert call(a7=-1) == ERR_ARG                                # top_k < 0
    assert call(a1=V - 1) == ERR_ARG and call(a3=V - 1) == ERR_ARG
    assert call(a0=P + 2) == ERR_ARG                             # not 4-byte aligned
    assert call(a11=need - 1) == ERR_WS and call(a11=0) == ERR_WS
