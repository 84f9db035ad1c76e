"""GPU: the head of the decode step on the library (opt-in, `enable_fused_prefill(model, head=True)` / `config.u2_fused_decode_head`;
u2tok_decode_head, u2tok_decoder_decode_stack_head): the stack's final RMSNorm and lm_head -- in the element type, in e4m3 or in e2m1 --
with fp32 logits, in the library call of the whole-stack step.  The head adds no kernel, so its test is BIT EQUALITY with the two calls
it is defined as (`ops.rmsnorm`, then the `ops.gemm_rows*` of its form with fp32 C), an element-wise float64 bound on top, the step
with the head against the step followed by the head, the model's route against the entries, the calls that must keep today's path, and
the refusals, which must come before anything is launched.  Both element builds.

Shapes: 2 layers, E = 256, I = 512, 4 / 2 heads of 64, V = 512 (Phi-3: the packed layout, E = 384, 4 heads of 96, window 8)."""
import copy
import ctypes as C

import pytest
import torch

from helpers import decisive_decoder_
from u2tokenizer_amd import synth

pytestmark = pytest.mark.gpu
D = "cuda"
bf, f16 = torch.bfloat16, torch.float16
DTYPES, IDS = [bf, f16], ["bf16", "fp16"]
NL, S0, STEPS, WINDOW, VOCAB = 2, 11, 4, 8, 512
FORM_NAMES = ["elem", "fp8", "fp4"]
u = 2.0 ** -24
U_OF = {bf: 2.0 ** -8, f16: 2.0 ** -11}                 # unit roundoff of the element types
TINY_OF = {bf: 2.0 ** -126, f16: 2.0 ** -25}            # what a rounding errs by below the normal range
_BASE = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


def _gen(*key):
    return torch.Generator().manual_seed(hash(key) % (2 ** 31))


# ----------------------------------------------------------------------------------------------- 1. the head entry, bit for bit
def _head_operands(ops, dt, form, E, V):
    g = torch.Generator().manual_seed(1000 * form + E + V)
    w = (torch.randn(V, E, generator=g) / E ** 0.5).to(D)
    nw = (1.0 + 0.1 * torch.randn(E, generator=g)).to(dt).to(D)
    wt = (w.to(dt),) if form == 0 else ops.quantize_rows_fp8(w) if form == 1 else ops.quantize_blocks_fp4(w)
    return nw, wt


def _product(ops, form, xn, wt, **kw):
    return (ops.gemm_rows, ops.gemm_rows_w8, ops.gemm_rows_w4)[form](xn, *wt, out_f32=True, **kw)


def _rows(B, E, dt, seed=0):
    return (2.0 * torch.randn(B, E, generator=torch.Generator().manual_seed(7 * B + E + seed))).to(dt).to(D)


@pytest.mark.parametrize("form", [0, 1, 2], ids=FORM_NAMES)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_head_logits_are_the_norm_then_the_few_rows_product(ops, dt, form):
    """B in {1, 3, 16, 17, 64} x (E, V) in {(128, 16), (256, 1000), (128, 32064)}: the logits equal ops.rmsnorm followed by the
    product of the form with fp32 C, bit for bit, written into a row-strided buffer whose guard columns keep their canary.  A shape
    the product refuses is refused by the head too."""
    for E, V in ((128, 16), (256, 1000), (128, 32064)):
        nw, wt = _head_operands(ops, dt, form, E, V)
        for B in (1, 3, 16, 17, 64):
            x = _rows(B, E, dt)
            xn = ops.rmsnorm(x, nw, 1e-6)
            try:
                want = _product(ops, form, xn, wt)
            except RuntimeError:
                with pytest.raises(RuntimeError, match="u2tok_decode_head"):
                    ops.decode_head(x, nw, 1e-6, *wt)
                continue
            buf = torch.full((B, V + 24), 7.0, dtype=torch.float32, device=D)
            got = ops.decode_head(x, nw, 1e-6, *wt, out=buf[:, 8:8 + V])
            assert got.dtype == torch.float32 and torch.isfinite(got).all() and got.abs().max() > 0.1
            assert torch.equal(got, want), (E, V, B, int((got != want).sum()))
            assert (buf[:, :8] == 7).all() and (buf[:, 8 + V:] == 7).all()
            assert torch.equal(ops.decode_head(x, nw, 1e-6, *wt), want)
    # x rows of a wider buffer (ldx > E)
    wide = _rows(5, 256 + 64, dt)
    nw, wt = _head_operands(ops, dt, form, 256, 1000)
    assert torch.equal(ops.decode_head(wide[:, 32:32 + 256], nw, 1e-6, *wt),
                       _product(ops, form, ops.rmsnorm(wide[:, 32:32 + 256].contiguous(), nw, 1e-6), wt))


def _dequant(ops, form, wt):
    return wt[0].double() if form == 0 else (ops.dequantize_rows_fp8(*wt) if form == 1 else ops.dequantize_blocks_fp4(*wt)).double()


@pytest.mark.parametrize("form", [0, 1, 2], ids=FORM_NAMES)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_head_logits_within_a_derived_float64_bound(ops, dt, form):
    """Every logit against float64: ref[m][n] = sum_k Wd[n][k] xh[m][k] with Wd the dequantised weights (exact in float64) and
    xh = x r w, r = (mean_k x^2 + eps)^(-1/2), the float64 RMSNorm of the rounded inputs.  The bound, first order, one U per rounding
    to the element type (U = 2^-8 bf16, 2^-11 f16), u = 2^-24 per fp32 operation, no fitted factor:
      * the normed row.  The kernel (csrc/rows.h: rmsnorm_row, the rounding points of LlamaRMSNorm) computes r in fp32 -- a sum of E
        squares, a division, an addition, a reciprocal square root: relative error (E + 4) u --, the fp32 product x r (u), rounds it
        to the element type (U |x r|, or `tiny` below the normal range), multiplies by w -- exact in fp32: two 8- or 11-bit
        significands -- and rounds again (U |xh|).  The gate charges ONE element rounding of the normed row, the rounding of the
        value the product reads:
            e[k] = max(U |xh|, tiny) + (E + 5) u |xh|
        (The norm's first rounding, max(U |x r|, tiny) |w|, is as large again in the worst case; with it charged as well the bound
        is `loose` below, printed next to the gate's.  The gate holds with room to spare because K independent roundings do not
        align: the worst |error| / bound over these cases is 0.32 in bf16 and 0.30 in f16.)
      * the product.  e[k] goes through the sum with |Wd|:  sum_k |Wd[n][k]| e[k].  The products A W are exact in fp32 (as above;
        e4m3 and e2m1 values times a power-of-two block scale are exact in the element type), their K-term accumulation in fp32, in
        whatever order and split, errs by at most K u sum_k |Wd| |y| with |y| <= |xh| + e; the e4m3 form multiplies the sum by its
        fp32 row scale (one more u), and the fp32 store rounds nothing further:
            bound[m][n] = sum_k |Wd[n][k]| e[m][k] + (K + 1) u sum_k |Wd[n][k]| (|xh[m][k]| + e[m][k])
    Shapes: (B, E, V) = (3, 128, 1000), (17, 256, 1000), (64, 4096, 48): every row block form of the product, one, two and sixteen
    waves' worth of K.  The worst ratio is printed."""
    U, tiny = U_OF[dt], TINY_OF[dt]
    worst = 0.0
    for B, E, V in ((3, 128, 1000), (17, 256, 1000), (64, 4096, 48)):
        nw, wt = _head_operands(ops, dt, form, E, V)
        x = _rows(B, E, dt, seed=1)
        got = ops.decode_head(x, nw, 1e-6, *wt).double().cpu()
        Wd, xd, wd = _dequant(ops, form, wt).cpu(), x.double().cpu(), nw.double().cpu()
        r = (xd.pow(2).mean(1, keepdim=True) + 1e-6).rsqrt()
        xr = xd * r
        xh = xr * wd
        e = (U * xh.abs()).clamp_min(tiny) + (E + 5) * u * xh.abs()
        e2 = e + (U * xr.abs()).clamp_min(tiny) * wd.abs()
        ref = xh @ Wd.T
        bound = e @ Wd.abs().T + (E + 1) * u * ((xh.abs() + e) @ Wd.abs().T)
        loose = e2 @ Wd.abs().T + (E + 1) * u * ((xh.abs() + e2) @ Wd.abs().T)
        assert torch.isfinite(got).all() and (bound > 0).all()
        ratio = ((got - ref).abs() / bound).max().item()
        print(f"decode_head {dt} form {form} B {B} E {E} V {V}: worst |error| / bound = {ratio:.3f} "
              f"(both roundings charged: {((got - ref).abs() / loose).max().item():.3f}), "
              f"bound / rms(logit) = {(bound.max() / ref.pow(2).mean().sqrt()).item():.2e}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (B, E, V, ratio)
    assert worst > 0.0


# ------------------------------------------------------------------------------- 2. the step with the head = the step, then the head
def _build(kind, vocab=VOCAB, tie=False):
    from transformers import (LlamaConfig, LlamaForCausalLM, Phi3Config, Phi3ForCausalLM, Qwen3Config, Qwen3ForCausalLM)
    common = dict(vocab_size=vocab, intermediate_size=512, num_hidden_layers=NL, max_position_embeddings=256, tie_word_embeddings=tie,
                  pad_token_id=0, bos_token_id=1, eos_token_id=2)
    if kind == "phi3":
        m = Phi3ForCausalLM(Phi3Config(hidden_size=384, num_attention_heads=4, num_key_value_heads=4, sliding_window=WINDOW, **common))
    else:
        common.update(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64)
        m = Qwen3ForCausalLM(Qwen3Config(**common)) if kind == "qwen3" else LlamaForCausalLM(LlamaConfig(**common, rope_theta=500000.0))
    synth.fill_module_(m, seed=23, prefix="decoder.")
    return m.eval()


def _model(kind, dt, **kw):
    key = (kind, tuple(sorted(kw.items())))
    if key not in _BASE:
        _BASE[key] = _build(kind, **kw)
    return copy.deepcopy(_BASE[key]).to(dt).to(D)


def _inputs(m, B, dt):
    E = m.config.hidden_size
    x = (0.5 * synth.synth_tensor("inputs_embeds", (B, S0, E), 5)).to(dt).to(D)
    xs = (0.5 * synth.synth_tensor("inputs_embeds", (B, STEPS, E), 6)).to(dt).to(D)
    return x, xs


def _prefilled(m, x):
    from transformers.cache_utils import DynamicCache
    cache = DynamicCache()
    m.model(inputs_embeds=x, past_key_values=cache, use_cache=True)
    return cache


def _raw_copy(m):
    """a copy of m whose stack hands out the last hidden state UN-NORMED: the stack route calls `norm` as the module it is"""
    r = copy.deepcopy(m)
    r.model.norm = torch.nn.Identity()
    return r


def _head_step(m, x1, cache, form=0):
    """one step through the route's own pieces, as `prefill.head_forward` strings them -> (hidden rows un-normed, logits)"""
    from u2tokenizer_amd import prefill
    plan = []
    kw = dict(past_key_values=cache, use_cache=True, output_hidden_states=False, output_attentions=False)
    prefill._mask_hook(m.model, (), {"attention_mask": None})
    assert prefill.head_route(m, x1.shape[0], 1, x1.dtype, True, kw, False, None, plan) == "head"
    return prefill._stack_step(m.model, plan, None, x1, cache, None, head=prefill._head_state(m, form))


@pytest.mark.parametrize("B", [1, 16])
@pytest.mark.parametrize("form", [0, 2], ids=["elem", "fp4"])
@pytest.mark.parametrize("kind", ["qwen3", "llama", "phi3"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_stack_with_head_equals_the_stack_then_the_head(ops, dt, kind, form, B):
    """Two copies of one model, the same fused prefill, 4 steps.  Copy a: u2tok_decoder_decode_stack_head.  Copy b: the whole-stack
    step (its stack's norm replaced by the identity, so the un-normed rows come out), then `ops.decode_head` on them.  Every step: the
    same hidden rows, the same logits, the same keys and values in every layer, bit for bit.  The steps of Phi-3 cross its window."""
    from u2tokenizer_amd import prefill
    ma = _model(kind, dt)
    mb = _raw_copy(ma)
    x, xs = _inputs(ma, B, dt)
    sw = dict(continued=True) if kind == "phi3" else {}
    prefill.enable_fused_prefill(ma, head=True, **sw)
    prefill.enable_fused_prefill(mb, stack_decode=True, **sw)
    ca, cb = _prefilled(ma, x), _prefilled(mb, x)
    nw, eps, w = ma.model.norm.weight, ma.model.norm.variance_epsilon, ma.lm_head.weight
    wt = (w,) if form == 0 else ops.quantize_blocks_fp4(w)
    n0 = dict(prefill.stack_stats)
    for t in range(STEPS):
        hid, logits = _head_step(ma, xs[:, t:t + 1], ca, form)
        raw = mb.model(inputs_embeds=xs[:, t:t + 1], past_key_values=cb, use_cache=True).last_hidden_state
        want = ops.decode_head(raw[:, 0], nw, eps, *wt)
        assert logits.shape == (B, 1, VOCAB) and logits.dtype == torch.float32 and torch.isfinite(logits).all()
        assert torch.equal(hid, raw), (t, "hidden rows")
        assert torch.equal(logits[:, 0], want), (t, "logits", int((logits[:, 0] != want).sum()))
        for i, (la, lb) in enumerate(zip(ca.layers, cb.layers)):
            assert la.keys.shape[2] == S0 + t + 1 and torch.equal(la.keys, lb.keys) and torch.equal(la.values, lb.values), (t, i)
    assert prefill.stack_stats["decode"] - n0["decode"] == 2 * STEPS
    prefill.disable_fused_prefill(ma)
    prefill.disable_fused_prefill(mb)


# ------------------------------------------------------------------------------------------------------------- 3. the model's route
def _u2(dt, head=True, decisive=False, tie=False, hidden=256, **cfg):
    """a u2Qwen3ForCausalLM of the shapes above whose config asks for the whole-stack step, with or without the head"""
    from u2tokenizer_amd import language_model as LM
    key = ("u2", decisive, tie, hidden)
    if key not in _BASE:
        c = LM.u2Qwen3Config(vocab_size=VOCAB, hidden_size=hidden, intermediate_size=512, num_hidden_layers=NL, num_attention_heads=4,
                             num_key_value_heads=2, head_dim=64, max_position_embeddings=256, tie_word_embeddings=tie,
                             pad_token_id=0, bos_token_id=1, eos_token_id=2)
        m = LM.u2Qwen3ForCausalLM(c)
        synth.fill_module_(m, seed=23, prefix="decoder.")
        _BASE[key] = decisive_decoder_(m.eval(), 0) if decisive else m.eval()
    m = copy.deepcopy(_BASE[key]).to(dt).to(D)
    m.config.u2_fused_stack_decode = True
    m.config.u2_fused_decode_head = head
    for k, v in cfg.items():
        setattr(m.config, k, v)
    return m


def _lm_prefilled(m, x):
    from transformers.cache_utils import DynamicCache
    cache = DynamicCache()
    m(inputs_embeds=x, past_key_values=cache, use_cache=True)
    return cache


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_model_logits_are_the_head_entry_on_the_stack_routes_hidden_state(ops, dt, form):
    """`model(...).logits` on the head route, (B, 1, V) fp32, equals the head entry applied to the un-normed hidden state of the same
    step from the stack route with the head off; "fp8" / "fp4": equal to ops.gemm_rows_w8 / _w4 on the quantiser's output, on
    `ops.rmsnorm` of that hidden state.  The counters say which route ran and in which form."""
    from u2tokenizer_amd import prefill
    B = 3
    ma = _u2(dt, head=True, u2_fused_head_form=form)
    mb = _raw_copy(_u2(dt, head=False))
    x, xs = _inputs(ma, B, dt)
    ca, cb = _lm_prefilled(ma, x), _lm_prefilled(mb, x)
    assert ma.model._u2_stack.head and ma.model._u2_stack.stack and not mb.model._u2_stack.head
    nw, eps, w = ma.model.norm.weight, ma.model.norm.variance_epsilon, ma.lm_head.weight
    n0, s0 = dict(prefill.head_stats), dict(prefill.stack_stats)
    for t in range(STEPS):
        out = ma(inputs_embeds=xs[:, t:t + 1], past_key_values=ca, use_cache=True)
        raw = mb.model(inputs_embeds=xs[:, t:t + 1], past_key_values=cb, use_cache=True).last_hidden_state[:, 0]
        assert out.logits.shape == (B, 1, VOCAB) and out.logits.dtype == torch.float32 and out.past_key_values is ca
        xn = ops.rmsnorm(raw, nw, eps)
        if form == "elem":
            assert torch.equal(out.logits[:, 0], ops.decode_head(raw, nw, eps, w))
            want = ops.gemm_rows(xn, w, out_f32=True)
        elif form == "fp8":
            want = ops.gemm_rows_w8(xn, *ops.quantize_rows_fp8(w), out_f32=True)
        else:
            want = ops.gemm_rows_w4(xn, *ops.quantize_blocks_fp4(w), out_f32=True)
        assert torch.equal(out.logits[:, 0], want), (t, form)
    assert prefill.head_stats == {**n0, "head": n0["head"] + STEPS}
    assert prefill.stack_stats["decode"] - s0["decode"] == 2 * STEPS
    assert (prefill.head_weights(ma) is None) == (form == "elem")
    prefill.disable_fused_prefill(ma)
    assert prefill.head_weights(ma) is None


def test_a_changed_lm_head_weight_is_picked_up(ops):
    """The e4m3 copy is kept from step to step, rebuilt after an in-place change of lm_head.weight, and the logits are then the
    product on the new weight's quantisation."""
    from u2tokenizer_amd import prefill
    m = _u2(bf, head=True, u2_fused_head_form="fp8")
    x, xs = _inputs(m, 2, bf)
    cache = _lm_prefilled(m, x)
    a = m(inputs_embeds=xs[:, :1], past_key_values=cache, use_cache=True).logits.clone()
    kept = prefill.head_weights(m)
    b = m(inputs_embeds=xs[:, 1:2], past_key_values=cache, use_cache=True).logits
    assert prefill.head_weights(m) is kept                         # (nothing changed: nothing rebuilt)
    m.lm_head.weight.data[7].mul_(3.0)                             # (.data: no version bump, but ...)
    m.lm_head.weight.mul_(1.0)                                     # ... an in-place op on the parameter bumps it
    mb = _raw_copy(_u2(bf, head=False))
    cb = _lm_prefilled(mb, x)
    for t in range(3):
        raw = mb.model(inputs_embeds=xs[:, t:t + 1], past_key_values=cb, use_cache=True).last_hidden_state[:, 0]
    c = m(inputs_embeds=xs[:, 2:3], past_key_values=cache, use_cache=True).logits
    assert prefill.head_weights(m) is not kept
    w8, sc = prefill.head_weights(m)
    wq, sq = ops.quantize_rows_fp8(m.lm_head.weight)
    assert torch.equal(w8.view(torch.uint8), wq.view(torch.uint8)) and torch.equal(sc, sq)
    assert a.shape == b.shape == c.shape and torch.isfinite(c).all()
    xn = ops.rmsnorm(raw, m.model.norm.weight, m.model.norm.variance_epsilon)
    assert torch.equal(c[:, 0], ops.gemm_rows_w8(xn, wq, sq, out_f32=True))
    prefill.disable_fused_prefill(m)
    prefill.disable_fused_prefill(mb)


def test_a_shape_the_form_does_not_take_runs_on_the_element_type_and_is_counted(ops):
    """E = 192: no multiple of 128, so "fp4" falls back -- the logits of "elem", bit for bit, one form_fallback per call, no copy
    kept --, while "fp8" (192 = 3 x 64) runs in its form."""
    from u2tokenizer_amd import prefill
    ma, mb, mc = (_u2(bf, head=True, hidden=192, u2_fused_head_form=f) for f in ("fp4", "elem", "fp8"))
    x, xs = _inputs(ma, 2, bf)
    ca, cb, cc = _lm_prefilled(ma, x), _lm_prefilled(mb, x), _lm_prefilled(mc, x)
    n0 = dict(prefill.head_stats)
    a = ma(inputs_embeds=xs[:, :1], past_key_values=ca, use_cache=True).logits
    assert prefill.head_stats == {**n0, "head": n0["head"] + 1, "form_fallback": n0["form_fallback"] + 1}
    b = mb(inputs_embeds=xs[:, :1], past_key_values=cb, use_cache=True).logits
    c = mc(inputs_embeds=xs[:, :1], past_key_values=cc, use_cache=True).logits
    assert prefill.head_stats == {**n0, "head": n0["head"] + 3, "form_fallback": n0["form_fallback"] + 1}
    assert torch.equal(a, b) and prefill.head_weights(ma) is None and not torch.equal(a, c)
    assert prefill.head_weights(mc)[0].dtype == torch.float8_e4m3fn
    for m in (ma, mb, mc):
        prefill.disable_fused_prefill(m)


def test_tied_embeddings_keep_reading_the_16_bit_table(ops):
    from u2tokenizer_amd import prefill
    m = _u2(bf, head=True, tie=True, u2_fused_head_form="fp4")
    assert m.lm_head.weight is m.model.embed_tokens.weight
    ids = torch.randint(3, VOCAB, (2, 9), generator=torch.Generator().manual_seed(5)).to(D)
    table = m.model.embed_tokens.weight.clone()
    e0 = m.model.embed_tokens(ids).clone()
    cache = _lm_prefilled(m, e0)
    n0 = prefill.head_stats["head"]
    out = m(input_ids=ids[:, :1], past_key_values=cache, use_cache=True)
    assert prefill.head_stats["head"] == n0 + 1 and prefill.head_weights(m) is not None
    assert prefill.head_weights(m)[0].dtype == torch.uint8 and torch.isfinite(out.logits).all()
    assert torch.equal(m.model.embed_tokens.weight, table) and torch.equal(m.model.embed_tokens(ids), e0)
    assert m.lm_head.weight is m.model.embed_tokens.weight and m.lm_head.weight.dtype == bf
    prefill.disable_fused_prefill(m)


# The prompt seed of the generate test, chosen on the CPU with the fp32 model alone: among seeds 1 .. 79 one at which all 4 decode
# steps of both sequences have a top-2 margin above 0.16 max |logit| (0.169 .. 0.655; max |logit| 7.2) and the ids move (37 269 269
# 269 269 | 172 373 137 172 373).
SEED = 71


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_greedy_generate_gives_the_ids_of_the_head_off(ops, dt):
    """Greedy `generate`, 5 new tokens (the first is the prefill's, 4 decode steps) for 2 prompts, helpers.decisive_decoder_: the ids
    with the head on equal the ids with it off at every step whose decision is clear in the head-off run.  Clear: the head-off run's
    own top-2 margin exceeds 4 U max |logit| of that step -- its two logits were rounded to 16 bits (U |logit| each), and as much
    again for the other orders of the norm's and the product's fp32 sums; the hidden states of the two runs are bit-equal while the
    ids agree.  At least 3 of the 4 steps of each sequence are compared; 4 head steps counted."""
    from u2tokenizer_amd import prefill
    new = 5
    ids = torch.randint(3, VOCAB, (2, 9), generator=torch.Generator().manual_seed(SEED)).to(D)
    kw = dict(max_new_tokens=new, min_new_tokens=new, do_sample=False, pad_token_id=0)
    off = _u2(dt, head=False, decisive=True)
    g_off = off.generate(inputs=ids, output_scores=True, return_dict_in_generate=True, **kw)
    on = _u2(dt, head=True, decisive=True)
    n0 = dict(prefill.head_stats)
    g_on = on.generate(inputs=ids, **kw)
    assert prefill.head_stats["head"] - n0["head"] == new - 1 and g_on.shape == g_off.sequences.shape == (2, new)
    for b in range(2):
        compared = 0
        for t in range(1, new):
            s = g_off.scores[t][b].float()
            s = s[torch.isfinite(s)]
            top = s.topk(2).values
            if float(top[0] - top[1]) > 4 * U_OF[dt] * float(s.abs().max()):
                assert g_on[b, t] == g_off.sequences[b, t], (b, t, g_on[b].tolist(), g_off.sequences[b].tolist())
                compared += 1
            elif g_on[b, t] != g_off.sequences[b, t]:
                break
        assert compared >= 3, (b, compared)
    prefill.disable_fused_prefill(on)
    prefill.disable_fused_prefill(off)


# ------------------------------------------------------------------------------------------------------------- 4. the fall-throughs
class _Adapter(torch.nn.Module):
    """lm_head behind an unmerged rank-4 adapter: another module type with a base layer (what an adapter library leaves there)"""

    def __init__(self, base_layer):
        super().__init__()
        self.base_layer = base_layer
        g = torch.Generator().manual_seed(11)
        dt, dev = base_layer.weight.dtype, base_layer.weight.device
        self.A = torch.nn.Parameter((0.1 * torch.randn(4, base_layer.in_features, generator=g)).to(dt).to(dev))
        self.B = torch.nn.Parameter((0.1 * torch.randn(base_layer.out_features, 4, generator=g)).to(dt).to(dev))

    @property
    def weight(self):
        return self.base_layer.weight

    def forward(self, x):
        return self.base_layer(x) + (x @ self.A.T) @ self.B.T


FALLS = ["lm_head with bias", "a hook on lm_head", "an adapter-wrapped lm_head", "a hook on norm", "labels", "output_hidden_states",
         "two positions", "the switch off"]


@pytest.mark.parametrize("why", FALLS)
def test_calls_that_keep_todays_path(ops, why):
    """Each of these runs the stack route, then the module norm and lm_head: the outputs of a model that never had the switch, bit for
    bit, no head step counted and -- while the switch is on -- one fallback per call."""
    from u2tokenizer_amd import prefill
    B = 2
    ma, mb = _u2(bf, head=True), _u2(bf, head=False)
    x, xs = _inputs(ma, B, bf)
    kw, S = {}, 1
    for m in (ma, mb):
        if why == "lm_head with bias":
            m.lm_head.bias = torch.nn.Parameter(synth.synth_tensor("lm_head.bias", (VOCAB,), 3).to(bf).to(D))
        elif why == "a hook on lm_head":
            m.lm_head.register_forward_hook(lambda mod, a, out: out * 2)
        elif why == "an adapter-wrapped lm_head":
            m.lm_head = _Adapter(m.lm_head)
        elif why == "a hook on norm":
            m.model.norm.register_forward_hook(lambda mod, a, out: out * 2)
    if why == "labels":
        kw = dict(labels=torch.randint(3, VOCAB, (B, 1), generator=torch.Generator().manual_seed(2)).to(D))
    elif why == "output_hidden_states":
        kw = dict(output_hidden_states=True)
    elif why == "two positions":
        S = 2
    ca, cb = _lm_prefilled(ma, x), _lm_prefilled(mb, x)
    if why == "the switch off":
        prefill.enable_fused_prefill(ma, stack_decode=True)
        assert not ma.model._u2_stack.head
    n0 = dict(prefill.head_stats)
    for t in range(0, STEPS, S):
        a = ma(inputs_embeds=xs[:, t:t + S], past_key_values=ca, use_cache=True, **kw)
        b = mb(inputs_embeds=xs[:, t:t + S], past_key_values=cb, use_cache=True, **kw)
        assert a.logits.dtype == b.logits.dtype and torch.equal(a.logits, b.logits), (why, t)
        # (bits: the loss of a single position, whose shifted labels are empty, is NaN on both sides)
        assert (a.loss is None) == (b.loss is None) and (a.loss is None or torch.equal(a.loss.view(torch.int32), b.loss.view(torch.int32)))
        if why == "output_hidden_states":
            assert all(torch.equal(p, q) for p, q in zip(a.hidden_states, b.hidden_states))
    calls = STEPS // S
    assert prefill.head_stats == {**n0, "fallback": n0["fallback"] + (0 if why == "the switch off" else calls)}, why
    prefill.disable_fused_prefill(ma)
    prefill.disable_fused_prefill(mb)


# ------------------------------------------------------------------------------------------------------------------ 5. the refusals
def test_every_refusal_of_layers_and_head_comes_before_the_first_launch(ops):
    """u2tok_decoder_decode_stack_head called directly on the descriptors of a step the route has taken: V = 1, a misaligned W, a
    head of e2m1 codes without scales, a null W / norm weight / logits / head, a short workspace (for the head's part, for the
    stack's), a bad last layer.  Each returns its error code, and the row of layer 0's cache buffers the step would write, the
    workspace, `out` and the logits keep their sentinels.  The standalone head likewise (E % 128 != 0 with form 2 among its cases).
    Then the descriptors were good: the call runs and equals the stack call followed by the head call."""
    from u2tokenizer_amd import _lib, prefill
    m = _model("qwen3", bf)
    B = 2
    x, xs = _inputs(m, B, bf)
    prefill.enable_fused_prefill(m, head=True)
    cache = _prefilled(m, x)
    _head_step(m, xs[:, :1], cache)                                              # (builds the descriptors)
    E = m.config.hidden_size
    arr = (_lib.DecodeStackLayer * NL)()
    keep = []
    for i, layer in enumerate(m.model.layers):
        lay, _, _, cfg = layer._u2_prefill.variants[(0, False)]
        cl = cache.layers[i]
        T0 = cl._room(1, cl.keys)
        s = arr[i]
        s.cfg, s.layer, s.k_cache, s.v_cache = C.addressof(cfg), C.addressof(lay), cl._kb.data_ptr(), cl._vb.data_ptr()
        s.kv_stride, s.s_off, s.k_first, s.T = cl._kb.stride(1), T0, 0, T0 + 1
        keep.append((lay, cfg))
    l0 = cache.layers[0]
    T0 = arr[0].s_off
    l0._kb[:, :, T0].fill_(7.0), l0._vb[:, :, T0].fill_(7.0)
    x2 = xs[:, 1].contiguous()
    cos, sin = m.model.rotary_emb(x2[:, None], torch.full((1, 1), T0, device=D))
    cos, sin = cos.expand(B, 1, 64).reshape(B, 64).float().contiguous(), sin.expand(B, 1, 64).reshape(B, 64).float().contiguous()
    out = torch.full((B, E), 7.0, dtype=bf, device=D)
    logits = torch.full((B, VOCAB + 8), 7.0, dtype=torch.float32, device=D)
    nw, w = m.model.norm.weight, m.lm_head.weight
    wbuf = torch.zeros(VOCAB * E + 8, dtype=bf, device=D)                         # (a misaligned copy of W: 8 bytes in)
    w_off = wbuf[4:4 + VOCAB * E].view(VOCAB, E)
    w_off.copy_(w)

    def desc(**kw):
        d = dict(w_norm=nw.data_ptr(), W=w.data_ptr(), scale=None, E=E, V=VOCAB, wform=0, eps=1e-6, ldw=0, lds=0)
        d.update(kw)
        return _lib.DecodeHead(**d)

    good = desc()
    with ops.on_device(x2) as (h, stream):
        sneed = h.u2tok_decoder_decode_stack_workspace_bytes(arr, NL)
        need = h.u2tok_decoder_decode_stack_head_workspace_bytes(arr, NL, C.byref(good))
        assert sneed > 0 and need == sneed + h.u2tok_decode_head_workspace_bytes(B, E)
        ws = torch.zeros(need, dtype=torch.uint8, device=D)
        ws[256:].fill_(0x55)

        def call(d=good, layers=arr, n=NL, nbytes=need, lg=logits, o=out):
            return h.u2tok_decoder_decode_stack_head(layers, n, x2.data_ptr(), cos.data_ptr(), sin.data_ptr(), 1, 64, 0, None, 0,
                                                     o.data_ptr() if o is not None else None, C.byref(d) if d is not None else None,
                                                     lg.data_ptr() if lg is not None else None, VOCAB + 8, ws.data_ptr(), nbytes, stream)

        def untouched():
            torch.cuda.synchronize()
            return bool((l0._kb[:, :, T0] == 7).all() and (l0._vb[:, :, T0] == 7).all() and (out == 7).all() and (logits == 7).all()
                        and (ws[256:] == 0x55).all() and not ws[:256].any())

        assert call(desc(V=1)) == -1 and untouched()
        assert w_off.data_ptr() % 16 == 8 and call(desc(W=w_off.data_ptr())) == -1 and untouched()
        assert call(desc(wform=2)) == -1 and call(desc(wform=1)) == -1 and call(desc(wform=5)) == -1 and untouched()
        assert call(desc(W=None)) == -1 and call(desc(w_norm=None)) == -1 and call(lg=None) == -1 and call(None) == -1 and untouched()
        assert call(o=None) == -1 and call(desc(E=2 * E)) == -1 and untouched()
        assert call(nbytes=need - 1) == -3 and call(nbytes=sneed) == -3 and call(nbytes=sneed - 1) == -3 and untouched()
        bad = _lib.DecodeLayer.from_buffer_copy(keep[NL - 1][0])
        bad.Wdown = None
        was = arr[NL - 1].layer
        arr[NL - 1].layer = C.addressof(bad)
        assert call() == -1 and untouched()
        arr[NL - 1].layer = was
        assert call(n=0) == -1 and call(layers=None) == -1 and untouched()
        # the standalone head: sentinels in its workspace and logits
        hws = torch.full((h.u2tok_decode_head_workspace_bytes(B, E),), 0x55, dtype=torch.uint8, device=D)
        x192 = torch.zeros(B, 192, dtype=bf, device=D)

        def head(d, xin=x2, ldx=E, nbytes=hws.numel()):
            return h.u2tok_decode_head(C.byref(d), xin.data_ptr(), ldx, B, logits.data_ptr(), VOCAB + 8, hws.data_ptr(), nbytes, stream)

        codes = torch.zeros(VOCAB * 96, dtype=torch.uint8, device=D)
        assert head(desc(E=192, wform=2, W=codes.data_ptr(), scale=codes.data_ptr()), x192, 192) == -1     # E % 128 != 0 with form 2
        assert head(desc(V=1)) == -1 and head(desc(W=w_off.data_ptr())) == -1 and head(desc(W=None)) == -1
        assert head(good, nbytes=hws.numel() - 1) == -3
        torch.cuda.synchronize()
        assert (hws == 0x55).all() and untouched()
        # ... and the descriptors were good
        assert call() == 0
        torch.cuda.synchronize()
        assert not (l0._kb[:, :, T0] == 7).all() and not (out == 7).any() and (logits[:, VOCAB:] == 7).all() and not ws[:4].any()
    assert torch.equal(logits[:, :VOCAB], ops.decode_head(out, nw, 1e-6, w))
    prefill.disable_fused_prefill(m)
