"""GPU: padded batches on the fused prefill and decode steps (opt-in, `enable_fused_prefill(model, padded=True)`): the prefill
attention with a key range per sequence (u2tok_attention_gqa_range) and the batched decode attention (csrc/decode_attn.hip,
u2tok_decode_attention) against fp32 softmaxes on the host, on the bf16 and the f16 build; whole small decoders (the shapes and
the gate of tests/test_gpu_prefill.py, copied here) with left- and right-padded batches against the fp32 model with the stock
bf16 GPU run as the yardstick; `generate` on a left-padded batch against every prompt generated alone; the switch off."""
import math

import pytest
import torch
import torch.nn.functional as F

from u2tokenizer_amd import synth

from helpers import decisive_decoder_

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"
EPS = 1e-3
ELEMS = [pytest.param((torch.bfloat16, 2.0 ** -8), id="bf16"), pytest.param((torch.float16, 2.0 ** -11), id="f16")]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


def rnd(*shape, scale=1.0, seed=0, dtype=bf):
    g = torch.Generator().manual_seed(seed * 7919 + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def close(got, ref, ulp, rounds=2):
    got, ref = got.float().cpu(), ref.float()
    assert torch.isfinite(got).all()
    tol = rounds * ulp * ref.abs() + ulp * ref.abs().max()
    bad = (got - ref).abs() > tol
    assert not bad.any(), f"{bad.sum().item()} elements off; worst {(got - ref).abs().max().item():.3e}"


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=D)


# ------------------------------------------------------------------------------------------------- 1. range prefill kernel
RANGE_CASES = [(3, 70, 4, 2, 64, (0, 5, 66), None),
               (2, 200, 8, 2, 128, (64, 130), (200, 170)),
               (1, 130, 3, 3, 96, (129,), None)]


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("nb,S,Hq,Hkv,d,start,length", RANGE_CASES)
def test_attention_gqa_range_against_masked_softmax(ops, elem, nb, S, Hq, Hkv, d, start, length):
    """Causal GQA with kv_start[b] <= j < kv_len[b]: starts at zero, inside the first 64-key tile, on a tile edge, past a whole
    tile plus part of the next, a single visible key.  Rows that see a key against fp32; rows that see none are exact zeros."""
    dt, ulp = elem
    buf = rnd(nb, S, (Hq + 2 * Hkv) * d, seed=S + d, dtype=dt)
    q, k, v = buf[..., :Hq * d], buf[..., Hq * d:(Hq + Hkv) * d], buf[..., (Hq + Hkv) * d:]
    dbuf = buf.to(D)
    dq, dk, dv = dbuf[..., :Hq * d], dbuf[..., Hq * d:(Hq + Hkv) * d], dbuf[..., (Hq + Hkv) * d:]
    scale = 1.5 / math.sqrt(d)
    got = ops.attention_gqa_range(dq, dk, dv, Hq, Hkv, scale, kv_start=_i32(start), kv_len=_i32(length), causal=True)
    assert torch.isfinite(got).all()
    qh = q.float().view(nb, S, Hq, d).transpose(1, 2)
    kh = k.float().view(nb, S, Hkv, d).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    vh = v.float().view(nb, S, Hkv, d).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    ks = torch.tensor(start)[:, None, None]
    kl = torch.tensor(length if length is not None else (S,) * nb)[:, None, None]
    vis = (j <= i)[None] & (j[None] >= ks) & (j[None] < kl)                      # (nb, S, S)
    s = (qh @ kh.transpose(-1, -2) * scale).masked_fill(~vis[:, None], float("-inf"))
    sees = vis.any(-1)                                                           # (nb, S)
    p = torch.where(sees[:, None, :, None], F.softmax(s, -1), torch.zeros(()))
    ref = (p @ vh).transpose(1, 2).reshape(nb, S, Hq * d)
    assert sees.any() and (~sees).any()
    close(got[sees.to(D)], ref[sees], ulp)
    assert (got[(~sees).to(D)] == 0).all()                                       # exact zeros, not small numbers


@pytest.mark.parametrize("elem", ELEMS)
def test_attention_gqa_range_without_a_range_is_attention_gqa(ops, elem):
    dt, _ = elem
    buf = rnd(2, 77, (8 + 2 * 4) * 64, seed=5, dtype=dt).to(D)
    q, k, v = buf[..., :512], buf[..., 512:768], buf[..., 768:]
    assert torch.equal(ops.attention_gqa_range(q, k, v, 8, 4, 0.125), ops.attention_gqa(q, k, v, 8, 4, 0.125, causal=True))


# ------------------------------------------------------------------------------------------------- 2. batched decode kernel
def _starts(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(int(t) for t in torch.randint(0, T, (B,), generator=g))


# (B, T, g, d, kv heads, starts, K / V as views of larger buffers)
DECODE_CASES = [(2, 5, 1, 128, 2, (0, 4), False),                                          # one tile, no split
                (3, 70, 2, 64, 2, (0, 5, 69), False),
                (8, 1100, 4, 128, 2, (0, 63, 64, 600, 1099, 1, 32, 1000), False),          # whole splits are empty
                (16, 1792, 4, 128, 2, _starts(16, 1792, 3), True),
                (2, 300, 8, 96, 1, (0, 131), True)]


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("B,T,g,d,Hkv,start,strided", DECODE_CASES)
def test_decode_attention_against_softmax(ops, elem, B, T, g, d, Hkv, start, strided):
    """One query row per sequence over keys [kv_start, T), all sequences and heads in one launch: against fp32, twice with equal
    bits; without kv_start also against the per-entry split kernel the unpadded decode step uses."""
    dt, ulp = elem
    Hq = g * Hkv
    q = rnd(B, Hq * d, seed=21, dtype=dt)
    cap = T + 37 if strided else T
    kb, vb = rnd(B, Hkv, cap, d, seed=22, dtype=dt), rnd(B, Hkv, cap, d, seed=23, dtype=dt)
    dkb, dvb = kb.to(D), vb.to(D)
    dK, dV = dkb[:, :, :T], dvb[:, :, :T]
    assert dK.is_contiguous() != strided or B * Hkv == 1
    scale = d ** -0.5
    sc = (q.float().view(B, Hkv, g, d) @ kb[:, :, :T].float().transpose(2, 3)) * scale          # (B, Hkv, g, T)
    vf = vb[:, :, :T].float()
    for st in (start, None):
        outs = [ops.decode_attention(q.to(D), dK, dV, Hq, Hkv, scale, kv_start=_i32(st)) for _ in range(2)]
        assert torch.equal(outs[0], outs[1])
        s = sc if st is None else sc.masked_fill(torch.arange(T)[None, None, None] < torch.tensor(st)[:, None, None, None],
                                                 float("-inf"))
        ref = (torch.softmax(s, -1) @ vf).reshape(B, Hq * d)
        close(outs[0], ref, ulp, rounds=3)
    per_entry = ops.attention_gqa(q.to(D).view(B * Hkv, 1, g * d), dK.contiguous().view(B * Hkv, T, d),
                                  dV.contiguous().view(B * Hkv, T, d), g, 1, scale, causal=False, split_keys=True)
    close(outs[0], per_entry.float().cpu().view(B, Hq * d), ulp, rounds=3)


def test_decode_attention_without_a_visible_key_is_zero(ops):
    q, k, v = rnd(2, 4 * 64, seed=1).to(D), rnd(2, 2, 40, 64, seed=2).to(D), rnd(2, 2, 40, 64, seed=3).to(D)
    out = ops.decode_attention(q, k, v, 4, 2, 0.125, kv_start=_i32((3, 40)))
    assert torch.isfinite(out).all() and (out[1] == 0).all() and (out[0] != 0).any()


# ------------------------------------------------------------------------------------------------- 3 - 8. whole decoders
def _small(kind, layers=3, wide=False):
    from transformers import LlamaConfig, LlamaForCausalLM, Qwen3Config, Qwen3ForCausalLM
    common = dict(vocab_size=1024, hidden_size=512, intermediate_size=1536, num_hidden_layers=layers, num_attention_heads=8,
                  num_key_value_heads=4, head_dim=64, max_position_embeddings=512, tie_word_embeddings=False,
                  pad_token_id=0, bos_token_id=1, eos_token_id=2)
    if wide:  # one layer at the Qwen3-8B width (E = 4096, I = 12288, 32 / 8 heads of 128)
        common.update(hidden_size=4096, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8, head_dim=128)
    if kind == "qwen3":
        m = Qwen3ForCausalLM(Qwen3Config(**common))
    else:
        m = LlamaForCausalLM(LlamaConfig(**common, rope_theta=500000.0))
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m.eval()


def _err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _mask(S, pads=None, lengths=None):
    n = len(pads if pads is not None else lengths)
    m = torch.ones(n, S, dtype=torch.int64)
    for b in range(n):
        if pads is not None:
            m[b, :pads[b]] = 0
        else:
            m[b, lengths[b]:] = 0
    return m


def _gate(fused, stock, ref, sel, what):
    """The project's gate at the selected (unpadded) positions: no further from the fp32 model than 1.5 x the stock bf16 run."""
    es, ef = _err(stock.float().cpu()[sel], ref[sel]), _err(fused.float().cpu()[sel], ref[sel])
    print(f"{what}: fused {ef:.3e} stock {es:.3e}")
    assert ef <= 1.5 * es + EPS, (what, ef, es)


def _gate_prefill(fused, stock, ref, mask, nl):
    sel = mask.bool()
    _gate(fused.logits, stock.logits, ref.logits, sel, "logits")
    for li in (0, nl - 1):
        for name in ("keys", "values"):
            f, s, r = (getattr(o.past_key_values.layers[li], name).transpose(1, 2) for o in (fused, stock, ref))
            _gate(f, s, r, sel, f"layer {li} {name}")


@pytest.mark.parametrize("kind", ["qwen3", "llama"])
@pytest.mark.parametrize("side", ["left", "right"])
def test_padded_prefill_matches_the_stock_decoder(ops, kind, side):
    """A left-padded (B = 3, pads 0 / 5 / 66: none, inside the first key tile, past it) or right-padded (B = 2, lengths 70 / 41)
    prefill through the patched layers: logits and the first / last layer's cache at the unpadded positions pass the gate, it
    took the fused route (counter, bits differ from the stock run), and nothing is non-finite, padding rows included."""
    from u2tokenizer_amd import prefill
    nl, S, E = 3, 70, 512
    mask = _mask(S, pads=(0, 5, 66)) if side == "left" else _mask(S, lengths=(70, 41))
    B = mask.shape[0]
    m32 = _small(kind, nl)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, E), 3)
    ref = m32(inputs_embeds=x, attention_mask=mask, use_cache=True)
    mg = _small(kind, nl).to(bf).to(D)
    xd, md = x.to(bf).to(D), mask.to(D)
    stock = mg(inputs_embeds=xd, attention_mask=md, use_cache=True)
    assert prefill.enable_fused_prefill(mg, padded=True) == nl
    n0 = dict(prefill.stats)
    fused = mg(inputs_embeds=xd, attention_mask=md, use_cache=True)
    prefill.disable_fused_prefill(mg)
    assert prefill.stats["padded_prefill"] - n0["padded_prefill"] == nl and prefill.stats["prefill"] == n0["prefill"]
    assert torch.isfinite(fused.logits).all()
    for lay in fused.past_key_values.layers:
        assert torch.isfinite(lay.keys).all() and torch.isfinite(lay.values).all() and lay.keys.shape[2] == S
    assert not torch.equal(fused.logits, stock.logits)
    _gate_prefill(fused, stock, ref, mask, nl)


@pytest.mark.parametrize("kind,wide", [("qwen3", False), ("llama", False), ("qwen3", True)])
def test_padded_decode_step_matches_the_stock_decoder(ops, kind, wide):
    """One decode step after a left-padded prefill, both through the patched layers: logits and the new cache entries pass the
    gate; the step took the padded decode route.  wide: one layer at the Qwen3-8B width, B = 2, S = 40, pads 0 / 7."""
    from u2tokenizer_amd import prefill
    nl, E, S, pads = (1, 4096, 40, (0, 7)) if wide else (3, 512, 70, (0, 5, 66))
    B = len(pads)
    mask = _mask(S, pads=pads)
    mask1 = torch.cat([mask, torch.ones(B, 1, dtype=torch.int64)], 1)
    m32 = _small(kind, nl, wide)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, E), 7)
    x1 = 0.5 * synth.synth_tensor("inputs_embeds", (B, 1, E), 8)
    p32 = m32(inputs_embeds=x, attention_mask=mask, use_cache=True)
    ref = m32(inputs_embeds=x1, attention_mask=mask1, past_key_values=p32.past_key_values, use_cache=True)
    mg = _small(kind, nl, wide).to(bf).to(D)
    xd, x1d, md, m1d = x.to(bf).to(D), x1.to(bf).to(D), mask.to(D), mask1.to(D)
    ps = mg(inputs_embeds=xd, attention_mask=md, use_cache=True)
    stock = mg(inputs_embeds=x1d, attention_mask=m1d, past_key_values=ps.past_key_values, use_cache=True)
    prefill.enable_fused_prefill(mg, padded=True)
    n0 = dict(prefill.stats)
    pf = mg(inputs_embeds=xd, attention_mask=md, use_cache=True)
    fused = mg(inputs_embeds=x1d, attention_mask=m1d, past_key_values=pf.past_key_values, use_cache=True)
    prefill.disable_fused_prefill(mg)
    assert prefill.stats["padded_prefill"] - n0["padded_prefill"] == nl
    assert prefill.stats["padded_decode"] - n0["padded_decode"] == nl and prefill.stats["decode"] == n0["decode"]
    assert fused.logits.shape == stock.logits.shape == (B, 1, ref.logits.shape[-1]) and torch.isfinite(fused.logits).all()
    assert not torch.equal(fused.logits, stock.logits)
    every = torch.ones(B, 1, dtype=torch.bool)
    _gate(fused.logits, stock.logits, ref.logits, every, "logits")
    for li in (0, nl - 1):
        for name in ("keys", "values"):
            f, s, r = (getattr(o.past_key_values.layers[li], name) for o in (fused, stock, ref))
            assert f.shape == r.shape and f.shape[2] == S + 1
            _gate(f[:, :, -1:].transpose(1, 2), s[:, :, -1:].transpose(1, 2), r[:, :, -1:].transpose(1, 2), every, f"layer {li} new {name}")


def test_generate_on_a_left_padded_batch_equals_each_prompt_alone(ops):
    """HF generate (greedy, 4 new tokens) on three prompts of 9 / 20 / 70 ids, left-padded into one batch, through the padded
    routes: the ids of every prompt equal those of that prompt generated alone, unpadded, through the fused route."""
    from u2tokenizer_amd import prefill
    new, lens = 4, (9, 20, 70)
    mg = decisive_decoder_(_small("qwen3", layers=2), 0).to(bf).to(D)
    g = torch.Generator().manual_seed(11)
    prompts = [torch.randint(3, 1024, (n,), generator=g) for n in lens]
    S = max(lens)
    ids = torch.zeros(len(lens), S, dtype=torch.int64)
    mask = torch.zeros(len(lens), S, dtype=torch.int64)
    for b, p in enumerate(prompts):
        ids[b, S - len(p):] = p
        mask[b, S - len(p):] = 1
    kw = dict(max_new_tokens=new, min_new_tokens=new, do_sample=False, pad_token_id=0)
    prefill.enable_fused_prefill(mg, padded=True)
    n0 = dict(prefill.stats)
    batch = mg.generate(input_ids=ids.to(D), attention_mask=mask.to(D), **kw).cpu()
    assert prefill.stats["padded_prefill"] - n0["padded_prefill"] == 2
    assert prefill.stats["padded_decode"] - n0["padded_decode"] == 2 * (new - 1)
    compared = 0
    for b, p in enumerate(prompts):
        alone = mg.generate(input_ids=p[None].to(D), attention_mask=torch.ones(1, len(p), dtype=torch.int64, device=D), **kw).cpu()
        assert alone.shape == (1, len(p) + new) and batch.shape == (len(lens), S + new)
        for t in range(new):
            assert batch[b, S + t] == alone[0, len(p) + t], (b, t, batch[b, S:], alone[0, len(p):])
            compared += 1
    prefill.disable_fused_prefill(mg)
    assert compared == new * len(lens)


def test_padded_batches_stay_stock_with_the_switch_off(ops):
    """The default: a padded batch through patched layers is bit-identical to the unpatched model; the padded counters stay put."""
    from u2tokenizer_amd import prefill
    mg = _small("qwen3").to(bf).to(D)
    xd = (0.5 * synth.synth_tensor("inputs_embeds", (3, 70, 512), 3)).to(bf).to(D)
    x1d = (0.5 * synth.synth_tensor("inputs_embeds", (3, 1, 512), 8)).to(bf).to(D)
    md = _mask(70, pads=(0, 5, 66)).to(D)
    m1d = torch.cat([md, torch.ones(3, 1, dtype=torch.int64, device=D)], 1)
    want = mg(inputs_embeds=xd, attention_mask=md, use_cache=True)
    want1 = mg(inputs_embeds=x1d, attention_mask=m1d, past_key_values=want.past_key_values, use_cache=True)
    prefill.enable_fused_prefill(mg)
    n0 = dict(prefill.stats)
    got = mg(inputs_embeds=xd, attention_mask=md, use_cache=True)
    got1 = mg(inputs_embeds=x1d, attention_mask=m1d, past_key_values=got.past_key_values, use_cache=True)
    prefill.disable_fused_prefill(mg)
    assert torch.equal(got.logits, want.logits) and torch.equal(got1.logits, want1.logits)
    assert prefill.stats == n0


# ------------------------------------------------------------------------------------------------- 9. the step's second half
def test_decode_post_null_kv_start_is_all_zeros_and_both_forms_repeat(ops):
    """u2tok_decoder_decode_post called directly at the smallest shape that still splits the keys (T = 300: five tiles of 64
    keys, the split picker wants four), 16-bit weights: batched = 1 gives the same bits for kv_start = NULL and kv_start = zeros,
    and either attention form gives the same bits twice.  (The two forms are not compared: the model tests above and in
    tests/test_gpu_prefill.py hold each to the float64 gate.)"""
    import ctypes as C
    from u2tokenizer_amd import _lib
    B, E, Hq, Hkv, d, inter, T = 2, 128, 4, 2, 64, 256, 300
    x, qkv = rnd(B, E, seed=31).to(D), rnd(B, (Hq + 2 * Hkv) * d, seed=32).to(D)
    K, V = rnd(B, Hkv, T, d, seed=33).to(D), rnd(B, Hkv, T, d, seed=34).to(D)
    Wo, wn = rnd(E, Hq * d, scale=0.06, seed=35).to(D), (1 + rnd(E, scale=0.1, seed=36).float()).to(bf).to(D)
    Wgu, Wd = rnd(2 * inter, E, scale=0.09, seed=37).to(D), rnd(E, inter, scale=0.06, seed=38).to(D)
    cfg = _lib.DecodeConfig(B=B, E=E, Hq=Hq, Hkv=Hkv, D=d, I=inter, eps=1e-6, qk_eps=1e-6, scale=d ** -0.5)
    lay = _lib.DecodeLayer(Wo=Wo.data_ptr(), w_post_norm=wn.data_ptr(), Wgu=Wgu.data_ptr(), Wdown=Wd.data_ptr())
    zeros = torch.zeros(B, dtype=torch.int32, device=D)
    with ops.on_device(x) as (h, stream):
        ws = torch.empty(h.u2tok_decoder_decode_workspace_bytes(C.byref(cfg), T), dtype=torch.uint8, device=D)

        def post(batched, kv_start=None):
            out = torch.full((B, E), float("nan"), dtype=bf, device=D)
            _lib.check(h.u2tok_decoder_decode_post(C.byref(cfg), C.byref(lay), x.data_ptr(), qkv.data_ptr(), K.data_ptr(), V.data_ptr(),
                                                   T, 0, batched, None if kv_start is None else kv_start.data_ptr(), out.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), stream), "u2tok_decoder_decode_post")
            return out

        loop, batched, with_zeros = (post(0), post(0)), (post(1), post(1)), post(1, zeros)
    assert torch.isfinite(loop[0]).all() and torch.isfinite(batched[0]).all()
    assert torch.equal(loop[0], loop[1]) and torch.equal(batched[0], batched[1])
    assert torch.equal(batched[0], with_zeros)
