"""GPU: the continued prefill (opt-in, `enable_fused_prefill(model, continued=True)`): the attention kernel with the lower edge of
an attention window and K / V read in a KV cache's own layout (u2tok_attention_gqa_band) against fp32 masked softmaxes on the
host, on the bf16 and the f16 build; whole small decoders (shapes, gate and helpers of tests/test_gpu_padded_batches.py and
tests/test_gpu_phi3_decoder.py, copied here) on a second turn, a chunked prefill, a Phi-3 prefill past its window, a left-padded
continuation and `generate` across two turns; the switch off."""
import math

import pytest
import torch
import torch.nn.functional as F

from u2tokenizer_amd import synth

from helpers import decisive_decoder_

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"
EPS = {torch.bfloat16: 1e-3, torch.float16: 1.5e-4}
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


def _visible(Sq, Skv, W, start=None):
    """(nb | 1, Sq, Skv): key j visible to query i iff i + c_off - W < j <= i + c_off, c_off = Skv - Sq, and j >= start[b]."""
    i, j = torch.arange(Sq)[:, None], torch.arange(Skv)[None, :]
    c = Skv - Sq
    vis = j <= i + c
    if W:
        vis = vis & (j > i + c - W)
    vis = vis[None]
    if start is not None:
        vis = vis & (j[None] >= torch.tensor(start)[:, None, None])
    return vis


def _softmax_ref(q, K, V, Hq, scale, vis):
    """fp32 masked softmax on the host: q (nb, Sq, Hq * d), K / V (nb, Hkv, Skv, d) -> (nb, Sq, Hq * d), rows that see a key."""
    nb, Sq, _ = q.shape
    Hkv, d = K.shape[1], K.shape[3]
    qh = q.float().view(nb, Sq, Hq, d).transpose(1, 2)
    kh, vh = K.float().repeat_interleave(Hq // Hkv, 1), V.float().repeat_interleave(Hq // Hkv, 1)
    s = (qh @ kh.transpose(-1, -2) * scale).masked_fill(~vis[:, None], float("-inf"))
    sees = vis.any(-1).expand(nb, Sq)
    p = torch.where(sees[:, None, :, None], F.softmax(s, -1), torch.zeros(()))
    return (p @ vh).transpose(1, 2).reshape(nb, Sq, Hq * d), sees


def _twice(fn):
    a, b = fn(), fn()
    assert torch.equal(a, b)
    return a


# ------------------------------------------------------------------------------------------------- 1. band, column layout
BAND_CASES = [(2, 200, 8, 2, 64, 32), (1, 200, 4, 4, 128, 32), (1, 200, 3, 3, 96, 32),   # block 1's band starts mid-tile
              (2, 200, 8, 2, 64, 64),                                                    # W = one tile
              (1, 130, 4, 2, 128, 1),                                                    # every row sees only itself
              (1, 70, 4, 2, 64, 500)]                                                    # W > S: attention_gqa's values


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("nb,S,Hq,Hkv,d,W", BAND_CASES)
def test_band_on_the_column_layout_against_masked_softmax(ops, elem, nb, S, Hq, Hkv, d, W):
    """Sq = Skv, q | k | v column views of one packed buffer, window W: against fp32, twice with equal bits.  With W = 32 and
    S = 200 the second query block loads key tile 0 for its first rows, in which its rows >= 95 see nothing (asserted)."""
    dt, ulp = elem
    buf = rnd(nb, S, (Hq + 2 * Hkv) * d, seed=S + d + W, dtype=dt)
    q, k, v = buf[..., :Hq * d], buf[..., Hq * d:(Hq + Hkv) * d], buf[..., (Hq + Hkv) * d:]
    dbuf = buf.to(D)
    dq, dk, dv = dbuf[..., :Hq * d], dbuf[..., Hq * d:(Hq + Hkv) * d], dbuf[..., (Hq + Hkv) * d:]
    scale = 1.5 / math.sqrt(d)
    got = _twice(lambda: ops.attention_gqa_band(dq, dk, dv, Hq, Hkv, scale, window=W))
    vis = _visible(S, S, W)
    if (S, W) == (200, 32):
        assert not vis[0, 95:128, :64].any() and vis[0, 64:95, :64].any(-1).all() and vis[0, 95:128, 64:128].any(-1).all()
    ref, sees = _softmax_ref(q, k.view(nb, S, Hkv, d).transpose(1, 2), v.view(nb, S, Hkv, d).transpose(1, 2), Hq, scale, vis)
    assert sees.all()
    close(got, ref, ulp)
    if W > S:
        assert torch.equal(got, ops.attention_gqa(dq, dk, dv, Hq, Hkv, scale, causal=True))


# ------------------------------------------------------------------------------------------------- 2. continued, cache layout
CACHE_CASES = [(2, 5, 133, 8, 2, 128, None),
               (1, 70, 200, 8, 8, 96, 96),
               (2, 130, 137, 8, 4, 64, None),
               (1, 37, 68, 4, 2, 64, 32)]     # a sliding layer's operand: W - 1 kept positions + S new ones


def _cache_operands(B, Sq, Skv, Hq, Hkv, d, dt, seed):
    """q (B, Sq, Hq d) and K / V as views [:, :, :Skv] of (B, Hkv, Skv + 37, d) buffers, on the host and on the GPU."""
    q = rnd(B, Sq, Hq * d, seed=seed, dtype=dt)
    kb, vb = rnd(B, Hkv, Skv + 37, d, seed=seed + 1, dtype=dt), rnd(B, Hkv, Skv + 37, d, seed=seed + 2, dtype=dt)
    dkb, dvb = kb.to(D), vb.to(D)
    return q, kb[:, :, :Skv], vb[:, :, :Skv], q.to(D), dkb[:, :, :Skv], dvb[:, :, :Skv]


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("B,Sq,Skv,Hq,Hkv,d,W", CACHE_CASES)
def test_new_rows_against_a_cache_view_against_masked_softmax(ops, elem, B, Sq, Skv, Hq, Hkv, d, W):
    """Sq new query rows at the end of Skv keys that lie in a cache's (B, Hkv, capacity, d) buffers (37 spare positions), read
    in place: against fp32, twice with equal bits."""
    dt, ulp = elem
    q, K, V, dq, dK, dV = _cache_operands(B, Sq, Skv, Hq, Hkv, d, dt, Sq + Skv)
    assert not dK.is_contiguous() and dK.stride(1) == (Skv + 37) * d
    scale = 1.5 / math.sqrt(d)
    got = _twice(lambda: ops.attention_gqa_band(dq, dK, dV, Hq, Hkv, scale, window=W))
    ref, sees = _softmax_ref(q, K, V, Hq, scale, _visible(Sq, Skv, W))
    assert sees.all()
    close(got, ref, ulp)


# ------------------------------------------------------------------------------------------------- 3. both layouts, equal bits
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("B,Sq,Skv,Hq,Hkv,d,W", [(2, 70, 137, 8, 4, 64, None), (2, 70, 137, 8, 4, 64, 32), (1, 37, 133, 4, 2, 128, 40),
                                                 (1, 70, 200, 8, 8, 96, 96)])
def test_cache_view_and_column_packed_copy_give_equal_bits(ops, elem, B, Sq, Skv, Hq, Hkv, d, W):
    dt, _ = elem
    _, _, _, dq, dK, dV = _cache_operands(B, Sq, Skv, Hq, Hkv, d, dt, 3)
    ck, cv = (t.transpose(1, 2).reshape(B, Skv, Hkv * d).contiguous() for t in (dK, dV))
    a = ops.attention_gqa_band(dq, dK, dV, Hq, Hkv, 0.11, window=W)
    b = ops.attention_gqa_band(dq, ck, cv, Hq, Hkv, 0.11, window=W)
    assert torch.equal(a, b) and a.abs().max() > 0


# ------------------------------------------------------------------------------------------------- 4. with kv_start
@pytest.mark.parametrize("elem", ELEMS)
def test_cache_view_with_a_first_visible_key_per_sequence(ops, elem):
    """(B, Sq, Skv) = (3, 6, 76), starts 0 / 5 / 66, cache layout: the mask of 6 new positions after a left-padded 70-position
    prefill.  Every row sees a key here (asserted; rows that saw none would have to be exact zeros), and the starts do hide keys
    the causal rule alone would show."""
    dt, ulp = elem
    B, Sq, Skv, Hq, Hkv, d, start = 3, 6, 76, 8, 4, 64, (0, 5, 66)
    q, K, V, dq, dK, dV = _cache_operands(B, Sq, Skv, Hq, Hkv, d, dt, 9)
    scale = 1.5 / math.sqrt(d)
    got = _twice(lambda: ops.attention_gqa_band(dq, dK, dV, Hq, Hkv, scale, kv_start=_i32(start)))
    vis = _visible(Sq, Skv, None, start)
    assert (vis.sum(-1)[1] < _visible(Sq, Skv, None).sum(-1)[0]).all() and vis[2].sum(-1).tolist() == [5, 6, 7, 8, 9, 10]
    ref, sees = _softmax_ref(q, K, V, Hq, scale, vis)
    assert sees.all()
    close(got[sees.to(D)], ref[sees], ulp)
    assert (got[(~sees).to(D)] == 0).all()
    assert not torch.equal(got, ops.attention_gqa_band(dq, dK, dV, Hq, Hkv, scale))


def test_rows_below_every_visible_key_are_exact_zeros(ops):
    """Sq = Skv = 70 with a window and starts 0 / 40: rows of sequence 1 before its first key see nothing and come back as exact
    zeros; rows 40 .. 69 of it see part of their window."""
    B, S, Hq, Hkv, d, W, start = 2, 70, 4, 2, 64, 8, (0, 40)
    buf = rnd(B, S, (Hq + 2 * Hkv) * d, seed=4)
    q, k, v = buf[..., :Hq * d], buf[..., Hq * d:(Hq + Hkv) * d], buf[..., (Hq + Hkv) * d:]
    dbuf = buf.to(D)
    got = ops.attention_gqa_band(dbuf[..., :Hq * d], dbuf[..., Hq * d:(Hq + Hkv) * d], dbuf[..., (Hq + Hkv) * d:], Hq, Hkv, 0.2,
                                 window=W, kv_start=_i32(start))
    ref, sees = _softmax_ref(q, k.view(B, S, Hkv, d).transpose(1, 2), v.view(B, S, Hkv, d).transpose(1, 2), Hq, 0.2,
                             _visible(S, S, W, start))
    assert sees[0].all() and not sees[1, :40].any() and sees[1, 40:].all()
    close(got[sees.to(D)], ref[sees], 2.0 ** -8)
    assert (got[(~sees).to(D)] == 0).all()


# ------------------------------------------------------------------------------------------------- 5. defaults
@pytest.mark.parametrize("elem", ELEMS)
def test_defaults_are_the_existing_kernels(ops, elem):
    dt, _ = elem
    buf = rnd(2, 77, (8 + 2 * 4) * 64, seed=5, dtype=dt).to(D)
    q, k, v = buf[..., :512], buf[..., 512:768], buf[..., 768:]
    assert torch.equal(ops.attention_gqa_band(q, k, v, 8, 4, 0.125), ops.attention_gqa(q, k, v, 8, 4, 0.125, causal=True))
    st, ln = _i32((3, 70)), _i32((60, 77))
    assert torch.equal(ops.attention_gqa_band(q, k, v, 8, 4, 0.125, kv_start=st, kv_len=ln),
                       ops.attention_gqa_range(q, k, v, 8, 4, 0.125, kv_start=st, kv_len=ln))


def test_wrapper_refuses_what_the_kernel_does_not_read(ops):
    q = rnd(1, 8, 4 * 64).to(D)
    kb, vb = rnd(1, 2, 40, 64, seed=1).to(D), rnd(1, 2, 48, 64, seed=2).to(D)
    with pytest.raises(RuntimeError):
        ops.attention_gqa_band(q, kb[:, :, :24], vb[:, :, :24], 4, 2, 0.1)               # two capacities
    with pytest.raises(RuntimeError):
        ops.attention_gqa_band(q, kb.transpose(1, 2), kb.transpose(1, 2), 4, 2, 0.1)     # not (B, Hkv, T, d)
    with pytest.raises(RuntimeError):
        ops.attention_gqa_band(q, kb[:, :, :24], kb[:, :, :24], 4, 2, 0.1, window=4, causal=False)
    with pytest.raises(RuntimeError):
        ops.attention_gqa_band(q, kb[:, :, :4], kb[:, :, :4], 4, 2, 0.1)                 # causal with fewer keys than queries


# ------------------------------------------------------------------------------------------------- 6 - 11. whole decoders
def _small(kind, layers=3):
    from transformers import LlamaConfig, LlamaForCausalLM, Qwen3Config, Qwen3ForCausalLM
    common = dict(vocab_size=1024, hidden_size=512, intermediate_size=1536, num_hidden_layers=layers, num_attention_heads=8,
                  num_key_value_heads=4, head_dim=64, max_position_embeddings=512, tie_word_embeddings=False,
                  pad_token_id=0, bos_token_id=1, eos_token_id=2)
    if kind == "qwen3":
        m = Qwen3ForCausalLM(Qwen3Config(**common))
    else:
        m = LlamaForCausalLM(LlamaConfig(**common, rope_theta=500000.0))
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m.eval()


def _phi3(layers=3, E=768, H=8, Hkv=8, inter=2048, window=2047, vocab=1024, **kw):
    from transformers import Phi3Config, Phi3ForCausalLM
    c = dict(vocab_size=vocab, hidden_size=E, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=H,
             num_key_value_heads=Hkv, max_position_embeddings=4096, sliding_window=window, tie_word_embeddings=False,
             pad_token_id=0, bos_token_id=1, eos_token_id=2)
    c.update(kw)
    m = Phi3ForCausalLM(Phi3Config(**c))
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m.eval()


def _err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _mask(S, pads):
    m = torch.ones(len(pads), S, dtype=torch.int64)
    for b, p in enumerate(pads):
        m[b, :p] = 0
    return m


def _gate(fused, stock, ref, sel, what, eps=EPS[bf]):
    """The project's gate at the selected positions: no further from the fp32 model than 1.5 x the stock run of the same type."""
    es, ef = _err(stock.float().cpu()[sel], ref[sel]), _err(fused.float().cpu()[sel], ref[sel])
    print(f"{what}: fused {ef:.3e} stock {es:.3e}")
    assert ef <= 1.5 * es + eps, (what, ef, es)


def _counts():
    """Layer calls per route so far: prefill.stats (the four routes it has always had) and prefill.extend_stats (the continued
    prefill's two) in one snapshot."""
    from u2tokenizer_amd import prefill
    return {**prefill.stats, **prefill.extend_stats}


def _turns(m, xs, cache=None, masks=None):
    """Feed the chunks `xs` one after the other on one cache; -> the outputs of every call."""
    outs = []
    for t, x in enumerate(xs):
        kw = {} if masks is None else {"attention_mask": masks[t]}
        outs.append(m(inputs_embeds=x, past_key_values=cache, use_cache=True, **kw))
        cache = outs[-1].past_key_values
    return outs


def _x(shape, seed, dt=None):
    x = 0.5 * synth.synth_tensor("inputs_embeds", shape, seed)
    return x if dt is None else x.to(dt).to(D)


@pytest.mark.parametrize("kind,filled_by,dt", [("qwen3", "fused", bf), ("llama", "fused", bf), ("qwen3", "stock", bf),
                                               ("llama", "stock", bf), ("qwen3", "fused", torch.float16)])
def test_second_turn_against_a_filled_cache(ops, kind, filled_by, dt):
    """70 positions, then 37 more against the cache (B = 2).  filled_by fused: the first turn runs on the patched layers and
    leaves the append-in-place layers the second turn writes behind; stock: the cache was filled by the stock layers before
    enable_fused_prefill (DynamicLayers: the cache's own `update`).  The second call's logits and the new cache entries of the
    first and last layer pass the gate; it took the new route (counter; not the stock bits)."""
    from u2tokenizer_amd import prefill
    nl, B, S1, S2, E = 3, 2, 70, 37, 512
    shapes = ((B, S1, E), (B, S2, E))
    ref = _turns(_small(kind, nl), [_x(s, 3 + i) for i, s in enumerate(shapes)])[1]
    mg = _small(kind, nl).to(dt).to(D)
    xd = [_x(s, 3 + i, dt) for i, s in enumerate(shapes)]
    stock = _turns(mg, xd)[1]
    first = mg(inputs_embeds=xd[0], use_cache=True) if filled_by == "stock" else None
    assert prefill.enable_fused_prefill(mg, continued=True) == nl
    if first is None:
        first = mg(inputs_embeds=xd[0], use_cache=True)
    kinds = {type(lay).__name__ for lay in first.past_key_values.layers}
    assert kinds == ({"AppendLayer"} if filled_by == "fused" else {"DynamicLayer"})
    n0 = _counts()
    fused = mg(inputs_embeds=xd[1], past_key_values=first.past_key_values, use_cache=True)
    prefill.disable_fused_prefill(mg)
    assert _counts()["extend"] - n0["extend"] == nl
    assert {k: v for k, v in _counts().items() if k != "extend"} == {k: v for k, v in n0.items() if k != "extend"}
    assert fused.logits.shape == (B, S2, 1024) and torch.isfinite(fused.logits).all()
    assert not torch.equal(fused.logits, stock.logits)
    every = torch.ones(B, S2, dtype=torch.bool)
    _gate(fused.logits, stock.logits, ref.logits, every, "logits", EPS[dt])
    for li in (0, nl - 1):
        for name in ("keys", "values"):
            f, s, r = (getattr(o.past_key_values.layers[li], name) for o in (fused, stock, ref))
            assert f.shape == r.shape == (B, 4, S1 + S2, 64)
            _gate(f[:, :, S1:].transpose(1, 2), s[:, :, S1:].transpose(1, 2), r[:, :, S1:].transpose(1, 2), every,
                  f"layer {li} new {name}", EPS[dt])


def test_chunked_prefill_against_the_one_shot_prefill(ops):
    """140 positions fed as 64 + 64 + 12 (B = 2): the last chunk's logits pass the gate against the fp32 model's ONE-SHOT
    prefill, with the stock bf16 run fed the same chunks as the yardstick; one prefill and two continued calls per layer."""
    from u2tokenizer_amd import prefill
    nl, B, S, E = 3, 2, 140, 512
    cuts = ((0, 64), (64, 128), (128, 140))
    x = _x((B, S, E), 6)
    ref = _small("qwen3", nl)(inputs_embeds=x).logits[:, 128:]
    mg = _small("qwen3", nl).to(bf).to(D)
    xd = [x[:, a:b].to(bf).to(D) for a, b in cuts]
    stock = _turns(mg, xd)[-1].logits
    prefill.enable_fused_prefill(mg, continued=True)
    n0 = _counts()
    fused = _turns(mg, xd)[-1]
    prefill.disable_fused_prefill(mg)
    assert _counts()["prefill"] - n0["prefill"] == nl and _counts()["extend"] - n0["extend"] == 2 * nl
    assert fused.past_key_values.get_seq_length() == S and fused.logits.shape == (B, 12, 1024)
    _gate(fused.logits, stock, ref, torch.ones(B, 12, dtype=torch.bool), "last chunk's logits")


@pytest.mark.parametrize("cache_kind", ["sliding", "plain"])
def test_phi3_prefill_past_the_window_and_a_continuation(ops, cache_kind):
    """sliding_window = 32, head dim 96: a 70-position prefill takes the new route (counter, gate, not the stock bits), then 20
    more positions onto that cache do -- on the DynamicSlidingWindowLayer cache `generate` builds for such a config (the kernel's
    operand: the kept W - 1 positions and the new ones) and on a plain DynamicCache (the append-in-place layer keeps every
    position; the attention reads the last S + W - 1).  The window matters: without it the fp32 model is far off."""
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd import prefill
    W, nl, E = 32, 3, 768
    mk = (lambda m: DynamicCache(config=m.config)) if cache_kind == "sliding" else (lambda m: DynamicCache())
    shapes = ((1, 70, E), (1, 20, E))
    xs = [_x(s, 4 + i) for i, s in enumerate(shapes)]
    m32 = _phi3(window=W)
    ref = _turns(m32, xs, mk(m32))
    mg = _phi3(window=W).to(bf).to(D)
    xd = [x.to(bf).to(D) for x in xs]
    stock = _turns(mg, xd, mk(mg))
    prefill.enable_fused_prefill(mg, continued=True)
    cache = mk(mg)
    n0 = _counts()
    f1 = mg(inputs_embeds=xd[0], past_key_values=cache, use_cache=True)
    assert _counts()["extend"] - n0["extend"] == nl and _counts()["prefill"] == n0["prefill"]
    f2 = mg(inputs_embeds=xd[1], past_key_values=cache, use_cache=True)
    prefill.disable_fused_prefill(mg)
    assert _counts()["extend"] - n0["extend"] == 2 * nl
    if cache_kind == "sliding":
        assert type(cache.layers[0]).__name__ == "DynamicSlidingWindowLayer" and cache.layers[0].keys.shape[2] == W - 1
    else:
        assert type(cache.layers[0]).__name__ == "AppendLayer" and cache.layers[0].keys.shape[2] == 90
    for t, (f, s, r) in enumerate(zip((f1, f2), stock, ref)):
        assert not torch.equal(f.logits, s.logits), t
        _gate(f.logits, s.logits, r.logits, torch.ones(1, shapes[t][1], dtype=torch.bool), f"call {t} logits")
    full = _turns(_phi3(window=None), xs, DynamicCache())
    assert _err(ref[0].logits, full[0].logits) > 10 * EPS[bf] and _err(ref[1].logits, full[1].logits) > 10 * EPS[bf]


def test_left_padded_continuation(ops):
    """padded=True, continued=True: pads 0 / 5 / 66 on a 70-position prefill, then 6 positions onto its cache under a mask of
    76 columns: the padded continued route (counter), the gate at the six new (unpadded) positions of every sequence."""
    from u2tokenizer_amd import prefill
    nl, B, S1, S2, E = 3, 3, 70, 6, 512
    m1 = _mask(S1, (0, 5, 66))
    masks = [m1, torch.cat([m1, torch.ones(B, S2, dtype=torch.int64)], 1)]
    xs = [_x((B, S1, E), 3), _x((B, S2, E), 8)]
    ref = _turns(_small("qwen3", nl), xs, masks=masks)[1]
    mg = _small("qwen3", nl).to(bf).to(D)
    xd, md = [x.to(bf).to(D) for x in xs], [m.to(D) for m in masks]
    stock = _turns(mg, xd, masks=md)[1]
    prefill.enable_fused_prefill(mg, padded=True, continued=True)
    n0 = _counts()
    fused = _turns(mg, xd, masks=md)[1]
    prefill.disable_fused_prefill(mg)
    assert _counts()["padded_prefill"] - n0["padded_prefill"] == nl
    assert _counts()["padded_extend"] - n0["padded_extend"] == nl and _counts()["extend"] == n0["extend"]
    assert torch.isfinite(fused.logits).all() and not torch.equal(fused.logits, stock.logits)
    every = torch.ones(B, S2, dtype=torch.bool)
    _gate(fused.logits, stock.logits, ref.logits, every, "logits")
    for li in (0, nl - 1):
        for name in ("keys", "values"):
            f, s, r = (getattr(o.past_key_values.layers[li], name)[:, :, S1:].transpose(1, 2) for o in (fused, stock, ref))
            _gate(f, s, r, every, f"layer {li} new {name}")


def test_generate_across_two_turns_equals_generating_in_one_go(ops):
    """HF `generate` itself, handed the cache it returned (this transformers accepts `past_key_values` there): greedy, 4 tokens
    from a 20-id prompt; then again with that cache and the sequence extended by 9 new prompt ids.  The 4 ids of the second turn
    equal those of generating from the concatenated 33 ids in one go, and the second call's first forward -- the one uncached
    generated id plus the 9 new ones against 23 cached positions -- took the continued route."""
    from u2tokenizer_amd import prefill
    new, nl = 4, 2
    mg = decisive_decoder_(_small("qwen3", layers=nl), 0).to(bf).to(D)
    g = torch.Generator().manual_seed(11)
    prompt, more = torch.randint(3, 1024, (1, 20), generator=g).to(D), torch.randint(3, 1024, (1, 9), generator=g).to(D)
    kw = dict(max_new_tokens=new, min_new_tokens=new, do_sample=False, pad_token_id=0, return_dict_in_generate=True)
    prefill.enable_fused_prefill(mg, continued=True)
    t1 = mg.generate(input_ids=prompt, **kw)
    assert t1.sequences.shape == (1, 24) and t1.past_key_values.get_seq_length() == 23
    ids2 = torch.cat([t1.sequences, more], 1)
    n0 = _counts()
    t2 = mg.generate(input_ids=ids2, past_key_values=t1.past_key_values, **kw)
    assert _counts()["extend"] - n0["extend"] == nl and _counts()["prefill"] == n0["prefill"]
    assert _counts()["decode"] - n0["decode"] == nl * (new - 1)
    n1 = _counts()
    whole = mg.generate(input_ids=ids2, **kw)
    prefill.disable_fused_prefill(mg)
    assert _counts()["prefill"] - n1["prefill"] == nl and _counts()["extend"] == n1["extend"]
    assert t2.sequences.shape == whole.sequences.shape == (1, 33 + new)
    assert torch.equal(t2.sequences, whole.sequences), (t2.sequences[0, 33:], whole.sequences[0, 33:])


def test_switch_off_is_the_stock_run(ops):
    """continued=False (the default): the second-turn call and the Phi-3 prefill past its window leave every counter unchanged
    and give the stock run's bits."""
    from u2tokenizer_amd import prefill
    mg = _small("qwen3").to(bf).to(D)
    xd = [_x((2, 70, 512), 3, bf), _x((2, 37, 512), 4, bf)]
    want = _turns(mg, xd)[1].logits
    first = mg(inputs_embeds=xd[0], use_cache=True)
    prefill.enable_fused_prefill(mg)
    n0 = _counts()
    got = mg(inputs_embeds=xd[1], past_key_values=first.past_key_values, use_cache=True).logits
    prefill.disable_fused_prefill(mg)
    assert torch.equal(got, want) and _counts() == n0
    mp = _phi3(window=32).to(bf).to(D)
    xl = _x((1, 70, 768), 4, bf)
    want = mp(inputs_embeds=xl, use_cache=True).logits
    prefill.enable_fused_prefill(mp)
    got = mp(inputs_embeds=xl, use_cache=True).logits
    prefill.disable_fused_prefill(mp)
    assert torch.equal(got, want) and _counts() == n0
