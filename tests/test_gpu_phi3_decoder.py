"""GPU: the Phi-3 decoder on the HIP layers (prefill.py: _PackedLayout; head dim 96 in tokattn.hip / decoder.hip) -- the
kernels at d = 96 against fp32 torch expressions, whole Phi-3 models against the same model in fp32 on the host with the stock
GPU run of the element type as the yardstick, the sliding window on both cache-layer kinds, `generate` through
u2Phi3ForCausalLM, and the cases that must stay stock.  Every case runs in bf16 AND fp16 (the f16 build of the library).

Cases that fail without the feature: every d = 96 kernel call (the library returned U2TOK_ERR_ARG), every fused Phi-3 run
(`enable_fused_prefill` refused the layer: the fused logits equalled the stock ones), the windowed decode steps."""
import math

import pytest
import torch
import torch.nn.functional as F

from u2tokenizer_amd import synth

pytestmark = pytest.mark.gpu
D = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
EPS = {torch.bfloat16: 1e-3, torch.float16: 1.5e-4}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


def rnd(dt, *shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dt)


def close(got, ref, dt, rounds=2):
    """tests/test_gpu_prefill.py: close_bf16 with the element type's unit roundoff"""
    got, ref = got.float().cpu(), ref.float()
    assert torch.isfinite(got).all()
    u = ULP[dt]
    tol = rounds * u * ref.abs() + u * ref.abs().max()
    bad = (got - ref).abs() > tol
    assert not bad.any(), f"{bad.sum().item()} elements off; worst {(got - ref).abs().max().item():.3e}"


def _err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


# ------------------------------------------------------------------------------------------------ kernels at d = 96
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("nb,Sq,Skv,Hq,Hkv", [(1, 1024, 1024, 32, 32), (2, 77, 77, 8, 4), (1, 40, 100, 8, 2), (3, 1, 1, 2, 1)])
def test_attention_gqa_causal_d96(ops, dt, nb, Sq, Skv, Hq, Hkv):
    """tok_attn_kernel<96>, causal grouped-query mode (the prefill's attention) against torch in fp32 on the same inputs;
    q / k / v are column slices of one packed buffer where Sq == Skv, as prefill.py passes them; repeatable bit for bit."""
    d = 96
    if Sq == Skv:
        buf = rnd(dt, nb, Sq, (Hq + 2 * Hkv) * d, seed=Sq + d)
        q, k, v = buf[..., :Hq * d], buf[..., Hq * d:(Hq + Hkv) * d], buf[..., (Hq + Hkv) * d:]
        dbuf = buf.to(D)
        dq, dk, dv = dbuf[..., :Hq * d], dbuf[..., Hq * d:(Hq + Hkv) * d], dbuf[..., (Hq + Hkv) * d:]
    else:
        q, kv = rnd(dt, nb, Sq, Hq * d, seed=1), rnd(dt, nb, Skv, 2 * Hkv * d, seed=2)
        k, v = kv[..., :Hkv * d], kv[..., Hkv * d:]
        dq, dkv = q.to(D), kv.to(D)
        dk, dv = dkv[..., :Hkv * d], dkv[..., Hkv * d:]
    scale = 1.5 / math.sqrt(d)
    got = [ops.attention_gqa(dq, dk, dv, Hq, Hkv, scale, causal=True) for _ in range(2)]
    assert torch.equal(got[0], got[1])
    qh = q.float().view(nb, Sq, Hq, d).transpose(1, 2)
    kh = k.float().view(nb, Skv, Hkv, d).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    vh = v.float().view(nb, Skv, Hkv, d).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    s = qh @ kh.transpose(-1, -2) * scale
    i, j = torch.arange(Sq)[:, None], torch.arange(Skv)[None, :]
    s = s.masked_fill(j > i + (Skv - Sq), float("-inf"))
    close(got[0], (F.softmax(s, -1) @ vh).transpose(1, 2).reshape(nb, Sq, Hq * d), dt)
    ref2 = (F.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).transpose(1, 2).reshape(nb, Sq, Hq * d)
    close(ops.attention_gqa(dq, dk, dv, Hq, Hkv, scale, causal=False), ref2, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("nb,T,g", [(32, 5, 1), (3, 70, 2), (8, 1070, 4), (32, 1100, 1), (16, 1792, 4)])
def test_attention_gqa_split_keys_single_query_row_d96(ops, dt, nb, T, g):
    """The decode step's attention at d = 96: one query row per (batch x kv head) entry, the keys split over workgroups and
    merged by the combine kernels (H d / 4 = 24 g float4 columns per row); 1 and 17 tiles of 64 keys are odd counts."""
    d = 96
    q = rnd(dt, nb, 1, g * d, seed=21)
    k, v = rnd(dt, nb, T, d, seed=22), rnd(dt, nb, T, d, seed=23)
    sc = (q.float().view(nb, g, d) @ k.float().transpose(1, 2)) * d ** -0.5
    ref = (torch.softmax(sc, -1) @ v.float()).reshape(nb, 1, g * d)
    outs = [ops.attention_gqa(q.to(D), k.to(D), v.to(D), g, 1, d ** -0.5, causal=False, split_keys=True) for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    close(outs[0], ref, dt, rounds=3)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,Hq,Hkv,norm,f32", [(1024, 32, 32, False, True), (70, 8, 4, False, False), (33, 4, 4, True, True),
                                                  (9, 8, 2, True, False)])
def test_qk_norm_rope_d96(ops, dt, rows, Hq, Hkv, norm, f32):
    """qk_norm_rope_kernel<96, float | element>: rotate_half over the 96-wide head (lanes 48..63 idle), optional head norm;
    V untouched; the KV-cache form writes the same keys and the values into (batch, kv heads, capacity, 96) buffers."""
    d = 96
    qkv = rnd(dt, rows, (Hq + 2 * Hkv) * d, seed=3)
    wq, wk = (1 + 0.1 * rnd(dt, d, seed=4).float()).to(dt), (1 + 0.1 * rnd(dt, d, seed=5).float()).to(dt)
    pos = torch.arange(rows, dtype=torch.float32)
    inv = 1.0 / (1e4 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.cat([pos[:, None] * inv[None]] * 2, -1)
    cos, sin = fr.cos(), fr.sin()
    if not f32:
        cos, sin = cos.to(dt), sin.to(dt)
    x = qkv.float().view(rows, Hq + 2 * Hkv, d)
    ref = x.clone()
    for lo, hi, w in ((0, Hq, wq), (Hq, Hq + Hkv, wk)):
        h = x[:, lo:hi]
        if norm:
            h = ((h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + 1e-6)).to(dt).float() * w.float()).to(dt).float()
        rot = torch.cat((-h[..., d // 2:], h[..., :d // 2]), -1)
        ref[:, lo:hi] = h * cos.float()[:, None] + rot * sin.float()[:, None]
    wqd, wkd = (wq.to(D), wk.to(D)) if norm else (None, None)
    got = qkv.to(D)
    ops.qk_norm_rope(got, wqd, wkd, cos.to(D), sin.to(D), Hq, Hkv, d, 1e-6)
    close(got, ref.reshape(rows, -1), dt)
    assert torch.equal(got[:, (Hq + Hkv) * d:].cpu(), qkv[:, (Hq + Hkv) * d:])
    S = rows // 3 if rows % 3 == 0 else rows
    got2 = qkv.to(D)
    r = ops.qk_norm_rope(got2, wqd, wkd, cos.to(D), sin.to(D), Hq, Hkv, d, 1e-6, kv_cache_seq=S)
    assert torch.equal(r[0], got)
    g4 = got.view(rows // S, S, Hq + 2 * Hkv, d)
    assert torch.equal(r[1], g4[:, :, Hq:Hq + Hkv].transpose(1, 2)) and torch.equal(r[2], g4[:, :, Hq + Hkv:].transpose(1, 2))
    cap, p0 = S + 5, 2
    kb = torch.full((rows // S, Hkv, cap, d), 7.0, dtype=dt, device=D)
    vb = torch.full((rows // S, Hkv, cap, d), 7.0, dtype=dt, device=D)
    ops.qk_norm_rope(qkv.to(D), wqd, wkd, cos.to(D), sin.to(D), Hq, Hkv, d, 1e-6, kv_cache_seq=S, kv_out=(kb, vb), kv_pos=p0)
    assert torch.equal(kb[:, :, p0:p0 + S], r[1]) and torch.equal(vb[:, :, p0:p0 + S], r[2])
    assert (kb[:, :, :p0] == 7).all() and (kb[:, :, p0 + S:] == 7).all() and (vb[:, :, p0 + S:] == 7).all()


# ------------------------------------------------------------------------------------------------ whole Phi-3 decoders
def _phi3(layers=3, E=768, H=8, Hkv=8, inter=2048, window=2047, vocab=1024, u2=False, **kw):
    from transformers import Phi3Config, Phi3ForCausalLM
    c = dict(vocab_size=vocab, hidden_size=E, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=H,
             num_key_value_heads=Hkv, max_position_embeddings=4096, sliding_window=window, tie_word_embeddings=False,
             pad_token_id=0, bos_token_id=1, eos_token_id=2)
    c.update(kw)
    if u2:
        from u2tokenizer_amd.language_model import u2Phi3Config, u2Phi3ForCausalLM
        m = u2Phi3ForCausalLM(u2Phi3Config(**c))
    else:
        m = Phi3ForCausalLM(Phi3Config(**c))
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m.eval()


def _check_caches(ref, stock, fused, layers, eps):
    for li in layers:
        for name in ("keys", "values"):
            r = getattr(ref.layers[li], name)
            gk = getattr(fused.layers[li], name)
            assert gk.shape == r.shape, (li, name, gk.shape, r.shape)
            es = _err(getattr(stock.layers[li], name).float().cpu(), r)
            ef = _err(gk.float().cpu(), r)
            assert ef <= 1.5 * es + eps, (li, name, ef, es)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("E,H,Hkv", [(768, 8, 8), (768, 8, 4), (512, 4, 2)], ids=["mha96", "gqa96", "gqa128"])
def test_fused_prefill_of_a_small_phi3_matches_the_stock_decoder(ops, dt, E, H, Hkv):
    """Logits and both caches of a prefill (B = 2, S = 70) through the patched Phi-3 layers: no further from the fp32 model than
    1.5 x the stock GPU run of the element type; the logits are not the stock ones (the fused path really ran)."""
    from u2tokenizer_amd.prefill import enable_fused_prefill
    B, S = 2, 70
    m32 = _phi3(E=E, H=H, Hkv=Hkv)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, E), 3)
    ref = m32(inputs_embeds=x, use_cache=True)
    mg = _phi3(E=E, H=H, Hkv=Hkv).to(dt).to(D)
    xd = x.to(dt).to(D)
    stock = mg(inputs_embeds=xd, use_cache=True)
    assert enable_fused_prefill(mg) == 3
    fused = mg(inputs_embeds=xd, use_cache=True)
    e_stock, e_fused = _err(stock.logits.float().cpu(), ref.logits), _err(fused.logits.float().cpu(), ref.logits)
    assert e_fused <= 1.5 * e_stock + EPS[dt], (e_fused, e_stock)
    assert not torch.equal(fused.logits, stock.logits)
    _check_caches(ref.past_key_values, stock.past_key_values, fused.past_key_values, (0, 2), EPS[dt])


def _steps(m, x, xs, cache):
    """prefill x, then one decode step per row of xs, on `cache`; logits of every call (last position of the prefill)"""
    out = [m(inputs_embeds=x, past_key_values=cache, use_cache=True).logits[:, -1]]
    for t in range(xs.shape[1]):
        out.append(m(inputs_embeds=xs[:, t:t + 1], past_key_values=cache, use_cache=True).logits[:, -1])
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("cache_kind", ["sliding", "plain"])
def test_sliding_window_prefill_and_decode(ops, dt, cache_kind):
    """sliding_window = 32: a 70-position prefill takes the stock layers (bit-identical logits); a 24-position fused prefill
    and fused decode steps up to position 39 (past the window) match the fp32 model step by step under the 1.5 x gate, on the
    DynamicSlidingWindowLayer cache that `generate` builds for such a config and on a plain DynamicCache passed in by hand."""
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd.prefill import disable_fused_prefill, enable_fused_prefill
    W, S, n = 32, 24, 16
    mk = (lambda m: DynamicCache(config=m.config)) if cache_kind == "sliding" else (lambda m: DynamicCache())
    m32 = _phi3(window=W)
    mg = _phi3(window=W).to(dt).to(D)
    xl = (0.5 * synth.synth_tensor("inputs_embeds", (1, 70, 768), 4)).to(dt).to(D)
    plain_long = mg(inputs_embeds=xl).logits
    enable_fused_prefill(mg)
    assert torch.equal(mg(inputs_embeds=xl).logits, plain_long)       # S > W: stock layers
    disable_fused_prefill(mg)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (1, S, 768), 5)
    xs = 0.5 * synth.synth_tensor("inputs_embeds", (1, n, 768), 6)
    ref = _steps(m32, x, xs, mk(m32))
    stock = _steps(mg, x.to(dt).to(D), xs.to(dt).to(D), mk(mg))
    enable_fused_prefill(mg)
    cache = mk(mg)
    fused = _steps(mg, x.to(dt).to(D), xs.to(dt).to(D), cache)
    if cache_kind == "sliding":
        assert type(cache.layers[0]).__name__ == "DynamicSlidingWindowLayer" and cache.layers[0].keys.shape[2] == W - 1
    else:
        assert type(cache.layers[0]).__name__ == "AppendLayer" and cache.layers[0].keys.shape[2] == S + n
    for t in range(n + 1):
        es, ef = _err(stock[t].float().cpu(), ref[t]), _err(fused[t].float().cpu(), ref[t])
        assert ef <= 1.5 * es + EPS[dt], (t, ef, es)
        assert not torch.equal(fused[t], stock[t]), t
    # ... and the window matters at these steps: attending over the whole cache would be far off
    assert _err(ref[-1], _steps(_phi3(window=None), x, xs, DynamicCache())[-1]) > 10 * EPS[dt]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_one_layer_at_phi3_mini_width(ops, dt):
    """One layer at the Phi-3-mini shape (E 3072, I 8192, 32 x 96 heads, W 2047): 1024-position prefill and one decode step,
    the kernel variants the real decoder takes; same gate."""
    from u2tokenizer_amd.prefill import enable_fused_prefill
    kw = dict(layers=1, E=3072, H=32, Hkv=32, inter=8192, window=2047)
    m32 = _phi3(**kw)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (1, 1024, 3072), 7)
    x1 = 0.5 * synth.synth_tensor("inputs_embeds", (1, 1, 3072), 8)
    p32 = m32(inputs_embeds=x, use_cache=True)
    r1 = m32(inputs_embeds=x1, past_key_values=p32.past_key_values, use_cache=True)
    mg = _phi3(**kw).to(dt).to(D)
    xd, x1d = x.to(dt).to(D), x1.to(dt).to(D)
    ps = mg(inputs_embeds=xd, use_cache=True)
    s1 = mg(inputs_embeds=x1d, past_key_values=ps.past_key_values, use_cache=True)
    assert enable_fused_prefill(mg) == 1
    pf = mg(inputs_embeds=xd, use_cache=True)
    e_stock, e_fused = _err(ps.logits.float().cpu(), p32.logits), _err(pf.logits.float().cpu(), p32.logits)
    assert e_fused <= 1.5 * e_stock + EPS[dt], (e_fused, e_stock)
    f1 = mg(inputs_embeds=x1d, past_key_values=pf.past_key_values, use_cache=True)
    e_stock, e_fused = _err(s1.logits.float().cpu(), r1.logits), _err(f1.logits.float().cpu(), r1.logits)
    assert e_fused <= 1.5 * e_stock + EPS[dt], (e_fused, e_stock)
    assert not torch.equal(f1.logits, s1.logits)
    _check_caches(r1.past_key_values, s1.past_key_values, f1.past_key_values, (0,), EPS[dt])


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_generate_through_u2phi3(ops, dt):
    """u2Phi3ForCausalLM.generate: the layers are patched on the first no-grad forward (config.u2_fused_prefill), the prefill
    and every decode step go through the HIP layers; greedy ids equal the fp32 model's up to the first step whose fp32 top-2
    margin is below 0.05."""
    from u2tokenizer_amd.prefill import is_patched
    m32 = _phi3(layers=2, u2=True)
    ids = torch.randint(3, 1024, (1, 48), generator=torch.Generator().manual_seed(5))
    new = 6
    g32 = m32.generate(inputs=ids, max_new_tokens=new, do_sample=False, output_scores=True, return_dict_in_generate=True)
    mg = _phi3(layers=2, u2=True).to(dt).to(D)
    g = mg.generate(inputs=ids.to(D), max_new_tokens=new, do_sample=False).cpu()
    assert all(is_patched(lay) for lay in mg.model.layers)
    assert g.shape == g32.sequences.shape
    for t in range(new):
        top2 = g32.scores[t][0].topk(2).values
        if (top2[0] - top2[1]).item() > 0.05:
            assert g[0, t] == g32.sequences[0, t], (t, g, g32.sequences)
        else:
            break


class _LoraLikeLinear(torch.nn.Module):
    """peft's lora.Linear from outside: `.weight` / `.bias` are the BASE layer's, forward adds the adapter"""

    def __init__(self, base, rank=4):
        super().__init__()
        self.base_layer = base
        g = torch.Generator().manual_seed(3)
        self.lora_A = torch.nn.Parameter(0.05 * torch.randn(rank, base.in_features, generator=g).to(base.weight))
        self.lora_B = torch.nn.Parameter(0.05 * torch.randn(base.out_features, rank, generator=g).to(base.weight))

    weight = property(lambda self: self.base_layer.weight)
    bias = property(lambda self: self.base_layer.bias)

    def forward(self, x):
        return self.base_layer(x) + (x @ self.lora_A.t()) @ self.lora_B.t()


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", ["lora", "hook", "padded", "partial_rotary"])
def test_phi3_stock_fallbacks(ops, dt, case):
    """What the fused forward cannot compute takes the stock layers: logits identical to the unpatched model."""
    from u2tokenizer_amd.prefill import disable_fused_prefill, enable_fused_prefill
    mg = _phi3(layers=1, partial_rotary_factor=0.5 if case == "partial_rotary" else 1.0).to(dt).to(D)
    B, S = 2, 40
    xd = (0.5 * synth.synth_tensor("inputs_embeds", (B, S, 768), 9)).to(dt).to(D)
    kw = {}
    if case == "lora":
        att = mg.model.layers[0].self_attn
        att.qkv_proj = _LoraLikeLinear(att.qkv_proj).to(D)
    elif case == "hook":
        mg.model.layers[0].mlp.register_forward_hook(lambda m, a, out: None)
    elif case == "padded":
        mask = torch.ones((B, S), dtype=torch.int64, device=D)
        mask[1, :5] = 0
        kw["attention_mask"] = mask
    want = mg(inputs_embeds=xd, use_cache=True, **kw).logits
    n = enable_fused_prefill(mg, strict=False)
    assert n == (0 if case == "partial_rotary" else 1)
    got = mg(inputs_embeds=xd, use_cache=True, **kw).logits
    disable_fused_prefill(mg)
    assert torch.equal(got, want)
