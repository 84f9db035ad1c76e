"""GPU: the whole-stack decode step (opt-in, `enable_fused_prefill(model, stack_decode=True)`; u2tok_decoder_decode_stack): one
library call per token for the whole decoder stack.  The route is the per-layer route's arithmetic re-sequenced, so its test is BIT
EQUALITY with the per-layer route (itself gated against fp32 by the tests of the routes it re-sequences), step by step, on the
hidden state and on every layer's cache -- in both element builds, the three weight forms, 1 .. 17 sequences, a left-padded batch,
an attention window that the steps cross, unmerged adapters, with the norms as launches of their own and in the products' tails
(the tail norm by itself: tests/test_gpu_rows_norm.py).  Then `generate`, the calls that must keep the per-layer routes, and the
C entry's refusals, which must come before anything is launched.

Shapes: 3 layers, E = 256, I = 512, 4 / 2 heads of 64 (every dimension a multiple of 128: e2m1 qualifies); Phi-3: the packed layout,
E = 384, 4 heads of 96, sliding_window = 8."""
import copy
import ctypes as C

import pytest
import torch

from test_gpu_lora_infer import _wrapped
from u2tokenizer_amd import synth

pytestmark = pytest.mark.gpu
D = "cuda"
bf, f16 = torch.bfloat16, torch.float16
DTYPES, IDS = [bf, f16], ["bf16", "fp16"]
NL, S0, STEPS, WINDOW = 3, 11, 6, 8
_BASE = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


@pytest.fixture(params=[False, True], ids=["norm launches", "tail norms"])
def tail(request, monkeypatch):
    from u2tokenizer_amd import prefill
    monkeypatch.setattr(prefill, "STACK_TAIL_NORM", request.param)
    return request.param


def _build(kind):
    from transformers import (LlamaConfig, LlamaForCausalLM, Phi3Config, Phi3ForCausalLM, Qwen3Config, Qwen3ForCausalLM)
    common = dict(vocab_size=512, intermediate_size=512, num_hidden_layers=NL, max_position_embeddings=256, tie_word_embeddings=False,
                  pad_token_id=0, bos_token_id=1, eos_token_id=2)
    if kind == "phi3":
        m = Phi3ForCausalLM(Phi3Config(hidden_size=384, num_attention_heads=4, num_key_value_heads=4, sliding_window=WINDOW, **common))
    else:
        common.update(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64)
        m = Qwen3ForCausalLM(Qwen3Config(**common)) if kind == "qwen3" else LlamaForCausalLM(LlamaConfig(**common, rope_theta=500000.0))
    synth.fill_module_(m, seed=23, prefix="decoder.")
    return m.eval()


def _model(kind, dt, lora=False):
    """a fresh copy of the seeded model of `kind` in `dt` on the GPU (lora: an unmerged adapter on q and down)"""
    if kind not in _BASE:
        _BASE[kind] = _build(kind)
    m = copy.deepcopy(_BASE[kind]).to(dt).to(D)
    if lora:
        m = _wrapped(m, torch.float32 if dt is f16 else None, ("q_proj", "down_proj"))   # (lora.adapter_of: bf16 or fp32 adapters)
    return m


def _inputs(m, B, dt, pads=None):
    E = m.config.hidden_size
    x = (0.5 * synth.synth_tensor("inputs_embeds", (B, S0, E), 5)).to(dt).to(D)
    xs = (0.5 * synth.synth_tensor("inputs_embeds", (B, STEPS, E), 6)).to(dt).to(D)
    mask = None
    if pads is not None:
        mask = torch.ones(B, S0, dtype=torch.int64, device=D)
        for b, p in enumerate(pads):
            mask[b, :p] = 0
    return x, xs, mask


def _prefilled(m, x, mask):
    """a plain DynamicCache after the fused prefill of x (bare: every layer a DynamicLayer, which the prefill replaces by its
    append-in-place layer -- with a window too, where the cache `generate` builds holds sliding layers the route leaves alone)"""
    from transformers.cache_utils import DynamicCache
    cache = DynamicCache()
    m.model(inputs_embeds=x, attention_mask=mask, past_key_values=cache, use_cache=True)
    return cache


def _steps(m, xs, cache, mask, **kw):
    """STEPS decode steps through the decoder stack -> per step (last hidden state, [(keys, values) per layer])"""
    out = []
    for t in range(xs.shape[1]):
        if mask is not None:
            mask = torch.cat([mask, mask.new_ones(mask.shape[0], 1)], 1)
        r = m.model(inputs_embeds=xs[:, t:t + 1], attention_mask=mask, past_key_values=cache, use_cache=True, **kw)
        assert r.past_key_values is cache
        out.append((r.last_hidden_state.clone(), [(l.keys.clone(), l.values.clone()) for l in cache.layers]))
    return out


def _same(a, b, what):
    assert len(a) == len(b) == STEPS
    for t, ((ha, ca), (hb, cb)) in enumerate(zip(a, b)):
        assert ha.shape == hb.shape and torch.isfinite(ha.float()).all()
        assert torch.equal(ha, hb), (what, "hidden state", t, int((ha != hb).sum()))
        assert len(ca) == len(cb) == NL
        for i, ((ka, va), (kb, vb)) in enumerate(zip(ca, cb)):
            assert ka.shape == kb.shape and ka.shape[2] == S0 + t + 1
            assert torch.equal(ka, kb) and torch.equal(va, vb), (what, "cache of layer", i, t)


CASES = {
    # kind, B, switches, pads, lora
    "qwen3 B=1": ("qwen3", 1, {}, None, False),
    "llama B=1": ("llama", 1, {}, None, False),
    "phi3 B=1 window": ("phi3", 1, dict(continued=True), None, False),
    "qwen3 B=1 fp8": ("qwen3", 1, dict(fp8_decode=True), None, False),
    "qwen3 B=1 fp4": ("qwen3", 1, dict(fp4_decode=True), None, False),
    "llama B=3 fp8": ("llama", 3, dict(fp8_decode=True), None, False),
    "phi3 B=3 window fp4": ("phi3", 3, dict(continued=True, fp4_decode=True), None, False),
    "phi3 B=16 window fp8": ("phi3", 16, dict(continued=True, fp8_decode=True), None, False),
    "qwen3 B=3": ("qwen3", 3, {}, None, False),
    "qwen3 B=16": ("qwen3", 16, {}, None, False),
    "llama B=16 fp4": ("llama", 16, dict(fp4_decode=True), None, False),
    "qwen3 B=17 wide": ("qwen3", 17, dict(wide_decode=True), None, False),
    "qwen3 B=17 wide fp8": ("qwen3", 17, dict(wide_decode=True, fp8_decode=True), None, False),
    "llama B=17 wide fp4": ("llama", 17, dict(wide_decode=True, fp4_decode=True), None, False),
    "qwen3 B=3 left-padded": ("qwen3", 3, dict(padded=True), (0, 2, 5), False),
    "llama B=3 left-padded fp4": ("llama", 3, dict(padded=True, fp4_decode=True), (4, 0, 1), False),
    "qwen3 B=1 lora": ("qwen3", 1, dict(lora=True), None, True),
    "qwen3 B=3 lora fp8": ("qwen3", 3, dict(lora=True, fp8_decode=True), None, True),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_bit_equal_to_the_per_layer_route(ops, tail, dt, case):
    """Two copies of one seeded model, the same fused prefill of 11 positions, 6 decode steps through `model.model`: one copy with
    stack_decode, one without.  Every step: the same last hidden state and the same keys and values in every layer, bit for bit.
    The counters show that the whole-stack call ran (6 model calls, 6 x 3 layer steps) and in which form."""
    from u2tokenizer_amd import prefill
    kind, B, sw, pads, lora = CASES[case]
    base = _model(kind, dt, lora)
    ma, mb = base, copy.deepcopy(base)
    x, xs, mask = _inputs(ma, B, dt, pads)
    prefill.enable_fused_prefill(ma, stack_decode=True, **sw)
    prefill.enable_fused_prefill(mb, **sw)
    ca, cb = _prefilled(ma, x, mask), _prefilled(mb, x, mask)
    key = "padded_decode" if pads is not None else "decode"
    n0 = {n: dict(getattr(prefill, n)) for n in ("stack_stats", "stats", "w8_stats", "w4_stats", "wide_stats", "lora_stats")}
    got = _steps(ma, xs, ca, mask)
    assert prefill.stack_stats[key] - n0["stack_stats"][key] == STEPS, "the whole-stack step did not run"
    assert prefill.stats[key] - n0["stats"][key] == STEPS * NL
    assert prefill.w8_stats[key] - n0["w8_stats"][key] == (STEPS * NL if sw.get("fp8_decode") else 0)
    assert prefill.w4_stats[key] - n0["w4_stats"][key] == (STEPS * NL if sw.get("fp4_decode") else 0)
    assert prefill.wide_stats[key] - n0["wide_stats"][key] == (STEPS * NL if B > 16 else 0)
    assert prefill.lora_stats["decode"] - n0["lora_stats"]["decode"] == (STEPS * NL if lora else 0)
    n1 = dict(prefill.stack_stats)
    want = _steps(mb, xs, cb, mask)
    assert prefill.stack_stats == n1 and prefill.stats[key] - n0["stats"][key] == 2 * STEPS * NL
    _same(got, want, case)
    if kind == "phi3":
        assert got[-1][1][0][0].shape[2] == S0 + STEPS > WINDOW
    prefill.disable_fused_prefill(ma)
    prefill.disable_fused_prefill(mb)


@pytest.mark.parametrize("padded", [False, True], ids=["B=1", "left-padded B=2"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_generate_gives_the_per_layer_routes_ids(ops, tail, dt, padded):
    """Greedy `generate`, 12 new tokens: the ids of the per-layer route, and 11 whole-stack steps (the first token is the prefill's)."""
    from u2tokenizer_amd import prefill
    new = 12
    g = torch.Generator().manual_seed(3)
    B = 2 if padded else 1
    ids = torch.randint(3, 512, (B, 9), generator=g).to(D)
    mask = torch.ones_like(ids)
    if padded:
        ids[1, :4], mask[1, :4] = 0, 0
    kw = dict(max_new_tokens=new, min_new_tokens=new, do_sample=False, pad_token_id=0, attention_mask=mask)
    m = _model("qwen3", dt)
    prefill.enable_fused_prefill(m, padded=padded)
    want = m.generate(input_ids=ids, **kw)
    prefill.enable_fused_prefill(m, padded=padded, stack_decode=True)
    n0 = dict(prefill.stack_stats)
    got = m.generate(input_ids=ids, **kw)
    prefill.disable_fused_prefill(m)
    key, other = ("padded_decode", "decode") if padded else ("decode", "padded_decode")
    assert prefill.stack_stats[key] - n0[key] == new - 1 and prefill.stack_stats[other] == n0[other]
    assert got.shape == (B, 9 + new) and torch.equal(got, want)


def _unpatch(m, i):
    layer = m.model.layers[i]
    layer.forward = layer.__dict__.pop("_u2_prefill").orig


def _plain_layer(cache, i):
    from transformers.cache_utils import DynamicLayer
    old = cache.layers[i]
    lay = DynamicLayer()
    lay.update(old.keys.clone(), old.values.clone())
    cache.layers[i] = lay


@pytest.mark.parametrize("why", ["a forward hook on one layer", "output_hidden_states", "a plain DynamicLayer in the cache",
                                 "one unpatched layer", "the switch off"])
def test_calls_that_keep_the_per_layer_routes(ops, why):
    """Each of these goes to the stack's own forward and the per-layer routes: the bits of a model that never had the switch, and
    no whole-stack step counted."""
    from u2tokenizer_amd import prefill
    ma = _model("qwen3", bf)
    mb = copy.deepcopy(ma)
    x, xs, mask = _inputs(ma, 2, bf)
    prefill.enable_fused_prefill(ma, stack_decode=True)
    prefill.enable_fused_prefill(mb)
    ca, cb = _prefilled(ma, x, mask), _prefilled(mb, x, mask)
    kw = {}
    for m, c in ((ma, ca), (mb, cb)):
        if why.startswith("a forward hook"):
            m.model.layers[1].register_forward_hook(lambda *a: None)
        elif why == "output_hidden_states":
            kw = dict(output_hidden_states=True)
        elif why.startswith("a plain DynamicLayer"):
            _plain_layer(c, 1)
        elif why == "one unpatched layer":
            _unpatch(m, 1)
    if why == "the switch off":
        assert "_u2_stack_run" in ma.model.__dict__
        prefill.enable_fused_prefill(ma)
        assert "_u2_stack_run" not in ma.model.__dict__ and "forward" not in ma.model.__dict__
    n0, d0 = dict(prefill.stack_stats), prefill.stats["decode"]
    got = _steps(ma, xs, ca, mask, **kw)
    assert prefill.stack_stats == n0, why
    # the layers that keep the fused step (a hook on the layer module fires around it; the recorders of output_hidden_states
    # send every layer to its stock forward)
    fused = {"one unpatched layer": NL - 1, "output_hidden_states": 0}.get(why, NL)
    assert prefill.stats["decode"] - d0 == STEPS * fused
    _same(got, _steps(mb, xs, cb, mask, **kw), why)
    prefill.disable_fused_prefill(ma)
    prefill.disable_fused_prefill(mb)


def test_every_refusal_comes_before_the_first_launch(ops):
    """u2tok_decoder_decode_stack called directly on the descriptors of a step the route has taken: with layer 2's Wdown null, with
    a short workspace, with no layers.  Each returns its error code, and the row of layer 0's cache buffers the step would write, the
    hidden rows of the workspace and `out` keep their sentinel: layers 0 and 1 were not run ahead of the refusal."""
    from u2tokenizer_amd import _lib, prefill
    m = _model("qwen3", bf)
    B = 2
    x, xs, mask = _inputs(m, B, bf)
    prefill.enable_fused_prefill(m, stack_decode=True)
    cache = _prefilled(m, x, mask)
    m.model(inputs_embeds=xs[:, :1], past_key_values=cache, use_cache=True)       # (builds the descriptors)
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
    pos = torch.full((1, 1), T0, device=D)
    cos, sin = m.model.rotary_emb(x2[:, None], pos)
    cos, sin = cos.expand(B, 1, 64).reshape(B, 64).float().contiguous(), sin.expand(B, 1, 64).reshape(B, 64).float().contiguous()
    out = torch.full((B, E), 7.0, dtype=bf, device=D)
    with ops.on_device(x2) as (h, stream):
        need = h.u2tok_decoder_decode_stack_workspace_bytes(arr, NL)
        assert need > 0
        ws = torch.zeros(need, dtype=torch.uint8, device=D)
        ws[256:].fill_(0x55)

        wf = m.model.norm.weight.data_ptr()

        def call(layers, n, nbytes, final=wf, tail=1, o=out):
            return h.u2tok_decoder_decode_stack(layers, n, x2.data_ptr(), cos.data_ptr(), sin.data_ptr(), 1, 64, 0, None, final, 1e-6,
                                                tail, o.data_ptr(), ws.data_ptr(), nbytes, stream)

        def untouched():
            torch.cuda.synchronize()
            return bool((l0._kb[:, :, T0] == 7).all() and (l0._vb[:, :, T0] == 7).all() and (out == 7).all()
                        and (ws[256:] == 0x55).all() and not ws[:256].any())

        bad = _lib.DecodeLayer.from_buffer_copy(keep[2][0])
        bad.Wdown = None
        good = arr[2].layer
        arr[2].layer = C.addressof(bad)
        assert call(arr, NL, need) == -1 and untouched()            # U2TOK_ERR_ARG from the last layer's second half
        arr[2].layer = good
        assert call(arr, NL, need - 1) == -3 and untouched()        # U2TOK_ERR_WORKSPACE
        assert call(arr, 0, need) == -1 and call(None, NL, need) == -1 and untouched()
        arr[1].kv_stride = arr[1].s_off * 64                        # a cache entry without room for the step's row
        assert call(arr, NL, need) == -1 and untouched()
        arr[1].kv_stride = cache.layers[1]._kb.stride(1)
        # ... and the descriptors were good: the call runs, writes the row and `out`.  The final norm -- in the tail of the last down
        # product, or as a launch -- is the library's RMSNorm of the hidden state the call hands out without one
        assert call(arr, NL, need) == 0
        torch.cuda.synchronize()
        assert not (l0._kb[:, :, T0] == 7).all() and not (out == 7).any() and not ws[:4].any()
        raw, out0 = torch.empty_like(out), torch.empty_like(out)
        assert call(arr, NL, need, final=None, tail=0, o=raw) == 0 and call(arr, NL, need, tail=0, o=out0) == 0
    normed = ops.rmsnorm(raw, m.model.norm.weight, 1e-6)
    assert torch.equal(out, normed) and torch.equal(out0, normed) and not torch.equal(raw, normed)
    # the route's own step from the same state: the same hidden state, under the module's norm
    want = m.model(inputs_embeds=xs[:, 1:2], past_key_values=cache, use_cache=True).last_hidden_state
    assert torch.equal(m.model.norm(raw[:, None]), want)
    prefill.disable_fused_prefill(m)


@pytest.mark.parametrize("entry", ["per sequence", "batched", "kv8"])
def test_a_per_layer_refusal_comes_before_the_first_launch(ops, entry):
    """u2tok_decoder_decode_post / _post_kv8 called directly (B = 2, E = 256, 4 / 2 heads of 64, I = 512, T = 18) with a 16-bit Wdown
    8 bytes off alignment -- an in-bounds offset into a real allocation, every other buffer real too, so a call that were accepted
    could not fault.  Only the down product's own check sees it, the last launch of the half: the call returns U2TOK_ERR_ARG and `out`,
    the whole workspace and (kv8) the code and scale buffers keep every sentinel byte -- neither the attention nor a product before
    the refusal was launched."""
    from u2tokenizer_amd import _lib
    B, E, Hq, Hkv, Dh, I, T, CAP = 2, 256, 4, 2, 64, 512, 18, 32
    nq = (Hq + 2 * Hkv) * Dh

    def z(*shape):
        return torch.zeros(*shape, dtype=bf, device=D)

    x, qkv, K, V = z(B, E), z(B, nq), z(B, Hkv, T, Dh), z(B, Hkv, T, Dh)
    Wo, post, Wgu, Wdown = z(E, Hq * Dh), z(E), z(2 * I, E), z(E * I + 8)
    cfg = _lib.DecodeConfig(B=B, E=E, Hq=Hq, Hkv=Hkv, D=Dh, I=I, eps=1e-6, qk_eps=1e-6, scale=Dh ** -0.5, wform=0)
    lay = _lib.DecodeLayer(Wo=Wo.data_ptr(), w_post_norm=post.data_ptr(), Wgu=Wgu.data_ptr(), Wdown=Wdown.data_ptr() + 8)
    assert Wdown.data_ptr() % 16 == 0
    out = torch.full((B, E), 7.0, dtype=bf, device=D)
    k_new, v_new = z(B, Hkv, 1, Dh), z(B, Hkv, 1, Dh)
    codes = [torch.full((B, Hkv, CAP, Dh), 0x55, dtype=torch.uint8, device=D) for _ in range(2)]
    scales = [torch.full((B, Hkv, CAP), 7.0, dtype=torch.float32, device=D) for _ in range(2)]
    with ops.on_device(x) as (h, stream):
        need = h.u2tok_decoder_decode_workspace_bytes(C.byref(cfg), T)
        assert need > 0
        ws = torch.full((need,), 0x55, dtype=torch.uint8, device=D)
        if entry == "kv8":
            st = h.u2tok_decoder_decode_post_kv8(C.byref(cfg), C.byref(lay), x.data_ptr(), qkv.data_ptr(), k_new.data_ptr(), v_new.data_ptr(),
                                                 codes[0].data_ptr(), codes[1].data_ptr(), scales[0].data_ptr(), scales[1].data_ptr(), CAP, 0,
                                                 T - 1, None, out.data_ptr(), ws.data_ptr(), need, stream)
        else:
            st = h.u2tok_decoder_decode_post(C.byref(cfg), C.byref(lay), x.data_ptr(), qkv.data_ptr(), K.data_ptr(), V.data_ptr(), T, 0,
                                             int(entry == "batched"), None, out.data_ptr(), ws.data_ptr(), need, stream)
        torch.cuda.synchronize()
    assert st == -1                                                   # U2TOK_ERR_ARG
    assert bool((out == 7).all()) and bool((ws == 0x55).all())
    assert all(bool((c == 0x55).all()) for c in codes) and all(bool((s == 7).all()) for s in scales)
