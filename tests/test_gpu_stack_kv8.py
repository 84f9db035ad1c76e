"""GPU: the whole-stack decode step on the FP8 (e4m3) KV cache (opt-in, `enable_fused_prefill(model, stack_kv8=True)`;
u2tok_decoder_decode_stack_kv8 / u2tok_decoder_decode_stack_head_kv8): one library call per token on a cache of `Kv8Layer`s, the
step's rows appended as codes by the rotary kernel.  The route is the per-layer kv8 route's arithmetic re-sequenced, with the
quantiser folded into another launch, so its test is BIT EQUALITY with that route -- step by step, on the hidden state and on every
layer's codes and scales -- in both element builds, the three weight forms, 1 .. 17 sequences, a left-padded batch, a window the
steps cross, an unmerged adapter, with the norms as launches of their own and in the products' tails.  Then the head, `generate`,
the calls that must keep the per-layer routes, and the C entries' refusals, which must come before anything is launched.

Models and shapes: those of tests/test_gpu_stack_decode.py (3 layers, E = 256, I = 512, 4 / 2 heads of 64; Phi-3: E = 384, 4 heads of
96, sliding_window = 8)."""
import copy
import ctypes as C

import pytest
import torch

from test_gpu_stack_decode import NL, S0, STEPS, WINDOW, _inputs, _model, _prefilled
from u2tokenizer_amd import synth

pytestmark = pytest.mark.gpu
D = "cuda"
bf, f16 = torch.bfloat16, torch.float16
DTYPES, IDS = [bf, f16], ["bf16", "fp16"]
VOCAB = 512
COUNTERS = ("stack_kv8_stats", "stack_stats", "kv8_stats", "stats", "w8_stats", "w4_stats", "wide_stats", "lora_stats", "head_stats")
_U2 = {}


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


def _counts():
    from u2tokenizer_amd import prefill
    return {n: dict(getattr(prefill, n)) for n in COUNTERS}


def _codes(cache):
    """every layer's (K codes, V codes, K scales, V scales) up to the layer's length, cloned"""
    from u2tokenizer_amd import prefill
    out = []
    for lay in cache.layers:
        assert type(lay) is prefill.Kv8Layer
        out.append(tuple(t.clone() for t in lay.codes()))
    return out


def _steps(m, xs, cache, mask, **kw):
    """STEPS decode steps through the decoder stack -> per step (last hidden state, the layers' codes and scales)"""
    out = []
    for t in range(xs.shape[1]):
        if mask is not None:
            mask = torch.cat([mask, mask.new_ones(mask.shape[0], 1)], 1)
        r = m.model(inputs_embeds=xs[:, t:t + 1], attention_mask=mask, past_key_values=cache, use_cache=True, **kw)
        assert r.past_key_values is cache
        out.append((r.last_hidden_state.clone(), _codes(cache)))
    return out


def _same(a, b, what):
    assert len(a) == len(b) == STEPS
    for t, ((ha, ca), (hb, cb)) in enumerate(zip(a, b)):
        assert ha.shape == hb.shape and torch.isfinite(ha.float()).all()
        assert torch.equal(ha, hb), (what, "hidden state", t, int((ha != hb).sum()))
        assert len(ca) == len(cb) == NL
        for i, (la, lb) in enumerate(zip(ca, cb)):
            assert la[0].shape == lb[0].shape and la[0].shape[2] == S0 + t + 1 and la[2].shape[2] == S0 + t + 1
            for name, x, y in zip(("k codes", "v codes", "k scales", "v scales"), la, lb):
                if x.dtype == torch.float32:
                    x, y = x.view(torch.int32), y.view(torch.int32)
                assert torch.equal(x, y), (what, name, "layer", i, "step", t)


CASES = {
    # kind, B, switches, pads, lora
    "qwen3 B=1": ("qwen3", 1, {}, None, False),
    "llama B=1": ("llama", 1, {}, None, False),
    "phi3 B=1 window": ("phi3", 1, dict(continued=True), None, False),
    "qwen3 B=1 fp8": ("qwen3", 1, dict(fp8_decode=True), None, False),
    "qwen3 B=1 fp4": ("qwen3", 1, dict(fp4_decode=True), None, False),
    "llama B=3 fp8": ("llama", 3, dict(fp8_decode=True), None, False),
    "qwen3 B=16": ("qwen3", 16, {}, None, False),
    "qwen3 B=17 wide": ("qwen3", 17, dict(wide_decode=True), None, False),
    "qwen3 B=3 left-padded": ("qwen3", 3, dict(padded=True), (0, 2, 5), False),
    "qwen3 B=1 lora": ("qwen3", 1, dict(lora=True), None, True),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_bit_equal_to_the_per_layer_kv8_route(ops, tail, dt, case):
    """Two copies of one seeded model, the same fused prefill of 11 positions onto an FP8 cache, 6 decode steps through `model.model`:
    one copy with stack_kv8, one with kv8 alone.  Every step: the same last hidden state and the same codes and scales in every
    layer, bit for bit.  The counters show that the whole-stack call on codes ran (6 model calls, 6 x 3 layer steps) and in which
    form; the per-layer copy counts no whole-stack call."""
    from u2tokenizer_amd import prefill
    kind, B, sw, pads, lora = CASES[case]
    base = _model(kind, dt, lora)
    ma, mb = base, copy.deepcopy(base)
    x, xs, mask = _inputs(ma, B, dt, pads)
    prefill.enable_fused_prefill(ma, stack_kv8=True, **sw)
    prefill.enable_fused_prefill(mb, kv8=True, **sw)
    ca, cb = _prefilled(ma, x, mask), _prefilled(mb, x, mask)
    assert all(type(l) is prefill.Kv8Layer and l.get_seq_length() == S0 for c in (ca, cb) for l in c.layers)
    key = "padded_decode" if pads is not None else "decode"
    n0 = _counts()
    got = _steps(ma, xs, ca, mask)
    n1 = _counts()

    def moved(name, k=key):
        return n1[name][k] - n0[name][k]

    assert moved("stack_kv8_stats") == STEPS, "the whole-stack step on the codes did not run"
    assert moved("stack_stats") == STEPS
    assert moved("kv8_stats") == STEPS * NL and moved("stats") == STEPS * NL
    assert moved("w8_stats") == (STEPS * NL if sw.get("fp8_decode") else 0)
    assert moved("w4_stats") == (STEPS * NL if sw.get("fp4_decode") else 0)
    assert moved("wide_stats") == (STEPS * NL if B > 16 else 0)
    assert moved("lora_stats", "decode") == (STEPS * NL if lora else 0)
    want = _steps(mb, xs, cb, mask)
    n2 = _counts()
    assert n2["stack_stats"] == n1["stack_stats"] and n2["stack_kv8_stats"] == n1["stack_kv8_stats"]
    assert n2["kv8_stats"][key] - n1["kv8_stats"][key] == STEPS * NL and n2["stats"][key] - n1["stats"][key] == STEPS * NL
    _same(got, want, case)
    if kind == "phi3":
        assert got[-1][1][0][0].shape[2] == S0 + STEPS > WINDOW
    prefill.disable_fused_prefill(ma)
    prefill.disable_fused_prefill(mb)


# ------------------------------------------------------------------------------------------------------------------- the head
def _u2(dt, **cfg):
    """a u2Qwen3ForCausalLM of the shapes above, V = 512, with the config attributes `cfg`"""
    from u2tokenizer_amd import language_model as LM
    if "m" not in _U2:
        c = LM.u2Qwen3Config(vocab_size=VOCAB, hidden_size=256, intermediate_size=512, num_hidden_layers=NL, num_attention_heads=4,
                             num_key_value_heads=2, head_dim=64, max_position_embeddings=256, tie_word_embeddings=False,
                             pad_token_id=0, bos_token_id=1, eos_token_id=2)
        m = LM.u2Qwen3ForCausalLM(c)
        synth.fill_module_(m, seed=23, prefix="decoder.")
        _U2["m"] = m.eval()
    m = copy.deepcopy(_U2["m"]).to(dt).to(D)
    for k, v in cfg.items():
        setattr(m.config, k, v)
    return m


def _lm_prefilled(m, x):
    from transformers.cache_utils import DynamicCache
    cache = DynamicCache()
    m(inputs_embeds=x, past_key_values=cache, use_cache=True)
    return cache


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_logits_are_the_head_entry_on_the_per_layer_routes_hidden_rows(ops, tail, dt, B):
    """`model(...).logits` of the step with the head on the codes, (B, 1, V) fp32, against u2tok_decode_head applied to the un-normed
    last hidden rows of the per-layer kv8 route (a copy whose stack norm is the identity); codes and scales equal at every step."""
    from u2tokenizer_amd import prefill
    ma = _u2(dt, u2_fused_stack_kv_fp8=True, u2_fused_decode_head=True)
    mb = _u2(dt, u2_fused_kv_fp8=True)
    mb.model.norm = torch.nn.Identity()
    x, xs, _ = _inputs(ma, B, dt)
    ca, cb = _lm_prefilled(ma, x), _lm_prefilled(mb, x)
    sa, sb = ma.model._u2_stack, mb.model._u2_stack
    assert sa.stack8 and sa.stack and sa.kv8 and sa.head and sb.kv8 and not sb.stack and not sb.stack8
    nw, eps, w = ma.model.norm.weight, ma.model.norm.variance_epsilon, ma.lm_head.weight
    n0 = _counts()
    for t in range(STEPS):
        out = ma(inputs_embeds=xs[:, t:t + 1], past_key_values=ca, use_cache=True)
        raw = mb.model(inputs_embeds=xs[:, t:t + 1], past_key_values=cb, use_cache=True).last_hidden_state[:, 0]
        assert out.logits.shape == (B, 1, VOCAB) and out.logits.dtype == torch.float32 and out.past_key_values is ca
        assert torch.isfinite(out.logits).all()
        want = ops.decode_head(raw, nw, eps, w)
        assert torch.equal(out.logits[:, 0], want), (t, int((out.logits[:, 0] != want).sum()))
        for i, (la, lb) in enumerate(zip(_codes(ca), _codes(cb))):
            assert la[0].shape[2] == S0 + t + 1 and all(torch.equal(p, q) for p, q in zip(la, lb)), (t, i)
    n1 = _counts()
    assert n1["head_stats"] == {**n0["head_stats"], "head": n0["head_stats"]["head"] + STEPS}
    assert n1["stack_kv8_stats"]["decode"] - n0["stack_kv8_stats"]["decode"] == STEPS
    assert n1["stack_stats"]["decode"] - n0["stack_stats"]["decode"] == STEPS
    assert n1["kv8_stats"]["decode"] - n0["kv8_stats"]["decode"] == 2 * STEPS * NL
    prefill.disable_fused_prefill(ma)
    prefill.disable_fused_prefill(mb)


# ------------------------------------------------------------------------------------------------------------------- generate
@pytest.mark.parametrize("padded", [False, True], ids=["B=1", "left-padded B=2"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_generate_gives_the_per_layer_kv8_routes_ids(ops, tail, dt, padded):
    """Greedy `generate`, 8 new tokens: the ids of the per-layer kv8 route, and 7 whole-stack steps on the codes."""
    from u2tokenizer_amd import prefill
    new = 8
    g = torch.Generator().manual_seed(3)
    B = 2 if padded else 1
    ids = torch.randint(3, 512, (B, 9), generator=g).to(D)
    mask = torch.ones_like(ids)
    if padded:
        ids[1, :4], mask[1, :4] = 0, 0
    kw = dict(max_new_tokens=new, min_new_tokens=new, do_sample=False, pad_token_id=0, attention_mask=mask)
    m = _model("qwen3", dt)
    prefill.enable_fused_prefill(m, padded=padded, kv8=True)
    k0 = dict(prefill.kv8_stats)
    want = m.generate(input_ids=ids, **kw)
    key, other = ("padded_decode", "decode") if padded else ("decode", "padded_decode")
    assert prefill.kv8_stats[key] - k0[key] == (new - 1) * NL          # (the reference ran on the codes, layer by layer)
    prefill.enable_fused_prefill(m, padded=padded, stack_kv8=True)
    n0 = _counts()
    got = m.generate(input_ids=ids, **kw)
    n1 = _counts()
    prefill.disable_fused_prefill(m)
    for name in ("stack_kv8_stats", "stack_stats"):
        assert n1[name][key] - n0[name][key] == new - 1 and n1[name][other] == n0[name][other], name
    assert n1["kv8_stats"][key] - n0["kv8_stats"][key] == (new - 1) * NL
    assert got.shape == (B, 9 + new) and torch.equal(got, want)


# ------------------------------------------------------------------------------------- calls that keep the per-layer routes
def _append_layer(cache, i):
    """layer i of the cache as the append-in-place layer, holding the dequantised rows"""
    from u2tokenizer_amd import prefill
    old = cache.layers[i]
    lay = prefill._append_layer_class()()
    lay.update(old.keys.clone(), old.values.clone())
    cache.layers[i] = lay


@pytest.mark.parametrize("why", ["a mixed cache", "a forward hook on one layer", "output_hidden_states"])
def test_calls_that_keep_the_per_layer_routes(ops, why):
    """Each of these goes to the stack's own forward and the per-layer routes: the bits of a model that has kv8 alone, and no
    whole-stack step counted."""
    from u2tokenizer_amd import prefill
    ma = _model("qwen3", bf)
    mb = copy.deepcopy(ma)
    x, xs, mask = _inputs(ma, 2, bf)
    prefill.enable_fused_prefill(ma, stack_kv8=True)
    prefill.enable_fused_prefill(mb, kv8=True)
    ca, cb = _prefilled(ma, x, mask), _prefilled(mb, x, mask)
    kw = {}
    for m, c in ((ma, ca), (mb, cb)):
        if why == "a mixed cache":
            _append_layer(c, 1)
        elif why.startswith("a forward hook"):
            m.model.layers[1].register_forward_hook(lambda *a: None)
        else:
            kw = dict(output_hidden_states=True)
    n0 = _counts()

    def run(m, c):
        out = []
        for t in range(STEPS):
            r = m.model(inputs_embeds=xs[:, t:t + 1], past_key_values=c, use_cache=True, **kw)
            lays = [tuple(p.clone() for p in (l.codes() if type(l) is prefill.Kv8Layer else (l.keys, l.values))) for l in c.layers]
            out.append((r.last_hidden_state.clone(), lays))
        return out

    got = run(ma, ca)
    n1 = _counts()
    assert n1["stack_stats"] == n0["stack_stats"] and n1["stack_kv8_stats"] == n0["stack_kv8_stats"], why
    # the layers that keep the fused step on the codes (the recorders of output_hidden_states send every layer to its stock forward)
    fused, on_codes = {"a mixed cache": (NL, NL - 1), "output_hidden_states": (0, 0)}.get(why, (NL, NL))
    assert n1["stats"]["decode"] - n0["stats"]["decode"] == STEPS * fused
    assert n1["kv8_stats"]["decode"] - n0["kv8_stats"]["decode"] == STEPS * on_codes
    want = run(mb, cb)
    for t, ((ha, la), (hb, lb)) in enumerate(zip(got, want)):
        assert torch.equal(ha, hb), (why, "hidden state", t)
        assert all(torch.equal(p, q) for a, b in zip(la, lb) for p, q in zip(a, b)), (why, "cache", t)
    prefill.disable_fused_prefill(ma)
    prefill.disable_fused_prefill(mb)


# ----------------------------------------------------------------------------------------------------- refusal before launch
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_every_refusal_comes_before_the_first_launch(ops, dt):
    """u2tok_decoder_decode_stack_kv8 and _stack_head_kv8 called directly on the descriptors of layers 0 and 1 of a step the route has
    taken, with layer 1 malformed: a null scale pointer (the rotary kernel's and the attention's refusal), a 16-bit Wo 8 bytes off
    alignment (the o product's, in the second half).  Each returns U2TOK_ERR_ARG, and layer 0's code and scale rows at s_off, the
    workspace, `out` and the logits keep their sentinels: layer 0 was not run ahead of the refusal.  The good descriptors then run."""
    from u2tokenizer_amd import _lib, prefill
    m = _model("qwen3", dt)
    B, n = 2, 2
    x, xs, mask = _inputs(m, B, dt)
    prefill.enable_fused_prefill(m, stack_kv8=True)
    cache = _prefilled(m, x, mask)
    m.model(inputs_embeds=xs[:, :1], past_key_values=cache, use_cache=True)       # (builds the descriptors)
    E, Hkv = m.config.hidden_size, m.config.num_key_value_heads
    arr = (_lib.DecodeStackLayerKv8 * n)()
    keep = []
    for i in range(n):
        lay, _, _, cfg = m.model.layers[i]._u2_prefill.variants[(0, False)]
        cl = cache.layers[i]
        T0 = cl._room(1, torch.empty(B, Hkv, 1, 64, device=x.device))
        s = arr[i]
        s.cfg, s.layer = C.addressof(cfg), C.addressof(lay)
        s.k_codes, s.v_codes, s.k_scales, s.v_scales = (t.data_ptr() for t in (cl._kc, cl._vc, cl._ks, cl._vs))
        s.capacity, s.s_off, s.k_first, s.T = cl._kc.shape[2], T0, 0, T0 + 1
        keep.append((lay, cfg))
    l0 = cache.layers[0]
    T0 = arr[0].s_off
    l0._kc[:, :, T0].fill_(0x55), l0._vc[:, :, T0].fill_(0x55), l0._ks[:, :, T0].fill_(7.0), l0._vs[:, :, T0].fill_(7.0)
    x2 = xs[:, 1].contiguous()
    pos = torch.full((1, 1), T0, device=D)
    cos, sin = m.model.rotary_emb(x2[:, None], pos)
    cos, sin = cos.expand(B, 1, 64).reshape(B, 64).float().contiguous(), sin.expand(B, 1, 64).reshape(B, 64).float().contiguous()
    out = torch.full((B, E), 7.0, dtype=dt, device=D)
    logits = torch.full((B, VOCAB), 7.0, dtype=torch.float32, device=D)
    head = ops.head_desc(m.model.norm.weight.detach(), m.model.norm.variance_epsilon, m.lm_head.weight.detach())
    with ops.on_device(x2) as (h, stream):
        need = h.u2tok_decoder_decode_stack_kv8_workspace_bytes(arr, n)
        hneed = h.u2tok_decoder_decode_stack_head_kv8_workspace_bytes(arr, n, C.byref(head))
        assert 0 < need < hneed
        ws = torch.zeros(hneed, dtype=torch.uint8, device=D)
        ws[256:].fill_(0x55)

        def stack(tail):
            return h.u2tok_decoder_decode_stack_kv8(arr, n, x2.data_ptr(), cos.data_ptr(), sin.data_ptr(), 1, 64, None, None, 0.0, tail,
                                                    out.data_ptr(), ws.data_ptr(), need, stream)

        def joint(tail):
            return h.u2tok_decoder_decode_stack_head_kv8(arr, n, x2.data_ptr(), cos.data_ptr(), sin.data_ptr(), 1, 64, None, tail,
                                                         out.data_ptr(), C.byref(head), logits.data_ptr(), VOCAB, ws.data_ptr(), hneed, stream)

        def untouched():
            torch.cuda.synchronize()
            return bool((l0._kc[:, :, T0] == 0x55).all() and (l0._vc[:, :, T0] == 0x55).all() and (l0._ks[:, :, T0] == 7).all()
                        and (l0._vs[:, :, T0] == 7).all() and (out == 7).all() and (logits == 7).all() and (ws[256:] == 0x55).all()
                        and not ws[:256].any())

        good = arr[1].k_scales
        arr[1].k_scales = None
        for tail in (0, 1):
            assert stack(tail) == -1 and untouched() and joint(tail) == -1 and untouched()      # U2TOK_ERR_ARG
        arr[1].k_scales = good
        bad = _lib.DecodeLayer.from_buffer_copy(keep[1][0])
        bad.Wo = keep[1][0].Wo + 8
        good = arr[1].layer
        arr[1].layer = C.addressof(bad)
        for tail in (0, 1):
            assert stack(tail) == -1 and untouched() and joint(tail) == -1 and untouched()
        arr[1].layer = good
        arr[1].capacity = arr[1].s_off                                                          # s_off == capacity
        assert stack(0) == -1 and untouched() and joint(0) == -1 and untouched()
        arr[1].capacity = cache.layers[1]._kc.shape[2]
        # ... and the descriptors were good: the calls run and write the rows, `out` and the logits
        assert stack(1) == 0
        torch.cuda.synchronize()
        assert not (l0._kc[:, :, T0] == 0x55).all() and not (l0._ks[:, :, T0] == 7).any() and not (out == 7).any() and not ws[:4].any()
        first = (out.clone(), l0._kc[:, :, T0].clone(), l0._ks[:, :, T0].clone())
        assert joint(0) == 0
        torch.cuda.synchronize()
        assert not (logits == 7).any() and not ws[:4].any()
    assert torch.equal(out, first[0]) and torch.equal(l0._kc[:, :, T0], first[1]) and torch.equal(l0._ks[:, :, T0], first[2])
    assert torch.equal(logits, ops.decode_head(out, m.model.norm.weight, m.model.norm.variance_epsilon, m.lm_head.weight))
    prefill.disable_fused_prefill(m)
