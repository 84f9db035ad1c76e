"""CPU: padded batches on the fused inference routes (opt-in, `enable_fused_prefill(model, padded=True)`) -- the mask rule
`prefill.pad_rule` on every kind of 2-D mask, and the route table of a patched layer with the switch on and off, in the style of
tests/test_decoder_route_host.py (whose small fixtures are copied here): the input is a CPU tensor that reports `is_cuda`, and
every route ends in a recorder before it would launch anything."""
import contextlib
import types

import pytest
import torch

from u2tokenizer_amd import decoder_train, ops, prefill

bf = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------- pad_rule
def _check(got, kind, start=None, length=None):
    assert got is not None and got[0] == kind
    for t, want in ((got[1], start), (got[2], length)):
        if want is None:
            assert t is None
        else:
            assert t.dtype == torch.int32 and t.shape == (len(want),) and t.tolist() == list(want)


def test_pad_rule_without_padding():
    assert prefill.pad_rule(None) == ("none", None, None)
    assert prefill.pad_rule(torch.ones(3, 7, dtype=torch.int64)) == ("none", None, None)
    assert prefill.pad_rule(torch.ones(1, 1, dtype=torch.bool)) == ("none", None, None)


@pytest.mark.parametrize("dtype", [torch.int64, torch.bool, torch.float32])
def test_pad_rule_right_and_left(dtype):
    right = torch.tensor([[1, 1, 1, 1, 1], [1, 1, 0, 0, 0], [1, 0, 0, 0, 0]]).to(dtype)
    _check(prefill.pad_rule(right), "right", length=(5, 2, 1))
    left = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 0, 1]]).to(dtype)
    _check(prefill.pad_rule(left), "left", start=(0, 3, 4))
    assert prefill.pad_rule(left)[1].device == left.device


@pytest.mark.parametrize("name,mask", [
    ("hole", [[1, 1, 1, 1], [1, 0, 1, 1]]),
    ("hole in a left-padded row", [[1, 1, 1, 1], [0, 1, 0, 1]]),
    ("empty row", [[1, 1, 1, 1], [0, 0, 0, 0]]),
    ("both sides", [[1, 1, 1, 1], [0, 1, 1, 0]]),
    ("left and right rows mixed", [[0, 1, 1, 1], [1, 1, 1, 0]]),
])
def test_pad_rule_sends_everything_else_to_the_stock_layers(name, mask):
    assert prefill.pad_rule(torch.tensor(mask)) is None


def test_pad_rule_needs_a_2d_tensor():
    assert prefill.pad_rule(torch.ones(2, 1, 4, 4, dtype=torch.bool)) is None
    assert prefill.pad_rule(torch.ones(2, 4, 4)) is None
    assert prefill.pad_rule(torch.ones(4)) is None
    assert prefill.pad_rule({"full_attention": torch.ones(2, 4)}) is None


def test_stats_has_the_four_routes():
    assert set(prefill.stats) == {"prefill", "decode", "padded_prefill", "padded_decode"}


# ---------------------------------------------------------------------------------------------------------- route table
class _FakeCuda(torch.Tensor):
    @property
    def is_cuda(self):
        return True


class _Routed(Exception):
    pass


def _model(kind="qwen3", dtype=bf, head_dim=64, hidden=128, inter=256, window=None, **kw):
    from transformers import (LlamaConfig, LlamaForCausalLM, Phi3Config, Phi3ForCausalLM, Qwen3Config,
                              Qwen3ForCausalLM)
    c = dict(vocab_size=64, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=1, max_position_embeddings=256)
    if kind == "phi3":
        c.update(num_attention_heads=hidden // head_dim, num_key_value_heads=hidden // head_dim, sliding_window=window,
                 pad_token_id=0, bos_token_id=1, eos_token_id=2)
        cfg, cls = Phi3Config, Phi3ForCausalLM
    else:
        c.update(num_attention_heads=2, num_key_value_heads=1, head_dim=head_dim)
        cfg, cls = (Qwen3Config, Qwen3ForCausalLM) if kind == "qwen3" else (LlamaConfig, LlamaForCausalLM)
    c.update(kw)
    torch.manual_seed(0)
    return cls(cfg(**c)).to(dtype).eval()


def _stock(self, hidden_states, *args, past_key_values=None, position_embeddings=None, **kwargs) -> torch.Tensor:
    self._calls.append("stock")
    return hidden_states


@pytest.fixture
def recorder(monkeypatch):
    calls = []

    def decode(layer, x, pe, cache, window=None, pr=None):
        calls.append(("decode", window))
        return x

    def first_prefill_kernel(*args, **kwargs):
        raise _Routed

    monkeypatch.setattr(prefill, "_decode_step", decode)
    monkeypatch.setattr(prefill, "_ensure_gemm_scratch", lambda device: None)
    monkeypatch.setattr(decoder_train, "layer_forward_train", lambda *a, **k: calls.append("train"))
    monkeypatch.setattr(ops, "on_device", lambda *a, **k: contextlib.nullcontext((None, None)))
    monkeypatch.setattr(ops, "rmsnorm", first_prefill_kernel)
    return calls


def _patch(m, calls, **flags):
    for layer in m.model.layers:
        layer._calls = calls
        layer.forward = types.MethodType(_stock, layer)
    prefill.enable_fused_prefill(m, **flags)


def _cache(m, B, T):
    from transformers.cache_utils import DynamicCache
    if T is None:
        return None
    cache = DynamicCache(config=m.config)
    att = m.model.layers[0].self_attn
    kv = torch.zeros(B, m.config.num_key_value_heads, T, att.head_dim, dtype=m.dtype)
    cache.update(kv, kv, 0)
    return cache


def _route(m, calls, stack_mask, B=2, S=8, T=None):
    """The route one call of layer 0 takes after the decoder stack's pre-hook has judged `stack_mask`."""
    layer = m.model.layers[0]
    with torch.no_grad():
        m.model(inputs_embeds=torch.zeros(stack_mask.shape[0], stack_mask.shape[1], m.config.hidden_size, dtype=m.dtype),
                attention_mask=stack_mask, use_cache=False)
    calls.clear()
    x = torch.zeros(B, S, m.config.hidden_size, dtype=m.dtype).as_subclass(_FakeCuda)
    d = layer.self_attn.head_dim
    kwargs = dict(attention_mask=None, position_embeddings=(torch.ones(B, S, d, dtype=m.dtype), torch.zeros(B, S, d, dtype=m.dtype)),
                  past_key_values=_cache(m, B, T))
    try:
        with torch.no_grad():
            layer(x, **kwargs)
    except _Routed:
        return "prefill"
    assert len(calls) == 1, calls
    return calls[0]


def _mask(kind, B=2, S=8):
    m = torch.ones(B, S, dtype=torch.int64)
    if kind == "left":
        m[-1, :3] = 0
    elif kind == "right":
        m[-1, 5:] = 0
    elif kind == "hole":
        m[-1, 2] = 0
    return m


PHI3W = dict(kind="phi3", hidden=192, head_dim=96, window=32)

# (model kwargs, stack mask, call kwargs, route with padded=True); with the default padded=False every one of them is stock
PADDED = {
    "prefill, left": ({}, _mask("left"), {}, "prefill"),
    "prefill, right": ({}, _mask("right"), {}, "prefill"),
    "prefill, llama, left": (dict(kind="llama"), _mask("left"), {}, "prefill"),
    "prefill, head dim 96, left": (dict(head_dim=96), _mask("left"), {}, "prefill"),
    "prefill, hole": ({}, _mask("hole"), {}, "stock"),
    "prefill, mask of another width": ({}, _mask("left", S=9), {}, "stock"),
    "prefill, mask of another batch": ({}, _mask("left", B=3), {}, "stock"),
    "prefill, windowed layer, left": (PHI3W, _mask("left"), {}, "stock"),
    "prefill, windowed layer, right": (PHI3W, _mask("right"), {}, "stock"),
    "decode, left, cache + 1 columns": ({}, _mask("left", S=6), dict(S=1, T=5), ("decode", None)),
    "decode, left, batch 16": ({}, _mask("left", B=16, S=6), dict(B=16, S=1, T=5), ("decode", None)),
    "decode, left, batch 17": ({}, _mask("left", B=17, S=6), dict(B=17, S=1, T=5), "stock"),
    "decode, left, cache columns": ({}, _mask("left", S=5), dict(S=1, T=5), "stock"),
    "decode, left, cache + 2 columns": ({}, _mask("left", S=7), dict(S=1, T=5), "stock"),
    "decode, right-padded cache": ({}, torch.tensor([[1] * 6, [1, 1, 1, 0, 0, 1]]), dict(S=1, T=5), "stock"),
    "decode, right": ({}, _mask("right", S=6), dict(S=1, T=5), "stock"),
    "decode, windowed layer, left": (PHI3W, _mask("left", S=6), dict(S=1, T=5), "stock"),
}


@pytest.mark.parametrize("name", list(PADDED))
def test_padded_route(recorder, name):
    mk, mask, call, want = PADDED[name]
    m = _model(**mk)
    _patch(m, recorder, padded=True)
    assert _route(m, recorder, mask, **call) == want


@pytest.mark.parametrize("name", list(PADDED))
def test_padded_route_is_stock_by_default(recorder, name):
    mk, mask, call, _ = PADDED[name]
    m = _model(**mk)
    _patch(m, recorder)
    assert _route(m, recorder, mask, **call) == "stock"


def test_unpadded_calls_route_as_before_with_the_switch_on(recorder):
    """All-ones and absent masks: the same routes with padded=True, the windowed layer included; the switch is set anew by
    every enable call."""
    m = _model()
    _patch(m, recorder, padded=True)
    assert m.model._u2_stack.padded is True
    assert _route(m, recorder, torch.ones(2, 8, dtype=torch.int64)) == "prefill"
    assert _route(m, recorder, torch.ones(2, 6, dtype=torch.int64), S=1, T=5) == ("decode", None)
    prefill.enable_fused_prefill(m)
    assert m.model._u2_stack.padded is False
    assert _route(m, recorder, _mask("left")) == "stock"
    w = _model(**PHI3W)
    _patch(w, recorder, padded=True)
    assert _route(w, recorder, torch.ones(2, 8, dtype=torch.int64)) == "prefill"
    assert _route(w, recorder, torch.ones(2, 6, dtype=torch.int64), S=1, T=5) == ("decode", 32)


def test_lm_config_switch_is_passed_on(monkeypatch):
    """`config.u2_fused_padded_batches` reaches enable_fused_prefill as `padded` (default: not passed, so False)."""
    from u2tokenizer_amd import language_model as LM
    seen = []
    monkeypatch.setattr(prefill, "enable_fused_prefill", lambda model, **kw: seen.append(kw) or 0)
    for on in (None, True):
        cfg = LM.u2Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                               num_key_value_heads=2, head_dim=16)
        if on is not None:
            cfg.u2_fused_padded_batches = on
        m = LM.u2Qwen3ForCausalLM(cfg).to(bf).eval()
        layer = m.model.layers[0]
        p0 = next(layer.parameters())
        layer.parameters = lambda *a, p0=p0, **k: iter([p0.detach().as_subclass(_FakeCuda)])
        with torch.no_grad():
            m(inputs_embeds=torch.zeros(1, 3, 64, dtype=bf))
    assert [kw.get("padded", False) for kw in seen] == [False, True]


# ------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("elem", ["bf16", "f16"])
def test_decode_attention_rejects_bad_arguments_and_sizes_its_workspace(elem):
    """u2tok_decode_attention returns before any launch on arguments it cannot take; its workspace depends on (B, Hq, Hkv, T, D)
    only, grows with T and is zero while the keys are too few to split."""
    from u2tokenizer_amd import _lib
    h = _lib.load_library(elem)
    P = 1 << 20   # an aligned address that is never dereferenced
    # q, K, V, out, B, Hq, Hkv, T, D, ldq, kv_stride, ldo, scale, kv_start, ws, ws_bytes, stream
    args = [P, P, P, P, 2, 8, 2, 100, 128, 8 * 128, 0, 8 * 128, 0.1, None, None, 0, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return h.u2tok_decode_attention(*a)

    for i in (0, 1, 2, 3):
        assert call(**{f"a{i}": None}) == -1, i
    assert call(a8=256) == -1 and call(a8=100) == -1          # head dim
    assert call(a5=34, a9=34 * 128, a11=34 * 128) == -1       # 17 query heads per kv head
    assert call(a5=7) == -1                                   # Hq % Hkv
    assert call(a4=0) == -1 and call(a7=0) == -1
    assert call(a10=100 * 128 - 8) == -1                      # kv_stride < T * D
    assert call(a9=8 * 128 - 8) == -1 and call(a9=8 * 128 + 4) == -1
    assert call(a12=0.0) == -1
    assert call(a0=P + 8) == -1 and call(a13=P + 2) == -1     # alignment of q / kv_start
    assert call(a7=1100, a14=P, a15=16) == -3                 # short workspace
    need = [h.u2tok_decode_attention_workspace_bytes(8, 32, 8, T, 128) for T in (5, 200, 1100, 1792, 4096)]
    assert need[0] == 0 and need == sorted(need) and need[2] > 0
    assert h.u2tok_decode_attention_workspace_bytes(0, 32, 8, 100, 128) == 0
    cfg = _lib.DecodeConfig(B=8, E=4096, Hq=32, Hkv=8, D=128, I=12288, eps=1e-6, qk_eps=1e-6, scale=0.1)
    import ctypes as C
    assert h.u2tok_decoder_decode_workspace_bytes(C.byref(cfg), 1100) >= need[2]   # the step's workspace covers the batched kernel
    assert h.u2tok_attention_gqa_range(None, P, P, P, 1, 8, 8, 4, 2, 64, 512, 512, 512, 256, 4096, 4096, 4096, 2048, 0.1, 1, P, None,
                                       None, 0, None) == -1
    assert h.u2tok_attention_gqa_range(P, P, P, P, 1, 8, 8, 4, 2, 64, 512, 512, 512, 256, 4096, 4096, 4096, 2048, 0.1, 1, P + 2, None,
                                       None, 0, None) == -1
