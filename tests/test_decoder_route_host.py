"""CPU: which forward a call of a patched decoder layer takes -- the training route, the fused decode step, the fused prefill
or the layer's stock forward -- pinned as a table.  Each case flips one input of an eligible baseline.

No GPU: the input is a CPU tensor that reports `is_cuda`, and every route ends in a recorder before it would launch anything
(the training route's `decoder_train.layer_forward_train`, the decode step `prefill._decode_step`, the prefill's first kernel
`ops.rmsnorm`, and the stock forward the layer had when it was patched)."""
import contextlib
import types

import pytest
import torch

from u2tokenizer_amd import decoder_train, ops, prefill

bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32


class _FakeCuda(torch.Tensor):
    @property
    def is_cuda(self):
        return True


class _Routed(Exception):
    pass


class _NotLinear(torch.nn.Linear):   # (a wrapped projection: same weight, another module type)
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

    def train(*args, **kwargs):
        calls.append("train")
        return "trained"

    def first_prefill_kernel(*args, **kwargs):
        raise _Routed

    monkeypatch.setattr(prefill, "_decode_step", decode)
    monkeypatch.setattr(prefill, "_ensure_gemm_scratch", lambda device: None)
    monkeypatch.setattr(decoder_train, "layer_forward_train", train)
    monkeypatch.setattr(ops, "on_device", lambda *a, **k: contextlib.nullcontext((None, None)))
    monkeypatch.setattr(ops, "rmsnorm", first_prefill_kernel)
    return calls


def _patch(m, calls, decode=True, train=False, prefill_on=True):
    for layer in m.model.layers:
        layer._calls = calls
        layer.forward = types.MethodType(_stock, layer)
    prefill.enable_fused_prefill(m, decode=decode, train=train, prefill=prefill_on)


def _cache(kind, m, B, T):
    from transformers.cache_utils import DynamicCache

    class OtherCache(DynamicCache):
        pass

    if kind is None:
        return None
    cls = OtherCache if kind.startswith("other") else DynamicCache
    cache = cls() if kind.startswith("bare") else cls(config=m.config)     # (bare: no per-config layer kinds)
    if kind.endswith("full"):
        att = m.model.layers[0].self_attn
        kv = torch.zeros(B, m.config.num_key_value_heads, T, att.head_dim, dtype=m.dtype)
        cache.update(kv, kv, 0)
    return cache


def _route(m, calls, B=2, S=8, dtype=None, grad=False, cache=None, T=5, mask=None, stack_mask=None, pe=True, args=(),
           **kw):
    """The route one call of layer 0 takes: "train", ("decode", W), "prefill" or "stock"."""
    layer = m.model.layers[0]
    att = layer.self_attn
    dtype = dtype or m.dtype
    if stack_mask is not None:          # the decoder stack's pre-hook judges the 2-D mask of the whole call
        with torch.no_grad():
            m.model(inputs_embeds=torch.zeros(stack_mask.shape[0], stack_mask.shape[1], m.config.hidden_size, dtype=m.dtype),
                    attention_mask=stack_mask, use_cache=False)
    calls.clear()
    x = torch.zeros(B, S, m.config.hidden_size, dtype=dtype).as_subclass(_FakeCuda)
    d = att.head_dim
    kwargs = dict(attention_mask=mask, position_embeddings=(torch.ones(B, S, d, dtype=dtype), torch.zeros(B, S, d, dtype=dtype))
                  if pe else None, past_key_values=_cache(cache, m, B, T), **kw)
    try:
        with torch.set_grad_enabled(grad):
            layer(x, *args, **kwargs)
    except _Routed:
        return "prefill"
    assert len(calls) == 1, calls
    return calls[0]


def _right_padded(B, S, valid):
    vis = torch.tril(torch.ones(S, S, dtype=torch.bool))[None, None].repeat(B, 1, 1, 1)
    vis[-1, :, :, valid:] = False
    return vis


def _left_padded(B, S):
    vis = torch.tril(torch.ones(S, S, dtype=torch.bool))[None, None].repeat(B, 1, 1, 1)
    vis[-1, :, :, :2] = False
    return vis


# (model kwargs, enable flags, call kwargs, expected route)
INFER = {
    "baseline": ({}, {}, {}, "prefill"),
    "fp16 model": (dict(dtype=f16), {}, {}, "prefill"),
    "fp32 model": (dict(dtype=f32), {}, {}, "stock"),
    "fp16 input, bf16 weights": ({}, {}, dict(dtype=f16), "stock"),
    "head dim 96": (dict(head_dim=96), {}, {}, "prefill"),
    "head dim 128": (dict(head_dim=128), {}, {}, "prefill"),
    "head dim 256": (dict(head_dim=256), {}, {}, "stock"),
    "llama": (dict(kind="llama"), {}, {}, "prefill"),
    "phi3": (dict(kind="phi3", hidden=192, head_dim=96), {}, {}, "prefill"),
    "prefill off": ({}, dict(prefill_on=False), {}, "stock"),
    "train flag without grad": ({}, dict(train=True), {}, "prefill"),
    "one position, no cache": ({}, {}, dict(S=1), "stock"),
    "empty plain cache": ({}, {}, dict(cache="plain"), "prefill"),
    "filled plain cache": ({}, {}, dict(cache="plain full"), "stock"),
    "empty non-plain cache": ({}, {}, dict(cache="other"), "prefill"),
    "filled non-plain cache": ({}, {}, dict(cache="other full"), "stock"),
    "padded stack mask": ({}, {}, dict(stack_mask=torch.tensor([[0, 1, 1, 1]])), "stock"),
    "all-ones stack mask": ({}, {}, dict(stack_mask=torch.ones(1, 4, dtype=torch.int64)), "prefill"),
    "output_attentions": ({}, {}, dict(output_attentions=True), "stock"),
    "positional argument": ({}, {}, dict(args=(None,)), "stock"),
    "past_key_value": ({}, {}, dict(past_key_value=None), "stock"),
    "no position embeddings": ({}, {}, dict(pe=False), "stock"),
    "window W, S < W": (dict(kind="phi3", hidden=192, head_dim=96, window=32), {}, dict(S=24), "prefill"),
    "window W, S = W": (dict(kind="phi3", hidden=192, head_dim=96, window=32), {}, dict(S=32), "prefill"),
    "window W, S > W": (dict(kind="phi3", hidden=192, head_dim=96, window=32), {}, dict(S=40), "stock"),
    # decode: one new position per sequence against a filled plain DynamicCache
    "decode": ({}, {}, dict(S=1, cache="plain full"), ("decode", None)),
    "decode, batch 16": ({}, {}, dict(S=1, B=16, cache="plain full"), ("decode", None)),
    "decode, batch 17": ({}, {}, dict(S=1, B=17, cache="plain full"), "stock"),
    "decode off": ({}, dict(decode=False), dict(S=1, cache="plain full"), "stock"),
    "decode, prefill off": ({}, dict(prefill_on=False), dict(S=1, cache="plain full"), "stock"),
    "decode, empty cache": ({}, {}, dict(S=1, cache="plain"), "stock"),
    "decode, non-plain cache": ({}, {}, dict(S=1, cache="other full"), "stock"),
    "decode, fp16": (dict(dtype=f16), {}, dict(S=1, cache="plain full"), ("decode", None)),
    "decode, fp32": (dict(dtype=f32), {}, dict(S=1, cache="plain full"), "stock"),
    "decode, head dim 256": (dict(head_dim=256), {}, dict(S=1, cache="plain full"), "stock"),
    "decode, padded stack mask": ({}, {}, dict(S=1, cache="plain full", stack_mask=torch.tensor([[0, 1, 1, 1]])), "stock"),
    "decode, window W": (dict(kind="phi3", hidden=192, head_dim=96, window=32), {}, dict(S=1, cache="plain full", T=40),
                         ("decode", 32)),
    "decode, window W, plain layers": (dict(kind="phi3", hidden=192, head_dim=96, window=32), {},
                                       dict(S=1, cache="bare full", T=40), ("decode", 32)),
}

TRAIN = {
    "baseline": ({}, {}, {}, "train"),
    "train flag off": ({}, dict(train=False), {}, "stock"),
    "prefill off": ({}, dict(prefill_on=False), {}, "train"),
    "decode off": ({}, dict(decode=False), {}, "train"),
    "llama": (dict(kind="llama"), {}, {}, "train"),
    "one position": ({}, {}, dict(S=1), "train"),
    "batch 17": ({}, {}, dict(B=17), "train"),
    "fp16": (dict(dtype=f16), {}, {}, "stock"),
    "fp32": (dict(dtype=f32), {}, {}, "stock"),
    "head dim 96": (dict(head_dim=96), {}, {}, "stock"),
    "head dim 128": (dict(head_dim=128), {}, {}, "train"),
    "head dim 256": (dict(head_dim=256), {}, {}, "stock"),
    "hidden % 8 != 0": (dict(hidden=132), {}, {}, "stock"),
    "intermediate % 8 != 0": (dict(inter=260), {}, {}, "stock"),
    "empty cache": ({}, {}, dict(cache="plain"), "stock"),
    "filled cache": ({}, {}, dict(cache="plain full"), "stock"),
    "output_attentions": ({}, {}, dict(output_attentions=True), "stock"),
    "positional argument": ({}, {}, dict(args=(None,)), "stock"),
    "past_key_value": ({}, {}, dict(past_key_value=None), "stock"),
    "no position embeddings": ({}, {}, dict(pe=False), "stock"),
    "right-padded layer mask": ({}, {}, dict(B=2, S=8, mask=_right_padded(2, 8, 5)), "train"),
    "left-padded layer mask": ({}, {}, dict(B=2, S=8, mask=_left_padded(2, 8)), "stock"),
    "padded stack mask": ({}, {}, dict(stack_mask=torch.tensor([[0, 1, 1, 1]])), "train"),   # (the layer's own mask rules)
    "phi3 layout": (dict(kind="phi3", hidden=192, head_dim=96), {}, {}, "stock"),
    "phi3 layout, head dim 64": (dict(kind="phi3", hidden=128, head_dim=64), {}, {}, "stock"),
}


@pytest.mark.parametrize("name", list(INFER))
def test_inference_route(recorder, name):
    mk, flags, call, want = INFER[name]
    m = _model(**mk)
    _patch(m, recorder, **flags)
    assert _route(m, recorder, **call) == want


@pytest.mark.parametrize("name", list(TRAIN))
def test_training_route(recorder, name):
    mk, flags, call, want = TRAIN[name]
    m = _model(**mk)
    _patch(m, recorder, **{"train": True, **flags})
    assert _route(m, recorder, grad=True, **call) == want


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("change", ["not linear", "hook", "attention dropout, training mode", "attention dropout, eval mode",
                                    "phi3 residual dropout, training mode", "phi3 no dropout, training mode"])
def test_route_of_modified_layers(recorder, grad, change):
    """Module-level changes after patching: a wrapped projection or a hook sends every route to the stock forward; active
    dropout blocks the training route (Llama / Qwen3 attention dropout) or every route (Phi-3 residual dropout)."""
    phi3 = change.startswith("phi3")
    m = _model("phi3", hidden=192, head_dim=96, resid_pdrop=0.0 if "no dropout" in change else 0.1) if phi3 else _model()
    _patch(m, recorder, train=True)
    layer = m.model.layers[0]
    fused = "train" if grad else "prefill"
    if change == "not linear":
        old = layer.self_attn.q_proj
        layer.self_attn.q_proj = _NotLinear(old.in_features, old.out_features, bias=False, dtype=old.weight.dtype)
        want = "stock"
    elif change == "hook":
        layer.mlp.register_forward_hook(lambda *a: None)
        want = "stock"
    elif change.startswith("attention dropout"):
        layer.self_attn.attention_dropout = 0.1
        if "training" in change:
            m.train()
        # (in training mode with grad off the fused prefill still runs, without the dropout)
        want = "stock" if grad and "training" in change else fused
    else:
        m.train()
        want = "stock" if grad or "no dropout" not in change else "prefill"
    assert _route(m, recorder, grad=grad) == want
