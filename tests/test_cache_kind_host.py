"""CPU: `kv_cache.layer_kind`, the one classifier of a call's cache layer, as a table: one row per answer, and for each row the
verdict `route` draws from it for a decode step and for a continued prefill, and `stack_route` for the whole-stack step, under each
switch that bears on it.  The expected verdicts are written out from the SWITCHES docs (`decode`, `continued`, `kv8`,
`kv8_continued`, `stack_decode`, `stack_kv8`), not computed.  The model is a one-layer Phi-3 stub with an attention window of 2, so
that a call of 3 positions is never the plain prefill; the sliding row is asked on a Qwen3 stub (no window) as well."""
import pytest
import torch
from transformers.cache_utils import DynamicCache, DynamicLayer, DynamicSlidingWindowLayer

from test_decoder_route_host import _FakeCuda, _model
from u2tokenizer_amd import kv_cache as KC
from u2tokenizer_amd import prefill

bf = torch.bfloat16
B, T, W = 2, 5, 2


class _Other(DynamicCache):
    pass


def _kv(m, batch=B):
    return torch.zeros(batch, m.config.num_key_value_heads, T, m.model.layers[0].self_attn.head_dim, dtype=bf)


def _of(lay):
    cache = DynamicCache()
    cache.layers.append(lay)
    return cache


def _filled(cls, m, batch=B, **kw):
    lay = cls(**kw)
    lay.update(_kv(m, batch), _kv(m, batch))
    return lay


def _kv8(m, batch=B, fake=True):
    lay = _filled(prefill.Kv8Layer, m, batch)
    if fake:
        lay._kc = lay._kc.as_subclass(_FakeCuda)
    return lay


def _foreign(m):
    cache = _Other()
    cache.update(_kv(m), _kv(m), 0)
    return cache


def _offloaded(m):
    cache = _of(_filled(DynamicLayer, m))
    cache.offloading = True
    return cache


A = prefill._append_layer_class
# name: (cache of a model, kind, decode {} / {kv8}, 3 positions {continued} / {kv8_continued}, stack {stack_decode} / {stack_kv8})
ROWS = {
    "no cache": (lambda m: None, KC.NO_CACHE, "stock", "stock", "extend", "extend", "layers", "layers"),
    "another cache class": (_foreign, KC.FOREIGN, "stock", "stock", "stock", "stock", "layers", "layers"),
    "an offloaded cache": (_offloaded, KC.FOREIGN, "stock", "stock", "stock", "stock", "layers", "layers"),
    "a layer still to be created": (lambda m: DynamicCache(), KC.LAZY, "stock", "stock", "extend", "extend", "layers", "layers"),
    "an empty DynamicLayer": (lambda m: _of(DynamicLayer()), KC.EMPTY, "stock", "stock", "extend", "extend", "layers", "layers"),
    "a DynamicLayer": (lambda m: _of(_filled(DynamicLayer, m)), KC.DENSE, "decode", "decode", "extend", "extend", "layers", "layers"),
    "a DynamicSlidingWindowLayer": (lambda m: _of(_filled(DynamicSlidingWindowLayer, m, sliding_window=W)), KC.SLIDING,
                                    "decode", "decode", "extend", "extend", "layers", "layers"),
    "append-in-place, this batch": (lambda m: _of(_filled(A(), m)), KC.APPEND, "decode", "decode", "extend", "extend", "stack", "stack"),
    "append-in-place, another batch": (lambda m: _of(_filled(A(), m, B + 1)), KC.APPEND_OTHER,
                                       "decode", "decode", "extend", "extend", "layers", "layers"),
    "codes the kernels take": (lambda m: _of(_kv8(m)), KC.KV8, "stock", "decode", "stock", "extend", "layers", "stack"),
    "codes of another batch": (lambda m: _of(_kv8(m, B + 1)), KC.KV8_OTHER, "stock", "stock", "stock", "stock", "layers", "layers"),
    "codes on the CPU": (lambda m: _of(_kv8(m, fake=False)), KC.KV8_OTHER, "stock", "stock", "stock", "stock", "layers", "layers"),
    "an empty Kv8Layer": (lambda m: _of(prefill.Kv8Layer()), KC.KV8_OTHER, "stock", "stock", "stock", "stock", "layers", "layers"),
}


class _Dec:   # what stack_route reads of `_decode_state`'s first result
    ok, hd = True, 96


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(prefill, "_decode_state", lambda layer, B, device, pr: (_Dec(), {}))


def _ask(m, cache, S):
    layer = m.model.layers[0]
    d = layer.self_attn.head_dim
    kw = dict(past_key_values=cache, position_embeddings=(torch.empty(0, d),) * 2)
    return prefill.route(layer, (B, S, m.config.hidden_size), bf, True, (), kw, False, layer._u2_prefill.layout.projections(layer))[0]


def _ask_stack(m, cache):
    call = dict(past_key_values=cache, use_cache=True, output_hidden_states=False, output_attentions=False)
    return prefill.stack_route(m.model, B, 1, bf, True, call, False)


@pytest.mark.parametrize("name", list(ROWS))
def test_each_answer_and_the_verdicts_drawn_from_it(stub, name):
    make, kind, dec, dec8, ext, ext8, stack, stack8 = ROWS[name]
    m = _model("phi3", hidden=192, head_dim=96, window=W)
    got, lay = KC.layer_kind(make(m), 0, B)
    assert got is kind
    assert (lay is None) == (kind in (KC.NO_CACHE, KC.LAZY) or name in ("another cache class", "an offloaded cache"))
    for sw, S, want in (({}, 1, dec), (dict(kv8=True), 1, dec8), (dict(decode=False, kv8=True), 1, "stock"),
                        ({}, 3, "stock"), (dict(kv8=True), 3, "stock"), (dict(continued=True), 3, ext),
                        (dict(continued=True, kv8=True), 3, ext), (dict(kv8_continued=True), 3, ext8)):
        prefill.enable_fused_prefill(m, **sw)
        assert _ask(m, make(m), S) == want, (sw, S)
    for sw, want in ((dict(stack_decode=True), stack), (dict(stack_decode=True, kv8=True), stack), (dict(stack_kv8=True), stack8),
                     ({}, "layers")):
        prefill.enable_fused_prefill(m, **sw)
        assert _ask_stack(m, make(m)) == want, sw
    prefill.disable_fused_prefill(m)


def test_policy_that_is_not_the_layers_kind_stays_in_route(stub, monkeypatch):
    """the cap on a group's query heads, the cap on the rows of a continued prefill on codes, and a window for a sliding layer"""
    m = _model(num_attention_heads=34, num_key_value_heads=2)              # 17 query heads per kv head
    prefill.enable_fused_prefill(m, kv8_continued=True)
    assert _ask(m, _of(_kv8(m)), 1) == "stock" and _ask(m, _of(_kv8(m)), 3) == "stock"
    assert _ask(m, _of(_filled(A(), m)), 1) == "decode" and _ask(m, _of(_filled(A(), m)), 3) == "extend"
    m = _model()
    prefill.enable_fused_prefill(m, kv8_continued=True, stack_decode=True)
    assert _ask(m, _of(_kv8(m)), 3) == "extend"
    monkeypatch.setattr(prefill, "KV8_EXTEND_MAX_ROWS", 2)
    assert _ask(m, _of(_kv8(m)), 3) == "stock" and _ask(m, _of(_kv8(m)), 2) == "extend"
    assert _ask(m, _of(_filled(A(), m)), 3) == "extend"                     # (the cap is the codes' alone)
    # a sliding layer under a model without a window: neither step takes it
    sliding = lambda: _of(_filled(DynamicSlidingWindowLayer, m, sliding_window=W))   # noqa: E731
    assert KC.layer_kind(sliding(), 0, B)[0] is KC.SLIDING and _ask(m, sliding(), 1) == "stock" and _ask(m, sliding(), 3) == "stock"
    # a cache that mixes the in-place kinds keeps the layers
    m2 = _model(num_hidden_layers=2)
    prefill.enable_fused_prefill(m2, stack_kv8=True)
    cache = _of(_kv8(m2))
    cache.layers.append(_filled(A(), m2))
    assert _ask_stack(m2, cache) == "layers"
    cache.layers[1] = _kv8(m2)
    assert _ask_stack(m2, cache) == "stack"
