"""CPU: u2tokenizer_amd.lora -- the LoRA wrapper with peft's attribute layout and state-dict keys, add_lora / merge_lora /
load_lora_state_dict on small Llama, Qwen3 and Phi-3 decoders -- and which forward a LoRA-wrapped layer takes (prefill.route with the
train_lora switch; called without GPU tensors, as tests/test_decoder_route_host.py does)."""
import types

import pytest
import torch
from torch import nn

from test_decoder_route_host import _model, _route, _stock, recorder  # noqa: F401
from u2tokenizer_amd import lora, prefill
from u2tokenizer_amd.lora import LoRALinear, add_lora, load_lora_state_dict, merge_lora

bf, f32 = torch.bfloat16, torch.float32
KINDS = ("llama", "qwen3", "phi3")
PER_LAYER = {"llama": 7, "qwen3": 7, "phi3": 4}


def _tiny(kind, dtype=f32):
    """two layers, hidden size 64"""
    kw = dict(hidden=64, inter=128, num_hidden_layers=2, dtype=dtype)
    return _model(kind, head_dim=32, **kw)


def _ids():
    return torch.randint(0, 64, (2, 9), generator=torch.Generator().manual_seed(1))


def _fill_b(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    for mod in m.modules():
        if isinstance(mod, LoRALinear):
            w = mod.lora_B["default"].weight
            w.data.copy_(torch.randn(w.shape, generator=g) * 0.05)


# ------------------------------------------------------------------------------------------------ the wrapper
@pytest.mark.parametrize("kind", KINDS)
def test_add_lora_keys_trainable_parameters_and_zero_b(kind):
    m = _tiny(kind)
    with torch.no_grad():
        before = m(_ids()).logits
    plain_keys = set(m.state_dict())
    assert add_lora(m) == 2 * PER_LAYER[kind]
    keys = set(m.state_dict())
    first = "qkv_proj" if kind == "phi3" else "q_proj"
    for suffix in ("base_layer.weight", "lora_A.default.weight", "lora_B.default.weight"):
        assert f"model.layers.0.self_attn.{first}.{suffix}" in keys
        assert f"model.layers.1.mlp.down_proj.{suffix}" in keys
    assert f"model.layers.0.self_attn.{first}.weight" not in keys
    # every key is a plain key, a plain key with .base_layer inserted, or an adapter weight
    for k in keys:
        assert k in plain_keys or k.replace(".base_layer.", ".") in plain_keys or ".lora_A.default." in k or ".lora_B.default." in k, k
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert trainable and all(".lora_A." in n or ".lora_B." in n for n in trainable)
    assert len(trainable) == 2 * 2 * PER_LAYER[kind]
    assert not m.lm_head.weight.requires_grad and not m.model.embed_tokens.weight.requires_grad
    lin = getattr(m.model.layers[0].self_attn, first)
    assert type(lin.base_layer) is nn.Linear and isinstance(lin.lora_A, nn.ModuleDict) and isinstance(lin.lora_dropout, nn.ModuleDict)
    assert type(lin.lora_dropout["default"]) is nn.Dropout and lin.lora_dropout["default"].p == 0.05
    assert lin.scaling == {"default": 2.0} and lin.r == {"default": 16} and lin.lora_alpha == {"default": 32}
    assert lin.active_adapters == ["default"] and lin.merged is False and lin.disable_adapters is False
    assert lin.weight is lin.base_layer.weight and lin.bias is lin.base_layer.bias
    assert lin.lora_A["default"].bias is None and lin.lora_B["default"].bias is None
    assert not lin.lora_B["default"].weight.any() and lin.lora_A["default"].weight.abs().max() > 0
    with torch.no_grad():
        assert torch.equal(m(_ids()).logits, before)       # zero B: bit-equal
    assert add_lora(m) == 0                                # nothing left to wrap (adapters' own Linears are not wrapped)


def test_add_lora_targets_dropout_and_dtype():
    m = _tiny("llama", dtype=bf)
    assert add_lora(m, r=32, alpha=16, dropout=0.0, target_modules=("q_proj", "v_proj"), adapter_dtype=f32) == 4
    att = m.model.layers[1].self_attn
    assert isinstance(att.q_proj, LoRALinear) and isinstance(att.v_proj, LoRALinear) and type(att.k_proj) is nn.Linear
    assert type(att.q_proj.lora_dropout["default"]) is nn.Identity and att.q_proj.scaling["default"] == 0.5
    assert att.q_proj.lora_A["default"].weight.dtype == f32 and att.q_proj.weight.dtype == bf
    _fill_b(m)
    x = torch.randn(2, 5, 64, generator=torch.Generator().manual_seed(2)).to(bf)
    y = att.q_proj(x)
    assert y.dtype == bf                                   # the branch runs in fp32, the result keeps the base dtype
    want = att.q_proj.base_layer(x).float() + (x.float() @ att.q_proj.lora_A["default"].weight.T
                                               @ att.q_proj.lora_B["default"].weight.T) * 0.5
    assert torch.allclose(y.float(), want, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("kind", KINDS)
def test_merge_and_state_dict_round_trip(kind):
    m = _tiny(kind)
    add_lora(m)
    m.eval()                                               # (the new dropout modules too)
    _fill_b(m)
    ids = _ids()
    with torch.no_grad():
        wrapped = m(ids).logits
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for prefix in ("", lora.PEFT_PREFIX):
        m2 = _tiny(kind).eval()
        with torch.no_grad():
            for p in m2.parameters():
                p.add_(0.01)                               # (another model: everything must come from the file)
        add_lora(m2)
        m2.eval()
        res = load_lora_state_dict(m2, {prefix + k: v for k, v in sd.items()})
        assert not res.missing_keys and not res.unexpected_keys
        with torch.no_grad():
            assert torch.equal(m2(ids).logits, wrapped)
    with pytest.raises(RuntimeError, match="without a partner"):
        load_lora_state_dict(_tiny(kind), sd)              # an unwrapped model has no place for the adapter keys
    with torch.no_grad():
        plain = _tiny(kind).eval()(ids).logits
    assert (wrapped - plain).abs().max() > 1e-3 * plain.abs().max()   # the adapters do something
    assert merge_lora(m) == 2 * PER_LAYER[kind]
    assert not any(isinstance(mod, LoRALinear) for mod in m.modules())
    for layer in m.model.layers:
        for mod in layer.modules():
            assert not list(mod.children()) or all(type(c) is nn.Linear for c in mod.children() if isinstance(c, nn.Linear))
    assert set(m.state_dict()) == set(_tiny(kind).state_dict())
    with torch.no_grad():
        merged = m(ids).logits
    rel = ((merged - wrapped).norm() / wrapped.norm()).item()
    assert rel <= 1e-5, rel


def test_merge_keeps_packed_buffers():
    """weights that are views of prefill._pack's q|k|v buffer stay views of it, and the buffer holds the merged rows"""
    m = _tiny("llama")
    att = m.model.layers[0].self_attn
    W, _ = prefill._pack((att.q_proj, att.k_proj, att.v_proj))
    add_lora(m)
    _fill_b(m)
    delta = att.k_proj.delta_weight("default")
    old = att.k_proj.weight.detach().clone()
    W2, _ = prefill._pack((att.q_proj, att.k_proj, att.v_proj))          # (reads .base_layer of the wrapped projections)
    assert W2.data_ptr() == W.data_ptr()
    merge_lora(m)
    nq = att.q_proj.weight.shape[0]
    assert att.k_proj.weight.data_ptr() == W.data_ptr() + nq * W.shape[1] * W.element_size()
    assert torch.allclose(W[nq:nq + old.shape[0]], old + delta, atol=1e-6)


# ------------------------------------------------------------------------------------------------ the route
def _patched(calls, kind="qwen3", wrap=True, adapter_dtype=None, **flags):
    mk = dict(kind="phi3", hidden=192, head_dim=96) if kind == "phi3" else dict(kind=kind)
    m = _model(**mk)
    for layer in m.model.layers:
        layer._calls = calls
        layer.forward = types.MethodType(_stock, layer)
    if wrap:
        add_lora(m, adapter_dtype=adapter_dtype)
    prefill.enable_fused_prefill(m, **flags)
    return m


def test_route_of_wrapped_layers(recorder):
    assert _route(_patched(recorder, train_lora=True), recorder, grad=True) == "train"
    assert _route(_patched(recorder, "llama", train_lora=True, adapter_dtype=f32), recorder, grad=True) == "train"
    assert _route(_patched(recorder, train=True, train_lora=True), recorder, grad=True) == "train"
    assert _route(_patched(recorder, train=True), recorder, grad=True) == "stock"          # train alone: wrapped stays stock
    assert _route(_patched(recorder), recorder, grad=True) == "stock"
    assert _route(_patched(recorder, wrap=False, train_lora=True), recorder, grad=True) == "train"   # the switch implies the route
    assert _route(_patched(recorder, train_lora=True), recorder, grad=False) == "stock"    # prefill / decode: never with adapters
    assert _route(_patched(recorder, "phi3", train_lora=True), recorder, grad=True) == "stock"        # Phi-3 needs train_phi3
    assert _route(_patched(recorder, "phi3", train_lora=True, train_phi3=True), recorder, grad=True) == "train"
    m = _patched(recorder, train_lora=True)
    merge_lora(m)
    assert _route(m, recorder, grad=True) == "train" and _route(m, recorder, grad=False) == "prefill"


class _LinearSub(nn.Linear):
    pass


class _Unreadable(LoRALinear):
    @property
    def use_dora(self):
        raise RuntimeError("not for you")


def _two_adapters(q):
    q.lora_A["other"], q.lora_B["other"] = nn.Linear(q.in_features, 16, bias=False), nn.Linear(16, q.out_features, bias=False)
    q.lora_dropout["other"] = nn.Identity()
    q.r["other"], q.scaling["other"], q.lora_alpha["other"] = 16, 2.0, 32
    q.active_adapters = ["default", "other"]


def _swap(q, which, new):
    getattr(q, which)["default"] = new.to(q.weight.dtype)


def _rank(q, r):
    q.r["default"] = r
    _swap(q, "lora_A", nn.Linear(q.in_features, r, bias=False))
    _swap(q, "lora_B", nn.Linear(r, q.out_features, bias=False))


def _unreadable(q):
    q.__class__ = _Unreadable


REFUSALS = {
    "two active adapters": _two_adapters,
    "no active adapter": lambda q: setattr(q, "active_adapters", []),
    "merged": lambda q: setattr(q, "merged", True),
    "disabled": lambda q: setattr(q, "disable_adapters", True),
    "lora_A a Linear subclass": lambda q: _swap(q, "lora_A", _LinearSub(q.in_features, 16, bias=False)),
    "lora_B with a bias": lambda q: _swap(q, "lora_B", nn.Linear(16, q.out_features, bias=True)),
    "fp16 adapter": lambda q: (q.lora_A.to(torch.float16), q.lora_B.to(torch.float16)),
    "A and B of two dtypes": lambda q: q.lora_B.to(f32),
    "r = 8": lambda q: _rank(q, 8),
    "r = 48": lambda q: _rank(q, 48),
    "r says 16, A has 32 rows": lambda q: _swap(q, "lora_A", nn.Linear(q.in_features, 32, bias=False)),
    "base layer a Linear subclass": lambda q: setattr(q, "base_layer", _LinearSub(q.in_features, q.out_features, bias=False).to(bf)),
    "in-place dropout": lambda q: setattr(q.lora_dropout["default"], "inplace", True),
    "no dropout entry": lambda q: q.lora_dropout.pop("default"),
    "hook on the wrapper": lambda q: q.register_forward_hook(lambda *a: None),
    "hook on the base layer": lambda q: q.base_layer.register_forward_pre_hook(lambda *a: None),
    "hook on A": lambda q: q.lora_A["default"].register_forward_hook(lambda *a: None),
    "hook on B": lambda q: q.lora_B["default"].register_full_backward_hook(lambda *a: None),
    "use_dora": lambda q: setattr(q, "use_dora", {"default": True}),
    "lora_variant": lambda q: setattr(q, "lora_variant", {"default": object()}),
    "lora_bias": lambda q: setattr(q, "lora_bias", {"default": True}),
    "fan_in_fan_out": lambda q: setattr(q, "fan_in_fan_out", True),
    "lora_magnitude_vector": lambda q: setattr(q, "lora_magnitude_vector", nn.ModuleDict({"default": nn.Identity()})),
    "lora_embedding_A": lambda q: setattr(q, "lora_embedding_A", nn.ParameterDict({"default": nn.Parameter(torch.zeros(2, 2))})),
    "unreadable attribute": _unreadable,
    "no scaling entry": lambda q: q.scaling.clear(),
}


# (these cannot run their stock forward either: the GPU sweep of tests/test_gpu_lora_train.py leaves them out)
NOT_RUNNABLE = ("r says 16, A has 32 rows", "no scaling entry", "no dropout entry", "A and B of two dtypes")


@pytest.mark.parametrize("name", list(REFUSALS))
def test_route_refuses_what_it_does_not_compute(recorder, name):
    m = _patched(recorder, train_lora=True)
    q = m.model.layers[0].self_attn.q_proj
    assert lora.adapter_of(q) is not None
    REFUSALS[name](q)
    assert lora.adapter_of(q) is None
    assert _route(m, recorder, grad=True) == "stock"


def test_unset_variants_of_the_peft_layout_are_admitted(recorder):
    """peft's lora.Linear carries these attributes on every wrapper: present but unset for the adapter, they do not refuse it"""
    m = _patched(recorder, train_lora=True)
    for q in m.model.layers[0].self_attn.children():
        if isinstance(q, LoRALinear):
            q.use_dora, q.lora_bias, q.lora_variant = {"default": False}, {"default": False}, {}
            q.fan_in_fan_out = False
            q.lora_magnitude_vector, q.lora_embedding_A = nn.ModuleDict(), nn.ParameterDict()
            q.use_dora["other"] = True                     # (another, inactive adapter's variant)
    assert _route(m, recorder, grad=True) == "train"


def test_switch_defaults_off_and_implies_the_training_route():
    import inspect
    assert inspect.signature(prefill.enable_fused_prefill).parameters["train_lora"].default is False
    m = _model()
    prefill.enable_fused_prefill(m, train_lora=True)
    assert m.model._u2_stack.train_lora and m.model._u2_stack.train
    prefill.enable_fused_prefill(m)                        # every call sets the switches anew
    assert not m.model._u2_stack.train_lora and not m.model._u2_stack.train
