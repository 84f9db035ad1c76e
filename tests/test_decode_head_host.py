"""CPU: the admission of the decode step's head (prefill.head_route), one flip of an admitted baseline at a time; the head's weight
form and its fallback (prefill.head_form); the fall-through of `head_forward` with its counter; the new exports in
_lib.SIGNATURES; and the two C entries' refusals and workspace sizing -- and the split-row sampling warper's, with the launch counts it
fixes from the parameters alone --, which need no GPU (an error code means nothing was launched: without a GPU a launch would not
return one of these codes).  The stub models and the patched two-layer stack with its cache are
those of tests/test_stack_decode_host.py."""
import ctypes as C

import pytest
import torch

from test_decoder_route_host import _NotLinear
from test_stack_decode_host import B, NL, T, _Dec, _stack
from u2tokenizer_amd import _lib, prefill

bf = torch.bfloat16


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(prefill, "_decode_state", lambda layer, B, device, pr: (_Dec(), {}))


def _ask(m, cache, B=B, S=1, dtype=bf, cuda=True, grad=False, labels=None, plan=None, **kw):
    call = dict(past_key_values=cache, use_cache=True, output_hidden_states=False, output_attentions=False)
    call.update(kw)
    return prefill.head_route(m, B, S, dtype, cuda, call, grad, labels, plan)


def test_the_admitted_baseline(stub):
    m, cache = _stack(head=True)
    assert m.model._u2_stack.head and m.model._u2_stack.stack      # (the switch implies the whole-stack route)
    plan = []
    assert _ask(m, cache, plan=plan) == "head" and [p[0] for p in plan] == list(m.model.layers)
    assert _ask(m, cache, logits_to_keep=1) == "head" and _ask(m, cache, logits_to_keep=None, return_dict=True) == "head"


def _bias(m, c):
    m.lm_head.bias = torch.nn.Parameter(torch.zeros(m.config.vocab_size, dtype=bf))


def _head_hook(m, c):
    m.lm_head.register_forward_hook(lambda *a: None)


def _head_pre_hook(m, c):
    m.lm_head.register_forward_pre_hook(lambda *a: None)


def _wrapped(m, c):
    class Wrapper(torch.nn.Module):   # (what an adapter library leaves in lm_head's place)
        def __init__(self, base_layer):
            super().__init__()
            self.base_layer = base_layer
            self.weight, self.bias = base_layer.weight, None

    m.lm_head = Wrapper(m.lm_head)


def _subclassed(m, c):
    lin = _NotLinear(m.config.hidden_size, m.config.vocab_size, bias=False).to(bf)
    m.lm_head = lin


def _head_other_type(m, c):
    m.lm_head.to(torch.float32)


def _head_elsewhere(m, c):
    m.lm_head.to("meta")


def _head_strided(m, c):
    w = m.lm_head.weight
    wide = torch.zeros(w.shape[0], w.shape[1] + 4, dtype=bf)      # rows 132 elements apart: no multiple of 8
    m.lm_head.weight = torch.nn.Parameter(wide[:, :w.shape[1]], requires_grad=False)


def _norm_hook(m, c):
    m.model.norm.register_forward_hook(lambda *a: None)


def _norm_other_class(m, c):
    m.model.norm = torch.nn.LayerNorm(m.config.hidden_size).to(bf)


def _norm_other_type(m, c):
    m.model.norm.to(torch.float32)


def _stack_hook(m, c):
    m.model.register_forward_hook(lambda *a: None)


def _stack_pre_hook(m, c):
    m.model.register_forward_pre_hook(lambda *a: None)


def _one_token_vocabulary(m, c):
    m.lm_head = torch.nn.Linear(m.config.hidden_size, 1, bias=False).to(bf)


def _other_hidden_size(m, c):
    m.lm_head = torch.nn.Linear(m.config.hidden_size * 2, m.config.vocab_size, bias=False).to(bf)


def _switch_off(m, c):
    m.model._u2_stack.head = False


def _stack_switch_off(m, c):
    m.model._u2_stack.stack = False


def _layer_hook(m, c):
    m.model.layers[1].register_forward_hook(lambda *a: None)


FLIPS = {
    "labels given": (None, dict(labels=torch.zeros(B, 1, dtype=torch.int64))),
    "two positions": (None, dict(S=2)),
    "logits_to_keep = 2": (None, dict(logits_to_keep=2)),
    "logits_to_keep a tensor": (None, dict(logits_to_keep=torch.tensor([0]))),
    "return_dict = False": (None, dict(return_dict=False)),
    "output_hidden_states": (None, dict(output_hidden_states=True)),
    "grad enabled": (None, dict(grad=True)),
    "a CPU input": (None, dict(cuda=False)),
    "another type than the weights'": (None, dict(dtype=torch.float16)),
    "no cache": (None, dict(past_key_values=None)),
    "lm_head with bias": (_bias, {}),
    "a forward hook on lm_head": (_head_hook, {}),
    "a forward pre-hook on lm_head": (_head_pre_hook, {}),
    "an adapter-wrapped lm_head": (_wrapped, {}),
    "a subclass of nn.Linear": (_subclassed, {}),
    "lm_head in fp32": (_head_other_type, {}),
    "lm_head on another device": (_head_elsewhere, {}),
    "lm_head rows not 16-byte aligned": (_head_strided, {}),
    "a hook on norm": (_norm_hook, {}),
    "norm of another class": (_norm_other_class, {}),
    "norm in fp32": (_norm_other_type, {}),
    "a forward hook on the stack": (_stack_hook, {}),
    "a second pre-hook on the stack": (_stack_pre_hook, {}),
    "a vocabulary of one": (_one_token_vocabulary, {}),
    "lm_head of another hidden size": (_other_hidden_size, {}),
    "the switch off": (_switch_off, {}),
    "the whole-stack switch off": (_stack_switch_off, {}),
    "a hook on a layer (the stack route says no)": (_layer_hook, {}),
}


@pytest.mark.parametrize("name", list(FLIPS))
def test_one_flip_sends_the_call_to_todays_path(stub, name):
    change, ask = FLIPS[name]
    m, cache = _stack(head=True)
    assert _ask(m, cache) == "head"
    if change is not None:
        change(m, cache)
    assert _ask(m, cache, **ask) == "stock"


def test_hidden_sizes_the_product_does_not_take(stub):
    """E = 192 (Phi-3 stub) is a multiple of 32: admitted; lm_head's E must be a multiple of 32 up to 8192"""
    m, cache = _stack(window=32, head=True)
    assert m.config.hidden_size == 192 and _ask(m, cache) == "head"
    for E in (200, 8192 + 32):
        m.lm_head = torch.nn.Linear(E, 8, bias=False).to(bf)
        m.model.norm.weight = torch.nn.Parameter(torch.ones(E, dtype=bf))
        assert _ask(m, cache) == "stock", E


def test_head_form_and_its_fallback():
    assert prefill.head_form("elem", 4096) == (0, False) and prefill.head_form("elem", 96) == (0, False)
    assert prefill.head_form("fp8", 4096) == (1, False) and prefill.head_form("fp8", 64) == (1, False)
    assert prefill.head_form("fp8", 96) == (0, True) and prefill.head_form("fp8", 32) == (0, True)
    assert prefill.head_form("fp4", 4096) == (2, False) and prefill.head_form("fp4", 128) == (2, False)
    assert prefill.head_form("fp4", 192) == (0, True) and prefill.head_form("fp4", 64) == (0, True)
    with pytest.raises(ValueError, match="u2_fused_head_form"):
        prefill.head_form("int8", 4096)
    assert prefill.HEAD_FORMS == {"elem": 0, "fp8": 1, "fp4": 2}


def test_the_switch_its_config_attribute_and_what_goes_with_it():
    s = {s.kw: s for s in prefill.SWITCHES}["head"]
    assert s.config == "u2_fused_decode_head" and s.default is False and s.implies == ("stack_decode",) and s.field == "head"
    m, _ = _stack(head=True)
    m.__dict__["_u2_head"] = "kept"
    prefill.enable_fused_prefill(m, stack_decode=True)               # the switch goes off: what the head kept goes with it
    assert not m.model._u2_stack.head and m.model._u2_stack.stack and "_u2_head" not in m.__dict__
    prefill.enable_fused_prefill(m, head=True)
    m.__dict__["_u2_head"] = "kept"
    prefill.disable_fused_prefill(m)
    assert "_u2_head" not in m.__dict__ and prefill.head_weights(m) is None


def test_a_call_that_is_not_admitted_goes_on_as_it_came_and_is_counted():
    """CPU tensors: `head_forward` answers None and counts the fallback; with the switch off it counts nothing"""
    m, cache = _stack(head=True)
    ids = torch.zeros(B, 1, dtype=torch.int64)
    n0 = dict(prefill.head_stats)
    assert prefill.head_forward(m, ids, None, None, cache, None, True, None, {}) is None
    assert prefill.head_stats == {**n0, "fallback": n0["fallback"] + 1}
    assert prefill.head_forward(m, ids, None, None, cache, None, True, ids, {}) is None      # labels
    assert prefill.head_forward(m, None, None, None, cache, None, True, None, {}) is None     # neither ids nor embeddings
    assert prefill.head_stats == {**n0, "fallback": n0["fallback"] + 3}
    prefill.enable_fused_prefill(m, stack_decode=True)
    assert prefill.head_forward(m, ids, None, None, cache, None, True, None, {}) is None
    assert prefill.head_stats == {**n0, "fallback": n0["fallback"] + 3}
    assert set(prefill.head_stats) == {"head", "fallback", "form_fallback"}


def test_signatures_list_the_new_exports():
    for name in ("u2tok_decode_head", "u2tok_decode_head_workspace_bytes", "u2tok_decoder_decode_stack_head",
                 "u2tok_decoder_decode_stack_head_workspace_bytes", "u2tok_sample_warp_split", "u2tok_sample_warp_split_workspace_bytes",
                 "u2tok_sample_warp_split_launches"):
        assert name in _lib.SIGNATURES, name
    assert C.sizeof(_lib.DecodeHead) == 3 * 8 + 4 * 4 + 2 * 8
    # u2tok_decoder_decode_stack itself keeps its signature; the split warper has u2tok_sample_warp's
    assert len(_lib.SIGNATURES["u2tok_decoder_decode_stack"][1]) == 16
    assert _lib.SIGNATURES["u2tok_sample_warp_split"] == _lib.SIGNATURES["u2tok_sample_warp"]


def test_split_warper_refuses_what_the_warper_refuses_and_fixes_its_launches_from_the_parameters(lib):
    V, rows = 1000, 2
    need = lib.u2tok_sample_warp_split_workspace_bytes(rows, V)
    assert need > lib.u2tok_sample_warp_workspace_bytes(rows, V) > 0
    assert lib.u2tok_sample_warp_split_workspace_bytes(0, V) == 0 and lib.u2tok_sample_warp_split_workspace_bytes(rows, 1) == 0

    def call(x=P, ld_in=V, out=P, ld_out=V, rows=rows, V=V, T=0.7, k=0, p=0.9, mk=1, ws=P, nbytes=need):
        return lib.u2tok_sample_warp_split(x, ld_in, out, ld_out, rows, V, T, k, p, mk, ws, nbytes, None)

    bad = [call(x=None), call(out=None), call(ws=None), call(rows=0), call(V=1), call(T=0.0), call(T=-1.0), call(p=0.0), call(p=1.5),
           call(mk=0), call(k=-1), call(ld_in=V - 1), call(ld_out=V - 1), call(x=P + 2), call(out=P + 1), call(ws=P + 2)]
    assert bad == [ERR_ARG] * len(bad)
    assert call(nbytes=need - 1) == ERR_WS and call(nbytes=lib.u2tok_sample_warp_workspace_bytes(rows, V)) == ERR_WS
    L = lib.u2tok_sample_warp_split_launches
    assert (L(V, 0, 1.0, 1), L(V, 5, 1.0, 1), L(V, 0, 0.9, 1), L(V, 0, 0.9, 2), L(V, 50, 0.95, 2)) == (3, 7, 11, 19, 23)
    assert L(V, V, 1.0, 1) == 3 and L(V, 0, 1.0, 3) == 3 and L(V, 2, 1.0, 5) == 7       # k >= V: no stage; k = max(top_k, min_keep)


# ---------------------------------------------------------------------------------------------------------------- the C entries
@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


P = 1 << 20       # a 256-byte aligned address that is never dereferenced
ERR_ARG, ERR_WS = -1, -3
E, V = 256, 1000


def _desc(**kw):
    d = dict(w_norm=P, W=P, scale=None, E=E, V=V, wform=0, eps=1e-6, ldw=0, lds=0)
    d.update(kw)
    return _lib.DecodeHead(**d)


def test_head_entry_refuses_before_any_launch(lib):
    need = lib.u2tok_decode_head_workspace_bytes(B, E)
    assert need == 1024 and lib.u2tok_decode_head_workspace_bytes(64, 4096) == 64 * 4096 * 2
    assert lib.u2tok_decode_head_workspace_bytes(0, E) == 0 and lib.u2tok_decode_head_workspace_bytes(65, E) == 0
    assert lib.u2tok_decode_head_workspace_bytes(B, 0) == 0

    def call(desc, x=P, ldx=E, rows=B, logits=P, ldl=V, ws=P, nbytes=need):
        return lib.u2tok_decode_head(C.byref(desc) if desc is not None else None, x, ldx, rows, logits, ldl, ws, nbytes, None)

    cases = {
        "V = 1": call(_desc(V=1)), "null W": call(_desc(W=None)), "null norm weight": call(_desc(w_norm=None)),
        "misaligned W": call(_desc(W=P + 8)), "misaligned norm weight": call(_desc(w_norm=P + 8)),
        "unknown form": call(_desc(wform=3)), "negative form": call(_desc(wform=-1)),
        "e4m3 without scales": call(_desc(wform=1)), "e2m1 without scales": call(_desc(wform=2)),
        "E % 128 != 0 with e2m1": call(_desc(wform=2, scale=P, E=192), ldx=192, nbytes=4096),
        "E % 64 != 0 with e4m3": call(_desc(wform=1, scale=P, E=96), ldx=96, nbytes=4096),
        "E % 32 != 0": call(_desc(E=24), ldx=24, nbytes=4096),
        "E > 8192": call(_desc(E=8192 + 32), ldx=8192 + 32, nbytes=1 << 20),
        "a short e2m1 scale row": call(_desc(wform=2, scale=P, lds=E // 32 - 1)),
        "a misaligned e4m3 scale": call(_desc(wform=1, scale=P + 2)),
        "a weight row shorter than E": call(_desc(ldw=E - 8)),
        "x rows shorter than E": call(_desc(), ldx=E - 8), "logits rows shorter than V": call(_desc(), ldl=V - 1),
        "no rows": call(_desc(), rows=0), "65 rows": call(_desc(), rows=65, nbytes=1 << 20),
        "null head": call(None), "null x": call(_desc(), x=None), "null logits": call(_desc(), logits=None),
        "misaligned logits": call(_desc(), logits=P + 2), "null workspace": call(_desc(), ws=None),
        "misaligned workspace": call(_desc(), ws=P + 8),
    }
    assert {k: v for k, v in cases.items() if v != ERR_ARG} == {}
    assert call(_desc(), nbytes=need - 1) == ERR_WS and call(_desc(wform=2, scale=P, E=128), ldx=128, nbytes=0) == ERR_WS


def _layers(n=NL, E=E):
    cfgs = [_lib.DecodeConfig(B=B, E=E, Hq=4, Hkv=2, D=64, I=512, eps=1e-6, qk_eps=1e-6, scale=0.125) for _ in range(n)]
    lays = [_lib.DecodeLayer(w_in_norm=P, Wqkv=P, Wo=P, w_post_norm=P, Wgu=P, Wdown=P) for _ in range(n)]
    arr = (_lib.DecodeStackLayer * n)()
    for i in range(n):
        arr[i].cfg, arr[i].layer = C.addressof(cfgs[i]), C.addressof(lays[i])
        arr[i].k_cache = arr[i].v_cache = P
        arr[i].kv_stride, arr[i].s_off, arr[i].k_first, arr[i].T = 256 * 64, T, 0, T + 1
    return arr, cfgs, lays


def test_stack_head_entry_refuses_layers_and_head_before_any_launch(lib):
    arr, cfgs, lays = _layers()
    good = _desc()
    sneed = lib.u2tok_decoder_decode_stack_workspace_bytes(arr, NL)
    need = lib.u2tok_decoder_decode_stack_head_workspace_bytes(arr, NL, C.byref(good))
    assert sneed > 0 and need == sneed + lib.u2tok_decode_head_workspace_bytes(B, E)
    assert lib.u2tok_decoder_decode_stack_head_workspace_bytes(arr, NL, None) == 0
    assert lib.u2tok_decoder_decode_stack_head_workspace_bytes(None, NL, C.byref(good)) == 0
    assert lib.u2tok_decoder_decode_stack_head_workspace_bytes(arr, NL, C.byref(_desc(E=512))) == 0

    def call(desc=good, layers=arr, n=NL, logits=P, ldl=V, ws=P, nbytes=need, out=P):
        return lib.u2tok_decoder_decode_stack_head(layers, n, P, P, P, 1, 64, 0, None, 0, out, C.byref(desc) if desc is not None else None,
                                                   logits, ldl, ws, nbytes, None)

    # the head's refusals behind a stack the walk accepts
    for what, desc in (("V = 1", _desc(V=1)), ("misaligned W", _desc(W=P + 8)), ("null W", _desc(W=None)),
                       ("null norm weight", _desc(w_norm=None)), ("e2m1 without scales", _desc(wform=2)),
                       ("another hidden size", _desc(E=512)), ("unknown form", _desc(wform=7))):
        assert call(desc) == ERR_ARG, what
    assert call(None) == ERR_ARG and call(logits=None) == ERR_ARG and call(ldl=V - 1) == ERR_ARG and call(ws=None) == ERR_ARG
    assert call(ws=P + 128) == ERR_ARG and call(out=None) == ERR_ARG
    assert call(nbytes=need - 1) == ERR_WS and call(nbytes=sneed) == ERR_WS and call(nbytes=sneed - 1) == ERR_WS
    # E % 128 != 0 with form 2: layers of E = 192 in the element type, a head of e2m1 codes
    arr2, cfgs2, lays2 = _layers(E=192)
    d2 = _desc(E=192, wform=2, scale=P)
    need2 = lib.u2tok_decoder_decode_stack_head_workspace_bytes(arr2, NL, C.byref(d2))
    assert need2 > 0 and call(_desc(E=192), layers=arr2, nbytes=need2 - 1) == ERR_WS      # (the walk takes these layers)
    assert call(d2, layers=arr2, nbytes=need2) == ERR_ARG
    # the layers' refusals with a good head
    lays[1].Wdown = None
    assert call() == ERR_ARG
    lays[1].Wdown = P
    arr[0].k_cache = None
    assert call() == ERR_ARG
    arr[0].k_cache = P
    assert call(n=0) == ERR_ARG and call(layers=None) == ERR_ARG
