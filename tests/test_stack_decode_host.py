"""CPU: the admission of the whole-stack decode step (prefill.stack_route), one flip of an admitted baseline at a time; the wrapper
on the decoder stack's forward coming and going with the switch; and the two C entries' refusals and workspace sizing, which need
no GPU.  The stub models are those of tests/test_decoder_route_host.py; `stack_route` takes the call's shape, type and device flag,
so no tensor has to claim a GPU."""
import ctypes as C
import types

import pytest
import torch

from test_decoder_route_host import _model, _stock
from u2tokenizer_amd import _lib, prefill

bf = torch.bfloat16
NL, B, T = 2, 2, 5


class _Dec:   # what stack_route reads of `_decode_state`'s first result
    def __init__(self, ok=True):
        self.ok, self.hd = ok, 64


@pytest.fixture
def stub(monkeypatch):
    """_decode_state without a GPU: the descriptor's verdict alone (`ok` per layer index, flipped by the cases)"""
    ok = {}
    monkeypatch.setattr(prefill, "_decode_state", lambda layer, B, device, pr: (_Dec(ok.get(layer.self_attn.layer_idx, True)), {}))
    return ok


def _stack(window=None, **kw):
    """a patched 2-layer stack with the switch on, and a plain cache whose layers are the append-in-place layers a fused prefill
    leaves, holding T positions of B sequences"""
    from transformers.cache_utils import DynamicCache
    m = _model("phi3", hidden=192, head_dim=96, window=window, num_hidden_layers=NL) if window else _model(num_hidden_layers=NL)
    prefill.enable_fused_prefill(m, **{"stack_decode": True, **kw})
    cache = DynamicCache()
    cls = prefill._append_layer_class()
    for layer in m.model.layers:
        att = layer.self_attn
        kv = torch.zeros(B, m.config.num_key_value_heads, T, att.head_dim, dtype=bf)
        lay = cls()
        lay.update(kv, kv)
        cache.layers.append(lay)
    return m, cache


def _ask(m, cache, B=B, S=1, dtype=bf, cuda=True, grad=False, plan=None, **kw):
    call = dict(past_key_values=cache, use_cache=True, output_hidden_states=False, output_attentions=False)
    call.update(kw)
    return prefill.stack_route(m.model, B, S, dtype, cuda, call, grad, plan)


def test_the_admitted_baseline(stub):
    m, cache = _stack()
    plan = []
    assert _ask(m, cache, plan=plan) == "stack"
    assert [p[0] for p in plan] == list(m.model.layers) and all(p[5] is None for p in plan)
    m, cache = _stack(window=32)
    plan = []
    assert _ask(m, cache, plan=plan) == "stack" and [p[5] for p in plan] == [32, 32]


def _hook(m, c):
    m.model.layers[1].register_forward_hook(lambda *a: None)


def _pre_hook(m, c):
    m.model.layers[0].register_forward_pre_hook(lambda *a: None)


def _inner_hook(m, c):
    m.model.layers[1].mlp.register_forward_hook(lambda *a: None)      # (route() itself answers "stock" for that layer)


def _unpatched(m, c):
    layer = m.model.layers[1]
    layer.forward = layer.__dict__.pop("_u2_prefill").orig


def _plain_layer(m, c):
    from transformers.cache_utils import DynamicLayer
    lay = DynamicLayer()
    lay.update(c.layers[1].keys, c.layers[1].values)
    c.layers[1] = lay


def _sliding_layer(m, c):
    from transformers.cache_utils import DynamicSlidingWindowLayer
    lay = DynamicSlidingWindowLayer(sliding_window=32)
    lay.update(c.layers[0].keys, c.layers[0].values)
    c.layers[0] = lay


def _other_cache(m, c):
    from transformers.cache_utils import DynamicCache

    class Other(DynamicCache):
        pass

    c.__class__ = Other


def _offloaded(m, c):
    c.offloading = True


def _other_batch(m, c):
    kv = torch.zeros(B + 1, m.config.num_key_value_heads, T, m.model.layers[0].self_attn.head_dim, dtype=bf)
    c.layers[0].keys = c.layers[0].values = kv


def _padded_call(m, c):
    m.model._u2_stack.pad, m.model._u2_stack.pad_shape = ("left", torch.zeros(B, dtype=torch.int32), None), (B, T + 1)


# what the case changes: a function of (model, cache) applied before the question, and / or other arguments of the question
FLIPS = {
    "grad enabled": (None, dict(grad=True)),
    "two positions": (None, dict(S=2)),
    "a CPU input": (None, dict(cuda=False)),
    "another type than the weights'": (None, dict(dtype=torch.float16)),
    "use_cache off": (None, dict(use_cache=False)),
    "no cache": (None, dict(past_key_values=None)),
    "output_hidden_states": (None, dict(output_hidden_states=True)),
    "output_attentions": (None, dict(output_attentions=True)),
    "a keyword route() refuses": (None, dict(past_key_value=None)),
    "more than 16 sequences without wide_decode": (None, dict(B=17)),
    "a padded call without `padded`": (_padded_call, {}),
    "a forward hook on a layer": (_hook, {}),
    "a forward pre-hook on a layer": (_pre_hook, {}),
    "a hook inside a layer": (_inner_hook, {}),
    "one unpatched layer": (_unpatched, {}),
    "a plain DynamicLayer": (_plain_layer, {}),
    "a DynamicSlidingWindowLayer": (_sliding_layer, {}),
    "another cache class": (_other_cache, {}),
    "an offloaded cache": (_offloaded, {}),
    "a layer holding another batch": (_other_batch, {}),
}


@pytest.mark.parametrize("name", list(FLIPS))
def test_one_flip_sends_the_call_to_the_layers(stub, name):
    change, ask = FLIPS[name]
    m, cache = _stack(window=32 if "Sliding" in name else None)
    assert _ask(m, cache) == "stack"
    if change is not None:
        change(m, cache)
    assert _ask(m, cache, **ask) == "layers"


def test_switches_route_keeps_deciding(stub):
    """the switch itself; the fused decode step off; a descriptor the step does not take; and what widens route() widens this"""
    m, cache = _stack()
    m.model._u2_stack.stack = False
    assert _ask(m, cache) == "layers"
    m, cache = _stack(decode=False)
    assert _ask(m, cache) == "layers"
    m, cache = _stack()
    stub[1] = False
    assert _ask(m, cache) == "layers"
    stub.clear()
    m, cache = _stack(padded=True)
    _padded_call(m, cache)
    assert _ask(m, cache) == "stack"


def test_the_wrapper_comes_and_goes_with_the_switch():
    m = _model(num_hidden_layers=NL)
    base = m.model
    assert "forward" not in base.__dict__
    prefill.enable_fused_prefill(m, stack_decode=True)
    assert base.__dict__["forward"].__func__ is prefill._stack_forward and base._u2_stack.stack
    base._u2_stack.scratch[(1, "cpu", 0)] = sc = {"qkv": None, "stack_ws": "kept", "stack_T": 1, "stack_arr": "kept", "stack_keep": ["kept"]}
    prefill.enable_fused_prefill(m)                      # a second call without the keyword: off, and what the route kept is freed
    assert "forward" not in base.__dict__ and "_u2_stack_run" not in base.__dict__ and not base._u2_stack.stack
    assert sc == {"qkv": None}
    assert all(prefill.is_patched(layer) for layer in base.layers)
    prefill.enable_fused_prefill(m, stack_decode=True)
    prefill.enable_fused_prefill(m, stack_decode=True)   # (idempotent: one wrapper, the stack's own forward beneath it)
    assert base._u2_stack_run.had is prefill._MISSING and base._u2_stack_run.orig.__func__ is type(base).forward
    prefill.disable_fused_prefill(m)
    assert "forward" not in base.__dict__ and "_u2_stack_run" not in base.__dict__ and "_u2_stack" not in base.__dict__
    # a stack whose forward was an instance attribute gets that very object back
    own = types.MethodType(lambda self, *a, **k: "own", base)
    base.forward = own
    prefill.enable_fused_prefill(m, stack_decode=True)
    assert base.forward is not own
    prefill.disable_fused_prefill(m)
    assert base.forward is own


def test_a_call_that_is_not_admitted_runs_the_stacks_own_forward():
    """CPU tensors: the wrapper hands the call on with its arguments as they came; the layers' stock forwards run."""
    m = _model(num_hidden_layers=NL)
    calls = []
    for layer in m.model.layers:
        layer._calls = calls
        layer.forward = types.MethodType(_stock, layer)
    prefill.enable_fused_prefill(m, stack_decode=True)
    n0 = dict(prefill.stack_stats)
    with torch.no_grad():
        out = m.model(torch.zeros(1, 1, dtype=torch.int64), use_cache=True)
    assert calls == ["stock"] * NL and out.last_hidden_state.shape == (1, 1, m.config.hidden_size)
    assert prefill.stack_stats == n0
    prefill.disable_fused_prefill(m)


# ---------------------------------------------------------------------------------------------------------------- the C entries
@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


def _descriptors(n=3, Bn=2, E=256, T=40, wform=0):
    P = 1 << 20   # a 256-byte aligned address that is never dereferenced
    cfgs = [_lib.DecodeConfig(B=Bn, E=E, Hq=4, Hkv=2, D=64, I=512, eps=1e-6, qk_eps=1e-6, scale=0.125, wform=wform) for _ in range(n)]
    lays = [_lib.DecodeLayer(**{f: P for f in ("w_in_norm", "Wqkv", "Wo", "w_post_norm", "Wgu", "Wdown")}) for _ in range(n)]
    arr = (_lib.DecodeStackLayer * n)()
    for i in range(n):
        s = arr[i]
        s.cfg, s.layer, s.k_cache, s.v_cache = C.addressof(cfgs[i]), C.addressof(lays[i]), P, P
        s.kv_stride, s.s_off, s.k_first, s.T = 256 * 64, T - 1, 0, T
    return arr, cfgs, lays


def test_stack_workspace_covers_the_layers_and_the_hidden_rows(lib):
    n, Bn, E = 3, 2, 256
    arr, cfgs, _ = _descriptors(n, Bn, E)
    last = 0
    for T in (1, 40, 512, 2048, 8192):
        for i in range(n):
            arr[i].T, arr[i].s_off = T, T - 1
        need = lib.u2tok_decoder_decode_stack_workspace_bytes(arr, n)
        per_layer = lib.u2tok_decoder_decode_workspace_bytes(C.byref(cfgs[0]), T)
        assert per_layer > 0 and need >= per_layer + 2 * Bn * E * 2
        assert need >= last                                                # monotone in T
        last = need
    arr[1].T = 16384                                                       # the largest layer decides
    assert lib.u2tok_decoder_decode_stack_workspace_bytes(arr, n) >= lib.u2tok_decoder_decode_workspace_bytes(C.byref(cfgs[0]), 16384)
    assert lib.u2tok_decoder_decode_stack_workspace_bytes(arr, 0) == 0 and lib.u2tok_decoder_decode_stack_workspace_bytes(None, n) == 0
    arr[1].T = 0
    assert lib.u2tok_decoder_decode_stack_workspace_bytes(arr, n) == 0
    arr[1].T = 40
    cfgs[2].E = 512                                                        # one hidden size for the whole stack
    assert lib.u2tok_decoder_decode_stack_workspace_bytes(arr, n) == 0
    cfgs[2].E = E
    arr[2].cfg = None
    assert lib.u2tok_decoder_decode_stack_workspace_bytes(arr, n) == 0


def test_null_and_malformed_arguments_are_refused_not_dereferenced(lib):
    """(no GPU: every one of these returns before anything is launched or read)"""
    ERR_ARG, ERR_WS = -1, -3
    n = 3
    arr, cfgs, lays = _descriptors(n)
    need = lib.u2tok_decoder_decode_stack_workspace_bytes(arr, n)
    P = 1 << 20
    # layers, n, x, cos, sin, cos_sin_f32, cs_ld, batched, kv_start, w_final_norm, final_eps, tail_norm, out, workspace, bytes, stream
    args = [arr, n, P, P, P, 1, 64, 0, None, P, 1e-6, 0, P, P, need, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.u2tok_decoder_decode_stack(*a)

    assert call(a0=None) == ERR_ARG and call(a1=0) == ERR_ARG and call(a1=-1) == ERR_ARG
    for i in (2, 3, 4, 12, 13):                                            # x, cos, sin, out, workspace
        assert call(**{f"a{i}": None}) == ERR_ARG, i
    assert call(a13=P + 16) == ERR_ARG                                     # workspace not 256-byte aligned
    assert call(a14=need - 1) == ERR_WS and call(a14=0) == ERR_WS
    for tail in (0, 1):
        for f in ("Wqkv", "Wdown", "w_post_norm", "w_in_norm"):            # a null weight in the LAST layer
            setattr(lays[2], f, None)
            assert call(a11=tail) == ERR_ARG, f
            setattr(lays[2], f, P)
    arr[1].k_cache = None
    assert call() == ERR_ARG
    arr[1].k_cache = P
    arr[1].kv_stride = 39 * 64                                             # no room for the row at s_off
    assert call() == ERR_ARG
    arr[1].kv_stride = 256 * 64
    arr[1].k_first = 1                                                     # reads past the step's own row
    assert call() == ERR_ARG
    arr[1].k_first = 0
    lays[0].scale_o = P                                                    # some, not all, of the four scales
    assert call() == ERR_ARG
    lays[0].scale_o = None
    cfgs[1].wform = 2                                                      # e2m1 without block scales
    assert call() == ERR_ARG
    cfgs[1].wform = 0
    assert call(a7=1, a8=P + 2) == ERR_ARG                                 # kv_start misaligned
    assert call(a8=P) == ERR_ARG                                           # kv_start without the batched attention
    # the tail norm's entry
    # A, W, C, bias, R, M, N, K, lda, ldw, ldc, ldr, flags, wform, scale, lds, w_norm, eps, Yn, ldn, ticket, stream
    rn = [P, P, P, None, P, 5, 256, 128, 128, 128, 256, 256, 8, 0, None, 0, P, 1e-6, P, 256, P, None]

    def norm(**kw):
        a = list(rn)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.u2tok_gemm_rows_norm(*a)

    for i in (0, 1, 2, 4, 16, 18, 20):                                     # A, W, C, R, w_norm, Yn, ticket
        assert norm(**{f"a{i}": None}) == ERR_ARG, i
    assert norm(a20=P + 2) == ERR_ARG                                      # ticket not 4-byte aligned
    assert norm(a12=512) == ERR_ARG and norm(a12=0) == ERR_ARG             # the pair form; no residual
    assert norm(a12=8 | 16) == ERR_ARG                                     # fp32 C
    assert norm(a13=3) == ERR_ARG and norm(a13=1) == ERR_ARG               # an unknown form; codes without scales
    assert norm(a6=4104, a10=4104, a11=4104, a19=4104) == ERR_ARG          # a row wider than the tail holds
    assert norm(a6=20, a10=24, a11=24, a19=24) == ERR_ARG                  # N % 8 != 0
    assert norm(a19=248) == ERR_ARG                                        # Yn rows shorter than N
