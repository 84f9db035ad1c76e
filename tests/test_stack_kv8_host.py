"""CPU: the whole-stack decode step on the FP8 (e4m3) KV cache (opt-in, `enable_fused_prefill(model, stack_kv8=True)`): the switch
record and its place in the table; what the keyword and the config attribute set; `stack_route` / `head_route` on caches of
`Kv8Layer`s -- the stub models and the fake-`is_cuda` tensor are those of tests/test_decoder_route_host.py --; and, through ctypes
without a GPU, the workspace sizing and the refusals of u2tok_decoder_decode_stack_kv8 / _stack_head_kv8 and
u2tok_qk_norm_rope_kv8, every one of which answers before anything is launched or dereferenced."""
import ctypes as C
import inspect

import pytest
import torch

from test_decoder_route_host import _FakeCuda, _model
from u2tokenizer_amd import _lib, prefill
from u2tokenizer_amd import language_model as LM

bf = torch.bfloat16
NL, B, T = 2, 2, 5


# ------------------------------------------------------------------------------------------------------------------ the switch
def test_the_switch_record_and_its_place_in_the_table():
    kws = [s.kw for s in prefill.SWITCHES]
    s = prefill.SWITCHES[kws.index("stack_kv8")]
    assert (s.field, s.config, s.default, s.implies, s.needs, s.frees) == \
        ("stack8", "u2_fused_stack_kv_fp8", False, ("stack_decode", "kv8"), (), ())
    assert kws[-3:] == ["stack_kv8", "kv8_continued", "kv8"]
    assert "u2tok_decoder_decode_stack_kv8" in s.doc and "stack_kv8_stats" in s.doc
    by = {x.kw: x for x in prefill.SWITCHES}
    assert "stack_kv8" in by["kv8"].doc and "stack_kv8" in by["kv8_continued"].doc
    params = list(inspect.signature(prefill.enable_fused_prefill).parameters)
    assert params.index("stack_kv8") == params.index("kv8_continued") - 1
    assert "stack8" in prefill._StackState.__dataclass_fields__
    assert prefill.stack_kv8_stats.keys() == {"decode", "padded_decode"}


def test_the_keyword_sets_the_three_fields():
    m = _model()
    prefill.enable_fused_prefill(m, stack_kv8=True)
    st = m.model._u2_stack
    assert st.stack8 and st.stack and st.kv8 and not st.head and not st.kv8x and not st.continued
    assert "_u2_stack_run" in m.model.__dict__                 # (the stack's forward is wrapped, as with stack_decode)
    prefill.enable_fused_prefill(m, stack_decode=True, kv8=True)
    assert not st.stack8 and st.stack and st.kv8
    prefill.enable_fused_prefill(m)
    assert not st.stack8 and not st.stack and not st.kv8
    prefill.disable_fused_prefill(m)


def test_the_config_attribute_sets_the_three_fields():
    cfg = LM.u2Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                           num_key_value_heads=2, head_dim=16)
    cfg.u2_fused_stack_kv_fp8 = True
    m = LM.u2Qwen3ForCausalLM(cfg).to(bf).eval()
    layer = m.model.layers[0]
    p0 = next(layer.parameters())
    layer.parameters = lambda *a, **k: iter([p0.detach().as_subclass(_FakeCuda)])
    with torch.no_grad():
        m(inputs_embeds=torch.zeros(1, 3, 64, dtype=bf))
    st = m.model._u2_stack
    assert st.stack8 and st.stack and st.kv8 and not st.head


# ------------------------------------------------------------------------------------------------------------------ the routes
class _Dec:   # what stack_route reads of `_decode_state`'s first result
    ok, hd = True, 64


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(prefill, "_decode_state", lambda layer, B, device, pr: (_Dec(), {}))


def _kv8_layer(m, Bn, fake=True):
    kv = torch.zeros(Bn, m.config.num_key_value_heads, T, m.model.layers[0].self_attn.head_dim, dtype=m.dtype)
    lay = prefill.Kv8Layer()
    lay.update(kv, kv)
    if fake:
        lay._kc = lay._kc.as_subclass(_FakeCuda)
    return lay


def _append_layer(m, Bn):
    kv = torch.zeros(Bn, m.config.num_key_value_heads, T, m.model.layers[0].self_attn.head_dim, dtype=m.dtype)
    lay = prefill._append_layer_class()()
    lay.update(kv, kv)
    return lay


def _stack(kinds=("kv8", "kv8"), batch=B, model_kw=None, **sw):
    from transformers.cache_utils import DynamicCache
    m = _model(num_hidden_layers=NL, **(model_kw or {}))
    prefill.enable_fused_prefill(m, **{"stack_kv8": True, **sw})
    cache = DynamicCache()
    cache.layers.extend(_kv8_layer(m, batch) if k == "kv8" else _append_layer(m, batch) for k in kinds)
    return m, cache


def _ask(m, cache, Bn=B, plan=None):
    call = dict(past_key_values=cache, use_cache=True, output_hidden_states=False, output_attentions=False)
    return prefill.stack_route(m.model, Bn, 1, bf, True, call, False, plan)


def _ask_head(m, cache, Bn=B):
    call = dict(past_key_values=cache, use_cache=True, output_hidden_states=False, output_attentions=False)
    return prefill.head_route(m, Bn, 1, bf, True, call, False)


def test_a_cache_of_kv8_layers_takes_the_stack(stub):
    m, cache = _stack()
    plan = []
    assert _ask(m, cache, plan=plan) == "stack" and [p[0] for p in plan] == list(m.model.layers)
    assert _ask_head(m, cache) == "stock"                       # (the head switch is off)
    m, cache = _stack(head=True)
    assert _ask(m, cache) == "stack" and _ask_head(m, cache) == "head"
    # the append-in-place cache keeps its route with the new switch on
    m, cache = _stack(kinds=("append", "append"), head=True)
    assert _ask(m, cache) == "stack" and _ask_head(m, cache) == "head"


@pytest.mark.parametrize("kinds", [("kv8", "append"), ("append", "kv8")])
def test_a_mixed_cache_keeps_the_layers(stub, kinds):
    m, cache = _stack(kinds=kinds, head=True)
    assert _ask(m, cache) == "layers" and _ask_head(m, cache) == "stock"


def test_what_the_decode_route_refuses_keeps_the_layers(stub):
    m, cache = _stack(model_kw=dict(num_attention_heads=34, num_key_value_heads=2), head=True)   # 17 query heads per kv head
    assert _ask(m, cache) == "layers" and _ask_head(m, cache) == "stock"
    m, cache = _stack(batch=B + 1, head=True)                   # a cache of another batch
    assert _ask(m, cache) == "layers" and _ask_head(m, cache) == "stock"
    m, cache = _stack(head=True)
    cache.layers[1] = _kv8_layer(m, B, fake=False)              # one layer's codes on the CPU
    assert _ask(m, cache) == "layers"
    m, cache = _stack(head=True)
    cache.layers[1] = prefill.Kv8Layer()                        # an empty layer
    assert _ask(m, cache) == "layers"
    m, cache = _stack(head=True)
    assert _ask(m, cache, Bn=17) == "layers"                    # more than 16 sequences without wide_decode


def test_the_switch_off_keeps_todays_answer(stub):
    m, cache = _stack(head=True)
    prefill.enable_fused_prefill(m, kv8=True, stack_decode=True, head=True, wide_decode=True)
    assert _ask(m, cache) == "layers" and _ask_head(m, cache) == "stock"
    prefill.enable_fused_prefill(m, stack_kv8=True, head=True)
    assert _ask(m, cache) == "stack" and _ask_head(m, cache) == "head"
    m.model._u2_stack.stack8 = False
    assert _ask(m, cache) == "layers"


def test_the_scratch_of_both_kinds_goes_with_the_switch():
    m = _model(num_hidden_layers=NL)
    prefill.enable_fused_prefill(m, stack_kv8=True)
    m.model._u2_stack.scratch[(1, "cpu", 0)] = sc = {"qkv": None, "stack_ws": 1, "stack_T": 1, "stack_arr8": 1, "stack_keep8": [1],
                                                      "stack_arr": 1, "stack_keep": [1], "stack_head": True}
    prefill.enable_fused_prefill(m)
    assert sc == {"qkv": None}
    prefill.disable_fused_prefill(m)


# ---------------------------------------------------------------------------------------------------------------- the C entries
ERR_ARG, ERR_WS = -1, -3
P = 1 << 20   # a 256-byte aligned address that is never dereferenced


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


def _descriptors(n=3, Bn=2, E=256, Tn=40, cap=256, Hq=4):
    cfgs = [_lib.DecodeConfig(B=Bn, E=E, Hq=Hq, Hkv=2, D=64, I=512, eps=1e-6, qk_eps=1e-6, scale=0.125, wform=0) for _ in range(n)]
    lays = [_lib.DecodeLayer(**{f: P for f in ("w_in_norm", "Wqkv", "Wo", "w_post_norm", "Wgu", "Wdown")}) for _ in range(n)]
    arr8, arr16 = (_lib.DecodeStackLayerKv8 * n)(), (_lib.DecodeStackLayer * n)()
    for i in range(n):
        s = arr8[i]
        s.cfg, s.layer = C.addressof(cfgs[i]), C.addressof(lays[i])
        s.k_codes, s.v_codes, s.k_scales, s.v_scales, s.capacity = P, P, P, P, cap
        s.s_off, s.k_first, s.T = Tn - 1, 0, Tn
        t = arr16[i]
        t.cfg, t.layer, t.k_cache, t.v_cache = s.cfg, s.layer, P, P
        t.kv_stride, t.s_off, t.k_first, t.T = cap * 64, Tn - 1, 0, Tn
    return arr8, arr16, cfgs, lays


def _head(E=256, V=1000, **kw):
    f = dict(w_norm=P, W=P, scale=None, E=E, V=V, wform=0, eps=1e-6, ldw=0, lds=0)
    f.update(kw)
    return _lib.DecodeHead(**f)


def test_the_struct_has_the_headers_layout():
    f = dict((n, (getattr(_lib.DecodeStackLayerKv8, n).offset, getattr(_lib.DecodeStackLayerKv8, n).size))
             for n, _ in _lib.DecodeStackLayerKv8._fields_)
    assert [f[n] for n in ("cfg", "layer", "k_codes", "v_codes", "k_scales", "v_scales")] == [(8 * i, 8) for i in range(6)]
    assert [f[n] for n in ("capacity", "s_off", "k_first", "T")] == [(48 + 4 * i, 4) for i in range(4)]
    assert C.sizeof(_lib.DecodeStackLayerKv8) == 64


def test_workspace_bytes_are_the_16_bit_entries(lib):
    n = 3
    arr8, arr16, cfgs, _ = _descriptors(n)
    head = _head()
    for Tn in (1, 40, 512, 2048, 8192):
        for i in range(n):
            arr8[i].T = arr16[i].T = Tn
            arr8[i].s_off = arr16[i].s_off = Tn - 1
        need = lib.u2tok_decoder_decode_stack_kv8_workspace_bytes(arr8, n)
        assert need > 0 and need == lib.u2tok_decoder_decode_stack_workspace_bytes(arr16, n)
        hneed = lib.u2tok_decoder_decode_stack_head_kv8_workspace_bytes(arr8, n, C.byref(head))
        assert hneed == lib.u2tok_decoder_decode_stack_head_workspace_bytes(arr16, n, C.byref(head))
        assert hneed == need + lib.u2tok_decode_head_workspace_bytes(2, 256)
    ws, hws = lib.u2tok_decoder_decode_stack_kv8_workspace_bytes, lib.u2tok_decoder_decode_stack_head_kv8_workspace_bytes
    assert ws(arr8, 0) == 0 and ws(None, n) == 0 and hws(arr8, 0, C.byref(head)) == 0 and hws(None, n, C.byref(head)) == 0
    assert hws(arr8, n, None) == 0 and hws(arr8, n, C.byref(_head(E=512))) == 0
    arr8[1].T = 0
    assert ws(arr8, n) == 0 and hws(arr8, n, C.byref(head)) == 0
    arr8[1].T = 8192
    cfgs[2].E = 512                                                        # one hidden size for the whole stack
    assert ws(arr8, n) == 0
    cfgs[2].E = 256
    arr8[2].cfg = None
    assert ws(arr8, n) == 0
    arr8[2].cfg = C.addressof(cfgs[2])
    arr8[0].layer = None
    assert ws(arr8, n) == 0


def test_the_entries_refuse_before_anything_is_read(lib):
    n = 3
    arr8, _, cfgs, lays = _descriptors(n)
    head = _head()
    need = lib.u2tok_decoder_decode_stack_kv8_workspace_bytes(arr8, n)
    hneed = lib.u2tok_decoder_decode_stack_head_kv8_workspace_bytes(arr8, n, C.byref(head))
    LG = P

    def stack(nbytes=need, layers=arr8, count=n, x=P, cos=P, out=P, ws=P, kv_start=None, tail=0):
        # layers, n, x, cos, sin, cos_sin_f32, cs_ld, kv_start, w_final_norm, final_eps, tail_norm, out, workspace, bytes, stream
        return lib.u2tok_decoder_decode_stack_kv8(layers, count, x, cos, P, 1, 64, kv_start, P, 1e-6, tail, out, ws, nbytes, None)

    def joint(nbytes=None, layers=arr8, count=n, x=P, cos=P, out=P, ws=P, kv_start=None, tail=0, h=head, logits=LG):
        # layers, n, x, cos, sin, cos_sin_f32, cs_ld, kv_start, tail_norm, out, head, logits, ld_logits, workspace, bytes, stream
        nbytes = hneed if nbytes is None else nbytes + (hneed - need)
        return lib.u2tok_decoder_decode_stack_head_kv8(layers, count, x, cos, P, 1, 64, kv_start, tail, out,
                                                       None if h is None else C.byref(h), logits, 1000, ws, nbytes, None)

    for call in (stack, joint):
        assert call(layers=None) == ERR_ARG and call(count=0) == ERR_ARG and call(count=-1) == ERR_ARG
        assert call(x=None) == ERR_ARG and call(cos=None) == ERR_ARG and call(out=None) == ERR_ARG and call(ws=None) == ERR_ARG
        assert call(ws=P + 16) == ERR_ARG                                   # workspace not 256-byte aligned
        assert call(nbytes=need - 1) == ERR_WS and call(nbytes=0) == ERR_WS
        assert call(kv_start=P + 2) == ERR_ARG                              # kv_start misaligned
        for tail in (0, 1):
            for f in ("k_codes", "v_codes", "k_scales", "v_scales"):        # a null buffer in the LAST layer
                setattr(arr8[2], f, None)
                assert call(tail=tail) == ERR_ARG, f
                setattr(arr8[2], f, P)
            for f in ("Wqkv", "Wdown", "w_post_norm", "w_in_norm"):         # a null weight in the last layer
                setattr(lays[2], f, None)
                assert call(tail=tail) == ERR_ARG, f
                setattr(lays[2], f, P)
        arr8[1].k_codes = P + 8                                             # codes not 16-byte aligned
        assert call() == ERR_ARG
        arr8[1].k_codes = P
        arr8[1].v_scales = P + 2                                            # scales not 4-byte aligned
        assert call() == ERR_ARG
        arr8[1].v_scales = P
        for cap in (39, 0, -1):                                             # s_off >= capacity
            arr8[1].capacity = cap
            assert call() == ERR_ARG, cap
        arr8[1].capacity = 1 << 25                                          # capacity * D >= 2^31
        assert call() == ERR_ARG
        arr8[1].capacity = 256
        arr8[1].s_off = 256                                                 # the buffer is full
        arr8[1].T = 257
        assert call(nbytes=1 << 30) == ERR_ARG                              # (room for the longer attention: the refusal is the row's)
        arr8[1].s_off, arr8[1].T = 39, 40
        arr8[1].k_first = 1                                                 # T != s_off - k_first + 1: reads past the step's row
        assert call() == ERR_ARG
        arr8[1].T = 38                                                      # ... or stops short of it
        assert call() == ERR_ARG
        arr8[1].T = 39                                                      # (k_first = 1, T = 39: a window -- passes the walk's checks)
        arr8[1].k_first = -1
        arr8[1].T = 41
        assert call() == ERR_ARG
        arr8[1].k_first, arr8[1].T = 0, 40
        lays[0].scale_o = P                                                 # some, not all, of the four scales
        assert call() == ERR_ARG
        lays[0].scale_o = None
        cfgs[1].wform = 2                                                   # e2m1 without block scales
        assert call() == ERR_ARG
        cfgs[1].wform = 0
        lays[1].Wo = P + 8                                                  # a 16-bit Wo 8 bytes off alignment
        assert call() == ERR_ARG and call(tail=1) == ERR_ARG
        lays[1].Wo = P
        cfgs[1].Hq = 34                                                     # 17 query heads per kv head: no batched attention
        assert call(nbytes=1 << 30) == ERR_ARG                              # (room for the wider rows: the refusal is the heads')
        cfgs[1].Hq = 4
    assert joint(h=None) == ERR_ARG and joint(logits=None) == ERR_ARG and joint(h=_head(E=512)) == ERR_ARG
    assert joint(h=_head(V=1)) == ERR_ARG and joint(h=_head(W=P + 8)) == ERR_ARG and joint(h=_head(wform=1)) == ERR_ARG
    assert lib.u2tok_decoder_decode_stack_head_kv8(arr8, n, P, P, P, 1, 64, None, 0, P, C.byref(head), LG, 1000, P, need, None) == ERR_WS


def test_the_per_layer_entry_still_asks_for_the_new_rows(lib):
    """u2tok_decoder_decode_post_kv8 keeps its two launches: null k_new / v_new -- what the whole-stack walk hands its second half --
    stay U2TOK_ERR_ARG there."""
    _, _, cfgs, lays = _descriptors(1)
    need = lib.u2tok_decoder_decode_workspace_bytes(C.byref(cfgs[0]), 40)
    for k_new, v_new in ((None, None), (None, P), (P, None)):
        assert lib.u2tok_decoder_decode_post_kv8(C.byref(cfgs[0]), C.byref(lays[0]), P, P, k_new, v_new, P, P, P, P, 256, 0, 39, None, P, P,
                                                 need, None) == ERR_ARG


def test_the_rotary_entry_refuses_before_anything_is_read(lib):
    # qkv, wq, wk, cos, sin, cos_sin_f32, rows, Hq, Hkv, D, ld, cs_ld, eps, k_codes, v_codes, k_scales, v_scales, S, capacity, s_off, stream
    args = [P, P, P, P, P, 1, 6, 4, 2, 64, 512, 64, 1e-6, P, P, P, P, 3, 16, 13, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.u2tok_qk_norm_rope_kv8(*a)

    for i in (0, 3, 4, 13, 14, 15, 16):                                     # qkv, cos, sin, the four buffers
        assert call(**{f"a{i}": None}) == ERR_ARG, i
    assert call(a1=None) == ERR_ARG and call(a2=None) == ERR_ARG            # one head-norm weight without the other
    assert call(a13=P + 8) == ERR_ARG and call(a14=P + 8) == ERR_ARG        # codes not 16-byte aligned
    assert call(a15=P + 2) == ERR_ARG and call(a16=P + 2) == ERR_ARG        # scales not 4-byte aligned
    assert call(a19=14) == ERR_ARG and call(a19=-1) == ERR_ARG              # s_off + S > capacity; a negative position
    assert call(a19=0x7fffffff) == ERR_ARG
    assert call(a18=0) == ERR_ARG and call(a18=1 << 25) == ERR_ARG          # no capacity; capacity * D >= 2^31
    assert call(a17=0) == ERR_ARG and call(a17=4) == ERR_ARG                # S < 1; rows not a multiple of S
    assert call(a9=80) == ERR_ARG and call(a6=0) == ERR_ARG and call(a7=0) == ERR_ARG and call(a8=0) == ERR_ARG
