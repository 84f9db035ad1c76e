"""Host: what tests/test_gpu_lora_rows.py and tests/test_gpu_lora_infer.py rest on, without a GPU.

* The per-element bounds of the few-rows adapter group product (u2tok_lora_rows; csrc/lora_rows.hip) as pure functions, reusing
  `down_model` / `up_model` of tests/test_lora_bounds_host.py: u under U |ref| + K u sum |x a|, then y under the up bound evaluated on
  the u it was computed from (the GPU's own u in the GPU test, the emulation's here) -- and a torch emulation of the kernels' sums
  (32-wide steps inside a K slice of max(8, ceil(K / 32 / 64)) steps, the slices' tiles added in slice order, u rounded to the
  element type, one rounding of y), shown inside the bounds on every case of the GPU module's table (imported, not copied).
* Every refusal of u2tok_lora_rows, and of u2tok_decoder_decode_pre / _post on a bad `lora` descriptor, returns its error code
  before any HIP call, on both builds; the workspace function.
* The route table (prefill.route needs no tensor): which forward a LoRA-wrapped layer takes without grad, per switch.
* prefill._lora_state rebuilds on each change it lists and on nothing else."""
import ctypes as C
import types

import pytest
import torch
from torch import nn

from test_decoder_route_host import _FakeCuda, _model, _route, _stock, recorder  # noqa: F401
from test_decoder_train_bounds_host import U, _gen, worst
from test_lora_bounds_host import U16, _chunked_f32, _rn, alpha_of, down_model, rnd16, up_model  # noqa: F401
from u2tokenizer_amd import _lib, lora, prefill
from u2tokenizer_amd.lora import LoRALinear, add_lora

bf, f32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------------ model and emulation
def rows_inputs(M, K, group, dtype=bf):
    """x (M, K), y (M, width) and per segment (A (r, K), B (N, r), col0, N, scale) for a group of (r, col0, N) triples"""
    g = _gen(15, M, K, *(v for seg in group for v in seg))
    width = max(c + n for _, c, n in group)
    segs = [(_rn(g, r, K, scale=K ** -0.5, dtype=dtype), _rn(g, n, r, scale=0.5, dtype=dtype), c, n, alpha_of(M, K, r, c)) for r, c, n in group]
    return dict(x=_rn(g, M, K, dtype=dtype), y=_rn(g, M, width, scale=1.5, dtype=dtype), segs=segs)


def slices_of(K):
    """the K slices of launch 1 as (first, last + 1) element ranges: max(8, ceil(steps / 64)) 32-wide steps each"""
    steps = K // 32
    per = max(8, -(-steps // 64))
    return [(32 * s, 32 * min(s + per, steps)) for s in range(0, steps, per)]


def rows_emulate(x, segs, y, drop_slice=None, drop_seg=None):
    """-> (u (M, sum r), y (M, width)) in float64 with the kernels' rounding points; drop_slice / drop_seg: a kernel that forgot one"""
    us, out = [], y.double().clone()
    for i, (a, b, c, n, s) in enumerate(segs):
        acc = torch.zeros(x.shape[0], a.shape[0], dtype=torch.float32)
        for j, (k0, k1) in enumerate(slices_of(x.shape[1])):
            if j != drop_slice:
                acc = acc + _chunked_f32(x[:, k0:k1], a[:, k0:k1].T, 32)
        uu = acc.to(x.dtype)
        us.append(uu.double())
        if i != drop_seg:
            out[:, c:c + n] = rnd16(y[:, c:c + n].float() + torch.tensor(s, dtype=torch.float32) * _chunked_f32(uu, b.T, 32), x.dtype)
    return torch.cat(us, 1), out


def rows_ratios(inp, u, y, U=U):
    """worst error / bound of u and of y (y's bound on the u handed in)"""
    o, ru, ry = 0, 0.0, 0.0
    for a, b, c, n, s in inp["segs"]:
        r = a.shape[0]
        md = down_model(inp["x"], a, 1.0, U=U)
        ru = max(ru, worst((u[:, o:o + r] - md["out"]).abs(), md["bound"]))
        mu = up_model(u[:, o:o + r].to(inp["x"].dtype), b, inp["y"][:, c:c + n], s, True, U=U)
        ry = max(ry, worst((y[:, c:c + n] - mu["out"]).abs(), mu["bound"]))
        o += r
    return ru, ry


def pytest_generate_tests(metafunc):
    """the cases are the GPU module's table (imported here, at collection: that module imports this one at its top)"""
    if "rows_case" in metafunc.fixturenames:
        import test_gpu_lora_rows as gpu
        metafunc.parametrize("rows_case", gpu.CASES, ids=lambda c: "-".join(str(x) for x in c).replace(" ", "_"))


def test_emulation_inside_bounds(rows_case):
    import test_gpu_lora_rows as gpu
    M, K, group = rows_case
    inp = rows_inputs(M, K, gpu.GROUPS[group])
    ru, ry = rows_ratios(inp, *rows_emulate(**inp))
    print(f"emulated error / bound, lora_rows {rows_case}: u {ru:.3f}, y {ry:.3f}")
    assert ru <= 1.0 and ry <= 1.0, (ru, ry)


def test_emulation_inside_bounds_on_half_elements():
    import test_gpu_lora_rows as gpu
    M, K, group = gpu.F16_CASE
    inp = rows_inputs(M, K, gpu.GROUPS[group], dtype=torch.float16)
    ru, ry = rows_ratios(inp, *rows_emulate(**inp), U=U16)
    assert ru <= 1.0 and ry <= 1.0, (ru, ry)


def test_slice_rule():
    assert slices_of(32) == [(0, 32)] and slices_of(96) == [(0, 96)]
    assert len(slices_of(1056)) == 5 and slices_of(1056)[-1] == (1024, 1056)           # 33 steps: 8, 8, 8, 8, 1
    assert len(slices_of(4096)) == 16 and len(slices_of(12288)) == 48
    assert len(slices_of(32 * 64 * 8)) == 64 and len(slices_of(32 * 64 * 8 + 32)) == 57  # never more than 64 slices


def test_bounds_see_a_dropped_slice_and_a_dropped_segment():
    """an emulation that forgets one K slice (the last: a single 32-wide step of 33) breaks the u bound by far; one that forgets a
    segment's product breaks the y bound by far"""
    import test_gpu_lora_rows as gpu
    inp = rows_inputs(17, 1056, gpu.GROUPS["mixed ranks"])
    for j in (0, 4):
        ru, _ = rows_ratios(inp, *rows_emulate(drop_slice=j, **inp))
        assert ru > 10, (j, ru)
    for i in range(3):
        u, y = rows_emulate(drop_seg=i, **inp)
        ru, ry = rows_ratios(inp, u, y)
        assert ru <= 1.0 and ry > 10, (i, ru, ry)


# ------------------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


P = 1 << 20   # an aligned address that is never dereferenced


def _segs(*triples, **kw):
    arr = (_lib.LoraSeg * max(len(triples), 1))()
    for e, (r, c, n) in zip(arr, triples):
        e.A, e.B, e.r, e.col0, e.N, e.scale = P, P + 4096, r, c, n, 2.0
    for k, v in kw.items():
        setattr(arr[int(k[1])], k[3:], v)
    return arr


def test_workspace_function(lib):
    ws = lib.u2tok_lora_rows_workspace_bytes
    one = _segs((16, 0, 32))
    assert ws(1, 32, C.addressof(one), 1) == 1 * 1 * 16 * 64
    assert ws(16, 32, C.addressof(one), 1) == 16 * 64 and ws(17, 32, C.addressof(one), 1) == 2 * 16 * 64   # blocks of 16 rows
    three = _segs((16, 0, 96), (64, 96, 32), (32, 128, 544))
    assert ws(64, 1056, C.addressof(three), 3) == 4 * 5 * 112 * 64                                         # 5 slices of 33 steps
    assert ws(1, 12288, C.addressof(three), 3) == 48 * 112 * 64                                            # a function of K alone
    assert ws(1, 12288, C.addressof(three), 2) == 48 * 80 * 64
    for bad in ((0, 32), (65, 32), (1, 0), (1, 40)):
        assert ws(*bad, C.addressof(one), 1) == 0
    assert ws(1, 32, None, 1) == 0 and ws(1, 32, C.addressof(one), 0) == 0 and ws(1, 32, C.addressof(three), 4) == 0
    assert ws(1, 32, C.addressof(_segs((8, 0, 32))), 1) == 0


def test_lora_rows_rejects_bad_arguments(lib):
    """u2tok_lora_rows returns U2TOK_ERR_ARG / U2TOK_ERR_WORKSPACE before any launch or memory access"""
    ERR_ARG, ERR_WS = -1, -3
    good = _segs((16, 0, 96), (64, 96, 32), (32, 160, 544))
    # X, ldx, segs, n, U, ldu, Y, ldy, M, K, ws, ws_bytes, stream
    args = [P, 1056, C.addressof(good), 3, P + (1 << 16), 112, P + (2 << 16), 704, 17, 1056, P + (4 << 16), 1 << 20, None]

    def call(segs=None, **kw):
        a = list(args)
        if segs is not None:
            a[2], a[3] = C.addressof(segs), len(segs)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.u2tok_lora_rows(*a)

    for i in (0, 2, 4, 6, 10):                                          # null X, segs, U, Y, workspace
        assert call(**{f"a{i}": None}) == ERR_ARG, i
    for i in (0, 4, 6, 10):                                             # ... and misaligned
        assert call(**{f"a{i}": args[i] + 8}) == ERR_ARG, i
    assert call(a8=0) == ERR_ARG and call(a8=65) == ERR_ARG             # M
    assert call(a9=0) == ERR_ARG and call(a9=1040, a1=1040) == ERR_ARG  # K = 0, K % 32 != 0
    assert call(a3=0) == ERR_ARG and call(a3=4) == ERR_ARG              # n
    assert call(a1=1024) == ERR_ARG and call(a1=1060) == ERR_ARG        # ldx < K, ldx % 8 != 0
    assert call(a5=104) == ERR_ARG and call(a5=116) == ERR_ARG          # ldu < sum r, ldu % 8 != 0
    assert call(a7=696) == ERR_ARG and call(a7=708) == ERR_ARG          # ldy < a segment's end, ldy % 8 != 0
    for r in (8, 48, 128, 0):
        assert call(_segs((r, 0, 96))) == ERR_ARG, r
    assert call(_segs((16, 0, 24))) == ERR_ARG and call(_segs((16, 0, 0))) == ERR_ARG       # N % 16 != 0, N = 0
    assert call(_segs((16, 8, 32))) == ERR_ARG and call(_segs((16, -16, 32))) == ERR_ARG    # col0 % 16 != 0, col0 < 0
    assert call(_segs((16, 0, 96), (16, 80, 32))) == ERR_ARG                                # overlapping segments
    assert call(_segs((16, 0, 96), (16, 96, 32), (32, 0, 16))) == ERR_ARG
    assert call(_segs((16, 0, 96), s0_A=None)) == ERR_ARG and call(_segs((16, 0, 96), s0_B=None)) == ERR_ARG
    assert call(_segs((16, 0, 96), s0_A=P + 2)) == ERR_ARG and call(_segs((16, 0, 96), s0_B=P + 8)) == ERR_ARG
    need = lib.u2tok_lora_rows_workspace_bytes(17, 1056, C.addressof(good), 3)
    assert need == 2 * 5 * 112 * 64
    assert call(a11=need - 1) == ERR_WS and call(a11=0) == ERR_WS
    assert call(_segs((16, 64, 32), (32, 0, 48)), a11=0) == ERR_WS      # (segments in any order, gaps: taken as far as the workspace)


def test_decode_entry_points_reject_a_bad_lora_descriptor(lib):
    """u2tok_decoder_decode_pre / _post return the error code of a `lora` descriptor they do not take before anything is launched:
    pre for the q|k|v group, post for o, gate|up and down"""
    ERR_ARG, ERR_WS = -1, -3
    cfg = _lib.DecodeConfig(B=2, E=128, Hq=4, Hkv=2, D=64, I=256, eps=1e-6, qk_eps=1e-6, scale=0.125)
    nq = (4 + 2 * 2) * 64
    keep = []

    def desc(**kw):
        d = _lib.DecodeLora(scratch=P + (8 << 20), scratch_bytes=1 << 20)
        for name, v in kw.items():
            if name.startswith("n_") or name.startswith("scratch"):
                setattr(d, name, v)
            else:
                for e, (r, c, n) in zip(getattr(d, name), v):
                    e.A, e.B, e.r, e.col0, e.N, e.scale = P, P + 4096, r, c, n, 2.0
                if "n_" + name not in kw:
                    setattr(d, "n_" + name, len(v))
        keep.append(d)
        return d

    def layer(d):
        return _lib.DecodeLayer(w_in_norm=P, Wqkv=P, Wo=P, w_post_norm=P, Wgu=P, Wdown=P, lora=C.addressof(d))

    def pre(d):
        # cfg, layer, x, cos, sin, f32, cs_ld, qkv, kc, vc, kv_stride, s_off, ws, bytes, stream
        return lib.u2tok_decoder_decode_pre(C.byref(cfg), C.byref(layer(d)), P, P, P, 1, 64, P, P, P, 0, 0, P, 1 << 20, None)

    def post(d):
        # cfg, layer, x, qkv, K, V, T, kv_stride, batched, kv_start, out, ws, bytes, stream
        return lib.u2tok_decoder_decode_post(C.byref(cfg), C.byref(layer(d)), P, P, P, P, 8, 0, 1, None, P, P, 1 << 24, None)

    assert C.sizeof(_lib.LoraSeg) == 32 and C.sizeof(_lib.DecodeLora) == 7 * 32 + 16 + 16
    assert C.sizeof(_lib.DecodeLayer) == 17 * C.sizeof(C.c_void_p)
    # q|k|v: pre's
    assert pre(desc(qkv=[(8, 0, 256)])) == ERR_ARG                                   # rank
    assert pre(desc(qkv=[(16, 0, 256), (16, 192, 128)])) == ERR_ARG                  # overlap
    assert pre(desc(qkv=[(16, 0, 256), (16, 256, 128), (16, 384, 256)])) == ERR_ARG  # past the packed row (nq = 512)
    assert nq == 512
    assert pre(desc(qkv=[(16, 0, 256)], n_qkv=4)) == ERR_ARG and pre(desc(qkv=[(16, 0, 256)], n_qkv=-1)) == ERR_ARG
    assert pre(desc(qkv=[(16, 0, 256)], scratch=None)) == ERR_ARG and pre(desc(qkv=[(16, 0, 256)], scratch=P + 8)) == ERR_ARG
    assert pre(desc(qkv=[(16, 0, 256)], scratch_bytes=1000)) == ERR_WS
    assert pre(desc(qkv=[(16, 0, 256)], scratch_bytes=_lib.DECODE_LORA_U_BYTES + 16 * 64 - 1)) == ERR_WS   # E = 128: 1 slice
    # o, gate|up, down: post's, each before the attention is launched
    for name, bad in (("o", [(48, 0, 128)]), ("o", [(16, 0, 256)]), ("gu", [(16, 0, 256), (16, 240, 256)]), ("gu", [(16, 0, 520)]),
                      ("down", [(16, 16, 128)]), ("down", [(16, 0, 120)])):
        assert post(desc(**{name: bad})) == ERR_ARG, (name, bad)
    assert post(desc(o=[(16, 0, 128)], n_o=2)) == ERR_ARG and post(desc(gu=[(16, 0, 256)], n_gu=3)) == ERR_ARG
    assert post(desc(down=[(16, 0, 128)], n_down=2)) == ERR_ARG
    assert post(desc(down=[(64, 0, 128)], scratch_bytes=_lib.DECODE_LORA_U_BYTES + 64 * 64 - 1)) == ERR_WS   # I = 256: 1 slice, r = 64
    assert post(desc(o=[(16, 0, 128)], scratch=None)) == ERR_ARG
    # a bad q|k|v list is not post's business, nor a bad down list pre's: each half checks its own groups
    assert pre(desc(down=[(8, 0, 128)], qkv=[(16, 0, 256)], scratch_bytes=10)) == ERR_WS


# ------------------------------------------------------------------------------------------------------------------ the route
def _patched(calls, kind="qwen3", wrap=True, adapter_dtype=None, dropout=0.05, targets=None, **flags):
    mk = dict(kind="phi3", hidden=192, head_dim=96) if kind == "phi3" else dict(kind=kind)
    m = _model(**mk)
    for layer in m.model.layers:
        layer._calls = calls
        layer.forward = types.MethodType(_stock, layer)
    if wrap:
        add_lora(m, adapter_dtype=adapter_dtype, dropout=dropout, target_modules=targets)
        m.eval()
    prefill.enable_fused_prefill(m, **flags)
    return m


def _routes(m, calls, continued=False):
    """(prefill, decode[, continued prefill]) routes of layer 0 without grad; a continued prefill that reaches the fused step reads
    "prefill" as well (the recorder stops at the step's first kernel)"""
    r = [_route(m, calls), _route(m, calls, S=1, cache="plain full")]
    if continued:
        r.append(_route(m, calls, cache="plain full"))
    return tuple(x[0] if isinstance(x, tuple) else x for x in r)


@pytest.mark.parametrize("kind", ["qwen3", "llama", "phi3"])
def test_route_of_wrapped_layers_without_grad(recorder, kind):
    assert _routes(_patched(recorder, kind, lora=True), recorder) == ("prefill", "decode")
    assert _routes(_patched(recorder, kind, lora=True, continued=True), recorder, True) == ("prefill", "decode", "prefill")
    assert _routes(_patched(recorder, kind, lora=True, adapter_dtype=f32), recorder) == ("prefill", "decode")
    assert _routes(_patched(recorder, kind), recorder) == ("stock", "stock")                       # the switch is off
    assert _routes(_patched(recorder, kind, continued=True), recorder, True) == ("stock", "stock", "stock")
    assert _routes(_patched(recorder, kind, train_lora=True), recorder) == ("stock", "stock")      # train_lora alone does not turn it on
    assert _routes(_patched(recorder, kind, wrap=False, lora=True), recorder) == ("prefill", "decode")
    m = _patched(recorder, kind, lora=True, train_lora=True, train_phi3=True)
    assert _route(m, recorder, grad=True) == "train" and _routes(m, recorder) == ("prefill", "decode")
    assert _route(_patched(recorder, kind, lora=True), recorder, grad=True) == "stock"             # ... nor the other way round


def test_only_some_projections_wrapped(recorder):
    m = _patched(recorder, lora=True, targets=("q_proj", "v_proj"))
    assert _routes(m, recorder) == ("prefill", "decode")
    ads = m.model.layers[0]._u2_prefill.ads
    assert [a is not None for a in ads] == [True, False, True, False, False, False, False]


def test_dropout_decides_per_call(recorder):
    """peft applies dropout in train mode even under no_grad: such a call keeps the stock forward"""
    m = _patched(recorder, lora=True)
    m.train()
    assert _routes(m, recorder) == ("stock", "stock")
    m.eval()
    assert _routes(m, recorder) == ("prefill", "decode")
    m = _patched(recorder, lora=True, dropout=0.0)         # nn.Identity
    m.train()
    assert _routes(m, recorder) == ("prefill", "decode")
    for mod in m.modules():
        if isinstance(mod, LoRALinear):
            mod.lora_dropout["default"] = nn.Dropout(p=0.0)
    m.train()
    assert _routes(m, recorder) == ("prefill", "decode")
    m.model.layers[0].mlp.up_proj.lora_dropout["default"] = nn.Dropout(p=0.05)      # one active dropout is enough
    m.train()
    assert _routes(m, recorder) == ("stock", "stock")
    m.model.layers[0].mlp.up_proj.lora_dropout["default"] = nn.AlphaDropout(p=0.0)  # a module the rule does not know
    assert _routes(m, recorder) == ("stock", "stock")


def test_route_refuses_what_it_does_not_compute(recorder):
    from test_lora_host import REFUSALS
    for name, break_it in REFUSALS.items():
        if name in ("merged", "disabled"):
            continue
        m = _patched(recorder, lora=True)
        q = m.model.layers[0].self_attn.q_proj
        break_it(q)
        assert lora.adapter_of(q) is None and lora.base_only_of(q) is None, name
        assert _routes(m, recorder) == ("stock", "stock"), name
    # ... and the same defects on a wrapper that is switched off: still not a layout that is understood
    for name in ("r = 8", "use_dora", "hook on the wrapper", "hook on A", "two active adapters", "base layer a Linear subclass",
                 "unreadable attribute"):
        m = _patched(recorder, lora=True)
        q = m.model.layers[0].self_attn.q_proj
        q.disable_adapters = True
        assert lora.base_only_of(q) is q.base_layer
        REFUSALS[name](q)
        assert lora.base_only_of(q) is None, name
        assert _routes(m, recorder) == ("stock", "stock"), name


@pytest.mark.parametrize("flag", ["disable_adapters", "merged"])
def test_a_disabled_or_merged_wrapper_is_routed_as_its_base(recorder, flag):
    m = _patched(recorder, lora=True)
    for mod in m.modules():
        if isinstance(mod, LoRALinear):
            setattr(mod, flag, True)
    m.train()                                             # (dropout does not matter: the branch is not computed)
    assert _routes(m, recorder) == ("prefill", "decode")
    st = m.model.layers[0]._u2_prefill
    assert st.ads is None                                 # nothing to add: the base layers alone
    q = m.model.layers[0].self_attn.q_proj
    assert lora.base_only_of(q) is q.base_layer and lora.adapter_of(q) is None
    setattr(q, flag, False)                               # one live adapter among disabled ones, in train mode with p = 0.05
    assert _routes(m, recorder) == ("stock", "stock")
    m.eval()
    assert _routes(m, recorder) == ("prefill", "decode")
    assert [a is not None for a in st.ads] == [True] + [False] * 6
    prefill.enable_fused_prefill(m)                       # the switch off: a disabled wrapper is not exactly nn.Linear
    assert _routes(m, recorder) == ("stock", "stock")


def test_switch_defaults_off_and_config_switch():
    import inspect
    assert inspect.signature(prefill.enable_fused_prefill).parameters["lora"].default is False
    m = _model()
    prefill.enable_fused_prefill(m, lora=True)
    assert m.model._u2_stack.lora and not m.model._u2_stack.train_lora and not m.model._u2_stack.train
    prefill.enable_fused_prefill(m, train_lora=True)      # every call sets the switches anew
    assert not m.model._u2_stack.lora
    assert set(prefill.lora_stats) == {"prefill", "extend", "decode", "adapters"}
    from u2tokenizer_amd.language_model import u2Qwen3Config
    assert not getattr(u2Qwen3Config(), "u2_fused_lora_inference", False)
    # the config attribute alone reaches the stack as `lora`, and as nothing else
    from u2tokenizer_amd import language_model as LM
    for on in (False, True):
        cfg = LM.u2Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                               num_key_value_heads=2, head_dim=16)
        cfg.u2_fused_lora_inference = on
        lm = LM.u2Qwen3ForCausalLM(cfg).to(bf).eval()
        layer = lm.model.layers[0]
        p0 = next(layer.parameters())
        layer.parameters = lambda *a, p0=p0, **k: iter([p0.detach().as_subclass(_FakeCuda)])
        with torch.no_grad():
            lm(inputs_embeds=torch.zeros(1, 3, 64, dtype=bf))
        stack = lm.model._u2_stack
        assert stack.lora is on and stack.prefill and not (stack.train or stack.train_lora or stack.padded or stack.fp8)


# ------------------------------------------------------------------------------------------------------------- the cached state
def test_lora_state_rebuilds_on_each_listed_change_and_on_nothing_else(recorder):
    m = _patched(recorder, lora=True, adapter_dtype=f32)
    layer = m.model.layers[0]
    st, lo = layer._u2_prefill, layer._u2_prefill.layout
    pr = lo.projections(layer)
    dev = torch.device("cpu")

    def state():
        n = prefill.lora_state_builds[0]
        assert _routes(m, recorder) == ("prefill", "decode")          # (route() leaves the call's adapters in st.ads; the prefill
        #                                                                step reads the state on its way to its first kernel)
        ls = prefill._lora_state(st, lo, pr, bf, dev)
        return ls, prefill.lora_state_builds[0] - n

    ls0, built = state()
    assert built == 1 and ls0.n == 7 and [len(g) for g in ls0.groups] == [3, 1, 2, 1]
    (A16, B16, col0, s), k_seg, v_seg = ls0.groups[0]
    q = layer.self_attn.q_proj
    assert A16.dtype == bf and B16.dtype == bf and A16.shape == (16, 128) and B16.shape == (128, 16) and s == 2.0
    assert (col0, k_seg[2], v_seg[2]) == (0, 128, 192) and ls0.groups[2][1][2] == 256                      # gate | up: col0 = I
    assert torch.equal(A16, q.lora_A["default"].weight.detach().to(bf))                                   # the 16-bit compute copy
    for _ in range(3):                                                                                    # nothing changed: kept
        ls, built = state()
        assert ls is ls0 and built == 0
    with torch.no_grad():
        q.lora_B["default"].weight.mul_(2)                                                                # _version
    ls1, built = state()
    assert built == 1 and torch.equal(ls1.groups[0][0][1], q.lora_B["default"].weight.detach().to(bf))
    q.lora_A["default"].weight.data = q.lora_A["default"].weight.data.clone()                             # data_ptr()
    assert state()[1] == 1 and state()[1] == 0
    q.scaling["default"] = 0.5                                                                            # a scaling
    ls2, built = state()
    assert built == 1 and ls2.groups[0][0][3] == 0.5
    for name, table in (("lora_A", q.lora_A), ("lora_B", q.lora_B)):                                      # the active adapter
        table["other"] = nn.Linear(*((128, 16) if name == "lora_A" else (16, 128)), bias=False)
    q.lora_dropout["other"], q.r["other"], q.scaling["other"], q.lora_alpha["other"] = nn.Identity(), 16, 1.0, 16
    assert state()[1] == 0                                                                                # (an inactive one: nothing)
    q.active_adapters = ["other"]
    ls3, built = state()
    assert built == 1 and ls3.groups[0][0][3] == 1.0
    for flag in ("merged", "disable_adapters"):                                                           # the flags, on and off
        setattr(layer.mlp.down_proj, flag, True)
        ls4, built = state()
        assert built == 1 and ls4.n == 6 and ls4.groups[3] == ()
        setattr(layer.mlp.down_proj, flag, False)
        assert state()[1] == 1 and state()[1] == 0
    with torch.no_grad():
        layer.mlp.down_proj.base_layer.weight.mul_(2)                                                     # a base weight: not the adapters'
    assert state()[1] == 0
    # bf16 adapters on the device are read where they lie
    m2 = _patched(recorder, lora=True)
    l2 = m2.model.layers[0]
    assert _routes(m2, recorder) == ("prefill", "decode")
    ls = prefill._lora_state(l2._u2_prefill, l2._u2_prefill.layout, l2._u2_prefill.layout.projections(l2), bf, dev)
    assert ls.groups[1][0][0].data_ptr() == l2.self_attn.o_proj.lora_A["default"].weight.data_ptr()
    # freed with the switch and with the patch
    prefill.enable_fused_prefill(m2)
    assert l2._u2_prefill.lora is None and l2._u2_prefill.ads is None
    prefill.disable_fused_prefill(m)
    assert "_u2_prefill" not in layer.__dict__
