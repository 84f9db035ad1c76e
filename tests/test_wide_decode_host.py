"""CPU: decode steps of 17 .. 64 sequences on the fused step (opt-in, `enable_fused_prefill(model, wide_decode=True)`) -- the
route table of a patched layer with the switch on and off, on the small fixtures of tests/test_pad_rule_host.py and
tests/test_decoder_route_host.py (a CPU tensor that reports `is_cuda`, every route ends in a recorder before it would launch
anything), the config plumbing, a CPU model with the switch, and the argument errors of the entry points that changed (nothing is
launched: they return before any HIP call)."""
import ctypes as C

import pytest
import torch

import test_decoder_route_host as R
import test_pad_rule_host as P
from test_pad_rule_host import recorder  # noqa: F401  (the fixture)
from u2tokenizer_amd import _lib, prefill

bf = torch.bfloat16


def _ones(B, S):
    return torch.ones(B, S, dtype=torch.int64)


# (model kwargs, enable flags, stack mask, call kwargs, expected route)
WIDE = {
    "off, batch 17": ({}, {}, _ones(17, 6), dict(B=17, S=1, T=5), "stock"),
    "off, batch 64": ({}, {}, _ones(64, 6), dict(B=64, S=1, T=5), "stock"),
    "on, batch 16": ({}, dict(wide_decode=True), _ones(16, 6), dict(B=16, S=1, T=5), ("decode", None)),
    "on, batch 17": ({}, dict(wide_decode=True), _ones(17, 6), dict(B=17, S=1, T=5), ("decode", None)),
    "on, batch 64": ({}, dict(wide_decode=True), _ones(64, 6), dict(B=64, S=1, T=5), ("decode", None)),
    "on, batch 65": ({}, dict(wide_decode=True), _ones(65, 6), dict(B=65, S=1, T=5), "stock"),
    "on, batch 17, llama": (dict(kind="llama"), dict(wide_decode=True), _ones(17, 6), dict(B=17, S=1, T=5), ("decode", None)),
    "on, batch 17, fp16": (dict(dtype=torch.float16), dict(wide_decode=True), _ones(17, 6), dict(B=17, S=1, T=5), ("decode", None)),
    "on, batch 17, window W": (P.PHI3W, dict(wide_decode=True), _ones(17, 41), dict(B=17, S=1, T=40), ("decode", 32)),
    "on, batch 17, decode off": ({}, dict(wide_decode=True, decode=False), _ones(17, 6), dict(B=17, S=1, T=5), "stock"),
    "on, batch 17, empty cache": ({}, dict(wide_decode=True), _ones(17, 1), dict(B=17, S=1, T=None), "stock"),
    "on, 16 query heads per kv head": (dict(num_attention_heads=16), dict(wide_decode=True), _ones(17, 6), dict(B=17, S=1, T=5),
                                       ("decode", None)),
    "on, 17 query heads per kv head": (dict(num_attention_heads=17), dict(wide_decode=True), _ones(17, 6), dict(B=17, S=1, T=5),
                                       "stock"),
    "on, 17 query heads per kv head, batch 16": (dict(num_attention_heads=17), dict(wide_decode=True), _ones(16, 6),
                                                 dict(B=16, S=1, T=5), ("decode", None)),   # (the per-sequence attention, as before)
    "on, right-padded": ({}, dict(wide_decode=True, padded=True), P._mask("right", B=17, S=6), dict(B=17, S=1, T=5), "stock"),
    "on, left-padded, padded": ({}, dict(wide_decode=True, padded=True), P._mask("left", B=17, S=6), dict(B=17, S=1, T=5),
                                ("decode", None)),
    "on, left-padded, batch 64, padded": ({}, dict(wide_decode=True, padded=True), P._mask("left", B=64, S=6),
                                          dict(B=64, S=1, T=5), ("decode", None)),
    "on, left-padded, without padded": ({}, dict(wide_decode=True), P._mask("left", B=17, S=6), dict(B=17, S=1, T=5), "stock"),
    "off, left-padded, padded": ({}, dict(padded=True), P._mask("left", B=17, S=6), dict(B=17, S=1, T=5), "stock"),
    "on, left-padded, windowed layer": (P.PHI3W, dict(wide_decode=True, padded=True), P._mask("left", B=17, S=6),
                                        dict(B=17, S=1, T=5), "stock"),
    "on, prefill of batch 17": ({}, dict(wide_decode=True), _ones(17, 8), dict(B=17, S=8), "prefill"),
}


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_route(recorder, name):
    mk, flags, mask, call, want = WIDE[name]
    m = P._model(**mk)
    P._patch(m, recorder, **flags)
    assert m.model._u2_stack.wide is bool(flags.get("wide_decode", False))
    assert P._route(m, recorder, mask, **call) == want


def test_grad_enabled_is_unaffected(recorder):
    """With grad enabled the switch changes nothing: batch 17 trains with train=True and is stock without it."""
    for train, want in ((True, "train"), (False, "stock")):
        m = P._model()
        P._patch(m, recorder, train=train, wide_decode=True)
        assert R._route(m, recorder, grad=True, B=17) == want
        assert R._route(m, recorder, grad=True, B=17, S=1, cache="plain full") == "stock"   # (no training step onto a cache)


def test_the_switch_is_set_anew_by_every_enable_call(recorder):
    m = P._model()
    P._patch(m, recorder, wide_decode=True)
    assert m.model._u2_stack.wide is True
    assert P._route(m, recorder, _ones(17, 6), B=17, S=1, T=5) == ("decode", None)
    prefill.enable_fused_prefill(m)
    assert m.model._u2_stack.wide is False
    assert P._route(m, recorder, _ones(17, 6), B=17, S=1, T=5) == "stock"
    assert P._route(m, recorder, _ones(16, 6), B=16, S=1, T=5) == ("decode", None)


def test_lm_config_switch_is_passed_on(monkeypatch):
    """`config.u2_fused_wide_decode` reaches enable_fused_prefill as `wide_decode` (default: not passed, so False)."""
    from u2tokenizer_amd import language_model as LM
    assert not getattr(LM.u2Qwen3Config(), "u2_fused_wide_decode", False)
    seen = []
    monkeypatch.setattr(prefill, "enable_fused_prefill", lambda model, **kw: seen.append(kw) or 0)
    for on in (None, True):
        cfg = LM.u2Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                               num_key_value_heads=2, head_dim=16)
        if on is not None:
            cfg.u2_fused_wide_decode = on
        m = LM.u2Qwen3ForCausalLM(cfg).to(bf).eval()
        layer = m.model.layers[0]
        p0 = next(layer.parameters())
        layer.parameters = lambda *a, p0=p0, **k: iter([p0.detach().as_subclass(P._FakeCuda)])
        with torch.no_grad():
            m(inputs_embeds=torch.zeros(1, 3, 64, dtype=bf))
    assert [kw.get("wide_decode", False) for kw in seen] == [False, True]


def test_cpu_model_with_the_switch_takes_the_stock_layers():
    import test_w8_host as H
    assert prefill.wide_stats.keys() == {"decode", "padded_decode"}
    m = H._small()
    x = 0.5 * torch.randn(17, 9, 128, generator=H._gen(4))
    with torch.no_grad():
        want = m(inputs_embeds=x, use_cache=True)
        want1 = m(inputs_embeds=x[:, :1], past_key_values=want.past_key_values, use_cache=True).logits
        n0, s0 = dict(prefill.wide_stats), dict(prefill.stats)
        assert prefill.enable_fused_prefill(m, wide_decode=True) == 2
        got = m(inputs_embeds=x, use_cache=True)
        got1 = m(inputs_embeds=x[:, :1], past_key_values=got.past_key_values, use_cache=True).logits
    assert torch.equal(got.logits, want.logits) and torch.equal(got1, want1)
    assert prefill.wide_stats == n0 and prefill.stats == s0
    prefill.disable_fused_prefill(m)


# ------------------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


def test_gemm_rows_rejects_bad_arguments(lib):
    """u2tok_gemm_rows returns U2TOK_ERR_ARG before any launch or memory access"""
    Pn = 1 << 20   # an aligned address that is never dereferenced
    # A, W, C, bias, R, M, N, K, lda, ldw, ldc, ldr, flags, stream
    args = [Pn, Pn + 4096, Pn + 12288, None, None, 20, 32, 64, 64, 64, 32, 0, 0, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.u2tok_gemm_rows(*a)

    for i in (0, 1, 2):
        assert call(**{f"a{i}": None}) == -1, i
    assert call(a5=0) == -1 and call(a5=65) == -1 and call(a5=-3) == -1 and call(a6=0) == -1 and call(a7=0) == -1
    assert call(a7=48, a8=48, a9=48) == -1                    # K = 48: not a multiple of 32
    assert call(a0=Pn + 8) == -1 and call(a1=Pn + 4096 + 8) == -1   # A / W not 16-byte aligned
    assert call(a8=56) == -1 and call(a8=68) == -1            # lda < K, lda not a multiple of 8
    assert call(a9=56) == -1 and call(a9=68) == -1            # ldw likewise
    assert call(a10=16) == -1                                 # ldc < N
    assert call(a12=1) == -1 and call(a12=8) == -1            # bias / residual flags without their pointers
    assert call(a12=8, a4=Pn, a11=16) == -1                   # ldr < N
    for flags in (2, 4, 32, 64, 128, 256, 512 | 16, 512 | 1):  # bias_m, GELU, internal / layout flags; the pair form stands alone
        assert call(a12=flags, a3=Pn) == -1, flags
    assert call(a12=512, a6=24, a10=12) == -1                 # pair: I % 8 != 0


def test_wide_entry_points_reject_bad_arguments(lib):
    """M = 65 on both e4m3 entry points and M = 17 on the one that keeps its published range; B = 65 on the step's two halves
    and B = 17 without the batched attention -- in both weight forms, before anything is launched."""
    Pn = 1 << 20
    w8 = [Pn, Pn + 4096, Pn + 8192, Pn + 12288, None, None, 20, 32, 64, 64, 64, 32, 0, 0, None]
    for M, fn, want_err in ((65, lib.u2tok_gemm_rows_w8_wide, True), (0, lib.u2tok_gemm_rows_w8_wide, True),
                            (65, lib.u2tok_gemm_rows_w8, True), (17, lib.u2tok_gemm_rows_w8, True)):
        a = list(w8)
        a[6] = M
        assert (fn(*a) == -1) is want_err, (M, fn)
    for i in (0, 1, 2, 3):
        a = list(w8)
        a[i] = None
        assert lib.u2tok_gemm_rows_w8_wide(*a) == -1, i
    a = list(w8)
    a[8], a[9], a[10] = 96, 96, 96                            # K = 96: not a multiple of 64
    assert lib.u2tok_gemm_rows_w8_wide(*a) == -1
    SCALES = ("scale_qkv", "scale_o", "scale_gu", "scale_down")

    def config(B):
        return _lib.DecodeConfig(B=B, E=128, Hq=4, Hkv=2, D=64, I=256, eps=1e-6, qk_eps=1e-6, scale=0.125)

    def layer(w8):
        fields = dict(w_in_norm=Pn, Wqkv=Pn, Wo=Pn, w_post_norm=Pn, Wgu=Pn, Wdown=Pn, **({n: Pn for n in SCALES} if w8 else {}))
        return _lib.DecodeLayer(**fields)

    for form in (False, True):
        lay = layer(form)
        assert lib.u2tok_decoder_decode_pre(C.byref(config(65)), C.byref(lay), Pn, Pn, Pn, 1, 64, Pn, Pn, Pn, 0, 0, Pn, 1 << 24,
                                            None) == -1
        for B, batched in ((65, 0), (65, 1), (17, 0), (64, 0)):
            assert lib.u2tok_decoder_decode_post(C.byref(config(B)), C.byref(lay), Pn, Pn, Pn, Pn, 8, 0, batched, None, Pn, Pn,
                                                 1 << 26, None) == -1, (B, batched)
        assert lib.u2tok_decoder_decode_workspace_bytes(C.byref(config(65)), 64) == 0
        assert lib.u2tok_decoder_decode_workspace_bytes(C.byref(config(64)), 64) > \
            lib.u2tok_decoder_decode_workspace_bytes(C.byref(config(16)), 64) > 0
