"""Host: the FP8 (e4m3) weight-only decode step without a GPU -- the row quantiser's properties (ops.quantize_rows_fp8), the
lossless fixture the GPU model tests rest on (ops.snap_fp8_: weights the quantiser keeps exactly), the float64 model and
per-element error bound tests/test_gpu_w8.py holds u2tok_gemm_rows_w8 to, the route's switch on a CPU model, and the argument
errors of the new entry points (nothing is launched: they return before any HIP call).

Conventions (tests/test_decoder_train_bounds_host.py): U = the unit roundoff of the element type (2^-8 bf16, 2^-11 fp16: what
round-to-nearest errs by, relatively, at the bottom of a binade and never exceeds), u = 2^-24 that of fp32."""
import ctypes as C

import pytest
import torch

from u2tokenizer_amd import _lib, ops

u = 2.0 ** -24
U_OF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
f64 = torch.float64


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def w8_rows_model(x, w8, scale, bias=None, R=None, U=2.0 ** -8, out_f32=False, waves=16):
    """float64 out = x . (scale[n] e4m3(W8[n][:]))^T (+ bias[n]) (+ R) and the per-element bound of the kernel's result:
      * the output rounding: U |out| (u for an fp32 output);
      * the fp32 accumulation: K u scale_n sum_k |x_k| |w_nk| -- K products, exact in fp32 (8 + 4 significant bits), each added
        with at most one fp32 rounding, in any order;
      * the epilogue's fp32 terms: `waves` u of that same magnitude (the cross-wave sum), u |acc| (the scale), u |acc + bias|,
        u |out| (bias and residual additions);
      * the last two groups times (1 + U): the value that is rounded to the element type is the kernel's, off by them from `out`."""
    xd, wq = x.double(), w8.float().double()
    sd = scale.double()
    K = xd.shape[1]
    acc = (xd @ wq.T) * sd[None]
    mag = (xd.abs() @ wq.abs().T) * sd[None]
    out = acc.clone()
    epi = u * acc.abs()
    if bias is not None:
        out = out + bias.double()[None]
        epi = epi + u * out.abs()
    if R is not None:
        out = out + R.double()
        epi = epi + u * out.abs()
    Uo = u if out_f32 else U
    bound = Uo * out.abs() + (1 + Uo) * ((K + waves) * u * mag + epi)
    return out, bound


def worst(err, bound):
    r = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return r.max().item() if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------ the quantiser
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_quantiser_properties(dt):
    g = _gen(1, 70, 192)
    w = (0.02 * torch.randn(70, 192, generator=g)).to(dt)
    w[3] = 0                                   # an all-zero row
    w[5, 7], w[5, 9] = 1.5, -1.5               # a row holding +-amax
    w[11] *= 1e-4                              # small rows scale like any other
    w8, sc = ops.quantize_rows_fp8(w)
    assert w8.shape == w.shape and w8.dtype == torch.float8_e4m3fn and w8.is_contiguous() and w8.element_size() == 1
    assert sc.shape == (70,) and sc.dtype == torch.float32 and (sc > 0).all()
    codes = w8.view(torch.uint8)
    assert not ((codes & 0x7F) == 0x7F).any()                 # 0x7F / 0xFF: NaN
    assert sc[3] == 1.0 and (codes[3] == 0).all()
    q = w8.float()
    assert q[5, 7] == 448 and q[5, 9] == -448 and (q.abs().amax(1)[sc != 1.0] == 448).all()
    dq = ops.dequantize_rows_fp8(w8, sc)
    assert dq.dtype == torch.float32 and dq.shape == w.shape
    wd, sd = w.double(), sc.double()[:, None]
    bound = sd * torch.maximum(2.0 ** -4 * (wd / sd).abs(), torch.tensor(2.0 ** -10, dtype=f64))   # half an e4m3 step
    err = (dq.double() - wd).abs()
    assert (err <= bound).all(), worst(err, bound)
    assert worst(err, bound) > 0.5                            # (the bound is what the format does, not a loose one)
    with pytest.raises(RuntimeError):
        ops.quantize_rows_fp8(w[0])
    with pytest.raises(RuntimeError):
        ops.quantize_rows_fp8(torch.full((2, 64), float("inf")))


def test_quantiser_clamps_instead_of_emitting_nan():
    """amax / 448 rounds, so W / scale can land a hair above 448, which torch's conversion turns into NaN: rows built so that it does"""
    amax = torch.tensor([448.0 * (1 + k * 2.0 ** -23) * 3.0 ** (k % 5) for k in range(1, 400)])
    w = torch.zeros(len(amax), 64)
    w[:, 0], w[:, 1] = amax, -amax
    w8, sc = ops.quantize_rows_fp8(w)
    assert ((w / sc[:, None]).abs() > 448).any()              # (the case exists among these rows)
    assert not ((w8.view(torch.uint8) & 0x7F) == 0x7F).any()
    assert (w8.float()[:, 0] == 448).all() and (w8.float()[:, 1] == -448).all()


# ------------------------------------------------------------------------------------------------------ the lossless fixture
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_snapped_weights_survive_the_quantiser_bit_for_bit(dt):
    lin = torch.nn.Linear(192, 70, bias=False)
    with torch.no_grad():
        lin.weight.copy_(0.02 * torch.randn(70, 192, generator=_gen(2)))
        lin.weight[4] = 0
    before = lin.weight.detach().clone()
    ops.snap_fp8_(lin)
    w = lin.weight.detach()
    assert (w - before).abs().max() <= before.abs().max()     # (snapped, not replaced: within the largest element's doubling)
    assert torch.equal(w.to(dt).float(), w)                   # exact in the element type
    w8, sc = ops.quantize_rows_fp8(w.to(dt))
    assert torch.equal(ops.dequantize_rows_fp8(w8, sc).to(dt), w.to(dt))
    assert torch.equal(ops.dequantize_rows_fp8(w8, sc), w)
    live = sc != 1.0
    assert (torch.log2(sc[live]) == torch.log2(sc[live]).round()).all() and (w8.float().abs().amax(1)[live] == 448).all()
    assert (2.0 ** -9 * sc[live] >= 2.0 ** -24).all()         # the fp16 condition at these magnitudes
    assert (w[4] == 0).all()


# ------------------------------------------------------------------------------------------------------ the error-bound model
def _case(M, N, K, dt, seed=3):
    g = _gen(seed, M, N, K)
    x = torch.randn(M, K, generator=g).to(dt)
    w8, sc = ops.quantize_rows_fp8(torch.randn(N, K, generator=g) / K ** 0.5)
    bias = (0.5 * torch.randn(N, generator=g)).to(dt)
    R = torch.randn(M, N, generator=g).to(dt)
    return x, w8, sc, bias, R


@pytest.mark.parametrize("M,N,K", [(5, 40, 192), (16, 16, 4096)])
def test_bound_holds_for_another_summation_order_and_is_not_vacuous(M, N, K):
    dt = torch.bfloat16
    x, w8, sc, bias, R = _case(M, N, K, dt)
    out, bound = w8_rows_model(x, w8, sc, bias, R)
    # the same sum in float64, K reversed and cut into 7 chunks added last-first
    xd, wd = x.double().flip(1), w8.float().double().flip(1)
    parts = [xd[:, c] @ wd[:, c].T for c in torch.arange(K).chunk(7)]
    other = sum(reversed(parts)) * sc.double()[None] + bias.double()[None] + R.double()
    assert worst((other - out).abs(), bound) < 1e-3
    # what the kernel may do at most: the element type's rounding of the float64 value
    assert 0.25 < worst((out.float().to(dt).double() - out).abs(), bound) <= 1.0
    # not vacuous: a far smaller bound than the result itself ...
    assert bound.max() < 2.0 ** -6 * out.abs().max() and (bound < 2.0 ** -7 * out.abs() + 2.0 ** -11 * x.abs().max() * K ** 0.5).all()
    # ... one weight's sign flipped (the row's largest product) falls outside it ...
    prod = (x.double()[0][None] * w8.float().double()).abs()
    n = 1
    k = int(prod[n].argmax())
    codes = w8.view(torch.uint8).clone()
    codes[n, k] ^= 0x80
    flipped, _ = w8_rows_model(x, codes.view(torch.float8_e4m3fn), sc, bias, R)
    assert (flipped - out).abs()[0, n] > bound[0, n]
    assert ((flipped - out).abs() > bound)[:, n].any() and not ((flipped - out).abs() > 0)[:, [c for c in range(N) if c != n]].any()
    # ... and so does a scale off by 2^-4, wherever the product is not cancelled by bias and residual or in itself
    off, _ = w8_rows_model(x, w8, sc * (1 + 2.0 ** -4), bias, R)
    acc = out - bias.double()[None] - R.double()
    mag = (x.double().abs() @ w8.float().double().abs().T) * sc.double()[None]
    big = (acc.abs() > 0.5 * out.abs()) & (acc.abs() > 2.0 ** -6 * mag)    # (nor by itself: K u mag < 2^-4 |acc| there)
    assert big.any() and ((off - out).abs() > bound)[big].all()


# ---------------------------------------------------------------------------------------------------------- the route on CPU
def _small(layers=2):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    from u2tokenizer_amd import synth
    m = Qwen3ForCausalLM(Qwen3Config(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=layers,
                                     num_attention_heads=4, num_key_value_heads=2, head_dim=32, max_position_embeddings=128,
                                     tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2))
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m.eval()


def test_cpu_model_with_the_switch_takes_the_stock_layers():
    from u2tokenizer_amd import prefill
    assert prefill.w8_stats.keys() == {"decode", "padded_decode"}
    assert prefill.stats.keys() == {"prefill", "decode", "padded_prefill", "padded_decode"}
    m = _small()
    x = 0.5 * torch.randn(1, 9, 128, generator=_gen(4))
    with torch.no_grad():
        want = m(inputs_embeds=x, use_cache=True)
        want1 = m(inputs_embeds=x[:, :1], past_key_values=want.past_key_values, use_cache=True).logits
        n0, s0 = dict(prefill.w8_stats), dict(prefill.stats)
        assert prefill.enable_fused_prefill(m, fp8_decode=True) == 2
        assert m.model._u2_stack.fp8 is True
        got = m(inputs_embeds=x, use_cache=True)
        got1 = m(inputs_embeds=x[:, :1], past_key_values=got.past_key_values, use_cache=True).logits
    assert torch.equal(got.logits, want.logits) and torch.equal(got1, want1)
    assert prefill.w8_stats == n0 and prefill.stats == s0
    assert all(prefill.w8_weights(lay) is None for lay in m.model.layers)
    prefill.enable_fused_prefill(m)                           # every call sets the switches anew
    assert m.model._u2_stack.fp8 is False
    prefill.disable_fused_prefill(m)
    assert prefill.w8_weights(m.model.layers[0]) is None


def test_u2_config_switch_defaults_off():
    from u2tokenizer_amd.language_model import u2Qwen3Config
    assert not getattr(u2Qwen3Config(), "u2_fused_decode_fp8", False)


# ------------------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


def test_gemm_rows_w8_rejects_bad_arguments(lib):
    """u2tok_gemm_rows_w8 returns U2TOK_ERR_ARG before any launch or memory access"""
    P = 1 << 20   # an aligned address that is never dereferenced
    # A, W8, scale, C, bias, R, M, N, K, lda, ldw, ldc, ldr, flags, stream
    args = [P, P + 4096, P + 8192, P + 12288, None, None, 4, 32, 64, 64, 64, 32, 0, 0, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.u2tok_gemm_rows_w8(*a)

    for i in (0, 1, 2, 3):
        assert call(**{f"a{i}": None}) == -1, i               # a2: the null scale
    assert call(a8=96, a9=96, a10=96) == -1                   # K = 96: not a multiple of 64
    assert call(a8=0) == -1 and call(a6=0) == -1 and call(a6=17) == -1 and call(a7=0) == -1
    assert call(a0=P + 8) == -1 and call(a1=P + 4096 + 8) == -1   # A / W8 not 16-byte aligned
    assert call(a2=P + 8192 + 2) == -1                        # scale not 4-byte aligned
    assert call(a9=56) == -1 and call(a9=68) == -1            # lda < K, lda not a multiple of 8
    assert call(a10=72) == -1 and call(a11=16) == -1          # ldw not a multiple of 16, ldc < N
    assert call(a13=1) == -1 and call(a13=8) == -1            # bias / residual flags without their pointers
    assert call(a13=8, a5=P, a12=16) == -1                    # ldr < N
    assert call(a13=4) == -1 and call(a13=512 | 16) == -1     # GELU is not an epilogue of this product; the pair form stands alone
    assert call(a13=512, a7=24, a11=12) == -1                 # pair: I % 8 != 0


def test_decode_w8_entry_points_reject_bad_arguments(lib):
    """u2tok_decoder_decode_pre / _post return U2TOK_ERR_ARG before any launch or memory access on a layer descriptor or a
    kv_start they do not take"""
    P = 1 << 20
    SCALES = ("scale_qkv", "scale_o", "scale_gu", "scale_down")

    def config(**kw):
        c = _lib.DecodeConfig(B=2, E=128, Hq=4, Hkv=2, D=64, I=256, eps=1e-6, qk_eps=1e-6, scale=0.125)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def layer(**kw):   # e4m3 codes with a scale behind each, no biases, no q / k norms
        fields = dict(w_in_norm=P, Wqkv=P, Wo=P, w_post_norm=P, Wgu=P, Wdown=P, **{n: P for n in SCALES})
        fields.update(kw)
        return _lib.DecodeLayer(**fields)

    def pre(lay, cfg=None):
        # cfg, layer, x, cos, sin, f32, cs_ld, qkv, kc, vc, kv_stride, s_off, ws, bytes, stream
        return lib.u2tok_decoder_decode_pre(C.byref(cfg or config()), C.byref(lay), P, P, P, 1, 64, P, P, P, 0, 0, P, 1 << 20, None)

    def post(lay, batched, cfg=None, kv_start=None):
        # cfg, layer, x, qkv, K, V, T, kv_stride, batched, kv_start, out, ws, bytes, stream
        return lib.u2tok_decoder_decode_post(C.byref(cfg or config()), C.byref(lay), P, P, P, P, 8, 0, batched, kv_start, P, P, 1 << 24,
                                             None)

    assert pre(layer(scale_qkv=None)) == -1                                  # null scale
    assert pre(layer(Wqkv=P + 8)) == -1                                      # misaligned weights
    for batched in (0, 1):
        for name in ("scale_o", "scale_gu", "scale_down"):
            assert post(layer(**{name: None}), batched) == -1, name          # null scales
        assert post(layer(Wgu=P + 4), batched) == -1
    for name, v in (("E", 96), ("I", 96), ("D", 96), ("Hq", 3)):             # E / I / Hq D not multiples of 64 (K = 96), or no config
        c2 = config(**{name: v}, **(dict(Hq=1, Hkv=1) if name == "D" else {}))
        assert pre(layer(), c2) == -1, name
        for batched in (0, 1):
            assert post(layer(), batched, c2) == -1, name
    # what only the descriptor can say: some of the four scales (a set one on a 16-bit layer, a missing one on an e4m3 layer:
    # each half refuses whichever scale it is, its own or the other half's), kv_start without the batched attention
    for name in SCALES:
        for lay in (layer(**{n: None for n in SCALES if n != name}), layer(**{name: None})):
            assert pre(lay) == -1, name
            assert post(lay, 0) == -1 and post(lay, 1) == -1, name
    for lay in (layer(), layer(**{n: None for n in SCALES})):
        assert post(lay, 0, kv_start=P) == -1
        # the batched attention's own limits: 16 query heads per kv head at the most, kv_start an int32 array
        assert post(lay, 1, config(Hq=64, Hkv=2)) == -1
        assert post(lay, 1, kv_start=P + 2) == -1
