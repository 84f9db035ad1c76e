"""Host: the MXFP4 (e2m1 codes, e8m0 block scales) weight-only decode step without a GPU -- the block quantiser's properties
(ops.quantize_blocks_fp4: the OCP MX rule), the lossless fixture the GPU model tests rest on (ops.snap_fp4_), the float64 model and
per-element error bound tests/test_gpu_w4.py holds u2tok_gemm_rows_w4 to, the argument errors of the new entry point and of the
layer descriptor's block scales (nothing is launched: they return before any HIP call), and the route's switch: precedence of
e2m1 over e4m3 over 16 bits per layer, the counters, the config default, a CPU model.

Conventions (tests/test_w8_host.py): U = the unit roundoff of the element type, u = 2^-24 that of fp32."""
import ctypes as C
import types

import pytest
import torch

from test_decoder_route_host import _model
from test_w8_host import U_OF, _gen, _small, u, worst
from u2tokenizer_amd import _lib, ops

f64 = torch.float64
GRID = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=f64)


def unpack(codes):
    """(N, K / 2) bytes -> (N, K) codes: even k from the low nibble"""
    return torch.stack((codes & 15, codes >> 4), 2).reshape(codes.shape[0], -1).long()


def w4_values(codes, scales):
    """float64 (N, K): e2m1(code) 2^(e - 127), from the format's definition alone"""
    return GRID[unpack(codes)] * torch.exp2(scales.double() - 127).repeat_interleave(32, 1)


def w4_rows_model(x, codes, scales, bias=None, R=None, U=2.0 ** -8, out_f32=False, waves=16):
    """float64 out = x . (e2m1(code[n][:]) 2^(e[n][: / 32] - 127))^T (+ bias[n]) (+ R) and the per-element bound of the kernel's
    result, built as test_w8_host.w8_rows_model is:
      * the output rounding: U |out| (u for an fp32 output);
      * the fp32 accumulation: K u sum_k |x_k| |w_nk| -- K products, exact in fp32 (8 or 11 significant bits times 2: the widened
        weight is exact in the element type), each added with at most one fp32 rounding, in any order;
      * the epilogue's fp32 terms: `waves` u of that same magnitude (the cross-wave sum), u |acc + bias|, u |out| (bias and
        residual additions) -- no scale multiply follows the sum in this form, so that term of the e4m3 model has no counterpart;
      * the last two groups times (1 + U): the value that is rounded to the element type is the kernel's, off by them from `out`."""
    xd, wd = x.double(), w4_values(codes, scales)
    K = xd.shape[1]
    acc = xd @ wd.T
    mag = xd.abs() @ wd.abs().T
    out = acc.clone()
    epi = torch.zeros_like(acc)
    if bias is not None:
        out = out + bias.double()[None]
        epi = epi + u * out.abs()
    if R is not None:
        out = out + R.double()
        epi = epi + u * out.abs()
    Uo = u if out_f32 else U
    bound = Uo * out.abs() + (1 + Uo) * ((K + waves) * u * mag + epi)
    return out, bound


# ------------------------------------------------------------------------------------------------------------ the quantiser
def _ocp_x(w):
    """the OCP rule in float64, independently: floor(log2(amax)) - 2 per block of 32, 0 for an all-zero block, clamped"""
    amax = w.double().reshape(w.shape[0], -1, 32).abs().amax(2)
    x = torch.where(amax > 0, torch.floor(torch.log2(torch.where(amax > 0, amax, torch.ones_like(amax)))) - 2, torch.zeros_like(amax))
    return x.clamp(-23, 13)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_quantiser_properties(dt):
    g = _gen(1, 70, 384)
    w = (0.02 * torch.randn(70, 384, generator=g)).to(dt)
    w[3, 64:96] = 0                            # an all-zero block
    w[5, 7], w[5, 9] = 1.5, -1.5               # a block holding +-amax
    w[11] *= 2.0 ** -10                        # small blocks scale like any other
    w[12, :32] = (2.0 ** -14 * torch.randn(32, generator=g)).to(dt)   # fp16 subnormals: x clamps at -23 for some of these ...
    w[13, :32] = 0
    w[13, 3] = 2.0 ** -24 if dt != torch.bfloat16 else 2.0 ** -30     # ... and certainly here
    w[14, :32] = (3e4 * torch.rand(32, generator=g)).to(dt)           # near the top: x = 12
    w[14, 0] = 40000.0                                                # 2^15 <= amax < 2^16: x = 13, the last one
    codes, sc = ops.quantize_blocks_fp4(w)
    assert codes.shape == (70, 192) and codes.dtype == torch.uint8 and codes.is_contiguous()
    assert sc.shape == (70, 12) and sc.dtype == torch.uint8 and sc.is_contiguous()
    x = sc.double() - 127
    assert torch.equal(x, _ocp_x(w))
    assert x.min() == -23 and x.max() == 13 and x[13, 0] == -23 and x[14, 0] == 13
    assert sc[3, 2] == 127 and (codes[3, 32:48] == 0).all()
    # every |w / 2^x| <= 6 after saturation, and what saturates lies in (6, 8)
    v = w.double() / torch.exp2(x).repeat_interleave(32, 1)
    q = GRID[unpack(codes)]
    assert q.abs().max() == 6 and (v.abs() < 8).all()
    assert ((q.abs() == 6) | (v.abs() <= 6)).all()
    # nearest on the grid (half a step: .25 below 2, .5 below 4, 1 above), ties to the even code, saturation apart
    step = torch.where(v.abs() < 2, 0.25, torch.where(v.abs() < 4, 0.5, 1.0)).double()
    err = (q - v).abs()
    inside = v.abs() <= 6
    assert (err[inside] <= step[inside]).all() and worst(err[inside], step[inside]) > 0.9
    assert q[5, 7] == 6 and q[5, 9] == -6 and x[5, 0] == -2
    dq = ops.dequantize_blocks_fp4(codes, sc)
    assert dq.dtype == torch.float32 and dq.shape == w.shape and torch.equal(dq.double(), w4_values(codes, sc))
    assert torch.equal(dq.to(torch.float16).float(), dq) and torch.equal(dq.to(torch.bfloat16).float(), dq)   # exact in both builds


def test_nibble_order_and_ties():
    """even k in the low nibble: a weight whose even columns hold 1 (code 2) and odd columns -3 (code 13) packs to 0xD2; the
    grid's ties go to the even code"""
    w = torch.zeros(2, 128)
    w[:, 0::2], w[:, 1::2] = 1.0, -3.0
    w[:, 0::32] = 4.0                                  # every block's amax = 4: x = 0
    codes, sc = ops.quantize_blocks_fp4(w)
    first = torch.arange(64) % 16 == 0
    assert (sc == 127).all() and (codes[:, first] == 0xD6).all() and (codes[:, ~first] == 0xD2).all()
    t = torch.zeros(1, 128)
    t[0, :9] = torch.tensor([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -5.0])
    c = unpack(ops.quantize_blocks_fp4(t)[0])[0, :9].tolist()
    assert c == [6, 0, 2, 2, 4, 4, 6, 6, 14], c        # 0, 1, 1, 2, 2, 4, 4, -4
    t[0, 0] = 7.9                                      # saturates, and x stays 0
    codes, sc = ops.quantize_blocks_fp4(t)
    assert unpack(codes)[0, 0] == 7 and sc[0, 0] == 127
    assert unpack(ops.quantize_blocks_fp4(-1e-30 * torch.ones(1, 128))[0]).sum() == 0   # (no negative zeros)


def test_quantiser_refusals():
    for bad in (torch.zeros(128), torch.zeros(2, 2, 128), torch.zeros(4, 192), torch.zeros(4, 128, dtype=torch.int32),
                torch.full((2, 128), float("inf")), torch.full((2, 128), float("nan")), torch.full((2, 128), 2.0 ** 16)):
        with pytest.raises(RuntimeError):
            ops.quantize_blocks_fp4(bad)
    ops.quantize_blocks_fp4(torch.full((2, 128), 2.0 ** 16 - 1))
    with pytest.raises(RuntimeError):
        ops.dequantize_blocks_fp4(torch.zeros(2, 64, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------ the lossless fixture
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_snapped_weights_survive_the_quantiser_bit_for_bit(dt):
    lin = torch.nn.Linear(384, 70, bias=False)
    odd = torch.nn.Linear(192, 8, bias=False)           # K % 128 != 0: not a weight of this format, left alone
    with torch.no_grad():
        lin.weight.copy_(0.02 * torch.randn(70, 384, generator=_gen(2)))
        lin.weight[4] = 0
        lin.weight[6] *= 2.0 ** -20
    before, odd_before = lin.weight.detach().clone(), odd.weight.detach().clone()
    ops.snap_fp4_(torch.nn.Sequential(lin, odd))
    w = lin.weight.detach()
    assert torch.equal(odd.weight.detach(), odd_before)
    assert (w - before).abs().max() <= before.abs().max() and not torch.equal(w, before)
    assert torch.equal(w.to(dt).float(), w)                   # exact in the element type
    codes, sc = ops.quantize_blocks_fp4(w.to(dt))
    assert torch.equal(ops.dequantize_blocks_fp4(codes, sc).to(dt), w.to(dt))
    assert torch.equal(ops.dequantize_blocks_fp4(codes, sc), w)
    c0, s0 = ops.quantize_blocks_fp4(before)
    assert torch.equal(s0, sc)                                # the same x is found ...
    free = (s0 > 127 - 23).repeat_interleave(16, 1)           # ... and, where it was not clamped from below, the same codes
    assert torch.equal(c0[free], codes[free]) and not free[6].any() and free[:4].all()
    top = GRID[unpack(codes)].reshape(70, 12, 32).abs().amax(2)
    live = w.reshape(70, 12, 32).abs().amax(2) > 0
    unclamped = live & (sc > 127 - 23)
    assert unclamped.any() and ((top[unclamped] == 6) | (top[unclamped] == 4)).all()
    assert (w[4] == 0).all()


# ------------------------------------------------------------------------------------------------------ the error-bound model
def _case(M, N, K, dt, seed=3):
    g = _gen(seed, M, N, K)
    x = torch.randn(M, K, generator=g).to(dt)
    codes, sc = ops.quantize_blocks_fp4(torch.randn(N, K, generator=g) / K ** 0.5)
    bias = (0.5 * torch.randn(N, generator=g)).to(dt)
    R = torch.randn(M, N, generator=g).to(dt)
    return x, codes, sc, bias, R


@pytest.mark.parametrize("M,N,K", [(5, 40, 384), (16, 16, 4096)])
def test_bound_holds_for_another_summation_order_and_is_not_vacuous(M, N, K):
    dt = torch.bfloat16
    x, codes, sc, bias, R = _case(M, N, K, dt)
    out, bound = w4_rows_model(x, codes, sc, bias, R)
    wd = w4_values(codes, sc)
    assert torch.equal(wd, ops.dequantize_blocks_fp4(codes, sc).double())
    # the same sum in float64, K reversed and cut into 7 chunks added last-first
    xr, wr = x.double().flip(1), wd.flip(1)
    parts = [xr[:, c] @ wr[:, c].T for c in torch.arange(K).chunk(7)]
    other = sum(reversed(parts)) + bias.double()[None] + R.double()
    assert worst((other - out).abs(), bound) < 1e-3
    # what the kernel may do at most: the element type's rounding of the float64 value
    assert 0.25 < worst((out.float().to(dt).double() - out).abs(), bound) <= 1.0
    # not vacuous: a far smaller bound than the result itself ...
    assert bound.max() < 2.0 ** -6 * out.abs().max() and (bound < 2.0 ** -7 * out.abs() + 2.0 ** -11 * x.abs().max() * K ** 0.5).all()
    # ... one weight's sign flipped (the row's largest product) falls outside it ...
    prod = (x.double()[0][None] * wd).abs()
    n = 1
    k = int(prod[n].argmax())
    flipped_codes = codes.clone()
    flipped_codes[n, k // 2] ^= 0x80 if k & 1 else 0x08
    flipped, _ = w4_rows_model(x, flipped_codes, sc, bias, R)
    assert (flipped - out).abs()[0, n] > bound[0, n]
    assert ((flipped - out).abs() > bound)[:, n].any() and not ((flipped - out).abs() > 0)[:, [c for c in range(N) if c != n]].any()
    # ... so do the two nibbles of every byte swapped (the other nibble order) ...
    swapped, _ = w4_rows_model(x, (codes << 4) | (codes >> 4), sc, bias, R)
    print("nibbles swapped: worst error / bound", worst((swapped - out).abs(), bound))
    assert worst((swapped - out).abs(), bound) > 20
    # ... and one block's exponent off by one: the output moves by that block's share of the sum, past the bound nearly everywhere
    sc2 = sc.clone()
    sc2[:, 0] += 1
    off, _ = w4_rows_model(x, codes, sc2, bias, R)
    d = (x.double()[:, :32] @ wd[:, :32].T).abs()              # what that block contributes: the change
    assert torch.allclose((off - out).abs(), d, rtol=1e-12, atol=1e-300)
    assert ((off - out).abs() > bound).double().mean() > 0.5


# ------------------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


def test_gemm_rows_w4_rejects_bad_arguments(lib):
    """u2tok_gemm_rows_w4 returns U2TOK_ERR_ARG before any launch or memory access"""
    P = 1 << 20   # an aligned address that is never dereferenced
    # A, W4, S, C, bias, R, M, N, K, lda, ldw, lds, ldc, ldr, flags, stream
    args = [P, P + 4096, P + 8192, P + 12288, None, None, 4, 32, 128, 128, 64, 4, 32, 0, 0, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.u2tok_gemm_rows_w4(*a)

    for i in (0, 1, 2, 3):
        assert call(**{f"a{i}": None}) == -1, i               # a2: the null block scales
    assert call(a8=64, a9=64, a10=32, a11=2) == -1            # K = 64, 192: not multiples of 128
    assert call(a8=192, a9=192, a10=96, a11=6) == -1
    assert call(a8=0) == -1 and call(a6=0) == -1 and call(a6=65) == -1 and call(a7=0) == -1
    assert call(a0=P + 8) == -1 and call(a1=P + 4096 + 8) == -1   # A / W4 not 16-byte aligned
    assert call(a3=P + 12288 + 1) == -1 and call(a3=P + 12288 + 2, a14=16) == -1    # C not aligned to its type
    assert call(a9=120) == -1 and call(a9=132) == -1          # lda < K, lda not a multiple of 8
    assert call(a10=48) == -1 and call(a10=72) == -1          # ldw < K / 2, ldw not a multiple of 16
    assert call(a11=3) == -1 and call(a12=16) == -1           # lds < K / 32, ldc < N
    assert call(a14=1) == -1 and call(a14=8) == -1            # bias / residual flags without their pointers
    assert call(a14=8, a5=P, a13=16) == -1                    # ldr < N
    assert call(a14=4) == -1 and call(a14=2) == -1 and call(a14=512 | 16) == -1   # unknown flags; the pair form stands alone
    assert call(a14=512, a7=24, a12=12) == -1                 # pair: I % 8 != 0


def test_decode_w4_entry_points_reject_bad_arguments(lib):
    """u2tok_decoder_decode_pre / _post return U2TOK_ERR_ARG before any launch or memory access on an e2m1 step they do not take.
    The form is said by u2tok_decode_config.wform = 2 and the block scales travel in the descriptor's four scale fields (the
    descriptor keeps its 17 pointers), so block scales beside fp32 scales cannot be written down; what can is refused: some or none
    of the four set, an unknown wform, misaligned codes, E / Hq D / I not a multiple of 128.  That the refusals are not a blanket
    one: the descriptor they are derived from passes the admission and stops at the workspace size (U2TOK_ERR_WORKSPACE)."""
    P = 1 << 20
    SCALES = ("scale_qkv", "scale_o", "scale_gu", "scale_down")

    def config(**kw):
        c = _lib.DecodeConfig(B=2, E=128, Hq=4, Hkv=2, D=64, I=256, eps=1e-6, qk_eps=1e-6, scale=0.125, wform=2)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def layer(**kw):   # e2m1 codes with the block scales' addresses behind each, no biases, no q / k norms
        fields = dict(w_in_norm=P, Wqkv=P, Wo=P, w_post_norm=P, Wgu=P, Wdown=P, **{n: P + 1 for n in SCALES})   # (bytes: any address)
        fields.update(kw)
        return _lib.DecodeLayer(**fields)

    def pre(lay, cfg=None, ws_bytes=1 << 20):
        return lib.u2tok_decoder_decode_pre(C.byref(cfg or config()), C.byref(lay), P, P, P, 1, 64, P, P, P, 0, 0, P, ws_bytes, None)

    def post(lay, batched, cfg=None, ws_bytes=1 << 24):
        return lib.u2tok_decoder_decode_post(C.byref(cfg or config()), C.byref(lay), P, P, P, P, 8, 0, batched, None, P, P, ws_bytes, None)

    assert C.sizeof(_lib.DecodeLayer) == 17 * C.sizeof(C.c_void_p) and C.sizeof(_lib.DecodeConfig) == 40
    assert _lib.DecodeConfig._fields_[-1][0] == "wform" and _lib.DecodeConfig(B=1).wform == 0
    assert pre(layer(), ws_bytes=0) == -3 and post(layer(), 0, ws_bytes=0) == -3 and post(layer(), 1, ws_bytes=0) == -3
    for name in SCALES:                                                      # partial block scales: one missing, or one alone
        for lay in (layer(**{name: None}), layer(**{n: None for n in SCALES if n != name})):
            assert pre(lay) == -1 and pre(lay, ws_bytes=0) == -1, name
            assert post(lay, 0) == -1 and post(lay, 1) == -1, name
    none = layer(**{n: None for n in SCALES})                                # none: NOT a 16-bit step (its weights are 4 x as long)
    assert pre(none) == -1 and post(none, 0) == -1 and post(none, 1) == -1
    for w in (1, 3, -1, 4):                                                  # a form the step does not have
        assert pre(layer(), config(wform=w)) == -1 and post(layer(), 1, config(wform=w)) == -1, w
    assert pre(layer(Wqkv=P + 8)) == -1 and post(layer(Wgu=P + 4), 1) == -1  # misaligned codes
    # E, Hq D or I not a multiple of 128 (64 or 192: what the e4m3 step takes)
    for kw in (dict(E=192), dict(E=64), dict(I=192), dict(I=320), dict(Hq=3, Hkv=1), dict(Hq=1, Hkv=1)):
        c2 = config(**kw)
        assert pre(layer(), c2) == -1, kw
        for batched in (0, 1):
            assert post(layer(), batched, c2) == -1, kw


# ---------------------------------------------------------------------------------------------------------- the route on CPU
def _layer_state(m):
    """a patched stub model's layer 0 with what `_decode_state` would have left: the config struct and the packed weights"""
    from u2tokenizer_amd import prefill
    layer = m.model.layers[0]
    st = layer._u2_prefill
    pr = st.layout.projections(layer)
    Wqkv, Wgu = st.layout.product(pr, 0)[1], st.layout.product(pr, 2)[1]
    cfg = layer.self_attn.config
    c = _lib.DecodeConfig(B=1, E=Wqkv.shape[1], Hq=cfg.num_attention_heads, Hkv=cfg.num_key_value_heads,
                          D=layer.self_attn.head_dim, I=Wgu.shape[0] // 2)
    return st, types.SimpleNamespace(cfg=c, keep=(Wqkv, None, Wgu, None)), pr


@pytest.mark.parametrize("kind", ["qwen3", "llama", "phi3"])
def test_precedence_of_e2m1_over_e4m3_over_16_bits_per_layer(kind):
    """`_weight_form` on the stub models of tests/test_decoder_route_host.py: a layer with E, Hq D and I multiples of 128 takes
    e2m1 when fp4_decode is on, with or without fp8_decode; one with multiples of 64 only takes e4m3 when fp8_decode is on and
    16 bits otherwise; the copies are those of the form that ran, and so is the counter `_count` moves."""
    from u2tokenizer_amd import prefill
    for inter, on, want in ((256, dict(fp4_decode=True), 2), (256, dict(fp4_decode=True, fp8_decode=True), 2),
                            (256, dict(fp8_decode=True), 1), (256, {}, 0),
                            (320, dict(fp4_decode=True), 0), (320, dict(fp4_decode=True, fp8_decode=True), 1),
                            (288, dict(fp4_decode=True, fp8_decode=True), 0)):
        m = _model(kind, inter=inter)
        prefill.enable_fused_prefill(m, **on)
        st, d, pr = _layer_state(m)
        assert (d.cfg.E, d.cfg.Hq * d.cfg.D) == (128, 128)
        assert prefill._weight_form(st, d, pr) == want, (kind, inter, on)
        assert (st.w4 is not None) == (want == 2) and (st.w8 is not None) == (want == 1)
        layer = m.model.layers[0]
        assert (prefill.w4_weights(layer) is not None) == (want == 2) and (prefill.w8_weights(layer) is not None) == (want == 1)
        if want == 2:
            pairs = prefill.w4_weights(layer)
            assert len(pairs) == 4 and all(c.dtype == s.dtype == torch.uint8 for c, s in pairs)
            nq = (d.cfg.Hq + 2 * d.cfg.Hkv) * d.cfg.D
            assert [tuple(c.shape) for c, _ in pairs] == [(nq, 64), (128, 64), (2 * inter, 64), (128, inter // 2)]
            assert [tuple(s.shape) for _, s in pairs] == [(nq, 4), (128, 4), (2 * inter, 4), (128, inter // 32)]
            Wo = st.layout.product(pr, 1)[1]
            assert torch.equal(pairs[1][0], ops.quantize_blocks_fp4(Wo)[0])
            # the staleness rule of the e4m3 copies: the same objects while nothing changed, new ones after an in-place change
            assert prefill._weight_form(st, d, pr) == 2 and prefill.w4_weights(layer) is pairs
            with torch.no_grad():
                pr[0].weight.mul_(2)
            assert prefill._weight_form(st, d, pr) == 2 and prefill.w4_weights(layer) is not pairs
        n4, n8, n = dict(prefill.w4_stats), dict(prefill.w8_stats), dict(prefill.stats)
        prefill._count(st, "decode", 1)
        assert prefill.stats["decode"] == n["decode"] + 1
        assert prefill.w4_stats["decode"] == n4["decode"] + (want == 2) and prefill.w8_stats["decode"] == n8["decode"] + (want == 1)
        assert prefill.w4_stats["padded_decode"] == n4["padded_decode"] and prefill.w8_stats["padded_decode"] == n8["padded_decode"]
        # the switch goes off: the copies and the descriptors built from them go with it
        st.variants[(2, False)] = "kept"
        prefill.enable_fused_prefill(m)
        assert st.w4 is None and st.w8 is None and st.variants == {}
        prefill.disable_fused_prefill(m)


def test_cpu_model_with_the_switch_takes_the_stock_layers():
    from u2tokenizer_amd import prefill
    assert prefill.w4_stats.keys() == {"decode", "padded_decode"}
    assert prefill.w8_stats.keys() == {"decode", "padded_decode"}
    assert prefill.stats.keys() == {"prefill", "decode", "padded_prefill", "padded_decode"}
    m = _small()
    x = 0.5 * torch.randn(1, 9, 128, generator=_gen(4))
    with torch.no_grad():
        want = m(inputs_embeds=x, use_cache=True)
        want1 = m(inputs_embeds=x[:, :1], past_key_values=want.past_key_values, use_cache=True).logits
        n0, s0 = dict(prefill.w4_stats), dict(prefill.stats)
        assert prefill.enable_fused_prefill(m, fp4_decode=True) == 2
        assert m.model._u2_stack.fp4 is True and m.model._u2_stack.fp8 is False
        got = m(inputs_embeds=x, use_cache=True)
        got1 = m(inputs_embeds=x[:, :1], past_key_values=got.past_key_values, use_cache=True).logits
    assert torch.equal(got.logits, want.logits) and torch.equal(got1, want1)
    assert prefill.w4_stats == n0 and prefill.stats == s0
    assert all(prefill.w4_weights(lay) is None for lay in m.model.layers)
    prefill.enable_fused_prefill(m)                           # every call sets the switches anew
    assert m.model._u2_stack.fp4 is False
    prefill.disable_fused_prefill(m)
    assert prefill.w4_weights(m.model.layers[0]) is None


def test_u2_config_switch_defaults_off_and_the_table_names_it():
    from u2tokenizer_amd import prefill
    from u2tokenizer_amd.language_model import u2Qwen3Config
    assert not getattr(u2Qwen3Config(), "u2_fused_decode_fp4", False)
    s = {s.kw: s for s in prefill.SWITCHES}["fp4_decode"]
    assert (s.field, s.config, s.default, s.implies, s.needs, s.frees) == ("fp4", "u2_fused_decode_fp4", False, (), (), ("w4",))
    assert "unmeasured on trained weights" in s.doc
    # (the keyword alone, the config attribute alone through `_maybe_fuse` and the teardown: tests/test_switch_table_host.py, which
    #  iterates over SWITCHES)
