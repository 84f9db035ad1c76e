"""GPU: decode steps of 17 .. 64 sequences on the fused step (opt-in, `enable_fused_prefill(model, wide_decode=True)`), in both
element builds.  The few-rows product for 17 .. 64 rows (u2tok_gemm_rows, u2tok_gemm_rows_w8_wide; csrc/rows.h) block by block
against the M <= 16 product BIT FOR BIT -- the contract: a sequence's products do not depend on how many sequences share the
step --, against float64 under the per-element bound of tests/test_w8_host.py, its refusals with poisoned outputs, the two entry
points of the step at B = 40 against the same calls on the row slices, the step through whole decoders under the project's
gate, and `generate` on a left-padded batch of 20 prompts."""
import ctypes as C
import functools

import pytest
import torch

import test_gpu_w8 as W
import test_w8_host as H
from helpers import decisive_decoder_
from u2tokenizer_amd import _lib, synth

pytestmark = pytest.mark.gpu
D = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
EPS = W.EPS
BLOCKS = lambda M: [(r, min(M, r + 16)) for r in range(0, M, 16)]   # noqa: E731


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


def _gen(*key):
    return H._gen(*key)


# ------------------------------------------------------------------------------------------------- 1. the product, bit for bit
FORMS = ["plain", "bias", "residual", "f32"]


@functools.lru_cache(maxsize=4)
def _weight(N, K):
    return (torch.randn(N, K, generator=_gen(40, N, K)) / K ** 0.5).to(D)


def _operands(ops, dt, w8, M, N, K, form):
    """x (M, K), the weight in either form, bias, a residual that is a view of a wider buffer"""
    g = _gen(41, M, N, K, FORMS.index(form))
    x = torch.randn(M, K, generator=g).to(dt).to(D)
    w = _weight(N, K)
    wt = ops.quantize_rows_fp8(w) if w8 else (w.to(dt),)
    bias = (0.5 * torch.randn(N, generator=g)).to(dt).to(D) if form == "bias" else None
    R = torch.randn(M, N + 24, generator=g).to(dt).to(D)[:, 8:8 + N] if form == "residual" else None
    return x, wt, bias, R


def _product(ops, w8, x, wt, **kw):
    return ops.gemm_rows_w8(x, *wt, **kw) if w8 else ops.gemm_rows(x, *wt, **kw)


@pytest.mark.parametrize("K", [64, 192, 4096])
@pytest.mark.parametrize("w8", [False, True], ids=["elem", "e4m3"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_every_block_of_16_rows_has_the_bits_of_the_few_rows_product(ops, dt, w8, K):
    """M in {17, 32, 33, 64} (one row in a second block, full blocks, a ragged third, four) x N in {16, 40, 1040} (40: a partial
    16-column group) x {plain, bias, residual from a strided buffer, fp32 out}: rows 16 b .. of the wide product equal the
    M <= 16 product on those rows.  K = 64: fewer steps than waves (empty slices); 192: 4 waves, an empty or short last slice;
    4096: 16 waves.  Element weights, once per K: the M <= 16 product itself equals u2tok_gemm_bf16's on the same operands."""
    for M in (17, 32, 33, 64):
        for N in (16, 40, 1040):
            for form in FORMS:
                x, wt, bias, R = _operands(ops, dt, w8, M, N, K, form)
                kw = dict(bias=bias, residual=R, out_f32=form == "f32")
                buf = torch.full((M, N + 16), 7.0, dtype=torch.float32 if form == "f32" else dt, device=D)
                got = _product(ops, w8, x, wt, out=buf[:, 8:8 + N], **kw)
                assert (buf[:, :8] == 7).all() and (buf[:, 8 + N:] == 7).all() and torch.isfinite(got).all()
                for r0, r1 in BLOCKS(M):
                    kwb = dict(kw, residual=None if R is None else R[r0:r1])
                    want = _product(ops, w8, x[r0:r1], wt, **kwb)
                    assert torch.equal(got[r0:r1], want), (M, N, K, form, r0, (got[r0:r1].float() - want.float()).abs().max())
                    if not w8 and (M, N) == (33, 40):
                        plan = ops.gemm(x[r0:r1], wt[0], bias=bias, residual=None if R is None else R[r0:r1].contiguous(),
                                        out_f32=form == "f32")
                        assert torch.equal(want, plan.reshape(want.shape)), (K, form, r0)
                assert got.float().abs().max() > 0.1


@pytest.mark.parametrize("M,K,I", [(17, 64, 16), (33, 192, 24), (64, 4096, 12288)])
@pytest.mark.parametrize("w8", [False, True], ids=["elem", "e4m3"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_pair_form_block_by_block(ops, dt, w8, M, K, I):
    """SiLU(gate) * up in the epilogue (flag 512): every block of 16 rows equals the M <= 16 pair form on those rows"""
    g = _gen(43, M, K, I)
    x = torch.randn(M, K, generator=g).to(dt).to(D)
    w = (2.0 * torch.randn(2 * I, K, generator=g) / K ** 0.5).to(D)
    wt = ops.quantize_rows_fp8(w) if w8 else (w.to(dt),)
    got = _product(ops, w8, x, wt, swiglu=True)
    assert got.shape == (M, I) and torch.isfinite(got).all() and got.float().abs().max() > 0.1
    for r0, r1 in BLOCKS(M):
        want = _product(ops, w8, x[r0:r1], wt, swiglu=True)
        assert torch.equal(got[r0:r1], want), (r0, (got[r0:r1].float() - want.float()).abs().max())
    if not w8 and ops.gemm_swiglu_supported(16, K, I):   # ... which is the plan's pair product on 16 rows
        assert torch.equal(got[:16], ops.gemm_swiglu(x[:16], wt[0]).reshape(16, I))


# ----------------------------------------------------------------------------------------------- 2. the product against float64
@pytest.mark.parametrize("w8", [False, True], ids=["elem", "e4m3"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_product_within_the_float64_bound(ops, dt, w8):
    """M = 33, N = 40, K = 4096, bias + residual: every element within tests/test_w8_host.py's w8_rows_model bound as
    tests/test_gpu_w8.py applies it; element-type weights: the same model with the weights as their own codes and unit scales
    (products of two bf16 / fp16 values are exact in fp32, as those of an element and an e4m3 value are)."""
    M, N, K = 33, 40, 4096
    g = _gen(45, M, N, K, int(w8))
    x = torch.randn(M, K, generator=g).to(dt)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    bias = (0.5 * torch.randn(N, generator=g)).to(dt)
    Rbuf = torch.randn(M, N + 24, generator=g).to(dt)
    R = Rbuf[:, 8:8 + N]
    if w8:
        codes, sc = ops.quantize_rows_fp8(w)
        wt = (codes.to(D), sc.to(D))
    else:
        codes, sc = w.to(dt), torch.ones(N)
        wt = (codes.to(D),)
    for f32 in (False, True):
        ref, bound = H.w8_rows_model(x, codes, sc, bias, R, U=H.U_OF[dt], out_f32=f32)
        got = _product(ops, w8, x.to(D), wt, bias=bias.to(D), residual=Rbuf.to(D)[:, 8:8 + N], out_f32=f32)
        err = (got.double().cpu() - ref).abs()
        r = H.worst(err, bound)
        print(f"wide product {'e4m3' if w8 else 'elem'} {IDS[DTYPES.index(dt)]} f32={f32}: worst error / bound {r:.4f}")
        assert torch.isfinite(got).all() and (err <= bound).all(), r


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_refusals_leave_the_outputs_untouched(ops, dt):
    """M = 0, M = 65 and K % 32 != 0 on u2tok_gemm_rows, M = 65 on both e4m3 entry points (and M = 17 on the one that keeps its
    published range), decode_pre / _post at B = 65, _post at B = 17 with batched = 0: U2TOK_ERR_ARG, every output still poison."""
    N, K = 32, 64
    x = torch.randn(65, 96, generator=_gen(47)).to(dt).to(D)
    w = torch.randn(N, 96, generator=_gen(48)).to(dt).to(D)
    w8c, sc = ops.quantize_rows_fp8(w[:, :K].contiguous())
    out = torch.full((65, N), 7.0, dtype=dt, device=D)
    with ops.on_device(x) as (h, stream):
        for M, Kc in ((0, K), (65, K), (20, 48), (20, 80)):
            assert h.u2tok_gemm_rows(x.data_ptr(), w.data_ptr(), out.data_ptr(), None, None, M, N, Kc, 96, 96, N, 0, 0, stream) == -1
        for fn, M in ((h.u2tok_gemm_rows_w8_wide, 65), (h.u2tok_gemm_rows_w8, 65), (h.u2tok_gemm_rows_w8, 17)):
            assert fn(x.data_ptr(), w8c.data_ptr(), sc.data_ptr(), out.data_ptr(), None, None, M, N, K, 96, K, N, 0, 0, stream) == -1
        torch.cuda.synchronize()
        assert (out == 7).all()
        # the step: a layer in either weight form, buffers sized for 65 sequences
        E, Hq, Hkv, d, inter, T = 128, 4, 2, 64, 256, 8
        nq = (Hq + 2 * Hkv) * d
        t = _step_tensors(ops, dt, 65, E, Hq, Hkv, d, inter, T, T, qk_norm=True, biases=False)
        for form in ("elem", "e4m3"):
            lay = t["layer"][form]
            for B, batched, pre in ((65, 1, True), (65, 0, False), (17, 0, False)):
                cfg = _lib.DecodeConfig(B=B, E=E, Hq=Hq, Hkv=Hkv, D=d, I=inter, eps=1e-6, qk_eps=1e-6, scale=d ** -0.5)
                qkv = torch.full((65, nq), 7.0, dtype=dt, device=D)
                kc, vc = t["kb"].clone(), t["vb"].clone()
                o = torch.full((65, E), 7.0, dtype=dt, device=D)
                ws = torch.empty(1 << 24, dtype=torch.uint8, device=D)
                if pre:
                    assert h.u2tok_decoder_decode_pre(C.byref(cfg), C.byref(lay), t["x"].data_ptr(), t["cos"].data_ptr(),
                                                      t["sin"].data_ptr(), 1, d, qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                                      T * d, T - 1, ws.data_ptr(), ws.numel(), stream) == -1
                assert h.u2tok_decoder_decode_post(C.byref(cfg), C.byref(lay), t["x"].data_ptr(), t["qkv"].data_ptr(), kc.data_ptr(),
                                                   vc.data_ptr(), T, T * d, batched, None, o.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   stream) == -1
                torch.cuda.synchronize()
                assert (qkv == 7).all() and (o == 7).all() and torch.equal(kc, t["kb"]) and torch.equal(vc, t["vb"])


# ------------------------------------------------------------------------------------------------ 4. the step at the C level
def _step_tensors(ops, dt, B, E, Hq, Hkv, d, inter, T, cap, qk_norm, biases):
    """synthetic inputs of one decode step: x, rotary tables, cache buffers (B, Hkv, cap, d) filled below position T - 1, a
    finished qkv for calls of the second half alone, and the layer descriptor in both weight forms (tensors kept alive in it)"""
    g = _gen(51, B, E, d, inter)
    r = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).to(dt).to(D)   # noqa: E731
    nq, qd = (Hq + 2 * Hkv) * d, Hq * d
    t = dict(x=r(B, E), qkv=r(B, nq), kb=r(B, Hkv, cap, d), vb=r(B, Hkv, cap, d))
    ang = torch.rand(B, d // 2, generator=g) * 6.28
    t["cos"], t["sin"] = (torch.cat([f(ang), f(ang)], 1).float().contiguous().to(D) for f in (torch.cos, torch.sin))
    norm = lambda n: (1 + 0.1 * torch.randn(n, generator=g)).to(dt).to(D)   # noqa: E731
    W4 = dict(Wqkv=r(nq, E, scale=E ** -0.5), Wo=r(E, qd, scale=qd ** -0.5), Wgu=r(2 * inter, E, scale=2 * E ** -0.5),
              Wdown=r(E, inter, scale=inter ** -0.5))
    small = dict(w_in_norm=norm(E), w_post_norm=norm(E))
    if qk_norm:
        small.update(wq_norm=norm(d), wk_norm=norm(d))
    if biases:
        small.update(bqkv=r(nq, scale=0.3), bo=r(E, scale=0.3), bgu=r(2 * inter, scale=0.3), bdown=r(E, scale=0.3))
    q4 = {k: ops.quantize_rows_fp8(v) for k, v in W4.items()}
    ptr = lambda d_: {k: v.data_ptr() for k, v in d_.items()}   # noqa: E731
    sname = dict(Wqkv="scale_qkv", Wo="scale_o", Wgu="scale_gu", Wdown="scale_down")
    t["layer"] = {"elem": _lib.DecodeLayer(**ptr(W4), **ptr(small)),
                  "e4m3": _lib.DecodeLayer(**{k: v[0].data_ptr() for k, v in q4.items()},
                                           **{sname[k]: v[1].data_ptr() for k, v in q4.items()}, **ptr(small))}
    t["keep"] = (W4, small, q4)
    return t


@pytest.mark.parametrize("form", ["elem", "e4m3"])
@pytest.mark.parametrize("d,qk_norm,biases,starts", [(64, True, False, False), (96, False, True, True), (128, True, False, True)],
                         ids=["d64", "d96-biases-kv_start", "d128-kv_start"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_step_of_40_sequences_equals_the_steps_of_its_row_slices(ops, dt, d, qk_norm, biases, starts, form):
    """u2tok_decoder_decode_pre + _post with B = 40, batched = 1, grouped heads (4 query / 2 kv), T = 70 in cache buffers of
    capacity 96 (kv_stride = 96 d; T = 70 is three key tiles: the batched attention does not split the keys, whose split count
    would depend on B), kv_start NULL or per sequence; biases: the gate | up product with a bias takes the two-launch SwiGLU,
    the others the pair form.  The same two calls on rows [0:16], [16:32], [32:40] of the same buffers give the same `out`, the
    same finished qkv and the same new cache entries, bit for bit."""
    B, E, Hq, Hkv, inter, T, cap = 40, 128, 4, 2, 256, 70, 96
    nq = (Hq + 2 * Hkv) * d
    t = _step_tensors(ops, dt, B, E, Hq, Hkv, d, inter, T, cap, qk_norm, biases)
    lay = t["layer"][form]
    kv_start = (torch.arange(B, dtype=torch.int32) * 7 % 66).to(D) if starts else None   # 0 .. 65: past the first two tiles too

    def run(r0, r1, kb, vb, qkv, out):
        n = r1 - r0
        cfg = _lib.DecodeConfig(B=n, E=E, Hq=Hq, Hkv=Hkv, D=d, I=inter, eps=1e-6, qk_eps=1e-5, scale=d ** -0.5)
        with ops.on_device(t["x"]) as (h, stream):
            ws = torch.empty(h.u2tok_decoder_decode_workspace_bytes(C.byref(cfg), T), dtype=torch.uint8, device=D)
            x, kc, vc = t["x"][r0:r1], kb[r0:r1], vb[r0:r1]
            _lib.check(h.u2tok_decoder_decode_pre(C.byref(cfg), C.byref(lay), x.data_ptr(), t["cos"][r0:r1].data_ptr(),
                                                  t["sin"][r0:r1].data_ptr(), 1, d, qkv[r0:r1].data_ptr(), kc.data_ptr(),
                                                  vc.data_ptr(), cap * d, T - 1, ws.data_ptr(), ws.numel(), stream), "pre")
            _lib.check(h.u2tok_decoder_decode_post(C.byref(cfg), C.byref(lay), x.data_ptr(), qkv[r0:r1].data_ptr(), kc.data_ptr(),
                                                   vc.data_ptr(), T, cap * d, 1, None if kv_start is None else kv_start[r0:r1].data_ptr(),
                                                   out[r0:r1].data_ptr(), ws.data_ptr(), ws.numel(), stream), "post")
        torch.cuda.synchronize()

    def fresh():
        return (t["kb"].clone(), t["vb"].clone(), torch.full((B, nq), float("nan"), dtype=dt, device=D),
                torch.full((B, E), float("nan"), dtype=dt, device=D))

    whole, parts = fresh(), fresh()
    run(0, B, *whole)
    for r0, r1 in BLOCKS(B):
        run(r0, r1, *parts)
    (kw_, vw_, qw, ow), (kp, vp, qp, op) = whole, parts
    assert torch.isfinite(ow).all() and torch.isfinite(qw).all() and ow.float().abs().max() > 0.1
    assert torch.equal(ow, op), (ow.float() - op.float()).abs().max()
    assert torch.equal(qw, qp)
    assert torch.equal(kw_, kp) and torch.equal(vw_, vp)
    assert not torch.equal(kw_[:, :, T - 1], t["kb"][:, :, T - 1]) and torch.equal(kw_[:, :, :T - 1], t["kb"][:, :, :T - 1])
    assert torch.equal(kw_[:, :, T:], t["kb"][:, :, T:])


# ------------------------------------------------------------------------------------------------- 5. the step through models
CASES = {"qwen3-17": ("qwen3", 17, False), "llama-40": ("llama", 40, False), "qwen3-wide-17": ("qwen3", 17, True)}


@functools.lru_cache(maxsize=None)
def _reference(case, padded):
    """the snapped fp32 model's state, the inputs and its outputs for one prefill + one decode step (computed once per case)"""
    kind, B, wide = CASES[case]
    nl, E, S = (1, 4096, 12) if wide else (3, 512, 40)
    m32 = W._small(kind, nl, wide)
    from u2tokenizer_amd import ops as _ops
    _ops.snap_fp8_(m32.model.layers)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, E), 7)
    x1 = 0.5 * synth.synth_tensor("inputs_embeds", (B, 1, E), 8)
    mask = mask1 = None
    if padded:   # pads 0 .. S - 2, every sequence another one where S allows
        mask = torch.ones(B, S, dtype=torch.int64)
        for b in range(B):
            mask[b, :(b * 5) % (S - 1)] = 0
        mask1 = torch.cat([mask, torch.ones(B, 1, dtype=torch.int64)], 1)
    kw, kw1 = ({} if t is None else {"attention_mask": t} for t in (mask, mask1))
    p32 = m32(inputs_embeds=x, use_cache=True, **kw)
    ref = m32(inputs_embeds=x1, past_key_values=p32.past_key_values, use_cache=True, **kw1)
    new = [(lay.keys[:, :, -1:].clone(), lay.values[:, :, -1:].clone()) for lay in ref.past_key_values.layers]
    return dict(state=m32.state_dict(), x=x, x1=x1, mask=mask, mask1=mask1, logits=ref.logits, new=new, nl=nl, S=S)


@functools.lru_cache(maxsize=2)
def _gpu_model(case, padded, dt):
    """the snapped model in `dt` on the GPU (kept across the 16-bit / fp8_decode pair of a case: building it is what costs)"""
    kind, _, wide = CASES[case]
    r = _reference(case, padded)
    mg = W._small(kind, r["nl"], wide)
    mg.load_state_dict(r["state"])
    return mg.to(dt).to(D)


@pytest.mark.parametrize("fp8", [False, True], ids=["16-bit", "fp8_decode"])
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "left-padded"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_wide_decode_step_matches_the_stock_decoder(ops, dt, case, padded, fp8):
    """Snapped weights (the e4m3 step and the 16-bit model compute the same function), a prefill, one decode step of 17 / 40
    sequences: logits and the new cache entries of the first and last layer no further from the fp32 model than 1.5 x the stock
    run of the element type; every layer counted in wide_stats (and in w8_stats with fp8_decode); on the append-in-place cache."""
    from u2tokenizer_amd import prefill
    kind, B, wide = CASES[case]
    r = _reference(case, padded)
    nl, S = r["nl"], r["S"]
    mg = _gpu_model(case, padded, dt)
    xd, x1d = r["x"].to(dt).to(D), r["x1"].to(dt).to(D)
    kwd, kw1d = ({} if t is None else {"attention_mask": t.to(D)} for t in (r["mask"], r["mask1"]))

    def run():
        p = mg(inputs_embeds=xd, use_cache=True, **kwd)
        return mg(inputs_embeds=x1d, past_key_values=p.past_key_values, use_cache=True, **kw1d)

    stock = run()
    prefill.enable_fused_prefill(mg, padded=padded, fp8_decode=fp8, wide_decode=True)
    n0, s0, w0 = dict(prefill.wide_stats), dict(prefill.stats), dict(prefill.w8_stats)
    fused = run()
    prefill.disable_fused_prefill(mg)
    which, other = ("padded_decode", "decode") if padded else ("decode", "padded_decode")
    assert prefill.wide_stats[which] - n0[which] == nl and prefill.wide_stats[other] == n0[other]
    assert prefill.stats[which] - s0[which] == nl
    assert prefill.w8_stats[which] - w0[which] == (nl if fp8 else 0)
    assert type(fused.past_key_values.layers[0]).__name__ == "AppendLayer"
    assert fused.logits.shape == stock.logits.shape == (B, 1, r["logits"].shape[-1]) and torch.isfinite(fused.logits).all()
    assert not torch.equal(fused.logits, stock.logits)
    W._gate(fused.logits, stock.logits, r["logits"], "logits", EPS[dt])
    for li in (0, nl - 1):
        for i, name in enumerate(("keys", "values")):
            f, s = (getattr(o.past_key_values.layers[li], name) for o in (fused, stock))
            assert f.shape[2] == S + 1
            W._gate(f[:, :, -1:], s[:, :, -1:], r["new"][li][i], f"layer {li} new {name}", EPS[dt])


@functools.lru_cache(maxsize=None)
def _phi3_reference():
    Wn, S, n, nl, B = 32, 30, 4, 2, 40
    m32 = W._phi3(nl, Wn)
    from u2tokenizer_amd import ops as _ops
    _ops.snap_fp8_(m32.model.layers)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, 768), 5)
    xs = 0.5 * synth.synth_tensor("inputs_embeds", (B, n, 768), 6)
    return dict(state=m32.state_dict(), x=x, xs=xs, logits=_phi3_steps(m32, x, xs)[0])


def _phi3_steps(m, x, xs):
    from transformers.cache_utils import DynamicCache
    cache = DynamicCache(config=m.config)
    out = [m(inputs_embeds=x, past_key_values=cache, use_cache=True).logits[:, -1]]
    for t in range(xs.shape[1]):
        out.append(m(inputs_embeds=xs[:, t:t + 1], past_key_values=cache, use_cache=True).logits[:, -1])
    return out, cache


@pytest.mark.parametrize("fp8", [False, True], ids=["16-bit", "fp8_decode"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_wide_decode_on_sliding_window_layers(ops, dt, fp8):
    """2 Phi-3 layers (head dim 96, packed projections) with sliding_window = 32 on the cache `generate` builds for them
    (DynamicSlidingWindowLayer: the torch.cat cache path), 40 sequences: a 30-position prefill and 4 steps, to position 33 > W,
    each under the gate."""
    from u2tokenizer_amd import prefill
    r = _phi3_reference()
    n, nl = r["xs"].shape[1], 2
    mg = W._phi3(nl, 32)
    mg.load_state_dict(r["state"])
    mg = mg.to(dt).to(D)
    xd, xsd = r["x"].to(dt).to(D), r["xs"].to(dt).to(D)
    stock, _ = _phi3_steps(mg, xd, xsd)
    prefill.enable_fused_prefill(mg, fp8_decode=fp8, wide_decode=True)
    n0, w0 = dict(prefill.wide_stats), dict(prefill.w8_stats)
    got, cache = _phi3_steps(mg, xd, xsd)
    prefill.disable_fused_prefill(mg)
    assert type(cache.layers[0]).__name__ == "DynamicSlidingWindowLayer"
    assert prefill.wide_stats["decode"] - n0["decode"] == nl * n and prefill.wide_stats["padded_decode"] == n0["padded_decode"]
    assert prefill.w8_stats["decode"] - w0["decode"] == (nl * n if fp8 else 0)
    for t in range(1, n + 1):
        es, ef = W._err(stock[t].float().cpu(), r["logits"][t]), W._err(got[t].float().cpu(), r["logits"][t])
        print(f"step {t}: fused {ef:.3e} stock {es:.3e}")
        assert ef <= 1.5 * es + EPS[dt], (t, ef, es)
        assert not torch.equal(got[t], stock[t]), t


# ------------------------------------------------------------------------------------------------------------- 6. generate
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_generate_on_a_left_padded_batch_of_20_prompts(ops, dt):
    """Greedy generate, 6 new tokens, 20 prompts of 5 .. 40 ids left-padded into one batch, helpers.decisive_decoder_: the ids of
    every sequence equal the unpatched model's at every step up to the first whose fp32 top-2 margin is 0.05 or less (past an
    ambiguous step continuations may differ); at least 3 steps compared per sequence; every decode step of every layer counted."""
    from u2tokenizer_amd import prefill
    B, new, nl = 20, 6, 2
    m32 = decisive_decoder_(W._small("qwen3", layers=nl), 0)
    # (prompt seed SEED: chosen with the fp32 model alone, on the CPU -- see below)
    g = torch.Generator().manual_seed(SEED)
    lens = [int(v) for v in torch.randint(5, 41, (B,), generator=g)]
    lens[0], lens[1] = 40, 5
    prompts = [torch.randint(3, 1024, (n,), generator=g) for n in lens]
    S = max(lens)
    ids = torch.zeros(B, S, dtype=torch.int64)
    mask = torch.zeros(B, S, dtype=torch.int64)
    for b, p in enumerate(prompts):
        ids[b, S - len(p):] = p
        mask[b, S - len(p):] = 1
    kw = dict(max_new_tokens=new, min_new_tokens=new, do_sample=False, pad_token_id=0)
    g32 = m32.generate(input_ids=ids, attention_mask=mask, output_scores=True, return_dict_in_generate=True, **kw)
    top2 = torch.stack([s.topk(2).values for s in g32.scores], 1)                   # (B, new, 2)
    clear = ((top2[..., 0] - top2[..., 1]) > 0.05).long().cumprod(1).sum(1)          # leading steps with a clear decision
    assert clear.tolist() == COMPARED and clear.min() >= 3
    mg = decisive_decoder_(W._small("qwen3", layers=nl), 0).to(dt).to(D)
    g_stock = mg.generate(input_ids=ids.to(D), attention_mask=mask.to(D), **kw).cpu()
    prefill.enable_fused_prefill(mg, padded=True, wide_decode=True)
    n0, s0 = dict(prefill.wide_stats), dict(prefill.stats)
    g_wide = mg.generate(input_ids=ids.to(D), attention_mask=mask.to(D), **kw).cpu()
    prefill.disable_fused_prefill(mg)
    assert g_wide.shape == g_stock.shape == (B, S + new)
    assert prefill.wide_stats["padded_decode"] - n0["padded_decode"] == nl * (new - 1) and prefill.wide_stats["decode"] == n0["decode"]
    assert prefill.stats["padded_prefill"] - s0["padded_prefill"] == nl
    for b in range(B):
        for t in range(int(clear[b])):
            assert g_wide[b, S + t] == g_stock[b, S + t], (b, t, g_wide[b, S:], g_stock[b, S:], g32.sequences[b, -new:])


# The prompt seed of the generate test, chosen on the CPU with the fp32 model alone: among seeds 1 .. 199 the one at which every
# sequence has 3 or more leading steps with a top-2 margin above 0.05 AND the smallest margin among those compared steps is the
# largest (0.091; 117 of the 120 steps are compared).  The fp32 margins of the 20 sequences at the 6 steps there, by sequence:
#   2.53 1.50 1.21 0.55 0.19 1.44 | 0.32 0.45 3.43 2.35 5.40 2.16 | 5.18 4.96 3.15 0.78 1.28 1.89 | 1.62 0.16 1.42 4.74 4.91 1.43
#   2.13 8.69 2.93 1.43 1.87 3.46 | 1.45 2.55 0.43 2.57 2.53 1.31 | 4.06 1.21 1.78 0.47 0.05 0.63 | 0.71 1.37 0.27 1.33 2.41 3.28
#   0.50 1.42 1.72 0.27 3.35 4.55 | 0.18 0.47 0.23 0.37 4.35 2.33 | 4.42 3.91 3.02 1.09 2.77 0.13 | 0.25 0.60 4.78 1.03 0.76 2.25
#   2.30 0.15 1.64 9.51 9.25 10.1 | 4.14 5.86 1.07 2.38 2.84 2.13 | 0.32 5.28 2.75 0.85 0.26 0.61 | 0.20 0.17 2.55 0.47 1.51 2.96
#   0.61 0.81 0.95 1.24 0.44 1.76 | 2.92 2.14 2.75 1.09 5.02 0.03 | 1.43 0.31 2.22 0.09 1.24 3.41 | 3.16 3.54 4.24 7.54 6.52 6.61
SEED = 66
COMPARED = [6, 6, 6, 6, 6, 6, 4, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 5, 6, 6]   # leading clear steps per sequence (re-asserted in the test)
