"""GPU: the MXFP4 (e2m1 codes, e8m0 block scales) weight-only decode step (opt-in, `enable_fused_prefill(model, fp4_decode=True)`),
in both element builds: the few-rows product on 4-bit weights (u2tok_gemm_rows_w4) against float64 under the per-element bound of
tests/test_w4_host.py, every code under every block exponent through one-hot activations (the conversion, the nibble order and the
K mapping of csrc/rows.h), the block-of-16 contract for 17 .. 64 rows, the gate | up pair form against the two-step form bit for
bit, and the route -- decode steps of models whose weights the quantiser keeps exactly (ops.snap_fp4_: the e2m1 step and the 16-bit
model compute the same function) under the project's gate, with padding, a window, adapters, 17 sequences and the e4m3 switch
beside it; staleness of the quantised copies, teardown, layers that keep another form, and `generate`."""
import copy

import pytest
import torch

import test_w4_host as H
from suite_budget import record
from test_gpu_w8 import EPS, _err, _phi3, _small
from u2tokenizer_amd import synth

pytestmark = pytest.mark.gpu
D = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
_RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    yield _ops
    record("gemm_rows_w4_error_over_bound", _RATIOS)


def _gen(*key):
    return H._gen(*key)


def _w4(ops, N, K, g, amp=1.0):
    return ops.quantize_blocks_fp4(amp * torch.randn(N, K, generator=g) / K ** 0.5)


# ------------------------------------------------------------------------------------------------------------- the product
# K = 128: one quad step, 4 waves of which 3 are idle; 384: 4 waves, the last with an empty slice; 2048: 8 waves; 8192: 16 waves
@pytest.mark.parametrize("K", [128, 384, 2048, 8192])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_product_within_the_float64_bound(ops, dt, K):
    """Every element of u2tok_gemm_rows_w4 within w4_rows_model's bound, M in {1, 5, 16} x N in {16, 40, 1040}, the epilogue
    forms rotating over the nine shapes so that each K sees all of them: plain, bias, residual with ldr != N, bias + residual
    into a strided C, fp32 out (+ bias).  Twice, bit-identical."""
    U = H.U_OF[dt]
    forms = ["plain", "bias", "residual", "bias+residual+strided", "f32", "f32+bias"]
    i = 0
    for M in (1, 5, 16):
        for N in (16, 40, 1040):
            form = forms[(i + K // 128) % len(forms)] if (M, N) != (16, 1040) else "bias+residual+strided"
            i += 1
            g = _gen(5, M, N, K)
            x = torch.randn(M, K, generator=g).to(dt)
            codes, sc = _w4(ops, N, K, g)
            bias = (0.5 * torch.randn(N, generator=g)).to(dt) if "bias" in form else None
            Rbuf = torch.randn(M, N + 24, generator=g).to(dt) if "residual" in form else None
            f32 = form.startswith("f32")
            ref, bound = H.w4_rows_model(x, codes, sc, bias, None if Rbuf is None else Rbuf[:, 8:8 + N], U=U, out_f32=f32)
            outs = []
            for _ in range(2):
                kw = {}
                if "strided" in form:
                    buf = torch.full((M, N + 16), 7.0, dtype=dt, device=D)
                    kw["out"] = buf[:, 8:8 + N]
                Rd = None if Rbuf is None else Rbuf.to(D)[:, 8:8 + N]
                got = ops.gemm_rows_w4(x.to(D), codes.to(D), sc.to(D), bias=None if bias is None else bias.to(D), residual=Rd,
                                       out_f32=f32, **kw)
                if "strided" in form:
                    assert (buf[:, :8] == 7).all() and (buf[:, 8 + N:] == 7).all()
                outs.append(got.clone())
            assert torch.equal(outs[0], outs[1]), (M, N, K, form)
            assert outs[0].dtype == (torch.float32 if f32 else dt) and outs[0].shape == (M, N)
            err = (outs[0].double().cpu() - ref).abs()
            r = H.worst(err, bound)
            key = f"{IDS[DTYPES.index(dt)]} M{M} N{N} K{K} {form}"
            _RATIOS[key] = round(r, 4)
            print(f"gemm_rows_w4 {key}: worst error / bound {r:.4f}")
            assert torch.isfinite(outs[0]).all() and (err <= bound).all(), (key, r)


@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_every_code_through_one_hot_rows(ops, dt, K):
    """Every block of 32 holds all 16 codes (twice), in a rotation that differs per row and per block; the block exponents sweep
    [-23, 13] over rows and blocks; x rows are one-hot, so out[m][n] = element(e2m1(code[n][k_m]) 2^x[n][k_m / 32]) EXACTLY (the
    widened weight is exact in the element type, one product, nothing to round): the other nibble order, a block that reaches
    another lane group's scale, a k that activations and weights map differently, or an inexact widening shows as a mismatch
    count with the first indices."""
    N = 40
    k = torch.arange(K)[None, :]
    n = torch.arange(N)[:, None]
    code = (k % 32 + 3 * n + 5 * (k // 32)) % 16
    for b in range(K // 32):
        assert sorted(code[7, 32 * b:32 * b + 32].tolist()) == sorted(2 * list(range(16)))
    assert not torch.equal(code[0, :32], code[0, 32:64]) and not torch.equal(code[0, :32], code[1, :32])
    x = -23 + (7 * n + 3 * torch.arange(K // 32)[None, :]) % 37                        # (N, K / 32)
    assert set(x.flatten().tolist()) == set(range(-23, 14))
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8).contiguous()         # even k in the low nibble
    sc = (x + 127).to(torch.uint8).contiguous()
    vals = H.w4_values(codes, sc)
    assert torch.equal(vals.float().to(dt).double(), vals)                              # exact in the element type
    want = vals.float().to(dt).T                                                        # (K, N): the row a one-hot at k must give
    cd, sd = codes.to(D), sc.to(D)
    eye = torch.eye(K, dtype=dt, device=D)
    got = torch.cat([ops.gemm_rows_w4(eye[r:r + 16], cd, sd) for r in range(0, K, 16)], 0)
    bad = got.cpu() != want
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:8].tolist(), got.cpu()[bad][:8].tolist(), want[bad][:8].tolist())


@pytest.mark.parametrize("K", [384, 8192])
@pytest.mark.parametrize("M", [17, 33, 64])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_block_of_16_contract(ops, dt, M, K):
    """Rows of block b of an M-row product (2 .. 4 blocks in one pass over K) are bit-equal to the M <= 16 product on those rows
    alone, in the plain form (with bias and residual) and in the pair form"""
    g = _gen(9, M, K)
    N, I = 40, 24
    x = torch.randn(M, K, generator=g).to(dt).to(D)
    codes, sc = (t.to(D) for t in _w4(ops, N, K, g))
    pc, ps = (t.to(D) for t in _w4(ops, 2 * I, K, g, 2.0))
    bias = (0.5 * torch.randn(N, generator=g)).to(dt).to(D)
    R = torch.randn(M, N, generator=g).to(dt).to(D)
    plain = ops.gemm_rows_w4(x, codes, sc, bias=bias, residual=R)
    pair = ops.gemm_rows_w4(x, pc, ps, swiglu=True)
    assert plain.shape == (M, N) and pair.shape == (M, I) and torch.isfinite(plain).all() and torch.isfinite(pair).all()
    for r in range(0, M, 16):
        rows = slice(r, min(M, r + 16))
        assert torch.equal(plain[rows], ops.gemm_rows_w4(x[rows], codes, sc, bias=bias, residual=R[rows])), (M, K, r)
        assert torch.equal(pair[rows], ops.gemm_rows_w4(x[rows], pc, ps, swiglu=True)), (M, K, r, "pair")
    assert pair.float().abs().max() > 0.05


@pytest.mark.parametrize("M,K,I", [(1, 128, 16), (7, 384, 24), (16, 4096, 12288)])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_pair_form_equals_the_two_step_form(ops, dt, M, K, I):
    g = _gen(7, M, K, I)
    x = torch.randn(M, K, generator=g).to(dt).to(D)
    codes, sc = ops.quantize_blocks_fp4((2.0 * torch.randn(2 * I, K, generator=g) / K ** 0.5).to(D))
    two = ops.swiglu(ops.gemm_rows_w4(x, codes, sc))
    one = ops.gemm_rows_w4(x, codes, sc, swiglu=True)
    assert one.shape == two.shape == (M, I) and torch.isfinite(one).all()
    assert torch.equal(one, two), (one.float() - two.float()).abs().max()
    assert one.float().abs().max() > 0.1


# --------------------------------------------------------------------------------------------------------------- the route
def _snapped_pair(make, dt, snap=None):
    """the fp32 model with snapped decoder-layer weights and its copy in `dt` on the GPU (exact: snapped weights are in dt)"""
    from u2tokenizer_amd import ops as _ops
    m32 = make()
    (snap or _ops.snap_fp4_)(m32.model.layers)
    mg = copy.deepcopy(m32)
    for a in m32.model.layers.parameters():
        assert torch.equal(a.to(dt).float(), a) or a.dim() != 2
    return m32, mg.to(dt).to(D)


def _gate(fused, stock, ref, what, eps):
    es, ef = _err(stock.float().cpu(), ref), _err(fused.float().cpu(), ref)
    print(f"{what}: w4 {ef:.3e} stock {es:.3e}")
    assert torch.isfinite(fused).all() and ef <= 1.5 * es + eps, (what, ef, es)


def _masks(B, S, padded):
    """() or the 2-D masks of a left-padded batch (pads 0 / 7): prefill and step, on the CPU and on the GPU"""
    if not padded:
        return {}, {}, {}, {}
    mask = torch.ones(B, S, dtype=torch.int64)
    mask[1, :7] = 0
    mask1 = torch.cat([mask, torch.ones(B, 1, dtype=torch.int64)], 1)
    return tuple({"attention_mask": t} for t in (mask, mask1, mask.to(D), mask1.to(D)))


def _two_calls(m, x, x1, kw, kw1):
    p = m(inputs_embeds=x, use_cache=True, **kw)
    return m(inputs_embeds=x1, past_key_values=p.past_key_values, use_cache=True, **kw1)


@pytest.mark.parametrize("kind,B,wide", [("qwen3", 1, False), ("llama", 2, False), ("qwen3", 2, True)])
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "left-padded"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_w4_decode_step_matches_the_stock_decoder(ops, dt, padded, kind, B, wide):
    """Snapped weights, a 40-position prefill, one decode step on e2m1 weights: logits and the new cache entries of the first
    and last layer no further from the fp32 model than 1.5 x the stock run of the element type (+ the EPS of
    tests/test_gpu_w8.py); every layer counted in w4_stats, w8_stats unmoved.  left-padded: the same with pads 0 / 7 under
    padded=True (batch >= 2).  That another kernel ran on other weights is shown by the counter and by zeroing the codes of one
    projection in place (the source weight untouched): the next step's logits change, without a rebuild."""
    from u2tokenizer_amd import prefill
    if padded and B == 1:
        B = 2
    nl, E, S = (1, 4096, 40) if wide else (3, 512, 40)
    m32, mg = _snapped_pair(lambda: _small(kind, nl, wide), dt)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, E), 7)
    x1 = 0.5 * synth.synth_tensor("inputs_embeds", (B, 1, E), 8)
    kw, kw1, kwd, kw1d = _masks(B, S, padded)
    ref = _two_calls(m32, x, x1, kw, kw1)
    xd, x1d = x.to(dt).to(D), x1.to(dt).to(D)
    stock = _two_calls(mg, xd, x1d, kwd, kw1d)
    prefill.enable_fused_prefill(mg, padded=padded, fp4_decode=True)
    n0, e0, s0 = dict(prefill.w4_stats), dict(prefill.w8_stats), dict(prefill.stats)
    w4 = _two_calls(mg, xd, x1d, kwd, kw1d)
    which, other = ("padded_decode", "decode") if padded else ("decode", "padded_decode")
    assert prefill.w4_stats[which] - n0[which] == nl and prefill.w4_stats[other] == n0[other]
    assert prefill.stats[which] - s0[which] == nl and prefill.stats.keys() == s0.keys() and prefill.w8_stats == e0
    pairs = prefill.w4_weights(mg.model.layers[0])
    assert pairs is not None and len(pairs) == 4 and all(c.dtype == torch.uint8 and s.dtype == torch.uint8 for c, s in pairs)
    assert all(c.shape[1] * 2 == s.shape[1] * 32 and c.shape[0] == s.shape[0] for c, s in pairs)
    assert prefill.w8_weights(mg.model.layers[0]) is None
    pairs[3][0].zero_()                                                       # the down projection's codes of layer 0
    poisoned = _two_calls(mg, xd, x1d, kwd, kw1d)
    assert prefill.w4_weights(mg.model.layers[0])[3][0] is pairs[3][0]        # (no rebuild: the source weight did not change)
    assert not torch.equal(poisoned.logits, w4.logits)
    prefill.disable_fused_prefill(mg)
    assert w4.logits.shape == stock.logits.shape == (B, 1, ref.logits.shape[-1])
    _gate(w4.logits, stock.logits, ref.logits, "logits", EPS[dt])
    for li in (0, nl - 1):
        for name in ("keys", "values"):
            f, s, r = (getattr(o.past_key_values.layers[li], name) for o in (w4, stock, ref))
            assert f.shape == r.shape and f.shape[2] == S + 1
            _gate(f[:, :, -1:], s[:, :, -1:], r[:, :, -1:], f"layer {li} new {name}", EPS[dt])


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_w4_decode_on_a_sliding_window_layer(ops, dt):
    """Phi-3 layers with sliding_window = 32 on the cache `generate` builds for them: a 24-position prefill and 16 steps, up to
    position 39 > W, each under the gate and on e2m1 weights."""
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd import prefill
    W, S, n, nl = 32, 24, 16, 2
    m32, mg = _snapped_pair(lambda: _phi3(nl, W), dt)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (1, S, 768), 5)
    xs = 0.5 * synth.synth_tensor("inputs_embeds", (1, n, 768), 6)

    def steps(m, x, xs):
        cache = DynamicCache(config=m.config)
        out = [m(inputs_embeds=x, past_key_values=cache, use_cache=True).logits[:, -1]]
        for t in range(xs.shape[1]):
            out.append(m(inputs_embeds=xs[:, t:t + 1], past_key_values=cache, use_cache=True).logits[:, -1])
        return out, cache

    ref, _ = steps(m32, x, xs)
    stock, _ = steps(mg, x.to(dt).to(D), xs.to(dt).to(D))
    prefill.enable_fused_prefill(mg, fp4_decode=True)
    n0 = dict(prefill.w4_stats)
    got, cache = steps(mg, x.to(dt).to(D), xs.to(dt).to(D))
    prefill.disable_fused_prefill(mg)
    assert type(cache.layers[0]).__name__ == "DynamicSlidingWindowLayer"
    assert prefill.w4_stats["decode"] - n0["decode"] == nl * n
    for t in range(1, n + 1):
        _gate(got[t], stock[t], ref[t], f"step {t}", EPS[dt])


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_w4_decode_with_unmerged_adapters(ops, dt):
    """lora=True with fp4_decode=True: a Qwen3 model with every projection wrapped (the adapters of tests/test_gpu_lora_infer.py;
    fp32 adapters, as peft keeps them beside an fp16 base), base weights snapped: one step under the gate against the wrapped fp32
    model, on e2m1 base weights with the adapter groups behind the products (a gate / up adapter: the pair in its unfused form);
    both counters move."""
    from test_gpu_lora_infer import _wrapped
    from u2tokenizer_amd import prefill
    nl, B, S = 2, 2, 37
    m32, mg = _snapped_pair(lambda: _small("qwen3", nl), dt)
    m32, mg = _wrapped(m32), _wrapped(mg, torch.float32)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, 512), 7)
    x1 = 0.5 * synth.synth_tensor("inputs_embeds", (B, 1, 512), 8)
    xd, x1d = x.to(dt).to(D), x1.to(dt).to(D)
    ref = _two_calls(m32, x, x1, {}, {})
    stock = _two_calls(mg, xd, x1d, {}, {})
    assert prefill.enable_fused_prefill(mg, lora=True, fp4_decode=True) == nl
    n0, l0, e0 = dict(prefill.w4_stats), dict(prefill.lora_stats), dict(prefill.w8_stats)
    got = _two_calls(mg, xd, x1d, {}, {})
    assert prefill.w4_stats["decode"] - n0["decode"] == nl and prefill.lora_stats["decode"] - l0["decode"] == nl
    assert prefill.lora_stats["adapters"] - l0["adapters"] == 2 * nl * 7 and prefill.w8_stats == e0
    prefill.disable_fused_prefill(mg)
    _gate(got.logits, stock.logits, ref.logits, "logits with adapters", EPS[dt])


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_w4_decode_of_17_sequences(ops, dt):
    """wide_decode=True at B = 17 (two blocks of 16 rows in one pass over the codes): one step under the gate; wide_stats and
    w4_stats both move"""
    from u2tokenizer_amd import prefill
    nl, B, S = 2, 17, 21
    m32, mg = _snapped_pair(lambda: _small("llama", nl), dt)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, 512), 7)
    x1 = 0.5 * synth.synth_tensor("inputs_embeds", (B, 1, 512), 8)
    xd, x1d = x.to(dt).to(D), x1.to(dt).to(D)
    ref = _two_calls(m32, x, x1, {}, {})
    stock = _two_calls(mg, xd, x1d, {}, {})
    prefill.enable_fused_prefill(mg, wide_decode=True, fp4_decode=True)
    n0, w0 = dict(prefill.w4_stats), dict(prefill.wide_stats)
    got = _two_calls(mg, xd, x1d, {}, {})
    assert prefill.w4_stats["decode"] - n0["decode"] == nl and prefill.wide_stats["decode"] - w0["decode"] == nl
    prefill.disable_fused_prefill(mg)
    _gate(got.logits, stock.logits, ref.logits, "logits of 17 sequences", EPS[dt])


def test_both_switches_each_layer_takes_the_first_form_it_qualifies_for(ops):
    """fp4_decode and fp8_decode on, a model whose layer 0 has I = 1600 (a multiple of 64, not of 128: e4m3) and whose layer 1
    qualifies for e2m1: each counter moves by one per step, each layer keeps the copies of its form, the step is under the gate"""
    from u2tokenizer_amd import ops as _ops
    from u2tokenizer_amd import prefill
    dt = torch.bfloat16

    def make():
        m = _small("qwen3", 2)
        cfg = copy.deepcopy(m.config)
        cfg.intermediate_size = 1600
        m.model.layers[0].mlp = type(m.model.layers[0].mlp)(cfg)
        synth.fill_module_(m, seed=17, prefix="decoder.")
        return m.eval()

    def snap(layers):
        _ops.snap_fp8_(layers[0]), _ops.snap_fp4_(layers[1])

    m32, mg = _snapped_pair(make, dt, snap)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (2, 40, 512), 7)
    x1 = 0.5 * synth.synth_tensor("inputs_embeds", (2, 1, 512), 8)
    xd, x1d = x.to(dt).to(D), x1.to(dt).to(D)
    ref = _two_calls(m32, x, x1, {}, {})
    stock = _two_calls(mg, xd, x1d, {}, {})
    prefill.enable_fused_prefill(mg, fp4_decode=True, fp8_decode=True)
    n4, n8, s0 = dict(prefill.w4_stats), dict(prefill.w8_stats), dict(prefill.stats)
    got = _two_calls(mg, xd, x1d, {}, {})
    assert prefill.w4_stats["decode"] - n4["decode"] == 1 and prefill.w8_stats["decode"] - n8["decode"] == 1
    assert prefill.stats["decode"] - s0["decode"] == 2
    l0, l1 = mg.model.layers
    assert prefill.w8_weights(l0) is not None and prefill.w4_weights(l0) is None
    assert prefill.w4_weights(l1) is not None and prefill.w8_weights(l1) is None
    prefill.disable_fused_prefill(mg)
    _gate(got.logits, stock.logits, ref.logits, "logits, e4m3 layer + e2m1 layer", EPS[dt])


def test_stale_copies_teardown_and_layers_that_keep_the_16_bit_step(ops):
    from u2tokenizer_amd import prefill
    dt = torch.bfloat16
    _, mg = _snapped_pair(lambda: _small("qwen3", 2), dt)
    plain = copy.deepcopy(mg)                     # never patched: the stock outputs, and stock-filled caches
    xd = (0.5 * synth.synth_tensor("inputs_embeds", (2, 40, 512), 7)).to(dt).to(D)
    x1d = (0.5 * synth.synth_tensor("inputs_embeds", (2, 1, 512), 8)).to(dt).to(D)

    def step(m, pre=None):   # pre: the model that fills the cache (`plain`: a DynamicLayer cache, the torch.cat path of the step)
        p = (pre or m)(inputs_embeds=xd, use_cache=True)
        return m(inputs_embeds=x1d, past_key_values=p.past_key_values, use_cache=True).logits

    unpatched = step(plain)
    prefill.enable_fused_prefill(mg, fp4_decode=True)
    n0 = prefill.w4_stats["decode"]
    first, first_cat = step(mg), step(mg, pre=plain)
    assert prefill.w4_stats["decode"] - n0 == 4
    assert torch.isfinite(first_cat).all() and _err(first_cat.float(), first.float()) < 5e-2
    pairs0 = prefill.w4_weights(mg.model.layers[1])
    # a projection changes in place: the next step follows the new weight -- the bits of a model enabled after the change
    mg.model.layers[1].mlp.down_proj.weight.mul_(2)
    after = step(mg)
    assert not torch.equal(after, first)
    new = prefill.w4_weights(mg.model.layers[1])
    assert torch.equal(new[3][1], pairs0[3][1] + 1) and torch.equal(new[3][0], pairs0[3][0])   # the down projection: x + 1, the same codes
    fresh = copy.deepcopy(plain)
    fresh.model.layers[1].mlp.down_proj.weight.mul_(2)
    prefill.enable_fused_prefill(fresh, fp4_decode=True)
    assert torch.equal(step(fresh), after)
    prefill.disable_fused_prefill(fresh)
    # ... and so does a load_state_dict (same storage, new values)
    mg.load_state_dict({k: v.clone() for k, v in plain.state_dict().items()})
    assert torch.equal(step(mg), first)
    # teardown: no copies left, the stock output bit-identical to the model that never was patched
    prefill.disable_fused_prefill(mg)
    assert all(prefill.w4_weights(lay) is None for lay in mg.model.layers)
    assert torch.equal(step(mg), unpatched)
    # I = 1568 (a multiple of 32, not of 64): the layers keep the 16-bit step, bit for bit what fp4_decode=False gives
    m2 = _small("qwen3", 2, inter=1568).to(dt).to(D)
    prefill.enable_fused_prefill(m2)
    want = step(m2)
    prefill.enable_fused_prefill(m2, fp4_decode=True)
    assert m2.model._u2_stack.fp4
    n0, s0 = dict(prefill.w4_stats), prefill.stats["decode"]
    got = step(m2)
    assert prefill.w4_stats == n0 and prefill.stats["decode"] - s0 == 2 and torch.equal(got, want)
    assert all(prefill.w4_weights(lay) is None for lay in m2.model.layers)
    prefill.disable_fused_prefill(m2)


GENERATE_SEED = 38


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_generate_on_e2m1_weights(ops, dt):
    """Greedy generate, 6 new tokens, snapped weights: ids equal the fp32 model's and the stock run's at every step where the
    fp32 top-2 margin exceeds 0.05 (past an ambiguous step continuations may differ); at least 3 steps compared; every decode
    step of every layer ran on e2m1 weights.
    Prompt seed 38: chosen among seeds 20 .. 59 on the fp32 snapped model alone, on the CPU, for the widest smallest margin -- its
    top-2 margins at the six steps are 0.273, 0.787, 0.220, 1.671, 0.593, 1.733."""
    from u2tokenizer_amd import prefill
    nl, new = 2, 6
    m32, mg = _snapped_pair(lambda: _small("qwen3", nl), dt)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (1, 48, 512), GENERATE_SEED)
    g32 = m32.generate(inputs_embeds=x, max_new_tokens=new, do_sample=False, output_scores=True, return_dict_in_generate=True)
    g_stock = mg.generate(inputs_embeds=x.to(dt).to(D), max_new_tokens=new, do_sample=False).cpu()
    prefill.enable_fused_prefill(mg, fp4_decode=True)
    n0 = prefill.w4_stats["decode"]
    g_w4 = mg.generate(inputs_embeds=x.to(dt).to(D), max_new_tokens=new, do_sample=False).cpu()
    prefill.disable_fused_prefill(mg)
    assert g_w4.shape == g_stock.shape == g32.sequences.shape
    assert g_w4.shape[1] == new and prefill.w4_stats["decode"] - n0 == nl * (g_w4.shape[1] - 1)
    compared = 0
    for t in range(new):
        top2 = g32.scores[t][0].topk(2).values
        if (top2[0] - top2[1]).item() <= 0.05:
            break
        assert g_w4[0, t] == g32.sequences[0, t] == g_stock[0, t], (t, g_w4, g_stock, g32.sequences)
        compared += 1
    assert compared >= 3, compared
