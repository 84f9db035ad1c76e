"""GPU: the FP8 (e4m3) weight-only decode step (opt-in, `enable_fused_prefill(model, fp8_decode=True)`), in both element builds:
the few-rows product on 1-byte weights (u2tok_gemm_rows_w8) against float64 under the per-element bound of
tests/test_w8_host.py, every finite e4m3 code through one-hot activations (the conversion and the K mapping of
csrc/rows.h), the gate | up pair form against the two-step form bit for bit, and the route -- decode steps of models whose
weights the quantiser keeps exactly (ops.snap_fp8_: the e4m3 step and the 16-bit model compute the same function) under the
project's gate, staleness of the quantised copies, teardown, layers that keep the 16-bit step, and `generate`."""
import pytest
import torch

import test_w8_host as H
from suite_budget import record
from u2tokenizer_amd import synth

pytestmark = pytest.mark.gpu
D = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
EPS = {torch.bfloat16: 1e-3, torch.float16: 1.5e-4}
_RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    yield _ops
    record("gemm_rows_w8_error_over_bound", _RATIOS)


def _gen(*key):
    return H._gen(*key)


# ------------------------------------------------------------------------------------------------------------- the product
# K = 64: one double step, 4 waves of which 3 are idle; 192: 4 waves, the last with an empty slice; 1024: 8 waves; 4096: 16 waves
@pytest.mark.parametrize("K", [64, 192, 1024, 4096])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_product_within_the_float64_bound(ops, dt, K):
    """Every element of u2tok_gemm_rows_w8 within w8_rows_model's bound, M in {1, 5, 16} x N in {16, 40, 1040}, the epilogue
    forms rotating over the nine shapes so that each K sees all of them: plain, bias, residual with ldr != N, bias + residual
    into a strided C, fp32 out (+ bias).  Twice, bit-identical."""
    U = H.U_OF[dt]
    forms = ["plain", "bias", "residual", "bias+residual+strided", "f32", "f32+bias"]
    i = 0
    for M in (1, 5, 16):
        for N in (16, 40, 1040):
            form = forms[(i + K // 64) % len(forms)] if (M, N) != (16, 1040) else "bias+residual+strided"
            i += 1
            g = _gen(5, M, N, K)
            x = torch.randn(M, K, generator=g).to(dt)
            w8, sc = ops.quantize_rows_fp8(torch.randn(N, K, generator=g) / K ** 0.5)
            bias = (0.5 * torch.randn(N, generator=g)).to(dt) if "bias" in form else None
            Rbuf = torch.randn(M, N + 24, generator=g).to(dt) if "residual" in form else None
            f32 = form.startswith("f32")
            ref, bound = H.w8_rows_model(x, w8, sc, bias, None if Rbuf is None else Rbuf[:, 8:8 + N], U=U, out_f32=f32)
            outs = []
            for _ in range(2):
                kw = {}
                if "strided" in form:
                    buf = torch.full((M, N + 16), 7.0, dtype=dt, device=D)
                    kw["out"] = buf[:, 8:8 + N]
                Rd = None if Rbuf is None else Rbuf.to(D)[:, 8:8 + N]
                got = ops.gemm_rows_w8(x.to(D), w8.to(D), sc.to(D), bias=None if bias is None else bias.to(D), residual=Rd,
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
            print(f"gemm_rows_w8 {key}: worst error / bound {r:.4f}")
            assert torch.isfinite(outs[0]).all() and (err <= bound).all(), (key, r)


@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_every_finite_code_through_one_hot_rows(ops, dt, K):
    """W8 rows hold all 254 finite codes (+-0, the subnormals, +-448), each row in another rotation; x rows are one-hot, so
    out[m][n] = element(scale[n] * e4m3(W8[n][k_m])) EXACTLY (one fp32 product, one rounding): a wrong conversion or any k
    that the activations and the weights map differently shows."""
    N = 40
    k = torch.arange(K)[None, :]
    n = torch.arange(N)[:, None]
    codes = ((k * 5 + n * 37 + (k // 256) * 11) % 256).to(torch.uint8)          # (5 is odd: each 256 columns hold every code)
    codes = torch.where((codes & 0x7F) == 0x7F, torch.tensor(0x3A, dtype=torch.uint8), codes)   # the two NaN codes
    assert set(codes[0, :256].tolist()) | {0x7F, 0xFF} == set(range(256))
    w8 = codes.view(torch.float8_e4m3fn)
    sc = (0.5 + torch.rand(N, generator=_gen(6))) * 2.0 ** -3
    want = (w8.float() * sc[:, None]).to(dt).T                                   # (K, N): the row a one-hot at k must give
    w8d, scd = w8.to(D), sc.to(D)
    eye = torch.eye(K, dtype=dt, device=D)
    got = torch.cat([ops.gemm_rows_w8(eye[r:r + 16], w8d, scd) for r in range(0, K, 16)], 0)
    bad = got.cpu() != want
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:8].tolist())


@pytest.mark.parametrize("M,K,I", [(1, 64, 16), (7, 192, 24), (16, 4096, 12288)])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_pair_form_equals_the_two_step_form(ops, dt, M, K, I):
    g = _gen(7, M, K, I)
    x = torch.randn(M, K, generator=g).to(dt).to(D)
    w8, sc = ops.quantize_rows_fp8((2.0 * torch.randn(2 * I, K, generator=g) / K ** 0.5).to(D))
    two = ops.swiglu(ops.gemm_rows_w8(x, w8, sc))
    one = ops.gemm_rows_w8(x, w8, sc, swiglu=True)
    assert one.shape == two.shape == (M, I) and torch.isfinite(one).all()
    assert torch.equal(one, two), (one.float() - two.float()).abs().max()
    assert one.float().abs().max() > 0.1


# --------------------------------------------------------------------------------------------------------------- the route
def _small(kind, layers=3, wide=False, inter=1536):
    """(the constructors of tests/test_gpu_prefill.py)"""
    from transformers import LlamaConfig, LlamaForCausalLM, Qwen3Config, Qwen3ForCausalLM
    common = dict(vocab_size=1024, hidden_size=512, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=8,
                  num_key_value_heads=4, head_dim=64, max_position_embeddings=512, tie_word_embeddings=False,
                  pad_token_id=0, bos_token_id=1, eos_token_id=2)
    if wide:  # one layer at the Qwen3-8B width
        common.update(hidden_size=4096, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8, head_dim=128)
    if kind == "qwen3":
        m = Qwen3ForCausalLM(Qwen3Config(**common))
    else:
        m = LlamaForCausalLM(LlamaConfig(**common, rope_theta=500000.0))
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m.eval()


def _phi3(layers=2, window=32):
    from transformers import Phi3Config, Phi3ForCausalLM
    m = Phi3ForCausalLM(Phi3Config(vocab_size=1024, hidden_size=768, intermediate_size=2048, num_hidden_layers=layers,
                                   num_attention_heads=8, num_key_value_heads=8, max_position_embeddings=4096,
                                   sliding_window=window, tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2))
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m.eval()


def _snapped_pair(make, dt):
    """the fp32 model with snapped decoder-layer weights and its copy in `dt` on the GPU (exact: snapped weights are in dt)"""
    from u2tokenizer_amd import ops as _ops
    m32 = make()
    _ops.snap_fp8_(m32.model.layers)
    mg = make()
    mg.load_state_dict(m32.state_dict())
    for a, b in zip(m32.model.layers.parameters(), mg.model.layers.parameters()):
        assert torch.equal(a.to(dt).float(), a) or a.dim() != 2
    return m32, mg.to(dt).to(D)


def _err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _gate(fused, stock, ref, what, eps):
    es, ef = _err(stock.float().cpu(), ref), _err(fused.float().cpu(), ref)
    print(f"{what}: w8 {ef:.3e} stock {es:.3e}")
    assert ef <= 1.5 * es + eps, (what, ef, es)


@pytest.mark.parametrize("kind,B,wide", [("qwen3", 1, False), ("llama", 2, False), ("qwen3", 2, True)])
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "left-padded"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_w8_decode_step_matches_the_stock_decoder(ops, dt, padded, kind, B, wide):
    """Snapped weights, a 40-position prefill, one decode step on e4m3 weights: logits and the new cache entries of the first
    and last layer no further from the fp32 model than 1.5 x the stock run of the element type; every layer counted in
    w8_stats; not the stock run's bits.  left-padded: the same with pads 0 / 7 under padded=True (batch >= 2).
    That another kernel ran on other weights is shown by the counter and by zeroing the e4m3 copy of one projection in place
    (the source weight untouched): the next step's logits change.  Comparing bits with the 16-bit fused step cannot show it: on
    snapped weights both steps compute the same function from products that are exact in fp32 (8 x 4 significant bits, scales
    powers of two), so they differ in the order of fp32 additions only, and after the rounding to the element type the logits
    of the small models come out bit-identical (measured on the MI355X: qwen3, B = 1, bf16 -- all 1024 logits equal)."""
    from u2tokenizer_amd import prefill
    if padded and B == 1:
        B = 2
    nl, E, S = (1, 4096, 40) if wide else (3, 512, 40)
    m32, mg = _snapped_pair(lambda: _small(kind, nl, wide), dt)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, E), 7)
    x1 = 0.5 * synth.synth_tensor("inputs_embeds", (B, 1, E), 8)
    kw, kw1, kwd, kw1d = {}, {}, {}, {}
    if padded:
        mask = torch.ones(B, S, dtype=torch.int64)
        mask[1, :7] = 0
        mask1 = torch.cat([mask, torch.ones(B, 1, dtype=torch.int64)], 1)
        kw, kw1, kwd, kw1d = ({"attention_mask": t} for t in (mask, mask1, mask.to(D), mask1.to(D)))
    p32 = m32(inputs_embeds=x, use_cache=True, **kw)
    ref = m32(inputs_embeds=x1, past_key_values=p32.past_key_values, use_cache=True, **kw1)
    xd, x1d = x.to(dt).to(D), x1.to(dt).to(D)

    def run():
        p = mg(inputs_embeds=xd, use_cache=True, **kwd)
        return mg(inputs_embeds=x1d, past_key_values=p.past_key_values, use_cache=True, **kw1d)

    stock = run()
    prefill.enable_fused_prefill(mg, padded=padded)
    fused16 = run()
    prefill.enable_fused_prefill(mg, padded=padded, fp8_decode=True)
    n0, s0 = dict(prefill.w8_stats), dict(prefill.stats)
    w8 = run()
    which, other = ("padded_decode", "decode") if padded else ("decode", "padded_decode")
    assert prefill.w8_stats[which] - n0[which] == nl and prefill.w8_stats[other] == n0[other]
    assert prefill.stats[which] - s0[which] == nl and prefill.stats.keys() == s0.keys()
    pairs = prefill.w8_weights(mg.model.layers[0])
    assert pairs is not None and len(pairs) == 4 and all(w.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 for w, s in pairs)
    assert type(w8.past_key_values.layers[0]).__name__ == "AppendLayer"       # (the append-in-place cache path)
    pairs[3][0].view(torch.uint8).zero_()                                     # the down projection's codes of layer 0
    poisoned = run()
    assert prefill.w8_weights(mg.model.layers[0])[3][0] is pairs[3][0]        # (no rebuild: the source weight did not change)
    assert not torch.equal(poisoned.logits, w8.logits)
    prefill.disable_fused_prefill(mg)
    assert w8.logits.shape == stock.logits.shape == (B, 1, ref.logits.shape[-1]) and torch.isfinite(w8.logits).all()
    print("bits equal to the 16-bit fused step's:", torch.equal(w8.logits, fused16.logits))
    assert not torch.equal(w8.logits, stock.logits)
    _gate(w8.logits, stock.logits, ref.logits, "logits", EPS[dt])
    for li in (0, nl - 1):
        for name in ("keys", "values"):
            f, s, r = (getattr(o.past_key_values.layers[li], name) for o in (w8, stock, ref))
            assert f.shape == r.shape and f.shape[2] == S + 1
            _gate(f[:, :, -1:], s[:, :, -1:], r[:, :, -1:], f"layer {li} new {name}", EPS[dt])


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_w8_decode_on_a_sliding_window_layer(ops, dt):
    """Phi-3 layers with sliding_window = 32 on the cache `generate` builds for them (DynamicSlidingWindowLayer: the torch.cat
    cache path): a 24-position prefill and 16 steps, up to position 39 > W, each under the gate and on e4m3 weights."""
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
    prefill.enable_fused_prefill(mg, fp8_decode=True)
    n0 = dict(prefill.w8_stats)
    got, cache = steps(mg, x.to(dt).to(D), xs.to(dt).to(D))
    prefill.disable_fused_prefill(mg)
    assert type(cache.layers[0]).__name__ == "DynamicSlidingWindowLayer"
    assert prefill.w8_stats["decode"] - n0["decode"] == nl * n
    for t in range(1, n + 1):
        es, ef = _err(stock[t].float().cpu(), ref[t]), _err(got[t].float().cpu(), ref[t])
        assert ef <= 1.5 * es + EPS[dt], (t, ef, es)
        assert not torch.equal(got[t], stock[t]), t


def test_stale_copies_teardown_and_layers_that_keep_the_16_bit_step(ops):
    import copy
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
    prefill.enable_fused_prefill(mg, fp8_decode=True)
    n0 = prefill.w8_stats["decode"]
    first, first_cat = step(mg), step(mg, pre=plain)
    assert prefill.w8_stats["decode"] - n0 == 4
    assert torch.isfinite(first_cat).all() and _err(first_cat.float(), first.float()) < 5e-2
    assert not torch.equal(first_cat, unpatched)
    pairs0 = prefill.w8_weights(mg.model.layers[1])
    # a projection changes in place: the next step follows the new weight -- the bits of a model enabled after the change
    mg.model.layers[1].mlp.down_proj.weight.mul_(2)
    after = step(mg)
    assert not torch.equal(after, first)
    assert torch.equal(prefill.w8_weights(mg.model.layers[1])[3][1], 2 * pairs0[3][1])      # the down projection's scales
    fresh = copy.deepcopy(plain)
    fresh.model.layers[1].mlp.down_proj.weight.mul_(2)
    prefill.enable_fused_prefill(fresh, fp8_decode=True)
    assert torch.equal(step(fresh), after)
    prefill.disable_fused_prefill(fresh)
    # ... and so does a load_state_dict (same storage, new values)
    mg.load_state_dict({k: v.clone() for k, v in plain.state_dict().items()})
    assert torch.equal(step(mg), first)
    # teardown: no copies left, the stock output bit-identical to the model that never was patched
    prefill.disable_fused_prefill(mg)
    assert all(prefill.w8_weights(lay) is None for lay in mg.model.layers)
    assert torch.equal(step(mg), unpatched)
    # I = 1568 (a multiple of 32, not of 64): the layers keep the 16-bit step, bit for bit what fp8_decode=False gives
    m2 = _small("qwen3", 2, inter=1568).to(dt).to(D)
    prefill.enable_fused_prefill(m2)
    want = step(m2)
    prefill.enable_fused_prefill(m2, fp8_decode=True)
    assert m2.model._u2_stack.fp8
    n0, s0 = dict(prefill.w8_stats), prefill.stats["decode"]
    got = step(m2)
    assert prefill.w8_stats == n0 and prefill.stats["decode"] - s0 == 2 and torch.equal(got, want)
    assert all(prefill.w8_weights(lay) is None for lay in m2.model.layers)
    prefill.disable_fused_prefill(m2)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_generate_on_e4m3_weights(ops, dt):
    """Greedy generate, 6 new tokens, snapped weights: ids equal the fp32 model's and the stock run's at every step where the
    fp32 top-2 margin exceeds 0.05 (past an ambiguous step continuations may differ); at least 3 steps compared; every decode
    step of every layer ran on e4m3 weights."""
    from u2tokenizer_amd import prefill
    nl, new = 2, 6
    m32, mg = _snapped_pair(lambda: _small("qwen3", nl), dt)
    # (prompt seed 25: chosen on the fp32 model alone, whose top-2 margins at the six steps are 0.18 .. 0.51 there)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (1, 48, 512), 25)
    g32 = m32.generate(inputs_embeds=x, max_new_tokens=new, do_sample=False, output_scores=True, return_dict_in_generate=True)
    g_stock = mg.generate(inputs_embeds=x.to(dt).to(D), max_new_tokens=new, do_sample=False).cpu()
    prefill.enable_fused_prefill(mg, fp8_decode=True)
    n0 = prefill.w8_stats["decode"]
    g_w8 = mg.generate(inputs_embeds=x.to(dt).to(D), max_new_tokens=new, do_sample=False).cpu()
    prefill.disable_fused_prefill(mg)
    assert g_w8.shape == g_stock.shape == g32.sequences.shape
    assert g_w8.shape[1] == new and prefill.w8_stats["decode"] - n0 == nl * (g_w8.shape[1] - 1)
    compared = 0
    for t in range(new):
        top2 = g32.scores[t][0].topk(2).values
        if (top2[0] - top2[1]).item() <= 0.05:
            break
        assert g_w8[0, t] == g32.sequences[0, t] == g_stock[0, t], (t, g_w8, g_stock, g32.sequences)
        compared += 1
    assert compared >= 3, compared
