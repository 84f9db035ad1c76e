"""GPU: the FP8 (e4m3) KV cache -- the quantising append (u2tok_kv_quantize_rows) bit for bit against ops.quantize_kv_fp8, the
decode attention over codes (u2tok_decode_attention_kv8) element by element against the float64 bound of tests/kv8_cases.py, its
repeatability and refusals, and the fused decode step on a cache of `Kv8Layer`s (`enable_fused_prefill(model, kv8=True)`) against
the stock layers on the same kind of cache -- on the bf16 and the f16 build."""
import ctypes as C

import pytest
import torch

import attn_edge_cases as A
import kv8_cases as K8

pytestmark = pytest.mark.gpu
D = "cuda"
ELEMS = [pytest.param(name, id=name) for name in A.ELEM]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


# ------------------------------------------------------------------------------------------------------- the quantising append
def _tie_rows(n, d, dt, gen):
    """rows whose largest element is 448 (scale exactly 1) and whose other elements sit on e4m3 midpoints -- halfway between two
    neighbouring codes, exact in bf16 and fp16 -- or on codes, in both signs: round to nearest EVEN decides every one of them"""
    grid = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    grid = grid[torch.isfinite(grid) & (grid >= 0)].sort().values
    mids = (grid[:-1] + grid[1:]) / 2
    pool = torch.cat([mids, grid, torch.tensor([2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -11])])
    x = pool[torch.randint(0, pool.numel(), (n, d), generator=gen)]
    x = x * torch.where(torch.rand(n, d, generator=gen) < 0.5, -1.0, 1.0)
    x[:, 0] = 448.0
    assert torch.equal(x.to(dt).float(), x)
    return x.to(dt)


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("d", K8.DS)
def test_quantise_kernel_is_bit_equal_to_the_reference(ops, elem, d):
    dt = A.ELEM[elem][0]
    gen = torch.Generator().manual_seed(d)
    for Bn in (1, 3):
        for Hkv in (1, 2):
            for n in (1, 5, 33):
                cap, s_off = n + 11, 6
                k = torch.randn(Bn, Hkv, n, d, generator=gen) * torch.exp2(torch.randint(-6, 7, (Bn, Hkv, n, 1), generator=gen).float())
                v = torch.randn(Bn, Hkv, n, d, generator=gen)
                k, v = k.to(dt), v.to(dt)
                v[0, 0, 0] = 0                                            # an all-zero row: scale 1, zero codes
                if n >= 5:
                    k[0, 0, :4] = _tie_rows(4, d, dt, gen)
                    v[-1, -1, -4:] = _tie_rows(4, d, dt, gen)
                # the model's layout: (B, n, Hkv, d) rows seen as (B, Hkv, n, d) -- strides that are no dense tensor's
                kg = k.transpose(1, 2).contiguous().to(D).transpose(1, 2)
                vg = v.to(D)
                bufs = [torch.full((Bn, Hkv, cap, d), 0xA5, dtype=torch.uint8, device=D), torch.full((Bn, Hkv, cap, d), 0x5A, dtype=torch.uint8, device=D),
                        torch.full((Bn, Hkv, cap), -7.0, device=D), torch.full((Bn, Hkv, cap), -9.0, device=D)]
                before = [b.clone() for b in bufs]
                ops.kv_quantize_rows(kg, vg, *bufs, s_off)
                for x, codes, scales in ((k, bufs[0], bufs[2]), (v, bufs[1], bufs[3])):
                    want_c, want_s = ops.quantize_kv_fp8(x)
                    assert torch.equal(codes[:, :, s_off:s_off + n].cpu(), want_c.view(torch.uint8)), (Bn, Hkv, n)
                    assert torch.equal(scales[:, :, s_off:s_off + n].cpu().view(torch.int32), want_s.view(torch.int32)), (Bn, Hkv, n)
                for b, b0 in zip(bufs, before):                             # the sentinels around the written range
                    assert torch.equal(b[:, :, :s_off], b0[:, :, :s_off]) and torch.equal(b[:, :, s_off + n:], b0[:, :, s_off + n:])


# ------------------------------------------------------------------------------------------------ the attention over codes
def _gpu(c, o):
    kc, vc = (o[n].view(torch.uint8).to(D).contiguous() for n in ("K8", "V8"))
    return o["q"].to(D)[:, 0], kc, vc, o["ks"].to(D).contiguous(), o["vs"].to(D).contiguous(), torch.tensor(c.kv_start, dtype=torch.int32, device=D)


def _sweep(ops, elem, cases, label):
    dt = A.ELEM[elem][0]
    worst, worst_id, bad = 0.0, None, []
    for c in cases:
        o = K8.operands(c, elem)
        q, kc, vc, ks, vs, st = _gpu(c, o)
        before = [t.clone() for t in (kc, vc, ks, vs)]
        got = ops.decode_attention_kv8(q, kc, vc, ks, vs, c.Skv, c.Hq, o["scale"], kv_start=st)
        again = ops.decode_attention_kv8(q, kc, vc, ks, vs, c.Skv, c.Hq, o["scale"], kv_start=st)
        assert got.dtype == dt and got.shape == (c.nb, c.Hq * c.d)
        assert torch.equal(got, again), A.case_id(c)                       # the same call twice: the same bits
        assert all(torch.equal(a, b) for a, b in zip(before, (kc, vc, ks, vs))), A.case_id(c)
        m = K8.model(*K8.split(c, o, D), o["scale"], A.case_visible(c, D), elem)
        got = got.double()[:, None]
        assert torch.isfinite(got).all(), A.case_id(c)
        r = A.ratio((got - A.rows(m["out"])).abs(), A.rows(m["bound"]))
        if r > worst:
            worst, worst_id = r, A.case_id(c)
        if not r <= 1.0:
            bad.append((A.case_id(c), r))
    print(f"kernel error / bound, {label} {elem}: {worst:.3f} over {len(cases)} cases ({worst_id})")
    assert not bad, f"{len(bad)} of {len(cases)} cases outside the bound: {bad[:8]}"


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("data", ("normal", "poison", "edge"))
@pytest.mark.parametrize("lo,hi", [(1, 65), (66, 130), (131, 300), (1023, 1792)])
def test_attention_over_codes_keeps_the_bound(ops, elem, data, lo, hi):
    cases = [K8.attn_case(T, data) for T in K8.LENGTHS if lo <= T <= hi]
    assert cases
    _sweep(ops, elem, cases, f"decode_attention_kv8 {data} (T = {lo} .. {hi})")


@pytest.mark.parametrize("elem", ELEMS)
def test_refusals_precede_every_launch(ops, elem):
    """(every call below is refused: nothing is launched, the output and the buffers keep their sentinels)"""
    from u2tokenizer_amd import _lib
    dt = A.ELEM[elem][0]
    ERR_ARG, ERR_WS = -1, -3
    Bn, Hkv, Hq, d, cap, T = 2, 2, 4, 64, 600, 512
    with ops.on_device(torch.empty(1, device=D), dt) as (h, stream):
        q = torch.zeros(Bn, Hq * d, dtype=dt, device=D)
        k = torch.zeros(Bn, Hkv, 4, d, dtype=dt, device=D)
        kc, vc = (torch.full((Bn, Hkv, cap, d), 0x11, dtype=torch.uint8, device=D) for _ in range(2))
        ks, vs = (torch.full((Bn, Hkv, cap), 3.0, device=D) for _ in range(2))
        out = torch.full((Bn, Hq * d), 5.0, dtype=dt, device=D)
        ws = torch.empty(max(16, h.u2tok_decode_attention_kv8_workspace_bytes(Bn, Hq, Hkv, T, d)), dtype=torch.uint8, device=D)
        p = [t.data_ptr() for t in (k, k, kc, vc, ks, vs)]
        st = k.stride()

        def quant(ptrs=p, d_=d, n=4, cap_=cap, s_off=0, strides=st):
            return h.u2tok_kv_quantize_rows(ptrs[0], ptrs[1], Bn, Hkv, n, d_, *strides[:3], *strides[:3], ptrs[2], ptrs[3], ptrs[4], ptrs[5],
                                            cap_, s_off, stream)

        for i in range(6):
            assert quant(ptrs=p[:i] + [None] + p[i + 1:]) == ERR_ARG, i
        assert quant(ptrs=[p[0] + 8] + p[1:]) == ERR_ARG and quant(ptrs=p[:2] + [p[2] + 8] + p[3:]) == ERR_ARG     # misaligned rows / codes
        assert quant(ptrs=p[:4] + [p[4] + 2] + p[5:]) == ERR_ARG                                                   # ... scales
        assert quant(d_=80) == ERR_ARG and quant(d_=32) == ERR_ARG
        assert quant(s_off=cap - 3) == ERR_ARG and quant(n=0) == ERR_ARG and quant(s_off=-1) == ERR_ARG
        assert quant(strides=(st[0], st[1], st[2] + 4)) == ERR_ARG

        a = [q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), vs.data_ptr(), out.data_ptr()]

        def attn(ptrs=a, Hq_=Hq, T_=T, d_=d, kvst=cap * d, scst=cap, scale=0.125, w=ws.data_ptr(), wb=ws.numel()):
            return h.u2tok_decode_attention_kv8(*ptrs, Bn, Hq_, Hkv, T_, d_, Hq_ * d_, kvst, scst, Hq_ * d_, scale, None, w, wb, stream)

        for i in range(6):
            assert attn(ptrs=a[:i] + [None] + a[i + 1:]) == ERR_ARG, i
        assert attn(ptrs=[a[0] + 8] + a[1:]) == ERR_ARG and attn(ptrs=a[:1] + [a[1] + 8] + a[2:]) == ERR_ARG
        assert attn(ptrs=a[:3] + [a[3] + 2] + a[4:]) == ERR_ARG
        assert attn(d_=80) == ERR_ARG and attn(Hq_=3) == ERR_ARG and attn(Hq_=34 * Hkv) == ERR_ARG and attn(T_=0) == ERR_ARG
        assert attn(kvst=T * d - 16) == ERR_ARG and attn(kvst=cap * d + 8) == ERR_ARG and attn(scst=T - 1) == ERR_ARG
        assert attn(scale=0.0) == ERR_ARG
        assert ws.numel() > 16 and attn(wb=ws.numel() - 1) == ERR_WS and attn(w=ws.data_ptr() + 8) == ERR_ARG
        torch.cuda.synchronize()
        assert bool((out == 5.0).all()) and bool((kc == 0x11).all()) and bool((vc == 0x11).all()) and bool((ks == 3.0).all())
    assert C.sizeof(_lib.DecodeConfig) == 40


# ----------------------------------------------------------------------------------------------------------- the model level
import functools  # noqa: E402

import test_gpu_w8 as W  # noqa: E402
from u2tokenizer_amd import synth  # noqa: E402

S0, STEPS, NL = 40, 6, 2
PADS = (0, 7, 3)


def _d128(layers):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    m = Qwen3ForCausalLM(Qwen3Config(vocab_size=1024, hidden_size=512, intermediate_size=1536, num_hidden_layers=layers, num_attention_heads=4,
                                     num_key_value_heads=2, head_dim=128, max_position_embeddings=512, tie_word_embeddings=False,
                                     pad_token_id=0, bos_token_id=1, eos_token_id=2))
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m.eval()


MODELS = {64: (lambda: W._small("qwen3", NL), 512), 96: (lambda: W._phi3(NL, 42), 768), 128: (lambda: _d128(NL), 512)}
# (head dim, sequences, weight form).  3 sequences: left-padded under padded=True; 20: wide_decode=True.  The Phi-3 layers carry a
# window of 42: the 40-position prefill is the plain causal one, the last steps (T = 43 .. 46) attend from k_first > 0.  A window
# with padding is the stock route's by route()'s standing rule: no such case.
MODEL_CASES = [(64, 1, "elem"), (64, 3, "elem"), (64, 20, "elem"), (96, 1, "elem"), (96, 20, "elem"), (128, 1, "elem"), (128, 3, "elem"),
               (128, 20, "elem"), (128, 1, "fp4")]


def _steps(m, x, xs, cache, masks):
    """prefill + teacher-forced steps on `cache` -> the logits of the last position of every call"""
    out = [m(inputs_embeds=x, past_key_values=cache, use_cache=True, **masks[0]).logits[:, -1]]
    for t in range(xs.shape[1]):
        out.append(m(inputs_embeds=xs[:, t:t + 1], past_key_values=cache, use_cache=True, **masks[t + 1]).logits[:, -1])
    return out


def _masks(Bn, device):
    if Bn != 3:
        return [{}] * (STEPS + 1)
    mask = torch.ones(Bn, S0 + STEPS, dtype=torch.int64)
    for b, p in enumerate(PADS):
        mask[b, :p] = 0
    return [{"attention_mask": mask[:, :S0 + t].to(device)} for t in range(STEPS + 1)]


@functools.lru_cache(maxsize=None)
def _reference(hd, Bn, form):
    """(c): the fp32 model on the CPU on a cache of `Kv8Layer`s (fp4: weights snapped onto values the e2m1 form keeps exactly)"""
    from u2tokenizer_amd import ops as _ops
    from u2tokenizer_amd import prefill
    make, E = MODELS[hd]
    m32 = make()
    if form == "fp4":
        _ops.snap_fp4_(m32.model.layers)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (Bn, S0, E), 7)
    xs = 0.5 * synth.synth_tensor("inputs_embeds", (Bn, STEPS, E), 8)
    logits = _steps(m32, x, xs, prefill.kv8_cache(NL), _masks(Bn, "cpu"))
    return dict(state=m32.state_dict(), x=x, xs=xs, logits=logits)


@pytest.mark.parametrize("hd,Bn,form", MODEL_CASES)
@pytest.mark.parametrize("dt", W.DTYPES, ids=W.IDS)
def test_fused_decode_on_a_kv8_cache(ops, dt, hd, Bn, form):
    """2 layers, a 40-position prefill and 6 teacher-forced steps: (a) the fused route with kv8, (b) the stock layers on a cache of
    `Kv8Layer`s, (c) the fp32 model on the CPU on such a cache.  dist(a, c) <= 1.5 dist(b, c) on every call's logits; every layer
    step counted; the cache holds `Kv8Layer`s; and its codes and scales are, bit for bit, the reference quantiser's of the rows the
    16-bit append-in-place cache of a twin run holds -- layer 0 at every position, deeper layers at the prefill's."""
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd import prefill
    r = _reference(hd, Bn, form)
    mg = MODELS[hd][0]()
    mg.load_state_dict(r["state"])
    mg = mg.to(dt).to(D)
    xd, xsd, masks = r["x"].to(dt).to(D), r["xs"].to(dt).to(D), _masks(Bn, D)
    stock = _steps(mg, xd, xsd, prefill.kv8_cache(NL), masks)                                   # (b)
    sw = dict(padded=Bn == 3, wide_decode=Bn > 16, fp4_decode=form == "fp4")
    prefill.enable_fused_prefill(mg, **sw)
    twin = DynamicCache()
    _steps(mg, xd, xsd, twin, masks)
    prefill.enable_fused_prefill(mg, kv8=True, **sw)
    n0, s0, w0 = dict(prefill.kv8_stats), dict(prefill.stats), dict(prefill.w4_stats)
    cache = DynamicCache()
    fused = _steps(mg, xd, xsd, cache, masks)                                                   # (a)
    prefill.disable_fused_prefill(mg)
    which, other = ("padded_decode", "decode") if Bn == 3 else ("decode", "padded_decode")
    assert prefill.kv8_stats[which] - n0[which] == NL * STEPS and prefill.kv8_stats[other] == n0[other]
    assert prefill.stats[which] - s0[which] == NL * STEPS
    assert prefill.w4_stats[which] - w0[which] == (NL * STEPS if form == "fp4" else 0)
    assert all(type(l) is prefill.Kv8Layer for l in cache.layers) and cache.get_seq_length() == S0 + STEPS
    assert all(type(l).__name__ == "AppendLayer" for l in twin.layers)
    for t in range(STEPS + 1):
        es, ef = W._err(stock[t].float().cpu(), r["logits"][t]), W._err(fused[t].float().cpu(), r["logits"][t])
        print(f"call {t}: fused {ef:.3e} stock {es:.3e}")
        assert torch.isfinite(fused[t]).all() and ef <= 1.5 * es + W.EPS[dt], (t, ef, es)
    for li in range(NL):
        T = S0 + STEPS if li == 0 else S0
        kc, vc, ks, vs = (t[:, :, :T].cpu() for t in cache.layers[li].codes())
        for x16, codes, scales in ((twin.layers[li].keys, kc, ks), (twin.layers[li].values, vc, vs)):
            want_c, want_s = ops.quantize_kv_fp8(x16[:, :, :T].cpu())
            assert torch.equal(codes, want_c.view(torch.uint8)), li
            assert torch.equal(scales.view(torch.int32), want_s.view(torch.int32)), li
