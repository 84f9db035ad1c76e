"""GPU: the continued prefill on an FP8 (e4m3) KV cache -- the rows form of the attention over codes (u2tok_attention_kv8_rows)
element by element against the float64 bound of tests/kv8_cases.py on the table of tests/kv8_rows_cases.py, its repeatability, its
equality with the decode entry at one new position, its refusals, and the route (`enable_fused_prefill(model, kv8_continued=True)`)
against the stock layers on the same kind of cache -- on the bf16 and the f16 build."""
import functools

import pytest
import torch

import attn_edge_cases as A
import kv8_cases as K8
import kv8_rows_cases as R
import test_gpu_w8 as W
from test_gpu_kv8 import MODELS
from u2tokenizer_amd import synth

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


# ------------------------------------------------------------------------------------------------------------- the kernel
def _sweep(ops, elem, cases, label):
    dt = A.ELEM[elem][0]
    worst, worst_id, bad = 0.0, None, []
    for n, c in enumerate(cases):
        o = K8.operands(c, elem)
        q, kc, vc, ks, vs, st = R.gpu_operands(c, o, D)
        if n % 2:   # the q columns of packed q|k|v rows: a row stride wider than the rows
            wide = torch.full((c.nb, c.Sq, (c.Hq + 2 * c.Hkv) * c.d), 3.0, dtype=dt, device=D)
            wide[..., :c.Hq * c.d] = q
            q = wide[..., :c.Hq * c.d]
        before = [t.clone() for t in (kc, vc, ks, vs)]
        got = ops.attention_kv8_rows(q, kc, vc, ks, vs, c.Skv, c.Hq, o["scale"], window=c.window, kv_start=st)
        again = ops.attention_kv8_rows(q, kc, vc, ks, vs, c.Skv, c.Hq, o["scale"], window=c.window, kv_start=st)
        assert got.dtype == dt and got.shape == (c.nb, c.Sq, c.Hq * c.d) and got.is_contiguous()
        assert torch.equal(got, again), A.case_id(c)                       # the same call twice: the same bits
        assert all(torch.equal(a, b) for a, b in zip(before, (kc, vc, ks, vs))), A.case_id(c)
        assert not bool(got[-1].any()), A.case_id(c)                       # the last sequence sees no key: exact zeros
        m = K8.model(*K8.split(c, o, D), o["scale"], A.case_visible(c, D), elem)
        got = got.double()
        assert torch.isfinite(got).all(), A.case_id(c)
        r = A.ratio((got - A.rows(m["out"])).abs(), A.rows(m["bound"]))
        if r > worst:
            worst, worst_id = r, A.case_id(c)
        if not r <= 1.0:
            bad.append((A.case_id(c), r))
    print(f"kernel error / bound, {label} {elem}: {worst:.3f} over {len(cases)} cases ({worst_id})")
    assert not bad, f"{len(bad)} of {len(cases)} cases outside the bound: {bad[:8]}"


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("data", ("normal", "poison"))
@pytest.mark.parametrize("part", range(3))
def test_rows_over_codes_keep_the_bound(ops, elem, data, part):
    cases = R.sweep(data)[part::3]
    assert len(cases) >= 48
    _sweep(ops, elem, cases, f"attention_kv8_rows {data} (part {part})")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("which", ("edge", "long"))
def test_rows_over_codes_keep_the_bound_on_edges_and_splits(ops, elem, which):
    cases = R.edge_cases() if which == "edge" else R.long_cases()
    assert len(cases) == (24 if which == "edge" else 8)
    _sweep(ops, elem, cases, f"attention_kv8_rows {which}")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("d", K8.DS)
def test_one_new_position_has_the_decode_entry_bits(ops, elem, d):
    for n, T in enumerate((1, 64, 65, 300, 1025)):
        g = A.GS[(n + d // 32) % len(A.GS)]
        start = tuple(min(max(s, 0), T) for s in (0, 1, 33, T // 2, T - 1, T))
        c = A.case("K8", "decode", 6, 1, T, 2 * g, 2, d, kv_start=start, spare=T % 2 * 3, data="normal", tile=K8.BK)
        o = K8.operands(c, elem)
        q, kc, vc, ks, vs, st = R.gpu_operands(c, o, D)
        for kv_start in (None, st):
            want = ops.decode_attention_kv8(q[:, 0], kc, vc, ks, vs, T, c.Hq, o["scale"], kv_start=kv_start)
            got = ops.attention_kv8_rows(q, kc, vc, ks, vs, T, c.Hq, o["scale"], kv_start=kv_start)
            assert torch.equal(got[:, 0], want), (T, g, d, kv_start is None)
        if T > 2:   # ... and from a first position > 0
            want = ops.decode_attention_kv8(q[:, 0], kc, vc, ks, vs, T - 2, c.Hq, o["scale"], k_first=2)
            assert torch.equal(ops.attention_kv8_rows(q, kc, vc, ks, vs, T - 2, c.Hq, o["scale"], k_first=2)[:, 0], want), (T, g, d)


@pytest.mark.parametrize("elem", ELEMS)
def test_refusals_precede_every_launch(ops, elem):
    """(every call below is refused: nothing is launched, the output, the workspace and the buffers keep their sentinels)"""
    dt = A.ELEM[elem][0]
    ERR_ARG, ERR_WS = -1, -3
    Bn, Sq, Hkv, Hq, d, cap, T = 2, 7, 2, 6, 64, 1100, 1025
    with ops.on_device(torch.empty(1, device=D), dt) as (h, stream):
        q = torch.zeros(Bn, Sq, Hq * d, dtype=dt, device=D)
        kc, vc = (torch.full((Bn, Hkv, cap, d), 0x11, dtype=torch.uint8, device=D) for _ in range(2))
        ks, vs = (torch.full((Bn, Hkv, cap), 3.0, device=D) for _ in range(2))
        out = torch.full((Bn, Sq, Hq * d), 5.0, dtype=dt, device=D)
        need = h.u2tok_attention_kv8_rows_workspace_bytes(Bn, Sq, Hq, Hkv, T, d)
        assert need == R.workspace_bytes(Bn, Sq, Hq, Hkv, T, d) > 16
        ws = torch.full((need,), 0x77, dtype=torch.uint8, device=D)
        a = [q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), vs.data_ptr(), out.data_ptr()]

        def attn(ptrs=a, Sq_=Sq, Hq_=Hq, T_=T, d_=d, kvst=cap * d, scst=cap, scale=0.125, window=0, w=ws.data_ptr(), wb=ws.numel()):
            return h.u2tok_attention_kv8_rows(*ptrs, Bn, Sq_, Hq_, Hkv, T_, d_, Hq_ * d_, kvst, scst, Hq_ * d_, scale, window, None, w, wb, stream)

        for i in range(6):
            assert attn(ptrs=a[:i] + [None] + a[i + 1:]) == ERR_ARG, i
        assert attn(ptrs=[a[0] + 8] + a[1:]) == ERR_ARG and attn(ptrs=a[:1] + [a[1] + 8] + a[2:]) == ERR_ARG
        assert attn(ptrs=a[:3] + [a[3] + 2] + a[4:]) == ERR_ARG
        assert attn(Sq_=0) == ERR_ARG and attn(Sq_=T + 1) == ERR_ARG and attn(window=-1) == ERR_ARG
        assert attn(d_=80) == ERR_ARG and attn(Hq_=3) == ERR_ARG and attn(Hq_=34 * Hkv) == ERR_ARG and attn(T_=0) == ERR_ARG
        assert attn(kvst=T * d - 16) == ERR_ARG and attn(kvst=cap * d + 8) == ERR_ARG and attn(scst=T - 1) == ERR_ARG
        assert attn(scale=0.0) == ERR_ARG
        used = R.splits(Bn, Sq, Hq, Hkv, T)[0] * Bn * Sq * Hq * (4 * d + 8)     # (no split beyond the last tile: at most what was asked)
        assert 16 < used <= need and attn(wb=used - 1) == ERR_WS and attn(w=ws.data_ptr() + 8) == ERR_ARG
        torch.cuda.synchronize()
        assert bool((out == 5.0).all()) and bool((ws == 0x77).all())
        assert bool((kc == 0x11).all()) and bool((vc == 0x11).all()) and bool((ks == 3.0).all()) and bool((vs == 3.0).all())
    with pytest.raises(RuntimeError):
        ops.attention_kv8_rows(q[:, :, :-8], kc, vc, ks, vs, T, Hq, 0.125)               # not heads * d wide
    with pytest.raises(RuntimeError):
        ops.attention_kv8_rows(q, kc, vc, ks, vs, Sq - 1, Hq, 0.125)                     # fewer positions than new rows


# ----------------------------------------------------------------------------------------------------------- the model level
NL, S0, CALLS, STEPS = 2, 40, (9, 21), 2    # the second continuation crosses the 64-key tile boundary at position 64
TOTAL = S0 + sum(CALLS) + STEPS
PADS = (0, 7, 3)
MODEL_CASES = [(64, 1), (128, 3), (96, 1)]   # hd 128: left-padded under padded=True; hd 96: Phi-3 with a window of 42


def _calls(m, xs, cache, masks):
    """the prefill, the two continuations and the decode steps on `cache` -> the logits of the last position of every call"""
    return [m(inputs_embeds=x, past_key_values=cache, use_cache=True, **mk).logits[:, -1] for x, mk in zip(xs, masks)]


def _inputs(hd, Bn):
    E = MODELS[hd][1]
    x = 0.5 * synth.synth_tensor("inputs_embeds", (Bn, TOTAL, E), 9)
    return list(x.split((S0,) + CALLS + (1,) * STEPS, 1))


def _masks(Bn, device):
    n = 1 + len(CALLS) + STEPS
    if Bn != 3:
        return [{}] * n
    mask = torch.ones(Bn, TOTAL, dtype=torch.int64)
    for b, p in enumerate(PADS):
        mask[b, :p] = 0
    ends = torch.tensor((S0,) + CALLS + (1,) * STEPS).cumsum(0).tolist()
    return [{"attention_mask": mask[:, :e].to(device)} for e in ends]


@functools.lru_cache(maxsize=None)
def _reference(hd, Bn):
    """(c): the fp32 model on the CPU on a cache of `Kv8Layer`s"""
    from u2tokenizer_amd import prefill
    m32 = MODELS[hd][0]()
    xs = _inputs(hd, Bn)
    return dict(state=m32.state_dict(), xs=xs, logits=_calls(m32, xs, prefill.kv8_cache(NL), _masks(Bn, "cpu")))


@pytest.mark.parametrize("hd,Bn", MODEL_CASES)
@pytest.mark.parametrize("dt", W.DTYPES, ids=W.IDS)
def test_continued_prefill_on_a_kv8_cache(ops, dt, hd, Bn, monkeypatch):
    """2 layers; a 40-position prefill, a 9- and a 21-position continuation, 2 decode steps: (a) the fused route with kv8_continued,
    (b) the stock layers on a cache of `Kv8Layer`s, (c) the fp32 model on the CPU on such a cache.  dist(a, c) <= 1.5 dist(b, c) +
    EPS on every call's logits; every continuation and decode step counted per layer; the cache holds `Kv8Layer`s of length 72; layer
    0's codes and scales are, bit for bit, the reference quantiser's of the rows a 16-bit twin run's cache holds.  With the switch
    off (kv8=True, continued=True) the continuations take the stock layers on the dequantised cache, as they do when the route's
    cap refuses them: no counter moves and the two runs' logits are equal bit for bit."""
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd import prefill
    r = _reference(hd, Bn)
    mg = MODELS[hd][0]()
    mg.load_state_dict(r["state"])
    mg = mg.to(dt).to(D)
    xs, masks = [x.to(dt).to(D) for x in r["xs"]], _masks(Bn, D)
    stock = _calls(mg, xs, prefill.kv8_cache(NL), masks)                                        # (b)
    sw = dict(padded=Bn == 3)
    prefill.enable_fused_prefill(mg, continued=True, **sw)
    twin = DynamicCache()
    _calls(mg, xs, twin, masks)
    prefill.enable_fused_prefill(mg, kv8_continued=True, **sw)
    x0, k0, e0 = dict(prefill.kv8_extend_stats), dict(prefill.kv8_stats), dict(prefill.extend_stats)
    cache = DynamicCache()
    fused = _calls(mg, xs, cache, masks)                                                        # (a)
    which, other = ("padded_", "") if Bn == 3 else ("", "padded_")
    assert prefill.kv8_extend_stats[which + "extend"] - x0[which + "extend"] == NL * len(CALLS)
    assert prefill.kv8_extend_stats[other + "extend"] == x0[other + "extend"]
    assert prefill.extend_stats[which + "extend"] - e0[which + "extend"] == NL * len(CALLS)
    assert prefill.kv8_stats[which + "decode"] - k0[which + "decode"] == NL * STEPS
    assert all(type(l) is prefill.Kv8Layer and l.get_seq_length() == TOTAL for l in cache.layers) and TOTAL == 72
    assert all(type(l).__name__ == "AppendLayer" for l in twin.layers)
    for t in range(len(xs)):
        es, ef = W._err(stock[t].float().cpu(), r["logits"][t]), W._err(fused[t].float().cpu(), r["logits"][t])
        print(f"call {t}: fused {ef:.3e} stock {es:.3e}")
        assert torch.isfinite(fused[t]).all() and ef <= 1.5 * es + W.EPS[dt], (t, ef, es)
    kc, vc, ks, vs = (t.cpu() for t in cache.layers[0].codes())
    for x16, codes, scales in ((twin.layers[0].keys, kc, ks), (twin.layers[0].values, vc, vs)):
        want_c, want_s = ops.quantize_kv_fp8(x16[:, :, :TOTAL].cpu())
        assert torch.equal(codes, want_c.view(torch.uint8)) and torch.equal(scales.view(torch.int32), want_s.view(torch.int32))
    # the switch off, and the switch on with every continuation above the cap: the stock layers on the dequantised cache
    x1, e1 = dict(prefill.kv8_extend_stats), dict(prefill.extend_stats)
    prefill.enable_fused_prefill(mg, kv8=True, continued=True, **sw)
    off = _calls(mg, xs, DynamicCache(), masks)
    prefill.enable_fused_prefill(mg, kv8_continued=True, **sw)
    monkeypatch.setattr(prefill, "KV8_EXTEND_MAX_ROWS", 1)
    capped = _calls(mg, xs, DynamicCache(), masks)
    prefill.disable_fused_prefill(mg)
    assert prefill.kv8_extend_stats == x1 and prefill.extend_stats == e1
    assert all(torch.equal(a, b) for a, b in zip(off, capped))
