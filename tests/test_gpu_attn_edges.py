"""GPU: the inference attention kernels (tok_attn_kernel<64|96|128, EX, BAND> through ops.attention_gqa, its split_keys form,
attention_gqa_range and attention_gqa_band; decode_attn_kernel + decode_attn_merge_kernel through ops.decode_attention) on the edge
sweeps and the hard softmax data of tests/attn_edge_cases.py, element by element against the float64 bound of `model` there
(tests/test_attn_edges_host.py shows that the kernels' rounding model keeps it and that one-key mask mutants break it more than
10-fold), on the bf16 and the f16 build.  The float64 reference is computed on the device.  Every call runs twice with equal bits
and leaves its K / V buffers as they were; no element is left out, and a row that sees no key must be exactly zero (its bound is 0).

Worst error / bound measured on the MI355X: DESIGN.md, "Inference attention: edge sweeps"."""
import pytest
import torch

import attn_edge_cases as E

pytestmark = pytest.mark.gpu
D = "cuda"
ELEMS = [pytest.param(name, id=name) for name in E.ELEM]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=D)


def _call(ops, c, o):
    """-> (fn() -> (nb, Sq, Hq d), the buffers the call reads K / V from)"""
    q, Kb, Vb = o["q"].to(D), o["K"].to(D), o["V"].to(D)
    st, ln, scale = _i32(c.kv_start), _i32(c.kv_len), o["scale"]
    if c.layout == "col":     # (nb, Skv, Hkv d) views: columns of one packed q | k | v buffer where Sq = Skv, else rows [:Skv] of a longer one
        cap = c.Skv + c.spare
        k3, v3 = (t.transpose(1, 2).reshape(c.nb, cap, c.Hkv * c.d) for t in (Kb, Vb))
        if c.Sq == c.Skv and not c.spare:
            buf = torch.cat([q, k3, v3], -1)
            q, k, v = buf[..., :c.Hq * c.d], buf[..., c.Hq * c.d:(c.Hq + c.Hkv) * c.d], buf[..., (c.Hq + c.Hkv) * c.d:]
            bufs = (buf,)
        else:
            k3, v3 = k3.contiguous(), v3.contiguous()
            k, v, bufs = k3[:, :c.Skv], v3[:, :c.Skv], (k3, v3)
    else:                     # (nb, Hkv, Skv, d) views of a cache's buffers
        k, v, bufs = Kb[:, :, :c.Skv], Vb[:, :, :c.Skv], (Kb, Vb)
    if c.entry == "decode":
        assert c.Sq == 1 and c.window is None and ln is None
        return (lambda: ops.decode_attention(q[:, 0], k, v, c.Hq, c.Hkv, scale, kv_start=st)[:, None]), bufs
    if c.entry == "gqa":
        assert st is None and ln is None and c.window is None
        return (lambda: ops.attention_gqa(q, k, v, c.Hq, c.Hkv, scale, causal=c.causal)), bufs
    if c.entry == "split":
        assert st is None and ln is None and not c.causal
        return (lambda: ops.attention_gqa(q, k, v, c.Hq, c.Hkv, scale, causal=False, split_keys=True)), bufs
    if c.entry == "range":
        assert c.window is None and c.layout == "col"
        return (lambda: ops.attention_gqa_range(q, k, v, c.Hq, c.Hkv, scale, kv_start=st, kv_len=ln, causal=c.causal)), bufs
    assert c.entry == "band" and (c.window or c.layout == "cache")     # (else the call would be attention_gqa_range's kernel)
    return (lambda: ops.attention_gqa_band(q, k, v, c.Hq, c.Hkv, scale, window=c.window, kv_start=st, kv_len=ln, causal=c.causal)), bufs


def _sweep(ops, elem, cases, label):
    """every case: twice with equal bits, buffers untouched, every element inside the bound -> prints the worst error / bound"""
    dt, U, tiny = E.ELEM[elem]
    assert cases
    worst, worst_id, bad = 0.0, None, []
    for c in cases:
        o = E.operands(c, elem)
        fn, bufs = _call(ops, c, o)
        before = [b.clone() for b in bufs]
        got, again = fn(), fn()
        assert got.dtype == dt and got.shape == (c.nb, c.Sq, c.Hq * c.d)
        assert torch.equal(got, again), E.case_id(c)
        assert all(torch.equal(a, b) for a, b in zip(before, bufs)), E.case_id(c)
        q, k, v = E.split_heads(c, o, D)
        m = E.model(q, k, v, o["scale"], E.case_visible(c, D), U, tiny)
        got = got.double()
        assert torch.isfinite(got).all(), E.case_id(c)
        r = E.ratio((got - E.rows(m["out"])).abs(), E.rows(m["bound"]))
        if r > worst:
            worst, worst_id = r, E.case_id(c)
        if not r <= 1.0:
            bad.append((E.case_id(c), r))
    print(f"kernel error / bound, {label} {elem}: {worst:.3f} over {len(cases)} cases ({worst_id})")
    assert not bad, f"{len(bad)} of {len(cases)} cases outside the bound: {bad[:8]}"


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("d", E.DS)
def test_a_every_window_from_1_to_151(ops, elem, d):
    _sweep(ops, elem, [c for c in E.cases("A") if c.d == d], f"A window (attention_gqa_band, d = {d})")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("c_off", (1, 31, 32, 63, 64, 65, 100))
def test_b_continued_prefill_on_a_cache_view(ops, elem, c_off):
    _sweep(ops, elem, [c for c in E.cases("B") if c.Skv - c.Sq == c_off], f"B continued prefill (attention_gqa_band, c_off = {c_off})")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("entry,Sq", [("range", 150), ("band", 150), ("range", 6), ("band", 6)])
def test_c_first_key_sweeps_through_the_batch(ops, elem, entry, Sq):
    cases = [c for c in E.cases("C") if c.entry == entry and c.Sq == Sq]
    empty = ~E.case_visible(cases[0]).any(-1)
    assert empty[150].all() and not empty[:145].all(-1).any()      # the last sequence sees nothing: exact zeros (a bound of 0)
    _sweep(ops, elem, cases, f"C ranges (attention_gqa_{entry}, Sq = {Sq})")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("lo,hi", [(1, 100), (101, 200), (201, 300), (1023, 1792)])
def test_d_batched_decode_at_every_length(ops, elem, lo, hi):
    _sweep(ops, elem, [c for c in E.cases("D") if lo <= c.Skv <= hi], f"D decode_attention (T = {lo} .. {hi})")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("lo,hi", [(1, 200), (1023, 1792)])
def test_e_split_form_at_every_length(ops, elem, lo, hi):
    _sweep(ops, elem, [c for c in E.cases("E") if lo <= c.Skv <= hi], f"E attention_gqa split_keys (T = {lo} .. {hi})")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("entry", ("gqa", "split", "range", "band", "decode"))
@pytest.mark.parametrize("data", ("rise", "first", "steps", "equal", "edge"))
def test_f_hard_softmax_data(ops, elem, entry, data):
    _sweep(ops, elem, [c for c in E.cases("F") if c.entry == entry and c.data == data], f"F {data} ({entry})")
