"""GPU: the split-row form of the sampling warper (u2tok_sample_warp_split; opt-in `config.u2_fused_sampling_split`): a row over several
workgroups, one launch per pass of the descent, integer partial histograms added with device-scope atomics.  The masses are integers,
so its test is an exact oracle: `out` BIT-EQUAL to u2tok_sample_warp on the same input, and the same kept count (record word 5).  The
float64 reference of tests/sampling_cases.py is not gated again here: the one-workgroup kernel is held to it
(tests/test_gpu_sampling.py), and bit equality carries it over.  No test waits on anything another workgroup sets; the number of
launches is the host's, from the parameters alone."""
import math

import pytest
import torch

import sampling_cases as SC
from test_gpu_sampling import _hard_rows, _lm

pytestmark = pytest.mark.gpu
D = "cuda"
NEG = -math.inf


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


def _warp(ops, split, x, prm, out=None, ws=None):
    """one call of either C entry on x (rows, V) fp32 (row-strided views allowed) -> (out, kept counts (rows,) from the records)"""
    T, k, p, mk = prm
    rows, V = x.shape
    with ops.on_device(x, torch.bfloat16) as (h, stream):
        name = "u2tok_sample_warp_split" if split else "u2tok_sample_warp"
        need = getattr(h, name + "_workspace_bytes")(rows, V)
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        assert ws.numel() >= need > 0
        if out is None:
            out = torch.empty((rows, V), dtype=torch.float32, device=x.device)
        st = getattr(h, name)(x.data_ptr(), x.stride(0) if rows > 1 else V, out.data_ptr(), out.stride(0) if rows > 1 else V, rows, V,
                              float(T), int(k), float(p), int(mk), ws.data_ptr(), ws.numel(), stream)
        assert st == 0, (name, st)
    rec = ws[:rows * 32].view(torch.int32).view(rows, 8)
    return out, rec[:, 5].clone()


def _same(ops, x, prm, what, **kw):
    want, kept_want = _warp(ops, False, x, prm)
    got, kept = _warp(ops, True, x, prm, **kw)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (what, int((got.view(torch.int32) != want.view(torch.int32)).sum()))
    assert torch.equal(kept, kept_want), (what, kept.tolist(), kept_want.tolist())
    return got


@pytest.mark.parametrize("V", [2, 255, 257, 4097, 151936])
def test_bit_equal_to_the_one_workgroup_kernel(ops, V):
    """rows in {1, 2, 4, 5} x the six parameter sets, random logits and logits with bf16 values (ties everywhere): `out` and the kept
    counts of u2tok_sample_warp.  V = 151 936: 16 workgroups per row; 4097: one; 2: a slice of two elements."""
    for rows in (1, 2, 4, 5):
        for bf16_values in (False, True):
            x = SC.logits(rows, V, seed=3 + bf16_values, bf16_values=bf16_values).to(D)
            for name, prm in SC.PARAMS.items():
                out = _same(ops, x, prm, (V, rows, name, bf16_values))
                assert (out > NEG).any(-1).all()


@pytest.mark.parametrize("V", [65, 1000, 20000])
def test_hard_rows(ops, V):
    """dominant token, uniform row, a 40-token tie group across the boundary, -inf rows, signed zeros at the k-th value, k >= V, min_keep
    past the nucleus, a vanishing top_p -- each alone and all rows that share a parameter set in one call"""
    for name, (r, prm) in _hard_rows(V).items():
        _same(ops, r[None].to(D), prm, (V, name))
        _same(ops, torch.stack([r, r.flip(0), r]).to(D), prm, (V, name, "x 3"))


def test_variants_of_the_call(ops):
    """a workspace full of 0xFF; in place; row-strided input and output with guard columns; a side stream; 20 back-to-back calls on one
    workspace with fresh inputs (a stale table or state would show)"""
    V, rows = 40000, 3
    prm = SC.PARAMS["T1.3_k50_p0.95_keep2"]
    x = SC.logits(rows, V, seed=9).to(D)
    with ops.on_device(x, torch.bfloat16) as (h, _):
        need = h.u2tok_sample_warp_split_workspace_bytes(rows, V)
        assert need > h.u2tok_sample_warp_workspace_bytes(rows, V) and h.u2tok_sample_warp_split_workspace_bytes(0, V) == 0
        assert h.u2tok_sample_warp_split_workspace_bytes(rows, 1) == 0
        assert h.u2tok_sample_warp_split_launches(V, 50, 0.95, 2) == 3 + 4 + 8 + 8
        assert h.u2tok_sample_warp_split_launches(V, 0, 0.9, 1) == 3 + 8 and h.u2tok_sample_warp_split_launches(V, 5, 1.0, 1) == 3 + 4
        assert h.u2tok_sample_warp_split_launches(V, V + 1, 1.0, 1) == 3
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=D)
    _same(ops, x, prm, "0xFF workspace", ws=ws)
    _same(ops, x, prm, "0xFF workspace, 4 bytes in", ws=torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=D)[4:])
    inplace = x.clone()
    got = _same(ops, inplace, prm, "in place", out=inplace)
    assert got.data_ptr() == inplace.data_ptr()
    wide = torch.full((rows, V + 24), 5.0, device=D)
    wide[:, 8:8 + V] = x
    obuf = torch.full((rows, V + 40), 7.0, device=D)
    _same(ops, wide[:, 8:8 + V], prm, "guard columns", out=obuf[:, 16:16 + V])
    assert (obuf[:, :16] == 7).all() and (obuf[:, 16 + V:] == 7).all() and (wide[:, :8] == 5).all() and (wide[:, 8 + V:] == 5).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _same(ops, x, prm, "side stream")
    torch.cuda.current_stream().wait_stream(side)
    names = list(SC.PARAMS)
    for i in range(20):
        xi = SC.logits(rows, V, seed=20 + i, bf16_values=i % 2 == 1).to(D)
        _same(ops, xi, SC.PARAMS[names[i % len(names)]], ("back to back", i), ws=ws)


def test_nan_and_inf_rows_end_and_leave_the_good_rows_alone(ops):
    V = 20000
    prm = SC.PARAMS["T0.7_p0.9"]
    good = SC.logits(5, V, seed=31)
    x = good.clone()
    x[1, 77] = float("nan")
    x[3, 5], x[3, 19000] = float("inf"), float("-inf")
    x[4] = NEG
    x = x.to(D)
    want, kept_want = _warp(ops, False, good.to(D), prm)
    got, kept = _warp(ops, True, x, prm)
    torch.cuda.synchronize()                                   # (the call ended)
    for r in (0, 2):
        assert torch.equal(got[r].view(torch.int32), want[r].view(torch.int32)) and kept[r] == kept_want[r], r
    assert got.shape == (5, V)


def test_generate_with_the_split_form_gives_the_ids_of_the_fused_warper(ops):
    """`generate` at batch 2, sampled (T 0.7, p 0.9), the same seed: `u2_fused_sampling_split` on top of `u2_fused_sampling` gives the
    ids of `u2_fused_sampling` alone; every call took the split form.  Above SPLIT_MAX_ROWS rows the one-workgroup kernel stays."""
    from u2tokenizer_amd import sampling
    new = 8
    ids = torch.randint(3, 512, (2, 12), generator=torch.Generator().manual_seed(5)).to(D)
    kw = dict(do_sample=True, top_p=0.9, temperature=0.7, max_new_tokens=new)
    m = _lm(u2_fused_sampling=True)
    torch.manual_seed(11)
    want = m.generate(None, ids, **kw)
    m.config.u2_fused_sampling_split = True
    n = dict(sampling.stats)
    torch.manual_seed(11)
    got = m.generate(None, ids, **kw)
    assert torch.equal(got, want)
    assert sampling.stats["split"] - n["split"] == new and sampling.stats["fused"] - n["fused"] == new and sampling.stats["stock"] == n["stock"]
    f = sampling.FusedSamplingWarper(0.7, 0, 0.9, 1, split=True)
    x = SC.logits(sampling.SPLIT_MAX_ROWS + 1, 4097, seed=2).to(D)
    n = dict(sampling.stats)
    out = f(None, x)
    assert sampling.stats["split"] == n["split"] and sampling.stats["fused"] == n["fused"] + 1
    assert torch.equal(out, ops.sample_warp(x, 0.7, 0, 0.9, 1)) and torch.equal(ops.sample_warp_split(x, 0.7, 0, 0.9, 1), out)
