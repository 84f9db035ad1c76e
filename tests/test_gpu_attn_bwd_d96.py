"""GPU: the flash attention backward at head dim 96 (u2tok_attention_gqa_bwd_d96: the <96, true> instantiations of csrc/attn_bwd.hip's
kernel pair) element by element against float64, as tests/test_gpu_decoder_train_ops.py holds the d = 64 / 128 instantiations: the
same first-order bounds (tests/test_decoder_train_bounds_host.py: attn_bwd_model, no fitted factor), the same buffers (column views
of a packed q | k | v at ld = W + 8 with batch gaps, NaN in every pad, compared as integers afterwards), on the cases of
tests/attn_d96_cases.py -- which tests/test_attn_bwd_d96_host.py shows the bf16 emulation to stay inside.  The worst error / bound
per output goes to the parity record under "decoder_train_ops_error_over_bound" (keys "attention_gqa_bwd_d96 ...")."""
import pytest
import torch

import test_decoder_train_bounds_host as B
import test_gpu_decoder_train_ops as G
from attn_d96_cases import D96_CASES, case_id, inputs, model
from test_gpu_backward_ops import call, guard_intact, nan32, ops, workspace  # noqa: F401
from u2tokenizer_amd import _lib

pytestmark = pytest.mark.gpu
D = "cuda"
NAME = "attention_gqa_bwd_d96"


def _backward(ops, x, out_b, dout, nb, S, Hq, Hkv, scale, kv, lse):
    """u2tok_attention_gqa_bwd_d96 through the C ABI: q | k | v column views at ld = W + 8, out / d_out at ld = Hq d + 8, dq, dk, dv
    three separate buffers at ld_d = Hq d + 4, all with batch gaps; lse (nb Hq, S) or None is passed at lse_ld = S + 3"""
    d = 96
    W = (Hq + 2 * Hkv) * d
    qkv = G.Batched(nb, S, W, W + 8, 16, x)
    o, g = G.Batched(nb, S, Hq * d, Hq * d + 8, 8, out_b), G.Batched(nb, S, Hq * d, Hq * d + 8, 8, dout)
    dq = G.Batched(nb, S, Hq * d, Hq * d + 4, 4)
    dk, dv = G.Batched(nb, S, Hkv * d, Hq * d + 4, 4), G.Batched(nb, S, Hkv * d, Hq * d + 4, 4)
    nbytes = _lib.load_library().u2tok_attention_gqa_bwd_workspace_bytes(nb, S, Hq)
    assert nbytes == 2 * ((nb * Hq * -(-S // 64) * 64 * 4 + 255) // 256 * 256)
    ws = workspace(nbytes)
    assert ws.data_ptr() % 256 == 0
    lp = None
    if lse is not None:
        lp = nan32(nb * Hq * (S + 3))
        lp.view(nb * Hq, S + 3)[:, :S] = lse
    call(ops, "u2tok_attention_gqa_bwd_d96", qkv.ptr(), qkv.ptr(Hq * d), qkv.ptr((Hq + Hkv) * d), qkv.ld, qkv.bs, o.ptr(), g.ptr(), o.ld,
         o.bs, dq.ptr(), dk.ptr(), dv.ptr(), dq.ld, dq.bs, nb, S, Hq, Hkv, scale, None if kv is None else kv.data_ptr(),
         None if lp is None else lp.data_ptr(), S + 3 if lp is not None else 0, ws.data_ptr(), nbytes)
    assert guard_intact(ws, nbytes)
    assert qkv.pads_intact() and o.pads_intact() and g.pads_intact(), "pads of the inputs changed"
    assert dq.pads_intact() and dk.pads_intact() and dv.pads_intact(), "pads of dq / dk / dv written"
    return dq.view.clone(), dk.view.clone(), dv.view.clone()


@pytest.mark.parametrize("case", D96_CASES, ids=case_id)
def test_attention_gqa_bwd_d96_bounds(ops, case):
    """dq, dk, dv per element within attn_bwd_model's bounds of float64, from the float64 forward's out rounded to bf16: with the
    forward kernel's lse (charged at its 1e-5) and with lse = NULL (the kernel's own sweep), the two within the bound of each other,
    each bit-repeatable over two launches; once more through ops.attention_gqa_bwd in the packed layout (which dispatches on d).
    dk / dv rows at or beyond kv_len are exactly zero, in blocks only partly beyond it too; other finite data (up to 64) in the k / v
    rows there changes no bit of dq or of dk / dv below kv_len; kv_len = NULL bit-equals kv_len = S.  The general entry point keeps
    refusing d = 96 with real buffers as well."""
    nb, S, Hq, Hkv, d, lens = case
    inp = inputs(case)
    x, dout, scale, kv = inp["qkv"], inp["dout"], d ** -0.5, G._kv(lens)
    m, m0 = model(case, True), model(case, False)
    xd = x.to(D)
    _, lse = ops.attention_gqa_ex(xd[..., :Hq * d], xd[..., Hq * d:(Hq + Hkv) * d], xd[..., (Hq + Hkv) * d:], Hq, Hkv, scale, kv_len=kv,
                                  with_lse=True)
    G.hold("attention_gqa_ex d96 lse", lse.double() * G.LN2, m["lse"], 1e-5 * m["lse"].abs().clamp_min(1.0))
    args = (nb, S, Hq, Hkv, scale)
    with_lse = _backward(ops, x, m["out_b"], dout, *args, kv, lse)
    G._hold_grads(NAME, with_lse, m)
    no_lse = _backward(ops, x, m["out_b"], dout, *args, kv, None)
    G._hold_grads(NAME + " (lse rebuilt)", no_lse, m0)
    for n, a, b in zip(("dq", "dk", "dv"), with_lse, no_lse):
        G.hold(f"{NAME} lse given vs rebuilt {n}", a, b.double().cpu(), m[n + "_bound"])
    for first, l in ((with_lse, lse), (no_lse, None)):
        again = _backward(ops, x, m["out_b"], dout, *args, kv, l)
        assert all(torch.equal(G.bits(a), G.bits(b)) for a, b in zip(first, again)), "not bit-repeatable"
    packed = ops.attention_gqa_bwd(xd, m["out_b"].to(D), dout.to(D), Hq, Hkv, scale, kv_len=kv, lse=lse)
    G._hold_grads(NAME + " (packed)", (packed[..., :Hq * d], packed[..., Hq * d:(Hq + Hkv) * d], packed[..., (Hq + Hkv) * d:]), m)
    if lens is None:
        full = _backward(ops, x, m["out_b"], dout, *args, G._kv([S] * nb), lse)
        assert all(torch.equal(G.bits(a), G.bits(b)) for a, b in zip(with_lse, full)), "kv_len = NULL differs from kv_len = S"
        return
    cut = [max(1, min(n, S)) for n in lens]
    for b, n in enumerate(cut):
        for t in (with_lse[1], with_lse[2], no_lse[1], no_lse[2], packed[..., Hq * d:(Hq + Hkv) * d], packed[..., (Hq + Hkv) * d:]):
            assert (t[b, n:].float() == 0).all(), f"dk / dv of sequence {b} not zero at or beyond kv_len = {n}"
    if any(n < S for n in cut):
        y = x.clone()
        y[..., Hq * d:] = B.other_tail(x[..., Hq * d:], cut, S)
        for first, l in ((with_lse, lse), (no_lse, None)):
            other = _backward(ops, y, m["out_b"], dout, *args, kv, l)
            assert torch.equal(G.bits(first[0]), G.bits(other[0])), "dq depends on keys at or beyond kv_len"
            for b, n in enumerate(cut):
                assert torch.equal(G.bits(first[1][b, :n]), G.bits(other[1][b, :n]))
                assert torch.equal(G.bits(first[2][b, :n]), G.bits(other[2][b, :n]))
                assert (other[1][b, n:].float() == 0).all() and (other[2][b, n:].float() == 0).all()


def test_the_general_entry_point_still_refuses_head_dim_96(ops):
    nb, S, Hq, Hkv, d = 1, 8, 2, 1, 96
    W = (Hq + 2 * Hkv) * d
    qkv, o = G.Batched(nb, S, W, W, 0), G.Batched(nb, S, Hq * d, Hq * d, 0)
    dqkv = G.Batched(nb, S, W, W, 0)
    nbytes = _lib.load_library().u2tok_attention_gqa_bwd_workspace_bytes(nb, S, Hq)
    ws = workspace(nbytes)
    call(ops, "u2tok_attention_gqa_bwd", qkv.ptr(), qkv.ptr(Hq * d), qkv.ptr((Hq + Hkv) * d), W, S * W, o.ptr(), o.ptr(), Hq * d, S * Hq * d,
         dqkv.ptr(), dqkv.ptr(Hq * d), dqkv.ptr((Hq + Hkv) * d), W, S * W, nb, S, Hq, Hkv, d, d ** -0.5, None, None, 0, ws.data_ptr(), nbytes,
         status=-1)
    assert G.is_nan16(dqkv.st) and guard_intact(ws, 0)
