"""GPU: the kernels of the decoder's training route element by element against float64 -- u2tok_rmsnorm_bwd, u2tok_qk_norm_rope_bwd,
u2tok_swiglu_bwd (csrc/backward.hip), u2tok_attention_gqa_ex (csrc/tokattn.hip), u2tok_attention_gqa_bwd and the non-causal
u2tok_flash_attention_d64_bwd (both csrc/attn_bwd.hip) -- at the branch points of their launchers: rows per wave (1, 2, 8, 16) with
ragged last waves and workgroups, every chunk tier of the row kernels, head dims 64 / 96 / 128, sequence and key lengths on and
next to the 64-row tile, 128-row block and 32-row wave edges, groups of 1, 2 and 8 query heads, padded leading dimensions and batch
strides, `accumulate`, NULL workspaces and statistics.

Every bound is the first-order model written out in tests/test_decoder_train_bounds_host.py (the *_model functions: one U = 2^-8
per bf16 rounding the kernel performs, n u sum |terms| for fp32 accumulation, no fitted factor), which also proves on the host that
an emulation of the kernel's rounding points stays inside it on exactly these cases and inputs.  Inputs are made on the host by
that module's *_inputs functions.  Buffers the kernels write are pre-filled with a NaN bit pattern, pads and guard tails included,
and compared as integers afterwards.  The worst error / bound ratio per kernel goes to the parity record under
"decoder_train_ops_error_over_bound"."""
import math
import time

import pytest
import torch

import test_decoder_train_bounds_host as B
from suite_budget import record
from test_gpu_backward_ops import NAN16, NAN32, bf16_key, call, guard_intact, nan16, nan32, ops, strided, workspace  # noqa: F401
from u2tokenizer_amd import _lib

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"
u, U = B.u, B.U
LN2 = math.log(2.0)

# rows, C, with dres: the chunk tiers (C <= 1024 / 2048 / 4096, partial and full chunk sets) at small row counts, then 1, 2 and 16
# rows per wave (rows / 2048 clamped to [1, 16]) with ragged last waves and workgroups at C = 264
RMS_CASES = [(3, 8, False), (5, 520, True), (7, 1024, False), (3, 1032, True), (5, 2048, False), (3, 2056, True), (5, 4096, True),
             (1, 264, True), (5, 264, False), (4095, 264, True), (4096, 264, False), (4097, 264, True), (32768 + 5, 264, False)]

# rows, Hq, Hkv, D, norm, fp32 cos / sin, padded strides: 1, 2 and 8 rows per wave (rows / 1024 clamped to [1, 8]) with few heads,
# (2, 1) / (4, 4) / (32, 8) heads at small row counts, every (D, norm, table type) combination
QK_CASES = [(1, 2, 1, 64, True, True, True), (9, 2, 1, 96, False, False, True), (2047, 2, 1, 128, True, False, True),
            (2048, 2, 1, 96, True, True, True), (2051, 2, 1, 64, False, True, False), (8197, 2, 1, 128, True, True, True),
            (9, 4, 4, 64, True, False, False), (9, 32, 8, 128, True, True, True), (9, 32, 8, 96, False, True, True),
            (9, 4, 4, 128, False, False, True), (9, 2, 1, 64, False, False, True), (9, 4, 4, 96, True, False, True),
            (2051, 2, 1, 128, False, True, True), (2051, 4, 4, 64, True, True, True)]

# rows, I, pads of ld_gu / ld_da / ld_dgu
SWIGLU_CASES = [(1, 8, (8, 16, 8)), (1, 16, (16, 8, 16)), (1, 1536, (8, 8, 16)), (7, 8, (16, 16, 8)), (7, 16, (8, 16, 16)),
                (7, 1536, (16, 8, 8)), (300, 8, (8, 8, 8)), (300, 16, (16, 16, 16)), (300, 1536, (8, 16, 8))]

# nb, S, Hq, Hkv, d, key lengths (as passed: values above S are the kernel's to clamp) -- forward and backward
ATTN_CASES = [(3, 1, 2, 1, 64, (1, 6, 1)), (3, 33, 8, 1, 64, (1, 33, 38)), (3, 64, 2, 2, 128, (63, 64, 65)),
              (3, 65, 4, 2, 64, (64, 65, 1)), (3, 128, 8, 1, 128, (63, 128, 65)), (3, 129, 2, 1, 128, (128, 129, 64)),
              (3, 257, 4, 2, 64, (128, 257, 65)), (3, 257, 2, 2, 128, (262, 64, 63)), (3, 257, 8, 1, 64, (129, 1, 257)),
              (1, 129, 8, 1, 64, None), (2, 257, 2, 1, 128, None)]

# nb, Sq, Skv, Hq, Hkv, d, key lengths: the forward with fewer queries than keys (query i sees keys j <= i + Skv - Sq)
FWD_UNEQUAL_CASES = [(2, 40, 100, 4, 2, 64, (100, 57)), (2, 40, 100, 2, 2, 128, (64, 105))]

# S, H of u2tok_flash_attention_d64_bwd (no mask, equal heads)
D64_CASES = [(64, 1), (65, 3), (129, 1), (257, 3)]

_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.monotonic()
    yield
    record("decoder_train_ops_wall_s", round(time.monotonic() - t, 1))
    print(f"\ntests/test_gpu_decoder_train_ops.py: {time.monotonic() - t:.1f} s; error / bound: {_RATIOS}")


def hold(name, got, ref, bound):
    """every element of got within bound of ref; the worst ratio is printed and recorded before it is asserted"""
    err = (got.detach().double().cpu() - ref).abs()
    assert torch.isfinite(err).all(), f"{name}: non-finite elements (left unwritten?)"
    r = B.worst(err, bound)
    _RATIOS[name] = round(max(_RATIOS.get(name, 0.0), r), 4)
    record("decoder_train_ops_error_over_bound", _RATIOS)
    print(f"{name}: error / bound = {r:.3f}")
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        ulps = (bf16_key(got.detach().cpu().to(bf)) - bf16_key(ref.to(bf))).abs()[bad].max().item() if got.dtype == bf else "-"
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst ratio {r:.3f}, up to {ulps} bf16 "
                             f"steps off; first at {i}: got {got[i].item()}, want {ref[i].item()} +- {bound[i].item()}")


def is_nan16(t):
    return bool((t.contiguous().view(torch.int16) == NAN16).all())


def is_nan32(t):
    return bool((t.contiguous().view(torch.int32) == NAN32).all())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf else torch.int32)


def strided32(rows, C, ld, src):
    st = nan32(rows * ld)
    st.view(rows, ld)[:, :C] = src.to(D)
    return st


# ---------------------------------------------------------------------------------------------------------------- RMSNorm
@pytest.mark.parametrize("rows,C,with_dres", RMS_CASES)
def test_rmsnorm_bwd_bounds(ops, rows, C, with_dres):
    """dx per element within rms_model's dx_bound: U |dx| + rstd U (|g| + |xhat| mean(|g| |xhat|)) + the fp32 terms; dw within
    rows u sum_r |dy n| + the near-tie allowance, n = bf16(xhat).  accumulate = 0 overwrites a NaN-filled dw; accumulate = 1 adds onto
    a finite one: within u (|prefill| + |sum|) of prefill + the first result.  Two calls are bit-equal.  The workspace is exactly
    u2tok_rmsnorm_bwd_workspace_bytes (one partial row per workgroup of 4 waves x rows-per-wave rows) with an intact guard; one byte
    less is U2TOK_ERR_WORKSPACE; dx's tail stays untouched."""
    inp = B.rms_inputs(rows, C, with_dres)
    m = B.rms_model(**inp)
    nbytes = _lib.load_library().u2tok_rmsnorm_bwd_workspace_bytes(rows, C)
    assert nbytes == -(-rows // (4 * max(1, min(16, rows // 2048)))) * C * 4
    x, w, dy = inp["x"].to(D), inp["w"].to(D), inp["dy"].to(D)
    dres = inp["dres"].to(D) if with_dres else None

    def run(dw, acc, ws_bytes=nbytes, status=0):
        ws, dx = workspace(nbytes), nan16(rows * C + 64)
        call(ops, "u2tok_rmsnorm_bwd", x.data_ptr(), w.data_ptr(), dy.data_ptr(), None if dres is None else dres.data_ptr(),
             dx.data_ptr(), dw.data_ptr(), rows, C, inp["eps"], ws.data_ptr(), ws_bytes, acc, status=status)
        assert guard_intact(ws, nbytes) and is_nan16(dx[rows * C:])
        return dx[:rows * C].view(rows, C)

    dw = nan32(C + 16)
    dx = run(dw, 0)
    assert is_nan32(dw[C:])
    hold("rmsnorm_bwd dx", dx, m["dx"], m["dx_bound"])
    hold("rmsnorm_bwd dw", dw[:C], m["dw"], m["dw_bound"])
    dw2 = nan32(C + 16)
    dx2 = run(dw2, 0)
    assert torch.equal(bits(dx), bits(dx2)) and torch.equal(bits(dw), bits(dw2))
    acc = torch.cat([inp["prefill"].to(D), nan32(16)])
    dx3 = run(acc, 1)
    assert torch.equal(bits(dx), bits(dx3)) and is_nan32(acc[C:])
    want = inp["prefill"].double() + dw[:C].double().cpu()
    hold("rmsnorm_bwd dw: accumulate", acc[:C], want, u * (inp["prefill"].double().abs() + dw[:C].double().cpu().abs()))
    left = nan32(C)
    untouched = run(left, 0, ws_bytes=nbytes - 1, status=-3)
    assert is_nan32(left) and is_nan16(untouched)


# ------------------------------------------------------------------------------------------------------- head norm + rotary
@pytest.mark.parametrize("rows,Hq,Hkv,Dh,norm,f32,padded", QK_CASES)
def test_qk_norm_rope_bwd_bounds(ops, rows, Hq, Hkv, Dh, norm, f32, padded):
    """In place on the q | k columns of dqkv.  Rotation only: within U |ref| + 2 u (|ya c| + |yb s|), and the row with cos = 1,
    sin = 0 comes back bit-identical; workspace NULL with 0 bytes.  With norm: qk_model's bound (the RMSNorm model over the D
    columns of a head); dwq / dwk within (N + 1) u sum |d n| + 3 u sum mag |n| + the near-tie allowance, bit-repeatable, and with
    accumulate within u (|prefill| + |sum|) of prefill + sum.  Padded: ld = (Hq + 2 Hkv) D + 8, ld_pre = (Hq + Hkv) D + 16,
    cs_ld = D + 8 with NaN in every pad element; pad columns, v columns, the tails of dwq / dwk and the workspace guard are
    bit-untouched."""
    inp = B.qk_inputs(rows, Hq, Hkv, Dh, norm, f32)
    m = B.qk_model(Hq=Hq, Hkv=Hkv, D=Dh, **inp)
    W, n = (Hq + 2 * Hkv) * Dh, (Hq + Hkv) * Dh
    ld, ld_pre, cs_ld = (W + 8, n + 16, Dh + 8) if padded else (W, n, Dh)
    pre = strided(rows, n, ld_pre, inp["pre"])[0] if norm else None
    wq, wk = (inp["wq"].to(D), inp["wk"].to(D)) if norm else (None, None)
    cs = [strided32(rows, Dh, cs_ld, t) if f32 else strided(rows, Dh, cs_ld, t)[0] for t in (inp["cos"], inp["sin"])]
    nbytes = _lib.load_library().u2tok_qk_norm_rope_bwd_workspace_bytes(rows, Dh)
    assert nbytes == 2 * -(-rows // (4 * max(1, min(8, rows // 1024)))) * Dh * 4

    def run(dwq, dwk, acc):
        st, view = strided(rows, W, ld, inp["dy"])
        ws = workspace(nbytes) if norm else None
        call(ops, "u2tok_qk_norm_rope_bwd", st.data_ptr(), pre.data_ptr() if norm else None, wq.data_ptr() if norm else None,
             wk.data_ptr() if norm else None, cs[0].data_ptr(), cs[1].data_ptr(), int(f32), rows, Hq, Hkv, Dh, ld, ld_pre if norm else 0,
             cs_ld, inp["eps"], dwq.data_ptr() if norm else None, dwk.data_ptr() if norm else None, ws.data_ptr() if norm else None,
             nbytes if norm else 0, acc)
        assert not norm or guard_intact(ws, nbytes)
        assert is_nan16(view[:, W:]), "pad columns written"
        assert torch.equal(bits(view[:, n:W]), bits(inp["dy"][:, n:].to(D))), "v columns written"
        return view[:, :n]

    dwq, dwk = nan32(Dh + 16), nan32(Dh + 16)
    out = run(dwq, dwk, 0)
    hold("qk_norm_rope_bwd dq|dk", out, m["out"], m["out_bound"])
    if not norm:
        assert is_nan32(dwq) and is_nan32(dwk)
        r = rows // 2
        assert torch.equal(bits(out[r]), bits(inp["dy"][r, :n].to(D))), "the identity rotation changed a value"
        return
    assert is_nan32(dwq[Dh:]) and is_nan32(dwk[Dh:])
    hold("qk_norm_rope_bwd dwq", dwq[:Dh], m["dwq"], m["dwq_bound"])
    hold("qk_norm_rope_bwd dwk", dwk[:Dh], m["dwk"], m["dwk_bound"])
    dwq2, dwk2 = nan32(Dh + 16), nan32(Dh + 16)
    out2 = run(dwq2, dwk2, 0)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(dwq), bits(dwq2)) and torch.equal(bits(dwk), bits(dwk2))
    aq, ak = torch.cat([inp["prefill_q"].to(D), nan32(16)]), torch.cat([inp["prefill_k"].to(D), nan32(16)])
    out3 = run(aq, ak, 1)
    assert torch.equal(bits(out), bits(out3)) and is_nan32(aq[Dh:]) and is_nan32(ak[Dh:])
    for name, got, first, pf in (("dwq", aq, dwq, inp["prefill_q"]), ("dwk", ak, dwk, inp["prefill_k"])):
        s = first[:Dh].double().cpu()
        hold(f"qk_norm_rope_bwd {name}: accumulate", got[:Dh], pf.double() + s, u * (pf.double().abs() + s.abs()))


# ------------------------------------------------------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("rows,I,pads", SWIGLU_CASES)
def test_swiglu_bwd_bounds(ops, rows, I, pads):
    """[d_gate | d_up] within swiglu_model's bounds (d_up: U |ref| + U |dact| |silu(g)|; d_gate: U |ref| + U |dact u| |silu'(g)|; a
    few u for the fp32 evaluation), gates out to +-30 where sigma saturates; ld_gu, ld_da and ld_dgu 8 or 16 above their minimum,
    NaN in the pads, the output's pads untouched."""
    inp = B.swiglu_inputs(rows, I)
    m = B.swiglu_model(**inp)
    ld_gu, ld_da, ld_dgu = 2 * I + pads[0], I + pads[1], 2 * I + pads[2]
    gu, da = strided(rows, 2 * I, ld_gu, inp["gu"])[0], strided(rows, I, ld_da, inp["dact"])[0]
    dgu = nan16(rows * ld_dgu + 64)
    call(ops, "u2tok_swiglu_bwd", gu.data_ptr(), da.data_ptr(), dgu.data_ptr(), rows, I, ld_gu, ld_da, ld_dgu)
    assert is_nan16(dgu[rows * ld_dgu:])
    got = dgu[:rows * ld_dgu].view(rows, ld_dgu)
    assert is_nan16(got[:, 2 * I:]), "pad columns written"
    hold("swiglu_bwd d_gate", got[:, :I], m["d_gate"], m["d_gate_bound"])
    hold("swiglu_bwd d_up", got[:, I:2 * I], m["d_up"], m["d_up_bound"])


# --------------------------------------------------------------------------------------------------------------- attention
class Batched:
    """(nb, S, W) bf16 at row stride ld and batch stride S ld + gap inside NaN-filled storage"""

    def __init__(self, nb, S, W, ld, gap, src=None):
        self.bs = S * ld + gap
        self.st = nan16(nb * self.bs)
        self.ld = ld
        self.view = self.st.as_strided((nb, S, W), (self.bs, ld, 1))
        self.pad = torch.ones(nb * self.bs, dtype=torch.bool, device=D)
        self.pad.as_strided((nb, S, W), (self.bs, ld, 1)).fill_(False)
        if src is not None:
            self.view.copy_(src.to(D))

    def ptr(self, col=0):
        return self.st.data_ptr() + 2 * col

    def pads_intact(self):
        return is_nan16(self.st[self.pad])


def _kv(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=D)


def _forward(ops, q, k, v, nb, Sq, Skv, Hq, Hkv, d, scale, kv):
    """u2tok_attention_gqa_ex through the C ABI on column views q / k / v ((Batched, first column)): out at ld = Hq d + 8 with a
    batch gap, lse at lse_ld = Sq + 3 -> (out (nb, Sq, Hq d), lse (nb Hq, Sq) in log2 units)"""
    out = Batched(nb, Sq, Hq * d, Hq * d + 8, 8)
    lse = nan32(nb * Hq * (Sq + 3))
    call(ops, "u2tok_attention_gqa_ex", q[0].ptr(q[1]), k[0].ptr(k[1]), v[0].ptr(v[1]), out.ptr(), nb, Sq, Skv, Hq, Hkv, d, q[0].ld, k[0].ld,
         v[0].ld, out.ld, q[0].bs, k[0].bs, v[0].bs, out.bs, scale, 1, None if kv is None else kv.data_ptr(), lse.data_ptr(), Sq + 3)
    assert out.pads_intact() and is_nan32(lse.view(nb * Hq, Sq + 3)[:, Sq:]), "pads of out / lse written"
    return out.view.clone(), lse.view(nb * Hq, Sq + 3)[:, :Sq].clone()


def _hold_forward(name, out, lse, f, nb, Hq):
    hold(name + " out", out, B.rows_of(f["out"]), B.rows_of(f["out_bound"]))
    want = f["lse"].reshape(nb * Hq, -1)
    hold(name + " lse", lse.double() * LN2, want, f["lse_tol"].reshape(want.shape))


@pytest.mark.parametrize("nb,S,Hq,Hkv,d,lens", ATTN_CASES)
def test_attention_gqa_ex_forward_bounds(ops, nb, S, Hq, Hkv, d, lens):
    """out per element within U |ref| (the output rounding) + U sum_j P_j |v_j| (P a bf16 operand of the P V product) + the fp32
    accumulation: 2 U |ref| where a row's terms do not cancel, and no floor on max|ref| (attn_fwd_model says why the second rounding
    is charged on sum_j P_j |v_j| and not on |ref|); lse ln 2 within 1e-5 max(1, |lse|) of float64 on EVERY row, rows at or beyond kv_len included (they see the keys below it).  q | k | v
    are column views of a packed buffer at ld = W + 8 with a batch gap, out and lse padded; pads stay NaN.  Other finite data (up to
    64) in the k / v rows at or beyond kv_len changes no bit of out or lse."""
    inp = B.attn_inputs(nb, S, Hq, Hkv, d)
    W, scale, kv = (Hq + 2 * Hkv) * d, d ** -0.5, _kv(lens)
    x = inp["qkv"]
    f = B.attn_fwd_model(B.heads(x[..., :Hq * d], Hq, d), B.heads(x[..., Hq * d:(Hq + Hkv) * d], Hkv, d),
                         B.heads(x[..., (Hq + Hkv) * d:], Hkv, d), scale, B.visible(nb, S, S, lens))
    qkv = Batched(nb, S, W, W + 8, 16, x)
    out, lse = _forward(ops, (qkv, 0), (qkv, Hq * d), (qkv, (Hq + Hkv) * d), nb, S, S, Hq, Hkv, d, scale, kv)
    _hold_forward("attention_gqa_ex", out, lse, f, nb, Hq)
    if lens is not None and any(n < S for n in lens):
        y = x.clone()
        y[..., Hq * d:] = B.other_tail(x[..., Hq * d:], lens, S)
        qkv2 = Batched(nb, S, W, W + 8, 16, y)
        out2, lse2 = _forward(ops, (qkv2, 0), (qkv2, Hq * d), (qkv2, (Hq + Hkv) * d), nb, S, S, Hq, Hkv, d, scale, kv)
        assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(lse), bits(lse2)), "keys at or beyond kv_len were read"


@pytest.mark.parametrize("nb,Sq,Skv,Hq,Hkv,d,lens", FWD_UNEQUAL_CASES)
def test_attention_gqa_ex_forward_fewer_queries_than_keys(ops, nb, Sq, Skv, Hq, Hkv, d, lens):
    """Sq < Skv: query i sees keys j <= i + Skv - Sq and j < kv_len; the same bounds."""
    inp = B.attn_inputs(nb, Sq, Hq, Hkv, d, Skv=Skv)
    scale = d ** -0.5
    f = B.attn_fwd_model(B.heads(inp["q"], Hq, d), B.heads(inp["kv"][..., :Hkv * d], Hkv, d), B.heads(inp["kv"][..., Hkv * d:], Hkv, d),
                         scale, B.visible(nb, Sq, Skv, lens))
    q, kvb = Batched(nb, Sq, Hq * d, Hq * d + 8, 8, inp["q"]), Batched(nb, Skv, 2 * Hkv * d, 2 * Hkv * d + 16, 8, inp["kv"])
    out, lse = _forward(ops, (q, 0), (kvb, 0), (kvb, Hkv * d), nb, Sq, Skv, Hq, Hkv, d, scale, _kv(lens))
    _hold_forward("attention_gqa_ex", out, lse, f, nb, Hq)


def _backward(ops, x, out_b, dout, nb, S, Hq, Hkv, d, scale, kv, lse):
    """u2tok_attention_gqa_bwd through the C ABI: q | k | v column views at ld = W + 8, out / d_out at ld = Hq d + 8, dq, dk, dv three
    separate buffers at ld_d = Hq d + 4, all with batch gaps; lse (nb Hq, S) or None is passed at lse_ld = S + 3 -> dq, dk, dv"""
    W = (Hq + 2 * Hkv) * d
    qkv = Batched(nb, S, W, W + 8, 16, x)
    o, g = Batched(nb, S, Hq * d, Hq * d + 8, 8, out_b), Batched(nb, S, Hq * d, Hq * d + 8, 8, dout)
    assert o.bs == g.bs
    dq = Batched(nb, S, Hq * d, Hq * d + 4, 4)
    dk, dv = Batched(nb, S, Hkv * d, Hq * d + 4, 4), Batched(nb, S, Hkv * d, Hq * d + 4, 4)
    nbytes = _lib.load_library().u2tok_attention_gqa_bwd_workspace_bytes(nb, S, Hq)
    assert nbytes == 2 * ((nb * Hq * -(-S // 64) * 64 * 4 + 255) // 256 * 256)
    ws = workspace(nbytes)
    assert ws.data_ptr() % 256 == 0
    lp = None
    if lse is not None:
        lp = nan32(nb * Hq * (S + 3))
        lp.view(nb * Hq, S + 3)[:, :S] = lse
    call(ops, "u2tok_attention_gqa_bwd", qkv.ptr(), qkv.ptr(Hq * d), qkv.ptr((Hq + Hkv) * d), qkv.ld, qkv.bs, o.ptr(), g.ptr(), o.ld, o.bs,
         dq.ptr(), dk.ptr(), dv.ptr(), dq.ld, dq.bs, nb, S, Hq, Hkv, d, scale, None if kv is None else kv.data_ptr(),
         None if lp is None else lp.data_ptr(), S + 3 if lp is not None else 0, ws.data_ptr(), nbytes)
    assert guard_intact(ws, nbytes)
    assert dq.pads_intact() and dk.pads_intact() and dv.pads_intact(), "pads of dq / dk / dv written"
    return dq.view.clone(), dk.view.clone(), dv.view.clone()


def _hold_grads(name, got, m):
    for n, t in zip(("dq", "dk", "dv"), got):
        hold(f"{name} {n}", t, m[n], m[n + "_bound"])


@pytest.mark.parametrize("nb,S,Hq,Hkv,d,lens", ATTN_CASES)
def test_attention_gqa_bwd_bounds(ops, nb, S, Hq, Hkv, d, lens):
    """dq, dk, dv per element within attn_bwd_model's bounds (dD = U rowsum(|dO| |out|), ddS = U |dS| + P dD; dq: U |dq| + scale
    ddS |K|; dk: U |dk| + scale ddS^T |Q| and dv: U |dv| + U P^T |dO|, summed over the group's heads; fp32 terms on top), from the
    float64 forward's out rounded to bf16: with the forward kernel's lse (held to 1e-5 by the test above, charged as such) and with
    lse = NULL (the kernel's own sweep), the two within the bound of each other, each bit-repeatable; once more through
    ops.attention_gqa_bwd in the packed layout.  dk / dv rows at or beyond kv_len are exactly zero, in blocks only partly beyond it
    too; other finite data (up to 64) in the k / v rows there changes no bit of dq or of dk / dv below kv_len; kv_len = NULL
    bit-equals kv_len = S."""
    inp = B.attn_inputs(nb, S, Hq, Hkv, d)
    x, dout, scale, kv = inp["qkv"], inp["dout"], d ** -0.5, _kv(lens)
    m = B.attn_bwd_model(x, dout, Hq, Hkv, d, scale, lens, lse_given=True)
    m0 = B.attn_bwd_model(x, dout, Hq, Hkv, d, scale, lens)
    W = (Hq + 2 * Hkv) * d
    xd = x.to(D)
    _, lse = ops.attention_gqa_ex(xd[..., :Hq * d], xd[..., Hq * d:(Hq + Hkv) * d], xd[..., (Hq + Hkv) * d:], Hq, Hkv, scale, kv_len=kv,
                                  with_lse=True)
    args = (nb, S, Hq, Hkv, d, scale)
    with_lse = _backward(ops, x, m["out_b"], dout, *args, kv, lse)
    _hold_grads("attention_gqa_bwd", with_lse, m)
    no_lse = _backward(ops, x, m["out_b"], dout, *args, kv, None)
    _hold_grads("attention_gqa_bwd (lse rebuilt)", no_lse, m0)
    for n, a, b in zip(("dq", "dk", "dv"), with_lse, no_lse):
        hold(f"attention_gqa_bwd lse given vs rebuilt {n}", a, b.double().cpu(), m[n + "_bound"])
    for first, l in ((with_lse, lse), (no_lse, None)):
        again = _backward(ops, x, m["out_b"], dout, *args, kv, l)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, again)), "not bit-repeatable"
    packed = ops.attention_gqa_bwd(xd, m["out_b"].to(D), dout.to(D), Hq, Hkv, scale, kv_len=kv, lse=lse)
    _hold_grads("attention_gqa_bwd (packed)", (packed[..., :Hq * d], packed[..., Hq * d:(Hq + Hkv) * d], packed[..., (Hq + Hkv) * d:]), m)
    if lens is None:
        full = _backward(ops, x, m["out_b"], dout, *args, _kv([S] * nb), lse)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(with_lse, full)), "kv_len = NULL differs from kv_len = S"
        return
    cut = [max(1, min(n, S)) for n in lens]
    for b, n in enumerate(cut):
        for t in (with_lse[1], with_lse[2], no_lse[1], no_lse[2]):
            assert (t[b, n:].float() == 0).all(), f"dk / dv of sequence {b} not zero at or beyond kv_len = {n}"
    if any(n < S for n in cut):
        y = x.clone()
        y[..., Hq * d:] = B.other_tail(x[..., Hq * d:], cut, S)
        for first, l in ((with_lse, lse), (no_lse, None)):
            other = _backward(ops, y, m["out_b"], dout, *args, kv, l)
            assert torch.equal(bits(first[0]), bits(other[0])), "dq depends on keys at or beyond kv_len"
            for b, n in enumerate(cut):
                assert torch.equal(bits(first[1][b, :n]), bits(other[1][b, :n])) and torch.equal(bits(first[2][b, :n]), bits(other[2][b, :n]))
                assert (other[1][b, n:].float() == 0).all() and (other[2][b, n:].float() == 0).all()


@pytest.mark.parametrize("S,H", D64_CASES)
def test_flash_attention_d64_bwd_bounds(ops, S, H):
    """The non-causal instantiation of the same kernels (the ViT's: equal heads, every key visible, only the ragged last tile masked):
    the same dq / dk / dv bounds, with the forward kernel's lse (itself within 1e-5 max(1, |lse|) here) and without, bit-repeatable."""
    nb, scale = 2, 0.125
    inp = B.attn_inputs(nb, S, H, H, 64)
    x, dout = inp["qkv"], inp["dout"]
    m = B.attn_bwd_model(x, dout, H, H, 64, scale, None, causal=False, lse_given=True)
    m0 = B.attn_bwd_model(x, dout, H, H, 64, scale, None, causal=False)
    xd, od, gd = x.to(D), m["out_b"].to(D), dout.to(D)
    _, lse = ops.flash_attention_d64(xd, H, scale, return_lse=True)
    hold("flash_attention_d64 lse", lse[:, :S].double() * LN2, m["lse"], 1e-5 * m["lse"].abs().clamp_min(1.0))
    for name, l, mm in (("flash_attention_d64_bwd", lse, m), ("flash_attention_d64_bwd (lse rebuilt)", None, m0)):
        got = ops.flash_attention_d64_bwd(xd, od, gd, H, scale, lse=l)
        _hold_grads(name, (got[..., :H * 64], got[..., H * 64:2 * H * 64], got[..., 2 * H * 64:]), mm)
        assert torch.equal(bits(got), bits(ops.flash_attention_d64_bwd(xd, od, gd, H, scale, lse=l)))
