"""GPU: the decoder's forward row kernels element by element against float64 -- u2tok_rmsnorm_bf16 (rmsnorm_row<NC>, csrc/rows.h),
u2tok_qk_norm_rope / u2tok_qk_norm_rope_kv (qk_norm_rope_kernel<D, CS>) and u2tok_swiglu_bf16 (csrc/decoder.hip) -- through the C
entry points, so that strides and pointers are the test's own, at the smallest shapes that reach every branch of their launchers:
the norm's tiers <2> <4> <8> <16>, each with a full and a partly filled set of 64 chunks, 1 / 5 / 37 rows (four per workgroup, the
last one ragged), dense and padded rows; every (head dim 64 / 96 / 128) x (norm on / off) x (fp32 / 16-bit table) instantiation of
the rotary kernel at (2, 1) / (3, 1) / (4, 4) heads and 1 / 9 / 37 rows, dense and padded, and the same with the KV-cache write,
dense and appended into a larger buffer; SwiGLU over one to three workgroups with dense and padded leading dimensions.

These kernels are what "has the bits of" means in tests/test_gpu_rows_norm.py, test_gpu_decode_head.py, test_gpu_rope_kv8.py, the
GEMM pair forms and the whole-stack decode step; this module is what holds the anchors themselves.  Every bound is the first-order
model written out in tests/test_decoder_fwd_bounds_host.py (the *_model functions), which also proves on the host that an emulation
of each kernel stays inside it on exactly these cases and inputs and that a kernel wrong in one of 11 named ways does not.  On top
of the bound: the norm's two rounding points bit for bit (`points_hold`: rnd(rnd(n) w), or a candidate where n is a near tie), the
rotation without norm on a 16-bit table bit for bit (`exact`), the identity table row, an all-zero row, the v columns untouched.
More than half of the rotary tables have independent halves, which a HuggingFace table cannot offer.  Every buffer a kernel writes
is pre-filled with a NaN bit pattern -- pads, the elements before an offset, unused cache positions and a guard tail -- and compared
as integers afterwards; every call runs twice and the two results have equal bits.  The first case of every kernel also runs on the
f16 build.  The worst error / bound ratio per kernel goes to the parity record under "decoder_fwd_error_over_bound", the module's
wall time under "decoder_fwd_wall_s".  First measured on the MI355X: rmsnorm 0.951 (padded 0.887), qk_norm_rope 0.991 (with the
head norm 0.811), swiglu 0.931; f16 0.731 / 0.649 / 0.696; no element of any case took the other candidate of a near tie; 0.7 s.
A ratio just under 1 is a correctly rounded result on the worst-placed element (see the host module's docstring), not a near miss."""
import time

import pytest
import torch

import test_decoder_fwd_bounds_host as M
from suite_budget import record
from test_gpu_backward_ops import nan32, ops  # noqa: F401
from test_gpu_row_fwd_bounds import GUARD, bits, call, canary, index3, only_wrote, place, tag, total_of
from test_row_fwd_bounds_host import worst

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ---- RMSNorm: C, rows, padded (ldx = C + 8, ldy = C + 16).  Rows 5 first: the first case, which also runs in f16, has the special rows
RMS_WIDTHS = (8, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8192)
RMS_CASES = [(C, rows, False) for C in RMS_WIDTHS for rows in (5, 1, 37)] + [(C, 5, True) for C in (520, 1032, 2056, 4104)]

# ---- q | k: rows, Hq, Hkv, D, norm, fp32 table, padded (ld = W + 8, cs_ld = D + 8), table ("free": independent halves, or theta).
# rows x (Hq + Hkv) is (9 x 4, 37 x 8) and is not (9 x 3, 37 x 3, 1 x 3) a multiple of the 4 items of a workgroup
QK_CASES = [(9, 2, 1, 64, True, False, True, "free"), (37, 3, 1, 64, True, True, False, "free"), (9, 4, 4, 64, False, False, False, "free"),
            (1, 2, 1, 64, False, True, True, "1e4"), (9, 3, 1, 96, True, True, True, "free"), (37, 2, 1, 96, True, False, False, "1e6"),
            (9, 2, 1, 96, False, False, True, "free"), (37, 4, 4, 96, False, True, False, "1e4"), (37, 4, 4, 128, True, False, True, "free"),
            (1, 3, 1, 128, True, True, False, "1e6"), (9, 3, 1, 128, False, False, False, "1e4"), (37, 2, 1, 128, False, True, True, "free")]

# ---- the same through u2tok_qk_norm_rope_kv: nb, S, Hq, Hkv, D, norm, fp32 table, table, capacity (0: dense, kv_stride = 0), s_off
QK_KV_CASES = [(2, 5, 2, 1, 64, True, False, "free", 0, 0), (3, 3, 4, 4, 128, False, True, "1e4", 0, 0),
               (2, 5, 3, 1, 96, True, True, "free", 16, 0), (3, 3, 2, 1, 64, True, False, "1e6", 16, 3),
               (2, 5, 4, 4, 128, False, False, "free", 16, 11)]

# ---- SwiGLU: rows, I, ld_in - 2 I, ld_out - I; (300, 16) is three workgroups, the last one ragged
SWIGLU_CASES = [(7, 16, 0, 0), (1, 8, 8, 16), (7, 1536, 16, 8), (300, 16, 0, 0), (300, 16, 8, 8), (1, 8, 0, 0), (7, 1536, 0, 0), (7, 16, 16, 8)]

_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.monotonic()
    yield
    record("decoder_fwd_wall_s", round(time.monotonic() - t, 1))
    print(f"\ntests/test_gpu_decoder_fwd_bounds.py: {time.monotonic() - t:.1f} s; error / bound: {_RATIOS}")


def hold(name, got, ref, bound):
    """every element of got finite and within bound of ref; the worst ratio is printed and recorded before it is asserted"""
    err = (got.detach().double().cpu() - ref).abs()
    assert torch.isfinite(err).all(), f"{name}: non-finite elements (left unwritten, or a pad was read?)"
    r = worst(err, bound)
    _RATIOS[name] = round(max(_RATIOS.get(name, 0.0), r), 4)
    record("decoder_fwd_error_over_bound", _RATIOS)
    print(f"{name}: error / bound = {r:.3f}")
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst ratio {r:.3f}; first at {i}: "
                             f"got {got[i].item()}, want {ref[i].item()} +- {bound[i].item()}")


def hold_points(name, got, p, sel=slice(None)):
    """the norm's rounding points, bit for bit (M.points_hold); the share of excused elements is printed"""
    ok, n_alt = M.points_hold(got, p, sel)
    print(f"{name}: {n_alt} of {p['want'][sel].numel()} elements took the other candidate of a near tie (share of near ties {p['share']:.4f})")
    assert p["share"] <= M.NEAR_TIE_CAP
    assert ok, f"{name}: an element is neither rnd(rnd(n) w) nor, at a near tie, a candidate"


def same_bits(a, b):
    return torch.equal(bits(a).cpu(), bits(b).cpu())


def untouched(st):
    return bool((bits(st) == bits(canary(1))[0]).all())


# ---------------------------------------------------------------------------------------------------------------- RMSNorm
def _rms_run(ops, inp, rows, C, padded, el=M.BF16):
    """x at ldx, y at ldy, both 8 elements into canary storage -> y (rows, C) after two bit-equal calls"""
    ldx, ldy = (C + 8, C + 16) if padded else (C, C)
    xi, yi = index3(8, 1, rows, C, 0, ldx)[0], index3(8, 1, rows, C, 0, ldy)[0]
    x = place(inp["x"], xi, total_of(xi), el)
    w = inp["w"].to(DEV)
    got = []
    for _ in range(2):
        y = canary(total_of(yi), el)
        call(ops, "u2tok_rmsnorm_bf16", x.data_ptr() + 16, w.data_ptr(), y.data_ptr() + 16, rows, C, ldx, ldy, inp["eps"], el=el)
        assert only_wrote(y, yi), "rmsnorm wrote outside its rows"
        got.append(y[yi.to(DEV)])
    assert same_bits(*got), "two calls differ"
    return got[0]


def _rms_check(ops, C, rows, padded, el=M.BF16):
    inp = M.rms_inputs(rows, C, el)
    m = M.rms_model(**inp, el=el)
    got = _rms_run(ops, inp, rows, C, padded, el)
    name = tag(el) + "rmsnorm" + (" padded" if padded else "")
    hold(name, got, m["y"], m["bound"])
    hold_points(name, got, m["points"])
    if rows >= 5:
        assert (got[4] == 0).all(), "the all-zero row"


@pytest.mark.parametrize("C", RMS_WIDTHS)
def test_rmsnorm_bounds_and_rounding_points_at_every_tier(ops, C):
    """y within rms_model's bound (the rounding of n = x rstd times |w|, (C / 2 + 4) u |y|, the store rounding on top) and equal to
    rnd(rnd(n) w) bit for bit outside the near ties of n, at rows 5 / 1 / 37; one width per tier also at ldx = C + 8, ldy = C + 16
    with NaN pads.  Rows 1 .. 4 of the 5- and 37-row inputs: scaled by 2^-40 (eps decides), scaled by 2^30, one non-zero element, all
    zero (exactly zero out)."""
    n = 0
    for case in RMS_CASES:
        if case[0] == C:
            _rms_check(ops, *case)
            n += 1
    assert n >= 3


def test_rmsnorm_refusals_leave_the_output_alone(ops):
    """C = 8200 (> 8192), C = 12, ldx = C + 4 and a pointer 8 bytes off 16-byte alignment: U2TOK_ERR_ARG, nothing written"""
    buf = torch.zeros(3 * 8200 + 64, dtype=torch.bfloat16, device=DEV)
    y = canary(8200 + 64)
    p, q = buf.data_ptr(), y.data_ptr()
    ptrs = dict(x=p, w=p + 2 * 8200, y=q)

    def refuse(C=8, ldx=8, ldy=8, **moved):
        a = dict(ptrs, **moved)
        call(ops, "u2tok_rmsnorm_bf16", a["x"], a["w"], a["y"], 1, C, ldx, ldy, 1e-6, status=-1)

    refuse(C=8200, ldx=8200, ldy=8200)
    refuse(C=12, ldx=16, ldy=16)
    refuse(ldx=12)
    refuse(ldy=12)
    for k in ptrs:
        refuse(**{k: ptrs[k] + 8})
    assert untouched(y)
    call(ops, "u2tok_rmsnorm_bf16", p, ptrs["w"], q, 1, 8, 8, 8, 1e-6)       # the same call, aligned
    assert untouched(y[8:]) and torch.isfinite(y[:8].float()).all()


# ------------------------------------------------------------------------------------------------------- head norm + rotary
def _qk_run(ops, inp, rows, Hq, Hkv, Dh, padded, el=M.BF16, cache=None):
    """qkv (rows, W) at ld, 8 elements into canary storage; the tables at cs_ld with NaN pads.  cache: (k storage, v storage, S,
    kv_stride, s_off) -> u2tok_qk_norm_rope_kv.  -> qkv (rows, W) after the call; pads and guard untouched."""
    W = (Hq + 2 * Hkv) * Dh
    ld, cs_ld = (W + 8, Dh + 8) if padded else (W, Dh)
    qi = index3(8, 1, rows, W, 0, ld)[0]
    st = place(inp["qkv"], qi, total_of(qi), el)
    tabs = []
    for t in (inp["cos"], inp["sin"]):
        if t.dtype == torch.float32:
            s = nan32(rows * cs_ld + GUARD)
            s[:rows * cs_ld].view(rows, cs_ld)[:, :Dh] = t.to(DEV)
        else:
            s = place(t, index3(0, 1, rows, Dh, 0, cs_ld)[0], rows * cs_ld + GUARD, el)
        tabs.append(s)
    norm = inp["wq"] is not None
    wq, wk = (inp["wq"].to(DEV), inp["wk"].to(DEV)) if norm else (None, None)
    args = (st.data_ptr() + 16, wq.data_ptr() if norm else None, wk.data_ptr() if norm else None, tabs[0].data_ptr(), tabs[1].data_ptr(),
            int(inp["cos"].dtype == torch.float32), rows, Hq, Hkv, Dh, ld, cs_ld, inp["eps"])
    if cache is None:
        call(ops, "u2tok_qk_norm_rope", *args, el=el)
    else:
        kc, vc, S, kvs, s_off = cache
        call(ops, "u2tok_qk_norm_rope_kv", *args, kc.data_ptr(), vc.data_ptr(), S, kvs, s_off, el=el)
    assert only_wrote(st, qi), "the rotary kernel wrote outside its rows"
    got = st[qi.to(DEV)]
    assert same_bits(got[:, (Hq + Hkv) * Dh:], inp["qkv"][:, (Hq + Hkv) * Dh:]), "v columns changed"
    return got


def _qk_check(ops, rows, Hq, Hkv, Dh, norm, tf, padded, table, el=M.BF16):
    inp = M.qk_inputs(rows, Hq, Hkv, Dh, norm, tf, table, el)
    m = M.qk_model(**inp, Hq=Hq, Hkv=Hkv, D=Dh, el=el)
    n = (Hq + Hkv) * Dh
    full = _qk_run(ops, inp, rows, Hq, Hkv, Dh, padded, el)
    assert same_bits(full, _qk_run(ops, inp, rows, Hq, Hkv, Dh, padded, el)), "two calls differ"
    got = full[:, :n]
    name = tag(el) + "qk_norm_rope" + (" norm" if norm else "")
    hold(name, got, m["out"], m["bound"])
    if "exact" in m:
        assert same_bits(got, m["exact"]), "no norm, 16-bit table: every element is the float64 value rounded through fp32"
    if rows >= 5:
        r = rows // 2
        if norm:
            hold_points(name + " identity row", got.reshape(rows, Hq + Hkv, Dh), m["points"], r)
        else:
            assert same_bits(got[r], inp["qkv"][r, :n]), "the identity rotation changed a value"
    return inp, full


@pytest.mark.parametrize("rows,Hq,Hkv,Dh,norm,tf,padded,table", QK_CASES)
def test_qk_norm_rope_bounds(ops, rows, Hq, Hkv, Dh, norm, tf, padded, table):
    """In place on the q | k columns, within qk_model's bound: the head norm's bound (the RMSNorm model over D columns, its store
    rounding included) carried through the rotation + 2 u (|a c| + |b s|) + the store rounding.  Seven of the twelve tables have
    independent halves, the others are rotary tables of theta 1e4 / 1e6 at positions past 1000.  The identity row comes back with
    the input's bits (no norm) or with the norm's rounding points; without norm and with a 16-bit table every element has the bits
    of the float64 expression rounded through fp32.  v columns, pads, the leading elements and the tail are bit-untouched."""
    _qk_check(ops, rows, Hq, Hkv, Dh, norm, tf, padded, table)


@pytest.mark.parametrize("nb,S,Hq,Hkv,Dh,norm,tf,table,cap,s_off", QK_KV_CASES)
def test_qk_norm_rope_kv_writes_the_cache_rows_and_nothing_else(ops, nb, S, Hq, Hkv, Dh, norm, tf, table, cap, s_off):
    """u2tok_qk_norm_rope_kv: the in-place result is bit-equal to the call without a cache (itself held to the bound); positions
    s_off .. s_off + S - 1 of k_cache / v_cache (nb, Hkv, capacity, D) have the bits of the finished k heads and of the v columns,
    every other cache element and the guard keep their canary.  Dense (kv_stride = 0: capacity = S) with two and three sequences,
    and appended at s_off = 0, 3 and capacity - S."""
    rows, padded = nb * S, bool(cap)
    inp, plain = _qk_check(ops, rows, Hq, Hkv, Dh, norm, tf, padded, table)
    capacity = cap or S
    assert 0 <= s_off <= capacity - S
    total = nb * Hkv * capacity * Dh
    idx = index3(s_off * Dh, nb * Hkv, S, Dh, capacity * Dh, Dh).view(nb, Hkv, S, Dh)
    results = []
    for _ in range(2):
        kc, vc = canary(total + GUARD), canary(total + GUARD)
        got = _qk_run(ops, inp, rows, Hq, Hkv, Dh, padded, cache=(kc, vc, S, cap * Dh, s_off))
        assert same_bits(got, plain), "the in-place result depends on the cache write"
        assert only_wrote(kc, idx) and only_wrote(vc, idx), "a cache position outside s_off .. s_off + S - 1 was written"
        k, v = (got[:, c * Dh:(c + Hkv) * Dh].view(nb, S, Hkv, Dh).permute(0, 2, 1, 3) for c in (Hq, Hq + Hkv))
        assert same_bits(kc[idx.to(DEV)], k), "k cache rows"
        assert same_bits(vc[idx.to(DEV)], v), "v cache rows"
        results.append((kc, vc))
    assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1])


# ------------------------------------------------------------------------------------------------------------------ SwiGLU
def _swiglu_check(ops, rows, I, pad_in, pad_out, el=M.BF16):
    inp = M.swiglu_inputs(rows, I, el)
    m = M.swiglu_model(**inp, el=el)
    ld_in, ld_out = 2 * I + pad_in, I + pad_out
    gi, oi = index3(8, 1, rows, 2 * I, 0, ld_in)[0], index3(8, 1, rows, I, 0, ld_out)[0]
    gu = place(inp["gu"], gi, total_of(gi), el)
    got = []
    for _ in range(2):
        out = canary(total_of(oi), el)
        call(ops, "u2tok_swiglu_bf16", gu.data_ptr() + 16, out.data_ptr() + 16, rows, I, ld_in, ld_out, el=el)
        assert only_wrote(out, oi), "swiglu wrote outside its rows"
        got.append(out[oi.to(DEV)])
    assert same_bits(*got), "two calls differ"
    hold(tag(el) + "swiglu", got[0], m["out"], m["bound"])


@pytest.mark.parametrize("rows,I,pad_in,pad_out", SWIGLU_CASES)
def test_swiglu_bounds(ops, rows, I, pad_in, pad_out):
    """out within swiglu_model's bound: (4 + 2 |g|) u |silu| and the rounding of silu, times |up|; the store rounding; |g| e^-|g| |up|
    for g <= -87, where 1 + e^-g overflows fp32 and the kernel returns zero.  Gates 2 N(0, 1) mixed with +-0, +-1e-30, +-20 ... +-104,
    +-1e4, -1.2785 and 2^-126; every output finite; NaN pads on both sides."""
    _swiglu_check(ops, rows, I, pad_in, pad_out)


def test_swiglu_refusals_leave_the_output_alone(ops):
    """I = 12, a pointer 8 bytes off 16-byte alignment, ld_out = I + 4 and ld_in = 2 I + 4: U2TOK_ERR_ARG, nothing written"""
    gu = torch.zeros(256, dtype=torch.bfloat16, device=DEV)
    out = canary(64 + GUARD)
    p, q = gu.data_ptr(), out.data_ptr()
    call(ops, "u2tok_swiglu_bf16", p, q, 1, 12, 24, 16, status=-1)
    call(ops, "u2tok_swiglu_bf16", p + 8, q, 1, 8, 16, 8, status=-1)
    call(ops, "u2tok_swiglu_bf16", p, q + 8, 1, 8, 16, 8, status=-1)
    call(ops, "u2tok_swiglu_bf16", p, q, 2, 8, 16, 12, status=-1)
    call(ops, "u2tok_swiglu_bf16", p, q, 2, 8, 20, 8, status=-1)
    assert untouched(out)
    call(ops, "u2tok_swiglu_bf16", p, q, 2, 8, 16, 8)       # the same call, admissible
    assert untouched(out[16:]) and (out[:16] == 0).all()


# ------------------------------------------------------------------------------------------------------------- f16 build
def test_first_case_of_every_kernel_on_the_f16_build(ops):
    """the same kernels compiled for IEEE half (U = 2^-11; the 16-bit rotary table is f16 too): the first case of every table, the
    rounding points included"""
    _rms_check(ops, *RMS_CASES[0], el=M.F16)
    _qk_check(ops, *QK_CASES[0], el=M.F16)
    _swiglu_check(ops, *SWIGLU_CASES[0], el=M.F16)
