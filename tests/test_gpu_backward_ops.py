"""GPU: the backward row kernels of csrc/backward.hip (gelu_bwd, colsum, layernorm_bwd, softmax_bwd, relbias_grad, rowdot) element by
element against a float64 CPU computation of the same bf16 inputs -- at the thresholds of their launchers (vector / scalar column
sums, slab counts, LayerNorm chunk tiers and rows per wave), through the C entry points where a test needs a pre-filled output, a
guarded workspace or an argument the ops wrappers do not pass.

Small-integer data makes every fp32 sum exact: there the results must be bit-identical to the float64 sums.  On random data each
test states its bound; u = 2^-24 is the fp32 unit roundoff, U = 2^-8 that of bf16.  Workspaces are allocated at
*_workspace_bytes(...) plus a guard tail; workspaces, guards and pre-filled outputs hold a fixed NaN bit pattern, compared as
integers."""
import math

import pytest
import torch

from u2tokenizer_amd import _lib

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"
u, U = 2.0 ** -24, 2.0 ** -8
NAN16, NAN32 = 0x7FC1, 0x7FC00001          # quiet NaNs with a payload no arithmetic produces
GUARD = 256                                 # bytes past every workspace


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    return _ops


def call(ops, name, *args, status=0):
    """u2tok_<name>(*args, stream) on the stream and context the ops wrappers use; returns after the stream has drained"""
    anchor = torch.empty(1, dtype=bf, device=D)
    with ops.on_device(anchor, bf) as (h, st):
        got = getattr(h, name)(*args, st)
    torch.cuda.synchronize()
    assert got == status, (name, got, _lib.ERRORS.get(got, got))


def nan16(n):
    return torch.full((n,), NAN16, dtype=torch.int16, device=D).view(bf)


def nan32(n):
    return torch.full((n,), NAN32, dtype=torch.int32, device=D).view(torch.float32)


def workspace(nbytes):
    assert nbytes % 4 == 0
    return nan32((nbytes + GUARD) // 4)


def guard_intact(ws, nbytes):
    return bool((ws[nbytes // 4:].view(torch.int32) == NAN32).all())


def ints(*shape, lo=-4, hi=4, seed=0):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(bf)


def randn(*shape, scale=1.0, seed=0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(bf)


def strided(rows, C, ld, src, nan=True, off=0):
    """(storage on the GPU, view): a (rows, C) matrix at row stride ld, elements [C, ld) of every row and `off` leading elements NaN"""
    st = nan16(off + rows * ld) if nan else torch.zeros(off + rows * ld, dtype=bf, device=D)
    view = st[off:].view(rows, ld)
    view[:, :C] = src.to(D)
    return st, view


def bf16_key(t):
    """bf16 bits -> integers that order like the values (adjacent representable values differ by 1)"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


# ---------------------------------------------------------------------------------------------------------------- gelu_bwd
def _gelu_grad64(z):
    z = z.double()
    return 0.5 * torch.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _rounded_or_neighbour(got, ref):
    """got (bf16) is ref rounded to bf16 or its neighbour; below the fp32 normal range (2^-126) a result may also have lost its
    subnormal bits (flushed)"""
    d = (bf16_key(got) - bf16_key(ref.to(bf))).abs()
    tiny = (ref.abs() < 2.0 ** -126) & ((got.double() - ref).abs() <= 2.0 ** -126)
    return (d <= 1) | tiny


def test_gelu_bwd_over_all_bf16_inputs(ops):
    """gelu_bwd differentiates EXACT erf-GELU (not the approximation gelu_fast that the forward evaluates): dz = dy (Phi(z) + z phi(z)).
    Every finite bf16 z with |z| <= 30, dy = 1, then random dy: the result is the float64 value rounded to bf16, or its neighbour.
    Bound: the kernel's fp32 gelu'(z) carries a relative error of a few u (erfc, exp and their arguments; Phi computed as
    erfc(-z / sqrt 2) / 2, which does not cancel in the left tail), the product with dy adds u; a relative error << U / 2 moves the
    value across at most one rounding boundary of bf16.  Saturated ends are exact: 0 for z <= -15 (erfc and exp underflow), dy for
    z >= 6 (z phi(z) < u / 2).  Misaligned pointers and n % 8 != 0 are U2TOK_ERR_ARG."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    z = bits.view(bf)
    z = z[torch.isfinite(z.float()) & (z.float().abs() <= 30)]
    z = torch.cat([z, z[:(-z.numel()) % 8]])
    ref = _gelu_grad64(z)
    one = torch.ones_like(z)
    got = ops.gelu_bwd(z.to(D), one.to(D)).cpu()
    ok = _rounded_or_neighbour(got, ref)
    assert ok.all(), f"{(~ok).sum().item()} off, e.g. z = {z[~ok][:8].tolist()} -> {got[~ok][:8].tolist()} want {ref[~ok][:8].tolist()}"
    dy = randn(z.numel(), scale=3.0, seed=1)
    got = ops.gelu_bwd(z.to(D), dy.to(D)).cpu()
    ok = _rounded_or_neighbour(got, ref * dy.double())
    assert ok.all(), f"{(~ok).sum().item()} off, e.g. z = {z[~ok][:8].tolist()}"
    left, right = z.float() <= -15, z.float() >= 6
    assert left.sum() > 0 and right.sum() > 0
    assert (got.float()[left] == 0).all()
    assert torch.equal(got[right], dy[right])
    # argument checks: n % 8 != 0 and a buffer 2 bytes off 16-byte alignment (nothing is launched; the pointers stay inside)
    buf = torch.zeros(512, dtype=bf, device=D)
    p = buf.data_ptr()
    call(ops, "u2tok_gelu_bwd", p, p + 128, p + 256, 12, status=-1)
    for off in ((2, 0, 0), (0, 2, 0), (0, 0, 2)):
        call(ops, "u2tok_gelu_bwd", p + off[0], p + 32 + off[1], p + 64 + off[2], 8, status=-1)
    call(ops, "u2tok_gelu_bwd", p, p + 32, p + 64, 8)


# ------------------------------------------------------------------------------------------------------------------ colsum
def _slab_rows(rows, C):   # csrc/backward.hip colsum_slab_rows
    return max(4, min(128, (rows * ((C + 511) // 512) // 1024) // 4 * 4))


# rows, C, ldx, x offset (elements), with y, outputs ("f32" / "bf16" / "both"), accumulate
COLSUM_CASES = [
    (300, 768, 768, 0, False, "f32", 0),        # vector path, 75 slabs (> 16, not a multiple of 8)
    (5, 520, 528, 0, True, "both", 0),          # vector, straddles a 512-column group, ldx > C
    (1, 1032, 1040, 0, False, "bf16", 0),       # vector, one row, out_bf16 only
    (16392, 768, 776, 0, True, "both", 1),      # vector, 513 slabs of 32 rows, accumulate
    (3, 2, 2, 0, True, "f32", 0),               # scalar path: C = 2
    (16392, 266, 270, 0, False, "both", 1),     # scalar: C % 8 != 0, ldx > C, accumulate
    (300, 768, 768, 2, True, "bf16", 0),        # scalar: x (and y) 2 elements past 16-byte alignment
    (2001, 520, 520, 0, False, "f32", 1),       # vector, 501 slabs (> 16, not a multiple of 8)
]


@pytest.mark.parametrize("rows,C,ldx,off,with_y,outs,acc", COLSUM_CASES)
def test_colsum_is_exact_on_integer_data(ops, rows, C, ldx, off, with_y, outs, acc):
    """out[c] (+)= sum_r x[r][c] (* y[r][c]) on integers in [-4, 4]: every product and every partial sum is an integer below 2^24, so
    the fp32 result equals the float64 sum bit for bit (plus the pre-filled value with accumulate), out_bf16 is that sum rounded once.
    NaN in the ldx gaps, the workspace and its guard; the workspace size follows the slab rule."""
    x, y = ints(rows, C, seed=rows + C), (ints(rows, C, seed=rows + C + 1) if with_y else None)
    xs, _ = strided(rows, C, ldx, x, off=off)
    ys = strided(rows, C, ldx, y, off=off)[0] if with_y else None
    nbytes = _lib.load_library().u2tok_colsum_workspace_bytes(rows, C)
    assert nbytes == -(-rows // _slab_rows(rows, C)) * C * 4
    ws = workspace(nbytes)
    init = torch.randint(-1000, 1001, (C,), generator=torch.Generator().manual_seed(3)).float()
    out = init.to(D) if acc else nan32(C)
    outb = nan16(C + 8)
    want = (x.double() * (y.double() if with_y else 1)).sum(0) + (init.double() if acc else 0)
    call(ops, "u2tok_colsum_bf16", xs.data_ptr() + 2 * off, None if ys is None else ys.data_ptr() + 2 * off,
         out.data_ptr() if outs != "bf16" else None, outb.data_ptr() if outs != "f32" else None, rows, C, ldx, ldx, ws.data_ptr(), acc)
    assert guard_intact(ws, nbytes)
    if outs != "bf16":
        assert torch.equal(out.cpu().double(), want)
    else:
        assert torch.equal(out.cpu().view(torch.int32), torch.full((C,), NAN32, dtype=torch.int32))
    ob = outb.cpu()
    if outs != "f32":
        assert torch.equal(ob[:C], want.float().to(bf))
    else:
        assert (ob[:C].view(torch.int16) == NAN16).all()
    assert (ob[C:].view(torch.int16) == NAN16).all()


def test_colsum_random_data_bound(ops):
    """Random bf16 x, y: each product x y is exact in fp32 (8 x 8 significant bits); a sum of n terms in any order is within
    (n - 1) u sum |terms| of the exact one (first order; n u < 1e-3 here); out_bf16 adds one bf16 rounding, U |sum|."""
    rows, C = 4100, 1032
    x, y = randn(rows, C, seed=11), randn(rows, C, seed=12)
    t = x.double() * y.double()
    want, mag = t.sum(0), t.abs().sum(0)
    nbytes = _lib.load_library().u2tok_colsum_workspace_bytes(rows, C)
    ws, out, outb = workspace(nbytes), nan32(C), nan16(C)
    xd, yd = x.to(D), y.to(D)
    call(ops, "u2tok_colsum_bf16", xd.data_ptr(), yd.data_ptr(), out.data_ptr(), outb.data_ptr(), rows, C, C, C, ws.data_ptr(), 0)
    assert guard_intact(ws, nbytes)
    err = (out.cpu().double() - want).abs()
    bound = rows * u * mag
    assert (err <= bound).all(), (err / bound).max().item()
    assert ((outb.cpu().double() - want).abs() <= bound + U * want.abs() * (1 + rows * u)).all()


# ----------------------------------------------------------------------------------------------------------- layernorm_bwd
def _lnb_rows_per_wave(rows):   # csrc/backward.hip lnb_rows_per_wave
    return max(1, min(16, rows // 2048))


def _layernorm_bwd64(x, res, w, dy, eps, chunk=1024):
    """float64 dv, dw, db and the magnitudes the bounds need, in row chunks (40000 x 520 stays small)"""
    C = x.shape[1]
    dv, tol = [], []
    dw = torch.zeros(C, dtype=torch.float64)
    dwmag, dwerr = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    db = torch.zeros(C, dtype=torch.float64)
    wd = w.double()
    for r0 in range(0, x.shape[0], chunk):
        v = x[r0:r0 + chunk].double() + (res[r0:r0 + chunk].double() if res is not None else 0)
        g0 = dy[r0:r0 + chunk].double()
        mean = v.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + eps)
        xh = (v - mean) * rstd
        g = g0 * wd
        s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
        d = rstd * (g - s1 - xh * s2)
        dv.append(d)
        # fp32 error of the row's statistics, relative to their magnitudes (see the test's docstring)
        vm = v.abs().mean(1, keepdim=True)
        dxh = C * u * (1 + xh.abs()) * (1 + rstd * vm)
        tol.append(U * d.abs() + 4 * rstd * (C * u * (g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True))
                                            + s2.abs() * dxh + (g.abs() * dxh).mean(1, keepdim=True) * xh.abs()) + 4 * C * u * d.abs())
        dw += (g0 * xh).sum(0)
        dwmag += (g0 * xh).abs().sum(0)
        dwerr += (g0.abs() * dxh).sum(0)
        db += g0.sum(0)
    return torch.cat(dv), torch.cat(tol), dw, dwmag, dwerr, db


# rows, C, with residual, eps, accumulate: C tiers NC = 2 / 4 / 8 with partial and full chunk sets, 1 / 2 / 8 / 16 rows per wave,
# last workgroups partly empty (1, 3, 4095, 16392 rows)
LNB_CASES = [
    (1, 520, True, 1e-5, 0),
    (3, 1032, False, 1e-3, 1),
    (4095, 2056, True, 1e-5, 0),
    (4096, 1024, False, 1e-5, 1),
    (3, 2048, True, 1e-6, 0),
    (1, 4096, False, 1e-2, 1),
    (16392, 520, True, 1e-6, 1),
    (4096, 4096, True, 1e-5, 0),
    (40000, 520, False, 1e-5, 0),
]


@pytest.mark.parametrize("rows,C,with_res,eps,acc", LNB_CASES)
def test_layernorm_bwd_against_float64(ops, rows, C, with_res, eps, acc):
    """y = LN(v) w + b, v = x (+ res): random x, res, w (!= 1); dy integers in [-4, 4].
    db = sum_r dy: integer sums, BIT-exact (also added onto a pre-filled value with accumulate).
    dv per element: dv = rstd (g - s1 - xh s2), g = dy w, s1 = mean g, s2 = mean(g xh), xh = (v - mean v) rstd, all against float64 with
    v = x + res in float64.  The kernel's fp32 row sums (C terms each) carry errors <= C u sum |terms| (mean, variance -> rstd, s1, s2),
    so the mean is off by dm <= C u mean|v|, rstd relatively by <= C u (1 / 2 + rstd mean|v|) (the variance sums (v - mean)^2 around
    the rounded mean), and xh = (v - mean) rstd by <= C u (1 + |xh|) (1 + rstd mean|v|) =: dxh; s1 by C u mean|g|, s2 by
    C u mean|g xh| + mean(|g| dxh).  That gives tol = U |dv| (one bf16 rounding) + 4 rstd (C u (mean|g| + |xh| mean|g xh|) +
    |s2| dxh + |xh| mean(|g| dxh)) + 4 C u |dv| (rstd's error on the whole; factor 4: second-order terms and the few roundings of the
    final expression).
    dw = sum_r dy xh: each term is off by |dy| dxh + u |dy xh|, the sum of rows terms by rows u sum |dy xh|: within
    2 ((rows + 1) u sum_r |dy xh| + sum_r |dy| dxh), plus u |dw| with accumulate.
    dv is pre-filled with NaN and must be entirely written; the workspace guard must survive."""
    x, w = randn(rows, C, seed=rows + C), randn(C, scale=0.5, seed=C).float().add(1.0).to(bf)
    res = randn(rows, C, scale=0.7, seed=rows + C + 1) if with_res else None
    dy = ints(rows, C, seed=rows + C + 2)
    h = _lib.load_library()
    nbytes = h.u2tok_layernorm_bwd_workspace_bytes(rows, C)
    assert nbytes == 2 * -(-rows // (4 * _lnb_rows_per_wave(rows))) * C * 4
    ws = workspace(nbytes)
    init_w = torch.randn(C, generator=torch.Generator().manual_seed(4)).float()
    init_b = torch.randint(-1000, 1001, (C,), generator=torch.Generator().manual_seed(5)).float()
    dw, db = (init_w.to(D), init_b.to(D)) if acc else (nan32(C), nan32(C))
    dv = nan16(rows * C + 64)
    xd, wdv, dyd = x.to(D), w.to(D), dy.to(D)
    rd = res.to(D) if with_res else None
    call(ops, "u2tok_layernorm_bwd", xd.data_ptr(), None if rd is None else rd.data_ptr(), wdv.data_ptr(), dyd.data_ptr(), dv.data_ptr(),
         dw.data_ptr(), db.data_ptr(), rows, C, eps, ws.data_ptr(), acc)
    assert guard_intact(ws, nbytes)
    want_dv, tol, want_dw, dwmag, dwerr, want_db = _layernorm_bwd64(x, res, w, dy, eps)
    got = dv.cpu()
    assert (got[rows * C:].view(torch.int16) == NAN16).all()
    got = got[:rows * C].view(rows, C).double()
    assert torch.isfinite(got).all(), "rows of dv left unwritten"
    bad = (got - want_dv).abs() > tol
    assert not bad.any(), f"{bad.sum().item()} elements of dv off, rows {bad.any(1).nonzero().flatten()[:8].tolist()}"
    assert torch.equal(db.cpu().double(), want_db + (init_b.double() if acc else 0))
    want_dw = want_dw + (init_w.double() if acc else 0)
    bound = 2 * ((rows + 1) * u * dwmag + dwerr) + (u * want_dw.abs() if acc else 0) + 1e-30
    err = (dw.cpu().double() - want_dw).abs()
    assert (err <= bound).all(), (err / bound).max().item()


# ------------------------------------------------------------------------------------------------------------- softmax_bwd
@pytest.mark.parametrize("n,nrows", [(1, 7), (63, 37), (64, 4), (65, 101), (200, 50), (1025, 13)])
def test_softmax_bwd_against_float64(ops, n, nrows):
    """dS = P (dP - sum_c P dP) per row: P = softmax probabilities rounded to bf16, dP random fp32, both with NaN in their pad columns
    (ldp > n, lddp > n); dS pre-filled with NaN: columns [n, ldp) must come back as exact zeros, rows past nrows untouched.
    Bound: the fp32 dot = sum of n products P dP (each rounded: u) has error <= (n + 1) u sum|P dP|; dP - dot and the product with P
    add 2 u; the bf16 store U: |dS - ref| <= U |ref| + |P| (n + 1) u sum|P dP| + 2 u |ref| (first order; x 1.01)."""
    ldp, lddp = (n + 7) // 8 * 8 + 8, n + 3
    g = torch.Generator().manual_seed(n * 1000 + nrows)
    p = torch.softmax(torch.randn(nrows, n, generator=g) * 2, -1).to(bf)
    dp = torch.randn(nrows, n, generator=g) * 3
    ps, _ = strided(nrows, n, ldp, p)
    dps = nan32(nrows * lddp)
    dps.view(nrows, lddp)[:, :n] = dp.to(D)
    ds = nan16(nrows * ldp + 64)
    call(ops, "u2tok_softmax_bwd", ps.data_ptr(), dps.data_ptr(), ds.data_ptr(), nrows, n, ldp, lddp)
    got = ds.cpu()
    assert (got[nrows * ldp:].view(torch.int16) == NAN16).all()
    got = got[:nrows * ldp].view(nrows, ldp)
    assert (got[:, n:].view(torch.int16) == 0).all(), "pad columns of dS are not +0"
    pd, dpd = p.double(), dp.double()
    dot = (pd * dpd).sum(1, keepdim=True)
    ref = pd * (dpd - dot)
    tol = 1.01 * (U * ref.abs() + pd * (n + 1) * u * (pd * dpd).abs().sum(1, keepdim=True) + 2 * u * ref.abs())
    err = (got[:, :n].double() - ref).abs()
    assert (err <= tol).all(), (err / tol.clamp_min(1e-30)).max().item()


# ------------------------------------------------------------------------------------------------------------ relbias_grad
@pytest.mark.parametrize("S,L,H,nzh", [(1, 1, 1, 1), (2, 512, 3, 3), (2, 2, 8, 1), (37, 37, 8, 3), (37, 512, 3, 1), (37, 512, 1, 3),
                                       (512, 512, 8, 1), (512, 512, 3, 3)])
def test_relbias_grad_is_exact_on_integer_data(ops, S, L, H, nzh):
    """dtable[d + L - 1][h] += sum over z % H == h and j - i = d of dS[z][i][j]: integer dS (NaN in the pad columns, ldp > S), dtable
    pre-filled with integers: entries of diagonals |d| <= S - 1 get exactly their sum added, every other entry (|d| > S - 1, up to
    max_len - 1) stays bit-identical, and so does a guard past the table."""
    nz = H * nzh
    ldp = (S + 7) // 8 * 8 + 8
    dS = ints(nz * S, S, seed=S * 10 + H)
    st, _ = strided(nz * S, S, ldp, dS)
    init = torch.randint(-1000, 1001, ((2 * L - 1) * H,), generator=torch.Generator().manual_seed(S + H)).float()
    tbl = torch.cat([init, torch.full((64,), NAN32, dtype=torch.int32).view(torch.float32)]).to(D)
    call(ops, "u2tok_relbias_grad", st.data_ptr(), tbl.data_ptr(), nz, S, H, ldp, L)
    got = tbl.cpu()
    assert (got[init.numel():].view(torch.int32) == NAN32).all()
    got = got[:init.numel()].view(2 * L - 1, H)
    want = init.view(2 * L - 1, H).double().clone()
    x = dS.double().view(nz // H, H, S, S)
    for d in range(-(S - 1), S):
        want[d + L - 1] += torch.diagonal(x, offset=d, dim1=2, dim2=3).sum((0, 2))
    assert torch.equal(got.double(), want)
    outside = torch.ones(2 * L - 1, dtype=torch.bool)
    outside[L - S:L + S - 1] = False
    assert torch.equal(got[outside].view(torch.int32), init.view(2 * L - 1, H)[outside].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------- rowdot
@pytest.mark.parametrize("C,rows,lda,ldb", [(1, 5, 3, 1), (63, 7, 63, 71), (64, 4, 65, 64), (65, 9, 67, 73), (768, 37, 769, 776),
                                            (4097, 6, 4103, 4097)])
def test_rowdot(ops, C, rows, lda, ldb):
    """out[r] = sum_c a[r][c] b[r][c] (fp32; not called by the ops wrappers): row strides lda / ldb >= C, odd ones too, NaN in the gaps;
    out pre-filled with NaN plus a guard.  Integer data: bit-exact.  Random data: the products are exact in fp32, the sum of C of them
    is within (C - 1) u sum |a b|."""
    for integer in (True, False):
        a = ints(rows, C, seed=C) if integer else randn(rows, C, seed=C)
        b = ints(rows, C, seed=C + 1) if integer else randn(rows, C, seed=C + 1)
        ast, _ = strided(rows, C, lda, a)
        bst, _ = strided(rows, C, ldb, b)
        out = nan32(rows + 16)
        call(ops, "u2tok_rowdot_bf16", ast.data_ptr(), bst.data_ptr(), out.data_ptr(), rows, C, lda, ldb)
        got = out.cpu()
        assert (got[rows:].view(torch.int32) == NAN32).all()
        t = a.double() * b.double()
        want = t.sum(1)
        if integer:
            assert torch.equal(got[:rows].double(), want)
        else:
            assert ((got[:rows].double() - want).abs() <= C * u * t.abs().sum(1)).all()
