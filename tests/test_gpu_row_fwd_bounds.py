"""GPU: the inference path's row kernels element by element against float64 -- layernorm_bf16 (through u2tok_layernorm_rows),
softmax_rows, transpose_bf16 (csrc/rowops.hip), avgpool3d_tokens, rope_apply, embed_splice (csrc/vision.hip) and temporal_attention
(csrc/attn.hip) -- at the smallest shapes that reach every kernel instantiation and branch of their launchers: the narrow LayerNorm
tiers <2> <4> <8> <16> and the wide ones <1> <2> <4> (option ln_wide at 0 and 1), each with full and partly filled chunk sets and
batch-strided rows; the softmax vector tiers 1 / 2 / 4 / 8 and the scalar kernel (by n, by lds, past 2048), lds > n, chunks wholly
past n, the relative bias in the vector and the scalar kernel; the scalar transpose with perm16, odd strides and batch gaps; floor
pooling; rotary positions up to 511 at head dims up to 512; a second trip of every grid-stride loop (avgpool, rope, embed_splice);
the id clamp; every T of the chunk-axis attention, with and without its bias, into a padded output.

Every bound is the first-order model written out in tests/test_row_fwd_bounds_host.py (the *_model functions), which also proves on
the host that an emulation of each kernel stays inside it on exactly these cases and inputs and that a kernel wrong in one of 17
named ways does not.  Data movement (transpose, embed_splice, pooling of small integers by a power-of-two window) is bit-exact.
Every buffer a kernel writes is pre-filled with a NaN bit pattern -- leading-dimension pads, batch gaps, the elements before an
offset and a guard tail -- and compared as integers afterwards: everything outside the documented output untouched, everything
inside finite.  The first case of every kernel also runs on the f16 build.  The worst error / bound ratio per kernel goes to the
parity record under "row_fwd_error_over_bound", the module's wall time under "row_fwd_wall_s".  First measured on the MI355X:
layernorm 0.993 (ln_wide 0 and 1: 0.991 both, strided 0.98), softmax_rows 0.978 (with the bias 0.999), avgpool3d_tokens 0.996,
rope_apply 0.998 (inverse 0.999, round trip 0.988), temporal_attention 0.984; f16 0.73 / 0.93 / 0.98 / 0.88; 2 s.  A ratio just
under 1 is a correctly rounded result on the worst-placed element (see the host module's docstring), not a near miss.

Not tested: layernorm_bf16's fallback to the wave-per-row kernel for more than 262140 long rows (a 1 GB operand)."""
import time

import pytest
import torch

import test_row_fwd_bounds_host as M
from suite_budget import record
from test_gpu_backward_ops import NAN16, bf16_key, guard_intact, nan16, nan32, ops, strided  # noqa: F401
from u2tokenizer_amd import _lib

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"
GUARD = 64            # canary elements past every output

# ---- LayerNorm: C, rows, with residual (dense); C, rows of the batch-strided set (LN_NB batch entries, with a residual)
LN_WIDTHS = (8, 520, 1024, 1032, 2040, 2048, 2056, 4096, 4104, 8192)
LN_CASES = [(C, rows, res) for C in LN_WIDTHS for rows in (1, 5, 37) for res in (False, True)]
LN_STRIDED_CASES = [(C, rows) for C in (520, 2056) for rows in (1, 5)]
LN_NB = 3

# ---- softmax: n, lds, ldp at SM_NZ x SM_ROWS rows; with the bias n, lds, ldp at SM_BIAS_NZ batches of n rows over SM_H heads
SM_NZ, SM_ROWS, SM_BIAS_NZ, SM_H, SM_MAX_LEN = 3, 5, 8, 4, 512
SOFTMAX_CASES = [(40, 40, 40), (256, 256, 256), (260, 264, 264), (512, 520, 512), (516, 516, 1024), (1028, 1028, 1032),
                 (2048, 2048, 2048), (2052, 2052, 2056), (13, 13, 16), (1, 1, 8), (40, 42, 40)]
SOFTMAX_BIAS_CASES = [(40, 40, 40), (260, 260, 260), (13, 13, 16), (42, 42, 48)]

# ---- avgpool: nb, grid, window, C (floor pooling: 5 / 2, 7 / 2, 13 / 4 leave cells over)
POOL_CASES = [(2, (5, 4, 7), (2, 2, 2), 8), (2, (5, 4, 7), (2, 2, 2), 264), (2, (1, 1, 13), (1, 1, 4), 8), (2, (1, 1, 13), (1, 1, 4), 264)]
POOL_BIG = (3, (16, 16, 16), (1, 1, 2), 2048)       # 1.5 x 4096 x 256 work items

# ---- rope: n_outer, S, n_inner, H, d; the last has 2 x 8192 x 256 pairs
ROPE_CASES = [(1, 512, 2, 2, 64), (2, 16, 3, 4, 128), (1, 512, 1, 1, 512), (1, 512, 4, 8, 512)]

# ---- temporal attention: B, T, N, H, d, bias, gain of q; B N H = 6 instances leave the last workgroup half empty
TA_CASES = ([(1, T, 3, 2, 64, T % 2 == 0, 1) for T in range(16, 0, -1)] +
            [(1, T, 3, 2, d, bias, 1) for T in (16, 5) for d in (128, 256, 512) for bias in (True, False)] +
            [(1, 16, 3, 2, 64, True, 8)])

_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.monotonic()
    yield
    record("row_fwd_wall_s", round(time.monotonic() - t, 1))
    print(f"\ntests/test_gpu_row_fwd_bounds.py: {time.monotonic() - t:.1f} s; error / bound: {_RATIOS}")


def call(ops, name, *args, status=0, el=M.BF16):
    """u2tok_<name>(*args, stream) of the build for `el` on the stream and context the ops wrappers use; returns after the stream drained"""
    anchor = torch.empty(1, dtype=el.dtype, device=D)
    with ops.on_device(anchor, el.dtype) as (h, st):
        got = getattr(h, name)(*args, st)
    torch.cuda.synchronize()
    assert got == status, (name, got, _lib.ERRORS.get(got, got))


def hold(name, got, ref, bound):
    """every element of got finite and within bound of ref; the worst ratio is printed and recorded before it is asserted"""
    err = (got.detach().double().cpu() - ref).abs()
    assert torch.isfinite(err).all(), f"{name}: non-finite elements (left unwritten, or a pad was read?)"
    r = M.worst(err, bound)
    _RATIOS[name] = round(max(_RATIOS.get(name, 0.0), r), 4)
    record("row_fwd_error_over_bound", _RATIOS)
    print(f"{name}: error / bound = {r:.3f}")
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst ratio {r:.3f}; first at {i}: "
                             f"got {got[i].item()}, want {ref[i].item()} +- {bound[i].item()}")
    return r


def tag(el):
    return "" if el is M.BF16 else el.name + " "


def canary(n, el=M.BF16):
    return nan16(n).view(torch.int16).view(el.dtype)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def place(src, idx, total, el=M.BF16):
    """canary storage of `total` elements holding src at the flat indices idx"""
    st = canary(total, el)
    st[idx.to(D)] = src.to(D)
    return st


def only_wrote(st, idx):
    """the canary is intact everywhere outside the flat indices idx"""
    out = torch.ones(st.numel(), dtype=torch.bool, device=D)
    out[idx.reshape(-1).to(D)] = False
    return bool((bits(st)[out] == NAN16).all())


def index3(off, nb, rows, C, bs, ld):
    """flat indices (nb, rows, C) of rows r of batch entries b at off + b bs + r ld"""
    return off + torch.arange(nb)[:, None, None] * bs + torch.arange(rows)[None, :, None] * ld + torch.arange(C)[None, None, :]


def total_of(idx):
    return int(idx.max()) + 1 + GUARD


# -------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_call(ops, inp, nb, rows, C, xi, ri, yi, strides, el=M.BF16, status=0):
    """x / res / y at the flat indices xi / ri / yi of canary storages; -> (y storage, y as (nb, rows, C))"""
    x = place(inp["x"], xi, total_of(xi), el)
    r = None if inp["res"] is None else place(inp["res"], ri, total_of(ri), el)
    y = canary(total_of(yi), el)
    w, b = inp["w"].to(D), inp["b"].to(D)
    es = 2
    call(ops, "u2tok_layernorm_rows", x.data_ptr() + es * int(xi.min()), None if r is None else r.data_ptr() + es * int(ri.min()),
         w.data_ptr(), b.data_ptr(), y.data_ptr() + es * int(yi.min()), nb, rows, C, *strides, inp["eps"], status=status, el=el)
    return y, y[yi.to(D)]


def _ln_dense(ops, C, rows, with_res, el=M.BF16):
    inp = M.ln_inputs(1, rows, C, with_res, el)
    i = index3(8, 1, rows, C, rows * C, C)
    y, got = _ln_call(ops, inp, 1, rows, C, i, i, i, (rows * C, C, rows * C, C, rows * C, C), el)
    assert only_wrote(y, i), "layernorm wrote outside its rows"
    return inp, got


def _ln_hold(name, inp, got, el=M.BF16):
    m = M.ln_model(**inp, el=el)
    hold(name, got, m["y"], m["bound"])
    if got.shape[1] >= 5:       # the constant row: every partial sum is exact, the output is the bias bit for bit
        assert torch.equal(got[:, 2].cpu(), inp["b"].expand(got.shape[0], -1)), "constant row"


@pytest.mark.parametrize("C", LN_WIDTHS)
def test_layernorm_bounds_at_every_tier(ops, C):
    """y within ln_model's bound: U |y| + |w| rstd (dd + |d| (e_r + 2 u)) + u (|t| + |b|), one rounding and the two-pass fp32
    statistics.  rows 1 / 5 / 37, with and without a residual; from C = 2048 up with option ln_wide at 1 (layernorm_wide_kernel
    <1> <2> <4>) and at 0 (layernorm_kernel <4> <8> <16>): each inside its bound, which makes them agree within the two bounds' sum."""
    first = {}
    try:
        for wide in ((1, 0) if C >= 2048 else (1,)):
            ops.set_option("ln_wide", wide)
            for rows in (1, 5, 37):
                for with_res in (False, True):
                    assert (C, rows, with_res) in LN_CASES
                    inp, got = _ln_dense(ops, C, rows, with_res)
                    _ln_hold(f"layernorm ln_wide={wide}" if C >= 2048 else "layernorm", inp, got)
                    other = first.setdefault((rows, with_res), got)
                    assert ((got.double() - other.double()).abs().cpu() <= 2 * M.ln_model(**inp)["bound"]).all(), "the two kernels disagree"
    finally:
        ops.set_option("ln_wide", 1)


@pytest.mark.parametrize("C,rows", LN_STRIDED_CASES)
def test_layernorm_batch_strided_rows(ops, C, rows):
    """LN_NB batch entries at x_ld = C + 8, y_ld = C + 16, res_ld = C + 24 and batch strides with gaps, 8 elements into each storage:
    pads, gaps, the leading elements and the tail keep their canary (an input pad that is read turns the row NaN).  Then the ViT's
    final norm as pipeline.hip issues it: patch rows of every chunk into out + C at batch stride (ntok + 1) C, then one cls row per
    chunk (rows = 1, x_bs = C) into out, res = NULL with res_bs = res_ld = 0: together they fill out exactly."""
    nb = LN_NB
    try:
        for wide in ((1, 0) if C >= 2048 else (1,)):
            ops.set_option("ln_wide", wide)
            inp = M.ln_inputs(nb, rows, C, True)
            x_ld, y_ld, r_ld = C + 8, C + 16, C + 24
            x_bs, y_bs, r_bs = rows * x_ld + 24, rows * y_ld + 40, rows * r_ld + 8
            xi, ri, yi = index3(8, nb, rows, C, x_bs, x_ld), index3(16, nb, rows, C, r_bs, r_ld), index3(8, nb, rows, C, y_bs, y_ld)
            y, got = _ln_call(ops, inp, nb, rows, C, xi, ri, yi, (x_bs, x_ld, r_bs, r_ld, y_bs, y_ld))
            assert only_wrote(y, yi), "layernorm wrote outside its rows"
            _ln_hold(f"layernorm strided ln_wide={wide}", inp, got)
            # the ViT's final norm: x = [nb x ntok patch rows | nb cls rows], out = nb x [cls | patches]
            ntok = rows
            vin = M.ln_inputs(1, nb * (ntok + 1), C, False)
            x = vin["x"][0].to(D)
            out = canary(nb * (ntok + 1) * C + GUARD)
            w, b = vin["w"].to(D), vin["b"].to(D)
            call(ops, "u2tok_layernorm_rows", x.data_ptr(), None, w.data_ptr(), b.data_ptr(), out.data_ptr() + 2 * C, nb, ntok, C,
                 ntok * C, C, 0, 0, (ntok + 1) * C, C, vin["eps"])
            cls_slots = index3(0, nb, 1, C, (ntok + 1) * C, C)
            assert (bits(out)[cls_slots.reshape(-1).to(D)] == bits(canary(1))[0]).all(), "the patch-row call wrote a cls slot"
            call(ops, "u2tok_layernorm_rows", x.data_ptr() + 2 * nb * ntok * C, None, w.data_ptr(), b.data_ptr(), out.data_ptr(), nb, 1,
                 C, C, C, 0, 0, (ntok + 1) * C, C, vin["eps"])
            assert (bits(out[nb * (ntok + 1) * C:]) == bits(canary(1))[0]).all()
            m = M.ln_model(**vin)
            want = torch.cat([m["y"][0, nb * ntok:].view(nb, 1, C), m["y"][0, :nb * ntok].view(nb, ntok, C)], 1)
            bound = torch.cat([m["bound"][0, nb * ntok:].view(nb, 1, C), m["bound"][0, :nb * ntok].view(nb, ntok, C)], 1)
            hold(f"layernorm strided ln_wide={wide}", out[:nb * (ntok + 1) * C].view(nb, ntok + 1, C), want, bound)
    finally:
        ops.set_option("ln_wide", 1)


def test_layernorm_refusals_leave_the_output_alone(ops):
    """C = 8200 (> 8192), C % 8 != 0, a stride that is no multiple of 8 and a pointer 2 bytes off 16-byte alignment: U2TOK_ERR_ARG"""
    buf = torch.zeros(4 * 8200 + 64, dtype=bf, device=D)
    y = canary(8200 + 64)
    p, q = buf.data_ptr(), y.data_ptr()

    def refuse(x=p, w=p + 2 * 8200, b=p + 4 * 8200, out=q, C=8, ld=8):
        call(ops, "u2tok_layernorm_rows", x, None, w, b, out, 1, 1, C, ld, ld, 0, 0, ld, ld, 1e-5, status=-1)

    refuse(C=8200, ld=8200)
    refuse(C=12, ld=16)
    refuse(C=8, ld=12)
    for k in ("x", "w", "b", "out"):
        refuse(**{k: {"x": p, "w": p + 2 * 8200, "b": p + 4 * 8200, "out": q}[k] + 2})
    call(ops, "u2tok_layernorm_rows", p, p + 6 * 8200 + 2, p + 2 * 8200, p + 4 * 8200, q, 1, 1, 8, 8, 8, 8, 8, 8, 8, 1e-5, status=-1)
    assert (bits(y) == bits(canary(1))[0]).all()
    call(ops, "u2tok_layernorm_rows", p, None, p + 2 * 8200, p + 4 * 8200, q, 1, 1, 8, 8, 8, 0, 0, 8, 8, 1e-5)       # the same call, aligned
    assert (bits(y[8:]) == bits(canary(1))[0]).all() and torch.isfinite(y[:8].float()).all()


# ---------------------------------------------------------------------------------------------------------------- softmax
def _softmax_run(ops, nz, rows, n, lds, ldp, H, el=M.BF16):
    inp = M.softmax_inputs(nz, rows, n, lds, H, SM_MAX_LEN, el)
    m = M.softmax_model(**inp, el=el)
    S = inp["S"].to(D)
    P = canary(nz * rows * ldp + GUARD, el)
    tbl = None if inp["tbl"] is None else inp["tbl"].to(D)
    call(ops, "u2tok_softmax_rows", S.data_ptr(), P.data_ptr(), nz, rows, n, lds, ldp, inp["scale"],
         None if tbl is None else tbl.data_ptr(), H, SM_MAX_LEN if H else 0, el=el)
    assert (bits(P[nz * rows * ldp:]) == bits(canary(1))[0]).all(), "softmax wrote past its last row"
    got = P[:nz * rows * ldp].view(nz, rows, ldp)
    assert (bits(got[..., n:]) == 0).all(), "the columns [n, ldp) are exact zeros"
    hold(tag(el) + "softmax_rows" + (" + bias" if H else ""), got[..., :n], m["P"], m["bound"])
    return got, m


@pytest.mark.parametrize("n,lds,ldp", SOFTMAX_CASES)
def test_softmax_bounds_at_every_tier(ops, n, lds, ldp):
    """P within softmax_model's bound (U P + P e(P)) at 3 x 5 rows (a ragged last workgroup), scale 0.7; S is handed over with its
    columns [n, lds) full of other data; the columns [n, ldp) of P come back as exact zeros and nothing past the last row is written.
    One row is decided by a single entry 60 above the rest; a constant row comes back as fl(1 / n) in every column."""
    got, _ = _softmax_run(ops, SM_NZ, SM_ROWS, n, lds, ldp, 0)
    if n > 1:
        assert got[0, 1, (n * 2) // 3].item() == 1.0
    inv = (torch.tensor(1.0) / torch.tensor(float(n))).to(bf)
    assert (got[1, 2, :n].cpu() == inv).all()


@pytest.mark.parametrize("n,lds,ldp", SOFTMAX_BIAS_CASES)
def test_softmax_relative_bias_bounds(ops, n, lds, ldp):
    """the Toeplitz bias tbl[c - r + max_len - 1][z % H] in the vector kernel's tiers 1 and 2 and in the scalar kernel (n % 4, lds % 4),
    8 batches over 4 heads, rows = n so that every diagonal is read; head 1 carries a bias of 96 on one diagonal"""
    _softmax_run(ops, SM_BIAS_NZ, n, n, lds, ldp, SM_H)


# -------------------------------------------------------------------------------------------------------------- transpose
_PERM16 = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]


# Z, R, C, ld_in, ld_out, gap of in_zs, gap of out_zs, perm16
@pytest.mark.parametrize("Z,R,C,ld_in,ld_out,gin,gout,perm16", [
    (2, 70, 130, 130, 80, 0, 0, 1),      # scalar kernel (C % 4), perm16, three column tiles, two row tiles
    (2, 65, 132, 134, 72, 0, 0, 0),      # scalar by ld_in % 4; R one past a tile
    (2, 65, 63, 63, 65, 3, 5, 0),        # scalar: C one short of a tile, odd strides and gaps
    (2, 65, 63, 65, 80, 1, 16, 1),       # scalar, perm16, R one past a tile into a second, partly filled group of 16
    (3, 65, 64, 72, 80, 8, 16, 0),       # vector kernel with batch gaps and ld_in > C
    (3, 65, 60, 64, 80, 8, 16, 1)])      # vector kernel, perm16, batch gaps
def test_transpose_is_bit_exact_with_strides_and_gaps(ops, Z, R, C, ld_in, ld_out, gin, gout, perm16):
    """out[z][c][r] = in[z][r][c] bit for bit, the columns [R, ld_out) zero, perm16 inside every group of 16 output columns; the pads
    of the input rows, the gaps between batch entries on both sides and the tail keep their canary"""
    x = torch.randn(Z, R, C, generator=M._gen(16, Z, R, C)).to(bf)
    in_zs, out_zs = R * ld_in + gin, C * ld_out + gout
    xi = index3(0, Z, R, C, in_zs, ld_in)
    oi = index3(0, Z, C, ld_out, out_zs, ld_out)
    xs = place(x, xi, total_of(xi))
    out = canary(total_of(oi))
    call(ops, "u2tok_transpose_bf16", xs.data_ptr(), out.data_ptr(), Z, R, C, ld_in, ld_out, in_zs, out_zs, perm16)
    assert only_wrote(out, oi), "transpose wrote into a gap"
    want = torch.zeros(Z, C, ld_out, dtype=bf)
    want[:, :, :R] = x.transpose(1, 2)
    if perm16:
        want = want[:, :, [16 * (j // 16) + _PERM16[j % 16] for j in range(ld_out)]]
    assert torch.equal(bits(out[oi.to(D)]).cpu(), bits(want))


# ---------------------------------------------------------------------------------------------------------------- avgpool
def _pool_run(ops, x, nb, grid, window, C, el=M.BF16):
    n_out = (grid[0] // window[0]) * (grid[1] // window[1]) * (grid[2] // window[2])
    xd = x.to(D)
    y = canary(nb * n_out * C + GUARD, el)
    call(ops, "u2tok_avgpool3d_tokens", xd.data_ptr(), y.data_ptr(), nb, *grid, *window, C, el=el)
    assert (bits(y[nb * n_out * C:]) == bits(canary(1))[0]).all(), "avgpool wrote past its output"
    return y[:nb * n_out * C].view(nb, n_out, C)


@pytest.mark.parametrize("nb,grid,window,C", POOL_CASES)
def test_avgpool_floor_semantics_and_bound(ops, nb, grid, window, C):
    """against F.avg_pool3d in float64 where trailing cells fill no window (5 / 2, 7 / 2, 13 / 4), within U |y| + (W + 2) u mean|x|"""
    inp = M.pool_inputs(nb, grid, C)
    m = M.pool_model(inp["x"], grid, window)
    hold("avgpool3d_tokens", _pool_run(ops, inp["x"], nb, grid, window, C), m["y"], m["bound"])


@pytest.mark.parametrize("nb,grid,window,C", [(2, (5, 4, 7), (2, 2, 2), 264), (2, (1, 1, 13), (1, 1, 4), 8), POOL_BIG])
def test_avgpool_of_small_integers_is_the_mean_rounded_once(ops, nb, grid, window, C):
    """integers in [-4, 4] and a power-of-two window: every fp32 sum and the product with 1 / W are exact, so the output is the
    float64 mean rounded once, bit for bit.  The last case has 1.5 x 4096 x 256 work items: every thread of the capped grid takes a
    second trip of the grid-stride loop, half of them."""
    x = M.pool_inputs(nb, grid, C, integer=True)["x"]
    want = M._pool(x.float(), grid, window).to(bf)        # exact in fp32 as well: |sum| <= 32, a dyadic mean
    assert torch.equal(bits(_pool_run(ops, x, nb, grid, window, C)).cpu(), bits(want))


# ------------------------------------------------------------------------------------------------------------------- RoPE
def _rope_run(ops, x, no, S, ni, H, d, inverse, el=M.BF16, max_len=512, status=0):
    """x (no, S, ni, H d) in place on columns [8, 8 + H d) of a canary storage of row stride H d + 16"""
    rows, ld = no * S * ni, H * d + 16
    xi = index3(8, 1, rows, H * d, 0, ld)[0]
    st = place(x.reshape(rows, H * d), xi, rows * ld + GUARD, el)
    call(ops, "u2tok_rope_apply", st.data_ptr() + 16, no, S, ni, H, d, ld, max_len, int(inverse), status=status, el=el)
    assert only_wrote(st, xi), "rope touched the neighbouring columns"
    return st[xi.to(D)].view(no, S, ni, H * d)


def _rope_check(ops, no, S, ni, H, d, el=M.BF16):
    x = M.rope_inputs(no, S, ni, H, d, el)["x"]
    fwd, inv = M.rope_model(x, H, d, False, el), M.rope_model(x, H, d, True, el)
    y = _rope_run(ops, x, no, S, ni, H, d, False, el)
    hold("rope_apply", y, fwd["out"], fwd["bound"])
    hold("rope_apply inverse", _rope_run(ops, x, no, S, ni, H, d, True, el), inv["out"], inv["bound"])
    return x, y.cpu(), fwd


@pytest.mark.parametrize("no,S,ni,H,d", ROPE_CASES)
def test_rope_bounds_at_pipeline_positions(ops, no, S, ni, H, d):
    """positions up to 511 at head dims 64 / 128 / 512, forward and inverse, within rope_model's bound (U |out| + 2 u (|a c| + |b s|)
    + one ulp of a near-tie table entry times its operand; at most 3 % of the entries are near ties).  The inverse applied to the
    forward's output is held to the inverse's bound for that input, and returns x within the forward's bound carried through the
    inverse rotation (|c| bound_a + |s| bound_b) + the inverse's bound + |c^2 + s^2 - 1| |x|: the rounded table is not quite a
    rotation (c^2 + s^2 is off by up to U), which the sum of the two bounds alone does not cover.  The last case has 2 x 8192 x 256
    pairs: every thread of the capped grid takes two trips."""
    x, y, fwd = _rope_check(ops, no, S, ni, H, d)
    back = _rope_run(ops, y, no, S, ni, H, d, True)
    inv_y = M.rope_model(y, H, d, True)
    hold("rope_apply inverse", back, inv_y["out"], inv_y["bound"])
    c32, s32, _ = M.rope_table(S, d)
    c, s = M.BF16.rnd(c32), M.BF16.rnd(s32)
    _, carried = M._rotate(fwd["bound"], c, s, H, d, 1.0)
    norm = (c * c + s * s - 1).abs()
    _, off = M._rotate(x.double(), norm, torch.zeros_like(norm), H, d, 1.0)
    hold("rope_apply round trip", back, x.double(), carried + inv_y["bound"] + off)


def test_rope_refuses_positions_past_the_table(ops):
    x = M.rope_inputs(1, 16, 1, 1, 64)["x"]
    got = _rope_run(ops, x, 1, 16, 1, 1, 64, False, max_len=15, status=-1)
    assert torch.equal(bits(got).cpu(), bits(x))


# ----------------------------------------------------------------------------------------------------------- embed_splice
def _splice_run(ops, table, ids, feats, B, S, E, nfeat, vocab):
    out = canary(B * S * E + GUARD)
    call(ops, "u2tok_embed_splice", table.data_ptr(), ids.data_ptr(), None if feats is None else feats.data_ptr(), out.data_ptr(),
         B, S, E, nfeat, vocab)
    assert (bits(out[B * S * E:]) == bits(canary(1))[0]).all(), "embed_splice wrote past its output"
    return out[:B * S * E].view(B, S, E)


@pytest.mark.parametrize("B,S,E,nfeat,vocab", [(2, 9, 64, 8, 50), (2, 9, 64, 0, 50), (2, 9, 64, 3, 50), (4, 1100, 4096, 600, 50)])
def test_embed_splice_is_bit_exact(ops, B, S, E, nfeat, vocab):
    """out[b][s] = feats[b][s - 1] for 1 <= s <= nfeat, else table[clamp(ids[b][s])]: nfeat = S - 1, nfeat = 0 with feats = NULL, ids
    -1 and vocab clamped to the rows 0 and vocab - 1 (include/u2tok.h), and 4 x 1100 x 4096 / 8 = 1.07 x 8192 x 256 work items"""
    g = M._gen(17, B, S, E, nfeat)
    table = torch.randn(vocab, E, generator=g).to(bf)
    ids = torch.randint(0, vocab, (B, S), generator=g)
    ids[0, 0], ids[-1, -1], ids[0, -1] = -1, vocab, vocab + 7
    feats = torch.randn(B, nfeat, E, generator=g).to(bf) if nfeat else None
    want = table[ids.clamp(0, vocab - 1)]
    if nfeat:
        want[:, 1:nfeat + 1] = feats
    got = _splice_run(ops, table.to(D), ids.to(D), None if feats is None else feats.to(D), B, S, E, nfeat, vocab)
    assert torch.equal(bits(got).cpu(), bits(want))


# ----------------------------------------------------------------------------------------------------- temporal attention
def _ta_run(ops, inp, B, T, N, H, d, el=M.BF16, status=0):
    """q | k | v as column slices of one (rows, 3 E + 8) storage whose pad is canary, out at ld_out = E + 8 into canary"""
    rows, E = B * T * N, H * d
    qi = index3(0, 1, rows, 3 * E, 0, 3 * E + 8)[0]
    qkv = place(inp["qkv"], qi, rows * (3 * E + 8) + GUARD, el)
    oi = index3(0, 1, rows, E, 0, E + 8)[0]
    out = canary(rows * (E + 8) + GUARD, el)
    tbl = None if inp["tbl"] is None else inp["tbl"].to(D)
    p = qkv.data_ptr()
    call(ops, "u2tok_temporal_attention", p, p + 2 * E, p + 4 * E, out.data_ptr(), B, T, N, H, d, 3 * E + 8, E + 8, inp["scale"],
         None if tbl is None else tbl.data_ptr(), inp["max_len"], status=status, el=el)
    assert only_wrote(out, oi) or status != 0, "temporal attention wrote into the pad of its output"
    return out, out[oi.to(D)]


def _ta_check(ops, case, el=M.BF16):
    B, T, N, H, d, bias, gain = case
    inp = M.ta_inputs(B, T, N, H, d, bias, gain, el=el)
    m = M.ta_model(**inp, B=B, T=T, N=N, H=H, d=d, el=el)
    _, got = _ta_run(ops, inp, B, T, N, H, d, el)
    hold(tag(el) + "temporal_attention", got, m["out"], m["bound"])


@pytest.mark.parametrize("T", range(1, 17))
def test_temporal_attention_bounds_at_every_T(ops, T):
    """every T at d = 64 (bias on the even ones), and the score spread by a gain of 8 at T = 16: out within ta_model's bound
    (U |out| + sum_j P_j (e(P_j) + (T + 1) u) |v_j|: P stays in fp32); 6 instances leave two waves of the last workgroup idle"""
    for case in TA_CASES:
        if case[1] == T and case[4] == 64:
            _ta_check(ops, case)


@pytest.mark.parametrize("d", [128, 256, 512])
def test_temporal_attention_bounds_at_every_head_dim(ops, d):
    """T = 16 and T = 5 at d = 128 / 256 / 512, each with and without the relative bias (d = 384: tests/test_gpu_tok_attn_d384.py)"""
    n = 0
    for case in TA_CASES:
        if case[4] == d:
            _ta_check(ops, case)
            n += 1
    assert n == 4


def test_temporal_attention_refuses_T17(ops):
    inp = M.ta_inputs(1, 17, 3, 2, 64, True)
    out, _ = _ta_run(ops, inp, 1, 17, 3, 2, 64, status=-1)
    assert (bits(out) == bits(canary(1))[0]).all()


# ------------------------------------------------------------------------------------------------------------- f16 build
def test_first_case_of_every_kernel_on_the_f16_build(ops):
    """the same kernels compiled for IEEE half (U = 2^-11; probabilities below 2^-14 are subnormal, below 2^-25 zero: `tiny`).
    Without rope_apply: in f16 6 to 13 % of the rotary table are near ties at every case, over the model's cap of 3 %
    (tests/test_row_fwd_bounds_host.py, test_rope_near_tie_share_is_under_its_cap)."""
    el = M.F16
    C, rows, with_res = LN_CASES[0]
    inp, got = _ln_dense(ops, C, rows, with_res, el)
    m = M.ln_model(**inp, el=el)
    hold("f16 layernorm", got, m["y"], m["bound"])
    n, lds, ldp = SOFTMAX_CASES[0]
    _softmax_run(ops, SM_NZ, SM_ROWS, n, lds, ldp, 0, el)
    nb, grid, window, C = POOL_CASES[0]
    x = M.pool_inputs(nb, grid, C, el=el)["x"]
    m = M.pool_model(x, grid, window, el)
    hold("f16 avgpool3d_tokens", _pool_run(ops, x, nb, grid, window, C, el), m["y"], m["bound"])
    _ta_check(ops, TA_CASES[0], el)
