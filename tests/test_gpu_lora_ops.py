"""GPU: the rank-r adapter kernels (u2tok_lora_down, u2tok_lora_up, u2tok_lora_wgrad; csrc/lora.hip) element by element against
float64, with the first-order bounds of tests/test_lora_bounds_host.py (which proves on the host that an emulation of the kernels'
rounding points stays inside them on exactly these cases and inputs).  Row counts on and next to the 16-row MFMA tile and the
128-row staging tile, contractions of one 32-wide step up to every slice count, column counts that leave partial 64-column units
and strips, all three ranks, alpha != 1, operands as column segments of wider buffers (padded row stride, non-zero offset).
Buffers the kernels write are pre-filled with a NaN bit pattern, pads and guard tails included, and compared as integers
afterwards.  The worst error / bound ratio per kernel goes to the parity record under "lora_ops_error_over_bound"."""
import time

import pytest
import torch

import test_lora_bounds_host as B
from suite_budget import record
from test_decoder_train_bounds_host import worst
from test_gpu_backward_ops import NAN16, NAN32, call, guard_intact, nan16, nan32, ops, workspace  # noqa: F401

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"

_MS = (1, 15, 16, 17, 63, 64, 65, 257)
_KS, _RS, _NS = (32, 64, 1056, 4096), (16, 32, 64), (16, 48, 528)


def _full_or_diagonal(ms, *axes):
    """the first and last m take every combination of the axes, the others one combination each, walking the axes' diagonals"""
    import itertools
    out = []
    for i, m in enumerate(ms):
        if i in (0, len(ms) - 1):
            out += [(m, *c) for c in itertools.product(*axes)]
        else:
            out.append((m, *(a[(i + j) % len(a)] for j, a in enumerate(axes))))
    return out


DOWN_CASES = _full_or_diagonal(_MS, _KS, _RS)                                                    # M, K, r
UP_CASES = [(m, n, r, acc) for m, n, r in _full_or_diagonal(_MS, _NS, _RS) for acc in (0, 1)]    # M, N, r, accumulate
WGRAD_CASES = [(m, c, _RS[(i + j) % 3], f32) for i, m in enumerate((1, 31, 32, 33, 257, 1100))   # M (contraction rows), C, r, fp32 out
               for j, c in enumerate((8, 72, 4096)) for f32 in (0, 1)]
F16_DOWN, F16_UP, F16_WGRAD = (65, 1056, 32), (65, 528, 16, 1), (257, 72, 64, 0)

_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.monotonic()
    yield
    print(f"\ntests/test_gpu_lora_ops.py: {time.monotonic() - t:.1f} s; error / bound: {_RATIOS}")


def hold(name, got, ref, bound):
    """every element of got within bound of ref; the worst ratio is printed and recorded before it is asserted"""
    err = (got.detach().double().cpu() - ref).abs()
    assert torch.isfinite(err).all(), f"{name}: non-finite elements (left unwritten?)"
    r = worst(err, bound)
    _RATIOS[name] = round(max(_RATIOS.get(name, 0.0), r), 4)
    record("lora_ops_error_over_bound", _RATIOS)
    print(f"{name}: error / bound = {r:.3f}")
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst ratio {r:.3f}; first at {i}: "
                             f"got {got[i].item()}, want {ref[i].item()} +- {bound[i].item()}")


def fill16(n, dtype=bf):
    return torch.full((n,), NAN16, dtype=torch.int16, device=D).view(dtype)


def is_nan16(t):
    return bool((t.contiguous().view(torch.int16) == NAN16).all())


def is_nan32(t):
    return bool((t.contiguous().view(torch.int32) == NAN32).all())


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def segment(src, off, pad, dtype=bf):
    """(storage, view): src (rows, C) as columns [off, off + C) of a NaN-filled (rows, off + C + pad) buffer with a NaN guard tail"""
    rows, C = src.shape
    ld = off + C + pad
    st = fill16(rows * ld + 64, dtype)
    view = st[:rows * ld].view(rows, ld)[:, off:off + C]
    view.copy_(src.to(D))
    return st, view


def outside_is_nan(st, rows, ld, off, C):
    """every element of the storage outside columns [off, off + C) of its rows, the guard tail included, still holds the fill"""
    body = st[:rows * ld].view(rows, ld)
    return is_nan16(body[:, :off]) and is_nan16(body[:, off + C:]) and is_nan16(st[rows * ld:])


# ------------------------------------------------------------------------------------------------------------------- down
@pytest.mark.parametrize("M,K,r", DOWN_CASES)
def test_lora_down_bounds(ops, M, K, r):
    """U = alpha X A^T per element within U |ref| + K u sum |alpha x a|; X a column segment (offset 8 or 24, padded stride) of a
    NaN-filled buffer, U written into a NaN-filled buffer with a padded row stride whose pads and tail stay NaN; two calls bit-equal."""
    inp = B.down_inputs(M, K, r)
    m = B.down_model(**inp)
    off = 8 if M % 2 else 24
    stx, x = segment(inp["x"], off, 8)
    a = inp["a"].to(D)

    def run():
        st = fill16(M * (r + 8) + 64)
        out = st[:M * (r + 8)].view(M, r + 8)[:, :r]
        with torch.no_grad():
            ops.lora_down(x, a, alpha=inp["alpha"], out=out)
        torch.cuda.synchronize()
        assert outside_is_nan(st, M, r + 8, 0, r)
        return out

    got = run()
    hold("lora_down", got, m["out"], m["bound"])
    assert torch.equal(bits(got), bits(run()))
    direct = fill16(M * r)      # the C ABI with the buffer's base address and the segment's element offset: the same bits
    call(ops, "u2tok_lora_down", stx.data_ptr(), off, x.stride(0), a.data_ptr(), K, direct.data_ptr(), r, M, K, r, inp["alpha"])
    assert torch.equal(bits(direct.view(M, r)), bits(got))


# --------------------------------------------------------------------------------------------------------------------- up
@pytest.mark.parametrize("M,N,r,accumulate", UP_CASES)
def test_lora_up_bounds(ops, M, N, r, accumulate):
    """Y = [Y +] alpha U W^T per element within U |ref| + (r + 2) u (|y| + |alpha| sum |u w|); Y is a column segment of a wider
    buffer whose other columns stay NaN (accumulate = 0: the segment itself is NaN before the call and never read)."""
    inp = B.up_inputs(M, N, r)
    m = B.up_model(accumulate=accumulate, **inp)
    uu, w = inp["uu"].to(D), inp["w"].to(D)
    off, pad = (16, 8) if M % 2 else (40, 24)

    def run():
        st, y = segment(inp["y"], off, pad)
        if not accumulate:
            y.copy_(fill16(M * N).view(M, N))
        with torch.no_grad():
            ops.lora_up(uu, w, y, alpha=inp["alpha"], accumulate=bool(accumulate))
        torch.cuda.synchronize()
        assert outside_is_nan(st, M, off + N + pad, off, N)
        return y

    got = run()
    hold(f"lora_up accumulate={accumulate}", got, m["out"], m["bound"])
    assert torch.equal(bits(got), bits(run()))
    st, y = segment(inp["y"], off, pad)   # the C ABI with the buffer's base address and the segment's element offset: the same bits
    call(ops, "u2tok_lora_up", uu.data_ptr(), r, w.data_ptr(), r, st.data_ptr(), off, y.stride(0), M, N, r, inp["alpha"], accumulate)
    assert outside_is_nan(st, M, off + N + pad, off, N) and torch.equal(bits(y), bits(got))


# ------------------------------------------------------------------------------------------------------------------ wgrad
@pytest.mark.parametrize("M,C,r,out_f32", WGRAD_CASES)
def test_lora_wgrad_bounds(ops, M, C, r, out_f32):
    """G = alpha U^T X per element within [U |ref| +] M u sum |alpha u x|; X a column segment, G a NaN-filled buffer with a padded
    row stride and a guard tail; with the wrapper's workspace (row ranges across workgroups) and without one (a direct C-ABI call: one
    workgroup per 64-column strip) -- each bit-repeatable, both inside the bound."""
    inp = B.wgrad_inputs(M, C, r)
    m = B.wgrad_model(out_f32=out_f32, **inp)
    stx, x = segment(inp["x"], 8, 16)
    uu = inp["uu"].to(D)
    ld = C + 8

    def buf():
        return nan32(r * ld + 16) if out_f32 else fill16(r * ld + 16)

    def view(st):
        body = st[:r * ld].view(r, ld)
        check = is_nan32 if out_f32 else is_nan16
        assert check(body[:, C:]) and check(st[r * ld:])
        return body[:, :C]

    def run():
        st = buf()
        with torch.no_grad():
            ops.lora_wgrad(uu, x, alpha=inp["alpha"], out_f32=bool(out_f32), out=st[:r * ld].view(r, ld)[:, :C])
        torch.cuda.synchronize()
        return view(st)

    def run_direct(ws_bytes):
        st = buf()
        ws = workspace(ws_bytes) if ws_bytes else None
        call(ops, "u2tok_lora_wgrad", uu.data_ptr(), r, stx.data_ptr(), 8, x.stride(0), st.data_ptr(), ld, M, C, r, inp["alpha"], out_f32,
             None if ws is None else ws.data_ptr(), ws_bytes)
        assert ws is None or guard_intact(ws, ws_bytes)
        return view(st)

    got = run()
    hold(f"lora_wgrad out_f32={out_f32}", got, m["out"], m["bound"])
    assert torch.equal(bits(got), bits(run()))
    one = run_direct(0)
    hold(f"lora_wgrad out_f32={out_f32}, no workspace", one, m["out"], m["bound"])
    assert torch.equal(bits(one), bits(run_direct(0)))
    nb = ops.lora_wgrad_workspace_bytes(M, C, r)
    if nb:   # the wrapper's workspace, with a guard behind it: the same bits as the wrapper's call
        assert torch.equal(bits(run_direct(nb)), bits(got))


# ------------------------------------------------------------------------------------------------------ arguments, f16
def test_arguments_outside_the_contract_are_refused(ops):
    """U2TOK_ERR_ARG before any launch: r = 8, K = 40 (down), N = 24 (up), C = 12 (wgrad), misaligned offsets and leading dimensions,
    null pointers; the outputs stay untouched"""
    x, a, uu = fill16(64 * 64).view(64, 64), fill16(64 * 64).view(64, 64), fill16(64 * 64).view(64, 64)
    P = x.data_ptr()

    def down(M=16, K=64, r=16, x_off=0, ldx=64, lda=64, ldu=64, X=P, A=a.data_ptr(), U=uu.data_ptr()):
        call(ops, "u2tok_lora_down", X, x_off, ldx, A, lda, U, ldu, M, K, r, 1.0, status=-1)

    def up(M=16, N=32, r=16, y_off=0, ldu=64, ldw=64, ldy=64, U=uu.data_ptr(), W=a.data_ptr(), Y=P):
        call(ops, "u2tok_lora_up", U, ldu, W, ldw, Y, y_off, ldy, M, N, r, 1.0, 1, status=-1)

    def wgrad(M=16, C=32, r=16, x_off=0, ldu=64, ldx=64, ldg=64, U=uu.data_ptr(), X=P, G=a.data_ptr()):
        call(ops, "u2tok_lora_wgrad", U, ldu, X, x_off, ldx, G, ldg, M, C, r, 1.0, 0, None, 0, status=-1)

    for fn in (down, up, wgrad):
        fn(r=8), fn(r=48), fn(r=128), fn(M=0), fn(ldu=60)
    down(K=40), down(K=0), down(x_off=4), down(ldx=60), down(ldx=32), down(X=None), down(A=None), down(U=None), down(X=P + 2)
    up(N=24), up(N=0), up(y_off=4), up(ldy=24), up(ldw=8), up(Y=None), up(W=None), up(U=None), up(Y=P + 8)
    wgrad(C=12), wgrad(C=0), wgrad(x_off=2), wgrad(ldx=24), wgrad(ldg=16), wgrad(X=None), wgrad(G=None), wgrad(U=None)
    assert is_nan16(x) and is_nan16(a) and is_nan16(uu)
    with pytest.raises(RuntimeError, match="U2TOK_ERR_ARG"):
        ops.lora_down(torch.zeros(16, 40, dtype=bf, device=D), torch.zeros(16, 40, dtype=bf, device=D))
    with pytest.raises(RuntimeError, match="U2TOK_ERR_ARG"):
        ops.lora_up(torch.zeros(16, 16, dtype=bf, device=D), torch.zeros(24, 16, dtype=bf, device=D))
    with pytest.raises(RuntimeError, match="U2TOK_ERR_ARG"):
        ops.lora_down(torch.zeros(16, 64, dtype=bf, device=D), torch.zeros(8, 64, dtype=bf, device=D))


def test_f16_build(ops):
    """one case per kernel on the IEEE-half build (the wrappers pick the build by the tensors' dtype): the same models, U = 2^-11"""
    h = torch.float16
    M, K, r = F16_DOWN
    inp = B.down_inputs(M, K, r, dtype=h)
    m = B.down_model(U=B.U16, **inp)
    _, x = segment(inp["x"], 8, 8, dtype=h)
    with torch.no_grad():
        got = ops.lora_down(x, inp["a"].to(D), alpha=inp["alpha"])
    hold("lora_down f16", got, m["out"], m["bound"])
    M, N, r, acc = F16_UP
    inp = B.up_inputs(M, N, r, dtype=h)
    m = B.up_model(accumulate=acc, U=B.U16, **inp)
    st, y = segment(inp["y"], 16, 8, dtype=h)
    with torch.no_grad():
        ops.lora_up(inp["uu"].to(D), inp["w"].to(D), y, alpha=inp["alpha"], accumulate=bool(acc))
    torch.cuda.synchronize()
    assert outside_is_nan(st, M, 16 + N + 8, 16, N)
    hold("lora_up f16", y, m["out"], m["bound"])
    M, C, r, f32 = F16_WGRAD
    inp = B.wgrad_inputs(M, C, r, dtype=h)
    m = B.wgrad_model(out_f32=f32, U=B.U16, **inp)
    _, x = segment(inp["x"], 8, 16, dtype=h)
    with torch.no_grad():
        got = ops.lora_wgrad(inp["uu"].to(D), x, alpha=inp["alpha"], out_f32=bool(f32))
    hold("lora_wgrad f16", got, m["out"], m["bound"])
