"""GPU: the RMSNorm in the tail of the few-rows product (u2tok_gemm_rows_norm; csrc/rows.h: rows_norm_tail), in both element builds
and the three weight forms.  Y must have the bits of the plain product (u2tok_gemm_rows / _w8_wide / _w4) and Yn the bits of
u2tok_rmsnorm_bf16(Y): the tail runs the row function of the norm's own kernel, so there is no tolerance.  Every shape runs 20 times
back to back on the SAME buffers and ticket with fresh inputs uploaded in between: a workgroup that normed rows another workgroup
had not made visible, or lines a compute unit kept from the run before, shows as the previous run's values; a ticket that was not put
back shows at the next run (no workgroup, or the wrong one, draws the last ticket) and in the word itself."""
import pytest
import torch

pytestmark = pytest.mark.gpu
D = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
FORMS = ["elem", "e4m3", "e2m1"]
EPS = 1e-6
RUNS = 20


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


def _weights(ops, form, N, K, dt, g):
    w = torch.randn(N, K, generator=g) / K ** 0.5
    if form == "elem":
        return w.to(dt).to(D), None
    q = ops.quantize_rows_fp8 if form == "e4m3" else ops.quantize_blocks_fp4
    return tuple(t.to(D) for t in q(w))


def _plain(ops, form, x, W, sc, bias, R):
    if form == "elem":
        return ops.gemm_rows(x, W, bias=bias, residual=R)
    return (ops.gemm_rows_w8 if form == "e4m3" else ops.gemm_rows_w4)(x, W, sc, bias=bias, residual=R)


# N = 16: one workgroup (the first ticket is the last); 32: two; 256: 16; 4096: 256 workgroups = the compute units of the device, and
# the widest row the tail takes (8 chunks per lane).  M: one row, a partial block, a full block, 2 and 4 blocks (waves loop over rows).
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_product_and_norm_have_the_bits_of_the_two_launches(ops, dt, form):
    g = torch.Generator().manual_seed(1234 + FORMS.index(form))
    ticket = torch.zeros(1, dtype=torch.int32, device=D)
    cases = 0
    for K in (128, 512):
        for N in (16, 32, 256, 4096):
            W, sc = _weights(ops, form, N, K, dt, g)
            wn = (1.0 + 0.25 * torch.randn(N, generator=g)).to(dt).to(D)
            bvec = (0.5 * torch.randn(N, generator=g)).to(dt).to(D)
            for M in (1, 5, 16, 17, 64):
                bias = bvec if (M + N // 16 + K // 128) % 2 else None     # (with and without, over every M, N and K)
                xs = torch.randn(RUNS, M, K, generator=g).to(dt).to(D)
                Rs = torch.randn(RUNS, M, N, generator=g).to(dt).to(D)
                x, R = torch.empty_like(xs[0]), torch.empty_like(Rs[0])
                Y, Yn = (torch.full((M, N), 7.0, dtype=dt, device=D) for _ in range(2))
                for run in range(RUNS):
                    x.copy_(xs[run]), R.copy_(Rs[run])
                    ops.gemm_rows_norm(x, W, wn, EPS, ticket, residual=R, scale=sc, bias=bias, out=Y, out_norm=Yn)
                    want = _plain(ops, form, x, W, sc, bias, R)
                    key = (form, M, N, K, bias is not None, run)
                    assert torch.equal(Y, want), key
                    assert torch.equal(Yn, ops.rmsnorm(want, wn, EPS)), key
                assert int(ticket.item()) == 0, (form, M, N, K)
                assert torch.isfinite(Yn).all() and Yn.float().abs().max() > 0.1
                cases += 1
    assert cases == 40


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_strided_outputs_stay_inside_their_columns(ops, dt):
    """Y and Yn as column blocks of wider buffers, the residual with its own row stride: nothing outside the blocks is written."""
    g = torch.Generator().manual_seed(77)
    M, N, K = 5, 256, 128
    W, _ = _weights(ops, "elem", N, K, dt, g)
    wn = (1.0 + 0.25 * torch.randn(N, generator=g)).to(dt).to(D)
    x = torch.randn(M, K, generator=g).to(dt).to(D)
    Rb = torch.randn(M, N + 24, generator=g).to(dt).to(D)
    Yb, Ynb = (torch.full((M, N + 16), 7.0, dtype=dt, device=D) for _ in range(2))
    ticket = torch.zeros(1, dtype=torch.int32, device=D)
    ops.gemm_rows_norm(x, W, wn, EPS, ticket, residual=Rb[:, 8:8 + N], out=Yb[:, 8:8 + N], out_norm=Ynb[:, 8:8 + N])
    want = ops.gemm_rows(x, W, residual=Rb[:, 8:8 + N])
    assert torch.equal(Yb[:, 8:8 + N], want) and torch.equal(Ynb[:, 8:8 + N], ops.rmsnorm(want, wn, EPS))
    for b in (Yb, Ynb):
        assert (b[:, :8] == 7).all() and (b[:, 8 + N:] == 7).all()
    assert int(ticket.item()) == 0


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_illegal_combinations_are_refused_with_nothing_written(ops, dt):
    g = torch.Generator().manual_seed(78)
    M, N, K = 5, 256, 128
    W, _ = _weights(ops, "elem", N, K, dt, g)
    wn = torch.ones(N, dtype=dt, device=D)
    x = torch.randn(M, K, generator=g).to(dt).to(D)
    R = torch.randn(M, N, generator=g).to(dt).to(D)
    ticket = torch.zeros(1, dtype=torch.int32, device=D)
    bytes8 = torch.zeros(8, dtype=torch.uint8, device=D)
    Y, Yn = (torch.full((M, N), 7.0, dtype=dt, device=D) for _ in range(2))

    def refused(**kw):
        args = dict(residual=R, out=Y, out_norm=Yn)
        args.update(kw)
        t = args.pop("ticket", ticket)
        with pytest.raises(RuntimeError, match="U2TOK_ERR_ARG"):
            ops.gemm_rows_norm(x, W, wn, EPS, t, **args)
        torch.cuda.synchronize()
        assert (Y == 7).all() and (Yn == 7).all() and int(ticket.item()) == 0 and not bytes8.any()

    refused(flags=512)                       # the pair form
    refused(flags=512 | 8)
    refused(residual=None)                   # no residual
    refused(flags=1, bias=wn)                # a bias, but no residual flag
    refused(flags=8 | 16)                    # fp32 C
    refused(ticket=None)
    refused(ticket=bytes8[2:])               # 2 bytes off a 4-byte boundary
    wide = torch.ones(4104, dtype=dt, device=D)
    with pytest.raises(RuntimeError, match="U2TOK_ERR_ARG"):    # a row wider than the tail holds
        ops.gemm_rows_norm(x, torch.zeros(4104, K, dtype=dt, device=D), wide, EPS, ticket, residual=torch.zeros(M, 4104, dtype=dt, device=D))
    with pytest.raises(RuntimeError, match="U2TOK_ERR_ARG"):    # N % 8 != 0
        ops.gemm_rows_norm(x, W[:20], wn[:20], EPS, ticket, residual=R[:, :20].contiguous())
    assert int(ticket.item()) == 0
