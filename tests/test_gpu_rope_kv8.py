"""GPU: the head norm + rotary kernel with the quantising append in its launch (u2tok_qk_norm_rope_kv8: what the whole-stack decode
step on an FP8 KV cache runs in the rotary kernel's place).  Its definition of correct is two existing entries: the q and k columns
of qkv have the bits u2tok_qk_norm_rope_kv leaves, the codes and scales the bits of u2tok_kv_quantize_rows on the dense 16-bit rows
that entry writes -- which are the bits of ops.quantize_kv_fp8.  So every comparison here is torch.equal, in both element builds,
over head dims 64 / 96 / 128, with and without head-norm weights, fp32 and 16-bit rotary tables, one and several positions per
sequence, both head groupings and the first, a middle and the last position of the buffers; every byte of the code and scale
buffers outside the written rows keeps its sentinel, and a refused call writes nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu
D = "cuda"
bf, f16 = torch.bfloat16, torch.float16
DTYPES, IDS = [bf, f16], ["bf16", "fp16"]
ROWS_S = [(1, 1), (3, 1), (6, 3)]
HEADS = [(4, 2), (4, 4)]
EPS = 1e-6


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


def _tie_row(d, dt, gen, k):
    """a row whose largest element is 448 * 2^k -- its scale is exactly 2^k -- and whose other elements are 2^k times e4m3
    midpoints (halfway between two neighbouring codes) or codes, in both signs, all exact in bf16 and fp16: the scaled values land
    on the midpoints, and round to nearest EVEN decides every one of them"""
    grid = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    grid = grid[torch.isfinite(grid) & (grid >= 0)].sort().values
    mids = (grid[:-1] + grid[1:]) / 2
    pool = torch.cat([mids, grid, torch.tensor([2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -11])])
    x = pool[torch.randint(0, pool.numel(), (d,), generator=gen)]
    x = x * torch.where(torch.rand(d, generator=gen) < 0.5, -1.0, 1.0)
    x[int(torch.randint(0, d, (1,), generator=gen))] = 448.0
    x = x * 2.0 ** k
    assert torch.equal(x.to(dt).float(), x)
    return x.to(dt)


def _case(dt, d, rows, S, Hq, Hkv, f32, gen):
    """qkv rows of N(0, 1) with the rows that try the quantiser, and rotary tables whose row 0 is position 0 (cos 1, sin 0: the
    rotation is the identity there, so without head-norm weights a k head of row 0 reaches the quantiser as it is written here)"""
    nq = (Hq + 2 * Hkv) * d
    qkv = torch.randn(rows, nq, generator=gen).to(dt)
    k0, v0 = Hq * d, (Hq + Hkv) * d
    qkv[0, v0 + d:v0 + 2 * d] = (torch.randn(d, generator=gen) * 2.0 ** -6).to(dt)       # rows of magnitude 2^-6
    qkv[rows - 1, k0 + d:k0 + 2 * d] = (torch.randn(d, generator=gen) * 2.0 ** -6).to(dt)
    qkv[0, k0:k0 + d] = _tie_row(d, dt, gen, -3)                # a k head on e4m3 midpoints (amax = 448 * 2^-3)
    qkv[0, v0:v0 + d] = 0                                       # an all-zero v row: scale 1, zero codes
    qkv[rows - 1, v0 + (Hkv - 1) * d:v0 + Hkv * d] = _tie_row(d, dt, gen, 2)       # a v head on midpoints (amax = 448 * 4)
    ang = torch.rand(rows, d // 2, generator=gen) * 6.28
    ang[0] = 0
    cos, sin = torch.cat([ang.cos(), ang.cos()], 1), torch.cat([ang.sin(), ang.sin()], 1)
    if not f32:
        cos, sin = cos.to(dt), sin.to(dt)
    return qkv, cos, sin


def _buffers(B, Hkv, cap, d):
    return [torch.full((B, Hkv, cap, d), 0xA5, dtype=torch.uint8, device=D), torch.full((B, Hkv, cap, d), 0x5A, dtype=torch.uint8, device=D),
            torch.full((B, Hkv, cap), -7.0, device=D), torch.full((B, Hkv, cap), -9.0, device=D)]


@pytest.mark.parametrize("norm", [True, False], ids=["head norm", "no head norm"])
@pytest.mark.parametrize("d", [64, 96, 128])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_bit_equal_to_the_rotary_kernel_followed_by_the_quantiser(ops, dt, d, norm):
    gen = torch.Generator().manual_seed(1000 * d + norm)
    n = 0
    for f32 in (True, False):
        for rows, S in ROWS_S:
            for Hq, Hkv in HEADS:
                B, cap = rows // S, S + 9
                wq = wk = None
                if norm:
                    wq, wk = ((1 + 0.25 * torch.randn(d, generator=gen)).to(dt).to(D) for _ in range(2))
                qkv, cos, sin = _case(dt, d, rows, S, Hq, Hkv, f32, gen)
                cos, sin = cos.to(D), sin.to(D)
                # the definition: the rotary kernel into dense 16-bit rows ...
                want = qkv.to(D)
                _, kd, vd = ops.qk_norm_rope(want, wq, wk, cos, sin, Hq, Hkv, d, EPS, kv_cache_seq=S)
                assert kd.shape == (B, Hkv, S, d)
                if not norm:   # (the identity rotation of row 0: the midpoint row reaches the quantiser as written)
                    assert torch.equal(kd[0, 0, 0].cpu(), qkv[0, Hq * d:(Hq + 1) * d])
                assert not bool(vd[0, 0, 0].any())
                for s_off in (0, 5, cap - S):
                    # ... followed by the quantiser of those rows
                    ref = _buffers(B, Hkv, cap, d)
                    ops.kv_quantize_rows(kd, vd, *ref, s_off)
                    got = qkv.to(D)
                    bufs = _buffers(B, Hkv, cap, d)
                    r = ops.qk_norm_rope_kv8(got, wq, wk, cos, sin, Hq, Hkv, d, EPS, *bufs, S, s_off)
                    assert r is got
                    what = (f32, rows, S, Hq, Hkv, s_off)
                    assert torch.equal(got, want), ("qkv", what)
                    # codes, scales (as bits) and every sentinel byte around them: the whole buffers
                    for name, a, b in zip(("k codes", "v codes"), bufs[:2], ref[:2]):
                        assert torch.equal(a, b), (name, what)
                    for name, a, b in zip(("k scales", "v scales"), bufs[2:], ref[2:]):
                        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, what)
                    fresh = _buffers(B, Hkv, cap, d)
                    for a, b in zip(bufs, fresh):
                        assert torch.equal(a[:, :, :s_off], b[:, :, :s_off]) and torch.equal(a[:, :, s_off + S:], b[:, :, s_off + S:]), what
                    # ... and the reference quantiser on those rows (on the CPU, where torch's division by 448 is IEEE's: on the
                    # GPU it multiplies by a reciprocal -- tests/test_gpu_kv8.py compares the quantising kernel the same way)
                    for x, codes, scales in ((kd, bufs[0], bufs[2]), (vd, bufs[1], bufs[3])):
                        wc, wsc = ops.quantize_kv_fp8(x.cpu())
                        assert torch.equal(codes[:, :, s_off:s_off + S].cpu(), wc.view(torch.uint8)), what
                        assert torch.equal(scales[:, :, s_off:s_off + S].cpu().view(torch.int32), wsc.view(torch.int32)), what
                    assert float(bufs[3][0, 0, s_off]) == 1.0 and not bool(bufs[1][0, 0, s_off].any())      # the all-zero v row
                    if not norm:
                        assert float(bufs[2][0, 0, s_off]) == 2.0 ** -3                                     # the midpoint k row
                    assert float(bufs[3][B - 1, Hkv - 1, s_off + S - 1]) == 4.0                             # the midpoint v row
                    n += 1
    assert n == 2 * len(ROWS_S) * len(HEADS) * 3


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_a_refused_call_writes_nothing(ops, dt):
    ERR_ARG = -1
    d, rows, S, Hq, Hkv, cap = 64, 6, 3, 4, 2, 12
    B = rows // S
    gen = torch.Generator().manual_seed(7)
    qkv, cos, sin = _case(dt, d, rows, S, Hq, Hkv, True, gen)
    got, cos, sin = qkv.to(D), cos.to(D), sin.to(D)
    bufs = _buffers(B, Hkv, cap, d)
    spare = torch.full((B * Hkv * cap * d + 16,), 0xA5, dtype=torch.uint8, device=D)     # room for a buffer that starts 8 bytes in
    assert spare.data_ptr() % 16 == 0
    with ops.on_device(got) as (h, stream):
        def call(kc=bufs[0].data_ptr(), ks=bufs[2].data_ptr(), s_off=0, S_=S, cap_=cap):
            return h.u2tok_qk_norm_rope_kv8(got.data_ptr(), None, None, cos.data_ptr(), sin.data_ptr(), 1, rows, Hq, Hkv, d, got.stride(0),
                                            cos.stride(0), EPS, kc, bufs[1].data_ptr(), ks, bufs[3].data_ptr(), S_, cap_, s_off, stream)

        assert call(s_off=cap - S + 1) == ERR_ARG                  # s_off + S > capacity
        assert call(s_off=-1) == ERR_ARG and call(cap_=0) == ERR_ARG and call(S_=0) == ERR_ARG and call(S_=4) == ERR_ARG
        assert call(kc=spare.data_ptr() + 8) == ERR_ARG            # a misaligned code buffer
        assert call(ks=bufs[2].data_ptr() + 2) == ERR_ARG and call(kc=None) == ERR_ARG and call(ks=None) == ERR_ARG
        torch.cuda.synchronize()
    assert torch.equal(got.cpu(), qkv) and bool((spare == 0xA5).all())
    assert all(torch.equal(a, b) for a, b in zip(bufs, _buffers(B, Hkv, cap, d)))
    with pytest.raises(RuntimeError, match="u2tok_qk_norm_rope_kv8"):
        ops.qk_norm_rope_kv8(got, None, None, cos, sin, Hq, Hkv, d, EPS, *bufs, S, cap - S + 1)
    assert torch.equal(got.cpu(), qkv) and all(torch.equal(a, b) for a, b in zip(bufs, _buffers(B, Hkv, cap, d)))
