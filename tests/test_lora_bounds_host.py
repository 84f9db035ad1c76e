"""Host: the per-element error bounds that tests/test_gpu_lora_ops.py holds the rank-r adapter kernels to (u2tok_lora_down,
u2tok_lora_up, u2tok_lora_wgrad; csrc/lora.hip), as pure functions of the 16-bit inputs, next to a torch emulation of each kernel's
rounding points, in the style of tests/test_decoder_train_bounds_host.py (whose helpers and conventions are used: U = 2^-8 per bf16
rounding, u = 2^-24 per fp32 operation, no fitted factor).  The tests run the emulation on every case of the GPU module's tables
(imported, not copied) and assert that it stays inside the bound.

The kernels round once, at the store; before it they sum exact products of 16-bit values in fp32, in some fixed order, and scale
the sum by alpha in fp32.  A sum of n terms in any order errs by at most (n - 1) u sum |terms| to first order, the scaling by one
more u:
  down    U |ref| + K u sum_k |alpha x a|
  up      U |ref| + (r + 2) u (|y| + |alpha| sum_k |u w|)        (r terms, the scaling, the addition of float(y))
  wgrad   U |ref| + M u sum_m |alpha u x|                        (M - 1 additions and the scaling; fp32 output: without U |ref|)
For the f16 build U is 2^-11 (the `U` argument of the *_model functions)."""
import pytest
import torch

from test_decoder_train_bounds_host import U, _gen, f64, u, worst

bf = torch.bfloat16
U16 = 2.0 ** -11   # IEEE half: 11 significand bits


def _rn(g, *shape, scale=1.0, dtype=bf):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def rnd16(t, dtype=bf):
    """an fp32 value rounded to the element type, back in float64"""
    return t.float().to(dtype).double()


def alpha_of(*key):
    """the cases' scale factors: exactly representable, 1 on a third of the cases"""
    return (1.0, 2.0, 0.375)[sum(int(k) for k in key) % 3]


# ------------------------------------------------------------------------------------------------------------------- down
def down_inputs(M, K, r, dtype=bf):
    g = _gen(11, M, K, r)
    return dict(x=_rn(g, M, K, dtype=dtype), a=_rn(g, r, K, scale=K ** -0.5, dtype=dtype), alpha=alpha_of(M, K, r))


def down_model(x, a, alpha, U=U):
    x, a = x.double(), a.double()
    ref = alpha * (x @ a.T)
    mag = abs(alpha) * (x.abs() @ a.abs().T)
    return dict(out=ref, bound=U * ref.abs() + x.shape[1] * u * mag)


def _chunked_f32(p, q, chunk):
    """p (m, n) @ q (n, c) with fp32 partial sums over chunks of the contraction, added in order"""
    acc = torch.zeros(p.shape[0], q.shape[1], dtype=torch.float32)
    for k in range(0, p.shape[1], chunk):
        acc = acc + p[:, k:k + chunk].float() @ q[k:k + chunk].float()
    return acc


def down_emulate(x, a, alpha, chunk=32):
    return rnd16(_chunked_f32(x, a.T, chunk) * torch.tensor(alpha, dtype=torch.float32), x.dtype)


# --------------------------------------------------------------------------------------------------------------------- up
def up_inputs(M, N, r, dtype=bf):
    g = _gen(12, M, N, r)
    return dict(uu=_rn(g, M, r, dtype=dtype), w=_rn(g, N, r, scale=0.5, dtype=dtype), y=_rn(g, M, N, scale=1.5, dtype=dtype),
                alpha=alpha_of(M, N, r))


def up_model(uu, w, y, alpha, accumulate, U=U):
    uu, w = uu.double(), w.double()
    y = y.double() if accumulate else torch.zeros(uu.shape[0], w.shape[0], dtype=f64)
    ref = y + alpha * (uu @ w.T)
    mag = y.abs() + abs(alpha) * (uu.abs() @ w.abs().T)
    return dict(out=ref, bound=U * ref.abs() + (uu.shape[1] + 2) * u * mag)


def up_emulate(uu, w, y, alpha, accumulate, chunk=16):
    acc = _chunked_f32(uu, w.T, chunk) * torch.tensor(alpha, dtype=torch.float32)
    if accumulate:
        acc = y.float() + acc
    return rnd16(acc, uu.dtype)


# ------------------------------------------------------------------------------------------------------------------ wgrad
def wgrad_inputs(M, C, r, dtype=bf):
    g = _gen(13, M, C, r)
    return dict(uu=_rn(g, M, r, dtype=dtype), x=_rn(g, M, C, dtype=dtype), alpha=alpha_of(M, C, r))


def wgrad_model(uu, x, alpha, out_f32, U=U):
    uu, x = uu.double(), x.double()
    ref = alpha * (uu.T @ x)
    mag = abs(alpha) * (uu.abs().T @ x.abs())
    return dict(out=ref, bound=(0.0 if out_f32 else U) * ref.abs() + uu.shape[0] * u * mag)


def wgrad_emulate(uu, x, alpha, out_f32, chunk=32):
    acc = _chunked_f32(uu.T, x, chunk) * torch.tensor(alpha, dtype=torch.float32)
    return acc.double() if out_f32 else rnd16(acc, uu.dtype)


# ------------------------------------------------------------------------------------------------------------------- tests
_TABLES = {"down_case": "DOWN_CASES", "up_case": "UP_CASES", "wgrad_case": "WGRAD_CASES"}


def pytest_generate_tests(metafunc):
    """the cases are the GPU module's tables (imported here, at collection: that module imports this one at its top)"""
    import test_gpu_lora_ops as gpu
    for arg, table in _TABLES.items():
        if arg in metafunc.fixturenames:
            metafunc.parametrize(arg, getattr(gpu, table), ids=lambda c: "-".join(str(x) for x in c))


def _report(name, ratio):
    print(f"emulated error / bound, {name}: {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


def test_down_emulation_inside_bound(down_case):
    inp = down_inputs(*down_case)
    m = down_model(**inp)
    for chunk in (32, 256):
        _report(f"lora_down (chunks of {chunk})", worst((down_emulate(chunk=chunk, **inp) - m["out"]).abs(), m["bound"]))


def test_up_emulation_inside_bound(up_case):
    M, N, r, accumulate = up_case
    inp = up_inputs(M, N, r)
    m = up_model(accumulate=accumulate, **inp)
    for chunk in (8, 64):
        _report(f"lora_up (chunks of {chunk})", worst((up_emulate(accumulate=accumulate, chunk=chunk, **inp) - m["out"]).abs(), m["bound"]))


def test_wgrad_emulation_inside_bound(wgrad_case):
    M, C, r, out_f32 = wgrad_case
    inp = wgrad_inputs(M, C, r)
    m = wgrad_model(out_f32=out_f32, **inp)
    for chunk in (32, 128):
        _report(f"lora_wgrad (chunks of {chunk})", worst((wgrad_emulate(out_f32=out_f32, chunk=chunk, **inp) - m["out"]).abs(), m["bound"]))


def test_emulation_inside_bound_on_half_elements():
    """the f16 build's cases: the same models with U = 2^-11"""
    import test_gpu_lora_ops as gpu
    M, K, r = gpu.F16_DOWN
    inp = down_inputs(M, K, r, dtype=torch.float16)
    m = down_model(U=U16, **inp)
    _report("lora_down f16", worst((down_emulate(**inp) - m["out"]).abs(), m["bound"]))
    M, N, r, acc = gpu.F16_UP
    inp = up_inputs(M, N, r, dtype=torch.float16)
    m = up_model(accumulate=acc, U=U16, **inp)
    _report("lora_up f16", worst((up_emulate(accumulate=acc, **inp) - m["out"]).abs(), m["bound"]))
    M, C, r, f32 = gpu.F16_WGRAD
    inp = wgrad_inputs(M, C, r, dtype=torch.float16)
    m = wgrad_model(out_f32=f32, U=U16, **inp)
    _report("lora_wgrad f16", worst((wgrad_emulate(out_f32=f32, **inp) - m["out"]).abs(), m["bound"]))


def test_the_issues_attainability_cases():
    """(M, K, r) at which a chunked fp32 emulation comes close to the down bound: it is not slack by an order of magnitude"""
    for M, K, r in ((5, 32, 16), (33, 520, 16), (130, 4096, 32), (257, 1056, 64)):
        g = _gen(14, M, K, r)
        inp = dict(x=_rn(g, M, K), a=_rn(g, r, K, scale=K ** -0.5), alpha=2.0)
        m = down_model(**inp)
        ratio = worst((down_emulate(**inp) - m["out"]).abs(), m["bound"])
        assert 0.3 <= ratio <= 1.0, (M, K, r, ratio)


def test_bounds_see_one_dropped_step():
    """dropping the last 32-wide step of the contraction, or one row of the wgrad sum, breaks the bound by far"""
    inp = down_inputs(33, 1056, 16)
    m = down_model(**inp)
    short = down_emulate(inp["x"][:, :-32], inp["a"][:, :-32], inp["alpha"])
    assert worst((short - m["out"]).abs(), m["bound"]) > 10
    inp = wgrad_inputs(257, 72, 16)
    m = wgrad_model(out_f32=True, **inp)
    short = wgrad_emulate(inp["uu"][:-1], inp["x"][:-1], inp["alpha"], True)
    assert worst((short - m["out"]).abs(), m["bound"]) > 10
