"""Host: the per-element bound that tests/test_gpu_gemm_bounds.py holds the forward GEMM kernels to (tests/gemm_cases.py: model), proved
on the CPU the way tests/test_row_fwd_bounds_host.py proves the row kernels' bounds.  `emulate` repeats a GEMM kernel's arithmetic in
torch fp32 -- an fp32 matmul per K slice of the case (gemm_cases.k_slices: the slices the launchers cut), the slices added in fp32,
then the epilogue with the documented rounding points: alpha (alpha_lo below nsplit) times the fp32 sum, + bias, GELU of the value
rounded to the element type (kernels.h: gelu_epi), + residual, ONE rounding at the store; the pair form rounds gate and up, then
silu(gate), then the product (rows.h: rows_pair_store).  The tests run it over every case and data set of the GPU module's tables
(imported, not copied) and assert that it stays inside the bound; with `fault=` it repeats a kernel that is wrong in one of the 13
named ways, and each of those must leave the bound on at least one named case of a form it can occur in.

Terms added to the bound the gate was specified with, each derived, none fitted:
  * SwiGLU pair: U (|silu'(g)| |g| |up| + |silu(g)| |up|).  The specification charged `elem(silu(gate)) * up`; the pair epilogue's
    contract (include/u2tok.h, rows.h) also rounds gate and up to the element type first, "the values u2tok_gemm_bf16 +
    u2tok_swiglu_bf16 produce, bit for bit".  A relative change U of g moves silu(g) up by |silu'(g)| U |g| |up|, one of up by
    |silu(g)| U |up|.  Without the term the emulation of the documented contract reaches 2.3 times the bound.
  * SwiGLU pair: the two roundings are charged at least what the formats underflow by (gemm_cases' docstring has the figures):
    integer data put gates at -100, where silu is below the subnormals of f16 and e^-g overflows fp32.

Worst emulated error / bound over the tables: plain / bias / residual 0.995, GELU 0.970, pair 0.815, fp32 outputs 0.024 -- a ratio near
1.0 is a correctly rounded result on the worst-placed element (value just above a power of two: half an ulp = U |value|); on fp32
outputs only the fp32 terms are left, and torch's blocked summation stays far below their any-order worst case.  What each planted fault
reaches on its named case (printed and kept in FAULT_REACH by the test, asserted > 1): K-slice partials rounded 6.9, accumulator
rounded 7.4, bias before alpha 41 000, residual before GELU 6 100, bias_m by n 57 000, last k 207, last chunk of the last row tile
1 069, K tile twice 1 743, alpha_lo 16 columns far 199, alpha_lo twice 199, tail rows by alpha 1 148; both V^T faults break bit-equality."""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as G
from gemm_cases import BF16, F16, ratio

f32 = torch.float32


def _rnd(t, el):
    return t.to(el.dtype).float()


def tile_rows(form):
    """rows per output tile of the form's kernel"""
    return 16 if "rows16" in form else 64 if "64" in form or "skinny" in form or form == "split_tile_splitk" else 128 if "128" in form else 256


def emulate(form, p, A, B, bias, R, el=BF16, fault=None):
    """-> C (nz, M, N or I) as the kernel stores it (element type, or fp32 with OUT_F32)"""
    M, N, K, flags = p["M"], p["N"], p["K"], p.get("flags", 0)
    A, B = A.float().clone(), B.float().clone()
    T = tile_rows(form)
    if fault == "last_k":
        A[..., K - 1] = 0
    if fault == "last_chunk_last_row_tile":
        A[:, (M - 1) // T * T:, K - 8:] = 0
    slices = G.k_slices(p)
    acc = torch.zeros(A.shape[0], M, N)
    for k0, k1 in slices:
        part = A[..., k0:k1] @ B[..., k0:k1].transpose(1, 2)
        if fault == "k_tile_twice" and k0 == 0 and K >= 128:        # output tile (0, 0): K tile 0 read in place of K tile 1
            t = min(T, M)
            part[:, :t, :64] += A[:, :t, 0:64] @ B[:, :64, 0:64].transpose(1, 2) - A[:, :t, 64:128] @ B[:, :64, 64:128].transpose(1, 2)
        if fault == "slice_rounded" and len(slices) > 1:
            part = _rnd(part, el)
        acc = acc + part
    if flags & G.SWIGLU:
        I = N // 2
        gate, up = _rnd(acc[..., :I], el), _rnd(acc[..., I:], el)
        return (_rnd(gate * torch.sigmoid(gate), el) * up).to(el.dtype)
    al = G.alpha_cols(p).float()
    ns = p.get("nsplit", 0)
    if ns:
        lo, hi = al[0].clone(), al[-1].clone()
        if fault == "alpha_lo_far":
            al[ns:ns + 16] = lo
        if fault == "alpha_lo_twice" and len(slices) > 1:
            al[:ns] = lo * lo
    al = al.expand(M, N).clone()
    if ns and fault == "tail_alpha" and M % 256:
        al[M - M % 256:, :ns] = hi
    b = 0.0 if bias is None else (bias.float()[:, None] if flags & G.BIAS_M else bias.float()[None, :])
    if fault == "bias_m_by_n" and flags & G.BIAS_M:
        b = bias.float()[torch.arange(N) % M][None, :]
    x = (acc + b) * al if fault == "bias_before_alpha" else acc * al
    if fault == "acc_rounded":
        x = _rnd(x, el)
    if fault != "bias_before_alpha":
        x = x + b
    r = 0.0 if R is None else R.float()
    if flags & G.GELU:
        x = F.gelu(_rnd(x + r, el)) if fault == "res_before_gelu" else F.gelu(_rnd(x, el)) + r
    else:
        x = x + r
    return x if flags & G.OUT_F32 else x.to(el.dtype)


def vt_of(C, p, fault=None):
    """the V^T side output of a q|k|v case from its row-major product C (M, N): vt[chunk][n - vt_n0][perm16(key)] over the many-row
    part (whole 256-row tiles)"""
    n0, rows = p["vt"]
    Mt = p["M"] // 256 * 256
    V = C[:Mt, n0:].reshape(Mt // rows, rows, -1)
    if fault == "vt_chunk_off":
        V = torch.roll(V, 1, 0)
    out = torch.empty_like(V.transpose(1, 2))
    out[:, :, torch.arange(rows) if fault == "vt_plain_order" else G.perm16(rows)] = V.transpose(1, 2)
    return out


FAULTS = ("slice_rounded", "acc_rounded", "bias_before_alpha", "res_before_gelu", "bias_m_by_n", "last_k", "last_chunk_last_row_tile",
          "k_tile_twice", "alpha_lo_far", "alpha_lo_twice", "tail_alpha", "vt_plain_order", "vt_chunk_off")
# fault -> (form, substring of the descriptor, data set): the named case it must leave the bound on
FAULT_CASE = {
    "slice_rounded": ("tile128_splitk", "gemm_splitk=3", "cancel_k"),
    "acc_rounded": ("skinny", "M=256 N=2048 K=1408", "cancel_r"),
    "bias_before_alpha": ("tile64", "alpha=0.5", "normal"),
    "res_before_gelu": ("tile64", f"flags={G.BIAS_N | G.GELU | G.RES:#x}", "normal"),
    "bias_m_by_n": ("tile64", f"flags={G.BIAS_M | G.OUT_F32:#x}", "normal"),
    "last_k": ("big24", "M=300 N=200 K=832", "normal"),
    "last_chunk_last_row_tile": ("big21", "M=300 N=200 K=448", "normal"),
    "k_tile_twice": ("big22_sliced", "M=300 N=200 K=832", "cancel_k"),
    "alpha_lo_far": ("qkv_drain_tail", "K=768", "normal"),
    "alpha_lo_twice": ("split_big_sliced", "nsplit=192", "normal"),
    "tail_alpha": ("qkv_deep_tail", "K=256", "normal"),
    "vt_plain_order": ("qkv_drain", "K=768", "normal"),
    "vt_chunk_off": ("qkv_drain_tail", "K=1152", "normal"),
}
# what each fault reached on its case when this module was written (error / bound; inf = a bit-exact property broken)
FAULT_REACH = {}


def _cases(form=None, has="", data=None):
    for f, d, ds in G.ALL_CASES:
        if (form is None or f == form) and has in d:
            for s in ds:
                if data is None or s == data:
                    yield f, d, s


@pytest.mark.parametrize("form", G.FORMS)
def test_emulation_stays_inside_the_bound(form):
    """every case and data set of the form, both element types on its first case: error / bound <= 1; on integer data the exact
    columns equal the float64 value rounded once"""
    worst = 0.0
    for i, (f, d, data) in enumerate(_cases(form)):
        p = G.parse(d)
        for el in ((BF16, F16) if i == 0 else (BF16,)):
            inp = G.inputs(f, p, data, el)
            m = G.model(p, **inp, el=el)
            got = emulate(f, p, **inp, el=el)
            r = ratio(got, m["ref"], m["bound"])
            worst = max(worst, r)
            assert r <= 1.0, (f, d, data, el.name, r)
            if data == "ints" and m["exact"] is not False:
                want = G.round_once(m["ref"], p.get("flags", 0), el)
                assert torch.equal(got[..., m["exact"]], want[..., m["exact"]]), (f, d, el.name)
    print(f"{form}: worst emulated error / bound {worst:.3f}")


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_leaves_the_bound(fault):
    form, has, data = FAULT_CASE[fault]
    found = list(_cases(form, has, data))
    assert found, (fault, "no such case in the tables")
    f, d, _ = found[0]
    p = G.parse(d)
    inp = G.inputs(f, p, data)
    m = G.model(p, **inp)
    if fault.startswith("vt_"):
        good = emulate(f, p, **inp)[0]
        assert not torch.equal(vt_of(good, p, fault), vt_of(good, p))
        r = math.inf
    else:
        assert ratio(emulate(f, p, **inp), m["ref"], m["bound"]) <= 1.0
        r = ratio(emulate(f, p, **inp, fault=fault), m["ref"], m["bound"])
    FAULT_REACH[fault] = (f, d, data, r)
    print(f"{fault}: error / bound {r:.1f} on {f} [{d}] {data}")
    assert r > 1.0, (fault, f, d, data, r)


def test_every_fault_has_a_gpu_case():
    """the named cases are cases of the GPU module's tables, of a form the fault can occur in"""
    for fault, (form, has, data) in FAULT_CASE.items():
        assert list(_cases(form, has, data)), fault
    assert set(FAULT_CASE) == set(FAULTS)


def test_perm16_is_the_flash_key_order():
    assert G.perm16(32).tolist()[:16] == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    assert sorted(G.perm16(256).tolist()) == list(range(256))
