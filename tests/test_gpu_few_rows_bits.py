"""The few-rows (weight-streaming) product, BIT FOR BIT: the SHA-256 of every case's output bytes against
tests/golden/few_rows_bits.json, recorded once with the kernels of the commit named inside it (before csrc/rows.h and
csrc/gemm_rows.hip replaced the three copies of this arithmetic), and for e2m1 weights against tests/golden/few_rows_bits_e2m1.json,
recorded with the commit that brought that form (before the weight form became a field of the kernels' arguments).  Every other test of these kernels compares them with each
other or holds them to a float64 bound, so a change that moves all of them together -- a different contraction in the shared
epilogue, another order of the partial sums -- passes there; here it does not.  A digest that moves is a changed bit: find the
expression.  The fixture is never re-recorded by this file.

Cases (tests/few_rows_cases.py): both builds x three weight forms x M in {1, 13, 16, 17, 33, 64} (NB = 1 .. 4 row blocks, ragged
and full) x the (N, K) of SHAPES / SHAPES_E2M1 (NW = 4 / 8 / 16 waves, empty slices, remainder blocks, the seam between whole
blocks and the remainder; e2m1: one, 3, 16 and 64 quad steps) x {plain, bias + residual through strided views, fp32 out, the pair
form}; the plan's route (alpha, bias, GELU at M = 13) and the last rows of three big-tile products.  Together they reach all 72
instantiations of gemm_rows16_kernel.

The host half (no GPU) checks that the inputs can tell two summation orders apart at all."""
import json

import pytest
import torch

import few_rows_cases as C


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


@pytest.fixture(scope="module")
def fixture():
    digests = {}
    for path in C.FIXTURES:
        f = json.loads(path.read_text())
        assert len(f["recorded_at_commit"]) == 40
        digests.update(f["digests"])
    return digests


def _compare(got, fixture):
    moved = sorted(k for k, v in got.items() if fixture.get(k) != v)
    assert not moved, f"{len(moved)} of {len(got)} outputs changed bits: {moved[:12]}"


@pytest.mark.gpu
@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("elem", list(C.DTYPES))
def test_product_bits(ops, fixture, elem, form):
    _compare(C.product_digests(ops, elem, form), fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("elem", list(C.DTYPES))
def test_plan_and_tail_bits(ops, fixture, elem):
    _compare(C.plan_digests(ops, elem), fixture)


# ------------------------------------------------------------------------------------------------------------- host: the inputs
def test_fixture_lists_exactly_the_cases():
    for path in C.FIXTURES:
        assert sorted(json.loads(path.read_text())["digests"]) == sorted(C.case_ids(path))
    ids = [k for path in C.FIXTURES for k in C.case_ids(path)]     # the union: every build x form x case, none twice
    assert len(set(ids)) == len(ids) == sum(len(C.product_cases(f)) for f in C.FORMS) * len(C.DTYPES) + len(C.PLAN_CASES) * len(C.DTYPES)


def test_inputs_are_what_the_case_file_promises():
    for N, K in C.SHAPES:
        x, w = C.activations(K), C.weights(N, K)
        for t, lo in ((x, -4), (w, -7)):
            assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.to(torch.float16).float(), t)
            e = torch.floor(torch.log2(t.abs()))
            assert e.min() == lo and e.max() == lo + 5 and len(e.unique()) == 6              # 6 binades
            assert len((t.abs() / torch.exp2(e)).unique()) == 128                            # every 8-bit significand
        c, s = C.weights_e4m3(N, K)
        assert len(c.unique()) == 254 and not ((c & 0x7F) == 0x7F).any()
        assert s.dtype == torch.float32 and (s > 0).all()
    # full mantissas: over the scales of all shapes, each of the 23 mantissa bits is set in about half, and hardly any scale has an
    # empty low byte (1 in 256 by chance)
    m = torch.cat([C.weights_e4m3(N, K)[1] for N, K in C.SHAPES]).view(torch.int32) & 0x7FFFFF
    share = torch.stack([((m >> b) & 1).float().mean() for b in range(23)])
    assert share.min() >= 0.4 and share.max() <= 0.6, share
    assert ((m & 0xFF) != 0).float().mean() >= 0.98
    for N, K in C.SHAPES_E2M1:   # e2m1: every code in both nibbles, the block scales over 10 binades or more
        codes, sc = C.weights_e2m1(N, K)
        assert codes.shape == (N, K // 2) and sc.shape == (N, K // 32) and codes.dtype == sc.dtype == torch.uint8
        for nib in (codes & 15, codes >> 4):                 # (-0, code 8, is the one code the quantiser never emits)
            assert sorted(nib.unique().tolist()) == [c for c in range(16) if c != 8]
        assert len(sc.unique()) >= 10


def _sum_in_slices(x, w, nw, per, step, reverse):
    """fp32 (M, N): the products x[m][k] w[n][k] (exact in fp32) added one k at a time within a slice of `per` steps of `step` k,
    the slices' sums then added one by one -- ascending in both, or descending in both"""
    K = x.shape[1]
    parts = []
    for s in range(nw):
        ks = list(range(min(K, s * per * step), min(K, (s + 1) * per * step)))
        acc = torch.zeros(x.shape[0], w.shape[0])
        for k in (reversed(ks) if reverse else ks):
            acc = acc + x[:, k, None] * w[None, :, k]
        parts.append(acc)
    total = torch.zeros_like(parts[0])
    for p in (reversed(parts) if reverse else parts):
        total = total + p
    return total


@pytest.mark.parametrize("form", C.FORMS)
def test_inputs_tell_two_summation_orders_apart(form):
    """Small integers would give the same fp32 sum in any order and hide a reordering.  For each K of the cases, 13 rows x 16
    columns: the sum over the kernel's K slices taken ascending and taken descending (fp32, on the CPU) differs in at least one
    output bit."""
    from u2tokenizer_amd import ops
    for N, K in C.shapes(form):
        x = C.activations(K)[:13]
        w = (C.weights_e4m3(N, K)[0].view(torch.float8_e4m3fn).float() if form == "e4m3"
             else ops.dequantize_blocks_fp4(*C.weights_e2m1(N, K)) if form == "e2m1" else C.weights(N, K))[:16]
        nw, per = C.slices(K, form=form)
        a = _sum_in_slices(x, w, nw, per, C.STEP_K[form], False)
        b = _sum_in_slices(x, w, nw, per, C.STEP_K[form], True)
        assert torch.isfinite(a).all() and (a != b).any(), (form, K)
