"""GPU: the front end and token selection kernels against exact references -- im2col_patches, fill_rows (csrc/vision.hip), score_gemv,
topk_sorted, gather_rows, multiscale_pool with dmtp_gate_partial (csrc/select.hip) -- at the smallest shapes that reach every branch
of their launchers and loops (tests/front_end_cases.py): im2col with three distinct extents and three distinct patch sizes from
fp16, bf16 and fp32 voxels, cells of fewer than 256 row groups and of more; gather with indices -1, n, 2^40 and -2^40 and a second
trip of its grid-stride loop; fill_rows with gaps between the slots and a second trip; score_gemv at E = 8 (one lane has work), E not
a multiple of 512, rows that leave waves of the last workgroup idle, with and without a bias; topk_sorted at every n around the
powers of two up to 8192 (64 KB of keys) on rows of ties, zeros of both signs, infinities, denormals, large negatives and NaNs of
both signs; pooling at every k up to 9 and around 16, 32, 64, with partly filled column groups, the second trip of the tail loop and
of the main loop, and the gates at every count of scales, with empty token slabs (k < 64), slabs of more than 8 tokens (k = 260)
and E = 8192, the gates' limit.

Data movement, the top-k order, scores of dyadic data and pooling of small integers are bit-exact.  The canonical top-k order
(oracle.canonical_topk): descending score, -0.0 == +0.0, ties by ascending index; every NaN, either sign bit, ranks first, above
+inf, ties among NaNs by ascending index.  Bounds are the first-order models of tests/test_front_end_bounds_host.py, which also shows
on the host that an emulation of each kernel stays inside them on these cases and that a kernel wrong in one of 22 named ways does
not.  Every buffer a kernel writes is pre-filled with a NaN bit pattern (the int64 index buffer with a sentinel integer), a guard
tail of 64 elements included, and compared as integers afterwards; every call runs twice and must repeat bit for bit; the first
case of every kernel also runs on the f16 build; refusals return U2TOK_ERR_ARG and leave the output untouched.  The worst
error / bound per kernel goes to the parity record under "front_end_error_over_bound", the wall time under "front_end_wall_s".
The preprocessing edges (u2tok_preprocess_volume through u2Transform.from_array) are held to the float64 reference and
preprocess_model of the host module; they found the one kernel change of this module besides the NaN key of topk_sorted: the
source index of the interpolation is now rounded to float before the weight is taken from it, as torch does (the compiler had
contracted product and subtraction into one fma; 3.24 x the bound at depth 33 -> 32).

First measured on the MI355X, worst error / bound: score_gemv 1.000 (an exact sum that IS a midpoint between two fp32 values,
rounded to even: half an ulp is the whole bound there; 0.5 on the f16 build's first case), multiscale_pool 0.996, gated 0.839 (the
f16 build at k = 7 and 17: 0.999 and 0.567; its first case, k = 1, is exact), preprocess 0.240 into fp32, 0.974 into bf16, 0.990
into fp16; no score excused; 81 tests, 1.7 s."""
import time

import pytest
import torch

import front_end_cases as K
import test_front_end_bounds_host as H
from oracle import u2_oracle as O
from suite_budget import record
from test_gpu_backward_ops import NAN32, guard_intact, nan16, nan32, ops, strided  # noqa: F401
from test_gpu_row_fwd_bounds import bits, call, canary

pytestmark = pytest.mark.gpu
D = "cuda"
GUARD = 64
BF16, F16 = H.BF16, H.F16

_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.monotonic()
    yield
    record("front_end_wall_s", round(time.monotonic() - t, 1))
    print(f"\ntests/test_gpu_front_end_bounds.py: {time.monotonic() - t:.1f} s; error / bound: {_RATIOS}")


def note(name, r):
    _RATIOS[name] = round(max(_RATIOS.get(name, 0.0), r), 4)
    record("front_end_error_over_bound", _RATIOS)
    print(f"{name}: error / bound = {r:.3f}")


def hold(name, got, ref, bound):
    """every element of got finite and within bound of ref; the worst ratio is printed and recorded before it is asserted"""
    err = (got.detach().double().cpu() - ref).abs()
    assert torch.isfinite(err).all(), f"{name}: non-finite elements (left unwritten?)"
    r = H.worst(err, bound)
    note(name, r)
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst ratio {r:.3f}; first at {i}: "
                             f"got {got[i].item()}, want {ref[i].item()} +- {bound[i].item()}")


def tag(el):
    return "" if el is BF16 else el.name + " "


def untouched(t):
    return bool((bits(t) == bits(canary(1))[0]).all())


def twice(run):
    """run() -> the written storage; called twice on fresh canaries, the two must agree bit for bit"""
    a, b = run(), run()
    assert torch.equal(bits(a), bits(b)), "the call does not repeat bit for bit"
    return a


def dev(t):
    return None if t is None else t.to(D)


def ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------------ im2col
def _im2col(ops, vol, patch, el=BF16, status=0, code=None, vol_off=0, out_off=0):
    n, Dd, Hh, Ww = vol.shape
    numel = vol.numel()
    v = vol.to(D)
    out = canary(numel + GUARD + 8, el)
    call(ops, "u2tok_im2col_patches", v.data_ptr() + vol_off, K.VOL_CODE[vol.dtype] if code is None else code, out.data_ptr() + out_off,
         n, Dd, Hh, Ww, *patch, status=status, el=el)
    return out, numel


def _im2col_check(ops, case, el=BF16):
    nchunk, dims, patch = case
    for dt in K.VOXEL_DTYPES:
        for fill in ("code", "mod"):
            vol = K.im2col_voxels(nchunk, dims, dt, fill)
            want = H.im2col_reference(vol, patch, el)
            out = twice(lambda: _im2col(ops, vol, patch, el)[0])
            assert untouched(out[want.numel():]), "im2col wrote past its output"
            got = out[:want.numel()].view(want.shape).cpu()
            if not torch.equal(bits(got), bits(want)):
                i = tuple((bits(got) != bits(want)).nonzero()[0].tolist())
                raise AssertionError(f"im2col {dt} {fill}: (chunk, token, feature) {i} holds {got[i].item()}, want {want[i].item()}")


@pytest.mark.parametrize("case", K.IM2COL_CASES, ids=["small", "production_patch", "33_groups"])
def test_im2col_is_the_einops_permutation(ops, case):
    """bit-equal to Rearrange("b c (h p1) (w p2) (d p3) -> b (h w d) (p1 p2 p3 c)") from fp16, bf16 and fp32 voxels rounded by torch,
    on voxels that encode their own (chunk, d, h, w) and on voxels that are exact in every type"""
    _im2col_check(ops, case)


def test_im2col_refusals_leave_the_output_alone(ops):
    """W or p3 no multiple of 8, D % p1 != 0, p1 p2 (2 W + 16) > 64 KB, a pointer 2 bytes off, an unknown dtype code"""
    f = torch.float16
    for dims, patch, kw in [((8, 6, 12), (4, 3, 4), {}), ((8, 6, 24), (4, 3, 12), {}), ((7, 6, 16), (4, 3, 8), {}),
                            ((4, 16, 512), (4, 16, 8), {}), ((8, 6, 16), (4, 3, 8), dict(vol_off=2)),
                            ((8, 6, 16), (4, 3, 8), dict(out_off=2)), ((8, 6, 16), (4, 3, 8), dict(code=3))]:
        out, _ = _im2col(ops, torch.ones(1, *dims, dtype=f), patch, status=-1, **kw)
        assert untouched(out), (dims, patch, kw)
    assert 4 * 16 * (2 * 512 + 16) > 64 * 1024 >= 4 * 16 * (2 * 504 + 16)
    out, numel = _im2col(ops, torch.ones(1, 4, 16, 504, dtype=f), (4, 16, 8))      # the widest row that fits is taken
    assert (out[:numel] == 1).all() and untouched(out[numel:])


# ------------------------------------------------------------------------------------------------------- gather, fill_rows
def _gather(ops, x, idx, el=BF16, status=0, over=()):
    B, n, E = x.shape
    k = idx.shape[1]
    xd, idd = x.to(D), idx.to(D)
    out = canary(B * k * E + GUARD, el)
    a = dict(B=B, n=n, k=k, E=E, x=xd.data_ptr(), out=out.data_ptr())
    a.update(dict(over))
    call(ops, "u2tok_gather_rows", a["x"], idd.data_ptr(), a["out"], a["B"], a["n"], a["k"], a["E"], status=status, el=el)
    return out


@pytest.mark.parametrize("B,n,k,E", K.GATHER_CASES + [K.GATHER_BIG])
def test_gather_rows_clamps_and_copies(ops, B, n, k, E):
    """out[b][j] = x[b][clamp(idx[b][j])] bit for bit with idx -1, n, 2^40 and -2^40 among duplicates; the last case has 1.0005 x
    8192 x 256 work items: the first 2048 threads of the capped grid take a second trip"""
    x, idx = K.gather_inputs(B, n, k, E)
    want = H.gather_reference(x, idx)
    out = twice(lambda: _gather(ops, x, idx))
    assert untouched(out[want.numel():]), "gather wrote past its output"
    assert torch.equal(bits(out[:want.numel()]).cpu().view(-1), bits(want).view(-1))


def test_gather_rows_refusals(ops):
    x, idx = K.gather_inputs(3, 7, 7, 8)
    assert untouched(_gather(ops, x, idx, status=-1, over=dict(E=12)))
    assert untouched(_gather(ops, x, idx, status=-1, over=dict(k=0)))
    assert untouched(_gather(ops, x, idx, status=-1, over=dict(n=0)))
    xd = torch.zeros(3 * 7 * 8 + 8, dtype=torch.bfloat16, device=D)
    assert untouched(_gather(ops, x, idx, status=-1, over=dict(x=xd.data_ptr() + 2)))


def _fill(ops, src, nb, n, dst_bs, el=BF16, status=0, null=None):
    total = (nb - 1) * dst_bs + n
    dst = canary(max(total, 1) + GUARD, el)
    s = src.to(D)
    call(ops, "u2tok_fill_rows", None if null == "src" else s.data_ptr(), None if null == "dst" else dst.data_ptr(), nb, n, dst_bs,
         status=status, el=el)
    return dst


def _fill_check(ops, nb, n, dst_bs, el=BF16):
    src = torch.randn(n, generator=H._gen(36, nb, n, dst_bs)).to(el.dtype)
    fill = bits(canary((nb - 1) * dst_bs + n + GUARD, el)).cpu()
    want = H.fill_reference(bits(src), nb, n, dst_bs, fill)
    dst = twice(lambda: _fill(ops, src, nb, n, dst_bs, el))
    assert torch.equal(bits(dst).cpu(), want), "fill_rows: a slot differs, or a gap or the tail lost its canary"


@pytest.mark.parametrize("nb,n,dst_bs", K.FILL_CASES + [K.FILL_BIG])
def test_fill_rows_broadcasts_into_strided_slots(ops, nb, n, dst_bs):
    """dst[b dst_bs + e] = src[e] bit for bit; the 5-element gaps between the slots and the tail keep their canary; the last case
    has 17 elements more than 4096 x 256: a second trip of the grid-stride loop"""
    _fill_check(ops, nb, n, dst_bs)


def test_fill_rows_refusals(ops):
    src = torch.ones(8, dtype=torch.bfloat16)
    for kw in (dict(nb=0, n=8), dict(nb=1, n=0), dict(nb=1, n=8, null="src")):
        assert untouched(_fill(ops, src, kw["nb"], kw["n"], 8, status=-1, null=kw.get("null")))
    _fill(ops, src, 1, 8, 8, status=-1, null="dst")


# ------------------------------------------------------------------------------------------------------------------- score
def _score(ops, inp, el=BF16, status=0, over=()):
    rows, E = inp["x"].shape
    x, w, b = dev(inp["x"]), dev(inp["w"]), dev(inp["bias"])
    s = nan32(rows + GUARD)
    a = dict(rows=rows, E=E, x=x.data_ptr())
    a.update(dict(over))
    call(ops, "u2tok_score_gemv", a["x"], w.data_ptr(), ptr(b), s.data_ptr(), a["rows"], a["E"], status=status, el=el)
    return s


def _score_check(ops, rows, E, with_bias, kind, el=BF16):
    inp = K.score_inputs(rows, E, with_bias, kind, el.dtype)
    m = H.score_model(**inp)
    s = twice(lambda: _score(ops, inp, el))
    assert (s[rows:].view(torch.int32) == NAN32).all(), "score_gemv wrote past its rows"
    got = s[:rows].cpu()
    if kind == "dyadic":
        assert torch.equal(got.view(torch.int32), m["want"].view(torch.int32)), (rows, E, with_bias, got, m["want"])
        return 0
    r, excused = H.score_check(got, m)
    note(tag(el) + "score_gemv", r)
    return excused


@pytest.mark.parametrize("E", sorted({c[1] for c in K.SCORE_CASES}))
def test_score_gemv_is_the_exact_sum_rounded_once(ops, E):
    """rows 1, 3, 4, 5, 9 with and without a bias.  Dyadic data: bit-equal to integer arithmetic.  N(0, 1) and cancelling rows: within
    half an fp32 ulp + E 2^-53 sum|terms| of math.fsum over the exact products, bit-equal away from rounding boundaries; at most 1 % of
    the scores excused as near one (none of the N(0, 1) ones: tests/test_front_end_bounds_host.py)"""
    n, excused = 0, 0
    for rows, E_, with_bias in K.SCORE_CASES:
        if E_ != E:
            continue
        for kind in K.SCORE_KINDS:
            ex = _score_check(ops, rows, E, with_bias, kind)
            if kind != "dyadic":
                n, excused = n + rows, excused + ex
    assert n == 2 * 2 * 22 and excused <= H.EXCUSED_SHARE * n, (excused, n)


def test_score_gemv_refusals(ops):
    inp = K.score_inputs(3, 8, True, "normal")
    for kw in (dict(E=12), dict(rows=0), dict(E=0)):
        s = _score(ops, inp, status=-1, over=kw)
        assert (s.view(torch.int32) == NAN32).all()
    xd = torch.zeros(64, dtype=torch.bfloat16, device=D)
    s = _score(ops, inp, status=-1, over=dict(x=xd.data_ptr() + 2))
    assert (s.view(torch.int32) == NAN32).all()


# ------------------------------------------------------------------------------------------------------------------- top-k
def _topk(ops, scores, k, el=BF16, status=0, over=()):
    B, n = scores.shape
    s = scores.to(D)
    idx = torch.full((B * max(k, 1) + GUARD,), H.SENTINEL, dtype=torch.int64, device=D)
    a = dict(B=B, n=n, k=k)
    a.update(dict(over))
    call(ops, "u2tok_topk_sorted", s.data_ptr(), idx.data_ptr(), a["B"], a["n"], a["k"], status=status, el=el)
    return idx


def _topk_check(ops, n, el=BF16):
    for mix, kinds in enumerate(K.TOPK_MIXES):
        s = K.topk_scores(n, mix)
        for k in K.ks_of(n):
            want = O.canonical_topk(s, k)
            a, b = _topk(ops, s, k, el), _topk(ops, s, k, el)
            assert torch.equal(a, b), "topk_sorted does not repeat"
            assert (a[K.TOPK_B * k:] == H.SENTINEL).all(), "topk_sorted wrote past its k indices"
            got = a[:K.TOPK_B * k].view(K.TOPK_B, k).cpu()
            for r, kind in enumerate(kinds):
                if not torch.equal(got[r], want[r]):
                    j = int((got[r] != want[r]).nonzero()[0])
                    raise AssertionError(f"topk n={n} k={k} row '{kind}': rank {j} is index {int(got[r, j])} (score {s[r, int(got[r, j]) % n]}), "
                                         f"want {int(want[r, j])} (score {s[r, int(want[r, j])]})")


@pytest.mark.parametrize("n", K.TOPK_NS)
def test_topk_is_the_canonical_order(ops, n):
    """k = 1, n // 2 and n against oracle.canonical_topk on rows that are all equal, of four values, ascending, descending, zeros of both
    signs, with infinities, denormal, large negative (the padding keys of a non-power-of-two n stay behind them) and with NaNs of both
    signs, which rank first by ascending index"""
    _topk_check(ops, n)


def test_topk_refusals(ops):
    s = torch.zeros(1, 8193)
    for kw in (dict(n=8193, k=4), dict(n=8, k=9), dict(n=8, k=0)):
        idx = _topk(ops, s, 4, status=-1, over=kw)
        assert (idx == H.SENTINEL).all(), kw
    idx = _topk(ops, s[:, :8192], 4)
    assert (idx[4:] == H.SENTINEL).all() and idx[:4].tolist() == [0, 1, 2, 3]


def test_score_topk_gather_chain(ops):
    """score -> top-k -> gather at B = 2, 8 x 33 tokens, E = 520, k = 100 against oracle.token_selection: the same 100 indices in the
    same order, the same rows bit for bit"""
    c = K.CHAIN
    x, w, b = K.chain_inputs()
    sd = {"s.score_net.weight": w.double(), "s.score_net.bias": b.double()}
    tok, idx = O.token_selection(sd, "s", x.double(), c["k"])
    flat = x.reshape(c["B"], c["T"] * c["N"], c["E"])
    s = _score(ops, dict(x=flat.reshape(-1, c["E"]), w=w.reshape(-1), bias=b))[:flat.shape[0] * flat.shape[1]]
    got_idx = _topk(ops, s.view(c["B"], -1).cpu(), c["k"])[:c["B"] * c["k"]].view(c["B"], c["k"]).cpu()
    assert torch.equal(got_idx, idx)
    out = _gather(ops, flat, got_idx)[:tok.numel()].view(tok.shape).cpu()
    assert torch.equal(out.double(), tok)


# ----------------------------------------------------------------------------------------------------------------- pooling
def _pool(ops, inp, el=BF16, status=0):
    x = inp["x"]
    B, k, E = x.shape
    L = k + k // 2 + k // 4
    xd, gw, gb = x.to(D), dev(inp["gate_w"]), dev(inp["gate_b"])
    out = canary(B * L * E + GUARD, el)
    nws = B * 3 * 16 * (-(-E // 256)) * 4
    ws = nan32(nws // 4 + GUARD) if gw is not None else None
    call(ops, "u2tok_multiscale_pool", xd.data_ptr(), out.data_ptr(), B, k, E, ptr(gw), ptr(gb), ptr(ws), status=status, el=el)
    if ws is not None:
        assert guard_intact(ws, nws), "the gate kernel wrote past its workspace"
    return out


def _pool_exact(ops, case, el=BF16, work=torch.float64):
    B, k, E = case
    inp = K.pool_inputs(B, k, E, True, dtype=el.dtype)
    want = O.multi_scale_pool(None, None, inp["x"].to(work)).to(el.dtype)
    out = twice(lambda: _pool(ops, inp, el))
    assert untouched(out[want.numel():]), "multiscale_pool wrote past its rows"
    got = out[:want.numel()].view(want.shape).cpu()
    if not torch.equal(bits(got), bits(want)):
        i = tuple((bits(got) != bits(want)).nonzero()[0].tolist())
        raise AssertionError(f"multiscale_pool {case}: (b, row, column) {i} holds {got[i].item()}, want {want[i].item()}")


def _pool_hold(ops, case, gated, el=BF16):
    B, k, E = case
    inp = K.pool_inputs(B, k, E, False, gated, el.dtype)
    m = H.multiscale_gate_model(inp["x"], inp["gate_w"], inp["gate_b"], el)
    out = twice(lambda: _pool(ops, inp, el))
    assert untouched(out[m["out"].numel():]), "multiscale_pool wrote past its rows"
    hold(tag(el) + ("multiscale_pool gated" if gated else "multiscale_pool"), out[:m["out"].numel()].view(m["out"].shape), m["out"],
         m["bound"])


@pytest.mark.parametrize("E", [8, 264, 512])
def test_fixed_pooling_is_exact_on_small_integers_and_rounds_once(ops, E):
    """k = 1 .. 9, 15, 16, 17, 30, 31, 64 without gates: integers up to 15 come back as the oracle's means bit for bit (every sum and
    every division by 2 or 4 is exact); N(0, 1) data within one rounding of the float64 mean, U |ref| plus the fp32 sum of up to four
    terms"""
    for case in K.POOL_FIXED_CASES:
        if case[2] == E:
            _pool_exact(ops, case)
            _pool_hold(ops, case, False)


def test_pooling_loops_second_trips(ops):
    """k = 3 at E = 8192: 4 tail rows x 1024 column groups on 4 workgroups, four trips of the tail loop; k = 4100 at E = 4096, B = 1:
    1025 x 512 items on the capped grid of 2048 x 256 threads, a second trip of the main loop (integers: the fp32 oracle is exact)"""
    _pool_exact(ops, K.POOL_TAIL_BIG)
    _pool_hold(ops, K.POOL_TAIL_BIG, False)
    _pool_exact(ops, K.POOL_MAIN_BIG, work=torch.float32)


@pytest.mark.parametrize("E", [264, 512, 8192])
def test_gated_pooling_stays_inside_the_gate_model(ops, E):
    """k = 1, 2, 3 (the softmax over one and two scales), 4, 5, 7, 17, 64 (token slabs empty or of one token), 130, 260 (a slab's loop
    takes more than one trip) with B = 2 against oracle.multi_scale_pool in double, within multiscale_gate_model's bound"""
    for case in K.POOL_GATED_CASES:
        if case[2] == E:
            _pool_hold(ops, case, True)


def test_gated_pooling_refuses_E_8200(ops):
    inp = K.pool_inputs(1, 4, 8200, False, True)
    assert untouched(_pool(ops, inp, status=-1))
    inp["gate_w"] = inp["gate_b"] = None
    out = _pool(ops, inp)                                   # without gates the width is taken
    assert untouched(out[7 * 8200:]) and torch.isfinite(out[:7 * 8200].float()).all()


# ------------------------------------------------------------------------------------------------------------ preprocessing
def _pre_run(c, dt):
    """u2Transform.from_array twice -> (voxels (pad, T, T) on the CPU, info as preprocess_info_equal takes it)"""
    from u2tokenizer_amd.preprocess import u2Transform
    tr = u2Transform(device=D, out_dtype=dt)
    aug = dict(rot90_k=c["rot90_k"]) if c["rot90_k"] else None
    runs = []
    for _ in range(2):
        out = tr.from_array(c["vol"], c["T"], c["pad"], aug=aug)
        torch.cuda.synchronize()
        assert out.shape == (c["pad"] // 32, 32, c["T"], c["T"]) and out.dtype == dt
        runs.append((out.cpu().reshape(c["pad"], c["T"], c["T"]), tr.last_info.cpu()))
    (out, info), (out2, info2) = runs
    assert torch.equal(bits(out), bits(out2)) and torch.equal(info[:1], info2[:1]) and torch.equal(info[10:], info2[10:])
    pct = info[10:12].view(torch.float32).numpy()
    return out, dict(status=int(info[0]), lo=info[1:4].tolist(), hi=info[4:7].tolist(), out_size=info[7:10].tolist(), a_min=pct[0],
                     a_max=pct[1])


@pytest.mark.parametrize("name", sorted(K.PREPROCESS_CASES))
def test_preprocess_edges(ops, name):
    """u2tok_preprocess_volume on volumes of at most 32^3 voxels (front_end_cases.preprocess_cases) against the float64 reference of
    the host module: status, crop box, resized size and both percentiles (np.percentile, as float32) exact; the voxels within
    preprocess_model's bound; everything outside the resized block exactly zero; without a foreground (status 1) and with a filter
    wider than 16 taps per side (status 2: a crop more than 9.25 x its resized extent) the whole output is zero, and status 2 still
    reports box and size (u2tokenizer_amd/preprocess.py).  A crop that already has the target size comes back as the scaled crop
    rounded once to the output type, bit for bit, in all three output types."""
    c = K.PREPROCESS_CASES[name]
    for dt in c["dtypes"]:
        m = H.preprocess_model(c["vol"], c["T"], c["pad"], c["rot90_k"], dt)
        out, info = _pre_run(c, dt)
        assert H.preprocess_info_equal(info, m), (info, {k: m[k] for k in info})
        if m["status"] != 0:
            assert (out == 0).all()
            continue
        od, oh, ow = m["out_size"]
        assert (out[od:] == 0).all() and (out[:, oh:] == 0).all() and (out[:, :, ow:] == 0).all()
        hold("preprocess" + ("" if dt == torch.float32 else " " + H.OUT_ELEMS[dt].name), out, m["out"], m["bound"])
        if name == "geo_exact":
            assert torch.equal(bits(out[:od, :oh, :ow]), bits(m["crop"].to(dt))), "the crop of the target size is not passed through"


# ------------------------------------------------------------------------------------------------------------- f16 build
def test_first_case_of_every_kernel_on_the_f16_build(ops):
    el = F16
    _im2col_check(ops, K.IM2COL_CASES[0], el)
    B, n, k, E = K.GATHER_CASES[0]
    x, idx = K.gather_inputs(B, n, k, E, el.dtype)
    want = H.gather_reference(x, idx)
    assert torch.equal(bits(_gather(ops, x, idx, el)[:want.numel()]).cpu().view(-1), bits(want).view(-1))
    _fill_check(ops, *K.FILL_CASES[0], el=el)
    rows, E, with_bias = K.SCORE_CASES[0]
    for kind in K.SCORE_KINDS:
        _score_check(ops, rows, E, with_bias, kind, el)
    _topk_check(ops, K.TOPK_NS[0], el)
    _pool_exact(ops, K.POOL_FIXED_CASES[0], el)
    _pool_hold(ops, K.POOL_FIXED_CASES[0], False, el)
    _pool_hold(ops, K.POOL_GATED_CASES[0], True, el)
    for case in ((2, 7, 264), (2, 17, 264)):               # the first cases have k = 1 (one scale, exact): two with all three scales
        assert case in K.POOL_FIXED_CASES and case in K.POOL_GATED_CASES
        _pool_exact(ops, case, el)
        _pool_hold(ops, case, False, el)
        _pool_hold(ops, case, True, el)
