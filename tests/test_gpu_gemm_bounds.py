"""GPU: the forward GEMM kernels -- gemm_bf16_nt_kernel (gemm.hip: 64 / 128 tiles, K-major and K-tile-major operands, split-K and its
reduce), gemm_rows16_kernel (gemm_rows.hip), gemm_skinny64_kernel (gemm_skinny.hip), gemm_bt_kernel and gemm_bt_drain_kernel
(gemm_bt.hip: variants 20 / 21 / 22 / 24 / 26 / 27, sliced, pair, with the in-launch tail and the V^T side output) -- element by
element against float64, at the smallest shapes that reach each instantiation (tests/gemm_cases.py; tests/test_gemm_plan.py pins
every case's route) with K swept over the entries and exits of every K loop: both parities of the two-stage loop with and without a
K tail, 8 to 11 K tiles of the skinny kernel's three stages, 2 to 13 K tiles of the big tiles' rings with a persistent workgroup
chaining three or more tiles (gemm_big_grid 2), the drain form's exit behind its twelfth body and the run-on, uneven K slices.

The bound is gemm_cases.model's: first order, derived, proved on the host by tests/test_gemm_bounds_host.py, which also shows that a
kernel wrong in one of 13 named ways leaves it on a case of these tables.  On integer data every fp32 output equals the float64
product bit for bit and every element-type output that value rounded once.  Every C lies in NaN-filled storage with ldc > N, a
nonzero offset, batch gaps and a guard tail, compared as integers afterwards: everything outside the product untouched, everything
inside finite; the gaps between the batch entries of A and B hold NaNs too.  Every case runs twice and must repeat bit for bit; the
first case of every form also runs on the f16 build.  Options are restored in `finally`.

Part 3: the column split and the V^T side output of the ViT's q|k|v product through u2tok_gemm_bf16_ex (ops.gemm_ex) -- scaled
columns within the bound, V^T bit-equal to transpose_bf16(perm16 = 1) of the plain product's V columns, sentinels in the V columns
of C's patch rows, the cls rows whole; the split alone on every other form, once on the sliced ones.

The worst error / bound per form goes to the parity record under "gemm_error_over_bound", the module's wall time under "gemm_wall_s".
First measured on the MI355X (bf16 and the f16 first cases together): tile64 0.991, tile64_bk 0.987, tile64_abk 0.984, tile64_ktile
0.975, tile128 0.995, tile128_bk 0.979, tile128_abk 0.987, tile128_ktile 0.962, tile128_splitk 0.908, tile64_splitk 0.899, rows16
0.934, rows16_pair 0.613, skinny 0.908, big20 0.982, big21 0.981, big22 0.985, big24 0.984, big26 0.990, big20_sliced 0.940,
big21_sliced 0.941, big22_sliced 0.941, drain27 0.938, heuristic_tail 0.913, big21_pair 0.815, qkv_drain_tail 0.909, qkv_drain 0.928,
qkv_deep_tail 0.976, qkv_nodrain 0.908, qkv_tail_unfused 0.907, split_tile64 0.920, split_skinny 0.940, split_rows16 0.976,
split_tile_splitk 0.843, split_big_sliced 0.900; 6 s.  No kernel of the parent commit left its bound.  A ratio just under 1 is a
correctly rounded result on the worst-placed element (the host module's docstring), not a near miss: the kernels reach what the
host emulation reaches, to the third digit."""
import time

import pytest
import torch

import gemm_cases as G
from gemm_cases import BF16, F16
from suite_budget import record
from test_gpu_backward_ops import NAN16, NAN32, ops  # noqa: F401

pytestmark = pytest.mark.gpu
D = "cuda"
GUARD = 64
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.monotonic()
    yield
    record("gemm_wall_s", round(time.monotonic() - t, 1))
    print(f"\ntests/test_gpu_gemm_bounds.py: {time.monotonic() - t:.1f} s; error / bound: {_RATIOS}")


def canary(n, dtype):
    if dtype == torch.float32:
        return torch.full((n,), NAN32, dtype=torch.int32, device=D).view(torch.float32)
    return torch.full((n,), NAN16, dtype=torch.int16, device=D).view(dtype)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def hold(name, got, ref, bound):
    """every element of got finite and within bound of ref; the worst ratio is printed and recorded before it is asserted"""
    err = (got.detach().double().cpu() - ref).abs()
    assert torch.isfinite(err).all(), f"{name}: non-finite elements (left unwritten, or a pad was read?)"
    r = G.worst(err, bound)
    key = name.split(" ")[0]
    _RATIOS[key] = round(max(_RATIOS.get(key, 0.0), r), 4)
    record("gemm_error_over_bound", _RATIOS)
    print(f"{name}: error / bound = {r:.3f}")
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst ratio {r:.3f}; first at {i}: "
                             f"got {got[i].item()}, want {ref[i].item()} +- {bound[i].item()}")
    return r


def _place(mats, ld, bs, dtype, kmajor=False):
    """NaN storage holding the batch entries' matrices (nz, rows, cols) -- transposed if kmajor -- at row stride ld, batch stride bs"""
    if kmajor:
        mats = mats.transpose(1, 2)
    nz, rows, cols = mats.shape
    st = canary((nz - 1) * bs + (rows - 1) * ld + cols + GUARD, dtype)
    for z in range(nz):
        torch.as_strided(st, (rows, cols), (ld, 1), z * bs).copy_(mats[z].to(D))
    return st


class Run:
    """one product of the tables on the GPU: storages, the launch (twice, bit-repeatable), the sentinel check, the output"""

    def __init__(self, ops, form, desc, data, el=BF16, overrides=None, drop_vt=False):
        self.ops, self.form, self.desc, self.data, self.el = ops, form, desc, data, el
        p = self.p = G.parse(desc)
        if drop_vt:
            p.pop("vt", None)
        self.opts = dict(G.options(p), **(overrides or {}))
        self.inp = G.inputs(form, p, data, el)
        self.flags = p.get("flags", 0)
        self.name = f"{form} {'' if el is BF16 else el.name + ' '}[{desc}] {data}"

    def launch(self):
        p, ops, el, inp, flags = self.p, self.ops, self.el, self.inp, self.flags
        M, N, K, nz = p["M"], p["N"], p["K"], p.get("nz", 1)
        ta, tb, f32, pair = bool(flags & G.A_KMAJOR), bool(flags & G.B_KMAJOR), bool(flags & G.OUT_F32), bool(flags & G.SWIGLU)
        lda, ldb, ldc = (M if ta else K), (N if tb else K), p["ldc"]
        sAb, sBb, sCb, c_off = p.get("sAb", 0), p.get("sBb", 0), p.get("sCb", 0), p["c_off"]
        Nc = N // 2 if pair else N
        a_st = _place(inp["A"], lda, sAb, el.dtype, ta)
        if p.get("ktile"):
            b_st, api_flags = ops.pack_ktile_major(inp["B"][0].contiguous()).to(D), flags | G.B_KTILE
        else:
            b_st, api_flags = _place(inp["B"], ldb, sBb, el.dtype, tb), flags
        bias = None if inp["bias"] is None else inp["bias"].to(D)
        res = None if inp["R"] is None else inp["R"].contiguous().to(D)
        cdt = torch.float32 if f32 else el.dtype
        self.c_st = canary(c_off + (nz - 1) * sCb + (M - 1) * ldc + Nc + GUARD, cdt)
        self.idx = c_off + torch.arange(nz)[:, None, None] * sCb + torch.arange(M)[None, :, None] * ldc + torch.arange(Nc)[None, None, :]
        self.vt_st = None
        kw = {}
        if "vt" in p:
            n0, rows = p["vt"]
            self.vt_ld, self.vt_bs, self.chunks = rows + 8, (N - n0) * (rows + 8) + 16, (M // 256 * 256) // rows
            self.vt_st = canary(8 + self.chunks * self.vt_bs + GUARD, el.dtype)
            kw = dict(vt=self.vt_st, vt_n0=n0, vt_rows=rows, vt_ld=self.vt_ld, vt_bs=self.vt_bs, vt_off=8)
        scratch = torch.empty(p["scratch"], dtype=torch.uint8, device=D) if "scratch" in p else None
        outs = []
        try:
            for k, v in self.opts.items():
                ops.set_option(k, v)
            ops.set_gemm_scratch(scratch)
            for _ in range(2):
                bits(self.c_st).fill_(NAN32 if f32 else NAN16)
                if "nsplit" in p or "vt" in p or self.form.startswith("ex_"):
                    ops.gemm_ex(a_st, b_st, self.c_st, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, ldr=N, nz=nz, sAb=sAb, sBb=sBb, sCb=sCb,
                                sRb=M * N if res is not None else 0, alpha=p.get("alpha", 1.0), flags=api_flags, bias=bias, residual=res,
                                c_off=c_off, nsplit=p.get("nsplit", 0), alpha_lo=G.ALPHA_LO if "nsplit" in p else 1.0, **kw)
                else:
                    anchor = torch.empty(1, dtype=el.dtype, device=D)
                    with ops.on_device(anchor, el.dtype) as (h, st):
                        got = h.u2tok_gemm_bf16(a_st.data_ptr(), b_st.data_ptr(), self.c_st.data_ptr() + self.c_st.element_size() * c_off,
                                                None if bias is None else bias.data_ptr(), None if res is None else res.data_ptr(),
                                                M, N, K, lda, ldb, ldc, N, nz, 1, sAb, 0, sBb, 0, sCb, 0, M * N if res is not None else 0,
                                                0, p.get("alpha", 1.0), api_flags, st)
                    assert got == 0, (self.name, got)
                torch.cuda.synchronize()
                outs.append((self.c_st.cpu(), None if self.vt_st is None else self.vt_st.cpu()))
        finally:
            for k in self.opts:
                ops.set_option(k, G.OPTION_DEFAULTS[k])
            ops.set_gemm_scratch(None)
            torch.cuda.synchronize()
        assert torch.equal(bits(outs[0][0]), bits(outs[1][0])), f"{self.name}: two launches differ"
        if self.vt_st is not None:
            assert torch.equal(bits(outs[0][1]), bits(outs[1][1])), f"{self.name}: two launches differ in V^T"
            self.vt = outs[0][1]
        self.c = outs[0][0]
        return self

    def written(self, idx=None):
        """C at the flat indices (default: the whole product), after checking that nothing outside them was touched"""
        idx = self.idx if idx is None else idx
        out = torch.ones(self.c.numel(), dtype=torch.bool)
        out[idx.reshape(-1)] = False
        sent = NAN32 if self.c.dtype == torch.float32 else NAN16
        n = int((bits(self.c)[out] != sent).sum())
        assert n == 0, f"{self.name}: {n} sentinel elements overwritten outside the product"
        return self.c[idx]

    def check(self, got=None, rows=None, cols=None):
        """got (default: the whole product) within the bound -- restricted to rows / cols --, exact on integer data"""
        m = G.model(self.p, **self.inp, el=self.el)
        got = self.written() if got is None else got
        ref, bound, exact = m["ref"], m["bound"], m["exact"]
        if rows is not None:
            ref, bound = ref[:, rows], bound[:, rows]
        if cols is not None:
            ref, bound = ref[..., cols], bound[..., cols]
            exact = exact if exact is False else exact[cols]
        r = hold(self.name, got, ref, bound)
        if self.data == "ints" and exact is not False:
            want = G.round_once(ref, self.flags, self.el)
            assert torch.equal(got[..., exact], want[..., exact]), f"{self.name}: integer data, not the float64 value rounded once"
        return r


def cases_of(form):
    return [(f, d, ds) for f, d, ds in G.ALL_CASES if f == form]


BOUND_FORMS = [f for f in G.FORMS if any(f == c[0] for c in G.BOUND_CASES)]


@pytest.mark.parametrize("form", BOUND_FORMS)
def test_gemm_form_within_bound(ops, form):
    """Every case and data set of the form: bit-repeatable, nothing outside the product written, every element within the bound, the
    integer data exact; the first case on the f16 build too.  Tile kernels: gemm_mubuf 0 gives gemm_mubuf 1's bits."""
    for i, (f, d, datas) in enumerate(cases_of(form)):
        for data in datas:
            for el in ((BF16, F16) if i == 0 else (BF16,)):
                run = Run(ops, f, d, data, el).launch()
                run.check()
                if form.startswith("tile") and data == "normal":
                    flat = Run(ops, f, d, data, el, overrides={"gemm_mubuf": 0}).launch()
                    assert torch.equal(bits(flat.c), bits(run.c)), f"{run.name}: gemm_mubuf 0 and 1 differ"


def test_skinny_flat_and_mubuf_pieces_agree(ops):
    """gemm_skinny 1 (FLAT-encoded LDS-DMA pieces) and 2 (buffer_load ... lds) give the same bits at every K phase of the three stages"""
    sk = cases_of("skinny")
    pairs = [(a, b) for a in sk for b in sk if b[1] == a[1] + " gemm_skinny=1"]
    assert len(pairs) == 4
    for (f, d2, datas), (_, d1, _) in pairs:
        for data in datas:
            assert torch.equal(bits(Run(ops, f, d2, data).launch().c), bits(Run(ops, f, d1, data).launch().c)), (d2, data)


@pytest.mark.parametrize("K", G.DRAIN_K)
def test_drain_form_equals_the_deep_form(ops, K):
    """Variant 27 (tile i's epilogue under tile i + 1's K loop) against variant 24 on the same product: plain, bias and alpha bit for
    bit; its GELU = gelu_fwd of variant 24's stored pre-activation (gelu_epi's contract) bit for bit."""
    wrong = []
    for f, d, datas in cases_of("drain27"):
        if f"K={K} " not in d:
            continue
        for data in datas:
            drain = Run(ops, f, d, data).launch()
            flags = drain.flags
            deep = Run(ops, f, d.replace(f"flags={flags:#x}", f"flags={flags & ~G.GELU:#x}"), data, overrides={"gemm_big": 24})
            deep.inp = drain.inp                      # (the data are seeded by the flags too)
            deep.launch()
            want = deep.c
            if flags & G.GELU:
                want = deep.c.clone()
                want[deep.idx] = ops.gelu_fwd(deep.c[deep.idx].to(D)).cpu()
            diff = (bits(drain.c) != bits(want)).nonzero().flatten()
            if diff.numel():
                pre = deep.c[diff[:8]].tolist()
                wrong.append(f"{drain.name}: {diff.numel()} elements differ from variant 24; pre-activation {pre}: got "
                             f"{drain.c[diff[:8]].tolist()} ({bits(drain.c)[diff[:8]].tolist()}), want {want[diff[:8]].tolist()} "
                             f"({bits(want)[diff[:8]].tolist()})")
    assert not wrong, "\n".join(wrong)


def test_tail_in_launch_equals_tail_launch(ops):
    """the 2 cls rows behind 512 patch rows: computed in the big-tile launch (gemm_tail_fused 1) or by a few-rows launch (0), same bits"""
    ht = cases_of("heuristic_tail")
    for f, d, datas in ht:
        if "gemm_tail_fused" in d:
            continue
        for data in datas:
            a, b = Run(ops, f, d, data).launch(), Run(ops, f, d + " gemm_tail_fused=0", data).launch()
            assert torch.equal(bits(a.c), bits(b.c)), (d, data)


# ------------------------------------------------------------------------------------------ the column split and V^T (u2tok_gemm_bf16_ex)
QKV_FORMS = [f for f in G.FORMS if f.startswith("qkv_")]
SPLIT_FORMS = [f for f in G.FORMS if f.startswith("split_")]


@pytest.mark.parametrize("form", QKV_FORMS)
def test_qkv_split_and_transposed_v(ops, form):
    """The ViT's q|k|v product as pipeline.hip issues it (nsplit 192, alpha_lo = 0.125 log2 e, vt_n0 384, vt_rows 256; 2 cls rows):
    (a) the q and k columns of every row within the bound, q scaled by alpha_lo, exact on the integer data's k columns;
    (b) vt[chunk][n - 384][perm16(key)] = transpose_bf16(perm16 = 1) of the V columns of the same product without vt, bit for bit,
        the pads of its rows (vt_ld = vt_rows + 8), the gaps between chunks and its tail untouched;
    (c) the V columns of C's patch rows keep their sentinels;  (d) the cls rows are whole in C, V columns included."""
    for f, d, data, el in [(f, d, data, el) for i, (f, d, datas) in enumerate(cases_of(form)) for data in datas
                           for el in ((BF16, F16) if i == 0 else (BF16,))]:
        run = Run(ops, f, d, data, el).launch()
        p = run.p
        M, N, (n0, rows) = p["M"], p["N"], p["vt"]
        Mt = M // 256 * 256
        patch_qk = run.idx[:, :Mt, :n0]
        cls = run.idx[:, Mt:, :]
        run.written(torch.cat([patch_qk.reshape(-1), cls.reshape(-1)]))                  # (c), and nothing outside C's product
        run.check(run.c[patch_qk], rows=slice(0, Mt), cols=slice(0, n0))                # (a)
        if M > Mt:
            run.check(run.c[cls], rows=slice(Mt, M))                                     # (d)
        plain = Run(ops, f, d, data, el, drop_vt=True).launch()
        full = plain.written()[0]
        assert torch.equal(bits(full[:, :n0]), bits(run.c[run.idx[0, :, :n0]])), f"{run.name}: q | k columns differ from the product without vt"
        V = full[:Mt, n0:].reshape(run.chunks, rows, N - n0).to(D)
        want = ops.transpose(V, perm16=True).cpu()                                        # (chunks, N - n0, rows)
        vidx = 8 + torch.arange(run.chunks)[:, None, None] * run.vt_bs + torch.arange(N - n0)[None, :, None] * run.vt_ld + torch.arange(rows)
        outside = torch.ones(run.vt.numel(), dtype=torch.bool)
        outside[vidx.reshape(-1)] = False
        assert bool((bits(run.vt)[outside] == NAN16).all()), f"{run.name}: V^T written outside its chunks"
        assert torch.equal(bits(run.vt[vidx]), bits(want)), f"{run.name}: V^T is not the transposed V of the plain product"
        host = want[:, :, G.perm16(rows)].transpose(1, 2).reshape(Mt, N - n0)             # perm16 is its own inverse
        assert torch.equal(bits(host), bits(full[:Mt, n0:])), "transpose_bf16(perm16 = 1) is not the flash key order"


@pytest.mark.parametrize("form", SPLIT_FORMS)
def test_column_split_on_every_form(ops, form):
    """columns below nsplit scaled by alpha_lo, the others by alpha, within the bound on every form that applies the split -- the tile
    kernel, its split-K reduce, the skinny kernel, the few-rows kernel, the sliced big tile (where the slices must not scale twice)"""
    for i, (f, d, datas) in enumerate(cases_of(form)):
        for data in datas:
            for el in ((BF16, F16) if i == 0 else (BF16,)):
                Run(ops, f, d, data, el).launch().check()


def test_gemm_ex_neutral_is_gemm(ops):
    """u2tok_gemm_bf16_ex with nsplit 0, alpha_lo 1 and vt NULL gives u2tok_gemm_bf16's bits: a tile, a skinny and a big-tile product"""
    picks = [("tile64", "K=136 "), ("skinny", "K=1152 ldc"), ("big24", "M=300 N=200 K=448 ldc=208 c_off=8 flags=0x9")]
    for form, has in picks:
        f, d, _ = next(c for c in cases_of(form) if has in c[1])
        base = Run(ops, f, d, "normal").launch()
        ex = Run(ops, "ex_" + f, d, "normal")
        ex.inp = base.inp
        assert torch.equal(bits(ex.launch().c), bits(base.c)), d


def test_gemm_ex_refuses_what_the_kernels_cannot_take(ops):
    """vt on a route without the transposed form, a misaligned or short vt: U2TOK_ERR_ARG, nothing launched"""
    f, d, _ = cases_of("qkv_drain")[0]
    p = G.parse(d)
    M, N, K = p["M"], p["N"], p["K"]
    a, b = torch.zeros(M * K, dtype=torch.bfloat16, device=D), torch.zeros(N * K, dtype=torch.bfloat16, device=D)
    c, vt = canary(M * N, torch.bfloat16), canary(2 * 192 * 256 + 64, torch.bfloat16)
    good = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, nsplit=192, alpha_lo=G.ALPHA_LO, vt=vt, vt_n0=384, vt_rows=256, vt_ld=256, vt_bs=192 * 256)
    bad = [dict(vt_off=4), dict(vt_ld=248), dict(vt_ld=260), dict(vt_bs=192 * 256 - 8), dict(vt_n0=400), dict(vt_rows=128), dict(nsplit=576),
           dict(flags=G.BIAS_N, bias=torch.zeros(N, dtype=torch.bfloat16, device=D)), dict(M=200), dict(nsplit=8)]
    try:
        ops.set_option("gemm_big_grid", 2)
        for kw in bad:
            with pytest.raises(RuntimeError, match="U2TOK_ERR_ARG"):
                ops.gemm_ex(a, b, c, **dict(good, **kw))
        ops.set_option("gemm_big", 24)
        with pytest.raises(RuntimeError, match="U2TOK_ERR_ARG"):
            ops.gemm_ex(a, b, c, **good)
    finally:
        ops.set_option("gemm_big_grid", 256)
        ops.set_option("gemm_big", 0)
    torch.cuda.synchronize()
    assert bool((bits(c) == NAN16).all()) and bool((bits(vt) == NAN16).all())
