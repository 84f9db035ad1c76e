"""Host: the bound that tests/test_gpu_enc_attn_bounds.py holds the encoder attention forwards to (tests/enc_attn_cases.py) is
(1) kept by the emulation of the kernels' rounding points on every case of every sweep, in both element types, against the exact row
max and against each stale one the kernels can run at (8 log2 units for tok_attn_kernel / tok_attn2_kernel and flash mode 1, 2^64 |
2^15 for flash mode 7), and (2) broken more than 10-fold by every mutant of a fixed list on every case of every sweep the mutant
belongs to on which the fault can be expressed.  No element of any case is left out and the bound has no floor."""
import pytest
import torch

import attn_edge_cases as E
import enc_attn_cases as C

SWEEPS = "GHIKJLT"


def test_case_tables_hold_what_the_sweeps_promise():
    g = C.cases("G")
    assert {(c.d, c.Skv) for c in g} == {(d, s) for d in C.WIDE for s in range(1, 131)} | {(d, s) for d in C.NARROW for s in range(1, 201)}
    assert all(c.Sq == 70 and c.nb == 2 and c.H == 2 and c.max_len == max(70, c.Skv) and c.splits == 1 for c in g)
    h = C.cases("H")
    assert {(c.d, c.Sq, c.max_len == 512) for c in h} == {(d, s, f) for d in C.WIDE + C.NARROW for s in range(1, 131) for f in (False, True)}
    assert all(c.Skv == 70 and c.max_len in (512, max(c.Sq, 70)) for c in h)
    i = C.cases("I")
    assert {c.Skv for c in i} >= {33, 64, 65, 97, 129, 161, 289, 321} and {c.splits for c in i} == set(range(11))
    assert {(c.d, c.Sq, c.max_len is None) for c in i} == {(d, s, f) for d in (64, 256, 512) for s in (16, 70) for f in (False, True)}
    for d in (256, 512):     # every compile-time merge, the run-time one at 9 and 10, one-tile splits and a short last split, with bias
        assert {C.split_shape(c)[0] for c in i if c.d == d and c.max_len} >= set(range(1, 11))
        assert any(C.split_shape(c) == (c.Skv // 32 + 1, 1) and c.Skv % 32 == 1 for c in i if c.d == d and c.max_len and c.splits)
    assert {C.split_shape(c)[0] for c in i if c.d == 64} == set(range(1, 7))
    k = C.cases("K")
    assert {(c.d, c.Sq, c.splits) for c in k if c.Skv == 576} == {(d, s, sp) for d in (64, 256, 512) for s in (1, 64, 65, 512) for sp in (1, 0, 3, 18)}
    assert all(c.max_len == 576 and -(-576 // 64) * 64 + 63 == 639 for c in k if c.Skv == 576)
    assert any(c.Sq > c.Skv for c in k) and any(c.Sq < c.Skv < 576 for c in k) and any(c.H == 3 and c.d == 64 for c in k)
    j = C.cases("J")
    assert {(c.kern, c.d, c.data) for c in j} == {(kn, d, da) for kn, ds in (("tok", C.WIDE), ("flash", (64,))) for d in ds
                                                  for da in ("rise", "first", "steps", "equal", "edge")}
    edges = {p for c in j if c.kern == "tok" and c.data == "edge" and c.splits == 3 for p in c.edge}
    assert C.split_shape([c for c in j if c.kern == "tok" and c.splits == 3][0]) == (3, 2) and edges >= {0, 31, 32, 63, 64, 127, 128, 148, 149}
    ll = C.cases("L")
    assert {(C.n_main(c), c.extra) for c in ll} == {(s, x) for s in list(range(1, 331)) + list(C.L_LONG) for x in (False, True)}
    t = C.cases("T")
    assert {(c.Sq, c.d, (c.nb, c.N, c.H)) for c in t} == {(T, d, x) for T in range(1, 17) for d in (64, 128, 256, 384, 512) for x in C.T_BNH}
    assert all({c.max_len for c in t if c.Sq == T} == {None, T, 512} for T in range(1, 17))


def test_bias_matrix_and_the_table_edges():
    tbl = torch.arange(1.0, 8.0)[:, None].expand(7, 2)                  # max_len = 4: rows 0 .. 6
    b = C.bias_matrix(tbl, 4, 4, 4)[0, 0]
    assert b[0].tolist() == [4, 5, 6, 7] and b[3].tolist() == [1, 2, 3, 4]          # row j - i + 3: both extreme rows are read
    assert C.bias_matrix(tbl, 4, 4, 4, shift=1)[0, 0, 0].tolist() == [5, 6, 7, 0]   # past the table: 0, as the kernel clips
    assert C.bias_matrix(tbl, 2, 3, 4, flip=True)[0, 0].tolist() == [[4, 3, 2], [5, 4, 3]]


def test_split_rule_restates_the_launcher():
    """tps = ceil(ntile / min(forced, ntile)), ns = ceil(ntile / tps); the heuristic: enough units for 256 CUs, two tiles per split"""
    c = C.case("I", "tok", 2, 70, 321, 2, 512, splits=9)
    assert C.split_shape(c) == (6, 2) and C.split_shape(c._replace(splits=10, Skv=289)) == (10, 1)
    assert C.split_shape(c._replace(splits=0)) == (4, 3) and C.split_shape(c._replace(splits=0, Skv=97)) == (2, 2)
    assert C.split_shape(c._replace(splits=0, Skv=96)) == (1, 3) and C.split_shape(c._replace(splits=0), ws_bytes=0) == (1, 11)
    assert C.split_shape(C.case("I", "tok", 2, 70, 321, 2, 64, splits=10)) == (6, 1)


@pytest.mark.parametrize("elem", list(C.ELEM))
def test_raised_and_hard_data_do_what_they_are_for(elem):
    """raised keys ~ 8 natural-log units above the rest (temporal: below, on odd rows); steps on both sides of each kernel's threshold"""
    for c in (C.cases("G")[129], C.cases("L")[200], C.cases("T")[-1]):
        o = C.operands(c, elem)
        s = C.reference(c._replace(max_len=None), dict(o, table=None), elem)
        q, k, v = C.heads64(o)
        sc = (q @ k.transpose(-1, -2)) * o["scale"]
        up = torch.zeros(c.Skv, dtype=torch.bool)
        up[C.raised_keys(c)] = True
        rows = slice(0, None, 2) if c.kern == "temporal" else slice(None)
        assert (sc[:, :, rows][..., up].mean() - sc[:, :, rows][..., ~up].mean() - C.RAISE).abs() < 1.0, C.case_id(c)
        if c.kern == "temporal":
            assert (sc[:, :, 1::2][..., up].mean() - sc[:, :, 1::2][..., ~up].mean() + C.RAISE).abs() < 1.0
        assert torch.isfinite(s["bound"]).all()
    for c in C.cases("J"):
        if c.data == "steps":
            thr = dict(c.thr)[elem] if isinstance(c.thr, tuple) else c.thr
            o = C.operands(c, elem)
            q, k, v = C.heads64(o)
            sc = (q @ k.transpose(-1, -2)) * o["scale"] * C.LOG2E
            t = torch.nn.functional.pad(sc, (0, (-c.Skv) % c.tile), value=float("-inf")).view(*sc.shape[:3], -1, c.tile).amax(-1)
            step = t[..., 1:] - t[..., :-1]
            assert step.shape[-1] >= 2 and ((step[..., 0::2] > thr - 0.2) & (step[..., 0::2] < thr - 0.02)).all(), (C.case_id(c), step[0, 0, 0])
            assert ((step[..., 1::2] > thr + 0.02) & (step[..., 1::2] < thr + 0.2)).all(), (C.case_id(c), step[0, 0, 0])


SPLIT_MUTANTS = (C.m_no_kbeg, C.m_split_first)     # (what these do depends on the case's split count, not on its operands alone)


@pytest.mark.parametrize("elem", list(C.ELEM))
@pytest.mark.parametrize("sweep", SWEEPS)
def test_emulation_inside_and_every_mutant_tenfold_outside(sweep, elem):
    """Every case of the sweep, one float64 reference each: the emulation inside the bound at every stale distance (flash: also on
    the pre-scaled q), and every mutant of the sweep more than 10 bounds away on EVERY case on which the fault can be expressed
    (a mutation function returns None where it cannot: one key, one head, no bias, no split, ...); the smallest ratio per mutant
    is printed with its case.  The six flash cases of 1024 rows and more are left to the emulation (a 2049 x 2049 float64 softmax
    per mutant); their mutants act on single keys as at 577."""
    worst, least, count = {}, {}, {}
    mutants = [(name, fn) for name, sweeps, fn in C.MUTANTS if sweep in sweeps]
    seen = None
    for c in C.cases(sweep):
        key = c._replace(splits=1)
        fresh = key != seen
        seen = key
        o = C.operands(c, elem)
        m = C.reference(c, o, elem)
        if fresh:
            for pre in ((False, True) if c.kern == "flash" else (False,)):
                op, mp = (C.prescaled(o, elem), None) if pre else (o, m)
                mp = mp or C.reference(c, op, elem)
                assert torch.isfinite(mp["bound"]).all() and torch.isfinite(mp["out"]).all() and torch.isfinite(mp["lse"]).all()
                for stale in C.stales(c, elem):
                    r = E.ratio((C.emulate(c, op, elem, stale) - mp["out"]).abs(), mp["bound"])
                    if r > worst.get((c.kern, stale), (-1.0, None))[0]:
                        worst[(c.kern, stale)] = (r, C.case_id(c) + ("-prescaled" if pre else ""))
        if c.Sq * c.Skv > 1 << 19:
            continue
        for name, fn in mutants:
            if not fresh and fn not in SPLIT_MUTANTS:
                continue
            kw = fn(c, o)
            if kw is None:
                continue
            r = E.ratio((C.emulate(c, o, elem, **kw) - m["out"]).abs(), m["bound"])
            count[name] = count.get(name, 0) + 1
            if r < least.get(name, (float("inf"), None))[0]:
                least[name] = (r, C.case_id(c))
    for (kern, stale), (r, cid) in worst.items():
        print(f"emulated error / bound, sweep {sweep} {elem} {kern}, row max {stale} log2 units stale: {r:.3f} ({cid})")
    for name, _ in mutants:
        r, cid = least.get(name, (0.0, None))
        print(f"mutant '{name}', sweep {sweep} {elem}: smallest error / bound {r:.1f} over {count.get(name, 0)} cases ({cid})")
    assert worst and all(r <= 1.0 for r, _ in worst.values()), worst
    assert all(least.get(name, (0.0, None))[0] > 10 for name, _ in mutants), {n: least.get(n) for n, _ in mutants if not least.get(n, (0.0,))[0] > 10}


def test_fp32_p_weight_is_what_separates_the_temporal_bound():
    """with the weight of sum P |v| at 0 the MFMA kernels' emulation (P rounded to the element type) leaves the temporal bound: the
    parameter is not slack"""
    c = [x for x in C.cases("T") if x.Sq == 16 and x.d == 64 and x.max_len == 16 and x.N == 3][0]
    o = C.operands(c, "bf16")
    m = C.reference(c, o, "bf16")
    assert E.ratio((C.emulate(c, o, "bf16") - m["out"]).abs(), m["bound"]) <= 1.0
    assert E.ratio((C.emulate(c._replace(kern="tok"), o, "bf16") - m["out"]).abs(), m["bound"]) > 1.0
