"""Host: the bound that tests/test_gpu_attn_edges.py holds the inference attention kernels to (tests/attn_edge_cases.py: model) is
(1) kept by a torch emulation of the kernels' rounding points on every case and data set of the sweeps, against the exact row max and
against a stale one (the lazy rescale), in both element types, and (2) broken more than 10-fold by every one-key mask mutant of a
fixed list on at least one case of the sweep the mutant belongs to.  No element of any case is left out: a row that sees no key has
a bound of zero and must be exactly zero."""
import pytest
import torch

import attn_edge_cases as E
import test_decoder_train_bounds_host as B

SWEEPS = "ABCDEF"


def _distinct(sweep):
    """the sweep's cases with distinct operands and masks (entry points share them)"""
    seen, out = set(), []
    for c in E.cases(sweep):
        key = c._replace(sweep="", entry="", layout="")
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_case_tables_hold_what_the_sweeps_promise():
    assert {c.window for c in E.cases("A") if c.d == 96} == set(range(1, 152))
    b = E.cases("B")
    assert {c.Skv - c.Sq for c in b} == {1, 31, 32, 63, 64, 65, 100} and {c.Sq for c in b} == {1, 15, 16, 17, 63, 64, 65, 70}
    assert all({None, 1, 16, 17, 63, 64, 65, co, co + 1} == {c.window for c in b if c.Skv - c.Sq == co and c.Sq == 17} for co in (1, 31, 100))
    assert {c.d for c in b} == set(E.DS)
    cc = E.cases("C")
    assert all(c.nb == 151 and c.kv_start == tuple(range(151)) for c in cc) and {c.Sq for c in cc} == {150, 6}
    assert {(c.entry, c.window, None if c.kv_len is None else c.kv_len[0]) for c in cc} == {
        ("range", None, None), ("band", None, None), ("range", None, 1), ("band", None, 1), ("range", None, 64), ("band", None, 64),
        ("range", None, 65), ("band", None, 65), ("band", 40, None)}
    d = E.cases("D")
    assert [c.Skv for c in d] == list(range(1, 301)) + [1023, 1024, 1025, 1792]
    assert {(c.Hq // c.Hkv, c.d) for c in d if c.Skv <= 36} == {(g, dd) for g in E.GS for dd in E.DS}
    assert all(c.kv_start == tuple(min(s, c.Skv) for s in (0, 1, 31, 32, 33, c.Skv // 2, c.Skv - 1, c.Skv)) for c in d)
    assert all((c.spare > 0) == (c.Skv % 2 == 1) for c in d) and all((c.data == "raised") == (c.Skv > 300) for c in d)
    e = E.cases("E")
    assert [c.Skv for c in e] == list(range(1, 201)) + [1023, 1024, 1025, 1792] and {c.Hq // c.Hkv for c in e} == {1, 3, 8}
    f = E.cases("F")
    assert {c.entry for c in f} == {"gqa", "split", "range", "band", "decode"}
    assert {(c.entry, c.data, c.d) for c in f} >= {(en, da, dd) for en in ("gqa", "split", "range", "band", "decode")
                                                   for da in ("rise", "first", "steps", "equal", "edge") for dd in E.DS}


def test_mask_rule():
    v = E.visible(3, 5, window=2, kv_start=(0, 3), kv_len=(5, 4))
    assert v[0].int().tolist() == [[0, 1, 1, 0, 0], [0, 0, 1, 1, 0], [0, 0, 0, 1, 1]]
    assert v[1].int().tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 1, 0]]
    assert E.visible(2, 3, causal=False).all()


def test_model_reuses_the_training_bound_terms():
    """at U = 2^-8 the bound is attn_fwd_model's plus the fp32 score term, which is under 1 % of it on N(0, 1) data"""
    c = E.case("A", "band", 2, 70, 133, 4, 2, 64)
    q, k, v = E.split_heads(c, E.operands(c, "bf16"))
    vis = E.case_visible(c)
    ref = B.attn_fwd_model(q, k, v, 0.125, vis)
    m = E.model(q, k, v, 0.125, vis, B.U)
    torch.testing.assert_close(m["out"], ref["out"], rtol=1e-12, atol=1e-14)
    extra = m["bound"] - ref["out_bound"]
    assert (extra >= -1e-15).all() and (extra <= 1e-2 * ref["out_bound"]).all()


def test_poison_is_far_above_every_visible_score():
    for c in (E.cases("B")[40], E.cases("C")[3], E.cases("D")[69], E.cases("D")[-1], E.cases("E")[100]):
        o = E.operands(c, "bf16")
        q = o["q"].double().view(c.nb, c.Sq, c.Hq, c.d).permute(0, 2, 1, 3)
        kk = o["K"].double().repeat_interleave(c.Hq // c.Hkv, 1)
        s = (q @ kk.transpose(-1, -2)) * o["scale"]                                     # over the whole buffer
        inv = torch.ones(c.nb, c.Skv + c.spare, dtype=torch.bool)
        inv[:, :c.Skv] = ~E.case_visible(c).any(1).expand(c.nb, c.Skv)
        assert inv.any() and torch.isfinite(o["K"].float()).all()
        lo = s.masked_fill(~inv[:, None, None, :], float("inf")).amin(-1)
        hi = s.masked_fill(inv[:, None, None, :], float("-inf")).amax(-1)
        assert (lo > hi + 10).all(), (c, (lo - hi).min().item())
        assert (o["V"].float().abs()[inv[:, None, :, None].expand_as(o["V"])] == 64).all()


@pytest.mark.parametrize("elem", list(E.ELEM))
def test_hard_data_does_what_it_is_for(elem):
    """rise: > 8 log2 units per tile; first: one key > 100 log2 units above the rest; steps: both sides of the threshold 8"""
    def tile_max_log2(c):
        o = E.operands(c, elem)
        q, k, v = E.split_heads(c, o)
        s = E.model(q, k, v, o["scale"], E.visible(c.Sq, c.Skv, causal=False), E.ELEM[elem][1])["s"] * E.LOG2E
        pad = (-c.Skv) % c.tile
        s = torch.nn.functional.pad(s, (0, pad), value=float("-inf"))
        return s.view(*s.shape[:3], -1, c.tile).amax(-1)               # (nb, Hq, Sq, tiles)
    for c in E.cases("F"):
        if c.data == "steps":
            t = tile_max_log2(c)
            step = t[..., 1:] - t[..., :-1]
            assert ((step[..., 0::2] > 7.8) & (step[..., 0::2] < 7.98)).all() and ((step[..., 1::2] > 8.02) & (step[..., 1::2] < 8.2)).all()
            assert step.shape[-1] >= 2
        elif c.data == "rise":
            t = tile_max_log2(c)
            assert (t[..., 1:] - t[..., :-1] > 8.0).all()
        elif c.data == "first":
            o = E.operands(c, elem)
            q, k, v = E.split_heads(c, o)
            s = E.model(q, k, v, o["scale"], E.case_visible(c), E.ELEM[elem][1])["s"] * E.LOG2E
            top = s.topk(2, -1).values if c.Skv > 1 else None
            gap = (top[..., 0] - top[..., 1])[torch.isfinite(top[..., 1])]
            assert gap.numel() and (gap > 100).all()


@pytest.mark.parametrize("elem", list(E.ELEM))
@pytest.mark.parametrize("sweep", SWEEPS)
def test_emulation_inside_bound(sweep, elem):
    dt, U, tiny = E.ELEM[elem]
    worst = {0.0: (0.0, None), E.STALE: (0.0, None)}
    empty_rows = 0
    for c in _distinct(sweep):
        o = E.operands(c, elem)
        q, k, v = E.split_heads(c, o)
        vis = E.case_visible(c)
        m = E.model(q, k, v, o["scale"], vis, U, tiny)
        assert torch.isfinite(m["bound"]).all() and torch.isfinite(m["out"]).all()
        empty = ~vis.any(-1).expand(c.nb, c.Sq)
        empty_rows += int(empty.sum())
        for stale in worst:
            got = E.emulate(q, k, v, o["scale"], vis, dt, stale)
            r = E.ratio((got - m["out"]).abs(), m["bound"])
            assert (E.rows(got)[empty] == 0).all()
            if r > worst[stale][0]:
                worst[stale] = (r, E.case_id(c))
    for stale, (r, cid) in worst.items():
        print(f"emulated error / bound, sweep {sweep} {elem}, row max {stale} log2 units stale: {r:.3f} ({cid})")
    assert all(r <= 1.0 for r, _ in worst.values()), worst
    assert empty_rows > 0 or sweep not in "CD"   # the ranges and the decode sweep hold sequences that see nothing


# --------------------------------------------------------------------------------------------------------------- mutants
def _shift_start(c, by):
    return E.visible(c.Sq, c.Skv, c.window, tuple(min(max(s + by, 0), c.Skv) for s in c.kv_start), c.kv_len, c.causal)


def _shift_len(c, by):
    return E.visible(c.Sq, c.Skv, c.window, c.kv_start, tuple(min(max(n + by, 0), c.Skv) for n in c.kv_len), c.causal)


def _hide_one_per_row(vis, cand, last):
    """hide, per row, the last (else the first) visible key among the candidate columns `cand` (Skv bool)"""
    hit = vis & cand[None, None, :]
    idx = torch.arange(vis.shape[-1])
    pick = torch.where(hit, idx, torch.full_like(idx, -1 if last else 1 << 30))
    col = pick.amax(-1) if last else pick.amin(-1)
    sel = hit.any(-1)
    out = vis.clone()
    b, i = sel.nonzero(as_tuple=True)
    out[b, i, col[b, i]] = False
    return out


def m_window_plus(c, vis):
    return E.visible(c.Sq, c.Skv, c.window + 1, c.kv_start, c.kv_len) if c.window else None


def m_window_minus(c, vis):
    return E.visible(c.Sq, c.Skv, c.window - 1, c.kv_start, c.kv_len) if c.window and c.window > 1 else None


def m_own_key_at_tile_edge(c, vis):
    j = torch.arange(c.Skv)
    diag = (j[None, :] == torch.arange(c.Sq)[:, None] + c.Skv - c.Sq) & ((j % c.tile == 0) | (j % c.tile == c.tile - 1))[None, :]
    return vis & ~diag[None] if c.causal else None


def m_past_diagonal(c, vis):
    j = torch.arange(c.Skv)
    return vis | (j[None, :] == torch.arange(c.Sq)[:, None] + c.Skv - c.Sq + 1)[None] if c.causal and c.Sq > 1 else None


def m_start_minus(c, vis):
    return _shift_start(c, -1) if c.kv_start else None


def m_start_plus(c, vis):
    return _shift_start(c, 1) if c.kv_start else None


def m_len_plus(c, vis):
    return _shift_len(c, 1) if c.kv_len else None


def m_len_minus(c, vis):
    return _shift_len(c, -1) if c.kv_len else None


def m_newest_key(c, vis):
    return _hide_one_per_row(vis, torch.ones(c.Skv, dtype=torch.bool), last=True)


def m_oldest_key(c, vis):
    return _hide_one_per_row(vis, torch.ones(c.Skv, dtype=torch.bool), last=False)


def m_tile_first(c, vis):
    return _hide_one_per_row(vis, torch.arange(c.Skv) % c.tile == 0, last=True)


def m_tile_last(c, vis):
    return _hide_one_per_row(vis, torch.arange(c.Skv) % c.tile == c.tile - 1, last=False)


NEIGHBOUR = "one group row reads its neighbour's query"
# (name, sweeps it belongs to, mutation of the mask)
MUTANTS = [("window sees W + 1 keys", "AB", m_window_plus), ("window sees W - 1 keys", "AB", m_window_minus),
           ("a row misses its own key at a tile edge", "AB", m_own_key_at_tile_edge),
           ("a row sees the key past its diagonal", "AB", m_past_diagonal),
           ("kv_start one lower", "C", m_start_minus), ("kv_start one higher", "C", m_start_plus),
           ("kv_len one higher", "C", m_len_plus), ("kv_len one lower", "C", m_len_minus),
           ("decode: kv_start one lower", "D", m_start_minus), ("decode: misses the newest key", "D", m_newest_key),
           ("decode: misses its first key", "D", m_oldest_key),
           ("split form: misses the last key", "E", m_newest_key), ("split form: misses key 0", "E", m_oldest_key),
           ("first key of a tile hidden", "ABCDE", m_tile_first), ("last key of a tile hidden", "ABCDE", m_tile_last),
           (NEIGHBOUR, "BCDE", None)]


def _mutant_ratio(c, mutate, name):
    o = E.operands(c, "bf16")
    q, k, v = E.split_heads(c, o)
    vis = E.case_visible(c)
    if name == NEIGHBOUR:
        if c.Hq // c.Hkv < 2:
            return None
        qm, vm = q.clone(), vis
        qm[:, 1] = q[:, 0]
    else:
        qm, vm = q, mutate(c, vis)
        if vm is None or torch.equal(vm.expand(c.nb, -1, -1), vis.expand(c.nb, -1, -1)):
            return None
    m = E.model(q, k, v, o["scale"], vis, E.ELEM["bf16"][1])
    return E.ratio((E.emulate(qm, k, v, o["scale"], vm, torch.bfloat16) - m["out"]).abs(), m["bound"])


@pytest.mark.parametrize("name,sweeps,mutate", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_every_mutant_breaks_the_bound_tenfold(name, sweeps, mutate):
    """per sweep the mutant belongs to: the first case on which some element exceeds the bound more than 10-fold (the factor of
    test_bounds_are_tight_enough_to_see_one_wrong_tile)"""
    for sweep in sweeps:
        best, hit = 0.0, None
        for c in _distinct(sweep):
            r = _mutant_ratio(c, mutate, name)
            if r is not None and r > best:
                best, hit = r, c
                if r > 10:
                    break
        print(f"mutant '{name}', sweep {sweep}: error / bound {best:.1f} on {E.case_id(hit) if hit else None}")
        assert best > 10, (name, sweep, best)


@pytest.mark.parametrize("T", [1025, 1792])
def test_raised_edges_show_a_dropped_end_key_at_long_decode_lengths(T):
    """with N(0, 1) keys a dropped first or last key of 1000 moves the output by a few bounds; the raised edges make it more than 10"""
    c = [x for x in E.cases("D") if x.Skv == T][0]
    for name, mutate in (("newest", m_newest_key), ("first", m_oldest_key)):
        r = _mutant_ratio(c, mutate, name)
        print(f"decode T = {T} (g = {c.Hq // c.Hkv}, d = {c.d}) misses its {name} key: error / bound {r:.1f}")
        assert r > 10, (T, name, r)
