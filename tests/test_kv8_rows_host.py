"""CPU: the continued prefill on an FP8 (e4m3) KV cache -- the ABI of u2tok_attention_kv8_rows and its workspace query, the refusals
that need no device, the row map and per-block tile range of decode_attn_kv8_kernel<D, true> restated in tests/kv8_rows_cases.py and
enumerated against attn_edge_cases.visible, the float64 bound of tests/kv8_cases.py against the emulation and its two mutants on the
rows table, the route (fake-cuda stubs of tests/test_decoder_route_host.py) and the switch record."""
import re
from pathlib import Path

import pytest
import torch

import attn_edge_cases as A
import kv8_cases as K8
import kv8_rows_cases as R
from test_decoder_route_host import _model
from test_kv8_host import _ask, _filled
from u2tokenizer_amd import _lib, prefill

ROOT = Path(__file__).resolve().parents[1]
NEW_EXPORTS = ("u2tok_attention_kv8_rows", "u2tok_attention_kv8_rows_workspace_bytes")


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_new_exports_are_declared_and_bound():
    import ctypes as C
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "u2tok.h").read_text(), flags=re.S)
    for n in NEW_EXPORTS:
        assert re.search(rf"\b{n}\s*\(", text), n
        assert n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES["u2tok_attention_kv8_rows"][1]) == 22 and len(_lib.SIGNATURES["u2tok_attention_kv8_rows_workspace_bytes"][1]) == 6
    assert C.sizeof(_lib.DecodeConfig) == 40 and C.sizeof(_lib.DecodeLayer) == 17 * C.sizeof(C.c_void_p)   # (no struct changed)


@pytest.mark.parametrize("elem", ["bf16", "f16"])
def test_exports_workspace_and_deviceless_refusals(elem):
    """(the addresses are never dereferenced: every call below returns before a launch)"""
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    h = _lib.load_library(elem)
    for n in NEW_EXPORTS:
        assert hasattr(h, n), n
    ws = h.u2tok_attention_kv8_rows_workspace_bytes
    for Bn, Sq, Hq, Hkv, T, d in ((1, 1, 32, 8, 2048, 128), (16, 4, 32, 8, 8196, 128), (1, 64, 32, 8, 1088, 128), (3, 7, 6, 2, 1025, 96),
                                  (3, 17, 14, 2, 117, 64), (2, 5, 16, 1, 300, 64)):
        assert ws(Bn, Sq, Hq, Hkv, T, d) == R.workspace_bytes(Bn, Sq, Hq, Hkv, T, d), (Bn, Sq, Hq, Hkv, T, d)
        if Sq == 1:   # one new position: the decode entry's splits
            assert ws(Bn, 1, Hq, Hkv, T, d) == h.u2tok_decode_attention_kv8_workspace_bytes(Bn, Hq, Hkv, T, d)
    assert ws(1, 7, 6, 2, 1025, 96) > 0 and ws(0, 1, 4, 2, 100, 64) == 0 and ws(1, 0, 4, 2, 100, 64) == 0 and ws(1, 1, 3, 2, 100, 64) == 0
    P = 1 << 20
    # q, k_codes, v_codes, k_scales, v_scales, out, B, Sq, Hq, Hkv, T, D, ldq, kv_stride, sc_stride, ldo, scale, window, kv_start, ws, ws_bytes, stream
    base = [P, P, P, P, P, P, 2, 4, 4, 2, 100, 64, 256, 0, 0, 256, 0.125, 0, None, None, 0, None]

    def call(**kw):
        a = list(base)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return h.u2tok_attention_kv8_rows(*a)

    for i in range(6):
        assert call(**{f"a{i}": None}) == -1, i
    assert call(a7=0) == -1 and call(a7=101) == -1 and call(a7=-3) == -1                 # Sq < 1, Sq > T
    assert call(a17=-1) == -1                                                            # window < 0
    assert call(a6=65535, a7=100000, a10=100000) == -1                                   # B Sq Hq beyond the merge's 32-bit index
    assert call(a6=65536) == -1 and call(a10=0) == -1 and call(a8=3) == -1 and call(a8=34) == -1 and call(a11=80) == -1
    assert call(a0=P + 8) == -1 and call(a1=P + 8) == -1 and call(a3=P + 2) == -1 and call(a5=P + 4) == -1 and call(a18=P + 2) == -1
    assert call(a12=248) == -1 and call(a12=260) == -1 and call(a15=254) == -1 and call(a13=6400 - 16) == -1 and call(a13=6408) == -1
    assert call(a14=99) == -1 and call(a16=0.0) == -1
    big = [P, P, P, P, P, P, 3, 7, 6, 2, 1025, 96, 576, 0, 0, 576, 0.1, 0, None, P, 16, None]
    assert h.u2tok_attention_kv8_rows(*big) == -3                                       # a workspace too small for the splits
    big[19], big[20] = P + 8, 1 << 30
    assert h.u2tok_attention_kv8_rows(*big) == -1                                       # ... and a misaligned one


# ------------------------------------------------------------------------------------------------------------------- row map
@pytest.mark.parametrize("G", A.GS)
def test_row_map_and_tile_ranges(G):
    """flat row -> (position, head); the last block's dead rows; and, per block, the tiles it walks against A.visible: every visible
    (row, key) pair lies in a walked tile, every walked tile holds a key one of the block's rows sees, and a tile off the masked path
    is seen whole by every row of the block"""
    for Sq in range(1, 41):
        blocks = R.row_blocks(G, Sq)
        flat = [r for blk in blocks for r in blk]
        assert flat == [(i, gh) for i in range(Sq) for gh in range(G)]                    # every (position, head) once, in order
        assert all(len(b) == R.ROWS for b in blocks[:-1]) and 1 <= len(blocks[-1]) <= R.ROWS
        assert len(blocks) == -(-Sq * G // R.ROWS) and R.ROWS - len(blocks[-1]) == len(blocks) * R.ROWS - Sq * G
        for c_off in (0, 1, 63, 64, 100):
            T = Sq + c_off
            for W in (None, 1, 17, 64, c_off + 1):
                starts = (0, min(33, T - 1), T, T + 5)
                vis = A.visible(Sq, T, W, starts)                                         # (4, Sq, T)
                for b, kvs in enumerate(starts):
                    for blk in blocks:
                        first, end, masked = R.block_tiles(blk, Sq, T, W or 0, kvs)
                        assert 0 <= first and end <= -(-T // R.BK)
                        rows = sorted({i for i, _ in blk})
                        seen = vis[b, rows]                                               # (rows of the block, T)
                        tiles = {int(j) // R.BK for j in seen.any(0).nonzero().flatten()}
                        assert tiles == set(range(first, end)), (Sq, T, W, kvs, blk[0], tiles, first, end)
                        for kt in range(first, end):
                            whole = bool(seen[:, kt * R.BK:(kt + 1) * R.BK].all()) and (kt + 1) * R.BK <= T
                            assert masked[kt] == (not whole), (Sq, T, W, kvs, blk[0], kt)
                        for i in rows:                                                    # the lane's own range is A.visible's row
                            lo, hi = R.row_keys(i, Sq, T, W or 0, kvs)
                            want = vis[b, i].nonzero().flatten().tolist()
                            assert want == list(range(lo, hi + 1)), (Sq, T, W, kvs, i)


def test_splits_cover_every_tile_once():
    for Bn, Sq, Hq, Hkv, T in ((3, 1, 6, 2, 1023), (3, 7, 6, 2, 1025), (3, 7, 32, 2, 1792), (1, 33, 16, 2, 300), (16, 4, 32, 8, 8196), (1, 1, 2, 2, 65)):
        ns, tps = R.splits(Bn, Sq, Hq, Hkv, T)
        ntile = -(-T // R.BK)
        assert ns >= 1 and (ns - 1) * tps < ntile <= ns * tps
        assert ns <= R.asked_splits(Bn, Sq, Hq, Hkv, T)                                    # never more partials than the workspace holds


# ------------------------------------------------------------------------------------------------------------------- bound
def _ratios(c, elem, mutants=False):
    o = K8.operands(c, elem)
    args, vis = K8.split(c, o), A.case_visible(c)
    m = K8.model(*args, o["scale"], vis, elem)
    assert bool((m["bound"][-1] == 0).all()) and bool((m["out"][-1] == 0).all())          # the last sequence sees no key
    r = A.ratio((K8.emulate(*args, o["scale"], vis, elem) - m["out"]).abs(), m["bound"])
    rm = [A.ratio((K8.emulate(*args, o["scale"], vis, elem, mutant=mu) - m["out"]).abs(), m["bound"]) for mu in ("shift", "swap")] \
        if mutants else []
    return r, rm


@pytest.mark.parametrize("elem", list(A.ELEM))
@pytest.mark.parametrize("data", ("normal", "poison", "edge"))
def test_emulation_keeps_the_bound_and_the_mutants_break_it(elem, data):
    cases = R.edge_cases() if data == "edge" else R.sweep(data) + (R.long_cases() if data == "normal" else ())
    assert len(cases) == {"edge": 24, "normal": 153, "poison": 145}[data]
    worst = 0.0
    for c in cases:
        hit = data == "normal" and c.Skv > 40
        r, rm = _ratios(c, elem, mutants=hit)
        worst = max(worst, r)
        assert r <= 1.0, (A.case_id(c), r)
        assert all(x > 1.0 for x in rm), (A.case_id(c), rm)
    print(f"emulation error / bound, rows {data} {elem}: {worst:.3f} over {len(cases)} cases")


# ------------------------------------------------------------------------------------------------------------------ routes
def test_routes_on_a_filled_kv8_cache(monkeypatch):
    m = _model()
    prefill.enable_fused_prefill(m, kv8_continued=True)
    stack = m.model._u2_stack
    assert stack.kv8x and stack.kv8 and stack.continued
    assert _ask(m, 2, 4, _filled(m, 2, 5)) == ("extend", None)
    assert _ask(m, 2, 1, _filled(m, 2, 5)) == ("decode", None)
    assert _ask(m, 2, 4, _filled(m, 3, 5)) == ("stock", None)                   # another batch than the cache's
    assert _ask(m, 2, 4, _filled(m, 2, 5, fake=False)) == ("stock", None)       # a cache on the CPU
    assert _ask(m, 2, 4, prefill.kv8_cache(1)) == ("prefill", None)             # an empty one: the plain prefill
    monkeypatch.setattr(prefill, "KV8_EXTEND_MAX_ROWS", 3)
    assert _ask(m, 2, 4, _filled(m, 2, 5)) == ("stock", None) and _ask(m, 2, 3, _filled(m, 2, 5)) == ("extend", None)
    monkeypatch.setattr(prefill, "KV8_EXTEND_MAX_ROWS", None)
    # off: today's answer
    prefill.enable_fused_prefill(m, kv8=True, continued=True)
    assert _ask(m, 2, 4, _filled(m, 2, 5)) == ("stock", None)
    prefill.disable_fused_prefill(m)
    wide = _model(num_attention_heads=34, num_key_value_heads=2)    # 17 query heads per kv head
    prefill.enable_fused_prefill(wide, kv8_continued=True)
    assert _ask(wide, 2, 4, _filled(wide, 2, 5)) == ("stock", None)
    prefill.disable_fused_prefill(wide)


def test_the_switch_record_and_the_counters():
    kws = [s.kw for s in prefill.SWITCHES]
    s = prefill.SWITCHES[kws.index("kv8_continued")]
    assert kws.index("kv8_continued") == kws.index("kv8") - 1 and kws[-1] == "kv8"
    assert (s.field, s.config, s.default, s.implies, s.needs, s.frees) == ("kv8x", "u2_fused_kv_fp8_continued", False, ("kv8", "continued"), (), ())
    assert "kv8_continued" in prefill.SWITCHES[-1].doc
    assert set(prefill.kv8_extend_stats) == {"extend", "padded_extend"} and set(prefill.kv8_stats) == {"decode", "padded_decode"}
    assert prefill.KV8_EXTEND_MAX_ROWS is None or (isinstance(prefill.KV8_EXTEND_MAX_ROWS, int) and prefill.KV8_EXTEND_MAX_ROWS >= 2)
