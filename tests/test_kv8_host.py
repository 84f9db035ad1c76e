"""CPU: the FP8 (e4m3) KV cache -- the quantiser reference's properties, the `Kv8Layer` protocol, a tiny HF model generating on a
cache of such layers through the stock forward, the routes (fake-cuda stubs of tests/test_decoder_route_host.py), the ABI of the
new exports, the LDS image and operand maps of decode_attn_kv8_kernel (in the style of tests/test_lds_layouts.py), and the float64
bound of tests/kv8_cases.py against a CPU emulation of the kernel's rounding points and two mutants."""
import re
from pathlib import Path

import pytest
import torch

import attn_edge_cases as A
import kv8_cases as K8
from test_decoder_route_host import _FakeCuda, _model
from u2tokenizer_amd import _lib, ops, prefill

ROOT = Path(__file__).resolve().parents[1]
bf, f16 = torch.bfloat16, torch.float16
NEW_EXPORTS = ("u2tok_kv_quantize_rows", "u2tok_decode_attention_kv8", "u2tok_decode_attention_kv8_workspace_bytes",
               "u2tok_decoder_decode_post_kv8")


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_new_exports_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "u2tok.h").read_text(), flags=re.S)
    for n in NEW_EXPORTS:
        assert re.search(rf"\b{n}\s*\(", text), n
        assert n in _lib.SIGNATURES, n
    # the step's structs keep their layout: new entry points, not new fields
    import ctypes as C
    assert C.sizeof(_lib.DecodeConfig) == 40 and C.sizeof(_lib.DecodeLayer) == 17 * C.sizeof(C.c_void_p)


@pytest.mark.parametrize("elem", ["bf16", "f16"])
def test_workspace_of_the_code_attention_fits_the_steps(elem):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    h = _lib.load_library(elem)
    for n in NEW_EXPORTS:
        assert hasattr(h, n), n
    for Bn, Hq, Hkv, T, d in ((1, 32, 8, 2048, 128), (16, 32, 8, 1800, 128), (64, 32, 32, 8192, 96), (3, 4, 2, 100, 64)):
        assert h.u2tok_decode_attention_kv8_workspace_bytes(Bn, Hq, Hkv, T, d) <= h.u2tok_decode_attention_workspace_bytes(Bn, Hq, Hkv, T, d)
    # refusals that need no device: returned before any launch
    assert h.u2tok_kv_quantize_rows(None, None, 1, 1, 1, 64, 64, 64, 64, 64, 64, 64, None, None, None, None, 8, 0, None) == -1
    assert h.u2tok_decode_attention_kv8(None, None, None, None, None, None, 1, 1, 1, 1, 64, 64, 0, 0, 64, 0.125, None, None, 0, None) == -1


@pytest.mark.parametrize("elem", ["bf16", "f16"])
def test_the_layer_step_refuses_before_any_launch(elem):
    """u2tok_decoder_decode_post_kv8 on arguments it cannot take: every call below carries one, and returns before a launch or a
    memory access (the addresses are never dereferenced)"""
    import ctypes as C
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    h = _lib.load_library(elem)
    ERR_ARG, ERR_WS = -1, -3
    P = 1 << 20
    cfg = _lib.DecodeConfig(B=2, E=128, Hq=2, Hkv=1, D=64, I=256, eps=1e-6, qk_eps=1e-6, scale=0.125, wform=0)
    lay = _lib.DecodeLayer(**{n: P for n in ("w_in_norm", "Wqkv", "wq_norm", "wk_norm", "Wo", "w_post_norm", "Wgu", "Wdown")})
    # cfg, layer, x, qkv, k_new, v_new, k_codes, v_codes, k_scales, v_scales, capacity, k_first, s_off, kv_start, out, ws, ws_bytes, stream
    base = [C.byref(cfg), C.byref(lay), P, P, P, P, P, P, P, P, 100, 0, 100, None, P, P, 1 << 30, None]

    def call(**kw):
        a = list(base)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return h.u2tok_decoder_decode_post_kv8(*a)

    assert call() == ERR_ARG                                   # s_off = capacity: no room for the step's row
    assert call(a11=5, a12=3) == ERR_ARG and call(a11=-1, a12=3) == ERR_ARG and call(a12=-1) == ERR_ARG
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15):
        assert call(**{f"a{i}": None}, a12=50) == ERR_ARG, i
    assert call(a4=P + 8, a12=50) == ERR_ARG and call(a6=P + 8, a12=50) == ERR_ARG and call(a8=P + 2, a12=50) == ERR_ARG
    assert call(a16=16, a12=50) == ERR_WS
    wide = _lib.DecodeConfig.from_buffer_copy(cfg)
    wide.Hq, wide.Hkv = 34, 2                                   # 17 query heads per kv head: the batched kernel holds 16
    assert call(a0=C.byref(wide), a12=50) == ERR_ARG


# ------------------------------------------------------------------------------------------------------- LDS image and maps
@pytest.mark.parametrize("D", K8.DS)
def test_dma_fills_the_image_the_reads_expect(D):
    """every 16-byte chunk of the tile lands once, and a read finds the bytes it asks for"""
    image = {}
    for piece in range(D // 16):
        for lane in range(64):
            row, byte = K8.dma_source(D, piece, lane)
            image[(piece * 64 + lane) * 16] = (row, byte)
    assert sorted(image.values()) == [(r, 16 * c) for r in range(64) for c in range(D // 16)]
    for lane in range(64):
        for kb in range(4):
            for ks in range(D // 32):
                off, row, d0 = K8.k_read(D, kb, ks, lane)
                assert off % 8 == 0 and image[off & ~15] == (row, d0 & ~15) and off & 15 == d0 & 15
        for blk in range(D // 32):
            for r16 in range(4):
                off, row, d0 = K8.v_read(D, blk, r16, lane)
                assert off % 8 == 0 and image[off & ~15] == (row, d0 & ~15) and off & 15 == d0 & 15


@pytest.mark.parametrize("D", K8.DS)
def test_reads_are_free_of_bank_conflicts(D):
    """ds_read_b64 and ds_read_b64_tr_b16 are served per 32-lane half, 64 banks of 4 bytes"""
    for half in (range(0, 32), range(32, 64)):
        for kb in range(4):
            for ks in range(D // 32):
                assert K8.bank_ways([K8.k_read(D, kb, ks, l)[0] for l in half]) == 1, ("K", kb, ks)
        for blk in range(D // 32):
            for r16 in range(4):
                assert K8.bank_ways([K8.v_read(D, blk, r16, l)[0] for l in half]) == 1, ("V", blk, r16)


@pytest.mark.parametrize("D", K8.DS)
def test_transposed_byte_pairs_meet_the_p_fragment(D):
    """the 8 byte pairs a lane receives for 32-key half hh are (d = 32 blk + 2 l15, + 1) of exactly the keys its P fragment carries
    in the same slots; over lanes, blocks and halves every (key, d) of the tile enters one MFMA once, and the accumulator rows are
    the d the store writes them to"""
    seen = set()
    for blk in range(D // 32):
        for hh in range(2):
            for lane in range(64):
                l15, g = lane & 15, lane >> 4
                got = K8.v_received(D, blk, 2 * hh, lane) + K8.v_received(D, blk, 2 * hh + 1, lane)
                assert [k for k, _ in got] == [K8.p_slot_key(hh, g, e) for e in range(8)]
                assert {d for _, d in got} == {32 * blk + 2 * l15}
                for key, d in got:
                    for odd in (0, 1):               # the low byte feeds the even MFMA's row l15, the high byte the odd one's
                        assert (key, d + odd) not in seen
                        seen.add((key, d + odd))
                        assert d + odd == K8.o_row_d(blk, odd, l15 >> 2, l15 & 3)
    assert seen == {(k, d) for k in range(64) for d in range(D)}
    rows = sorted(K8.o_row_d(blk, odd, g, r) for blk in range(D // 32) for odd in (0, 1) for g in range(4) for r in range(4))
    assert rows == list(range(D))


# ------------------------------------------------------------------------------------------------------ the quantiser reference
@pytest.mark.parametrize("dt", [bf, f16, torch.float32])
def test_quantiser_reference_properties(dt):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(3, 2, 40, 96, generator=g) * torch.exp2(torch.randint(-6, 7, (3, 2, 40, 1), generator=g).float())).to(dt)
    x[0, 0, 0] = 0
    codes, scale = ops.quantize_kv_fp8(x)
    assert codes.dtype == torch.float8_e4m3fn and codes.shape == x.shape and scale.dtype == torch.float32 and scale.shape == x.shape[:3]
    raw = codes.view(torch.uint8)
    assert not bool(((raw & 0x7F) == 0x7F).any())                            # no NaN code
    assert scale[0, 0, 0] == 1.0 and bool((raw[0, 0, 0] & 0x7F == 0).all())   # a zero row: scale 1, zero codes
    xf = x.float()
    amax = xf.abs().amax(-1)
    assert torch.equal(scale[amax > 0], (amax / 448.0)[amax > 0])
    at = xf.abs().argmax(-1, keepdim=True)
    assert bool((codes.float().gather(-1, at).abs()[amax > 0] == 448.0).all())   # the amax element maps to +-448
    dq = ops.dequantize_kv_fp8(codes, scale, torch.float64)
    assert torch.equal(dq, codes.double() * scale.double()[..., None])
    assert torch.equal(ops.dequantize_kv_fp8(raw, scale, torch.float64), dq)
    err = (x.double() - dq).abs()
    assert bool((err <= torch.maximum(2.0 ** -4 * x.double().abs(), 2.0 ** -10 * scale.double()[..., None])).all())


# ------------------------------------------------------------------------------------------------------------ the cache layer
def _rows(B, H, n, d, seed, dt=bf):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, n, d, generator=g).to(dt), torch.randn(B, H, n, d, generator=g).to(dt)


def _ref(parts):
    """the reference arrays: the codes and scales of everything cached so far, per call"""
    k = [ops.quantize_kv_fp8(p[0]) for p in parts]
    v = [ops.quantize_kv_fp8(p[1]) for p in parts]
    cat = lambda xs, i: torch.cat([x[i] if i else x[i].view(torch.uint8) for x in xs], 2)   # noqa: E731
    return cat(k, 0), cat(v, 0), cat(k, 1), cat(v, 1)


def _same(lay, ref):
    got = lay.codes()
    return all(torch.equal(a, b) for a, b in zip(got, ref))


def test_layer_update_returns_and_growth():
    lay = prefill.Kv8Layer()
    assert lay.get_seq_length() == 0 and lay.keys is None and lay.get_mask_sizes(5) == (5, 0) and lay.get_max_length() == -1
    parts = [_rows(2, 3, 40, 64, 1)]
    k, v = lay.update(*parts[0])
    assert k is parts[0][0] and v is parts[0][1]                  # an empty layer returns its inputs
    assert lay.get_seq_length() == 40 and _same(lay, _ref(parts))
    parts.append(_rows(2, 3, 1, 64, 2))
    k, v = lay.update(*parts[1])                                  # a filled one the whole cache, dequantised in the callers' type
    ref = _ref(parts)
    assert k.dtype == bf and k.shape == (2, 3, 41, 64)
    assert torch.equal(k, ops.dequantize_kv_fp8(ref[0], ref[2], bf)) and torch.equal(v, ops.dequantize_kv_fp8(ref[1], ref[3], bf))
    assert torch.equal(lay.keys, k) and torch.equal(lay.values, v) and lay.get_mask_sizes(1) == (42, 0)
    cap = lay._kc.shape[2]
    parts.append(_rows(2, 3, cap, 64, 3))                         # past the capacity: the buffers grow, the old codes keep their bits
    lay.update(*parts[2])
    assert lay._kc.shape[2] >= 41 + cap and lay.get_seq_length() == 41 + cap and _same(lay, _ref(parts))
    with pytest.raises(AttributeError):
        lay.keys = k
    with pytest.raises(AttributeError):
        lay.values = v


def test_layer_operations_work_on_codes_and_scales():
    parts = [_rows(4, 2, 30, 96, 4), _rows(4, 2, 3, 96, 5)]
    ref = _ref(parts)

    def fresh():
        lay = prefill.Kv8Layer()
        for p in parts:
            lay.update(*p)
        return lay
    lay = fresh()
    lay.crop(-5)
    assert lay.get_seq_length() == 28 and _same(lay, [r[:, :, :28] for r in ref])
    lay.crop(20)
    assert lay.get_seq_length() == 20 and _same(lay, [r[:, :, :20] for r in ref])
    lay.crop(25)                                                  # not shorter than the cache: nothing happens
    assert lay.get_seq_length() == 20
    more = _rows(4, 2, 2, 96, 6)
    lay.update(*more)                                             # ... and the next rows follow position 20
    again = _ref([more])
    assert _same(lay, [torch.cat([r[:, :, :20], a], 2) for r, a in zip(ref, again)])
    lay = fresh()
    idx = torch.tensor([2, 0])
    lay.batch_select_indices(idx)
    assert _same(lay, [r[idx] for r in ref])
    lay = fresh()
    lay.batch_repeat_interleave(3)
    assert _same(lay, [r.repeat_interleave(3, 0) for r in ref])
    lay = fresh()
    beam = torch.tensor([3, 3, 0, 1])
    lay.reorder_cache(beam)
    assert _same(lay, [r.index_select(0, beam) for r in ref])
    lay.update(*_rows(4, 2, 1, 96, 7))                            # a reordered layer goes on appending
    assert lay.get_seq_length() == 34
    lay.offload(), lay.prefetch()
    assert lay.get_seq_length() == 34
    lay.reset()
    assert lay.get_seq_length() == 0
    k, v = lay.update(*parts[0])
    assert k is parts[0][0] and _same(lay, _ref(parts[:1]))


def test_a_tiny_model_generates_on_a_cache_of_kv8_layers():
    m = _model("qwen3", dtype=torch.float32, num_hidden_layers=2)
    ids = torch.tensor([[3, 9, 27, 5, 11, 40, 2, 8]])
    cache = prefill.kv8_cache(2)
    with torch.no_grad():
        out = m.generate(ids, past_key_values=cache, max_new_tokens=6, do_sample=False, pad_token_id=0)
        assert out.shape == (1, 14) and all(type(l) is prefill.Kv8Layer for l in cache.layers)
        assert cache.get_seq_length() == 13
        # teacher-forced on a second cache of the same kind: the same tokens
        c2 = prefill.kv8_cache(2)
        logits = m(ids, past_key_values=c2, use_cache=True).logits[:, -1]
        for t in range(6):
            assert int(logits.argmax(-1)) == int(out[0, 8 + t])
            logits = m(out[:, 8 + t:9 + t], past_key_values=c2, use_cache=True).logits[:, -1]
    assert all(torch.equal(a, b) for l1, l2 in zip(cache.layers, c2.layers) for a, b in zip(l1.codes(), [x[:, :, :13] for x in l2.codes()]))


# ------------------------------------------------------------------------------------------------------------------ routes
def _filled(m, B, T, fake=True):
    att = m.model.layers[0].self_attn
    cache = prefill.kv8_cache(1)
    kv = torch.zeros(B, m.config.num_key_value_heads, T, att.head_dim, dtype=m.dtype)
    cache.update(kv, kv, 0)
    if fake:
        lay = cache.layers[0]
        lay._kc = lay._kc.as_subclass(_FakeCuda)
    return cache


def _ask(m, B, S, cache):
    layer = m.model.layers[0]
    d = layer.self_attn.head_dim
    pr = layer._u2_prefill.layout.projections(layer)
    kw = dict(position_embeddings=(torch.ones(B, S, d, dtype=m.dtype),) * 2, past_key_values=cache)
    return prefill.route(layer, (B, S, m.config.hidden_size), m.dtype, True, (), kw, False, pr)


def test_routes_on_a_kv8_cache():
    m = _model()
    prefill.enable_fused_prefill(m, kv8=True, continued=True, stack_decode=True, head=True, wide_decode=True)
    assert _ask(m, 2, 1, _filled(m, 2, 5)) == ("decode", None)
    assert _ask(m, 20, 1, _filled(m, 20, 5)) == ("decode", None)
    assert _ask(m, 2, 1, _filled(m, 3, 5)) == ("stock", None)                   # another batch than the cache's
    assert _ask(m, 2, 1, _filled(m, 2, 5, fake=False)) == ("stock", None)       # a cache on the CPU
    assert _ask(m, 2, 4, _filled(m, 2, 5)) == ("stock", None)                   # extend refuses the layer
    assert _ask(m, 2, 4, prefill.kv8_cache(1)) == ("prefill", None)             # an empty one: the plain prefill
    # the whole-stack and head calls are out of scope on such a cache
    kw = dict(past_key_values=_filled(m, 2, 5), use_cache=True)
    assert prefill.stack_route(m.model, 2, 1, m.dtype, True, kw, False) == "layers"
    assert prefill.head_route(m, 2, 1, m.dtype, True, kw, False) == "stock"
    # off: the layer is nobody's
    prefill.enable_fused_prefill(m)
    assert _ask(m, 2, 1, _filled(m, 2, 5)) == ("stock", None)
    prefill.disable_fused_prefill(m)


def test_the_prefill_places_a_kv8_layer_where_the_append_layer_goes():
    from transformers.cache_utils import DynamicCache
    like = torch.zeros(1, dtype=bf)
    cache = DynamicCache()
    assert prefill._prefill_append_layer(cache, 1, 2, 2, 8, 64, like, kv8=True) is None
    assert type(cache.layers[1]) is prefill.Kv8Layer and type(cache.layers[0]) is not prefill.Kv8Layer
    kept = cache.layers[1]
    assert prefill._prefill_append_layer(cache, 1, 2, 2, 8, 64, like, kv8=True) is None and cache.layers[1] is kept
    lay = prefill._prefill_append_layer(cache, 0, 2, 2, 8, 64, like)
    assert type(lay) is prefill._append_layer_class() and cache.layers[0] is lay

    class Other(DynamicCache):
        pass
    other = Other()
    assert prefill._prefill_append_layer(other, 0, 2, 2, 8, 64, like, kv8=True) is None and not other.layers
    s = {s.kw: s for s in prefill.SWITCHES}["kv8"]
    assert prefill.SWITCHES[-1] is s and (s.field, s.config, s.default, s.implies, s.needs) == ("kv8", "u2_fused_kv_fp8", False, (), ())
    assert "whole-stack" in s.doc and "unmeasured" in s.doc


# ------------------------------------------------------------------------------------------------------------------- bound
@pytest.mark.parametrize("elem", list(A.ELEM))
@pytest.mark.parametrize("data", ("normal", "poison", "edge"))
def test_emulation_keeps_the_bound_and_the_mutants_break_it(elem, data):
    worst = 0.0
    for T in K8.HOST_LENGTHS:
        c = K8.attn_case(T, data)
        o = K8.operands(c, elem)
        args, vis = K8.split(c, o), A.case_visible(c)
        m = K8.model(*args, o["scale"], vis, elem)
        assert bool((m["bound"][-1] == 0).all())                   # the last sequence sees no key: exact zeros
        r = A.ratio((K8.emulate(*args, o["scale"], vis, elem) - m["out"]).abs(), m["bound"])
        worst = max(worst, r)
        assert r <= 1.0, (T, r)
        if data == "normal" and T >= 31:
            for mutant in ("shift", "swap"):
                rm = A.ratio((K8.emulate(*args, o["scale"], vis, elem, mutant=mutant) - m["out"]).abs(), m["bound"])
                assert rm > 10.0, (T, mutant, rm)
    print(f"emulation error / bound, {data} {elem}: {worst:.3f}")
