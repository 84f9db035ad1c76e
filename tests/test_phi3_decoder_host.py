"""CPU: the Phi-3 decoder layer on the fused prefill / decode path (prefill.py: _PackedLayout) and the LDS layout of the
head-dim-96 attention tiles (tokattn.hip: tok_attn_kernel<96>), restated in Python (no GPU needed).

Phi-3 layers hold q | k | v in one qkv_proj and gate | up in one gate_up_proj -- the packed layout the fused forward builds
for Llama / Qwen3 -- so `enable_fused_prefill` patches them as they are; a Phi-3 layer the kernels do not compute (another
activation, partial rotary, a head dim outside 64 / 96 / 128) is declined, and a layer in training mode with active residual
dropout takes its stock forward.

The d = 96 tiles: 64 keys x 192 bytes, twelve 16-byte chunks per row, filled by LDS-DMA (64 consecutive chunks per wave
instruction, the permutation on the SOURCE chunk) and read as ds_read_b128 K fragments (lane (l15, g) of 16-key block kb and
k step ks: chunk 4 ks + g of row 16 kb + l15) and ds_read_b64_tr_b16 V^T fragments (lane i of a 16-lane group receives
element i & 3 of the 8-byte pieces lanes (i >> 2) + 4 j point at: tests/test_lds_layouts.py).  Both tiles place logical
chunk L of row r at position L ^ ((r >> 1) & 2).
"""
import pytest
import torch

from test_lds_layouts import slots_of, tr_read

DH, BK, CPR, ROWB = 96, 64, 12, 192
NP, KS, DB = BK * CPR // 256, DH // 32, DH // 16


def t96_pos(row, L):
    return L ^ ((row >> 1) & 2)


# ds_read_b128 lane groups (one LDS cycle each, MI355X_MICROARCH.md §LDS)
B128_GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)],
               [*range(32, 36), *range(44, 48), *range(52, 60)], [*range(36, 44), *range(48, 52), *range(60, 64)]]


def dma_image(pos=t96_pos):
    """LDS chunk c -> (tile row, logical chunk) as dma_k / dma_v leave it: piece i of thread (w, lane) is chunk
    c = 256 i + 64 w + lane = (row c / 12, position c % 12) and reads the source chunk pos(row, position)"""
    img = {}
    for i in range(NP):
        for w in range(4):
            for lane in range(64):
                c = i * 256 + w * 64 + lane
                row, cp = c // CPR, c % CPR
                img[c] = (row, pos(row, cp))
    return img


def test_dma_fills_every_row_chunk_once_and_stays_inside_the_row():
    img = dma_image()
    assert len(img) == BK * CPR
    assert all(0 <= L < CPR for _, L in img.values())
    assert sorted(img.values()) == [(r, L) for r in range(BK) for L in range(CPR)]
    # the power-of-two forms of the other widths do leave a 12-chunk row: XOR (row & 7) sends chunks 8..11 to 12..15
    assert any((cp ^ (row & 7)) >= CPR for row in range(BK) for cp in range(CPR))


def k_addr(kb, ks, lane):
    l15, g = lane & 15, lane >> 4
    return kb * 16 * ROWB + l15 * ROWB + (((ks * 4 + g) ^ ((l15 >> 1) & 2)) << 4)


def test_k_fragments_receive_their_keys_and_chunks():
    img = dma_image()
    for kb in range(BK // 16):
        for ks in range(KS):
            for lane in range(64):
                a = k_addr(kb, ks, lane)
                assert a % 16 == 0
                assert img[a // 16] == (16 * kb + (lane & 15), 4 * ks + (lane >> 4)), (kb, ks, lane)


def test_k_fragment_reads_are_conflict_free():
    for kb in range(BK // 16):
        for ks in range(KS):
            for grp in B128_GROUPS:
                slots = [(k_addr(kb, ks, l) % 256) // 16 for l in grp]
                assert len(set(slots)) == 16, (kb, ks, grp, slots)


def test_unpermuted_192_byte_rows_conflict_four_ways():
    """what the permutation is for: without it one logical chunk of 16 consecutive rows sits on 4 slots only"""
    slots = [(row * ROWB + 16 * 5) % 256 // 16 for row in range(16)]
    assert len(set(slots)) == 4


def v_addrs(j, db, second):
    """lane -> byte address of the transpose read of P fragment j, d block db (second: the +16 key rows)"""
    out = []
    for lane in range(64):
        l15, g = lane & 15, lane >> 4
        v_row = 4 * g + (l15 >> 2)
        cc = 2 * db + ((l15 & 3) >> 1)
        out.append(j * 32 * ROWB + v_row * ROWB + (l15 & 1) * 8 + t96_pos(v_row, cc) * 16 + (16 * ROWB if second else 0))
    return out


def test_v_transpose_reads_receive_their_rows_and_columns():
    img = dma_image()
    lds = {}
    for c, (row, L) in img.items():
        for e in range(8):
            lds[16 * c + 2 * e] = (row, 8 * L + e)   # element value = (key row, column)
    for j in range(BK // 32):
        for db in range(DB):
            for second in (False, True):
                got = tr_read(v_addrs(j, db, second), lds)
                for lane in range(64):
                    l15, g = lane & 15, lane >> 4
                    want = [(32 * j + 16 * second + 4 * g + r, 16 * db + l15) for r in range(4)]
                    assert got[lane] == want, (j, db, second, lane)


def test_v_transpose_reads_are_conflict_free():
    for j in range(BK // 32):
        for db in range(DB):
            for second in (False, True):
                a = v_addrs(j, db, second)
                for half in (a[:32], a[32:]):   # ds_read_b64_tr_b16: 2 x 32 lanes, 8 bytes each -> 64 banks
                    pieces = [(x % 256) // 8 for x in half]
                    assert len(set(pieces)) == 32, (j, db, second)
                    assert len(set(slots_of(half))) == 16


# ------------------------------------------------------------------------------------------------ host: the layer layout
def _phi3(**kw):
    from transformers import Phi3Config, Phi3ForCausalLM
    c = dict(vocab_size=128, hidden_size=192, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
             num_key_value_heads=2, max_position_embeddings=256, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    c.update(kw)
    return Phi3ForCausalLM(Phi3Config(**c)).eval()


def test_enable_fused_prefill_patches_every_phi3_layer():
    from u2tokenizer_amd.prefill import _PackedLayout, disable_fused_prefill, enable_fused_prefill
    m = _phi3(num_hidden_layers=3)
    assert m.model.layers[0].self_attn.head_dim == 96
    assert enable_fused_prefill(m, strict=True) == 3
    for lay in m.model.layers:
        assert lay._u2_prefill.layout is _PackedLayout
        pr = _PackedLayout.projections(lay)
        _, W, b = _PackedLayout.product(pr, 0)
        assert W is lay.self_attn.qkv_proj.weight and b is None   # used as they are: no repacking
        assert _PackedLayout.product(pr, 2)[1] is lay.mlp.gate_up_proj.weight
        assert _PackedLayout.ready(lay, lay.self_attn)
    with torch.no_grad():   # on the host the patched layers hand every call to their stock forward
        ids = torch.arange(10)[None] % 128
        got = m(input_ids=ids).logits
        disable_fused_prefill(m)
        assert torch.equal(got, m(input_ids=ids).logits)
    # grouped heads of 128 (Phi-3-medium-like) and 64 take the path too
    assert enable_fused_prefill(_phi3(hidden_size=512, num_attention_heads=4, num_key_value_heads=2), strict=True) == 2
    assert enable_fused_prefill(_phi3(hidden_size=256, num_attention_heads=4, num_key_value_heads=4), strict=True) == 2


@pytest.mark.parametrize("kw", [dict(partial_rotary_factor=0.5), dict(hidden_act="gelu_new"),
                                dict(hidden_size=192, num_attention_heads=4, num_key_value_heads=4)])
def test_phi3_layers_the_kernels_do_not_compute_stay_stock(kw):
    from u2tokenizer_amd.prefill import enable_fused_prefill, is_patched
    m = _phi3(**kw)
    assert enable_fused_prefill(m, strict=False) == 0
    assert not any(is_patched(lay) for lay in m.model.layers)
    with pytest.raises(RuntimeError, match="unsupported decoder layer"):
        enable_fused_prefill(m)


def test_phi3_training_mode_with_residual_dropout_takes_the_stock_forward():
    from u2tokenizer_amd.prefill import _PackedLayout, enable_fused_prefill
    m = _phi3(resid_pdrop=0.1)
    assert enable_fused_prefill(m) == 2
    lay = m.model.layers[0]
    assert _PackedLayout.ready(lay, lay.self_attn)          # eval: dropout inactive
    m.train()
    assert not _PackedLayout.ready(lay, lay.self_attn)
    m2 = _phi3(resid_pdrop=0.0)
    enable_fused_prefill(m2)
    m2.train()
    assert _PackedLayout.ready(m2.model.layers[0], m2.model.layers[0].self_attn)   # training mode with nothing to drop


def test_the_sliding_window_cache_layer_is_taken_only_for_windowed_layers():
    from transformers.cache_utils import DynamicCache, DynamicSlidingWindowLayer
    from u2tokenizer_amd.kv_cache import DENSE, SLIDING, layer_kind
    from u2tokenizer_amd.prefill import _PackedLayout
    m = _phi3(sliding_window=32)
    assert _PackedLayout.window(m.model.layers[0]) == 32
    cache = DynamicCache(config=m.config)
    assert type(cache.layers[0]) is DynamicSlidingWindowLayer
    kv = torch.zeros(1, 2, 5, 96)
    cache.update(kv, kv, 0)
    assert layer_kind(cache, 0, 1) == (SLIDING, cache.layers[0])     # (a kind of its own: `route` takes it under a window alone)
    plain = DynamicCache()
    plain.update(kv, kv, 0)
    assert layer_kind(plain, 0, 1) == (DENSE, plain.layers[0])
