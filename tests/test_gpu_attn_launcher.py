"""GPU: the entry points of the fused attention forward that are documented to be one kernel give one set of bits, on the bf16 and
the f16 build: u2tok_tok_attention and u2tok_attention_gqa at equal heads, the key-split forms of both, u2tok_attention_gqa_ex
without a key length or statistics and u2tok_attention_gqa, and u2tok_attention_gqa_band on a KV cache view against
u2tok_attention_gqa_range on the column-packed copy.  Sq = 70 over Skv = 130: a ragged last query block and a ragged last key tile
(64- and 32-key tiles alike)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
D = "cuda"
ELEMS = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="f16")]
SQ, SKV = 70, 130


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


def rnd(*shape, seed=0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed * 7919 + sum(shape))
    return torch.randn(*shape, generator=g).to(dtype).to(D)


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("d", [64, 256])
def test_tok_attention_is_attention_gqa_at_equal_heads(ops, elem, d):
    """12 sequences of 8 heads: 192 (batch, head, 64-query) units, at which tok_attention's heuristic cuts no key splits (at d = 256
    the 130 keys are 5 tiles, enough for two splits on fewer units) -- so both entries are the unsplit kernel."""
    nb, H = 12, 8
    q, k, v = rnd(nb, SQ, H * d, seed=1, dtype=elem), rnd(nb, SKV, H * d, seed=2, dtype=elem), rnd(nb, SKV, H * d, seed=3, dtype=elem)
    a = ops.tok_attention(q, k, v, H, d ** -0.5)
    assert torch.equal(a, ops.attention_gqa(q, k, v, H, H, d ** -0.5, causal=False)) and a.abs().max() > 0


@pytest.mark.parametrize("elem", ELEMS)
def test_split_keys_is_tok_attentions_heuristic_split(ops, elem):
    """2 units over 8 key tiles: the heuristic gives 4 splits, so both calls go through the combine kernel."""
    nb, H, Sq, Skv, d = 1, 2, 64, 512, 128
    assert ops._lib.load_library().u2tok_tok_attention_workspace_bytes(nb, H, Sq, Skv, d) == 4 * nb * Sq * (H * d * 4 + H * 8)
    q, k, v = rnd(nb, Sq, H * d, seed=4, dtype=elem), rnd(nb, Skv, H * d, seed=5, dtype=elem), rnd(nb, Skv, H * d, seed=6, dtype=elem)
    a = ops.attention_gqa(q, k, v, H, H, d ** -0.5, causal=False, split_keys=True)
    assert torch.equal(a, ops.tok_attention(q, k, v, H, d ** -0.5, splits=0)) and a.abs().max() > 0


@pytest.mark.parametrize("elem", ELEMS)
def test_attention_gqa_ex_without_a_key_length_is_attention_gqa(ops, elem):
    nb, Hq, Hkv, d = 2, 4, 2, 96
    q, k, v = rnd(nb, SQ, Hq * d, seed=7, dtype=elem), rnd(nb, SKV, Hkv * d, seed=8, dtype=elem), rnd(nb, SKV, Hkv * d, seed=9, dtype=elem)
    a, lse = ops.attention_gqa_ex(q, k, v, Hq, Hkv, d ** -0.5)
    assert lse is None
    assert torch.equal(a, ops.attention_gqa(q, k, v, Hq, Hkv, d ** -0.5, causal=True)) and a.abs().max() > 0


@pytest.mark.parametrize("elem", ELEMS)
def test_band_on_a_cache_view_is_range_on_the_packed_copy(ops, elem):
    nb, Hq, Hkv, d, cap = 2, 4, 2, 128, 192
    q = rnd(nb, SQ, Hq * d, seed=10, dtype=elem)
    K, V = rnd(nb, Hkv, cap, d, seed=11, dtype=elem)[:, :, :SKV], rnd(nb, Hkv, cap, d, seed=12, dtype=elem)[:, :, :SKV]
    assert not K.is_contiguous()
    ck, cv = (t.transpose(1, 2).reshape(nb, SKV, Hkv * d).contiguous() for t in (K, V))
    a = ops.attention_gqa_band(q, K, V, Hq, Hkv, d ** -0.5, window=None)
    assert torch.equal(a, ops.attention_gqa_range(q, ck, cv, Hq, Hkv, d ** -0.5)) and a.abs().max() > 0
