"""CPU: the argument checks of the fused attention forward's exported entry points (csrc/tokattn.hip behind csrc/capi.hip), as a
table over both element builds.  Every case is a refusal, which returns before any launch: the addresses are aligned and never
dereferenced.  Which entry refuses what is part of the C ABI, so the table holds across any rearrangement of the host side."""
import pytest

from u2tokenizer_amd import _lib

ARG, WORKSPACE = -1, -3   # U2TOK_ERR_ARG, U2TOK_ERR_WORKSPACE
P = 1 << 20               # an aligned address that is never dereferenced

COMMON = ["q", "k", "v", "out", "nb", "Sq", "Skv", "Hq", "Hkv", "d", "ldq", "ldk", "ldv", "ldo", "q_bs", "k_bs", "v_bs", "o_bs",
          "scale"]
RANGE = ["causal", "kv_start", "kv_len", "lse", "lse_ld"]
ENTRIES = {   # the arguments of include/u2tok.h, in order
    "u2tok_tok_attention": [n for n in COMMON if n != "Hkv"] + ["rel_bias", "max_len", "splits", "ws", "ws_bytes", "stream"],
    "u2tok_attention_gqa": COMMON + ["causal", "stream"],
    "u2tok_attention_gqa_split": COMMON + ["ws", "ws_bytes", "stream"],
    "u2tok_attention_gqa_ex": COMMON + ["causal", "kv_len", "lse", "lse_ld", "stream"],
    "u2tok_attention_gqa_range": COMMON + RANGE + ["stream"],
    "u2tok_attention_gqa_band": COMMON + RANGE + ["k_hs", "v_hs", "window", "stream"],
}
TOK, GQA, SPLIT, EX, RNG, BAND = ENTRIES
CAUSAL = (GQA, EX, RNG, BAND)
GROUPED = (GQA, SPLIT, EX, RNG, BAND)


def _call(h, entry, **kw):
    """`entry` on a call it would take -- 8 query rows over 24 keys, 4 query heads (2 kv heads where it has them), d = 64,
    column-packed operands -- with the fields of `kw` replaced."""
    f = dict(q=P, k=P, v=P, out=P, nb=1, Sq=8, Skv=24, Hq=4, Hkv=2, d=64, scale=0.125, causal=1, max_len=512, splits=0, ws_bytes=0,
             lse_ld=0, window=0)
    f.update(kw)
    d, Sq, Skv = f["d"], f["Sq"], f["Skv"]
    ldq = f["Hq"] * d
    ldk = (f["Hq"] if entry == TOK else f["Hkv"]) * d
    f = {**dict(ldq=ldq, ldk=ldk, ldv=ldk, ldo=ldq, q_bs=Sq * ldq, k_bs=Skv * ldk, v_bs=Skv * ldk, o_bs=Sq * ldq, k_hs=d, v_hs=d), **f}
    return getattr(h, entry)(*[f.get(n) for n in ENTRIES[entry]])


CACHE = dict(k_hs=64 * 64, v_hs=64 * 64)   # a KV cache view: the kv heads 64 positions apart

# name -> (entries, fields, status)
TABLE = {
    **{f"null {p}": (tuple(ENTRIES), {p: None}, ARG) for p in ("q", "k", "v", "out")},
    "Hq % Hkv": (GROUPED, dict(Hq=3), ARG),
    "causal with Skv < Sq": (CAUSAL, dict(Sq=32), ARG),
    "rel_bias with max_len < Sq": ((TOK,), dict(rel_bias=P, max_len=7), ARG),
    "head dim 32": (tuple(ENTRIES), dict(d=32), ARG),
    "head dim 32, key range": ((EX, RNG, BAND), dict(d=32, kv_len=P), ARG),
    "head dim 32, cache view": ((BAND,), dict(d=32, k_hs=64 * 32, v_hs=64 * 32), ARG),
    "head dim 384 with kv_len": ((EX,), dict(d=384, kv_len=P), ARG),
    "head dim 384 with lse": ((EX,), dict(d=384, lse=P, lse_ld=8), ARG),
    "head dim 384 with kv_start": ((RNG,), dict(d=384, kv_start=P), ARG),
    "head dim 384 on a cache view": ((BAND,), dict(d=384, k_hs=64 * 384, v_hs=64 * 384), ARG),
    "head dim 384 with a window": ((BAND,), dict(d=384, window=16), ARG),
    "head dim 256 with a window": ((BAND,), dict(d=256, window=16), ARG),
    "lse with lse_ld < Sq": ((EX, RNG, BAND), dict(lse=P, lse_ld=7), ARG),
    "lse with lse_ld < Sq, cache view": ((BAND,), dict(lse=P, lse_ld=7, **CACHE), ARG),
    "misaligned kv_len": ((EX, RNG, BAND), dict(kv_len=P + 2), ARG),
    "misaligned kv_len, cache view": ((BAND,), dict(kv_len=P + 2, **CACHE), ARG),
    "misaligned kv_start": ((RNG, BAND), dict(kv_start=P + 2), ARG),
    "misaligned lse": ((EX, RNG, BAND), dict(lse=P + 2, lse_ld=8), ARG),
    # 4 splits of one 64-key tile each; a split's partial sums: nb * Sq * (H * d * 4 + H * 8) = 8 * (1024 + 32) bytes
    "forced splits without a workspace": ((TOK,), dict(splits=4, Skv=256), WORKSPACE),
    "forced splits, workspace one byte short": ((TOK,), dict(splits=4, Skv=256, ws=P, ws_bytes=4 * 8448 - 1), WORKSPACE),
}


@pytest.mark.parametrize("elem", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(TABLE))
def test_entry_point_refuses_before_any_launch(name, elem):
    h = _lib.load_library(elem)
    entries, fields, status = TABLE[name]
    for entry in entries:
        assert _call(h, entry, **fields) == status, entry
