"""CPU: the decoder training route's host side -- which attention masks it computes (the pure mask rule, and the verdict on
the 4-D masks HF hands the layers) -- and the new C-ABI entry points refusing NULL or inconsistent arguments with
U2TOK_ERR_ARG before touching any memory (no GPU needed: nothing is launched)."""
import pytest
import torch

from u2tokenizer_amd import _lib
from u2tokenizer_amd.decoder_train import layer_mask_kv_len, train_mask_rule

ERR_ARG, ERR_WS = -1, -3


def test_mask_rule_all_ones_and_none_are_plain_causal():
    assert train_mask_rule(None) == ("causal", None)
    assert train_mask_rule(torch.ones(3, 17, dtype=torch.int64)) == ("causal", None)


def test_mask_rule_right_padding_gives_lengths():
    m = torch.zeros(3, 10, dtype=torch.int64)
    m[0, :10], m[1, :4], m[2, :1] = 1, 1, 1
    kind, lens = train_mask_rule(m)
    assert kind == "lengths" and lens.tolist() == [10, 4, 1]
    kind, lens = train_mask_rule(m.bool())
    assert kind == "lengths" and lens.tolist() == [10, 4, 1]


@pytest.mark.parametrize("case", ["left", "hole", "empty", "3d"])
def test_mask_rule_sends_everything_else_to_the_stock_layers(case):
    m = torch.ones(2, 8, dtype=torch.int64)
    if case == "left":
        m[1, :3] = 0
    elif case == "hole":
        m[0, 4] = 0
    elif case == "empty":
        m[1] = 0
    else:
        m = m[None]
    assert train_mask_rule(m) is None


def _hf_mask(lens, S, as_float=False):
    pos = torch.arange(S)
    vis = (pos[None, :] <= pos[:, None])[None] & (pos[None, None, :] < torch.tensor(lens)[:, None, None])
    vis = vis[:, None]
    if as_float:
        return torch.zeros(vis.shape).masked_fill(~vis, torch.finfo(torch.float32).min)
    return vis


@pytest.mark.parametrize("as_float", [False, True])
def test_layer_mask_verdict(as_float):
    assert layer_mask_kv_len(None, 2, 9) == (True, None)
    ok, kv = layer_mask_kv_len(_hf_mask([9, 9], 9, as_float), 2, 9)
    assert ok and kv is None
    am = _hf_mask([9, 5], 9, as_float)
    ok, kv = layer_mask_kv_len(am, 2, 9)
    assert ok and kv.dtype == torch.int32 and kv.tolist() == [9, 5]
    assert layer_mask_kv_len(am, 2, 9)[1] is kv            # stored on the mask: the recompute reads the same verdict
    # left padding / a sliding window / another shape: stock
    left = _hf_mask([9, 9], 9, False).clone()
    left[1, 0, :, :2] = False
    assert layer_mask_kv_len(left, 2, 9) == (False, None)
    band = _hf_mask([9, 9], 9, False).clone()
    band[:, 0, 8, 0] = False
    assert layer_mask_kv_len(band, 2, 9) == (False, None)
    assert layer_mask_kv_len(_hf_mask([9, 9], 9), 3, 9) == (False, None)


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


def test_new_entry_points_reject_null_and_inconsistent_arguments(lib):
    P = 1 << 20   # a 256-byte aligned address that is never dereferenced: every call below returns before any access
    # forward with key lengths
    assert lib.u2tok_attention_gqa_ex(None, None, None, None, 1, 8, 8, 4, 2, 64, 512, 512, 512, 256, 0, 0, 0, 0, 0.125, 1, P, None,
                                      0, None) == ERR_ARG
    assert lib.u2tok_attention_gqa_ex(P, P, P, P, 1, 8, 8, 4, 3, 64, 512, 512, 512, 256, 0, 0, 0, 0, 0.125, 1, P, None, 0,
                                      None) == ERR_ARG                                # Hq % Hkv
    assert lib.u2tok_attention_gqa_ex(P, P, P, P, 1, 8, 8, 4, 2, 64, 512, 512, 512, 256, 0, 0, 0, 0, 0.125, 1, None, P, 4,
                                      None) == ERR_ARG                                # lse_ld < Sq
    # backward
    args = [P, P, P, 512, 8 * 512, P, P, 256, 8 * 256, P, P, P, 512, 8 * 512, 1, 8, 4, 2, 64, 0.125, None, None, 0, P, 1 << 20,
            None]
    bad = list(args)
    bad[0] = None
    assert lib.u2tok_attention_gqa_bwd(*bad) == ERR_ARG
    bad = list(args)
    bad[23] = None
    assert lib.u2tok_attention_gqa_bwd(*bad) == ERR_ARG                              # no workspace
    bad = list(args)
    bad[18] = 96
    assert lib.u2tok_attention_gqa_bwd(*bad) == ERR_ARG                              # head dim 96: not built
    bad = list(args)
    bad[17] = 3
    assert lib.u2tok_attention_gqa_bwd(*bad) == ERR_ARG                              # Hq % Hkv
    bad = list(args)
    bad[24] = 16
    assert lib.u2tok_attention_gqa_bwd(*bad) == ERR_WS
    assert lib.u2tok_attention_gqa_bwd_workspace_bytes(1, 8, 4) > 0
    assert lib.u2tok_attention_gqa_bwd_workspace_bytes(0, 8, 4) == 0
    # RMSNorm
    assert lib.u2tok_rmsnorm_bwd(None, P, P, None, P, P, 4, 64, 1e-6, P, 1 << 20, 0, None) == ERR_ARG
    assert lib.u2tok_rmsnorm_bwd(P, P, P, None, P, None, 4, 64, 1e-6, P, 1 << 20, 0, None) == ERR_ARG   # no dw
    assert lib.u2tok_rmsnorm_bwd(P, P, P, None, P, P, 4, 8192, 1e-6, P, 1 << 30, 0, None) == ERR_ARG   # C > 4096
    assert lib.u2tok_rmsnorm_bwd(P, P, P, None, P, P, 4, 60, 1e-6, P, 1 << 20, 0, None) == ERR_ARG     # C % 8
    assert lib.u2tok_rmsnorm_bwd(P, P, P, None, P, P, 4, 64, 1e-6, P, 4, 0, None) == ERR_WS
    # head norm + rotary
    assert lib.u2tok_qk_norm_rope_bwd(None, None, None, None, P, P, 1, 4, 4, 2, 64, 512, 0, 64, 1e-6, None, None, None, 0, 0,
                                      None) == ERR_ARG
    assert lib.u2tok_qk_norm_rope_bwd(P, P, P, None, P, P, 1, 4, 4, 2, 64, 512, 384, 64, 1e-6, P, P, P, 1 << 20, 0,
                                      None) == ERR_ARG                                # wq without wk
    assert lib.u2tok_qk_norm_rope_bwd(P, None, P, P, P, P, 1, 4, 4, 2, 64, 512, 384, 64, 1e-6, P, P, P, 1 << 20, 0,
                                      None) == ERR_ARG                                # norm without the pre-norm heads
    assert lib.u2tok_qk_norm_rope_bwd(P, None, None, None, P, P, 1, 4, 4, 2, 64, 256, 0, 64, 1e-6, None, None, None, 0, 0,
                                      None) == ERR_ARG                                # ld < (Hq + 2 Hkv) D
    # SwiGLU
    assert lib.u2tok_swiglu_bwd(None, P, P, 4, 64, 128, 64, 128, None) == ERR_ARG
    assert lib.u2tok_swiglu_bwd(P, P, P, 4, 12, 24, 12, 24, None) == ERR_ARG          # I % 8
    assert lib.u2tok_swiglu_bwd(P, P, P, 4, 64, 64, 64, 128, None) == ERR_ARG         # ld_gu < 2 I
