"""CPU: the C-ABI library -- both builds of it: bf16 elements (libu2tok_hip.so) and IEEE-half elements (libu2tok_hip_f16.so) --
builds, loads and exports exactly what include/u2tok.h declares (no compute calls)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from u2tokenizer_amd import _lib

ROOT = Path(__file__).resolve().parents[1]


def _declared():
    text = (ROOT / "include" / "u2tok.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(u2tok_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    h = _lib.load_library(request.param)
    assert h.u2tok_elem() == request.param.encode()
    return h


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/u2tok.h but not exported by {_lib.lib_path().name}"
    assert sorted(_lib.SIGNATURES) == names, set(_lib.SIGNATURES) ^ set(names)


def test_identity(lib):
    assert lib.u2tok_version() >= 100
    assert lib.u2tok_arch() == b"gfx950"
    assert lib.u2tok_set_option(b"no_such_option", 1) == -1


def test_config_struct_sizes_match_header():
    # the header uses only int32_t / float fields: packed size must be 4 * nfields
    assert C.sizeof(_lib.VitConfig) == 4 * 14
    assert C.sizeof(_lib.SppConfig) == 4 * 10
    assert C.sizeof(_lib.TokConfig) == 4 * 16


def test_workspace_sizing_runs_without_a_gpu(lib):
    cfg = _lib.VitConfig(nchunk=8, img=(C.c_int32 * 3)(32, 256, 256), patch=(C.c_int32 * 3)(4, 16, 16), hidden=768,
                         mlp_dim=3072, depth=12, heads=12, vol_dtype=0, keep_cls=0, ln_eps=1e-5)
    assert lib.u2tok_vit_workspace_bytes(C.byref(cfg)) > 100 << 20
    cfg.heads = 7  # hidden != heads * 64 -> rejected
    assert lib.u2tok_vit_workspace_bytes(C.byref(cfg)) == 0
    t = _lib.TokConfig(B=1, T=8, N=256, E=4096, Lt=1024, num_heads=8, num_layers=4, top_k=1024, num_query=256,
                       use_multi_scale=1, attn_type=0, enable_diffts=1, enable_dmtp=1, max_seq_len=512,
                       diffts_tau=1.0, ln_eps=1e-5)
    assert lib.u2tok_tokenizer_workspace_bytes(C.byref(t)) > 64 << 20
    t.N = 600  # > max_seq_len: RelativeMultiheadAttention cannot index its bias table (rma.py:64-68)
    assert lib.u2tok_tokenizer_workspace_bytes(C.byref(t)) == 0
    t.N, t.enable_diffts, t.top_k = 256, 0, 4096  # top_k > T*N: torch.topk would raise
    assert lib.u2tok_tokenizer_workspace_bytes(C.byref(t)) == 0


def test_null_arguments_are_rejected_not_dereferenced(lib):
    assert lib.u2tok_gemm_bf16(None, None, None, None, None, 8, 8, 8, 8, 8, 8, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0,
                               None) == -1
    assert lib.u2tok_gemm_bf16_ex(None, None, None, None, None, 8, 8, 8, 8, 8, 8, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0,
                                  0, 1.0, None, 0, 0, 0, 0, None) == -1
    assert lib.u2tok_topk_sorted(None, None, 1, 8, 4, None) == -1
    assert lib.u2tok_im2col_patches(None, 0, None, 1, 32, 64, 64, 4, 16, 16, None) == -1


def test_flash_attention_d64_bwd_rejects_bad_arguments(lib):
    """u2tok_flash_attention_d64_bwd returns before any launch or memory access on arguments it cannot take."""
    ERR_ARG, ERR_WS = -1, -3
    P = 1 << 20   # a 256-byte aligned address that is never dereferenced
    H, S = 4, 8
    # q, k, v, ld_qkv, bs_qkv, out, d_out, ld_o, bs_o, dq, dk, dv, ld_d, bs_d, nb, S, H, scale, lse, lse_ld, ws, ws_bytes, stream
    args = [P, P + 512, P + 1024, 3 * H * 64, S * 3 * H * 64, P, P, H * 64, S * H * 64, P, P + 512, P + 1024, 3 * H * 64,
            S * 3 * H * 64, 1, S, H, 0.125, None, 0, P, 1 << 20, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.u2tok_flash_attention_d64_bwd(*a)

    for i in (0, 1, 2, 5, 6, 9, 10, 11, 20):                  # every pointer but lse and the stream
        assert call(**{f"a{i}": None}) == ERR_ARG, i
    assert call(a3=3 * H * 64 + 4) == ERR_ARG                 # ld_qkv not a multiple of 8 elements
    assert call(a7=H * 64 + 4) == ERR_ARG                     # ld_o likewise
    assert call(a12=3 * H * 64 + 2) == ERR_ARG                # ld_d not a multiple of 4 elements
    assert call(a3=H * 64 - 8) == ERR_ARG                     # ld < H * 64
    assert call(a7=H * 64 - 8) == ERR_ARG
    assert call(a12=H * 64 - 8) == ERR_ARG
    assert call(a0=P + 8) == ERR_ARG                          # q not 16-byte aligned
    assert call(a20=P + 128) == ERR_ARG                       # workspace not 256-byte aligned
    assert call(a14=0) == ERR_ARG and call(a15=0) == ERR_ARG and call(a16=0) == ERR_ARG
    assert call(a17=0.0) == ERR_ARG                           # scale must be positive
    assert call(a14=16384, a16=4) == ERR_ARG                  # nb * H > 65535
    assert call(a18=P, a19=S - 1) == ERR_ARG                  # lse_ld < S
    assert call(a18=P + 2, a19=S) == ERR_ARG                  # lse not 4-byte aligned
    assert call(a21=16) == ERR_WS                             # short workspace
    need = lib.u2tok_flash_attention_d64_bwd_workspace_bytes(1, S, H)
    assert need == 2 * 256 * ((H * 64 * 4 + 255) // 256) and call(a21=need - 1) == ERR_WS
    assert lib.u2tok_flash_attention_d64_bwd_workspace_bytes(0, S, H) == 0
    assert lib.u2tok_flash_attention_d64_bwd_workspace_bytes(1, 0, H) == 0
    assert lib.u2tok_flash_attention_d64_bwd_workspace_bytes(1, S, 0) == 0
