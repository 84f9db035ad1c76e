"""CPU: head dim 96 on the decoder's training route, host side (no GPU: nothing is launched).

  * the bf16 emulations of the flash backward and of the attention forward (tests/test_decoder_train_bounds_host.py) stay inside
    the first-order float64 bounds at d = 96 on the cases the GPU test holds the kernels to (tests/attn_d96_cases.py);
  * u2tok_attention_gqa_bwd_d96 is declared in include/u2tok.h, exported by both element builds and bound in _lib.py, and refuses
    NULL or inconsistent arguments before any access, as u2tok_attention_gqa_bwd does (which keeps refusing d = 96)."""
import re
from pathlib import Path

import pytest

import test_decoder_train_bounds_host as B
from attn_d96_cases import D96_CASES, case_id, inputs, model
from u2tokenizer_amd import _lib

ERR_ARG, ERR_WS = -1, -3
ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("case", D96_CASES, ids=case_id)
def test_emulation_inside_bound_at_head_dim_96(case):
    nb, S, Hq, Hkv, d, lens = case
    inp, m, scale = inputs(case), model(case), d ** -0.5
    for name, e in zip(("dq", "dk", "dv"), B.attn_bwd_emulate(inp["qkv"], inp["dout"], Hq, Hkv, d, scale, lens)):
        r = B.worst((e - m[name]).abs(), m[name + "_bound"])
        print(f"emulated error / bound, flash backward d = 96 {name}: {r:.3f}")
        assert r < 1.0, (name, r)
    x = inp["qkv"]
    q, k, v = B.heads(x[..., :Hq * d], Hq, d), B.heads(x[..., Hq * d:(Hq + Hkv) * d], Hkv, d), B.heads(x[..., (Hq + Hkv) * d:], Hkv, d)
    vis = B.visible(nb, S, S, lens)
    f = B.attn_fwd_model(q, k, v, scale, vis)
    r = B.worst((B.attn_fwd_emulate(q, k, v, scale, vis) - f["out"]).abs(), f["out_bound"])
    print(f"emulated error / bound, attention forward d = 96 out: {r:.3f}")
    assert r < 1.0, r
    if lens is not None:   # keys at or beyond the length get exactly zero
        for b, n in enumerate(lens):
            assert (m["dk"][b, n:] == 0).all() and (m["dv"][b, n:] == 0).all()


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


def test_d96_entry_point_is_declared_and_bound():
    header = (ROOT / "include" / "u2tok.h").read_text()
    decl = re.search(r"\bint\s+u2tok_attention_gqa_bwd_d96\s*\(([^;]*)\)\s*;", header)
    assert decl, "u2tok_attention_gqa_bwd_d96 is not declared in include/u2tok.h"
    general = re.search(r"\bint\s+u2tok_attention_gqa_bwd\s*\(([^;]*)\)\s*;", header)
    norm = lambda a: [" ".join(p.split()) for p in a.split(",")]
    assert norm(decl.group(1)) == [p for p in norm(general.group(1)) if p != "int32_t d"]   # the same list without d
    sig, gen = _lib.SIGNATURES["u2tok_attention_gqa_bwd_d96"], _lib.SIGNATURES["u2tok_attention_gqa_bwd"]
    assert sig[0] is gen[0] and list(sig[1]) == list(gen[1][:18]) + list(gen[1][19:]) and len(sig[1]) == len(norm(decl.group(1)))


def test_d96_entry_point_rejects_null_and_inconsistent_arguments(lib):
    assert hasattr(lib, "u2tok_attention_gqa_bwd_d96")
    P = 1 << 20   # a 256-byte aligned address that is never dereferenced: every call below returns before any access
    nb, S, Hq, Hkv, W = 1, 8, 4, 2, 8 * 96
    args = [P, P, P, W, S * W, P, P, Hq * 96, S * Hq * 96, P, P, P, W, S * W, nb, S, Hq, Hkv, 96 ** -0.5, None, None, 0, P, 1 << 20, None]
    fn = lib.u2tok_attention_gqa_bwd_d96

    def bad(**changes):
        a = list(args)
        for i, v in changes.items():
            a[int(i[1:])] = v
        return fn(*a)

    for i in (0, 1, 2, 5, 6, 9, 10, 11):
        assert bad(**{f"a{i}": None}) == ERR_ARG, f"NULL pointer argument {i}"
    assert bad(a22=None) == ERR_ARG                               # no workspace
    assert bad(a17=3) == ERR_ARG                                  # Hq % Hkv
    assert bad(a3=W + 4) == ERR_ARG                               # ld_qkv not a multiple of 8 elements
    assert bad(a7=Hq * 96 + 4) == ERR_ARG                         # ld_o likewise
    assert bad(a12=W + 2) == ERR_ARG                              # ld_d not a multiple of 4
    assert bad(a12=Hq * 96 - 4) == ERR_ARG                        # ld_d below Hq d
    assert bad(a0=P + 8) == ERR_ARG                               # q not 16-byte aligned
    assert bad(a22=P + 128) == ERR_ARG                            # workspace not 256-byte aligned
    assert bad(a20=P, a21=S - 1) == ERR_ARG                       # lse_ld < S
    assert bad(a18=0.0) == ERR_ARG                                # scale
    assert bad(a14=2, a4=S * W - 8) == ERR_ARG                    # overlapping batches
    need = lib.u2tok_attention_gqa_bwd_workspace_bytes(nb, S, Hq)
    assert need > 0
    assert bad(a23=need - 1) == ERR_WS and bad(a23=16) == ERR_WS  # a short workspace
    # the general entry point keeps refusing head dim 96, whatever else is right
    general = args[:18] + [96] + args[18:]
    assert lib.u2tok_attention_gqa_bwd(*general) == ERR_ARG
