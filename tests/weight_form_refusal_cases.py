"""The cases of tests/test_gpu_weight_form_refusals.py: what the four few-rows exports (u2tok_gemm_rows, _w8, _w8_wide, _w4) and the
two halves of the decode step (u2tok_decoder_decode_pre / _post) ANSWER -- the returned status -- over the ways a call can say its
weight form, pinned in tests/golden/weight_form_refusals.json.  Recorded with the library of the commit named inside it, in which
every layer below the C API inferred the form from which scale pointer was set; a later change of how the form travels must
leave every status where it was, accepted calls included.

Every pointer is a real device allocation, large enough for the largest accepted call of the table, and a misaligned pointer an
in-bounds offset into it: a call that some change wrongly accepts computes into scratch and cannot fault.  All buffers hold zeros.

The nominal calls: M = 1, N = 16, K = 128; a decode step with B = 1, E = Hq D = 128 (2 query heads, 1 kv head of 64), I = 128 over a
cache of 8 positions.  The grid: the form x wform 0 .. 3 x which of the four scales are set; K, E, Hq D or I off the multiple of a
form (32 / 64 / 128); weight, scale and activation pointers off their alignment; ldw / lds / lda below the row; M (B) in {0, 16, 17,
64, 65}; unknown flags, the pair form with other flags.  Importable without a GPU (the host half of the test reads the case list).

`python tests/weight_form_refusal_cases.py --record --commit HASH [--out FILE]` runs every case on the GPU and writes the fixture;
the test itself only ever reads it."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

FIXTURE = Path(__file__).resolve().parent / "golden" / "weight_form_refusals.json"
BUF_BYTES, WS_BYTES = 1 << 20, 1 << 24   # every buffer; the decode step's workspace
BIAS, RES, F32, PAIR = 1, 8, 16, 512     # GEMM_BIAS_N, GEMM_RESIDUAL, GEMM_OUT_F32, GEMM_SWIGLU (include/u2tok.h)
ROWS_EXPORTS = {"rows": "u2tok_gemm_rows", "w8": "u2tok_gemm_rows_w8", "w8wide": "u2tok_gemm_rows_w8_wide", "w4": "u2tok_gemm_rows_w4"}
SCALES = ("scale_qkv", "scale_o", "scale_gu", "scale_down")
WEIGHTS = ("Wqkv", "Wo", "Wgu", "Wdown")


def P(name, off=0):
    """A pointer of a case: `off` bytes into the buffer `name`"""
    return ("ptr", name, off)


# ------------------------------------------------------------------------------------------------------------- the few-rows exports
def _rows(export, **kw):
    """The named arguments of one call of a few-rows export; ld* default to the packed rows of the export's form"""
    a = dict(A=P("A"), W=P("W"), S=P("S"), C=P("C"), bias=None, R=None, M=1, N=16, K=128, ldr=0, flags=0)
    a.update(kw)
    K, N = a["K"], a["N"]
    a.setdefault("lda", K)
    a.setdefault("ldw", K // 2 if export == "w4" else K)
    a.setdefault("lds", K // 32)
    a.setdefault("ldc", N // 2 if a["flags"] & PAIR else N)
    return (export, a)


def rows_cases():
    out = {}
    for ex in ROWS_EXPORTS:
        add = lambda name, _ex=ex, **kw: out.__setitem__(f"{_ex}-{name}", _rows(_ex, **kw))   # noqa: E731
        codes = ex != "rows"
        add("nominal")
        for K in (32, 64, 96, 160, 192, 256):
            add(f"K{K}", K=K)
        for M in (0, 16, 17, 64, 65):
            add(f"M{M}", M=M)
        for n in ("A", "W", "C"):
            add(f"null-{n}", **{n: None})
            add(f"{n}-off8", **{n: P(n, 8)})
        add("C-off1", C=P("C", 1))
        add("C-off2-f32", C=P("C", 2), flags=F32)
        if codes:
            add("null-S", S=None)
            for off in (1, 2, 4):
                add(f"S-off{off}", S=P("S", off))
        add("lda-below", lda=120)
        add("lda-off4", lda=132)
        add("lda-wide", lda=136)
        nominal_ldw = 64 if ex == "w4" else 128
        add("ldw-below", ldw=nominal_ldw - 16)
        add("ldw-off8", ldw=nominal_ldw + 8)
        add("ldw-wide", ldw=nominal_ldw + 16)
        if ex == "w4":
            add("lds-below", lds=3)
            add("lds-wide", lds=5)
        add("ldc-below", ldc=8)
        add("N0", N=0)
        add("N24", N=24)
        for f in (2, 4, 32, 1 << 20):
            add(f"flags{f}", flags=f)
        add("bias-null", flags=BIAS)
        add("bias", flags=BIAS, bias=P("bias"))
        add("res-null", flags=RES)
        add("res", flags=RES, R=P("R"), ldr=16)
        add("res-ldr-below", flags=RES, R=P("R"), ldr=8)
        add("bias-res-f32", flags=BIAS | RES | F32, bias=P("bias"), R=P("R"), ldr=24)
        add("pair", flags=PAIR)
        add("pair-N24", flags=PAIR, N=24)
        add("pair-bias", flags=PAIR | BIAS, bias=P("bias"))
        add("pair-res", flags=PAIR | RES, R=P("R"), ldr=16)
        add("pair-f32", flags=PAIR | F32)
        add("pair-ldc-below", flags=PAIR, ldc=4)
    return out


def rows_argv(export, a, resolve, stream):
    """The positional arguments of the export (include/u2tok.h)"""
    p = lambda n: resolve(a[n])   # noqa: E731
    scale = [] if export == "rows" else [p("S")]
    lds = [a["lds"]] if export == "w4" else []
    return [p("A"), p("W"), *scale, p("C"), p("bias"), p("R"), a["M"], a["N"], a["K"], a["lda"], a["ldw"], *lds, a["ldc"], a["ldr"],
            a["flags"], stream]


# ------------------------------------------------------------------------------------------------------------- the decode step
def _decode(half, cfg=None, lay=None, batched=0, x=P("x")):
    """One call of a half of the step.  cfg: fields of u2tok_decode_config over the nominal ones; lay: fields of u2tok_decode_layer over
    the nominal 16-bit layer (the four weights, the two norms, no bias, no head norm, no scale)"""
    c = dict(B=1, E=128, Hq=2, Hkv=1, D=64, I=128, eps=1e-6, qk_eps=1e-6, scale=0.125, wform=0)
    c.update(cfg or {})
    fields = dict(w_in_norm=P("w_in_norm"), w_post_norm=P("w_post_norm"), **{w: P(w) for w in WEIGHTS})
    fields.update(lay or {})
    return (half, dict(cfg=c, lay=fields, batched=batched, x=x))


def _scales(which):
    return {n: P(n) for n in which}


FORMS = {"elem": (0, ()), "e4m3": (0, SCALES), "e2m1": (2, SCALES)}   # how the ABI says a form: (wform, the scales set)
HALVES = (("pre", 0), ("post", 0), ("post", 1))                        # (half, batched)


def decode_cases():
    out = {}
    for half, batched in HALVES:
        tag = half + ("-batched" if batched else "")
        add = lambda name, _h=half, _b=batched, _t=tag, **kw: out.__setitem__(f"{_t}-{name}", _decode(_h, batched=_b, **kw))   # noqa: E731
        # wform x which scales are set: none, each single one, all
        for wform in (0, 1, 2, 3):
            for name, which in (("none", ()), *((n, (n,)) for n in SCALES), ("all", SCALES)):
                add(f"wform{wform}-{name}", cfg=dict(wform=wform), lay=_scales(which))
        for form, (wform, which) in FORMS.items():
            sc = _scales(which)
            # E, Hq D, I off the form's multiple (and on it)
            for kw in (dict(E=32), dict(E=64), dict(E=96), dict(E=192), dict(E=256), dict(I=32), dict(I=64), dict(I=192), dict(I=320),
                       dict(I=256), dict(Hq=1), dict(Hq=3), dict(Hq=4), dict(Hq=4, Hkv=2), dict(D=96, Hq=4), dict(D=128, Hq=1)):
                add(f"{form}-" + "-".join(f"{k}{v}" for k, v in kw.items()), cfg=dict(wform=wform, **kw), lay=sc)
            for B in (0, 16, 17, 64, 65):
                add(f"{form}-B{B}", cfg=dict(wform=wform, B=B), lay=sc)
            for w in WEIGHTS:
                add(f"{form}-{w}-off8", cfg=dict(wform=wform), lay={**sc, w: P(w, 8)})
                add(f"{form}-{w}-null", cfg=dict(wform=wform), lay={**sc, w: None})
            for s in which:
                for off in (1, 2):
                    add(f"{form}-{s}-off{off}", cfg=dict(wform=wform), lay={**sc, s: P(s, off)})
            add(f"{form}-x-off8", cfg=dict(wform=wform), lay=sc, x=P("x", 8))
            add(f"{form}-x-null", cfg=dict(wform=wform), lay=sc, x=None)
            add(f"{form}-bias", cfg=dict(wform=wform), lay={**sc, "bqkv": P("bqkv"), "bo": P("bo"), "bgu": P("bgu"), "bdown": P("bdown")})
            add(f"{form}-head-norm", cfg=dict(wform=wform), lay={**sc, "wq_norm": P("wq_norm"), "wk_norm": P("wk_norm")})
    return out


def decode_call(lib, half, a, resolve, stream):
    from u2tokenizer_amd import _lib
    cfg = _lib.DecodeConfig(**a["cfg"])
    lay = _lib.DecodeLayer(**{k: resolve(v) for k, v in a["lay"].items()})
    r = lambda n: resolve(P(n))   # noqa: E731
    x = resolve(a["x"])
    if half == "pre":    # cfg, layer, x, cos, sin, cos_sin_f32, cs_ld, qkv, k_cache, v_cache, kv_stride, s_off, workspace, bytes, stream
        return lib.u2tok_decoder_decode_pre(C.byref(cfg), C.byref(lay), x, r("cos"), r("sin"), 1, 128, r("qkv"), r("kc"), r("vc"), 0, 0,
                                            r("ws"), WS_BYTES, stream)
    # cfg, layer, x, qkv, K, V, T, kv_stride, batched, kv_start, out, workspace, bytes, stream
    return lib.u2tok_decoder_decode_post(C.byref(cfg), C.byref(lay), x, r("qkv"), r("K"), r("V"), 8, 0, a["batched"], None, r("out"),
                                         r("ws"), WS_BYTES, stream)


# ------------------------------------------------------------------------------------------------------------- all of them
def cases():
    return {**rows_cases(), **decode_cases()}


def case_ids():
    return list(cases())


def largest_call_fits():
    """The sizes the buffers are chosen for: no accepted call of the table reads or writes past BUF_BYTES / WS_BYTES"""
    for _, (what, a) in cases().items():
        if what in ROWS_EXPORTS:
            assert 64 * max(a["lda"], a["ldr"], a["ldc"], 1) * 4 + 16 <= BUF_BYTES and max(a["N"], 1) * max(a["ldw"], a["lds"]) * 2 + 16 <= BUF_BYTES
        else:
            c = a["cfg"]
            nq, B = (c["Hq"] + 2 * c["Hkv"]) * c["D"], min(max(c["B"], 1), 64)
            assert max(nq, 2 * c["I"]) * max(c["E"], c["I"], c["Hq"] * c["D"]) * 2 + 16 <= BUF_BYTES      # the largest weight, as elements
            assert B * max(nq, c["E"], c["Hkv"] * 8 * c["D"], 128) * 4 + 16 <= BUF_BYTES                  # activations, cache, cos / sin
            assert 2 * B * (3 * c["E"] + c["Hq"] * c["D"] + 3 * c["I"]) + (1 << 20) <= WS_BYTES


def run_all():
    """{case id: status} on the GPU, one synchronisation behind them all"""
    import torch
    from u2tokenizer_amd import ops
    ops.device_check()
    bufs = {}

    def resolve(p):
        if p is None:
            return None
        _, name, off = p
        if name not in bufs:
            bufs[name] = torch.zeros(WS_BYTES if name == "ws" else BUF_BYTES, dtype=torch.uint8, device="cuda")
        return bufs[name].data_ptr() + off

    largest_call_fits()
    out = {}
    with ops.on_device(torch.zeros(1, dtype=torch.bfloat16, device="cuda")) as (lib, stream):   # (the bf16 build)
        for cid, (what, a) in cases().items():
            if what in ROWS_EXPORTS:
                out[cid] = int(getattr(lib, ROWS_EXPORTS[what])(*rows_argv(what, a, resolve, stream)))
            else:
                out[cid] = int(decode_call(lib, what, a, resolve, stream))
        torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", action="store_true", help="run every case on the GPU and write the statuses")
    ap.add_argument("--commit", default="", help="the commit whose library is recorded (written into the file)")
    ap.add_argument("--out", default=str(FIXTURE))
    a = ap.parse_args()
    if not a.record:
        print(f"{len(case_ids())} cases; --record writes their statuses")
        return 0
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    status = run_all()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps({"recorded_at_commit": a.commit, "status": status}, indent=0, sort_keys=True) + "\n")
    print(f"wrote {len(status)} statuses to {a.out}: {sum(v == 0 for v in status.values())} accepted")
    return 0


if __name__ == "__main__":
    sys.exit(main())
