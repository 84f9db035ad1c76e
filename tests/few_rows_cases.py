"""The inputs and the case list of tests/test_gpu_few_rows_bits.py: the few-rows (weight-streaming) product's OUTPUT BITS, pinned as
SHA-256 digests in tests/golden/few_rows_bits.json (16-bit and e4m3 weights, the plan's route) and
tests/golden/few_rows_bits_e2m1.json (e2m1 weights).  Importable without a GPU (the host half of the test checks the inputs).

Inputs are an explicit integer hash of (seed, row, column), computed in int64 with every intermediate below 2^63 -- no random
generator whose stream could change:
  * activations and 16-bit weights: sign x (128 + m) x 2^e with m in 0 .. 127 (a full 8-bit significand: exact in bf16 and in fp16)
    and e over 6 binades, so that fp32 partial sums of their (exact, 16-bit) products round;
  * e4m3 weights: the 254 finite codes (0x7F / 0xFF, the NaNs, left out);
  * scales: (2^23 + m) x 2^-32 with m in 0 .. 2^23 - 1: positive fp32 with full mantissas;
  * e2m1 weights: ops.quantize_blocks_fp4 of 16-bit weights whose blocks of 32 are moved over 10 binades, block by block: every
    code the quantiser emits (all but -0) and 10 block scales or more per shape.

`python tests/few_rows_cases.py --record --commit HASH [--form e2m1] [--out FILE]` runs the cases of one fixture on the GPU and
writes it; the test itself only ever reads them."""
import argparse
import functools
import hashlib
import json
import sys
from pathlib import Path

import torch

P31 = 2147483647   # 2^31 - 1
FIXTURE = Path(__file__).resolve().parent / "golden" / "few_rows_bits.json"
FIXTURE_E2M1 = FIXTURE.with_name("few_rows_bits_e2m1.json")   # recorded later, at another commit: a file of its own
FIXTURES = (FIXTURE, FIXTURE_E2M1)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
FORMS = ("elem", "e4m3", "e2m1")
STEP_K = {"elem": 32, "e4m3": 64, "e2m1": 128}   # the k of one step (e4m3: double step, e2m1: quad step) -- csrc/rows.h
ROWS = (1, 13, 16, 17, 33, 64)
# (N, K): what it exercises (steps = K / 32, e4m3: double steps = K / 64; NW = slices(steps) waves of `per` steps each)
SHAPES = (
    (40, 64),      # a partial column block; 2 steps / 1 double step: most waves have an empty slice
    (16, 192),     # a remainder block only, `per` not dividing the steps
    (40, 1024),    # NW = 8 in both weight forms (32 steps / 16 double steps)
    (1040, 4096),  # NW = 16
    (40, 9216),    # per = 18 steps / 9 double steps: whole blocks of steps in flight plus a remainder in the same slice
)
# e2m1: quad steps = K / 128 -- every NW, the one-step product, a ragged number of steps
SHAPES_E2M1 = (
    (40, 128),     # one quad step: three of the four waves have an empty slice
    (16, 384),     # 3 quad steps on 4 waves
    (40, 2048),    # NW = 8 (16 quad steps)
    (72, 8192),    # NW = 16 (64 quad steps)
)
EPILOGUES = ("plain", "bias_res", "f32")
PAIR_I = {64: 24, 192: 24, 1024: 24, 4096: 1024, 9216: 24,   # the pair form (SiLU(gate) * up): I per K; N = 2 I
          128: 24, 384: 24, 2048: 24, 8192: 40}


def _hash(seed, rows, cols):
    """(rows, cols) int64 in [0, 2^31 - 1): a quadratic map of a linear one, both modulo the prime 2^31 - 1"""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    h = ((r * 1000003 + c) * 7919 + seed * 104729 + 12345) % P31      # < 2^48 before the reduction
    h = (h * h + h * 48271 + seed) % P31                              # < 2^62 + 2^47
    return (h * 69621 + (h >> 7)) % P31


def values(seed, rows, cols, e0):
    """fp32 (rows, cols): sign x (128 + m) x 2^(e0 + e - 7), e in 0 .. 5 -- magnitudes in [2^e0, 2^(e0 + 6))"""
    h = _hash(seed, rows, cols)
    m, e, s = h % 128, (h >> 7) % 6, (h >> 10) % 2
    return (1 - 2 * s).float() * (128 + m).float() * torch.exp2((e + (e0 - 7)).float())


def codes(seed, rows, cols):
    """uint8 (rows, cols): finite e4m3 codes"""
    i = _hash(seed, rows, cols) % 254
    return (i + (i >= 127).long()).to(torch.uint8)     # 0 .. 126, 128 .. 254


def scales(seed, n):
    return ((_hash(seed, n, 1)[:, 0] % (1 << 23)) + (1 << 23)).float() * 2.0 ** -32


def shapes(form):
    return SHAPES_E2M1 if form == "e2m1" else SHAPES


def slices(K, w8=False, form=None):
    """(NW, per) of the kernels for weights in `form` (not named: e4m3 if w8, else the element type): NW waves, `per` steps (e4m3:
    double steps, e2m1: quad steps) each -- csrc/rows.h"""
    steps = K // STEP_K[form or ("e4m3" if w8 else "elem")]
    nw = 16 if steps >= 64 else 8 if steps >= 16 else 4
    return nw, -(-steps // nw)


@functools.lru_cache(maxsize=None)
def activations(K):
    return values(1000 + K, 64, K, -4)       # rows 0 .. M - 1 of it are the M-row case's


@functools.lru_cache(maxsize=None)
def weights(N, K):
    return values(2000 + N + K, N, K, -7)


@functools.lru_cache(maxsize=None)
def weights_e4m3(N, K):
    return codes(3000 + N + K, N, K), scales(4000 + N + K, N)


@functools.lru_cache(maxsize=None)
def weights_e2m1(N, K):
    """(codes uint8 (N, K / 2), block scales uint8 (N, K / 32)): the quantiser's output on `weights` with block j of row n moved up
    by 0 .. 9 binades"""
    from u2tokenizer_amd import ops
    up = torch.exp2((_hash(8000 + N + K, N, K // 32) % 10).float()).repeat_interleave(32, 1)
    return ops.quantize_blocks_fp4(weights(N, K) * up)


def epilogue_inputs(M, N):
    """bias (N), and the residual's (M, N + 24) storage: the case reads its columns 8 .. 8 + N"""
    return values(5000 + N, 1, N, -3)[0], values(6000 + N, 64, N + 24, -3)[:M]


def product_cases(form="elem"):
    """(id suffix, M, N, K, epilogue) for one build and weight form; "pair": N = 2 I"""
    out = []
    for M in ROWS:
        for N, K in shapes(form):
            for epi in EPILOGUES:
                out.append((f"{epi}-M{M}-N{N}-K{K}", M, N, K, epi))
            out.append((f"pair-M{M}-N{2 * PAIR_I[K]}-K{K}", M, 2 * PAIR_I[K], K, "pair"))
    return out


# what goes through the plan and the big-tile launch (element-type weights): (id suffix, M, N, K, ops.gemm keywords, options, the
# last rows that are digested)
PLAN_CASES = (
    ("plan-M13-N40-K4096-alpha-bias-gelu", 13, 40, 4096, dict(alpha=0.5, bias=True, gelu=True), {}, 13),
    # the last 8 rows of tests/test_gpu_ops.py GEMM_WRITE_CASES "heuristic_big_rows16_tail": a few-rows step behind the tiles ...
    ("tail-M2056-N1536-K768-grid16", 2056, 1536, 768, {}, {"gemm_big_grid": 16}, 8),
    # ... and of two products whose last rows are computed INSIDE the big-tile launch (both kernels that carry the tail)
    ("tail-M2056-N768-K768-bias-res-grid16", 2056, 768, 768, dict(bias=True, residual=True), {"gemm_big_grid": 16}, 8),
    ("tail-M1032-N384-K768-grid4", 1032, 384, 768, {}, {"gemm_big_grid": 4}, 8),
)
OPTION_DEFAULTS = {"gemm_big_grid": 256}


def case_ids(fixture=FIXTURE):
    """The cases of one fixture file"""
    if fixture == FIXTURE_E2M1:
        return [f"{d}-e2m1-{s[0]}" for d in DTYPES for s in product_cases("e2m1")]
    ids = [f"{d}-{f}-{s[0]}" for d in DTYPES for f in ("elem", "e4m3") for s in product_cases(f)]
    return ids + [f"{d}-elem-{c[0]}" for d in DTYPES for c in PLAN_CASES]


def _sha(t):
    t = t.contiguous().cpu()
    bits = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    return hashlib.sha256(bits.numpy().tobytes()).hexdigest()


def product_digests(ops, elem, form):
    """{case id: SHA-256 of the output bytes} of every product case of one build and weight form, on the GPU"""
    dt, w8, w4, dev = DTYPES[elem], form == "e4m3", form == "e2m1", "cuda"
    out = {}
    dev_w = functools.lru_cache(maxsize=None)(
        lambda N, K: tuple(t.to(dev) for t in ((weights_e4m3(N, K)[0].view(torch.float8_e4m3fn), weights_e4m3(N, K)[1]) if w8
                                               else weights_e2m1(N, K) if w4 else (weights(N, K).to(dt),))))
    for suffix, M, N, K, epi in product_cases(form):
        x = activations(K)[:M].to(dt).to(dev)
        fn = ops.gemm_rows_w8 if w8 else ops.gemm_rows_w4 if w4 else ops.gemm_rows
        if epi == "pair":
            got = fn(x, *dev_w(N, K), swiglu=True)
        elif epi == "bias_res":
            bias, R = epilogue_inputs(M, N)
            buf = torch.zeros((M, N + 16), dtype=dt, device=dev)
            got = fn(x, *dev_w(N, K), bias=bias.to(dt).to(dev), residual=R.to(dt).to(dev)[:, 8:8 + N], out=buf[:, 8:8 + N])
        else:
            got = fn(x, *dev_w(N, K), out_f32=epi == "f32")
        out[f"{elem}-{form}-{suffix}"] = _sha(got)
    return out


def plan_digests(ops, elem):
    dt, dev = DTYPES[elem], "cuda"
    out = {}
    for suffix, M, N, K, kw, options, last in PLAN_CASES:
        x = values(7000 + M + K, M, K, -4).to(dt).to(dev)
        w = weights(N, K).to(dt).to(dev)
        bias, R = values(5000 + N, 1, N, -3)[0], values(6000 + N + M, M, N, -3)
        kw = dict(kw)
        if kw.pop("bias", False):
            kw["bias"] = bias.to(dt).to(dev)
        if kw.pop("residual", False):
            kw["residual"] = R.to(dt).to(dev)
        try:
            for k, v in options.items():
                ops.set_option(k, v)
            got = ops.gemm(x, w, **kw)
            torch.cuda.synchronize()
        finally:
            for k in options:
                ops.set_option(k, OPTION_DEFAULTS[k])
        out[f"{elem}-elem-{suffix}"] = _sha(got.reshape(M, N)[M - last:])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", action="store_true", help="run every case on the GPU and write the digests")
    ap.add_argument("--commit", default="", help="the commit whose kernels are recorded (written into the file)")
    ap.add_argument("--form", default="", choices=("", "e2m1"), help="e2m1: the cases of few_rows_bits_e2m1.json instead")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fixture = FIXTURE_E2M1 if a.form == "e2m1" else FIXTURE
    a.out = a.out or str(fixture)
    if not a.record:
        print(f"{len(case_ids(fixture))} cases; --record writes their digests")
        return 0
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    from u2tokenizer_amd import ops
    ops.device_check()
    torch.set_grad_enabled(False)
    digests = {}
    for elem in DTYPES:
        if a.form == "e2m1":
            digests.update(product_digests(ops, elem, "e2m1"))
            continue
        for form in ("elem", "e4m3"):
            digests.update(product_digests(ops, elem, form))
        digests.update(plan_digests(ops, elem))
    assert sorted(digests) == sorted(case_ids(fixture))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps({"recorded_at_commit": a.commit, "digests": digests}, indent=0, sort_keys=True) + "\n")
    print(f"wrote {len(digests)} digests to {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
