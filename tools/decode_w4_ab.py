#!/usr/bin/env python
"""A/B of the decode step's three weight forms -- 16-bit, e4m3 (fp8_decode) and MXFP4 / e2m1 (fp4_decode) -- in one process per
measurement, interleaved, on one GPU, with synthetic weights:

  steps     per shape and batch size, three copies of the same decoder (one per form, each patched once, so nothing is
            re-quantised between runs) take turns: the same 64 greedy decode steps after a fused prefill; per-step ms (device
            events around the 64 steps, host time of the calls included, as `generate` pays it), medians over the rounds, and the
            spread of each ratio (largest deviation of a round's ratio from the median ratio).  Shapes: the Qwen3-8B layer at
            B = 1, 16, 64 (64: wide_decode) and a Phi-3-mini layer at B = 1.  The decoder has --layers layers: its weights in
            any form are larger than the 256 MB of last-level cache, so every step streams them from HBM as the 36-layer model's
            step does; per-step times scale with the layer count, the ratios do not.
  products  the four products of the Qwen3-8B layer (q|k|v, o, gate|up pair, down) called directly, each form at M = 1, 16, 64,
            over a ring of weight copies larger than the cache (cold weights, as the step sees them), through the C entry points
            with every argument prepared (a few us of host time per call, so that the device is the clock): us per product
            (device events around a pass over the ring, median over passes) and the achieved TB/s on its weight bytes.
  trace     a child under `rocprofv3 --kernel-trace --stats` (Qwen3-8B layer, B = 1, the 64 steps once per form): total time of the
            few-rows product kernels of each form per step and the weight bytes they streamed -> kernel ms per step and achieved
            TB/s, to set against the step times above (what of a step is not these kernels is the single-row kernels and the host).

    python tools/decode_w4_ab.py [--layers 8] [--rounds 5] [--out profiles/decode_w4_ab.json]

The parent process never opens the GPU: every GPU step is a child process of its own under its own time limit, started only if
the one before it ended clean; nothing is tried twice.  No trained checkpoint is involved: quality on trained weights is NOT
measured here (tests/test_gpu_w4.py holds the step to the project's gate on weights the quantiser keeps exactly)."""
import argparse
import csv
import json
import platform
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS = 64
SHAPES = {   # hidden, intermediate, query heads, kv heads, head dim
    "qwen3-8b": dict(kind="qwen3", E=4096, I=12288, Hq=32, Hkv=8, D=128, batches=(1, 16, 64)),
    "phi3-mini": dict(kind="phi3", E=3072, I=8192, Hq=32, Hkv=32, D=96, batches=(1,)),
}
FORMS = ("bf16", "e4m3", "e2m1")
FLAGS = {"bf16": {}, "e4m3": dict(fp8_decode=True), "e2m1": dict(fp4_decode=True)}
CACHE_BYTES = 256 << 20


def _model(shape, layers, dev, dtype, seed=0):
    import torch
    s = SHAPES[shape]
    common = dict(vocab_size=1024, hidden_size=s["E"], intermediate_size=s["I"], num_hidden_layers=layers,
                  num_attention_heads=s["Hq"], num_key_value_heads=s["Hkv"], max_position_embeddings=4096,
                  tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    if s["kind"] == "qwen3":
        from transformers import Qwen3Config, Qwen3ForCausalLM
        cfg, cls = Qwen3Config(head_dim=s["D"], **common), Qwen3ForCausalLM
    else:
        from transformers import Phi3Config, Phi3ForCausalLM
        cfg, cls = Phi3Config(**common), Phi3ForCausalLM
    torch.manual_seed(seed)
    with torch.device(dev):
        m = cls(cfg)
    return m.to(dtype).eval()


def _box():
    import torch
    return {"host": platform.node(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__}


def _ratios(num, den):
    r = [x / y for x, y in zip(num, den)]
    med = statistics.median(r)
    return round(med, 3), round(max(abs(x - med) for x in r), 3)


def child_steps(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    s = SHAPES[a.shape]
    models = {}
    for f in FORMS:     # the same weights three times; each copy keeps its form's switches for good
        models[f] = _model(a.shape, a.layers, dev, torch.bfloat16)
        prefill.enable_fused_prefill(models[f], wide_decode=True, **FLAGS[f])
    res = []
    for B in s["batches"]:
        ids = torch.randint(3, 1024, (B, 128), device=dev, generator=torch.Generator(device=dev).manual_seed(B))

        def run(m):
            out = m(input_ids=ids, use_cache=True)
            cache, tok = out.past_key_values, out.logits[:, -1].argmax(-1, keepdim=True)
            tok = m(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)   # (outside the clock)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(STEPS):
                tok = m(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / STEPS

        for f in FORMS:     # warm-up (builds the quantised copies, loads the code objects)
            run(models[f])
        n8, n4 = prefill.w8_stats["decode"], prefill.w4_stats["decode"]
        t = {f: [] for f in FORMS}
        for _ in range(a.rounds):
            for f in FORMS:
                t[f].append(run(models[f]))
        calls = a.rounds * (STEPS + 1) * a.layers
        assert prefill.w8_stats["decode"] - n8 == calls and prefill.w4_stats["decode"] - n4 == calls
        row = {"shape": a.shape, "B": B, "layers": a.layers, "steps": STEPS, "rounds": a.rounds}
        for f in FORMS:
            row[f + "_ms_per_step"] = round(statistics.median(t[f]), 4)
        row["bf16_over_e4m3"], row["bf16_over_e4m3_spread"] = _ratios(t["bf16"], t["e4m3"])
        row["bf16_over_e2m1"], row["bf16_over_e2m1_spread"] = _ratios(t["bf16"], t["e2m1"])
        row["e4m3_over_e2m1"], row["e4m3_over_e2m1_spread"] = _ratios(t["e4m3"], t["e2m1"])
        res.append(row)
    for m in models.values():
        prefill.disable_fused_prefill(m)
    print("RESULT " + json.dumps({"box": _box(), "rows": res}), flush=True)


def child_products(a):
    import torch
    from u2tokenizer_amd import _lib, ops
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    h = _lib.load_library("bf16")
    s = SHAPES["qwen3-8b"]
    E, inter, nq = s["E"], s["I"], (s["Hq"] + 2 * s["Hkv"]) * s["D"]
    products = (("qkv", nq, E, False), ("o", E, s["Hq"] * s["D"], False), ("gate|up pair", 2 * inter, E, True), ("down", E, inter, False))
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for name, N, K, pair in products:
        w = (torch.randn(N, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16)
        forms = {"bf16": ((w,), 2.0 * N * K), "e4m3": (ops.quantize_rows_fp8(w), 1.0 * N * K + 4.0 * N),
                 "e2m1": (ops.quantize_blocks_fp4(w), 0.5 * N * K + N * K / 32)}
        flags = ops.GEMM_SWIGLU if pair else 0
        cols = N // 2 if pair else N
        rings = {}
        for f, (ws, nbytes) in forms.items():     # a ring of copies larger than twice the cache: every call reads cold weights
            n = int(2 * CACHE_BYTES // nbytes) + 2
            rings[f] = [tuple(t.clone() for t in ws) for _ in range(n)]
        for M in (1, 16, 64):
            x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            out = torch.empty(M, cols, dtype=torch.bfloat16, device=dev)
            xp, op, st = x.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream
            # A, W, [scales,] C, bias, R, M, N, K, lda, ldw, [lds,] ldc, ldr, flags, stream  (include/u2tok.h)
            calls = {"bf16": [(h.u2tok_gemm_rows, (xp, w.data_ptr(), op, None, None, M, N, K, K, K, cols, 0, flags, st)) for (w,) in rings["bf16"]],
                     "e4m3": [(h.u2tok_gemm_rows_w8_wide, (xp, w.data_ptr(), sc.data_ptr(), op, None, None, M, N, K, K, K, cols, 0, flags, st))
                              for w, sc in rings["e4m3"]],
                     "e2m1": [(h.u2tok_gemm_rows_w4, (xp, w.data_ptr(), sc.data_ptr(), op, None, None, M, N, K, K, K // 2, K // 32, cols, 0, flags, st))
                              for w, sc in rings["e2m1"]]}
            for f in FORMS:     # every form once through the checked wrapper's eyes: the raw call must succeed
                fn, args = calls[f][0]
                assert fn(*args) == 0, f
            t = {f: [] for f in FORMS}
            for rnd in range(a.rounds + 1):       # (round 0: warm-up)
                for f in FORMS:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0.record()
                    for fn, args in calls[f]:
                        fn(*args)
                    t1.record()
                    torch.cuda.synchronize()
                    if rnd:
                        t[f].append(1e3 * t0.elapsed_time(t1) / len(rings[f]))
            row = {"product": name, "N": N, "K": K, "M": M}
            for f in FORMS:
                us = statistics.median(t[f])
                row[f + "_us"], row[f + "_TB_s"], row[f + "_ring"] = round(us, 2), round(forms[f][1] / us / 1e6, 3), len(rings[f])
            row["bf16_over_e2m1"], _ = _ratios(t["bf16"], t["e2m1"])
            row["e4m3_over_e2m1"], _ = _ratios(t["e4m3"], t["e2m1"])
            rows.append(row)
        del rings, forms, w
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"box": _box(), "rows": rows}), flush=True)


def child_trace(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    ids = torch.randint(3, 1024, (1, 128), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for f in FORMS:
        m = _model("qwen3-8b", a.layers, dev, torch.bfloat16)
        prefill.enable_fused_prefill(m, **FLAGS[f])
        out = m(input_ids=ids, use_cache=True)
        cache, tok = out.past_key_values, out.logits[:, -1].argmax(-1, keepdim=True)
        for _ in range(STEPS):
            tok = m(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
        torch.cuda.synchronize()
        prefill.disable_fused_prefill(m)
        del m, cache, out


def _trace_table(d, layers):
    """achieved TB/s of the four products per form from rocprofv3's kernel statistics (weights streamed once per step and layer)"""
    files = sorted(Path(d).rglob("*kernel_stats.csv"))
    if not files:
        return {"error": "no kernel_stats.csv written"}
    s = SHAPES["qwen3-8b"]
    per_layer = (s["Hq"] + 2 * s["Hkv"]) * s["D"] * s["E"] + s["E"] * s["Hq"] * s["D"] + 3 * s["I"] * s["E"]   # weights of the four products
    rows = list(csv.DictReader(files[0].open()))
    out = {}
    # gemm_rows16_kernel<NW, NB, PAIR, (u2::WForm)F> (csrc/gemm_rows.hip): the weight form is the last template argument
    for i, (f, nbytes) in enumerate((("bf16", 2.0), ("e4m3", 1.0), ("e2m1", 0.5 + 1.0 / 32))):
        sel = [r for r in rows if re.search(r"gemm_rows16_kernel<[^>]*WForm\)%d>" % i, r["Name"])]
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        total = per_layer * nbytes * layers * STEPS
        out[f] = {"kernel_calls": sum(int(r["Calls"]) for r in sel), "expected_calls": 4 * layers * STEPS,
                  "kernel_ms_per_step": round(ns / STEPS / 1e6, 4), "weight_GB_per_step": round(total / STEPS / 1e9, 4),
                  "achieved_TB_s": round(total / ns / 1e3, 3) if ns else None}
    return out


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"decode_w4_ab: timed out after {limit} s: {' '.join(cmd)} -- stopping here")
    if r.returncode != 0:
        raise SystemExit(f"decode_w4_ab: exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}{r.stderr[-2000:]} -- stopping here")
    return r.stdout


def _result(stdout):
    return json.loads(next(ln for ln in stdout.splitlines() if ln.startswith("RESULT "))[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["steps", "products", "trace"])
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--shape", default="qwen3-8b", choices=list(SHAPES))
    a = ap.parse_args()
    if a.child:
        return {"steps": child_steps, "products": child_products, "trace": child_trace}[a.child](a)
    me = [sys.executable, str(Path(__file__).resolve()), "--layers", str(a.layers), "--rounds", str(a.rounds)]
    res = {"what": "decode step on 16-bit, e4m3 and e2m1 (MXFP4) weights of the same tree, interleaved in one process; synthetic "
                   "weights; 64 greedy steps per run, medians over the rounds, spread = largest deviation of a round's ratio from "
                   "the median ratio; products: cold weights from a ring of copies larger than the cache; quality on trained "
                   "weights: not measured (no checkpoint)", "layers": a.layers, "steps": []}
    for shape in SHAPES:
        r = _result(_run(me + ["--child", "steps", "--shape", shape], 400))
        res["box"] = r["box"]
        res["steps"] += r["rows"]
        print(json.dumps(r["rows"]), flush=True)
    res["products"] = _result(_run(me + ["--child", "products"], 400))["rows"]
    print(json.dumps(res["products"]), flush=True)
    prof = shutil.which("rocprofv3")
    if a.no_trace or prof is None:
        res["trace"] = {"skipped": "rocprofv3 not found" if prof is None else "--no-trace"}
    else:
        d = tempfile.mkdtemp(prefix="decode_w4_trace_")
        _run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace"], 400)
        res["trace"] = _trace_table(d, a.layers)
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res["trace"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
