#!/usr/bin/env python
"""A/B of the per-layer fused decode step on the 16-bit append-in-place KV cache (a: the parent route) and on the FP8 (e4m3) cache
of `enable_fused_prefill(model, kv8=True)` (b), interleaved pairs in one process per measurement, on one GPU, synthetic weights:

  steps   per shape, weight form (bf16, e2m1), batch size and cache length T, two copies of the same decoder (a and b, each patched
          once) take turns: the same 16 greedy decode steps against a cache of T positions of N(0, 1) keys and values (written
          through the layers' own `update`, so b's cache is what its quantiser makes of a's); per-step ms (device events around
          the steps, host time of the calls included, as `generate` pays it), medians over the rounds, the spread of the ratio
          (largest deviation of a round's ratio from the median ratio), and the caches' bytes.  Shapes: 8 layers of Qwen3-8B at
          B = 1, 16, 64 x T = 1 024, 2 048, 8 192 and one Phi-3-mini-shaped run (B = 16, T = 2 048).
  attn    the two attention entries alone (u2tok_decode_attention / u2tok_decode_attention_kv8, merge included) at the same (B, T),
          over a ring of caches larger than the last-level cache where one fits 64 times (cold keys, as a step of many layers
          sees them): us per call (device events around a pass over the ring, median over passes) and the achieved TB/s on the
          bytes of K and V (b: codes and scales) against the 8 TB/s roof.

    python tools/decode_kv8_ab.py [--layers 8] [--rounds 5] [--out profiles/decode_kv8_ab.json]

The parent process never opens the GPU: every GPU step is a child process of its own under its own time limit, started only if the
one before it ended clean; nothing is tried twice.  Quality on trained weights is NOT measured here (no checkpoint):
tests/test_gpu_kv8.py holds the step to the project's gate against the stock layers on the same quantised cache."""
import argparse
import json
import math
import statistics
import subprocess
import sys
import threading
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from decode_w4_ab import SHAPES, _box, _model, _ratios, _result  # noqa: E402

STEPS = 16
GRID = {"qwen3-8b": [(B, T) for B in (1, 16, 64) for T in (1024, 2048, 8192)], "phi3-mini": [(16, 2048)]}
FORMS = {"bf16": {}, "e2m1": dict(fp4_decode=True)}
LLC_BYTES = 256 << 20
ROOF_TB_S = 8.0


def _fill(m, cache, B, T, kv8, k, v):
    """T cached positions in every layer, through the layer's own `update`"""
    from u2tokenizer_amd import prefill
    cache.layers.clear()
    for _ in range(m.config.num_hidden_layers):
        lay = prefill.Kv8Layer() if kv8 else prefill._append_layer_class()()
        lay.update(k, v)
        cache.layers.append(lay)


def child_steps(a):
    import torch
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    s = SHAPES[a.shape]
    res = []
    for form, flags in FORMS.items():
        ma, mb = (_model(a.shape, a.layers, dev, torch.bfloat16) for _ in range(2))
        prefill.enable_fused_prefill(ma, wide_decode=True, **flags)
        prefill.enable_fused_prefill(mb, wide_decode=True, kv8=True, **flags)
        for B, T in GRID[a.shape]:
            g = torch.Generator(device=dev).manual_seed(B + T)
            k, v = (torch.randn(B, s["Hkv"], T, s["D"], device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
            ca, cb = DynamicCache(), DynamicCache()
            _fill(ma, ca, B, T, False, k, v)
            _fill(mb, cb, B, T, True, k, v)
            del k, v
            tok0 = torch.randint(3, 1024, (B, 1), device=dev, generator=g)

            def run(m, cache):
                tok = m(input_ids=tok0, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)   # (outside the clock)
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(STEPS):
                    tok = m(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
                t1.record()
                torch.cuda.synchronize()
                cache.crop(T)
                return t0.elapsed_time(t1) / STEPS

            n0, n8 = prefill.stats["decode"], prefill.kv8_stats["decode"]
            run(ma, ca), run(mb, cb)     # warm-up (quantised weight copies, code objects)
            t = {"a": [], "b": []}
            for _ in range(a.rounds):
                t["a"].append(run(ma, ca))
                t["b"].append(run(mb, cb))
            calls = (a.rounds + 1) * (STEPS + 1) * a.layers
            assert prefill.kv8_stats["decode"] - n8 == calls and prefill.stats["decode"] - n0 == 2 * calls
            assert all(type(l) is prefill.Kv8Layer for l in cb.layers) and all(type(l).__name__ == "AppendLayer" for l in ca.layers)
            rows = B * s["Hkv"] * T * a.layers
            row = {"shape": a.shape, "weights": form, "B": B, "T": T, "layers": a.layers, "steps": STEPS, "rounds": a.rounds,
                   "a_ms_per_step": round(statistics.median(t["a"]), 4), "b_ms_per_step": round(statistics.median(t["b"]), 4),
                   "a_cache_MB": round(rows * 2 * s["D"] * 2 / 1e6, 1), "b_cache_MB": round(rows * 2 * (s["D"] + 4) / 1e6, 1)}
            row["a_over_b"], row["a_over_b_spread"] = _ratios(t["a"], t["b"])
            res.append(row)
            print(json.dumps(row), flush=True)
            del ca, cb
            torch.cuda.empty_cache()
        prefill.disable_fused_prefill(ma), prefill.disable_fused_prefill(mb)
        del ma, mb
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"box": _box(), "rows": res}), flush=True)


def child_attn(a):
    import torch
    from u2tokenizer_amd import ops
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    rows = []
    for shape, grid in GRID.items():
        s = SHAPES[shape]
        Hq, Hkv, D = s["Hq"], s["Hkv"], s["D"]
        for B, T in grid:
            g = torch.Generator(device=dev).manual_seed(B + T)
            bytes_a, bytes_b = B * Hkv * T * D * 2 * 2, B * Hkv * T * (D + 4) * 2
            n = max(1, min(64, math.ceil(2 * LLC_BYTES / bytes_a)))
            q = torch.randn(B, Hq * D, device=dev, generator=g).to(torch.bfloat16)
            ring_a, ring_b = [], []
            for _ in range(n):
                k, v = (torch.randn(B, Hkv, T, D, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
                bufs = (torch.empty(B, Hkv, T, D, dtype=torch.uint8, device=dev), torch.empty(B, Hkv, T, D, dtype=torch.uint8, device=dev),
                        torch.empty(B, Hkv, T, device=dev), torch.empty(B, Hkv, T, device=dev))
                ops.kv_quantize_rows(k, v, *bufs, 0)
                ring_a.append((k, v))
                ring_b.append(bufs)
            scale = D ** -0.5
            fa = lambda: [ops.decode_attention(q, k, v, Hq, Hkv, scale) for k, v in ring_a]               # noqa: E731
            fb = lambda: [ops.decode_attention_kv8(q, *bufs, T, Hq, scale) for bufs in ring_b]           # noqa: E731
            t = {"a": [], "b": []}
            for rnd in range(a.rounds + 1):     # (round 0: warm-up)
                for name, fn in (("a", fa), ("b", fb)):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0.record()
                    fn()
                    t1.record()
                    torch.cuda.synchronize()
                    if rnd:
                        t[name].append(1e3 * t0.elapsed_time(t1) / n)
            ua, ub = statistics.median(t["a"]), statistics.median(t["b"])
            row = {"shape": shape, "B": B, "T": T, "ring": n, "cold": 2 * n * bytes_b > LLC_BYTES, "a_us": round(ua, 2), "b_us": round(ub, 2),
                   "a_TB_s": round(bytes_a / ua / 1e6, 3), "b_TB_s": round(bytes_b / ub / 1e6, 3),
                   "a_of_roof": round(bytes_a / ua / 1e6 / ROOF_TB_S, 3), "b_of_roof": round(bytes_b / ub / 1e6 / ROOF_TB_S, 3)}
            row["a_over_b"], row["a_over_b_spread"] = _ratios(t["a"], t["b"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ring_a, ring_b
            torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"box": _box(), "rows": rows}), flush=True)


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    late = threading.Timer(limit, p.kill)
    late.start()
    lines = []
    for ln in p.stdout:          # (a child's rows are shown as they come: the largest shapes take minutes)
        lines.append(ln)
        if not ln.startswith("RESULT "):
            print("  " + ln, end="", flush=True)
    rc = p.wait()
    expired = not late.is_alive()
    late.cancel()
    if rc != 0:
        why = f"timed out after {limit} s" if expired else f"exit status {rc}"
        raise SystemExit(f"decode_kv8_ab: {why}: {' '.join(cmd)}\n{''.join(lines)[-3000:]} -- stopping here")
    return "".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["steps", "attn"])
    ap.add_argument("--shape", default="qwen3-8b", choices=list(SHAPES))
    a = ap.parse_args()
    if a.child:
        return {"steps": child_steps, "attn": child_attn}[a.child](a)
    me = [sys.executable, str(Path(__file__).resolve()), "--layers", str(a.layers), "--rounds", str(a.rounds)]
    res = {"what": "per-layer fused decode step on the 16-bit append-in-place KV cache (a) and on the e4m3 cache of kv8 (b), interleaved "
                   "in one process; synthetic weights and N(0, 1) caches; 16 greedy steps per run, medians over the rounds, spread = "
                   "largest deviation of a round's ratio from the median ratio; attn: the attention entries alone over a ring of "
                   "caches; quality on trained weights: not measured (no checkpoint)", "layers": a.layers, "steps": []}
    res["attn"] = _result(_run(me + ["--child", "attn"], 300))["rows"]
    print(json.dumps(res["attn"]), flush=True)
    for shape in SHAPES:
        r = _result(_run(me + ["--child", "steps", "--shape", shape], 420))
        res["box"] = r["box"]
        res["steps"] += r["rows"]
        print(json.dumps(r["rows"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
