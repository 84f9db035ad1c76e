#!/usr/bin/env python
"""A/B of a continued prefill -- S new positions per sequence against a cache of T0 -- on an FP8 (e4m3) KV cache, three arms
interleaved in one process per batch size, on one GPU, synthetic weights and N(0, 1) caches:

  a   today's behaviour: `enable_fused_prefill(model, kv8=True, continued=True)` -- route() refuses the filled `Kv8Layer` for
      "extend", the layer call runs on the stock modules, `Kv8Layer.update` returns the whole cache dequantised;
  b   the new route: `kv8_continued=True` -- the new rows quantised in place, u2tok_attention_kv8_rows over the codes;
  c   context only: the 16-bit append-in-place cache on the existing band route (`continued=True`).

8 layers at the Qwen3-8B shape (the decoder stack without its head), B in {1, 16} x T0 in {1024, 8192} x S in {4, 16, 64, 256, 1024}.
Per arm: ms per call (device events around each call, host time included; a round is the mean of REPS calls, the figure the median
of the rounds) and the largest rise of torch.cuda.max_memory_allocated over a call; a_over_b and c_over_b are medians of the rounds' ratios, their spread the largest
deviation of a round's ratio from that median.  The cache is cropped back to T0 after every call (outside the clock).

Verdict: KV8_EXTEND_MAX_ROWS = the largest measured S up to which, at every measured (B, T0), b is faster than a by more than the
recorded spread (a_over_b - spread > 1); None when that holds for every measured S.

    python tools/kv8_extend_ab.py [--layers 8] [--rounds 3] [--out profiles/kv8_extend_ab.json]

The parent process never opens the GPU: each batch size is a child process of its own under its own time limit, started only if the
one before it ended clean; nothing is tried twice.  Quality on trained weights is NOT measured here (no checkpoint):
tests/test_gpu_kv8_rows.py holds the route to the project's gate against the stock layers on the same quantised cache."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from decode_kv8_ab import _fill, _run  # noqa: E402
from decode_w4_ab import SHAPES, _box, _model, _ratios, _result  # noqa: E402

SHAPE = "qwen3-8b"
BATCHES, T0S, SS = (1, 16), (1024, 8192), (4, 16, 64, 256, 1024)
REPS = 5     # calls per arm and round: a single call of a few ms measures the host's scheduler as much as the layers
ARMS = {"a": dict(kv8=True, continued=True), "b": dict(kv8_continued=True), "c": dict(continued=True)}


def child(a):
    import torch
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    prefill.KV8_EXTEND_MAX_ROWS = None                   # (every S is measured, whatever the committed verdict)
    dev = torch.device("cuda", 0)
    s = SHAPES[SHAPE]
    m = _model(SHAPE, a.layers, dev, torch.bfloat16)     # one set of weights; the arm's switches are set before its call
    B, rows = a.batch, []
    for T0 in T0S:
        g = torch.Generator(device=dev).manual_seed(B + T0)
        k, v = (torch.randn(B, s["Hkv"], T0, s["D"], device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
        caches = {arm: DynamicCache() for arm in ARMS}
        for arm, cache in caches.items():
            _fill(m, cache, B, T0, arm != "c", k, v)
        del k, v
        for S in SS:
            x = torch.randn(B, S, s["E"], device=dev, generator=g).to(torch.bfloat16)

            def run(arm):
                prefill.enable_fused_prefill(m, **ARMS[arm])
                cache = caches[arm]
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                m.model(inputs_embeds=x, past_key_values=cache, use_cache=True)
                t1.record()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - base
                assert cache.get_seq_length() == T0 + S
                cache.crop(T0)
                return t0.elapsed_time(t1), peak

            n8, nx = prefill.kv8_extend_stats["extend"], prefill.extend_stats["extend"]
            t = {arm: [] for arm in ARMS}
            peak = {}
            for rnd in range(a.rounds + 1):     # (round 0: warm-up, one call per arm)
                for arm in ARMS:
                    got = [run(arm) for _ in range(REPS if rnd else 1)]
                    if rnd:
                        t[arm].append(sum(ms for ms, _ in got) / REPS)
                        peak[arm] = max([peak.get(arm, 0)] + [pk for _, pk in got])
            calls = (a.rounds * REPS + 1) * a.layers    # a ran stock, b on the codes, c on the band kernel
            assert prefill.kv8_extend_stats["extend"] - n8 == calls and prefill.extend_stats["extend"] - nx == 2 * calls
            assert all(type(l) is prefill.Kv8Layer for arm in "ab" for l in caches[arm].layers)
            row = {"B": B, "T0": T0, "S": S, "layers": a.layers, "rounds": a.rounds, "reps": REPS}
            for arm in ARMS:
                row[arm + "_ms"] = round(statistics.median(t[arm]), 3)
                row[arm + "_peak_MB"] = round(peak[arm] / 1e6, 1)
            row["a_over_b"], row["a_over_b_spread"] = _ratios(t["a"], t["b"])
            row["c_over_b"], row["c_over_b_spread"] = _ratios(t["c"], t["b"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x
        del caches
        torch.cuda.empty_cache()
    prefill.disable_fused_prefill(m)
    print("RESULT " + json.dumps({"box": _box(), "rows": rows}), flush=True)


def verdict(rows):
    """-> KV8_EXTEND_MAX_ROWS from the rows: the largest measured S up to which b beats a beyond the spread at every (B, T0)"""
    best = 0
    for S in sorted({r["S"] for r in rows}):
        if not all(r["a_over_b"] - r["a_over_b_spread"] > 1.0 for r in rows if r["S"] == S):
            return best or 1
        best = S
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = [sys.executable, str(Path(__file__).resolve()), "--layers", str(a.layers), "--rounds", str(a.rounds), "--child"]
    res = {"what": "continued prefill of S positions on T0 cached ones, 8 layers of the Qwen3-8B shape without the head: (a) kv8=True, "
                   "continued=True (the stock layers on the dequantised e4m3 cache), (b) kv8_continued=True (u2tok_attention_kv8_rows on "
                   "the codes), (c) continued=True on the 16-bit append-in-place cache; interleaved in one process per batch size; "
                   "synthetic weights and N(0, 1) caches; ms per call (a round: the mean of 5 calls), medians over the rounds, spread = largest deviation of a round's "
                   "ratio from the median ratio; peak_MB = rise of torch.cuda.max_memory_allocated over the call; quality on trained "
                   "weights: not measured (no checkpoint)", "layers": a.layers, "rows": []}
    for B in BATCHES:
        r = _result(_run(me + ["--batch", str(B)], 420))
        res["box"] = r["box"]
        res["rows"] += r["rows"]
    res["KV8_EXTEND_MAX_ROWS"] = verdict(res["rows"])
    print(json.dumps({"KV8_EXTEND_MAX_ROWS": res["KV8_EXTEND_MAX_ROWS"]}), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
