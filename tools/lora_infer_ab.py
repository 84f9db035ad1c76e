#!/usr/bin/env python
"""A/B of the unmerged-adapter branch on the no-grad routes (enable_fused_prefill(lora=True): the down / up kernels of csrc/lora.hip on
the prefill, the two-launch group product of csrc/lora_rows.hip inside the decode step) on one GPU:

  speed   one Qwen3-8B decoder layer (E 4096, 32 / 8 heads of 128, I 12288), bf16, every projection wrapped with r = 16, alpha = 32,
          B filled (N(0, 0.02)), eval mode.  Three cases -- a decode step at B = 1 and at B = 16 against a 1024-position cache, a
          prefill at S = 1024 (B = 1) -- and three sides:
            a  the stock forward of the wrapped layer (what the model runs without the switch),
            b  the route (lora=True),
            c  the fused step on a copy with the adapters merged (lora.merge_lora): the floor.
          `--calls` calls between two device events, host time included; interleaved triples a, b, c in ONE process; medians, and per
          comparison the median pair difference with its "spread" = the largest deviation of a pair's difference from that median.
          The bar is a against b: the median difference positive and larger than the spread.  b against c is recorded without a bar.
  trace   a child under `rocprofv3 --kernel-trace --stats`: `--calls` decode steps on the route at B = 1 and as many at B = 16; the two
          kernels of csrc/lora_rows.hip: launches and microseconds per step, the bytes they must move, and the TB/s that makes.

    python tools/lora_infer_ab.py [--pairs 7] [--calls 8] [--out profiles/lora_infer_ab.json]

The parent process never opens the GPU: each part is a child process under its own time limit, started only if the one before it
ended clean; nothing is tried twice."""
import argparse
import copy
import csv
import json
import shutil
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
E, INTER, HQ, HKV, HD, T, R = 4096, 12288, 32, 8, 128, 1024, 16
# the four products of the decode step: (K, [N of each wrapped projection])
GROUPS = [(E, [HQ * HD, HKV * HD, HKV * HD]), (HQ * HD, [E]), (E, [INTER, INTER]), (INTER, [E])]
CASES = (("decode_B1", 1, 1), ("decode_B16", 16, 1), ("prefill_S1024", 1, T))


def _models(dev):
    import torch
    from transformers import Qwen3Config, Qwen3ForCausalLM
    from u2tokenizer_amd.lora import LoRALinear, add_lora, merge_lora
    cfg = Qwen3Config(vocab_size=64, hidden_size=E, intermediate_size=INTER, num_hidden_layers=1, num_attention_heads=HQ,
                      num_key_value_heads=HKV, head_dim=HD, max_position_embeddings=4096, tie_word_embeddings=False)
    torch.manual_seed(0)
    with torch.device(dev):
        m = Qwen3ForCausalLM(cfg)
    m = m.to(torch.bfloat16)
    assert add_lora(m, r=R, alpha=32, dropout=0.05) == 7
    g = torch.Generator(device=dev).manual_seed(1)
    for mod in m.modules():
        if isinstance(mod, LoRALinear):
            w = mod.lora_B["default"].weight
            w.data.copy_(torch.randn(w.shape, device=dev, generator=g) * 0.02)
    m.eval()
    merged = copy.deepcopy(m)
    assert merge_lora(merged) == 7
    return m, merged.eval(), g


def _inputs(dev, g, B, S):
    import torch
    return (torch.randn(B, S, E, device=dev, generator=g) * 0.5).bfloat16()


def _cache(m, prompt):
    """a fresh cache holding the prompt's T positions (untimed)"""
    from transformers.cache_utils import DynamicCache
    cache = DynamicCache(config=m.config)
    m.model(inputs_embeds=prompt, past_key_values=cache, use_cache=True)
    return cache


def _timed(m, x, cache, calls):
    import torch
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        if cache is None:
            m.model(inputs_embeds=x, use_cache=False)
        else:
            m.model(inputs_embeds=x, past_key_values=cache, use_cache=True)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / calls                       # ms per call


def child_speed(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    m, merged, g = _models(dev)
    prefill.enable_fused_prefill(merged)
    sides = {"a": (m, False), "b": (m, True), "c": (merged, None)}

    def run(side, x, prompt):
        model, lora = sides[side]
        if lora is not None:
            prefill.enable_fused_prefill(model, lora=lora)
        cache = _cache(model, prompt) if prompt is not None else None
        return _timed(model, x, cache, a.calls)

    res = {}
    for name, B, S in CASES:
        x = _inputs(dev, g, B, S)
        prompt = _inputs(dev, g, B, T) if S == 1 else None
        for side in "abcabc":                                 # warm-up, every side twice
            run(side, x, prompt)
        n0 = dict(prefill.lora_stats)
        t = {s: [] for s in sides}
        for _ in range(a.pairs):
            for side in "abc":
                t[side].append(run(side, x, prompt))
        key = "decode" if S == 1 else "prefill"
        assert prefill.lora_stats[key] - n0[key] >= a.pairs * a.calls, (name, prefill.lora_stats, n0)   # (the route ran on side b)
        out = {"B": B, "S": S, "cache_positions": T if S == 1 else 0}
        for s, label in (("a", "stock_wrapped"), ("b", "route"), ("c", "merged_fused")):
            out[label + "_ms"] = round(statistics.median(t[s]), 4)
            out[label + "_ms_all"] = [round(v, 4) for v in t[s]]
        for p, q, label in (("a", "b", "stock_minus_route"), ("b", "c", "route_minus_merged")):
            diff = [u - v for u, v in zip(t[p], t[q])]
            md = statistics.median(diff)
            out[label + "_ms"] = round(md, 4)
            out[label + "_spread_ms"] = round(max(abs(d - md) for d in diff), 4)
        out["bar_met"] = out["stock_minus_route_ms"] > 0 and out["stock_minus_route_ms"] > out["stock_minus_route_spread_ms"]
        res[name] = out
        print(name, json.dumps(out), flush=True)
    print("RESULT " + json.dumps(res), flush=True)


def child_trace(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    m, _, g = _models(dev)
    prefill.enable_fused_prefill(m, lora=True)
    for B in (1, 16):
        cache = _cache(m, _inputs(dev, g, B, T))
        x = _inputs(dev, g, B, 1)
        for _ in range(a.calls):
            m.model(inputs_embeds=x, past_key_values=cache, use_cache=True)
    torch.cuda.synchronize()


def must_move():
    """bytes per pair of decode steps (one at B = 1, one at B = 16) that each kernel has to read and write once"""
    el, b = 2, {"lora_rows_down_kernel": 0, "lora_rows_up_kernel": 0}
    for M in (1, 16):
        for K, Ns in GROUPS:
            steps = K // 32
            per = max(8, -(-steps // 64))
            tiles = -(-steps // per) * R * len(Ns) * 64               # the fp32 partial tiles of one block of 16 rows
            b["lora_rows_down_kernel"] += (M * K + R * K * len(Ns)) * el + tiles
            b["lora_rows_up_kernel"] += tiles + sum(N * R + 2 * M * N for N in Ns) * el + M * R * len(Ns) * el
    return b


def _trace_table(d, calls):
    files = sorted(Path(d).rglob("*kernel_stats.csv"))
    if not files:
        return {"error": "no kernel_stats.csv written"}
    rows = list(csv.DictReader(files[0].open()))
    out = {}
    for key, nbytes in must_move().items():
        sel = [r for r in rows if key in r["Name"]]
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        n = sum(int(r["Calls"]) for r in sel)
        out[key] = {"launches_per_step": n / (2 * calls), "expected_launches_per_step": 4, "us_per_launch": round(ns / max(n, 1) / 1e3, 2),
                    "us_per_step": round(ns / (2 * calls) / 1e3, 2), "must_move_MB_per_step_pair": round(nbytes / 1e6, 3),
                    "achieved_TB_s": round(nbytes * calls / ns / 1e3, 3) if ns else None}
    total = sum(float(r["TotalDurationNs"]) for r in rows if "lora" not in r["Name"])
    out["other_kernels_us"] = round(total / 1e3, 1)
    return out


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"lora_infer_ab: timed out after {limit} s: {' '.join(cmd)} -- stopping here")
    if r.returncode != 0:
        raise SystemExit(f"lora_infer_ab: exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}{r.stderr[-2000:]} -- stopping here")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["speed", "trace"])
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    a = ap.parse_args()
    if a.child:
        return {"speed": child_speed, "trace": child_trace}[a.child](a)
    me = [sys.executable, str(Path(__file__).resolve()), "--pairs", str(a.pairs), "--calls", str(a.calls)]
    res = {"what": "one LoRA-wrapped Qwen3-8B decoder layer (E 4096, 32 / 8 heads of 128, I 12288; bf16; r 16, alpha 32 on all seven "
                   "projections, eval mode) without grad: a = its stock forward, b = the route (lora=True), c = the fused step on merged "
                   "weights; a decode step at B 1 and B 16 against 1024 cached positions and a prefill at S 1024; interleaved triples in "
                   "one process, ms per call with host time; spread = largest deviation of a pair's difference from the median "
                   "difference; bar: stock_minus_route_ms > max(0, its spread); trace: rocprofv3 --kernel-trace --stats of the route's "
                   "decode steps"}
    out = _run(me + ["--child", "speed"], 420)
    res["speed"] = json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])
    print(json.dumps(res["speed"]), flush=True)
    prof = shutil.which("rocprofv3")
    if a.no_trace or prof is None:
        res["trace"] = {"skipped": "rocprofv3 not found" if prof is None else "--no-trace"}
    else:
        d = tempfile.mkdtemp(prefix="lora_infer_trace_")
        _run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace"], 420)
        res["trace"] = _trace_table(d, a.calls)
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res["trace"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
