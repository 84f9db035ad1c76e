#!/usr/bin/env python
"""A/B of the LoRA training route (enable_fused_prefill(train_lora=True): decoder_train.LoraDeltaFn over csrc/lora.hip) against the
stock forward of the same LoRA-wrapped layer -- what a wrapped layer runs without the switch --, on one GPU:

  speed   one Qwen3-8B decoder layer (E 4096, 32 / 8 heads of 128, I 12288), bf16, B = 1, S = 1024, every projection wrapped with
          r = 16, alpha = 32, nn.Dropout(0.05), B filled (N(0, 0.02)), base frozen, the input requires grad: forward + backward through
          the decoder stack of that one layer (the final norm included on both sides), `--calls` calls between two device events,
          host time included; interleaved pairs a = stock, b = route in ONE process; medians, and "spread" = the largest deviation of
          a pair's difference from the median difference.
  trace   a child under `rocprofv3 --kernel-trace --stats`: `--calls` forward + backward calls on the route; the adapter kernels' total
          time per call next to the bytes each must move (every operand read or written once) and the TB/s that makes.

    python tools/lora_train_ab.py [--pairs 7] [--calls 5] [--out profiles/lora_train_ab.json]

The parent process never opens the GPU: each part is a child process under its own time limit, started only if the one before it
ended clean; nothing is tried twice."""
import argparse
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
E, INTER, HQ, HKV, HD, S, R = 4096, 12288, 32, 8, 128, 1024, 16
# (in features, out features) of the seven projections
PROJ = [(E, HQ * HD), (E, HKV * HD), (E, HKV * HD), (HQ * HD, E), (E, INTER), (E, INTER), (INTER, E)]


def _layer(dev):
    import torch
    from transformers import Qwen3Config, Qwen3ForCausalLM
    from u2tokenizer_amd.lora import LoRALinear, add_lora
    cfg = Qwen3Config(vocab_size=64, hidden_size=E, intermediate_size=INTER, num_hidden_layers=1, num_attention_heads=HQ,
                      num_key_value_heads=HKV, head_dim=HD, max_position_embeddings=2048, tie_word_embeddings=False)
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
    m.train()
    x = (torch.randn(1, S, E, device=dev, generator=g) * 0.5).bfloat16().requires_grad_(True)
    dy = torch.randn(1, S, E, device=dev, generator=g).bfloat16()
    return m, x, dy


def _step(m, x, dy):
    import torch
    with torch.enable_grad():
        h = m.model(inputs_embeds=x, use_cache=False).last_hidden_state
        h.backward(dy)
    x.grad = None
    m.zero_grad(set_to_none=True)


def child_speed(a):
    import torch
    from u2tokenizer_amd import decoder_train, ops, prefill
    ops.device_check()
    dev = torch.device("cuda", 0)
    m, x, dy = _layer(dev)

    def run(route):
        prefill.enable_fused_prefill(m, train_lora=route, prefill=False)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.calls):
            _step(m, x, dy)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.calls                   # ms per forward + backward

    for route in (False, True, False, True):                   # warm-up, both sides
        run(route)
    ta, tb = [], []
    l0, n0 = decoder_train.lora_stats["layers"], decoder_train.lora_stats["adapters"]
    for _ in range(a.pairs):
        ta.append(run(False))
        tb.append(run(True))
    assert decoder_train.lora_stats["layers"] - l0 == a.pairs * a.calls and decoder_train.lora_stats["adapters"] - n0 == 7 * a.pairs * a.calls
    diff = [p - q for p, q in zip(ta, tb)]
    md = statistics.median(diff)
    res = {"pairs": a.pairs, "calls": a.calls, "stock_ms": round(statistics.median(ta), 4), "route_ms": round(statistics.median(tb), 4),
           "stock_minus_route_ms": round(md, 4), "spread_ms": round(max(abs(d - md) for d in diff), 4),
           "stock_over_route": round(statistics.median(ta) / statistics.median(tb), 3),
           "stock_ms_all": [round(t, 4) for t in ta], "route_ms_all": [round(t, 4) for t in tb]}
    print("RESULT " + json.dumps(res), flush=True)


def child_trace(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    dev = torch.device("cuda", 0)
    m, x, dy = _layer(dev)
    prefill.enable_fused_prefill(m, train_lora=True, prefill=False)
    for _ in range(a.calls):
        _step(m, x, dy)
    torch.cuda.synchronize()


def must_move():
    """bytes per forward + backward of the layer that each kernel class has to read and write once (bf16 everywhere)"""
    M, el = S, 2
    b = {"lora_down_kernel": 0, "lora_up_kernel": 0, "lora_wgrad_kernel": 0}
    for K, N in PROJ:
        b["lora_down_kernel"] += (M * K + R * K + M * R) * el          # u = xd A^T
        b["lora_down_kernel"] += (M * N + R * N + M * R) * el          # du = s dy B
        b["lora_up_kernel"] += (2 * M * N + M * R + N * R) * el        # y += s u B^T
        b["lora_up_kernel"] += (M * K + M * R + K * R) * el            # d xd = du A
        b["lora_wgrad_kernel"] += (M * K + M * R + R * K) * el         # dA = du^T xd
        b["lora_wgrad_kernel"] += (M * N + M * R + R * N) * el         # dB^T = s u^T dy
    return b


def _trace_table(d, calls):
    files = sorted(Path(d).rglob("*kernel_stats.csv"))
    if not files:
        return {"error": "no kernel_stats.csv written"}
    rows = list(csv.DictReader(files[0].open()))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {"all_kernels_ms_per_call": round(total / calls / 1e6, 4)}
    want = {"lora_down_kernel": 14, "lora_up_kernel": 14, "lora_wgrad_kernel": 14}
    for key, nbytes in must_move().items():
        sel = [r for r in rows if key in r["Name"]]
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        out[key] = {"launches_per_call": sum(int(r["Calls"]) for r in sel) / calls, "expected_launches_per_call": want[key],
                    "us_per_call": round(ns / calls / 1e3, 2), "must_move_MB_per_call": round(nbytes / 1e6, 2),
                    "achieved_TB_s": round(nbytes * calls / ns / 1e3, 3) if ns else None}
    sel = [r for r in rows if "lora_wgrad_reduce_kernel" in r["Name"]]
    out["lora_wgrad_reduce_kernel"] = {"launches_per_call": sum(int(r["Calls"]) for r in sel) / calls,
                                       "us_per_call": round(sum(float(r["TotalDurationNs"]) for r in sel) / calls / 1e3, 2)}
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]
    out["top_kernels_us_per_call"] = {r["Name"][:60]: round(float(r["TotalDurationNs"]) / calls / 1e3, 1) for r in top}
    return out


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"lora_train_ab: timed out after {limit} s: {' '.join(cmd)} -- stopping here")
    if r.returncode != 0:
        raise SystemExit(f"lora_train_ab: exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}{r.stderr[-2000:]} -- stopping here")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["speed", "trace"])
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    a = ap.parse_args()
    if a.child:
        return {"speed": child_speed, "trace": child_trace}[a.child](a)
    me = [sys.executable, str(Path(__file__).resolve()), "--pairs", str(a.pairs), "--calls", str(a.calls)]
    res = {"what": "forward + backward of one LoRA-wrapped Qwen3-8B decoder layer (E 4096, 32 / 8 heads of 128, I 12288; bf16, B 1, S 1024; "
                   "r 16, alpha 32, dropout 0.05 on all seven projections, base frozen) on the training route (train_lora) against its "
                   "stock forward; interleaved pairs in one process, ms per call with host time; spread = largest deviation of a pair's "
                   "difference from the median difference; trace: rocprofv3 --kernel-trace --stats of the route"}
    out = _run(me + ["--child", "speed"], 420)
    res["speed"] = json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])
    print(json.dumps(res["speed"]), flush=True)
    prof = shutil.which("rocprofv3")
    if a.no_trace or prof is None:
        res["trace"] = {"skipped": "rocprofv3 not found" if prof is None else "--no-trace"}
    else:
        d = tempfile.mkdtemp(prefix="lora_train_trace_")
        _run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace"], 420)
        res["trace"] = _trace_table(d, a.calls)
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res["trace"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
