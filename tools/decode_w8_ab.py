#!/usr/bin/env python
"""A/B of the FP8 (e4m3) weight-only decode step (enable_fused_prefill(model, fp8_decode=True)) against the 16-bit decode step of the
same tree, on one GPU, at the Qwen3-8B layer shape with synthetic weights:

  speed    interleaved pairs: the same 64 greedy decode steps after a fused prefill, a = bf16 decode, b = e4m3 decode, at B = 1
           and B = 8; per-step ms (device events around the 64 steps, host time of the calls included, as `generate` pays it),
           medians over the pairs, "spread" = the largest deviation of a pair's difference from the median difference
  trace    a child under `rocprofv3 --kernel-trace --stats` (B = 1): total time of the few-rows product kernels of either kind and
           the weight bytes they streamed -> achieved TB/s of the four products.  (Counters, if wanted, in a run of their own.)
  quality  teacher-forced on the fp32 model's greedy ids: distance of the e4m3 decode logits from the fp32 model next to the bf16
           run's distance, and greedy-id agreement over 64 steps -- on the synthetic weights as they are, and on the same model
           with weights snapped onto values the quantiser keeps exactly (ops.snap_fp8_: the control, where e4m3 loses nothing)

    python tools/decode_w8_ab.py [--layers 4] [--pairs 5] [--out profiles/decode_w8_ab.json]

The parent process never opens the GPU: every GPU step is a child process of its own under its own time limit, started only if
the one before it ended clean; nothing is tried twice.  The decoder has --layers layers (36 in Qwen3-8B): per-step times scale
with the layer count, the ratio does not.  No trained checkpoint is involved: quality on trained weights is NOT measured here."""
import argparse
import csv
import json
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS, E, INTER, HQ, HKV, HD = 64, 4096, 12288, 32, 8, 128


def _model(layers, dev, dtype, seed=0):
    import torch
    from transformers import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config(vocab_size=1024, hidden_size=E, intermediate_size=INTER, num_hidden_layers=layers, num_attention_heads=HQ,
                      num_key_value_heads=HKV, head_dim=HD, max_position_embeddings=4096, tie_word_embeddings=False,
                      pad_token_id=0, bos_token_id=1, eos_token_id=2)
    torch.manual_seed(seed)
    with torch.device(dev):
        m = Qwen3ForCausalLM(cfg)
    return m.to(dtype).eval()


def _greedy(m, ids, steps, forced=None):
    """prefill `ids`, then `steps` decode steps; -> (logits of every decode step (steps, B, V), ids chosen (B, steps), ids fed
    (B, steps)); forced: the ids fed instead of the model's own (teacher forcing)"""
    import torch
    out = m(input_ids=ids, use_cache=True)
    cache, tok = out.past_key_values, out.logits[:, -1].argmax(-1, keepdim=True)
    logits, chosen, fed = [], [], []
    for t in range(steps):
        if forced is not None:
            tok = forced[:, t:t + 1]
        fed.append(tok)
        o = m(input_ids=tok, past_key_values=cache, use_cache=True)
        logits.append(o.logits[:, -1])
        tok = o.logits[:, -1].argmax(-1, keepdim=True)
        chosen.append(tok)
    return torch.stack(logits), torch.cat(chosen, 1), torch.cat(fed, 1)


def child_speed(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    m = _model(a.layers, dev, torch.bfloat16)
    res = []
    for B in (1, 8):
        ids = torch.randint(3, 1024, (B, 128), device=dev, generator=torch.Generator(device=dev).manual_seed(B))

        def run(fp8):
            prefill.enable_fused_prefill(m, fp8_decode=fp8)      # (sets the switches only once the layers are patched)
            out = m(input_ids=ids, use_cache=True)
            cache, tok = out.past_key_values, out.logits[:, -1].argmax(-1, keepdim=True)
            # one step outside the clock: switching fp8_decode off drops the e4m3 copies, so the first e4m3 step rebuilds them
            tok = m(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(STEPS):
                tok = m(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / STEPS

        for fp8 in (False, True):     # warm-up (builds the e4m3 copies)
            run(fp8)
        n0 = dict(prefill.w8_stats)
        ta, tb = [], []
        for _ in range(a.pairs):
            ta.append(run(False))
            tb.append(run(True))
        assert prefill.w8_stats["decode"] - n0["decode"] == a.pairs * (STEPS + 1) * a.layers
        diff = [x - y for x, y in zip(ta, tb)]
        md = statistics.median(diff)
        res.append({"B": B, "layers": a.layers, "steps": STEPS, "pairs": a.pairs, "bf16_ms_per_step": round(statistics.median(ta), 4),
                    "w8_ms_per_step": round(statistics.median(tb), 4), "bf16_minus_w8_ms": round(md, 4),
                    "spread_ms": round(max(abs(x - md) for x in diff), 4),
                    "bf16_over_w8": round(statistics.median(ta) / statistics.median(tb), 3)})
    prefill.disable_fused_prefill(m)
    print("RESULT " + json.dumps(res), flush=True)


def child_trace(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    m = _model(a.layers, dev, torch.bfloat16)
    ids = torch.randint(3, 1024, (1, 128), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for fp8 in (False, True):
        prefill.enable_fused_prefill(m, fp8_decode=fp8)
        _greedy(m, ids, STEPS)
    torch.cuda.synchronize()
    prefill.disable_fused_prefill(m)


def child_quality(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)

    def err(x, ref):
        return ((x.double() - ref.double()).pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()

    res = {}
    for name in ("synthetic", "snapped"):
        m32 = _model(a.layers, dev, torch.float32, seed=1)       # the reference: fp32 on the GPU, stock layers
        if name == "snapped":
            ops.snap_fp8_(m32.model.layers)
        ids = torch.randint(3, 1024, (1, 128), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        ref, want, forced = _greedy(m32, ids, STEPS)
        mg = _model(a.layers, dev, torch.float32, seed=1)
        mg.load_state_dict(m32.state_dict())
        del m32
        mg = mg.to(torch.bfloat16)
        row = {}
        for fp8 in (False, True):
            prefill.enable_fused_prefill(mg, fp8_decode=fp8)
            n0 = prefill.w8_stats["decode"]
            logits, chosen, _ = _greedy(mg, ids, STEPS, forced=forced)
            assert (prefill.w8_stats["decode"] - n0 == STEPS * a.layers) == fp8
            k = "w8" if fp8 else "bf16"
            row[f"{k}_logit_distance"] = round(err(logits, ref), 6)
            row[f"{k}_greedy_agreement"] = round((chosen == want).double().mean().item(), 4)
        prefill.disable_fused_prefill(mg)
        del mg
        res[name] = row
    print("RESULT " + json.dumps(res), flush=True)


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"decode_w8_ab: timed out after {limit} s: {' '.join(cmd)} -- stopping here")
    if r.returncode != 0:
        raise SystemExit(f"decode_w8_ab: exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}{r.stderr[-2000:]} -- stopping here")
    return r.stdout


def _result(stdout):
    return json.loads(next(ln for ln in stdout.splitlines() if ln.startswith("RESULT "))[7:])


def _trace_table(d, layers):
    """achieved TB/s of the four products from rocprofv3's kernel statistics (weights streamed once per step and layer)"""
    files = sorted(Path(d).rglob("*kernel_stats.csv"))
    if not files:
        return {"error": "no kernel_stats.csv written"}
    per_layer = ((HQ + 2 * HKV) * HD * E + E * HQ * HD + 2 * INTER * E + E * INTER)      # weight elements of the four products
    out = {}
    rows = list(csv.DictReader(files[0].open()))
    # gemm_rows16_kernel<NW, NB, PAIR, WForm> (csrc/gemm_rows.hip): the weight form is the last template argument, (u2::WForm)0 / 1
    for key, pat, nbytes in (("bf16", r"gemm_rows16_kernel<[^>]*WForm\)0>", 2), ("w8", r"gemm_rows16_kernel<[^>]*WForm\)1>", 1)):
        sel = [r for r in rows if re.search(pat, r["Name"])]
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        calls = sum(int(r["Calls"]) for r in sel)
        total = per_layer * nbytes * layers * STEPS
        out[key] = {"kernel_calls": calls, "expected_calls": 4 * layers * STEPS, "kernel_ms_per_step": round(ns / STEPS / 1e6, 4),
                    "weight_GB_per_step": round(total / STEPS / 1e9, 4), "achieved_TB_s": round(total / ns / 1e3, 3) if ns else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["speed", "trace", "quality"])
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    a = ap.parse_args()
    if a.child:
        return {"speed": child_speed, "trace": child_trace, "quality": child_quality}[a.child](a)
    me = [sys.executable, str(Path(__file__).resolve()), "--layers", str(a.layers), "--pairs", str(a.pairs)]
    res = {"what": "FP8 (e4m3) weight-only decode step against the bf16 decode step of the same tree; Qwen3-8B layer shape, synthetic "
                   "weights; interleaved pairs of 64 greedy steps; spread = largest deviation of a pair's difference from the median "
                   "difference; quality on trained weights: not measured (no checkpoint)", "layers": a.layers}
    res["speed"] = _result(_run(me + ["--child", "speed"], 420))
    print(json.dumps(res["speed"]), flush=True)
    res["quality"] = _result(_run(me + ["--child", "quality"], 420))
    print(json.dumps(res["quality"]), flush=True)
    prof = shutil.which("rocprofv3")
    if a.no_trace or prof is None:
        res["trace"] = {"skipped": "rocprofv3 not found" if prof is None else "--no-trace"}
    else:
        d = tempfile.mkdtemp(prefix="decode_w8_trace_")
        _run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace"], 420)
        res["trace"] = _trace_table(d, a.layers)
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res["trace"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
