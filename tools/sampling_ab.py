#!/usr/bin/env python
"""A/B of the fused sampling warper (u2tokenizer_amd/sampling.py, csrc/sample.hip) against the transformers warpers it replaces
(TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper), on one GPU, in one process per part:

  warper   interleaved pairs on the same fp32 logits (randn * 3 rounded to bf16 values: what a bf16 lm_head hands over; the logits are
           rewritten before every call so that neither side finds its input warmer than `generate` would): a = the stock list,
           b = FusedSamplingWarper; us per call (device events around `--calls` calls, host time of the calls included, as `generate`
           pays it), medians over the pairs, "spread" = the largest deviation of a pair's difference from the median difference.
           Shapes (rows, V) = (1, 151936), (8, 151936), (16, 128256), (1, 32064); parameter sets T 0.7 p 0.9 / T 1 k 50 p 0.9 / T 1 p 0.9.
           Next to the times: histogram passes the kernel took per row (from its workspace records) and whether both kept the same
           number of tokens.
  decode   64 sampled decode steps (do_sample, top_p 0.9, temperature 0.7; torch.multinomial draws on both sides) after a fused prefill
           at the Qwen3-8B layer shape with synthetic weights and the Qwen3 vocabulary, `config.u2_fused_sampling` on against off,
           interleaved pairs; ms per step.

    python tools/sampling_ab.py [--layers 4] [--pairs 7] [--calls 50] [--out profiles/sampling_ab.json]

The parent process never opens the GPU: each part is a child process under its own time limit, started only if the one before it
ended clean; nothing is tried twice."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS, E, INTER, HQ, HKV, HD, VOCAB = 64, 4096, 12288, 32, 8, 128, 151936
SHAPES = [(1, 151936), (8, 151936), (16, 128256), (1, 32064)]
PARAMS = [("T0.7_p0.9", 0.7, 0, 0.9), ("T1_k50_p0.9", 1.0, 50, 0.9), ("T1_p0.9", 1.0, 0, 0.9)]


def _pairs(run_a, run_b, pairs):
    ta, tb = [], []
    for _ in range(pairs):
        ta.append(run_a())
        tb.append(run_b())
    diff = [x - y for x, y in zip(ta, tb)]
    md = statistics.median(diff)
    return statistics.median(ta), statistics.median(tb), md, max(abs(x - md) for x in diff)


def child_warper(a):
    import torch
    from transformers.generation.logits_process import (LogitsProcessorList, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    from u2tokenizer_amd import _lib, ops, sampling
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    res = []
    for rows, V in SHAPES:
        src = (torch.randn(rows, V, device=dev, generator=torch.Generator(device=dev).manual_seed(V + rows)) * 3).bfloat16()
        x = torch.empty(rows, V, dtype=torch.float32, device=dev)
        for name, T, k, p in PARAMS:
            stock = LogitsProcessorList(([TemperatureLogitsWarper(T)] if T != 1.0 else []) + ([TopKLogitsWarper(k)] if k else []) +
                                        [TopPLogitsWarper(p)])
            fused = sampling.fuse_warpers(stock)
            assert len(fused) == 1 and type(fused[0]) is sampling.FusedSamplingWarper

            def run(procs):
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                tot = 0.0
                for _ in range(a.calls):
                    x.copy_(src)                       # (the .float() of the lm_head's output, as `generate` does it: outside the clock)
                    t0.record()
                    procs(None, x)
                    t1.record()
                    t1.synchronize()
                    tot += t0.elapsed_time(t1)
                return tot / a.calls * 1e3             # us per call

            x.copy_(src)
            ka, kb = (stock(None, x) > -float("inf")).sum(-1), (fused(None, x) > -float("inf")).sum(-1)
            # the kernel's own record of the last call: histogram passes per row
            h = _lib.load_library("bf16")
            nbytes = h.u2tok_sample_warp_workspace_bytes(rows, V)
            ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
            out = torch.empty_like(x)
            _lib.check(h.u2tok_sample_warp(x.data_ptr(), V, out.data_ptr(), V, rows, V, T, k, p, 1, ws.data_ptr(), nbytes,
                                           torch.cuda.current_stream().cuda_stream), "u2tok_sample_warp")
            passes = ws.view(-1, 8)[:rows, 3].tolist()
            for procs in (stock, fused):               # warm-up
                run(procs)
            n0 = sampling.stats["fused"]
            sa, sb, md, spread = _pairs(lambda: run(stock), lambda: run(fused), a.pairs)
            assert sampling.stats["fused"] - n0 == a.pairs * a.calls
            res.append({"rows": rows, "V": V, "params": name, "pairs": a.pairs, "calls": a.calls, "stock_us": round(sa, 2),
                        "fused_us": round(sb, 2), "stock_minus_fused_us": round(md, 2), "spread_us": round(spread, 2),
                        "stock_over_fused": round(sa / sb, 2), "same_kept_count": bool(torch.equal(ka, kb)),
                        "kept_per_row_max": int(kb.max()), "histogram_passes_per_row": [min(passes), max(passes)]})
            print(json.dumps(res[-1]), flush=True)
    print("RESULT " + json.dumps(res), flush=True)


def child_decode(a):
    import torch
    from u2tokenizer_amd import language_model as LM, ops, prefill, sampling
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    cfg = LM.u2Qwen3Config(vocab_size=VOCAB, hidden_size=E, intermediate_size=INTER, num_hidden_layers=a.layers,
                           num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=HD, max_position_embeddings=4096,
                           tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=None)
    torch.manual_seed(0)
    with torch.device(dev):
        m = LM.u2Qwen3ForCausalLM(cfg)
    m = m.to(torch.bfloat16).eval()
    res = []
    for B in (1, 8):
        ids = torch.randint(3, VOCAB, (B, 128), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
        kw = dict(do_sample=True, top_p=0.9, temperature=0.7, max_new_tokens=STEPS + 1, min_new_tokens=STEPS + 1)

        def run(on):
            m.config.u2_fused_sampling = on
            torch.manual_seed(1)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            m.generate(None, ids, **kw)
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / (STEPS + 1)       # ms per generated token (the prefill's share is the same on both sides)

        for on in (False, True):
            run(on)
        n0, d0 = sampling.stats["fused"], prefill.stats["decode"]
        sa, sb, md, spread = _pairs(lambda: run(False), lambda: run(True), a.pairs)
        assert sampling.stats["fused"] - n0 == a.pairs * (STEPS + 1)
        assert prefill.stats["decode"] - d0 == 2 * a.pairs * STEPS * a.layers
        res.append({"B": B, "layers": a.layers, "steps": STEPS, "pairs": a.pairs, "stock_ms_per_step": round(sa, 4),
                    "fused_ms_per_step": round(sb, 4), "stock_minus_fused_ms": round(md, 4), "spread_ms": round(spread, 4)})
        print(json.dumps(res[-1]), flush=True)
    print("RESULT " + json.dumps(res), flush=True)


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"sampling_ab: timed out after {limit} s: {' '.join(cmd)} -- stopping here")
    if r.returncode != 0:
        raise SystemExit(f"sampling_ab: exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}{r.stderr[-2000:]} -- stopping here")
    return r.stdout


def _result(stdout):
    return json.loads(next(ln for ln in stdout.splitlines() if ln.startswith("RESULT "))[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["warper", "decode"])
    ap.add_argument("--no-decode", action="store_true", help="skip the generate part")
    a = ap.parse_args()
    if a.child:
        return {"warper": child_warper, "decode": child_decode}[a.child](a)
    me = [sys.executable, str(Path(__file__).resolve()), "--layers", str(a.layers), "--pairs", str(a.pairs), "--calls", str(a.calls)]
    res = {"what": "fused sampling warper (one HIP launch) against the transformers temperature / top-k / top-p warpers on the same fp32 "
                   "logits (bf16-valued randn * 3); interleaved pairs; us per call with the host time of the calls; spread = largest "
                   "deviation of a pair's difference from the median difference.  decode: 64 sampled steps of `generate` after a fused "
                   "prefill, Qwen3-8B layer shape, synthetic weights, config.u2_fused_sampling off against on",
           "layers": a.layers}
    res["warper"] = _result(_run(me + ["--child", "warper"], 300))
    print(json.dumps(res["warper"]), flush=True)
    if a.no_decode:
        res["decode"] = {"skipped": "--no-decode"}
    else:
        res["decode"] = _result(_run(me + ["--child", "decode"], 420))
    print(json.dumps(res["decode"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
