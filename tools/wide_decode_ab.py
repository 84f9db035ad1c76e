#!/usr/bin/env python
"""A/B of the decode step of more than 16 sequences (enable_fused_prefill(model, wide_decode=True)), on one GPU, at the Qwen3-8B
layer shape with synthetic weights, for bf16 and e4m3 (fp8_decode=True) weights, at B = 16, 32, 48, 64 sequences against KV caches
of T = 1024 / 2048 positions.  Three ways to advance the same B sequences by one token, interleaved on the same box:

  a  wide    one fused step of B sequences (B = 16: today's fused step, the wide kernels start at 17)
  b  stock   the stock HF layers on the B sequences: what a batch of more than 16 takes without the switch
  c  chunks  ceil(B / 16) fused steps of at most 16 sequences each, one after the other: the workaround without the switch

Per variant: 16 greedy steps (after one outside the clock) on append-in-place caches filled with T random positions (built as the fused prefill leaves them),
per-step ms from device events around the 16 steps, host time of the calls included, as `generate` pays it; medians over the
rounds, "spread" = the largest deviation of a round's a - c difference from the median difference.  The route counters are checked.

    python tools/wide_decode_ab.py [--layers 4] [--rounds 3] [--variants wide,stock,chunks] [--batches 16,32,48,64]
                                   [--lengths 1024,2048] [--out profiles/wide_decode_ab.json]

--variants / --batches / --lengths cut the run down, e.g. `--variants wide --batches 16,64 --lengths 1024` to compare the fused
step between two builds of the library (one run per build); the a - c columns are left out when a or c is.

The parent process never opens the GPU: each weight form is a child process of its own under its own time limit, started only if
the one before it ended clean; nothing is tried twice.  The decoder has --layers layers (36 in Qwen3-8B): per-step times scale
with the layer count, the ratios do not (the stock layers' per-step host cost included: it is per layer too)."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS, E, INTER, HQ, HKV, HD = 16, 4096, 12288, 32, 8, 128
BATCHES, LENGTHS = (16, 32, 48, 64), (1024, 2048)


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


def _cache(m, B, T, like):
    """a DynamicCache whose layers are the append-in-place layers a fused prefill of T positions leaves, filled with noise"""
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd import prefill
    cache = DynamicCache(config=m.config)
    for li in range(m.config.num_hidden_layers):
        lay = prefill._prefill_append_layer(cache, li, B, HKV, T, HD, like)
        assert lay is not None, "this transformers' DynamicCache does not take the append-in-place layer"
        lay._kb.normal_()
        lay._vb.normal_()
        lay._commit(T)
    return cache


def child(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    fp8 = a.child == "w8"
    m = _model(a.layers, dev, torch.bfloat16)
    like = torch.empty(1, dtype=torch.bfloat16, device=dev)
    res = []

    def steps(caches, toks):
        """STEPS greedy steps of every (cache, token) chunk in turn -> ms per step of the whole batch"""
        def one(toks):
            return [m(input_ids=tok, past_key_values=c, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
                    for c, tok in zip(caches, toks)]

        toks = one(toks)   # outside the clock: re-enabling the route rebuilds its per-layer state (the e4m3 copies among it)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(STEPS):
            toks = one(toks)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / STEPS

    def run(how, B, T):
        tok = torch.randint(3, 1024, (B, 1), device=dev, generator=torch.Generator(device=dev).manual_seed(B + T))
        if how == "stock":
            prefill.disable_fused_prefill(m)
        else:
            prefill.enable_fused_prefill(m, fp8_decode=fp8, wide_decode=how == "wide")
        sizes = [min(16, B - r) for r in range(0, B, 16)] if how == "chunks" else [B]
        caches = [_cache(m, n, T, like) for n in sizes]
        n0, s0, w0 = dict(prefill.wide_stats), dict(prefill.stats), dict(prefill.w8_stats)
        ms = steps(caches, list(tok.split(sizes)))
        calls = (STEPS + 1) * a.layers * len(sizes)
        assert prefill.stats["decode"] - s0["decode"] == (0 if how == "stock" else calls), how
        assert prefill.wide_stats["decode"] - n0["decode"] == (calls if how == "wide" and B > 16 else 0), how
        assert prefill.w8_stats["decode"] - w0["decode"] == (calls if fp8 and how != "stock" else 0), how
        return ms

    hows = [h for h in ("wide", "stock", "chunks") if h in a.variants.split(",")]
    for T in (int(v) for v in a.lengths.split(",")):
        for B in (int(v) for v in a.batches.split(",")):
            for how in hows:     # warm-up (builds the e4m3 copies, sizes the workspaces)
                run(how, B, T)
            t = {how: [] for how in hows}
            for _ in range(a.rounds):
                for how in hows:
                    t[how].append(run(how, B, T))
            med = {k: statistics.median(v) for k, v in t.items()}
            row = {"weights": a.child, "B": B, "T": T, "layers": a.layers, "steps": STEPS, "rounds": a.rounds}
            row.update({f"{k}_ms_per_step": round(v, 4) for k, v in med.items()})
            row.update({f"{k}_ms_per_step_min_max": [round(min(v), 4), round(max(v), 4)] for k, v in t.items()})
            if "wide" in med and "chunks" in med:
                diff = [x - y for x, y in zip(t["wide"], t["chunks"])]
                md = statistics.median(diff)
                row.update({"wide_minus_chunks_ms": round(md, 4), "spread_ms": round(max(abs(x - md) for x in diff), 4),
                            "chunks_over_wide": round(med["chunks"] / med["wide"], 3)})
            if "wide" in med and "stock" in med:
                row["stock_over_wide"] = round(med["stock"] / med["wide"], 3)
            if "wide" in med:
                row["wide_tokens_per_s"] = round(B / med["wide"] * 1e3, 1)
            res.append(row)
            print(json.dumps(res[-1]), flush=True)
    prefill.disable_fused_prefill(m)
    print("RESULT " + json.dumps(res), flush=True)


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"wide_decode_ab: timed out after {limit} s: {' '.join(cmd)} -- stopping here")
    if r.returncode != 0:
        raise SystemExit(f"wide_decode_ab: exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}{r.stderr[-2000:]} -- stopping here")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variants", default="wide,stock,chunks")
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    ap.add_argument("--lengths", default=",".join(str(t) for t in LENGTHS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["bf16", "w8"])
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = [sys.executable, str(Path(__file__).resolve()), "--layers", str(a.layers), "--rounds", str(a.rounds), "--variants", a.variants,
          "--batches", a.batches, "--lengths", a.lengths]
    res = {"what": "decode step of B sequences at the Qwen3-8B layer shape, synthetic weights: a = one fused step of B sequences "
                   "(wide_decode=True), b = the stock layers, c = ceil(B / 16) fused steps of <= 16 sequences; interleaved rounds "
                   "of 16 greedy steps on append-in-place caches of T positions; ms per step, host time included; spread = largest "
                   "deviation of a round's a - c from the median a - c", "layers": a.layers, "rows": []}
    for form in ("bf16", "w8"):
        out = _run(me + ["--child", form], 420)
        rows = json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])
        res["rows"] += rows
        for r in rows:
            print(json.dumps(r), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
