#!/usr/bin/env python
"""A/B of the decode step on the FP8 (e4m3) KV cache: the per-layer step (a: what `kv8=True, stack_decode=True` does on such a cache
without the new switch -- two library calls and a Python loop iteration per layer, the quantiser a launch of its own) against the
whole-stack step on the codes (b: `stack_kv8=True`, one library call per token, the quantising append in the rotary kernel), with
the whole-stack step on the 16-bit append-in-place cache beside them for context (c: `stack_decode=True`).  One process per
measurement, the arms interleaved, on one GPU, synthetic weights:

  grid    8 layers of Qwen3-8B (V = 1 024: the head is not what is measured), weights in bf16 and in e2m1, B = 1, 16 and 64
          (`wide_decode`) x T = 1 024 and 8 192 cached positions of N(0, 1) keys and values written through the layers' own `update`
          (so the e4m3 cache is what its quantiser makes of the 16-bit one).  ONE model per weight form: the arms are the same
          weights with the switches set anew before each run, outside the clock.
  deep    one cell of 36 layers at B = 1, T = 1 024 on e2m1 weights with the real vocabulary (V = 151 936), with and without the
          `head` switch (a with `head` runs the module norm and nn.Linear: the parent's `head_route` says "stock" on this cache).

Per run: 16 greedy steps after one unclocked step; per-step ms from device events around the steps, host time of the calls
included, as `generate` pays it; medians over the rounds, and for a / b and c / b the median of the rounds' ratios with its spread
(the largest deviation of a round's ratio from that median).  The counters are checked after every run: an arm that took another
route than its name says stops the tool.

    python tools/stack_kv8_ab.py [--rounds 3] [--out profiles/stack_kv8_ab.json]

The parent process never opens the GPU: every GPU step is a child process of its own under its own time limit, started only if the
one before it ended clean; nothing is tried twice.  NOT measured here: trained weights (no checkpoint; the bits are those of the
per-layer kv8 route, tests/test_gpu_stack_kv8.py), the f16 build's speed, Phi-3 shapes, B between 1 and 16."""
import argparse
import json
import statistics
import subprocess
import sys
import threading
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from decode_w4_ab import _box, _ratios, _result  # noqa: E402

STEPS = 16
QWEN3_8B = dict(E=4096, I=12288, Hq=32, Hkv=8, D=128)
FORMS = {"bf16": {}, "e2m1": dict(fp4_decode=True)}
CHILDREN = {   # layers, vocabulary, weight forms, (B, T) cells, head switch off / on, time limit of the child in seconds
    "grid": dict(layers=8, vocab=1024, forms=("bf16", "e2m1"), cells=[(B, T) for B in (1, 16, 64) for T in (1024, 8192)], heads=(False,),
                 limit=540),
    "deep": dict(layers=36, vocab=151936, forms=("e2m1",), cells=[(1, 1024)], heads=(False, True), limit=420),
}
ARMS = {   # the switches of each arm (all: wide_decode and the weight form's) and the cache it runs on
    "a": (dict(kv8=True, stack_decode=True), "e4m3"),
    "b": (dict(stack_kv8=True), "e4m3"),
    "c": (dict(stack_decode=True), "16-bit"),
}
NOT_MEASURED = ["trained weights (no checkpoint: accuracy of the e4m3 cache is the per-layer kv8 route's, bit for bit)",
                "the f16 build's speed", "Phi-3 shapes", "B between 1 and 16"]


def _model(layers, vocab, dev):
    import torch
    from u2tokenizer_amd import language_model as LM
    s = QWEN3_8B
    cfg = LM.u2Qwen3Config(vocab_size=vocab, hidden_size=s["E"], intermediate_size=s["I"], num_hidden_layers=layers,
                           num_attention_heads=s["Hq"], num_key_value_heads=s["Hkv"], head_dim=s["D"], max_position_embeddings=16384,
                           tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    torch.manual_seed(0)
    with torch.device(dev):
        m = LM.u2Qwen3ForCausalLM(cfg)
    m = m.to(torch.bfloat16).eval()
    m.__dict__["_u2_fuse_checked"] = {False, True}   # (the switches are set per arm below, not from the config)
    return m


def _filled(layers, kv8, k, v):
    """a plain DynamicCache of T cached positions in every layer, through the layer's own `update`"""
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd import prefill
    cache = DynamicCache()
    for _ in range(layers):
        lay = prefill.Kv8Layer() if kv8 else prefill._append_layer_class()()
        lay.update(k, v)
        cache.layers.append(lay)
    return cache


def child(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    c, s = CHILDREN[a.child], QWEN3_8B
    layers = c["layers"]
    res = []
    for form in c["forms"]:
        m = _model(layers, c["vocab"], dev)
        for B, T in c["cells"]:
            g = torch.Generator(device=dev).manual_seed(B + T)
            k, v = (torch.randn(B, s["Hkv"], T, s["D"], device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
            caches = {"e4m3": _filled(layers, True, k, v), "16-bit": _filled(layers, False, k, v)}
            del k, v
            tok0 = torch.randint(3, 1024, (B, 1), device=dev, generator=g)
            for head in c["heads"]:
                def run(arm):
                    sw, kind = ARMS[arm]
                    prefill.enable_fused_prefill(m, wide_decode=True, head=head, **sw, **FORMS[form])     # (outside the clock)
                    cache = caches[kind]
                    n0 = {n: dict(getattr(prefill, n)) for n in ("stack_stats", "stack_kv8_stats", "kv8_stats", "stats", "head_stats")}
                    tok = m(input_ids=tok0, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)   # (unclocked)
                    torch.cuda.synchronize()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(STEPS):
                        tok = m(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
                    t1.record()
                    torch.cuda.synchronize()
                    cache.crop(T)
                    moved = {n: getattr(prefill, n)["head" if n == "head_stats" else "decode"] - n0[n]["head" if n == "head_stats" else "decode"]
                             for n in n0}
                    calls = STEPS + 1
                    want = {"stack_stats": 0 if arm == "a" else calls, "stack_kv8_stats": calls if arm == "b" else 0,
                            "kv8_stats": 0 if arm == "c" else calls * layers, "stats": calls * layers,
                            "head_stats": calls if head and arm != "a" else 0}
                    assert moved == want, (arm, form, B, T, head, moved, want)
                    return t0.elapsed_time(t1) / STEPS

                for arm in ARMS:     # warm-up: the quantised weight copies, the code objects, the workspaces
                    run(arm)
                t = {arm: [] for arm in ARMS}
                for _ in range(a.rounds):
                    for arm in ARMS:
                        t[arm].append(run(arm))
                rows = B * s["Hkv"] * T * layers
                row = {"child": a.child, "layers": layers, "vocab": c["vocab"], "weights": form, "B": B, "T": T, "head": head, "steps": STEPS,
                       "rounds": a.rounds, "e4m3_cache_MB": round(rows * 2 * (s["D"] + 4) / 1e6, 1),
                       "16bit_cache_MB": round(rows * 2 * s["D"] * 2 / 1e6, 1)}
                for arm in ARMS:
                    row[f"{arm}_ms_per_step"] = round(statistics.median(t[arm]), 4)
                row["a_over_b"], row["a_over_b_spread"] = _ratios(t["a"], t["b"])
                row["c_over_b"], row["c_over_b_spread"] = _ratios(t["c"], t["b"])
                res.append(row)
                print(json.dumps(row), flush=True)
            del caches
            torch.cuda.empty_cache()
        prefill.disable_fused_prefill(m)
        del m
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"box": _box(), "rows": res}), flush=True)


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    late = threading.Timer(limit, p.kill)
    late.start()
    lines = []
    for ln in p.stdout:          # (a child's rows are shown as they come)
        lines.append(ln)
        if not ln.startswith("RESULT "):
            print("  " + ln, end="", flush=True)
    rc = p.wait()
    expired = not late.is_alive()
    late.cancel()
    if rc != 0:
        why = f"timed out after {limit} s" if expired else f"exit status {rc}"
        raise SystemExit(f"stack_kv8_ab: {why}: {' '.join(cmd)}\n{''.join(lines)[-3000:]} -- stopping here")
    return "".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=list(CHILDREN))
    ap.add_argument("--only", default=None, choices=list(CHILDREN), help="run this child alone")
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = [sys.executable, str(Path(__file__).resolve()), "--rounds", str(a.rounds)]
    res = {"what": "decode step on the e4m3 KV cache: a = the per-layer step (kv8=True, stack_decode=True: the route before stack_kv8), "
                   "b = the whole-stack step on the codes (stack_kv8=True), c = the whole-stack step on the 16-bit append-in-place cache "
                   "(context); one model per weight form, the switches set anew before each run, arms interleaved in one process; "
                   "synthetic weights and N(0, 1) caches; 16 greedy steps per run, medians over the rounds, spread = largest deviation "
                   "of a round's ratio from the median ratio",
           "not_measured": NOT_MEASURED, "rows": []}
    for name, c in CHILDREN.items():
        if a.only and name != a.only:
            continue
        r = _result(_run(me + ["--child", name], c["limit"]))
        res["box"] = r["box"]
        res["rows"] += r["rows"]
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
