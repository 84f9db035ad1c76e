#!/usr/bin/env python
"""A/B of the three ways to run a decode step -- the per-layer route (two library calls per layer), the whole-stack route
(stack_decode: one call per token) with its norms as launches of their own, and the whole-stack route with the norms in the tails of
the o and down products (prefill.STACK_TAIL_NORM) -- in the three weight forms, interleaved in one process per case, on one GPU, with
synthetic weights:

  steps   per case (layer shape, layer count, batch sizes) one decoder per weight form; its route is switched between runs (the
          quantised copies stay).  A run is a fused prefill of 128 positions, one untimed step, then 64 greedy steps through the
          causal LM: per-step ms (device events around the 64 steps: what `generate` pays), host ms (the time the host needs to
          ISSUE the 64 steps -- nothing in the loop waits for the device -- per step).  Rounds take turns over routes and forms;
          medians over the rounds, and for every ratio its spread (largest deviation of a round's ratio from the median ratio).
  trace   device ms: children under `rocprofv3 --kernel-trace --stats`, one per (form, route) and step count; the kernel time of
          128 steps minus that of 64 steps, per step -- what the device computes when it never waits for the host.

    python tools/stack_decode_ab.py [--rounds 5] [--out profiles/stack_decode_ab.json] [--no-trace] [--no-deep]

The parent never opens the GPU: every GPU step is a child process of its own under its own time limit, started only if the one
before it ended clean; nothing is tried twice.  Thread and job counts are left as the machine sets them."""
import argparse
import csv
import json
import platform
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS, PROMPT = 64, 128
QWEN3_8B = dict(E=4096, I=12288, Hq=32, Hkv=8, D=128)
FORMS = ("bf16", "e4m3", "e2m1")
FLAGS = {"bf16": {}, "e4m3": dict(fp8_decode=True), "e2m1": dict(fp4_decode=True)}
ROUTES = ("layers", "stack", "stack+tail")
CASES = {"8 layers": dict(layers=8, batches=(1, 16), forms=FORMS), "36 layers": dict(layers=36, batches=(1,), forms=("bf16", "e2m1"))}


def _model(layers, dev):
    import torch
    from transformers import Qwen3Config, Qwen3ForCausalLM
    s = QWEN3_8B
    cfg = Qwen3Config(vocab_size=1024, hidden_size=s["E"], intermediate_size=s["I"], num_hidden_layers=layers,
                      num_attention_heads=s["Hq"], num_key_value_heads=s["Hkv"], head_dim=s["D"], max_position_embeddings=4096,
                      tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    torch.manual_seed(0)
    with torch.device(dev):
        m = Qwen3ForCausalLM(cfg)
    return m.to(torch.bfloat16).eval()


def _route(m, form, route):
    from u2tokenizer_amd import prefill
    prefill.STACK_TAIL_NORM = route == "stack+tail"
    prefill.enable_fused_prefill(m, stack_decode=route != "layers", **FLAGS[form])


def _box():
    import torch
    return {"host": platform.node(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__}


def _ratios(num, den):
    r = [x / y for x, y in zip(num, den)]
    med = statistics.median(r)
    return round(med, 3), round(max(abs(x - med) for x in r), 3)


def _run_steps(m, ids, steps, timed=True):
    """prefill, one step, then `steps` greedy steps -> (ms per step on the device's clock, ms per step the host took to issue them)"""
    import torch
    out = m(input_ids=ids, use_cache=True)
    cache, tok = out.past_key_values, out.logits[:, -1].argmax(-1, keepdim=True)
    tok = m(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    h0 = time.perf_counter()
    for _ in range(steps):
        tok = m(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
    h1 = time.perf_counter()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps, 1e3 * (h1 - h0) / steps


def child_steps(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    case = CASES[a.case]
    models = {f: _model(case["layers"], dev) for f in case["forms"]}
    res = []
    for B in case["batches"]:
        ids = torch.randint(3, 1024, (B, PROMPT), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
        combos = [(f, r) for f in case["forms"] for r in ROUTES]
        for f, r in combos:   # warm-up: the quantised copies, the code objects, the workspaces
            _route(models[f], f, r)
            _run_steps(models[f], ids, 4)
        ms, host = {c: [] for c in combos}, {c: [] for c in combos}
        for _ in range(a.rounds):
            for f, r in combos:
                _route(models[f], f, r)
                n0 = prefill.stack_stats["decode"]
                t, h = _run_steps(models[f], ids, STEPS)
                assert prefill.stack_stats["decode"] - n0 == (0 if r == "layers" else STEPS + 1), (f, r)
                ms[(f, r)].append(t)
                host[(f, r)].append(h)
        for f in case["forms"]:
            row = {"case": a.case, "layers": case["layers"], "B": B, "form": f, "steps": STEPS, "rounds": a.rounds}
            for r in ROUTES:
                row[r + "_ms_per_step"] = round(statistics.median(ms[(f, r)]), 4)
                row[r + "_host_ms_per_step"] = round(statistics.median(host[(f, r)]), 4)
            row["layers_over_stack"], row["layers_over_stack_spread"] = _ratios(ms[(f, "layers")], ms[(f, "stack")])
            row["stack_over_tail"], row["stack_over_tail_spread"] = _ratios(ms[(f, "stack")], ms[(f, "stack+tail")])
            res.append(row)
        for r in ROUTES:      # does the step follow its weight bytes?
            row = {"case": a.case, "layers": case["layers"], "B": B, "route": r}
            fs = case["forms"]
            for x, y in zip(fs, fs[1:]):
                row[f"{x}_over_{y}"], row[f"{x}_over_{y}_spread"] = _ratios(ms[(x, r)], ms[(y, r)])
            res.append(row)
    for m in models.values():
        prefill.disable_fused_prefill(m)
    print("RESULT " + json.dumps({"box": _box(), "rows": res}), flush=True)


def child_trace(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    m = _model(8, dev)
    _route(m, a.form, a.route)
    ids = torch.randint(3, 1024, (1, PROMPT), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    _run_steps(m, ids, a.steps)
    prefill.disable_fused_prefill(m)


def _kernel_ns(d):
    files = sorted(Path(d).rglob("*kernel_stats.csv"))
    if not files:
        raise SystemExit("stack_decode_ab: rocprofv3 wrote no kernel_stats.csv -- stopping here")
    return sum(float(r["TotalDurationNs"]) for r in csv.DictReader(files[0].open()))


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"stack_decode_ab: timed out after {limit} s: {' '.join(cmd)} -- stopping here")
    if r.returncode != 0:
        raise SystemExit(f"stack_decode_ab: exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}{r.stderr[-2000:]} -- stopping here")
    return r.stdout


def _result(stdout):
    return json.loads(next(ln for ln in stdout.splitlines() if ln.startswith("RESULT "))[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["steps", "trace"])
    ap.add_argument("--case", default="8 layers", choices=list(CASES))
    ap.add_argument("--form", default="bf16", choices=FORMS)
    ap.add_argument("--route", default="layers", choices=ROUTES)
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 children (device ms)")
    ap.add_argument("--no-deep", action="store_true", help="skip the 36-layer case")
    a = ap.parse_args()
    if a.child:
        return {"steps": child_steps, "trace": child_trace}[a.child](a)
    me = [sys.executable, str(Path(__file__).resolve()), "--rounds", str(a.rounds)]
    res = {"what": "decode step of a decoder at the Qwen3-8B layer shape: per-layer route | whole-stack route | whole-stack route "
                   "with tail norms, x 16-bit / e4m3 / e2m1 weights, interleaved in one process per case; synthetic weights; a "
                   "fused prefill of 128 positions, then 64 greedy steps per run; medians over the rounds, spread = largest "
                   "deviation of a round's ratio from the median ratio; host ms = time to issue the steps, per step",
           "steps": [], "not_measured": []}
    for case in CASES:
        if a.no_deep and case != "8 layers":
            res["not_measured"].append(case)
            continue
        r = _result(_run(me + ["--child", "steps", "--case", case], 500))
        res["box"] = r["box"]
        res["steps"] += r["rows"]
        print(json.dumps(r["rows"]), flush=True)
    prof = shutil.which("rocprofv3")
    if a.no_trace or prof is None:
        res["not_measured"].append("device ms (kernel time per step): " + ("rocprofv3 not found" if prof is None else "--no-trace"))
    else:
        res["device_ms_per_step"] = []
        for form in ("bf16", "e2m1"):
            for route in ROUTES:
                ns = []
                for steps in (STEPS, 2 * STEPS):
                    d = tempfile.mkdtemp(prefix="stack_decode_trace_")
                    _run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me +
                         ["--child", "trace", "--form", form, "--route", route, "--steps", str(steps)], 300)
                    ns.append(_kernel_ns(d))
                    shutil.rmtree(d, ignore_errors=True)
                row = {"layers": 8, "B": 1, "form": form, "route": route, "kernel_ms_per_step": round((ns[1] - ns[0]) / STEPS / 1e6, 4)}
                res["device_ms_per_step"].append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
