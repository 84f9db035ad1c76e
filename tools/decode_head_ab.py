#!/usr/bin/env python
"""A/B of the head of the decode step -- everything between the last layer and the next token id -- at the Qwen3-8B layer shape with
its vocabulary (E = 4096, V = 151 936), synthetic weights, on one GPU, interleaved in one process per case:

  head     off (the whole-stack step, then the module norm, nn.Linear and the widening to fp32: the path before the switch existed)
           | elem | fp8 | fp4 (`config.u2_fused_decode_head` with `config.u2_fused_head_form`: the final norm and lm_head in the
           whole-stack step's library call, fp32 logits)
  pick     greedy (argmax) | sampled (temperature 0.7, top-p 0.9: transformers' warpers, softmax, multinomial) | sampled+warp (the
           same with `sampling.fuse_warpers`: the one-workgroup fused warper) | sampled+split (... its split-row form for calls of
           at most sampling.SPLIT_MAX_ROWS rows)
  warp     the warpers alone, us per call: stock | one workgroup | split at 1, 2, 4, 8 rows x V in {32 064, 128 256, 151 936}
  layers   bf16 | e2m1 (fp4_decode)

A run is a fused prefill of 128 positions, one untimed step, then 64 steps: per-step ms (device events around the 64 steps) and host
ms (the time the host needs to ISSUE the 64 steps -- nothing in the loop waits for the device -- per step).  Rounds take turns over
all arms; medians over the rounds, and for every ratio its spread (largest deviation of a round's ratio from the median ratio).

    python tools/decode_head_ab.py [--rounds 5] [--out profiles/decode_head_ab.json] [--no-deep]

The parent never opens the GPU: every case is a child process of its own under its own time limit, started only if the one before it
ended clean; nothing is tried twice."""
import argparse
import json
import platform
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS, PROMPT, VOCAB = 64, 128, 151936
QWEN3_8B = dict(E=4096, I=12288, Hq=32, Hkv=8, D=128)
LAYER_FORMS = {"bf16": {}, "e2m1": dict(fp4_decode=True)}
HEADS = ("off", "elem", "fp8", "fp4")
PICKS = ("greedy", "sampled", "sampled+warp", "sampled+split")
WARP_ROWS, WARP_VOCABS, WARP_CALLS = (1, 2, 4, 8), (32064, 128256, 151936), 100
CASES = {"8 layers": dict(layers=8, batches=(1, 16)), "36 layers": dict(layers=36, batches=(1,))}


def _model(layers, dev):
    import torch
    from u2tokenizer_amd import language_model as LM
    s = QWEN3_8B
    cfg = LM.u2Qwen3Config(vocab_size=VOCAB, hidden_size=s["E"], intermediate_size=s["I"], num_hidden_layers=layers,
                           num_attention_heads=s["Hq"], num_key_value_heads=s["Hkv"], head_dim=s["D"], max_position_embeddings=4096,
                           tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    torch.manual_seed(0)
    with torch.device(dev):
        m = LM.u2Qwen3ForCausalLM(cfg)
    m = m.to(torch.bfloat16).eval()
    m.__dict__["_u2_fuse_checked"] = {False, True}   # (the switches are set below, not from the config)
    return m


def _arm(m, layer_form, head):
    from u2tokenizer_amd import prefill
    if head != "off":
        m.config.u2_fused_head_form = head
    prefill.enable_fused_prefill(m, stack_decode=True, head=head != "off", **LAYER_FORMS[layer_form])


def _pickers():
    import torch
    from transformers.generation.logits_process import LogitsProcessorList, TemperatureLogitsWarper, TopPLogitsWarper
    from u2tokenizer_amd.sampling import fuse_warpers
    stock = LogitsProcessorList([TemperatureLogitsWarper(0.7), TopPLogitsWarper(0.9)])
    fused = fuse_warpers(LogitsProcessorList([TemperatureLogitsWarper(0.7), TopPLogitsWarper(0.9)]))
    split = fuse_warpers(LogitsProcessorList([TemperatureLogitsWarper(0.7), TopPLogitsWarper(0.9)]), split=True)

    def sampled(procs):
        def pick(logits, ids):   # (what `_sample` does with a step's logits)
            scores = procs(ids, logits[:, -1].to(torch.float32))
            return torch.multinomial(torch.softmax(scores, -1), 1)
        return pick

    return {"greedy": lambda logits, ids: logits[:, -1].argmax(-1, keepdim=True), "sampled": sampled(stock),
            "sampled+warp": sampled(fused), "sampled+split": sampled(split)}


def _run_steps(m, ids, steps, pick):
    import torch
    out = m(input_ids=ids, use_cache=True)
    cache, tok = out.past_key_values, pick(out.logits, ids)
    tok = pick(m(input_ids=tok, past_key_values=cache, use_cache=True).logits, ids)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    h0 = time.perf_counter()
    for _ in range(steps):
        tok = pick(m(input_ids=tok, past_key_values=cache, use_cache=True).logits, ids)
    h1 = time.perf_counter()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps, 1e3 * (h1 - h0) / steps


def _ratios(num, den):
    r = [x / y for x, y in zip(num, den)]
    med = statistics.median(r)
    return round(med, 3), round(max(abs(x - med) for x in r), 3)


def child(a):
    import torch
    from u2tokenizer_amd import ops, prefill
    ops.device_check()
    torch.set_grad_enabled(False)
    torch.manual_seed(1)
    dev = torch.device("cuda", 0)
    case = CASES[a.case]
    models = {f: _model(case["layers"], dev) for f in LAYER_FORMS}
    picks = _pickers()
    res = []
    for B in case["batches"]:
        ids = torch.randint(3, VOCAB, (B, PROMPT), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
        arms = [(f, h, p) for f in LAYER_FORMS for h in HEADS for p in PICKS]
        for f, h, p in arms:   # warm-up: the quantised copies, the code objects, the workspaces
            _arm(models[f], f, h)
            _run_steps(models[f], ids, 4, picks[p])
        ms, host = {c: [] for c in arms}, {c: [] for c in arms}
        for _ in range(a.rounds):
            for f, h, p in arms:
                _arm(models[f], f, h)
                n0, s0 = prefill.head_stats["head"], prefill.stack_stats["decode"]
                t, hst = _run_steps(models[f], ids, STEPS, picks[p])
                assert prefill.stack_stats["decode"] - s0 == STEPS + 1, (f, h, p)
                assert prefill.head_stats["head"] - n0 == (0 if h == "off" else STEPS + 1), (f, h, p)
                ms[(f, h, p)].append(t)
                host[(f, h, p)].append(hst)
        for f in LAYER_FORMS:
            for p in PICKS:
                row = {"case": a.case, "layers": case["layers"], "B": B, "layer_form": f, "pick": p, "steps": STEPS, "rounds": a.rounds}
                for h in HEADS:
                    row[f"head_{h}_ms_per_token"] = round(statistics.median(ms[(f, h, p)]), 4)
                    row[f"head_{h}_host_ms_per_token"] = round(statistics.median(host[(f, h, p)]), 4)
                for h in HEADS[1:]:
                    row[f"off_over_{h}"], row[f"off_over_{h}_spread"] = _ratios(ms[(f, "off", p)], ms[(f, h, p)])
                res.append(row)
    for m in models.values():
        prefill.disable_fused_prefill(m)
    box = {"host": platform.node(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    print("RESULT " + json.dumps({"box": box, "rows": res}), flush=True)


def child_warp(a):
    """per-call us of the warpers alone at T 0.7, p 0.9: the stock transformers pair | the one-workgroup kernel | the split-row form,
    interleaved, WARP_CALLS back-to-back calls per timing, medians over the rounds"""
    import torch
    from u2tokenizer_amd import _lib, ops
    from transformers.generation.logits_process import LogitsProcessorList, TemperatureLogitsWarper, TopPLogitsWarper
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    stock = LogitsProcessorList([TemperatureLogitsWarper(0.7), TopPLogitsWarper(0.9)])
    arms = {"stock": lambda x: stock(None, x), "one_workgroup": lambda x: ops.sample_warp(x, 0.7, 0, 0.9, 1),
            "split": lambda x: ops.sample_warp_split(x, 0.7, 0, 0.9, 1)}
    h = _lib.load_library("bf16")
    res = []
    for V in WARP_VOCABS:
        for rows in WARP_ROWS:
            x = (3 * torch.randn(rows, V, device=dev, generator=torch.Generator(device=dev).manual_seed(rows + V))).bfloat16().float()
            us = {k: [] for k in arms}
            for r in range(a.rounds + 1):
                for k, f in arms.items():
                    torch.cuda.synchronize()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(WARP_CALLS):
                        f(x)
                    t1.record()
                    torch.cuda.synchronize()
                    if r:   # (round 0: warm-up)
                        us[k].append(1e3 * t0.elapsed_time(t1) / WARP_CALLS)
            row = {"rows": rows, "V": V, "calls": WARP_CALLS, "rounds": a.rounds,
                   "split_workgroups_per_row": min(16, -(-V // 8192)), "split_launches_per_call": h.u2tok_sample_warp_split_launches(V, 0, 0.9, 1)}
            for k in arms:
                row[k + "_us_per_call"] = round(statistics.median(us[k]), 1)
            row["one_workgroup_over_split"], row["one_workgroup_over_split_spread"] = _ratios(us["one_workgroup"], us["split"])
            row["stock_over_split"], row["stock_over_split_spread"] = _ratios(us["stock"], us["split"])
            res.append(row)
    print("RESULT " + json.dumps({"rows": res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--warp", action="store_true", help="(child) the warpers' per-call table instead of a case")
    ap.add_argument("--case", default="8 layers", choices=list(CASES))
    ap.add_argument("--no-deep", action="store_true", help="skip the 36-layer case")
    a = ap.parse_args()
    if a.child:
        return child_warp(a) if a.warp else child(a)
    me = [sys.executable, str(Path(__file__).resolve()), "--rounds", str(a.rounds), "--child"]
    res = {"what": "the head of the decode step at the Qwen3-8B layer shape, V = 151936: head off (whole-stack step, module norm, "
                   "nn.Linear, widening) | head on with lm_head in the element type / e4m3 / e2m1, x greedy / sampled (T 0.7, p 0.9, "
                   "stock warpers) / sampled with the fused one-workgroup warper, x layers in bf16 / e2m1; synthetic weights; a fused "
                   "prefill of 128 positions, then 64 steps per run, interleaved in one process per case; medians over the rounds, "
                   "spread = largest deviation of a round's ratio from the median ratio; host ms = time to issue the steps, per "
                   "token (the loop never waits for the device: `generate`'s one synchronisation per token is not in it)",
           "rows": [],
           "warp_calls": [],
           "not_measured": ["quality of a quantised lm_head on trained weights", "the f16 build's speed", "Phi-3 shapes"]}

    def run(cmd):
        print("+", " ".join(cmd), flush=True)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"decode_head_ab: timed out: {' '.join(cmd)} -- stopping here")
        if r.returncode != 0:
            raise SystemExit(f"decode_head_ab: exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}{r.stderr[-2000:]} -- stopping here")
        return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])

    res["warp_calls"] = run(me + ["--warp"])["rows"]
    print(json.dumps(res["warp_calls"]), flush=True)
    for case in CASES:
        if a.no_deep and case != "8 layers":
            res["not_measured"].append(case)
            continue
        got = run(me + ["--case", case])
        res["box"] = got["box"]
        res["rows"] += got["rows"]
        print(json.dumps(got["rows"]), flush=True)
        if a.out:   # (after every case: a later case that does not end leaves the earlier ones recorded)
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
