#!/usr/bin/env python
"""A/B of the loss head's statistics pass on one GPU (sibling of tools/loss_head_ab.py):

  * u2tok_ce_stats_update against u2tok_ce_lse_update on the same rows x vocab block of logits, walked in the planner's slices,
    interleaved in one process (plain, all statistics, argmax alone, logit sum alone, lse2 alone, plain, ...): device-event time
    of one whole pass over the block, min and median of the repeats;
  * the peak memory of one evaluation step (no grad, labels given) of a small Qwen3-shaped causal LM at the full vocabulary:
    the stock head (logits come back, the driver takes their argmax) against `u2_fused_loss_head` +
    `u2_fused_loss_head_predictions` (the (B, S) predictions come back).

    python tools/loss_stats_ab.py [--rows 1024] [--vocab 151936] [--reps 15] [--seq 1024] [--out profiles/loss_stats_ab.json]

Needs the GPU: there is nothing to measure without one."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FLAVOURS = {"plain (ce_lse_update)": None, "all statistics": ("amax", "zsum", "l2"), "argmax alone": ("amax",),
            "logit sum alone": ("zsum",), "lse2 alone": ("l2",)}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def kernel_ab(rows, V, reps, dev):
    from u2tokenizer_amd import loss_head, ops
    g = torch.Generator(device=dev).manual_seed(7)
    plan = loss_head.plan_slices(rows, V)
    blocks = [(torch.randn((rows, vs), device=dev, generator=g) * 4).to(torch.bfloat16) for _, vs in plan]
    labels = torch.randint(0, V, (rows,), device=dev, generator=g)
    f32 = lambda v: torch.full((rows,), v, device=dev)
    m, l, zt = f32(float("-inf")), f32(0.0), f32(0.0)
    extra = {"amax": f32(float("-inf")), "aidx": torch.full((rows,), (1 << 63) - 1, dtype=torch.int64, device=dev), "zsum": f32(0.0),
             "l2": f32(0.0)}

    def one_pass(want):
        if want is None:
            for (v0, _), z in zip(plan, blocks):
                ops.ce_lse_update(z, v0, labels, m, l, zt)
        else:
            kw = {k: extra[k] for k in want}
            if "amax" in kw:
                kw["aidx"] = extra["aidx"]
            for (v0, _), z in zip(plan, blocks):
                ops.ce_stats_update(z, v0, labels, m, l, zt, **kw)

    for want in FLAVOURS.values():
        one_pass(want), one_pass(want)
    torch.cuda.synchronize()
    times = {k: [] for k in FLAVOURS}
    for _ in range(reps):
        for name, want in FLAVOURS.items():
            times[name].append(_timed(lambda: one_pass(want)) * 1e3)
    nbytes = rows * V * 2.0
    out = {"rows": rows, "vocab": V, "slices": plan, "block_mib": round(nbytes / 2 ** 20), "reps": reps,
           "timing": "device events around one pass over all slices (us), flavours interleaved", "flavours": {}}
    base = statistics.median(times["plain (ce_lse_update)"])
    for name, ts in times.items():
        med = statistics.median(ts)
        out["flavours"][name] = {"us_min": round(min(ts), 1), "us_median": round(med, 1), "over_plain_median": round(med / base, 3),
                                 "tb_per_s_median": round(nbytes / (med * 1e-6) / 1e12, 3)}
    return out


def eval_peak(S, V, dev, hidden=1024, layers=2):
    from u2tokenizer_amd import language_model as LM, loss_head, synth

    def model(**switches):
        cfg = LM.u2Qwen3Config(vocab_size=V, hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=layers,
                               num_attention_heads=hidden // 128, num_key_value_heads=hidden // 256, head_dim=128,
                               max_position_embeddings=max(S, 512), tie_word_embeddings=False, pad_token_id=0, bos_token_id=1,
                               eos_token_id=2)
        for k, v in switches.items():
            setattr(cfg, k, v)
        m = LM.u2Qwen3ForCausalLM(cfg)
        synth.fill_module_(m, seed=17, prefix="decoder.")
        return m.to(torch.bfloat16).to(dev).eval()

    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, V, (1, S), generator=g).to(dev)
    labels = ids.clone()
    labels[:, :S // 4] = -100

    def step(m):
        with torch.no_grad():
            out = m(input_ids=ids, labels=labels)
            pred = loss_head.predictions_for_metrics(out.logits, labels)
        return out.loss.item(), pred

    res = {"what": "peak MiB allocated during one evaluation step (no grad; loss + predictions_for_metrics) above what the model and "
                   "the batch hold", "batch": 1, "positions": S, "labelled": int((labels[:, 1:] != -100).sum()), "vocab": V,
           "hidden": hidden, "layers": layers, "logits_bf16_mib": round(S * V * 2 / 2 ** 20)}
    preds = {}
    for name, sw in (("stock_head", {}), ("loss_head_predictions", dict(u2_fused_loss_head=True, u2_fused_loss_head_predictions=True))):
        m = model(**sw)
        step(m)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss, preds[name] = step(m)
        torch.cuda.synchronize()
        res[name] = {"peak_mib": round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1), "loss": loss}
        del m
        torch.cuda.empty_cache()
    on = labels[:, 1:] != -100
    res["predictions_agree_share"] = round((preds["stock_head"][:, :-1][on] == preds["loss_head_predictions"][:, :-1][on])
                                           .double().mean().item(), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_stats_ab: needs the GPU (no CPU measurement stands in for it)")
    from u2tokenizer_amd import ops
    ops.device_check()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernel_ab(a.rows, a.vocab, a.reps, dev)}
    print(json.dumps(res["kernel"]), flush=True)
    res["evaluation_step"] = eval_peak(a.seq, a.vocab, dev)
    print(json.dumps(res["evaluation_step"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
