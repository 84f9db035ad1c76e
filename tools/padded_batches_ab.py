#!/usr/bin/env python
"""A/B of the padded-batch routes (enable_fused_prefill(model, padded=True)) on one GPU, interleaved in one process:

  decode   one decode step of a left-padded batch (B = 8, cache ~1100 positions, pads up to 300) at the Qwen3-8B layer width,
           through the padded decode route against the same call with the switch off (the stock HF layers: what such a batch
           took before the switch existed); both sides step on their own cache, pair by pair
  kernel   u2tok_decode_attention (kv_start = NULL) against the per-sequence loop of u2tok_decoder_decode_post -- one
           u2tok_attention_gqa_split call per sequence, as decoder.hip issues them -- at B = 1 / 4 / 8 / 16, T = 1100 / 1792,
           d = 128, 8 kv heads of 4 query heads; and the two whole second halves of the step (u2tok_decoder_decode_post with
           batched = 0 against batched = 1), which differ in nothing else
  prefill  a B = 4, S = 1024 left-padded prefill through the range kernel against the stock layers, with the share of 64-key
           tiles the kernel skips

    python tools/padded_batches_ab.py [--layers 4] [--reps 9] [--out profiles/padded_batches_ab.json]

Times are device-event times in ms of whole calls (host time of the call included, as a `generate` step pays it); every figure
is the median over the interleaved repeats, "spread" the largest deviation of a pair's difference from the median difference.
The decoder has --layers layers (36 in Qwen3-8B): per-step times scale with the layer count, the ratio does not.  Needs the GPU."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
bf = torch.bfloat16


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _pairs(fa, fb, reps, warm=2):
    """Interleaved (a, b) timings -> medians, and the run-to-run spread of the pair differences."""
    for _ in range(warm):
        fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(_timed(fa))
        tb.append(_timed(fb))
    diff = [x - y for x, y in zip(ta, tb)]
    md = statistics.median(diff)
    return {"a_ms": round(statistics.median(ta), 4), "b_ms": round(statistics.median(tb), 4), "a_minus_b_ms": round(md, 4),
            "spread_ms": round(max(abs(x - md) for x in diff), 4), "pairs": reps}


def _model(layers, dev):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config(vocab_size=1024, hidden_size=4096, intermediate_size=12288, num_hidden_layers=layers, num_attention_heads=32,
                      num_key_value_heads=8, head_dim=128, max_position_embeddings=4096, tie_word_embeddings=False,
                      pad_token_id=0, bos_token_id=1, eos_token_id=2)
    torch.manual_seed(0)
    with torch.device(dev):
        m = Qwen3ForCausalLM(cfg)
    return m.to(bf).eval()


def _left_mask(B, S, pads, dev):
    m = torch.ones(B, S, dtype=torch.int64, device=dev)
    for b, p in enumerate(pads):
        m[b, :p] = 0
    return m


def decode_ab(m, reps, dev):
    from u2tokenizer_amd import prefill
    B, S, pads = 8, 1100, (0, 40, 80, 120, 160, 200, 250, 300)
    E = m.config.hidden_size
    g = torch.Generator(device=dev).manual_seed(1)
    x = (0.5 * torch.randn((B, S, E), device=dev, generator=g)).to(bf)
    x1 = (0.5 * torch.randn((B, 1, E), device=dev, generator=g)).to(bf)
    state = {}
    for padded in (False, True):
        prefill.enable_fused_prefill(m, padded=padded)
        state[padded] = [m(inputs_embeds=x, attention_mask=_left_mask(B, S, pads, dev), use_cache=True).past_key_values, S]

    def step(padded):
        def run():
            prefill.enable_fused_prefill(m, padded=padded)       # (sets the switches only: the layers stay patched)
            cache, T = state[padded]
            m(inputs_embeds=x1, attention_mask=_left_mask(B, T + 1, pads, dev), past_key_values=cache, use_cache=True)
            state[padded][1] = T + 1
        return run

    n0 = dict(prefill.stats)
    r = _pairs(step(False), step(True), reps)
    taken = prefill.stats["padded_decode"] - n0["padded_decode"]
    prefill.disable_fused_prefill(m)
    assert taken == (reps + 2) * len(m.model.layers), taken
    return {"what": "one decode step, left-padded batch: a = switch off (stock layers), b = padded=True", "B": B,
            "cache_positions": f"{S}..{state[True][1]}", "pads": pads, "layers": len(m.model.layers), **r,
            "stock_over_padded": round(r["a_ms"] / r["b_ms"], 2)}


def prefill_ab(m, reps, dev):
    from u2tokenizer_amd import prefill
    B, S, pads = 4, 1024, (0, 100, 400, 700)
    E = m.config.hidden_size
    g = torch.Generator(device=dev).manual_seed(2)
    x = (0.5 * torch.randn((B, S, E), device=dev, generator=g)).to(bf)
    mask = _left_mask(B, S, pads, dev)

    def run(padded):
        def f():
            prefill.enable_fused_prefill(m, padded=padded)
            m(inputs_embeds=x, attention_mask=mask, use_cache=True)
        return f

    r = _pairs(run(False), run(True), reps)
    prefill.disable_fused_prefill(m)
    total = sum(qb + 1 for _ in pads for qb in range(S // 64))                      # causal 64-key tiles per head
    skipped = sum(min(p // 64, qb + 1) for p in pads for qb in range(S // 64))
    return {"what": "left-padded prefill: a = switch off (stock layers), b = padded=True (range kernel)", "B": B, "S": S, "pads": pads,
            "layers": len(m.model.layers), **r, "stock_over_padded": round(r["a_ms"] / r["b_ms"], 2),
            "key_tiles_per_head": total, "key_tiles_skipped": skipped, "skipped_share": round(skipped / total, 3)}


def kernel_ab(B, T, reps, dev, iters=20):
    from u2tokenizer_amd import ops
    Hq, Hkv, d = 32, 8, 128
    g = torch.Generator(device=dev).manual_seed(B + T)
    rn = lambda *s, k=1.0: (k * torch.randn(s, device=dev, generator=g)).to(bf)  # noqa: E731
    qkv, K, V = rn(B, (Hq + 2 * Hkv) * d), rn(B, Hkv, T, d), rn(B, Hkv, T, d)
    out = torch.empty((B, Hq * d), dtype=bf, device=dev)
    scale = d ** -0.5
    with ops.on_device(qkv) as (h, stream):
        return _kernel_ab(h, stream, B, T, reps, dev, iters, rn, qkv, K, V, out, scale)


def _kernel_ab(h, stream, B, T, reps, dev, iters, rn, qkv, K, V, out, scale):
    from u2tokenizer_amd import _lib
    Hq, Hkv, d, E, inter = 32, 8, 128, 4096, 12288
    ws_new = torch.empty(max(h.u2tok_decode_attention_workspace_bytes(B, Hq, Hkv, T, d), 16), dtype=torch.uint8, device=dev)
    ws_old = torch.empty(max(h.u2tok_tok_attention_workspace_bytes(Hkv, Hq // Hkv, 1, T, d), 16), dtype=torch.uint8, device=dev)
    nq, gq = qkv.shape[1], Hq // Hkv

    def new():
        for _ in range(iters):
            _lib.check(h.u2tok_decode_attention(qkv.data_ptr(), K.data_ptr(), V.data_ptr(), out.data_ptr(), B, Hq, Hkv, T, d, nq,
                                                T * d, Hq * d, scale, None, ws_new.data_ptr(), ws_new.numel(), stream), "new")

    def old():   # decoder.hip's loop: entries of one sequence = its kv heads, the group's query heads as the heads
        es = 2
        for _ in range(iters):
            for b in range(B):
                _lib.check(h.u2tok_attention_gqa_split(qkv.data_ptr() + b * nq * es, K.data_ptr() + b * Hkv * T * d * es,
                                                       V.data_ptr() + b * Hkv * T * d * es, out.data_ptr() + b * Hq * d * es,
                                                       Hkv, 1, T, gq, 1, d, gq * d, d, d, gq * d, gq * d, T * d, T * d, gq * d, scale,
                                                       ws_old.data_ptr(), ws_old.numel(), stream), "old")

    old()
    ref = out.clone()
    new()
    agree = (out.float() - ref.float()).abs().max().item()
    r = _pairs(old, new, reps)
    # the two whole second halves of the step
    cfg = _lib.DecodeConfig(B=B, E=E, Hq=Hq, Hkv=Hkv, D=d, I=inter, eps=1e-6, qk_eps=1e-6, scale=scale)
    ws = torch.empty(h.u2tok_decoder_decode_workspace_bytes(C.byref(cfg), T), dtype=torch.uint8, device=dev)
    x, y = rn(B, E), torch.empty((B, E), dtype=bf, device=dev)
    Wo, wn, Wgu, Wd = rn(E, Hq * d, k=0.02), rn(E).add_(1), rn(2 * inter, E, k=0.02), rn(E, inter, k=0.02)
    lay = _lib.DecodeLayer(Wo=Wo.data_ptr(), w_post_norm=wn.data_ptr(), Wgu=Wgu.data_ptr(), Wdown=Wd.data_ptr())

    def post(batched):
        def run():
            for _ in range(iters):
                _lib.check(h.u2tok_decoder_decode_post(C.byref(cfg), C.byref(lay), x.data_ptr(), qkv.data_ptr(), K.data_ptr(),
                                                       V.data_ptr(), T, 0, batched, None, y.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       stream), "u2tok_decoder_decode_post")
        return run

    rp = _pairs(post(0), post(1), reps)
    us = lambda v: round(v * 1e3 / iters, 2)  # noqa: E731
    return {"B": B, "T": T, "attention_loop_us": us(r["a_ms"]), "attention_batched_us": us(r["b_ms"]), "attention_spread_us": us(r["spread_ms"]),
            "loop_over_batched": round(r["a_ms"] / r["b_ms"], 2), "max_abs_diff": agree,
            "post_loop_us": us(rp["a_ms"]), "post_batched_us": us(rp["b_ms"]), "post_spread_us": us(rp["spread_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("padded_batches_ab: needs the GPU (no CPU measurement stands in for it)")
    from u2tokenizer_amd import ops
    ops.device_check()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    res = {"what": "padded-batch routes, interleaved A/B in one process; device-event ms of whole calls, medians; spread = largest "
                   "deviation of a pair's difference from the median difference", "device": torch.cuda.get_device_name(0), "kernel": []}
    for T in (1100, 1792):
        for B in (1, 4, 8, 16):
            r = kernel_ab(B, T, a.reps, dev)
            print(json.dumps(r), flush=True)
            res["kernel"].append(r)
    m = _model(a.layers, dev)
    res["decode"] = decode_ab(m, a.reps, dev)
    print(json.dumps(res["decode"]), flush=True)
    res["prefill"] = prefill_ab(m, a.reps, dev)
    print(json.dumps(res["prefill"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
