#!/usr/bin/env python
"""The Phi-3 decoder after the path (the reference's default decoder, train_stage1.py:35; eval/mrg.py:70-75 prefills 1024
positions and decodes up to 768 tokens): a Phi-3-mini-shaped decoder (32 layers, E 3072, 32 x 96 heads, I 8192, vocab 32064,
sliding_window 2047; random bf16 weights) timed on a prefill of 1024 embeddings and 64 greedy decode steps, stock HF layers
on PyTorch-ROCm against u2tokenizer_amd.prefill (HIP layers), in one process.  Prints one JSON line.  Measurement only.

    python tools/phi3_decoder_probe.py [layers] [steps]
"""
import json
import sys
import time
from pathlib import Path

import torch
from transformers import Phi3Config, Phi3ForCausalLM
from transformers.cache_utils import DynamicCache

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from u2tokenizer_amd.prefill import disable_fused_prefill, enable_fused_prefill  # noqa: E402

layers = int(sys.argv[1]) if len(sys.argv) > 1 else 32
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 64
S = 1024
cfg = Phi3Config(vocab_size=32064, hidden_size=3072, intermediate_size=8192, num_hidden_layers=layers, num_attention_heads=32,
                 num_key_value_heads=32, max_position_embeddings=4096, sliding_window=2047, tie_word_embeddings=False,
                 pad_token_id=32000, bos_token_id=1, eos_token_id=32000)
torch.set_grad_enabled(False)
dev = torch.device("cuda", 0)
with torch.device("meta"):
    m = Phi3ForCausalLM(cfg)
m = m.to(torch.bfloat16).to_empty(device=dev).eval()
for p in m.parameters():
    p.normal_(0, 0.02)
m.model.rotary_emb.__init__(config=cfg, device=dev)  # buffers of a meta-built module are uninitialised
x = (torch.randn(1, S, 3072, device=dev) * 0.05).to(torch.bfloat16)
layer_bytes = 2 * sum(p.numel() for p in m.model.layers.parameters())


def prefill(n=5):
    for _ in range(2):
        m(inputs_embeds=x, past_key_values=DynamicCache(config=cfg), use_cache=True, logits_to_keep=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = m(inputs_embeds=x, past_key_values=DynamicCache(config=cfg), use_cache=True, logits_to_keep=1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, out.logits[:, -1].float()


def decode(n):
    """prefill, then n greedy steps (argmax -> embedding -> one position) on the cache generate() builds for this config;
    returns ms per step and the ids"""
    cache = DynamicCache(config=cfg)
    out = m(inputs_embeds=x, past_key_values=cache, use_cache=True, logits_to_keep=1)
    ids = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tok = out.logits[:, -1].argmax(-1)
        ids.append(tok)
        out = m(inputs_embeds=m.model.embed_tokens(tok)[:, None], past_key_values=cache, use_cache=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, torch.stack(ids, 1).cpu()


res = {}
for label, fused in (("stock", False), ("fused", True)):
    disable_fused_prefill(m)
    if fused:
        assert enable_fused_prefill(m) == layers
    ms, logits = prefill()
    decode(4)                                               # warm-up: workspaces, the few-rows kernels' first launches
    step_ms, ids = decode(steps)
    res[label] = (ms, logits, step_ms, ids)
d = res["fused"][1] - res["stock"][1]
agree = int((res["fused"][3] == res["stock"][3]).cumprod(1).sum())
print(json.dumps({
    "what": f"Phi-3-mini-shaped decoder ({layers} layers, E 3072, 32 x 96 heads, I 8192, W 2047, random bf16 weights): prefill "
            f"of {S} embeddings (last-position logits, as generate asks) and {steps} greedy decode steps, stock HF layers "
            "on PyTorch-ROCm against u2tokenizer_amd.prefill (HIP layers)",
    "prefill_ms_stock": round(res["stock"][0], 2), "prefill_ms": round(res["fused"][0], 2),
    "decode_ms_per_step_stock": round(res["stock"][2], 3), "decode_ms_per_step": round(res["fused"][2], 3),
    "decode_steps_timed": steps, "layer_weights_gb": round(layer_bytes / 1e9, 2),
    "decode_layer_weights_tb_s": round(layer_bytes / (res["fused"][2] * 1e-3) / 1e12, 2),
    "last_logits_rel_rms_vs_stock": round((d.pow(2).mean().sqrt() / res["stock"][1].pow(2).mean().sqrt()).item(), 5),
    "greedy_ids_equal_to_stock_for_steps": agree}))
