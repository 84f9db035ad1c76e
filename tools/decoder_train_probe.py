#!/usr/bin/env python
"""The decoder's training route (u2tokenizer_amd/decoder_train.py) against the stock HF layer: ONE decoder layer, forward +
backward, batch 1, S = 1024, at the Qwen3-8B shape (E 4096, 32 / 8 heads of 128, I 12288), the Llama-3.2-1B shape (E 2048,
32 / 8 heads of 64, I 8192) and the Phi-3-mini shape (E 3072, 32 heads of 96, I 8192, window 2047; the route's train_phi3 switch),
unpadded and right-padded to 1024 from 700 valid positions.  Stock and fused are timed as interleaved pairs in one process (stock,
fused, stock, fused, ... after a warm-up of both): medians of HIP-event times, and the median and the spread (min .. max) of the
pair differences stock - fused.  Then the causal attention backward kernel alone (u2tok_attention_gqa_bwd, or _d96) with its
TFLOP/s over the visible (causal) pairs, counted as the 5 matmul units of a flash backward.  Measurement only; nothing here is on
the product path.

    python tools/decoder_train_probe.py [reps] [--shapes phi3-mini,qwen3-8b,llama-3.2-1b] [--out result.json]
"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402
from transformers import (LlamaConfig, LlamaForCausalLM, Phi3Config, Phi3ForCausalLM, Qwen3Config,  # noqa: E402
                          Qwen3ForCausalLM)

from u2tokenizer_amd import decoder_train, ops  # noqa: E402
from u2tokenizer_amd.prefill import disable_fused_prefill, enable_fused_prefill  # noqa: E402

ARGV = sys.argv[1:]
OUT = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else None
ONLY = ARGV[ARGV.index("--shapes") + 1].split(",") if "--shapes" in ARGV else None
REPS = int(ARGV[0]) if ARGV and ARGV[0].isdigit() else 10
dev = torch.device("cuda", 0)
bf = torch.bfloat16
S, VALID = 1024, 700
SHAPES = {"qwen3-8b": (Qwen3Config, Qwen3ForCausalLM, dict(hidden_size=4096, intermediate_size=12288, num_attention_heads=32,
                                                           num_key_value_heads=8, head_dim=128)),
          "llama-3.2-1b": (LlamaConfig, LlamaForCausalLM, dict(hidden_size=2048, intermediate_size=8192, num_attention_heads=32,
                                                               num_key_value_heads=8, head_dim=64, rope_theta=500000.0)),
          "phi3-mini": (Phi3Config, Phi3ForCausalLM, dict(hidden_size=3072, intermediate_size=8192, num_attention_heads=32,
                                                          num_key_value_heads=32, sliding_window=2047, pad_token_id=0,
                                                          bos_token_id=1, eos_token_id=2))}


def median_ms(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def paired_ms(stock, fused, run, reps=REPS, warm=3):
    """stock() / fused() switch the route, run() is the step: warm both, then `reps` interleaved (stock, fused) pairs -> medians and
    the pair differences stock - fused (median, min, max)"""
    for _ in range(warm):
        stock(), run(), fused(), run()
    ts, tf = [], []
    for _ in range(reps):
        stock()
        ts.append(timed(run))
        fused()
        tf.append(timed(run))
    d = sorted(a - b for a, b in zip(ts, tf))
    med = lambda v: sorted(v)[len(v) // 2]
    return med(ts), med(tf), (d[len(d) // 2], d[0], d[-1])


def layer_model(name):
    C, M, kw = SHAPES[name]
    cfg = C(vocab_size=1024, num_hidden_layers=1, max_position_embeddings=4096, tie_word_embeddings=False, **kw)
    torch.manual_seed(0)
    with torch.device("meta"):
        m = M(cfg)
    m = m.to(bf).to_empty(device=dev)
    for p in m.parameters():
        p.data.normal_(0, 0.02)
    for layer in m.model.layers:
        for n in (layer.input_layernorm, layer.post_attention_layernorm, getattr(layer.self_attn, "q_norm", None),
                  getattr(layer.self_attn, "k_norm", None)):
            if n is not None:
                n.weight.data.fill_(1.0)
    m.model.rotary_emb.__init__(config=cfg, device=dev)
    return m.train()


def step_fn(m, x, mask, g):
    def run():
        m.zero_grad(set_to_none=False)
        xe = x.detach().requires_grad_(True)
        with torch.enable_grad():
            h = m.model(inputs_embeds=xe, attention_mask=mask, use_cache=False).last_hidden_state
            h.backward(g)
    return run


res = {"S": S, "valid_padded": VALID, "reps": REPS, "device": torch.cuda.get_device_name(0)}
for name in SHAPES:
    if ONLY is not None and name not in ONLY:
        continue
    m = layer_model(name)
    phi3 = name.startswith("phi3")
    E = m.config.hidden_size
    x = (torch.randn(1, S, E, device=dev) * 0.5).to(bf)
    g = (torch.randn(1, S, E, device=dev) * 0.01).to(bf)
    full = torch.ones(1, S, dtype=torch.int64, device=dev)
    pad = full.clone()
    pad[:, VALID:] = 0
    for tag, mask in (("unpadded", full), ("right_padded", pad)):
        n0 = decoder_train.stats["layers"]
        t_stock, t_fused, (dm, dlo, dhi) = paired_ms(lambda: disable_fused_prefill(m),
                                                     lambda: enable_fused_prefill(m, train=True, train_phi3=phi3),
                                                     step_fn(m, x, mask, g))
        assert decoder_train.stats["layers"] - n0 == REPS + 3, "the training route did not run in every fused step"
        res[f"{name}/{tag}"] = {"stock_ms": round(t_stock, 3), "fused_ms": round(t_fused, 3),
                                "speedup": round(t_stock / t_fused, 3), "pair_diff_ms": {"median": round(dm, 3),
                                                                                         "min": round(dlo, 3), "max": round(dhi, 3)}}
        print(name, tag, res[f"{name}/{tag}"], flush=True)
    disable_fused_prefill(m)
    # the attention backward kernel alone
    cfg = m.config
    Hq, Hkv, d = cfg.num_attention_heads, cfg.num_key_value_heads, m.model.layers[0].self_attn.head_dim
    qkv = (torch.randn(1, S, (Hq + 2 * Hkv) * d, device=dev)).to(bf)
    dout = torch.randn(1, S, Hq * d, device=dev).to(bf)
    for tag, lens in (("unpadded", None), ("right_padded", VALID)):
        kv = None if lens is None else torch.tensor([lens], dtype=torch.int32, device=dev)
        with torch.no_grad():
            out, lse = ops.attention_gqa_ex(qkv[..., :Hq * d], qkv[..., Hq * d:(Hq + Hkv) * d], qkv[..., (Hq + Hkv) * d:], Hq, Hkv,
                                            d ** -0.5, kv_len=kv, with_lse=True)
            ms = median_ms(lambda: ops.attention_gqa_bwd(qkv, out, dout, Hq, Hkv, d ** -0.5, kv_len=kv, lse=lse))
        n = S if lens is None else lens
        pairs = n * (n + 1) / 2 + (S - n) * n        # (pad queries see the n valid keys)
        flop = 5 * 2.0 * d * pairs * Hq
        res[f"{name}/attn_bwd/{tag}"] = {"ms": round(ms, 4), "tflops_visible": round(flop / ms / 1e9, 1)}
        print(name, "attention backward", tag, res[f"{name}/attn_bwd/{tag}"], flush=True)
    del m
    torch.cuda.empty_cache()
print(json.dumps(res))
if OUT:
    Path(OUT).parent.mkdir(parents=True, exist_ok=True)
    Path(OUT).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")
