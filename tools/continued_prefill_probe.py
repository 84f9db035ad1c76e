#!/usr/bin/env python
"""The continued prefill (`enable_fused_prefill(model, continued=True)`) against the stock HF layers, in one process on one
GPU: pairs of (stock, fused) calls interleaved, medians reported.  Measurement only; nothing here is on the product path.

  (a) Qwen3-8B-shaped layers (E 4096, 32 / 8 heads of 128): 64 and 512 new positions onto a 1024-position cache
  (b) Phi-3-mini-shaped layers (E 3072, 32 x 96, W 2047): a 3072-position prefill (longer than the window)
  (c) Qwen3-8B-shaped layers: a 6-row verification step onto a 2048-position cache, and a sweep over the rows of such a step

Every timed call gets a fresh cache, filled (untimed) by the route under test: the stock layers leave DynamicLayers, the HIP
layers their append-in-place layers.  Times are wall clock around one synchronised forward of the decoder stack (host launch
overhead included: it is what a few-row call mostly costs).

    python tools/continued_prefill_probe.py [layers] [pairs] [out.json]
"""
import json
import statistics
import sys
import time
from pathlib import Path

import torch
from transformers import Phi3Config, Phi3ForCausalLM, Qwen3Config, Qwen3ForCausalLM
from transformers.cache_utils import DynamicCache

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from u2tokenizer_amd import prefill  # noqa: E402

layers = int(sys.argv[1]) if len(sys.argv) > 1 else 4
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 7
out_path = Path(sys.argv[3]) if len(sys.argv) > 3 else Path(__file__).resolve().parents[1] / "profiles" / "continued_prefill.json"
torch.set_grad_enabled(False)
dev = torch.device("cuda", 0)


def build(kind):
    if kind == "qwen3":
        cfg = Qwen3Config(vocab_size=1024, hidden_size=4096, intermediate_size=12288, num_hidden_layers=layers,
                          num_attention_heads=32, num_key_value_heads=8, head_dim=128, max_position_embeddings=8192,
                          tie_word_embeddings=False)
        cls = Qwen3ForCausalLM
    else:
        cfg = Phi3Config(vocab_size=1024, hidden_size=3072, intermediate_size=8192, num_hidden_layers=layers,
                         num_attention_heads=32, num_key_value_heads=32, max_position_embeddings=8192, sliding_window=2047,
                         tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2)
        cls = Phi3ForCausalLM
    with torch.device("meta"):
        m = cls(cfg)
    m = m.to(torch.bfloat16).to_empty(device=dev)
    for p in m.parameters():
        p.normal_(0, 0.02)
    m.model.rotary_emb.__init__(config=cfg, device=dev)  # buffers of a meta-built module are uninitialised
    return m.eval()


def one_call(m, fused, T0, S, E):
    """Wall time (ms) of S new positions against a cache of T0 (0: no earlier call) through the decoder stack."""
    if fused:
        prefill.enable_fused_prefill(m, continued=True)
    else:
        prefill.disable_fused_prefill(m)
    cache = DynamicCache(config=m.config)
    if T0:
        m.model(inputs_embeds=(torch.randn(1, T0, E, device=dev) * 0.05).to(torch.bfloat16), past_key_values=cache, use_cache=True)
    x = (torch.randn(1, S, E, device=dev) * 0.05).to(torch.bfloat16)
    n0 = prefill.extend_stats["extend"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.model(inputs_embeds=x, past_key_values=cache, use_cache=True)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    assert (prefill.extend_stats["extend"] - n0 == layers) == bool(fused), "the fused call did not take the continued route"
    return ms


def case(m, name, T0, S, E, n=pairs):
    for _ in range(2):
        one_call(m, False, T0, S, E), one_call(m, True, T0, S, E)
    st, fu = [], []
    for _ in range(n):
        st.append(one_call(m, False, T0, S, E))
        fu.append(one_call(m, True, T0, S, E))
    r = {"case": name, "cached": T0, "new": S, "layers": layers, "pairs": n, "stock_ms": round(statistics.median(st), 3),
         "fused_ms": round(statistics.median(fu), 3), "stock_ms_all": [round(v, 3) for v in st],
         "fused_ms_all": [round(v, 3) for v in fu]}
    r["stock_over_fused"] = round(r["stock_ms"] / r["fused_ms"], 3)
    print(json.dumps({k: r[k] for k in ("case", "cached", "new", "stock_ms", "fused_ms", "stock_over_fused")}), flush=True)
    return r


results = []
m = build("qwen3")
results.append(case(m, "a: Qwen3-8B shape, 64 new onto 1024", 1024, 64, 4096))
results.append(case(m, "a: Qwen3-8B shape, 512 new onto 1024", 1024, 512, 4096))
results.append(case(m, "c: Qwen3-8B shape, 6-row verification onto 2048", 2048, 6, 4096))
for rows in (2, 4, 8, 16, 17, 32):
    results.append(case(m, f"c sweep: {rows} rows onto 2048", 2048, rows, 4096, n=5))
del m
torch.cuda.empty_cache()
m = build("phi3")
results.append(case(m, "b: Phi-3-mini shape, 3072-position prefill, W 2047", 0, 3072, 3072))
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps({"what": "continued prefill, HIP layers against stock HF layers, decoder stack only, bf16, batch 1, "
                                        "wall ms per call (medians of interleaved pairs)",
                                "device": torch.cuda.get_device_name(0), "results": results}, indent=1) + "\n")
print("written", out_path)
