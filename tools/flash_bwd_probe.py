#!/usr/bin/env python
"""The flash attention backward (the kernel pair of attn_bwd.hip), every instantiation, microseconds per call:

  * the ViT's (d = 64, no mask, equal heads) at one layer of the benchmark shape (8 chunks x 2049 tokens x 12 heads), with the
    forward's row statistics and rebuilding them, against the unfused chain (probabilities rebuilt in HBM): agreement and the
    matrix-pipe rate of the fused pair (8 matmul units of 2 S^2 64 flop per head);
  * the decoder's (causal, grouped-query heads) at S = 1024, batch 1: a Qwen3-8B-like shape (32 / 8 heads of 128) and a
    Llama-3.2-1B-like one (32 / 8 heads of 64), as tools/decoder_train_probe.py, with and without the statistics; TFLOP/s over
    the visible pairs, counted as the 5 matmul units of a flash backward.

    python tools/flash_bwd_probe.py [nb S H]          (nb S H: the ViT shape)
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from u2tokenizer_amd import autograd as AG  # noqa: E402
from u2tokenizer_amd import ops  # noqa: E402

DECODER_S = 1024
DECODER_SHAPES = {"qwen3-8b": (32, 8, 128), "llama-3.2-1b": (32, 8, 64)}   # query heads, kv heads, head dim


def vit_case(dev, nb, S, H):
    """-> {name: call} of the ViT instantiations, and the unfused chain."""
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(nb, S, 3 * H * 64, device=dev, generator=g).to(torch.bfloat16)
    dO = torch.randn(nb, S, H * 64, device=dev, generator=g).to(torch.bfloat16)
    out, lse = ops.flash_attention_d64(qkv, H, 0.125, extra_last=S > 1, return_lse=True)
    E = H * 64

    def unfused():
        q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
        P = AG._attn_probs(q, k, H, 0.125, None, 0)
        d = torch.empty_like(qkv)
        AG._attn_backward(q, k, v, P, dO, H, 0.125, d[..., :E], d[..., E:2 * E], d[..., 2 * E:], None, 0)
        return d

    return {"vit/lse": lambda: ops.flash_attention_d64_bwd(qkv, out, dO, H, 0.125, lse=lse),
            "vit/own_stats": lambda: ops.flash_attention_d64_bwd(qkv, out, dO, H, 0.125)}, unfused


def decoder_cases(dev, S=DECODER_S):
    """-> {name: call} of the causal instantiations."""
    calls = {}
    for name, (Hq, Hkv, d) in DECODER_SHAPES.items():
        g = torch.Generator(device=dev).manual_seed(1)
        qkv = torch.randn(1, S, (Hq + 2 * Hkv) * d, device=dev, generator=g).to(torch.bfloat16)
        dO = torch.randn(1, S, Hq * d, device=dev, generator=g).to(torch.bfloat16)
        with torch.no_grad():
            out, lse = ops.attention_gqa_ex(qkv[..., :Hq * d], qkv[..., Hq * d:(Hq + Hkv) * d], qkv[..., (Hq + Hkv) * d:], Hq, Hkv,
                                            d ** -0.5, with_lse=True)
        calls[f"{name}/lse"] = lambda a=(qkv, out, dO, Hq, Hkv, d ** -0.5), s=lse: ops.attention_gqa_bwd(*a, lse=s)
        calls[f"{name}/own_stats"] = lambda a=(qkv, out, dO, Hq, Hkv, d ** -0.5): ops.attention_gqa_bwd(*a)
    return calls


def timeit(fn, n=5):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3, r


def main():
    nb, S, H = (int(x) for x in sys.argv[1:4]) if len(sys.argv) > 3 else (8, 2049, 12)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ops.device_check()
    AG.ensure_gemm_scratch(dev)
    vit, unfused = vit_case(dev, nb, S, H)
    tf, df = timeit(vit["vit/lse"])
    ts, _ = timeit(vit["vit/own_stats"])
    tu, du = timeit(unfused)
    unit = 2.0 * nb * H * S * S * 64
    print(f"attention backward nb={nb} S={S} H={H}: fused with the forward's row statistics {tf:.1f} us ({7 * unit / tf / 1e6:.0f} "
          f"TF/s over its 7 matmul units), rebuilding them {ts:.1f} us ({8 * unit / ts / 1e6:.0f} TF/s over 8), unfused chain "
          f"{tu:.1f} us, x{tu / tf:.2f}")
    E = H * 64
    for i, n in enumerate(("dq", "dk", "dv")):
        a, b = df[..., i * E:(i + 1) * E].float(), du[..., i * E:(i + 1) * E].float()
        print(f"  {n}: rel rms fused vs unfused {((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item():.3e}, "
              f"rms {b.pow(2).mean().sqrt().item():.3e}")
    for name, fn in decoder_cases(dev).items():
        Hq, _, d = DECODER_SHAPES[name.split("/")[0]]
        t, _ = timeit(fn, n=20)
        flop = 5 * 2.0 * d * (DECODER_S * (DECODER_S + 1) / 2) * Hq
        print(f"causal attention backward {name} S={DECODER_S}: {t:.1f} us ({flop / t / 1e6:.1f} TF/s over the visible pairs)")


if __name__ == "__main__":
    main()
