#!/usr/bin/env python
"""A/B of the HOST side of the decoder routes (u2tokenizer_amd/prefill.py) between two checkouts of this repository that share one
build of the library: ms per step of the fused decode step and the fused prefill with the host time of the calls included, at the
Qwen3-8B layer shape with synthetic weights, and the microseconds `route` plus admission cost per layer call.

    python tools/decoder_routes_ab.py --a DIR_A --b DIR_B [--yardstick AA.json] [--out profiles/decoder_routes_ab.json]
                                      [--pairs 3] [--rounds 3] [--layers 4] [--host-only]

Cells: decode B = 1 and B = 8 at T = 1024 on append-in-place caches; B = 8 left-padded (padded); B = 1 fp8_decode; B = 32
wide_decode; B = 1 lora (r = 16 on all seven projections); B = 1 fp4_decode; B = 32 fp4_decode + wide_decode; B = 1 and B = 8
stack_decode (the whole-stack step: one library call per token); on an FP8 KV cache (`Kv8Layer`s of T positions) B = 1 kv8, B = 8
kv8 left-padded and B = 1 stack_kv8; B = 1 head (the whole-stack step with the head, through `prefill.head_forward`); a continued
prefill of 16 positions against 1024 cached on codes (kv8_continued; the cache is cropped back after every call); prefill B = 1,
S = 1024; and `route_us`, which needs no GPU: a patched
layer's forward on the decode route with `_decode_step` replaced by a stub, on the CPU with a tensor that reports `is_cuda`
(--host-only runs this cell alone and opens no GPU anywhere).

One child process per tree in alternation -- A, B, A, B, ... (--pairs of them) --, each under its own time limit, the next one
started only if the last ended clean; the parent never opens the GPU and nothing is tried twice.  A child imports the package of
ITS tree, builds --layers layers and times, per cell, --rounds rounds of 16 steps after one warm-up round (device events around
the 16 calls: the host time between launches counts, as `generate` pays it); its figure per cell is the median round.

Per cell: median over the pairs of (B - A), and "spread" = the largest deviation of a pair's difference from that median.  The
yardstick is the same run with the parent tree on both sides (--b DIR_A): a cell passes when B is faster, or when |median(B - A)|
is at most the larger of the yardstick's |median difference| and its spread -- the box's own noise on one tree.  Exit status 1
when a cell fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

STEPS, E, INTER, HQ, HKV, HD, T = 16, 4096, 12288, 32, 8, 128, 1024
# cell -> (batch, enable_fused_prefill keywords, left-padded, adapters[, "kv8": the cache holds codes | "head": the step with the head])
DECODE_CELLS = {
    "decode_b1": (1, {}, False, False),
    "decode_b8": (8, {}, False, False),
    "decode_b8_left_padded": (8, dict(padded=True), True, False),
    "decode_b1_fp8": (1, dict(fp8_decode=True), False, False),
    "decode_b32_wide": (32, dict(wide_decode=True), False, False),
    "decode_b1_lora": (1, dict(lora=True), False, True),
    "decode_b1_fp4": (1, dict(fp4_decode=True), False, False),
    "decode_b32_wide_fp4": (32, dict(fp4_decode=True, wide_decode=True), False, False),
    "decode_b1_stack": (1, dict(stack_decode=True), False, False),
    "decode_b8_stack": (8, dict(stack_decode=True), False, False),
    "decode_b1_kv8": (1, dict(kv8=True), False, False, "kv8"),
    "decode_b8_kv8_left_padded": (8, dict(kv8=True, padded=True), True, False, "kv8"),
    "decode_b1_stack_kv8": (1, dict(stack_kv8=True), False, False, "kv8"),
    "decode_b1_stack_head": (1, dict(head=True), False, False, "head"),
}
EXTEND_CELL, EXTEND_S = "extend_b1_s16_kv8", 16
GPU_CELLS = list(DECODE_CELLS) + [EXTEND_CELL, "prefill_b1_s1024"]
HOST_CELL = "route_us"


# ----------------------------------------------------------------------------------------------------------------------- the child
def _route_us(calls=3000):
    """microseconds per call of a patched layer's forward on the decode route, the step itself stubbed: `route` and admission"""
    import torch
    from transformers import Qwen3Config, Qwen3ForCausalLM
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd import prefill

    class FakeCuda(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    bf = torch.bfloat16
    torch.manual_seed(0)
    m = Qwen3ForCausalLM(Qwen3Config(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                                     num_key_value_heads=1, head_dim=64, max_position_embeddings=256)).to(bf).eval()
    prefill.enable_fused_prefill(m)
    real, prefill._decode_step = prefill._decode_step, lambda layer, x, pe, cache, window=None, pr=None: x
    try:
        layer = m.model.layers[0]
        cache = DynamicCache(config=m.config)
        kv = torch.zeros(2, 1, 5, 64, dtype=bf)
        cache.update(kv, kv, 0)
        x = torch.zeros(2, 1, 128, dtype=bf).as_subclass(FakeCuda)
        kw = dict(attention_mask=None, position_embeddings=(torch.ones(2, 1, 64, dtype=bf), torch.zeros(2, 1, 64, dtype=bf)),
                  past_key_values=cache)
        n0 = prefill.stats["decode"]
        rounds = []
        with torch.no_grad():
            for _ in range(6):
                t0 = time.perf_counter()
                for _ in range(calls):
                    layer(x, **kw)
                rounds.append((time.perf_counter() - t0) / calls * 1e6)
        assert prefill.stats["decode"] - n0 == 6 * calls, "the calls did not take the decode route"
    finally:
        prefill._decode_step = real
        prefill.disable_fused_prefill(m)
    return statistics.median(rounds[1:])


def child(a):
    out = {HOST_CELL: _route_us()}
    if a.host_only:
        print("RESULT " + json.dumps(out), flush=True)
        return
    import torch
    from transformers import Qwen3Config, Qwen3ForCausalLM
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd import ops, prefill
    from u2tokenizer_amd.lora import add_lora, merge_lora
    ops.device_check()
    torch.set_grad_enabled(False)
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    cfg = Qwen3Config(vocab_size=1024, hidden_size=E, intermediate_size=INTER, num_hidden_layers=a.layers, num_attention_heads=HQ,
                      num_key_value_heads=HKV, head_dim=HD, max_position_embeddings=4096, tie_word_embeddings=False,
                      pad_token_id=0, bos_token_id=1, eos_token_id=2)
    torch.manual_seed(0)
    with torch.device(dev):
        m = Qwen3ForCausalLM(cfg)
    m = m.to(bf).eval()
    like = torch.empty(1, dtype=bf, device=dev)

    def timed(call):
        """one round outside the clock, then a.rounds rounds of STEPS calls -> the median ms per call"""
        ms = []
        for r in range(a.rounds + 1):
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(STEPS):
                call(r * STEPS + i)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1) / STEPS)
        return statistics.median(ms[1:])

    def codes_cache(B):
        """`Kv8Layer`s holding T positions of noise"""
        cache = prefill.kv8_cache(a.layers)
        for lay in cache.layers:
            lay.update(torch.randn(B, HKV, T, HD, device=dev, dtype=bf), torch.randn(B, HKV, T, HD, device=dev, dtype=bf))
        return cache

    for cell, (B, flags, padded, adapters, *kind) in DECODE_CELLS.items():
        kind = kind[0] if kind else None
        if adapters:
            add_lora(m, r=16, alpha=32, dropout=0.0)
        prefill.enable_fused_prefill(m, **flags)
        if kind == "kv8":
            cache = codes_cache(B)
        else:
            cache = DynamicCache(config=m.config)   # the append-in-place layers a fused prefill of T positions leaves, filled with noise
            for li in range(a.layers):
                lay = prefill._prefill_append_layer(cache, li, B, HKV, T, HD, like)
                assert lay is not None, "this transformers' DynamicCache does not take the append-in-place layer"
                lay._kb.normal_()
                lay._vb.normal_()
                lay._commit(T)
        x = torch.randn(B, 1, E, device=dev, dtype=bf, generator=torch.Generator(device=dev).manual_seed(B))
        n = (a.rounds + 1) * STEPS
        masks = None
        if padded:   # (built outside the clock: sequence b has 3 b pads)
            full = (torch.arange(T + n, device=dev)[None, :] >= 3 * torch.arange(B, device=dev)[:, None]).long()
            masks = [full[:, :T + i + 1].contiguous() for i in range(n)]
        whole = bool(flags.get("stack_decode") or flags.get("stack_kv8") or flags.get("head"))
        s0, k0, q0, h0 = dict(prefill.stats), prefill.stack_stats["decode"], dict(prefill.kv8_stats), prefill.head_stats["head"]
        if kind == "head":   # (the causal LM's route, asked for as `_u2CausalLMMixin.forward` asks)
            out[cell] = timed(lambda i: prefill.head_forward(m, None, None, None, cache, x, True, None, {}).logits)
        else:
            out[cell] = timed(lambda i: m.model(inputs_embeds=x, past_key_values=cache, use_cache=True,
                                                **({} if masks is None else {"attention_mask": masks[i]})))
        key = "padded_decode" if padded else "decode"
        assert prefill.stats[key] - s0[key] == n * a.layers, (cell, "the steps did not take the fused route")
        assert prefill.stack_stats["decode"] - k0 == (n if whole else 0), (cell, "whole-stack steps")
        assert prefill.kv8_stats[key] - q0[key] == (n * a.layers if kind == "kv8" else 0), (cell, "steps on codes")
        assert prefill.head_stats["head"] - h0 == (n if kind == "head" else 0), (cell, "steps with the head")
        prefill.disable_fused_prefill(m)
        if adapters:
            merge_lora(m)   # (B is zero: the weights are what they were)
        del cache
    prefill.enable_fused_prefill(m, kv8_continued=True)
    cache = codes_cache(1)
    xe = torch.randn(1, EXTEND_S, E, device=dev, dtype=bf, generator=torch.Generator(device=dev).manual_seed(5))
    s0 = prefill.kv8_extend_stats["extend"]

    def extend(i):
        m.model(inputs_embeds=xe, past_key_values=cache, use_cache=True)
        cache.crop(T)   # (back to T cached positions: a length, nothing is copied)

    out[EXTEND_CELL] = timed(extend)
    assert prefill.kv8_extend_stats["extend"] - s0 == (a.rounds + 1) * STEPS * a.layers, (EXTEND_CELL, "the calls did not attend over the codes")
    prefill.disable_fused_prefill(m)
    del cache
    prefill.enable_fused_prefill(m)
    xs = torch.randn(1, 1024, E, device=dev, dtype=bf, generator=torch.Generator(device=dev).manual_seed(7))
    s0 = prefill.stats["prefill"]
    out["prefill_b1_s1024"] = timed(lambda i: m.model(inputs_embeds=xs, use_cache=False))
    assert prefill.stats["prefill"] - s0 == (a.rounds + 1) * STEPS * a.layers
    prefill.disable_fused_prefill(m)
    print("RESULT " + json.dumps(out), flush=True)


# ---------------------------------------------------------------------------------------------------------------------- the parent
def _run(tree, args, limit, script=None):
    """one child on `tree` under its own time limit; -> its figures, or SystemExit (nothing further is started)"""
    cmd = [sys.executable, str(Path(script or __file__).resolve()), "--child"] + args
    env = dict(os.environ, PYTHONPATH=str(tree))
    print("+", tree, flush=True)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=str(tree), env=env)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"decoder_routes_ab: timed out after {limit} s on {tree} -- stopping here")
    if r.returncode != 0:
        raise SystemExit(f"decoder_routes_ab: exit status {r.returncode} on {tree}\n{r.stdout[-2000:]}{r.stderr[-3000:]} -- stopping here")
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])


def run_pairs(trees, args, pairs, limit, script=None):
    """{"a": [figures per child], "b": [...]}: one child of `script` (this file by default) per tree in alternation -- a, b, a, b, ..."""
    runs = {"a": [], "b": []}
    for _ in range(pairs):
        for side in ("a", "b"):
            runs[side].append(_run(trees[side], args, limit, script))
    return runs


def compare(runs, yard, unit_of):
    """-> ({cell: row}, [cells slower beyond the yardstick's margin]).  Per cell: median over the pairs of (b - a) and its spread; with
    a yardstick (the "cells" of the same run with tree a on both sides) the margin and whether the cell passes."""
    cells, failed = {}, []
    for cell in runs["a"][0]:
        va, vb = [r[cell] for r in runs["a"]], [r[cell] for r in runs["b"]]
        diff = [y - x for x, y in zip(va, vb)]
        md = statistics.median(diff)
        row = {"unit": unit_of(cell), "a": [round(v, 4) for v in va], "b": [round(v, 4) for v in vb],
               "a_median": round(statistics.median(va), 4), "b_median": round(statistics.median(vb), 4),
               "median_b_minus_a": round(md, 4), "spread": round(max(abs(x - md) for x in diff), 4)}
        if yard is not None and cell in yard:
            row["margin"] = max(abs(yard[cell]["median_b_minus_a"]), yard[cell]["spread"])
            row["passes"] = bool(md <= 0 or abs(md) <= row["margin"])
            if not row["passes"]:
                failed.append(cell)
        cells[cell] = row
        print(cell, json.dumps(row), flush=True)
    return cells, failed


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--a")
    ap.add_argument("--b")
    ap.add_argument("--yardstick", default=None, help="the JSON of the same run with --b DIR_A")
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.a or not a.b:
        ap.error("--a and --b are required")
    trees = {"a": Path(a.a).resolve(), "b": Path(a.b).resolve()}
    args = ["--rounds", str(a.rounds), "--layers", str(a.layers)] + (["--host-only"] if a.host_only else [])
    runs = run_pairs(trees, args, a.pairs, a.limit)
    yard = json.loads(Path(a.yardstick).read_text())["cells"] if a.yardstick else None
    cells, failed = compare(runs, yard, lambda cell: "us per call" if cell == HOST_CELL else "ms per step")
    res = {"what": "host side of the decoder routes, tree b against tree a on one build of the library: ms per step (host time of the "
                   "calls included) of 16-step rounds at the Qwen3-8B layer shape, us per call for route_us; one child per tree in "
                   "alternation; margin = the larger of |median difference| and spread of the yardstick run (tree a on both sides)",
           "a": str(a.a), "b": str(a.b), "same_tree": trees["a"] == trees["b"], "pairs": a.pairs, "rounds": a.rounds, "layers": a.layers,
           "steps": STEPS, "T": T, "cells": cells}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    if failed:
        print("slower beyond the yardstick's margin:", failed, flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
