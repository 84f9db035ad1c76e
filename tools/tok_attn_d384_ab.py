#!/usr/bin/env python
"""A/B of the tokenizer's attention at head dim 384 (E = 3072, 8 heads): the fused kernels (tok_attn_kernel<384>,
temporal_attention_kernel<6>) against the GEMM -> softmax -> GEMM chain that width took before it had them (what option
tok_flash = 0 still runs), on one GPU, one process per part:

  launches  interleaved pairs on the same bf16 tensors (q / k / v as column slices of packed buffers): a = the chain through the
            pipeline's building blocks (batched scores GEMM into fp32, softmax_rows, batched P V GEMM reading V in place),
            b = the fused launch; us per call (device events around `--calls` calls, host time of the calls included), medians
            over the pairs, "spread" = the largest deviation of a pair's difference from the median difference.  Shapes:
            SVR spatial attention (8, 256, 256, 8) with the relative bias, TTA visual cross attention (1, 256, 1792, 8), and
            the chunk-axis attention at T = 8, N = 256 (chain: the N positions x 8 heads as the batch of 8-row products).
  forward   one whole tokenizer forward at the configuration-2 sizes (batch 4, 4 chunks of 64 tokens, 4 layers, DiffTS 1024, DMTP,
            256 queries, text 1024) with E = 3072 and random weights: option tok_flash = 0 against 1, interleaved pairs; ms.
  pmc       `--child pmc --d D`: 20 fused launches of the spatial shape at head dim D, for a counter pass of their own
            (rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -- python tools/tok_attn_d384_ab.py --child pmc --d 384);
            `--pmc-summary DIR` then prints the counters per dispatch of the attention kernel from the csv files under DIR.

    python tools/tok_attn_d384_ab.py [--pairs 7] [--calls 30] [--out profiles/tok_attn_d384_ab.json]

The parent process never opens the GPU: each part is a child process under its own time limit, started only if the one before it
ended clean; nothing is tried twice."""
import argparse
import json
import math
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
E, H = 3072, 8
D = "cuda"


def _pairs(run_a, run_b, pairs):
    ta, tb = [], []
    for _ in range(pairs):
        ta.append(run_a())
        tb.append(run_b())
    diff = [x - y for x, y in zip(ta, tb)]
    md = statistics.median(diff)
    return statistics.median(ta), statistics.median(tb), md, max(abs(x - md) for x in diff)


def _timed(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def _chain(ops, q, k, v, heads, scale, tbl):
    """attention_core's unfused form on (nb, S, E) views: fp32 scores in HBM, softmax_rows, P V with V read in place"""
    import torch
    nb, Sq, Eq = q.shape
    d, Skv = Eq // heads, k.shape[1]
    s = torch.empty((nb * heads, Sq, Skv), dtype=torch.float32, device=q.device)
    ops.gemm_strided(q, k, s, M=Sq, N=Skv, K=d, lda=q.stride(1), ldb=k.stride(1), ldc=Skv, nz=nb * heads, nbh=heads, sAb=q.stride(0),
                     sAh=d, sBb=k.stride(0), sBh=d, sCb=heads * Sq * Skv, sCh=Sq * Skv, out_f32=True)
    p = ops.softmax_rows(s, scale, tbl, heads, 512)
    o = torch.empty((nb, Sq, Eq), dtype=q.dtype, device=q.device)
    ops.gemm_strided(p, v, o, M=Sq, N=d, K=Skv, lda=Skv, ldb=v.stride(1), ldc=Eq, nz=nb * heads, nbh=heads, sAb=heads * Sq * Skv,
                     sAh=Sq * Skv, sBb=v.stride(0), sBh=d, sCb=Sq * Eq, sCh=d, b_kmajor=True)
    return o


def child_launches(a):
    import torch
    from u2tokenizer_amd import ops
    ops.device_check()
    torch.set_grad_enabled(False)
    bf = torch.bfloat16
    g = torch.Generator(device=D).manual_seed(0)
    d = E // H
    scale = 1 / math.sqrt(d)
    tbl = (0.2 * torch.randn((1023, H), device=D, generator=g)).to(bf)
    res = []

    def measure(name, shape, chain, fused, flops):
        ref, got = chain().float(), fused().float()
        err = (got - ref).abs().max().item()
        for fn in (chain, fused):
            _timed(fn, a.calls)                   # warm-up
        sa, sb, md, spread = _pairs(lambda: _timed(chain, a.calls) * 1e3, lambda: _timed(fused, a.calls) * 1e3, a.pairs)
        res.append({"launch": name, "shape": shape, "pairs": a.pairs, "calls": a.calls, "chain_us": round(sa, 2), "fused_us": round(sb, 2),
                    "chain_minus_fused_us": round(md, 2), "spread_us": round(spread, 2), "chain_over_fused": round(sa / sb, 2),
                    "fused_tflops": round(flops / sb / 1e6, 1), "max_abs_fused_minus_chain": err,
                    "fused_not_slower_within_spread": bool(md >= -spread)})
        print(json.dumps(res[-1]), flush=True)

    # SVR spatial attention: 8 chunks x 256 tokens, relative bias, q | k | v packed
    qkv = torch.randn((8, 256, 3 * E), device=D, generator=g).to(bf)
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    measure("svr_spatial", [8, 256, 256, H], lambda: _chain(ops, q, k, v, H, scale, tbl),
            lambda: ops.tok_attention(q, k, v, H, scale, tbl, 512, 0), 4.0 * 8 * H * 256 * 256 * d)
    # TTA visual cross attention: 256 queries over 1024 + 512 + 256 visual tokens, k | v packed
    q2 = torch.randn((1, 256, E), device=D, generator=g).to(bf)
    kv = torch.randn((1, 1792, 2 * E), device=D, generator=g).to(bf)
    k2, v2 = kv[..., :E], kv[..., E:]
    measure("tta_visual_cross", [1, 256, 1792, H], lambda: _chain(ops, q2, k2, v2, H, scale, None),
            lambda: ops.tok_attention(q2, k2, v2, H, scale, None, 512, 0), 4.0 * 1 * H * 256 * 1792 * d)
    # chunk-axis attention: rows in (b t n) order, sequences of T = 8 rows that are N rows apart
    T, N = 8, 256
    rows = torch.randn((T * N, 3 * E), device=D, generator=g).to(bf)
    seq = rows.view(T, N, 3 * E).permute(1, 0, 2)            # (N, T, 3E): batch = token position, as chunk_axis_attention's chain
    q3, k3, v3 = seq[..., :E], seq[..., E:2 * E], seq[..., 2 * E:]

    def fused3():
        return ops.temporal_attention(rows[:, :E], rows[:, E:2 * E], rows[:, 2 * E:], 1, T, N, H, scale, tbl, 512)

    def chain3():
        return _chain(ops, q3, k3, v3, H, scale, tbl)

    ref = chain3().float().permute(1, 0, 2).reshape(T * N, E)
    assert (fused3().float() - ref).abs().max().item() < 0.05
    measure("chunk_axis_T8", [1, T, N, H], lambda: chain3().permute(1, 0, 2), lambda: fused3().view(T, N, E), 4.0 * N * H * T * T * d)
    print("RESULT " + json.dumps(res), flush=True)


def child_forward(a):
    import torch
    from u2tokenizer_amd import ops
    from u2tokenizer_amd.tokenizer import u2Tokenizer
    ops.device_check()
    torch.set_grad_enabled(False)
    bf = torch.bfloat16
    B, T, N, Lt = 4, 4, 64, 1024
    with torch.device("meta"):
        tok = u2Tokenizer(E, H, 4, 1024, True, 256, E, "rma", True, True)
    tok = tok.to(bf).to_empty(device=D)
    g = torch.Generator(device=D).manual_seed(1)
    for name, p in tok.state_dict().items():
        if p.is_floating_point():
            x = torch.randn(p.shape, device=D, generator=g)
            p.copy_((x / math.sqrt(p.shape[-1]) if p.dim() == 2 else 0.02 * x).to(bf))
    v = torch.randn((B, T, N, E), device=D, generator=g).to(bf)
    t = (0.25 * torch.randn((B, Lt, E), device=D, generator=g)).to(bf)

    def run(flash):
        ops.set_option("tok_flash", flash)
        try:
            return _timed(lambda: tok(v_token=v, t_token=t), a.calls)
        finally:
            ops.set_option("tok_flash", 1)

    for flash in (0, 1):
        run(flash)
    sa, sb, md, spread = _pairs(lambda: run(0), lambda: run(1), a.pairs)
    res = {"B": B, "chunks": T, "tokens_per_chunk": N, "text": Lt, "layers": 4, "E": E, "pairs": a.pairs, "calls": a.calls,
           "chain_ms": round(sa, 4), "fused_ms": round(sb, 4), "chain_minus_fused_ms": round(md, 4), "spread_ms": round(spread, 4)}
    print("RESULT " + json.dumps(res), flush=True)


def child_pmc(a):
    import torch
    from u2tokenizer_amd import ops
    ops.device_check()
    torch.set_grad_enabled(False)
    bf = torch.bfloat16
    g = torch.Generator(device=D).manual_seed(0)
    Ed = H * a.d
    qkv = torch.randn((8, 256, 3 * Ed), device=D, generator=g).to(bf)
    tbl = (0.2 * torch.randn((1023, H), device=D, generator=g)).to(bf)
    ops.set_option("tok_wide", a.wide)
    for _ in range(20):
        ops.tok_attention(qkv[..., :Ed], qkv[..., Ed:2 * Ed], qkv[..., 2 * Ed:], H, 1 / math.sqrt(a.d), tbl, 512, 0)
    torch.cuda.synchronize()


def pmc_summary(root):
    import collections
    import csv
    acc = collections.defaultdict(lambda: collections.defaultdict(lambda: [0.0, 0]))
    for f in Path(root).rglob("*counter_collection.csv"):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name", "")
            if "tok_attn" in name and "combine" not in name:
                c = acc[name.split("(")[0]][r["Counter_Name"]]
                c[0] += float(r["Counter_Value"])
                c[1] += 1
    out = {}
    for k, ctr in acc.items():
        e = {n: round(s / max(c, 1), 1) for n, (s, c) in ctr.items()}
        e["dispatches"] = max(c for _, c in ctr.values())
        if e.get("SQ_LDS_IDX_ACTIVE"):
            e["conflict_share"] = round(e.get("SQ_LDS_BANK_CONFLICT", 0.0) / e["SQ_LDS_IDX_ACTIVE"], 5)
        out[k] = e
    print(json.dumps(out, indent=1))
    return out


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"tok_attn_d384_ab: timed out after {limit} s: {' '.join(cmd)} -- stopping here")
    if r.returncode != 0:
        raise SystemExit(f"tok_attn_d384_ab: exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}{r.stderr[-2000:]} -- stopping here")
    return r.stdout


def _result(stdout):
    return json.loads(next(ln for ln in stdout.splitlines() if ln.startswith("RESULT "))[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["launches", "forward", "pmc"])
    ap.add_argument("--d", type=int, default=384, help="pmc: head dim of the spatial launch")
    ap.add_argument("--wide", type=int, default=2, help="pmc: option tok_wide (0: the 4-wave form at 256 / 512 too)")
    ap.add_argument("--pmc-summary", default=None, metavar="DIR")
    ap.add_argument("--no-forward", action="store_true", help="skip the whole-forward part")
    a = ap.parse_args()
    if a.pmc_summary:
        return pmc_summary(a.pmc_summary)
    if a.child:
        return {"launches": child_launches, "forward": child_forward, "pmc": child_pmc}[a.child](a)
    me = [sys.executable, str(Path(__file__).resolve()), "--pairs", str(a.pairs), "--calls", str(a.calls)]
    res = {"what": "tokenizer attention at head dim 384 (E = 3072, 8 heads), bf16: the fused kernels against the GEMM -> softmax -> GEMM "
                   "chain on the same tensors; interleaved pairs; us per call with the host time of the calls; spread = largest deviation "
                   "of a pair's difference from the median difference.  forward: one tokenizer forward at the configuration-2 sizes "
                   "with E = 3072, option tok_flash 0 against 1"}
    res["launches"] = _result(_run(me + ["--child", "launches"], 300))
    print(json.dumps(res["launches"]), flush=True)
    if a.no_forward:
        res["forward"] = {"skipped": "--no-forward"}
    else:
        res["forward"] = _result(_run(me + ["--child", "forward"], 300))
    print(json.dumps(res["forward"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
