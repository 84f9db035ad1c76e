#!/usr/bin/env python
"""A/B of the loss head alone on one GPU: forward + backward of lm_head + cross-entropy from given hidden states, the stock
expression (F.cross_entropy((h W^T).float(), labels): what transformers' ForCausalLMLoss runs) against
u2tokenizer_amd.loss_head.linear_cross_entropy, interleaved in one process (stock, new, stock, new, ...), with the peak memory of
each above the inputs (the two gradients a call leaves behind count); then the two row kernels' achieved bytes/s, on one reused
block of logits (cache-resident, as in the head) and on rotating blocks (from HBM), next to the 8 TB/s HBM figure.

    python tools/loss_head_ab.py [--rows 1024 4096 8192] [--ignored 0 0.6] [--hidden 4096] [--vocab 151936] [--reps 7]
                                 [--out profiles/loss_head_ab.json]

Times are device-event times of whole forward + backward calls (ms; min and median of the timed repeats after two warm-up calls
of each side).  Needs the GPU: there is nothing to measure without one."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8.0e12


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _peak(fn, drop):
    """Peak bytes allocated during fn() above what is held once drop() has released the previous call's results: everything fn
    allocates counts, the two gradients it leaves behind included."""
    drop()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def head_ab(rows, ignored, E, V, reps, dev):
    from u2tokenizer_amd import loss_head
    g = torch.Generator(device=dev).manual_seed(rows + int(ignored * 100))
    h = torch.randn((rows, E), device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    w = (torch.randn((V, E), device=dev, generator=g) * (3.0 / E ** 0.5)).to(torch.bfloat16).requires_grad_(True)
    labels = torch.randint(0, V, (rows,), device=dev, generator=g)
    if ignored > 0:
        labels[torch.rand(rows, device=dev, generator=g) < ignored] = -100

    def drop():
        h.grad = w.grad = None

    def stock():
        drop()
        F.cross_entropy((h @ w.t()).float(), labels, ignore_index=-100).backward()

    def new():
        drop()
        loss_head.linear_cross_entropy(h, w, labels, shift=False).backward()

    for _ in range(2):
        stock(), new()
    torch.cuda.synchronize()
    ts, tn = [], []
    for _ in range(reps):
        ts.append(_timed(stock))
        tn.append(_timed(new))
    mem_s, mem_n = _peak(stock, drop), _peak(new, drop)
    stock()
    ls, gs = F.cross_entropy((h @ w.t()).float(), labels, ignore_index=-100).item(), (h.grad.clone(), w.grad.clone())
    new()
    ln = loss_head.linear_cross_entropy(h, w, labels, shift=False).item()
    rel = [((a.float() - b.float()).norm() / b.float().norm()).item() for a, b in zip((h.grad, w.grad), gs)]
    labelled = int((labels != -100).sum())
    return {"rows": rows, "ignored_share": ignored, "labelled_rows": labelled, "slices": len(loss_head.plan_slices(max(labelled, 1), V)),
            "stock_ms_min": round(min(ts), 3), "stock_ms_median": round(statistics.median(ts), 3),
            "new_ms_min": round(min(tn), 3), "new_ms_median": round(statistics.median(tn), 3),
            "new_over_stock_median": round(statistics.median(tn) / statistics.median(ts), 3),
            "gradients_mib": round((rows * E + V * E) * 2 / 2 ** 20),
            "stock_peak_mib": round(mem_s / 2 ** 20), "new_peak_mib": round(mem_n / 2 ** 20),
            "loss_stock": ls, "loss_new": ln, "dh_rel_diff": rel[0], "dW_rel_diff": rel[1]}


def kernels_bw(rows, Vs, iters, dev, nblocks=8):
    """The two row kernels on (rows, Vs) blocks of logits, timed with device events around a loop of launches (not per-kernel
    profiler times), two ways: "one_block_reused" -- every launch on the same block (<= 256 MiB: it can stay in the 256 MiB
    last-level cache between launches, which is also the head's own situation, where the GEMM has just written Z) -- and
    "rotating_blocks" -- the launches cycle through `nblocks` distinct blocks (over 1 GiB together), so every pass comes from HBM."""
    from u2tokenizer_amd import ops
    g = torch.Generator(device=dev).manual_seed(7)
    blocks = [(torch.randn((rows, Vs), device=dev, generator=g) * 4).to(torch.bfloat16) for _ in range(nblocks)]
    labels = torch.randint(0, Vs, (rows,), device=dev, generator=g)
    m, l, zt = torch.full((rows,), float("-inf"), device=dev), torch.zeros(rows, device=dev), torch.zeros(rows, device=dev)
    lse = torch.logsumexp(blocks[0].float(), -1) + 1.0
    coef = torch.full((rows,), 1.0 / rows, device=dev)
    assert iters % nblocks == 0 and nblocks * rows * Vs * 2 > (1 << 30)

    def lse_loop(k):
        for i in range(iters):
            ops.ce_lse_update(blocks[i % k], 0, labels, m, l, zt)

    def grad_loop(k):   # (in place: later passes read gradients instead of logits -- the same bytes move)
        for i in range(iters):
            ops.ce_grad_inplace(blocks[i % k], 0, labels, lse, coef)

    out = {"rows": rows, "Vs": Vs, "block_mib": round(rows * Vs * 2 / 2 ** 20), "blocks": nblocks, "launches_per_timing": iters,
           "timing": "device events around the loop of launches, best of 3 loops"}
    for name, fn, bytes_per in (("ce_lse_update", lse_loop, rows * Vs * 2.0), ("ce_grad_inplace", grad_loop, rows * Vs * 4.0)):
        out[name] = {}
        for mode, k in (("one_block_reused", 1), ("rotating_blocks", nblocks)):
            fn(k)
            ms = min(_timed(lambda: fn(k)) for _ in range(3)) / iters
            out[name][mode] = {"us": round(ms * 1e3, 1), "tb_per_s": round(bytes_per / (ms * 1e-3) / 1e12, 3),
                               "over_8_tb_per_s": round(bytes_per / (ms * 1e-3) / HBM_BYTES_PER_S, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096, 8192])
    ap.add_argument("--ignored", type=float, nargs="+", default=[0.0, 0.6])
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_head_ab: needs the GPU (no CPU measurement stands in for it)")
    from u2tokenizer_amd import ops
    ops.device_check()
    dev = torch.device("cuda", 0)
    res = {"what": "forward + backward of lm_head + cross-entropy alone, stock torch expression vs u2tokenizer_amd.loss_head, interleaved "
                   "in one process; device-event ms; peak MiB allocated above the inputs, the two gradients the call returns "
                   "(gradients_mib) included",
           "hidden": a.hidden, "vocab": a.vocab, "reps": a.reps, "device": torch.cuda.get_device_name(0), "head": [], "kernels": []}
    for rows in a.rows:
        for ig in a.ignored:
            r = head_ab(rows, ig, a.hidden, a.vocab, a.reps, dev)
            print(json.dumps(r), flush=True)
            res["head"].append(r)
    for rows, Vs in ((1024, 76032), (8192, 15360)):
        r = kernels_bw(rows, Vs, 24, dev)
        print(json.dumps(r), flush=True)
        res["kernels"].append(r)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
