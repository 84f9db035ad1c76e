"""Sampling warpers of `generate` on one HIP launch (opt-in: `config.u2_fused_sampling`, default False).

Every sampling caller of the reference passes `do_sample=True, top_p=0.9, temperature=...` (the demo drivers, the three `generate`
calls of dpo_u2trainer.py:71-103); transformers turns that into TemperatureLogitsWarper -> [TopKLogitsWarper] -> TopPLogitsWarper: per
generated token a full sort of the vocabulary row, a softmax, a cumsum, a scatter and two masked fills.  `FusedSamplingWarper` stands
in for that run of the processor list and calls ops.sample_warp (csrc/sample.hip: a radix descent to the nucleus boundary, no sort).
The random draw stays torch.multinomial on the filtered scores, so the torch RNG stream is consumed exactly as before.

What it computes is what the stock warpers compute, with ONE rule made definite: among EQUAL logits straddling the nucleus boundary the
ones with the HIGHER INDEX are kept (the order of a stable ascending sort).  Stock transformers keeps the same NUMBER of them, but
which ones follows torch.sort's unstable order and is arbitrary.  Tokens whose cumulative mass lies within rounding of 1 - top_p may
also fall on the other side than under the stock fp32 cumsum (the kernel sums integer masses at 2^-40).
"""
from __future__ import annotations

import math

import torch
from transformers.generation.logits_process import (LogitsProcessor, LogitsProcessorList, TemperatureLogitsWarper, TopKLogitsWarper,
                                                    TopPLogitsWarper)

stats = {"fused": 0, "stock": 0, "split": 0}   # calls of FusedSamplingWarper per branch (as prefill.stats counts the decoder's routes);
#                                                  "split": the fused calls (counted there as well) that took the split-row form
# `config.u2_fused_sampling_split` (default False; read only with `u2_fused_sampling`): calls of at most SPLIT_MAX_ROWS rows go to
# ops.sample_warp_split -- a row over G = min(16, ceil(V / 8192)) workgroups, one launch per pass, the same bits.  Measured
# (profiles/decode_head_ab.json; us per call at T 0.7, p 0.9, one workgroup | split): V = 151 936: 327 | 71 at 1 row,
# 330 | 72 at 8 rows; V = 32 064: 79 | 60 at 1 row, 79 | 63 at 8.  The split form wins at every measured row count, so the crossover
# lies above 8 rows, the largest count measured: that is the constant.
SPLIT_MAX_ROWS = 8


class FusedSamplingWarper(LogitsProcessor):
    """temperature -> top-k -> top-p as one processor.  `stock`: the warpers it replaces, in order; they are applied instead
    whenever the scores are not what the kernel takes (fp32, on the GPU, 2-D, at least two columns)."""

    def __init__(self, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, min_tokens_to_keep: int = 1, stock=(),
                 split: bool = False):
        if not temperature > 0 or top_k < 0 or not 0 < top_p <= 1 or min_tokens_to_keep < 1:
            raise ValueError(f"FusedSamplingWarper: temperature {temperature}, top_k {top_k}, top_p {top_p}, "
                             f"min_tokens_to_keep {min_tokens_to_keep}")
        self.temperature = float(temperature)
        self.top_k = int(top_k)
        self.top_p = float(top_p)
        self.min_tokens_to_keep = int(min_tokens_to_keep)
        self.stock = list(stock)
        self.split = bool(split)

    def __call__(self, input_ids: torch.LongTensor, scores: torch.FloatTensor) -> torch.FloatTensor:
        if scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.shape[1] >= 2 and scores.shape[0] >= 1:
            from . import ops
            stats["fused"] += 1
            if scores.stride(1) != 1:
                scores = scores.contiguous()
            if self.split and scores.shape[0] <= SPLIT_MAX_ROWS:
                stats["split"] += 1
                return ops.sample_warp_split(scores, self.temperature, self.top_k, self.top_p, self.min_tokens_to_keep)
            return ops.sample_warp(scores, self.temperature, self.top_k, self.top_p, self.min_tokens_to_keep)
        stats["stock"] += 1
        for p in self.stock:
            scores = p(input_ids, scores)
        return scores

    def __repr__(self):
        return (f"FusedSamplingWarper(temperature={self.temperature}, top_k={self.top_k}, top_p={self.top_p}, "
                f"min_tokens_to_keep={self.min_tokens_to_keep})")


_KINDS = (TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper)


def fuse_warpers(processors, split: bool = False) -> LogitsProcessorList:
    """The processor list with its run [TemperatureLogitsWarper]? [TopKLogitsWarper]? [TopPLogitsWarper]? replaced by one
    FusedSamplingWarper; every other object stays, by identity and in place.  The run is taken only when it is the whole story: the
    list's temperature / top-k / top-p warpers (subclasses counted) are adjacent, in that order, at most one of each, each EXACTLY the
    stock class (a subclass may compute anything) filtering to -inf, with at least one of top-k / top-p.  Anything else -- another
    order, a subclass, another filter value, a processor in between, a lone temperature -- gets the list back as it is."""
    procs = list(processors)
    same = processors if isinstance(processors, LogitsProcessorList) else LogitsProcessorList(procs)
    at = [i for i, p in enumerate(procs) if isinstance(p, _KINDS)]
    run = [procs[i] for i in at]
    kinds = [type(p) for p in run]
    if not at or at != list(range(at[0], at[0] + len(at))) or any(k not in _KINDS for k in kinds) \
            or kinds != [k for k in _KINDS if k in kinds]:
        return same
    filters = [p for p in run if not isinstance(p, TemperatureLogitsWarper)]
    if not filters or any(p.filter_value != -math.inf for p in filters):
        return same
    topk = next((p for p in run if type(p) is TopKLogitsWarper), None)
    topp = next((p for p in run if type(p) is TopPLogitsWarper), None)
    min_keep = filters[0].min_tokens_to_keep
    # (TopPLogitsWarper accepts top_p = 0, "keep min_tokens_to_keep", and 1, which still drops exact zeros: left to it; two different floors are not one rule either)
    if (topp is not None and not 0 < topp.top_p < 1) or any(p.min_tokens_to_keep != min_keep for p in filters):
        return same
    temp = run[0].temperature if type(run[0]) is TemperatureLogitsWarper else 1.0
    # TopKLogitsWarper stores max(top_k, min_tokens_to_keep) as its top_k; the kernel takes the same maximum again
    fused = FusedSamplingWarper(temp, topk.top_k if topk is not None else 0, topp.top_p if topp is not None else 1.0, min_keep, stock=run,
                                split=split)
    return LogitsProcessorList(procs[:at[0]] + [fused] + procs[at[-1] + 1:])
