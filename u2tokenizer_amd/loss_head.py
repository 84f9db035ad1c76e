"""Loss head (opt-in): lm_head + cross-entropy from the final hidden states without ever holding a rows x vocab tensor.

Stock HuggingFace (`transformers.loss.loss_utils.ForCausalLMLoss`) runs lm_head over every position, upcasts the logits to fp32
and calls F.cross_entropy: per 1024 rows of a 151 936-word vocabulary autograd holds ~2.5 GB of logits, copies and gradients,
and it does so for the rows that carry no label (prompt, visual tokens, padding) as well.  Here:

  * rows whose label is `ignore_index` never enter a product: the hidden states are compacted to the labelled rows first
    (ops.gather_rows), their gradient is scattered back into zeros -- exact, those rows' gradient is zero in the stock path too;
  * the vocabulary is walked in slices of Vs columns (plan_slices): Z = h' W[v0:v0+Vs]^T into one reused buffer (ops.gemm), then
    u2tok_ce_lse_update folds the slice into each row's running (max, sum exp, label logit);  nll = m + log l - z_label;
  * the backward recomputes Z per slice, turns it in place into the gradient of the logits (u2tok_ce_grad_inplace: the fp32
    expression coef (softmax - onehot) rounded to bf16, the very operand stock autograd hands to lm_head's backward), and runs the
    two products on the K-major GEMM forms: dW[v0:v0+Vs] = Z^T h' straight into the rows of one (V, E) bf16 gradient (each element
    one fp32 accumulation over all rows, rounded once), dh' = sum over slices of Z W[v0:v0+Vs] in fp32, rounded once at the end.

The upstream gradient is per row, so the same Function gives the SFT loss (mean, or sum / num_items_in_batch) and the per-token
log-probabilities of DPO.  No atomics anywhere: the same call twice gives the same bits.

Whatever else a driver reads from the logits per row is folded into the same walk while the slice is in flight (`token_stats`,
u2tok_ce_stats_update: no second read, no logits): the argmax (token accuracy of an SFT evaluation; `predictions_for_metrics`), the
sum of the logits and log sum softmax^2 (the mean logits, WPO weights and RPO term of a DPO step; `dpo_outputs`).
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops
from .autograd import _bind_context

DEFAULT_SLICE_BYTES = 256 << 20

# calls of the head, labelled rows it computed, rows it skipped for carrying no label (tests read it: a route that silently fell
# back to the stock head would otherwise pass every check)
stats = {"calls": 0, "rows": 0, "rows_skipped": 0}


def plan_slices(rows: int, vocab: int, slice_bytes: int = DEFAULT_SLICE_BYTES) -> List[Tuple[int, int]]:
    """[(v0, Vs), ...] tiling [0, vocab): every Vs but the last a multiple of 256, rows * Vs * 2 bytes <= slice_bytes (Vs = 256 when
    even that does not fit), the slices of near-equal width."""
    if rows < 1 or vocab < 1:
        raise ValueError(f"plan_slices: rows {rows}, vocab {vocab}")
    cap = max(256, (int(slice_bytes) // (2 * rows)) // 256 * 256)
    n = (vocab + cap - 1) // cap                 # slices needed at the widest legal width ...
    per = (vocab + n - 1) // n                   # ... and the even share of one, rounded up to 256 columns (<= cap: cap % 256 == 0)
    vs = min(cap, (per + 255) // 256 * 256)
    return [(v0, min(vs, vocab - v0)) for v0 in range(0, vocab, vs)]


def supported(hidden_size: int, vocab: int, dtype) -> bool:
    """Shapes and type the head computes (else the caller keeps the stock head)."""
    return dtype == torch.bfloat16 and vocab % 8 == 0 and hidden_size % 64 == 0


def shift_labels(labels: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """ForCausalLMLoss's label handling: position t is scored against token t + 1, the last position against nothing."""
    return torch.nn.functional.pad(labels, (0, 1), value=ignore_index)[..., 1:].contiguous()


def compact_rows(labels: torch.Tensor, vocab: int, ignore_index: int = -100):
    """labels (R,) -> (idx, lab): the rows that carry a label, ascending, and their labels.  One pass validates 0 <= label < vocab
    on those rows (ValueError otherwise)."""
    keep = labels != ignore_index
    bad = keep & ((labels < 0) | (labels >= vocab))
    if int(bad.sum()):
        raise ValueError(f"loss head: labels outside [0, {vocab}) that are not ignore_index ({ignore_index})")
    idx = torch.nonzero(keep).squeeze(1)
    return idx, labels[idx].contiguous()


WANT = ("argmax", "logit_sum", "lse2")     # the extras of token_stats, in the order TokenStatsFn returns them
INT64_MAX = (1 << 63) - 1


def _want(want: Sequence[str]) -> Tuple[str, ...]:
    want = (want,) if isinstance(want, str) else tuple(want)
    bad = [w for w in want if w not in WANT]
    if bad:
        raise ValueError(f"loss head: unknown statistics {bad} (known: {WANT})")
    return tuple(w for w in WANT if w in want)


def _forward(ctx, h, weight, labels, ignore_index: int, slice_bytes: int, want: Tuple[str, ...], who: str):
    """The one walk over the vocabulary: -> (nll (R,) fp32, {name: (R,) tensor} for the names in `want`); saves for _backward.
    Without extras every slice goes through ops.ce_lse_update, with any through ops.ce_stats_update (the same m, l, zt bits)."""
    R, E = h.shape
    V = weight.shape[0]
    ops.training_needs_bf16(h.dtype, who)
    if weight.dtype != h.dtype or weight.shape[1] != E or not supported(E, V, h.dtype):
        raise RuntimeError(f"{who}: bf16 h (R, E) and weight (V, E) with V % 8 == 0 and E % 64 == 0, got {tuple(h.shape)} "
                           f"{h.dtype}, {tuple(weight.shape)} {weight.dtype}")
    if labels.shape != (R,) or labels.dtype != torch.int64:
        raise RuntimeError(f"{who}: labels must be int64 ({R},)")
    idx, lab = compact_rows(labels, V, int(ignore_index))
    Rp = idx.numel()
    stats["calls"] += 1
    stats["rows"] += Rp
    stats["rows_skipped"] += R - Rp
    ctx.shape, ctx.rows = (R, E, V), Rp
    nll = torch.zeros(R, dtype=torch.float32, device=h.device)
    extras = {}
    if "argmax" in want:
        extras["argmax"] = torch.full((R,), int(ignore_index), dtype=torch.int64, device=h.device)
    if "logit_sum" in want:
        extras["logit_sum"] = torch.zeros(R, dtype=torch.float32, device=h.device)
    if "lse2" in want:
        extras["lse2"] = torch.zeros(R, dtype=torch.float32, device=h.device)
    if Rp == 0:
        return nll, extras
    weight = weight.contiguous()
    if Rp == R:
        idx, hp = None, h.contiguous()
    else:
        hp = ops.gather_rows(h.contiguous().unsqueeze(0), idx.unsqueeze(0))[0]
    slices = plan_slices(Rp, V, slice_bytes)
    zbuf = torch.empty(Rp * slices[0][1], dtype=h.dtype, device=h.device)
    m = torch.full((Rp,), float("-inf"), dtype=torch.float32, device=h.device)
    l = torch.zeros(Rp, dtype=torch.float32, device=h.device)
    zt = torch.zeros(Rp, dtype=torch.float32, device=h.device)
    run = {}
    if "argmax" in want:
        run["amax"] = torch.full((Rp,), float("-inf"), dtype=torch.float32, device=h.device)
        run["aidx"] = torch.full((Rp,), INT64_MAX, dtype=torch.int64, device=h.device)
    if "logit_sum" in want:
        run["zsum"] = torch.zeros(Rp, dtype=torch.float32, device=h.device)
    if "lse2" in want:
        run["l2"] = torch.zeros(Rp, dtype=torch.float32, device=h.device)
    for v0, vs in slices:
        z = zbuf[:Rp * vs].view(Rp, vs)
        ops.gemm(hp, weight[v0:v0 + vs], out=z)
        if run:
            ops.ce_stats_update(z, v0, lab, m, l, zt, **run)
        else:
            ops.ce_lse_update(z, v0, lab, m, l, zt)
    log_l = torch.log(l)
    lse = m + log_l
    found = {}
    if "argmax" in want:
        found["argmax"] = run["aidx"]
    if "logit_sum" in want:
        found["logit_sum"] = run["zsum"]
    if "lse2" in want:       # lse2 - 2 lse = (2 m + log l2) - 2 (m + log l): the 2 m cancel exactly, so they are never added
        found["lse2"] = torch.log(run["l2"]) - 2.0 * log_l
    if idx is None:
        nll = lse - zt
        extras = found
    else:
        nll.index_copy_(0, idx, lse - zt)
        for k, t in found.items():
            extras[k].index_copy_(0, idx, t)
    ctx.save_for_backward(hp, weight, lab, lse, idx)
    ctx.slices = slices
    return nll, extras


def _backward(ctx, g):
    """(dh, dW) of sum(g . nll): recomputes Z per slice (see the module docstring)."""
    R, E, V = ctx.shape
    Rp = ctx.rows
    need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if Rp == 0:
        dh = torch.zeros((R, E), dtype=torch.bfloat16, device=g.device) if need_h else None
        dw = torch.zeros((V, E), dtype=torch.bfloat16, device=g.device) if need_w else None
        return dh, dw
    hp, weight, lab, lse, idx = ctx.saved_tensors
    g = g.to(torch.float32)
    coef = (g if idx is None else g[idx]).contiguous()
    slices = ctx.slices
    zbuf = torch.empty(Rp * slices[0][1], dtype=hp.dtype, device=hp.device)
    dw = torch.empty((V, E), dtype=hp.dtype, device=hp.device) if need_w else None
    dh32 = torch.empty((Rp, E), dtype=torch.float32, device=hp.device) if need_h else None
    part = torch.empty_like(dh32) if need_h and len(slices) > 1 else None
    for i, (v0, vs) in enumerate(slices if (need_h or need_w) else ()):
        z = zbuf[:Rp * vs].view(Rp, vs)
        w = weight[v0:v0 + vs]
        ops.gemm(hp, w, out=z)
        ops.ce_grad_inplace(z, v0, lab, lse, coef)
        if need_w:
            ops.gemm_kmajor(z, hp, a_kmajor=True, out=dw[v0:v0 + vs])
        if need_h:
            if i == 0:
                ops.gemm_kmajor(z, w, a_kmajor=False, out_f32=True, out=dh32)
            else:
                dh32 += ops.gemm_kmajor(z, w, a_kmajor=False, out_f32=True, out=part)
    dh = None
    if need_h:
        if idx is None:
            dh = dh32.to(hp.dtype)
        else:
            dh = torch.zeros((R, E), dtype=hp.dtype, device=hp.device).index_copy_(0, idx, dh32.to(hp.dtype))
    return dh, dw


@_bind_context
class TokenNLLFn(Function):
    """nll (R,) fp32 = -log softmax(h W^T)[label], 0 where label == ignore_index.  h (R, E) bf16, weight (V, E) bf16, labels (R,)
    int64."""

    @staticmethod
    def forward(ctx, h, weight, labels, ignore_index: int, slice_bytes: int):
        return _forward(ctx, h, weight, labels, ignore_index, slice_bytes, (), "TokenNLLFn")[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return (*_backward(ctx, g), None, None, None)


@_bind_context
class TokenStatsFn(Function):
    """TokenNLLFn with extras from the same walk: -> (nll, *extras), the extras those of `want` (a subset of WANT, in WANT's order),
    (R,) each and not differentiable: argmax int64 (`ignore_index` where the row carries no label), logit_sum fp32 and
    lse2 = log sum softmax^2 fp32 (0 there).  nll and the backward are TokenNLLFn's."""

    @staticmethod
    def forward(ctx, h, weight, labels, ignore_index: int, slice_bytes: int, want: Tuple[str, ...]):
        nll, extras = _forward(ctx, h, weight, labels, ignore_index, slice_bytes, want, "TokenStatsFn")
        outs = tuple(extras[k] for k in want)
        ctx.mark_non_differentiable(*outs)
        return (nll, *outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        return (*_backward(ctx, g), None, None, None, None)


def token_nll(hidden: torch.Tensor, weight: torch.Tensor, labels: torch.Tensor, *, ignore_index: int = -100,
              slice_bytes: int = DEFAULT_SLICE_BYTES) -> torch.Tensor:
    """-log p(labels) per position, fp32, shaped like labels; 0 where labels == ignore_index.  hidden (..., E), labels (...)
    already aligned with the positions (no shift)."""
    if hidden.shape[:-1] != labels.shape:
        raise RuntimeError(f"loss head: hidden {tuple(hidden.shape)} and labels {tuple(labels.shape)} do not match")
    lab = labels.to(device=hidden.device, dtype=torch.int64).reshape(-1).contiguous()
    nll = TokenNLLFn.apply(hidden.reshape(-1, hidden.shape[-1]), weight, lab, int(ignore_index), int(slice_bytes))
    return nll.view(labels.shape)


def linear_cross_entropy(hidden: torch.Tensor, weight: torch.Tensor, labels: torch.Tensor, *, ignore_index: int = -100,
                         num_items_in_batch=None, shift: bool = True, slice_bytes: int = DEFAULT_SLICE_BYTES) -> torch.Tensor:
    """ForCausalLMLoss(lm_head(hidden), labels) without the logits: the labels padded and shifted by one (shift=True; False: the
    labels are `shift_labels` already), then the mean of the labelled rows' losses, or their sum / num_items_in_batch."""
    if shift:
        labels = shift_labels(labels, ignore_index)
    nll = token_nll(hidden, weight, labels, ignore_index=ignore_index, slice_bytes=slice_bytes)
    return reduce_nll(nll, labels != ignore_index, num_items_in_batch)


def reduce_nll(nll: torch.Tensor, labelled: torch.Tensor, num_items_in_batch=None) -> torch.Tensor:
    """ForCausalLMLoss's reduction of per-position losses (0 where not `labelled`): their mean over the labelled rows, or their
    sum / num_items_in_batch."""
    total = nll.sum()
    if num_items_in_batch is None:
        return total / labelled.sum().to(total.device)     # (no labelled row: nan, as F.cross_entropy's mean)
    if torch.is_tensor(num_items_in_batch):
        num_items_in_batch = num_items_in_batch.to(total.device)
    return total / num_items_in_batch


def token_logprobs(hidden: torch.Tensor, weight: torch.Tensor, labels: torch.Tensor, *, ignore_index: int = -100,
                   shift: bool = True, slice_bytes: int = DEFAULT_SLICE_BYTES) -> torch.Tensor:
    """log p(label) per position (B, S) fp32, 0 where ignored: what a DPO trainer gathers from log_softmax(logits) and masks
    (position t scored against labels[t + 1] when shift)."""
    if shift:
        labels = shift_labels(labels, ignore_index)
    return -token_nll(hidden, weight, labels, ignore_index=ignore_index, slice_bytes=slice_bytes)


class TokenStats(NamedTuple):
    """Per-position statistics of the logits, each shaped like the labels.  `labelled`: the positions that carry a label; the others
    hold the fill values (logprob 0, argmax `ignore_index`, logit_sum 0, lse2m 0).  An extra that was not asked for is None."""
    logprob: torch.Tensor                      # fp32, log p(label); differentiable
    labelled: torch.Tensor                     # bool
    argmax: Optional[torch.Tensor] = None      # int64, first index of the row's largest logit
    logit_sum: Optional[torch.Tensor] = None   # fp32, sum of the row's logits
    lse2m: Optional[torch.Tensor] = None       # fp32, log sum softmax^2 = logsumexp(2 z) - 2 logsumexp(z)

    @classmethod
    def filled(cls, labelled: torch.Tensor, want: Sequence[str] = (), ignore_index: int = -100) -> "TokenStats":
        """What positions without a label hold, everywhere."""
        want = _want(want)
        zeros = lambda: torch.zeros(labelled.shape, dtype=torch.float32, device=labelled.device)
        return cls(zeros(), labelled,
                   torch.full(labelled.shape, int(ignore_index), dtype=torch.int64, device=labelled.device) if "argmax" in want else None,
                   zeros() if "logit_sum" in want else None, zeros() if "lse2" in want else None)


def token_stats(hidden: torch.Tensor, weight: torch.Tensor, labels: torch.Tensor, *, want: Sequence[str] = (),
                ignore_index: int = -100, shift: bool = True, slice_bytes: int = DEFAULT_SLICE_BYTES) -> TokenStats:
    """`token_logprobs` (the same bits, the same backward) and, from the same single walk over the vocabulary, the per-position
    extras named in `want` ("argmax", "logit_sum", "lse2"; not differentiable).  Position t is scored against labels[t + 1] when
    `shift`.  want=() is `token_logprobs` itself."""
    want = _want(want)
    if shift:
        labels = shift_labels(labels, ignore_index)
    if not want:
        return TokenStats(-token_nll(hidden, weight, labels, ignore_index=ignore_index, slice_bytes=slice_bytes),
                          (labels != ignore_index).to(hidden.device))
    if hidden.shape[:-1] != labels.shape:
        raise RuntimeError(f"loss head: hidden {tuple(hidden.shape)} and labels {tuple(labels.shape)} do not match")
    lab = labels.to(device=hidden.device, dtype=torch.int64).reshape(-1).contiguous()
    nll, *outs = TokenStatsFn.apply(hidden.reshape(-1, hidden.shape[-1]), weight, lab, int(ignore_index), int(slice_bytes), want)
    extras = {k: t.view(labels.shape) for k, t in zip(want, outs)}
    return TokenStats(-nll.view(labels.shape), (lab != ignore_index).view(labels.shape), extras.get("argmax"),
                      extras.get("logit_sum"), extras.get("lse2"))


def dpo_outputs(stats: TokenStats, num_examples: int, *, vocab: int, use_weighting: bool = False, ipo: bool = False,
                rpo: bool = False) -> Dict[str, torch.Tensor]:
    """What a DPO trainer's concatenated forward returns, from the TokenStats (B = 2 num_examples sequences, the chosen half first;
    want "logit_sum", and "lse2" for use_weighting) of the concatenated batch instead of its logits:
      chosen_logps / rejected_logps   the sequences' sums of log p(label) (ipo: their means over the labelled positions);
      mean_chosen_logits / mean_rejected_logits   the mean of all logits of the half's labelled positions;
      policy_weights (use_weighting)  min(1, exp(w_chosen + w_rejected)), w a sequence's mean over its labelled positions of
                                      log p(label) - log sum_v p(v)^2; detached;
      nll_loss (rpo)                  the mean of -log p(label) over the chosen half's labelled positions."""
    n = int(num_examples)
    lp, on = stats.logprob, stats.labelled
    if lp.dim() != 2 or lp.shape[0] != 2 * n:
        raise ValueError(f"dpo_outputs: statistics of a (2 x {n}, S) batch expected, got {tuple(lp.shape)}")
    if stats.logit_sum is None or (use_weighting and stats.lse2m is None):
        raise ValueError('dpo_outputs: needs want=("logit_sum",), and "lse2" with use_weighting')
    count = on.sum(-1)
    logps = lp.sum(-1)
    out = {}
    if use_weighting:
        with torch.no_grad():
            w = ((lp - stats.lse2m) * on).sum(-1) / count
            out["policy_weights"] = torch.clamp(torch.exp(w[:n] + w[n:]), max=1)
    if rpo:
        out["nll_loss"] = -lp[:n].sum() / count[:n].sum()
    if ipo:
        logps = logps / count
    out["chosen_logps"], out["rejected_logps"] = logps[:n], logps[n:]
    for name, half in (("mean_chosen_logits", slice(0, n)), ("mean_rejected_logits", slice(n, 2 * n))):
        out[name] = (stats.logit_sum[half].sum(dtype=torch.float64) / (count[half].sum() * int(vocab))).float()
    return out


def predictions_for_metrics(logits: torch.Tensor, labels=None) -> torch.Tensor:
    """A `preprocess_logits_for_metrics` for transformers' Trainer that serves both heads: predictions already (an integer tensor:
    the loss head with `config.u2_fused_loss_head_predictions`) pass through, logits give their argmax over the last dimension."""
    if not logits.is_floating_point():
        return logits
    return torch.argmax(logits, dim=-1)
