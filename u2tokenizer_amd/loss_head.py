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
"""
from __future__ import annotations

from typing import List, Optional, Tuple

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


@_bind_context
class TokenNLLFn(Function):
    """nll (R,) fp32 = -log softmax(h W^T)[label], 0 where label == ignore_index.  h (R, E) bf16, weight (V, E) bf16, labels (R,)
    int64."""

    @staticmethod
    def forward(ctx, h, weight, labels, ignore_index: int, slice_bytes: int):
        R, E = h.shape
        V = weight.shape[0]
        ops.training_needs_bf16(h.dtype, "TokenNLLFn")
        if weight.dtype != h.dtype or weight.shape[1] != E or not supported(E, V, h.dtype):
            raise RuntimeError(f"TokenNLLFn: bf16 h (R, E) and weight (V, E) with V % 8 == 0 and E % 64 == 0, got {tuple(h.shape)} "
                               f"{h.dtype}, {tuple(weight.shape)} {weight.dtype}")
        if labels.shape != (R,) or labels.dtype != torch.int64:
            raise RuntimeError(f"TokenNLLFn: labels must be int64 ({R},)")
        idx, lab = compact_rows(labels, V, int(ignore_index))
        Rp = idx.numel()
        stats["calls"] += 1
        stats["rows"] += Rp
        stats["rows_skipped"] += R - Rp
        ctx.shape, ctx.rows = (R, E, V), Rp
        nll = torch.zeros(R, dtype=torch.float32, device=h.device)
        if Rp == 0:
            return nll
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
        for v0, vs in slices:
            z = zbuf[:Rp * vs].view(Rp, vs)
            ops.gemm(hp, weight[v0:v0 + vs], out=z)
            ops.ce_lse_update(z, v0, lab, m, l, zt)
        lse = m + torch.log(l)
        if idx is None:
            nll = lse - zt
        else:
            nll.index_copy_(0, idx, lse - zt)
        ctx.save_for_backward(hp, weight, lab, lse, idx)
        ctx.slices = slices
        return nll

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        R, E, V = ctx.shape
        Rp = ctx.rows
        need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if Rp == 0:
            dh = torch.zeros((R, E), dtype=torch.bfloat16, device=g.device) if need_h else None
            dw = torch.zeros((V, E), dtype=torch.bfloat16, device=g.device) if need_w else None
            return dh, dw, None, None, None
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
        return dh, dw, None, None, None


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
    total = nll.sum()
    if num_items_in_batch is None:
        return total / (labels != ignore_index).sum().to(total.device)     # (no labelled row: nan, as F.cross_entropy's mean)
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
