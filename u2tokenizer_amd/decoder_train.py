"""Training route of the decoder layers (opt-in): the layer's forward AND backward on the library's kernels.

`enable_fused_prefill(model, train=True)` (prefill.py) -- or `config.u2_fused_decoder_training = True` on a u2 causal LM --
makes a patched Llama / Qwen3 decoder layer that is called with grad enabled (with `train_phi3=True` /
`config.u2_fused_phi3_training = True` on top: a Phi-3 layer as well, and head dim 96 for all three) run as

    RMSNormFn -> PackedLinearFn (q|k|v) -> HeadNormRopeFn -> GqaAttentionFn -> PackedLinearFn (o, + residual)
    -> RMSNormFn -> PackedLinearFn (gate|up) -> SwiGLUFn -> PackedLinearFn (down, + residual)

torch.autograd.Functions over the C-ABI blocks, each saving what its backward needs:
  * the products run on u2tok_gemm_bf16 both ways (dX = dY W and dW = dY^T X on the K-major operand forms, as autograd.LinearFn).
    q|k|v and gate|up use the packed buffers prefill._pack lays out (the nn.Parameters are views of them): ONE product forward,
    ONE packed dW backward, handed to autograd as one view per Parameter -- `.grad` of q_proj / k_proj / v_proj (or gate / up)
    receives its rows, accumulated in place into an existing `.grad` (a view into a flat optimizer bucket stays one);
  * the attention is the causal GQA kernel with per-sequence key lengths (u2tok_attention_gqa_ex, which also leaves the row
    statistics) and its flash backward (u2tok_attention_gqa_bwd: the causal instantiations of csrc/attn_bwd.hip's bwd_dq_kernel /
    bwd_dkv_kernel, the pair the ViT's backward also runs; head dim 96 through u2tok_attention_gqa_bwd_d96), which writes
    dq | dk | dv straight into one packed gradient;
  * RMSNorm, head norm + rotary and SwiGLU have their backward kernels in csrc/backward.hip (fixed-order fp32 weight gradients);
  * torch moves data and adds the residual stream's two gradient contributions.
  * with `train_lora=True` / `config.u2_fused_lora_training = True` on top, a LoRA-wrapped projection (lora.adapter_of) adds its
    branch after the packed product it belongs to (LoraDeltaFn, on the rank-r kernels of csrc/lora.hip); the frozen base weights
    need no dW product.

When a layer takes the route (prefill.route, decided on every call; everything else keeps the stock forward): bf16 on the
GPU, every projection exactly nn.Linear with no hooks, no active attention or residual dropout, head dim 64 or 128 (train_phi3:
96 too), no KV cache, no sliding window on Llama / Qwen3 (train_phi3, Phi-3's `sliding_window` = W: calls of S <= W positions,
where the window hides nothing), and an attention mask that is causal with at most right padding.  The mask is read from the LAYER's own
`attention_mask` argument (the 4-D mask HF builds, or None; layer_mask_kv_len below) and the verdict is stored on that
tensor: the recompute of non-reentrant gradient checkpointing calls the layer with the same argument objects, so it sees the
key lengths of ITS forward, not those of whatever forward of the model ran last.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd import Function

from . import ops
from .autograd import _bind_context
from .lora import adapter_of

# layers whose forward took the training route (tests read it: a route that silently fell back to the stock layers would
# otherwise pass every gradient check)
stats = {"layers": 0}
# ... and, of those, the layers that ran with at least one LoRA adapter on the rank-r kernels, and the adapters they ran
lora_stats = {"layers": 0, "adapters": 0}


def train_mask_rule(mask: Optional[torch.Tensor]):
    """The 2-D attention masks the training route computes: ("causal", None) for no mask or all ones, ("lengths", lens) for
    right padding (every row ones then zeros, at least one one; lens int64 (B,)), None for anything else (left padding, holes,
    an empty row: stock layers).  Pure tensor logic: runs on the CPU as well."""
    if mask is None:
        return "causal", None
    if not torch.is_tensor(mask) or mask.dim() != 2 or mask.shape[1] == 0:
        return None
    m = mask.to(torch.bool)
    if bool(m.all()):
        return "causal", None
    lens = m.sum(dim=1)
    pos = torch.arange(m.shape[1], device=m.device)
    if bool((lens < 1).any()) or not bool(torch.equal(m, pos[None, :] < lens[:, None])):
        return None
    return "lengths", lens


def layer_mask_kv_len(am, B: int, S: int):
    """Verdict on a decoder LAYER's attention_mask argument: (True, None) plain causal, (True, kv_len int32 (B,) on the mask's
    device) right padding, (False, None) anything else.  HF hands layers None (sdpa, no padding) or the 4-D (B, 1, S, S) mask
    it built (bool: True = visible; float: 0 = visible); its last query row is the 2-D key mask, and the whole mask must equal
    causal AND key < length.  Stored on the mask tensor (one check per model forward, and the recompute reads the same)."""
    if am is None:
        return True, None
    if not torch.is_tensor(am):
        return False, None
    hit = getattr(am, "_u2_train_kv", None)
    if hit is not None:
        return hit
    verdict = (False, None)
    if am.dim() == 4 and am.shape[0] == B and am.shape[1] == 1 and am.shape[2] == S and am.shape[3] == S:
        vis = am if am.dtype == torch.bool else am == 0
        rule = train_mask_rule(vis[:, 0, -1, :])
        if rule is not None:
            pos = torch.arange(S, device=am.device)
            causal = pos[None, :] <= pos[:, None]
            if rule[0] == "causal":
                want = causal[None].expand(B, S, S)
            else:
                want = causal[None] & (pos[None, None, :] < rule[1][:, None, None])
            if bool(torch.equal(vis[:, 0], want)):
                verdict = (True, None if rule[0] == "causal" else rule[1].to(torch.int32).contiguous())
    try:
        am._u2_train_kv = verdict
    except (AttributeError, RuntimeError):
        pass
    return verdict


# ------------------------------------------------------------------------------------------------ Functions
@_bind_context
class PackedLinearFn(Function):
    """y = x W^T (+ b) (+ res) with W the packed rows of `nw` projections (their weights are `params[:nw]`, their biases
    `params[nw:]`, packed in `b`).  W / b are the forward's operands (views of the Parameters' storage, no autograd); the
    Parameters are inputs so that autograd hands each its gradient: one packed dW (and db), split into views."""

    @staticmethod
    def forward(ctx, x, res, W, b, nw: int, *params):
        y = ops.gemm(x, W, bias=b, residual=res)
        ctx.save_for_backward(x, W)
        ctx.nw, ctx.has_b, ctx.has_res = nw, b is not None, res is not None
        ctx.rows = [p.shape[0] for p in params[:nw]]
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        N, K = W.shape
        dy = dy.contiguous()
        nw = ctx.nw
        need = ctx.needs_input_grad
        dx = dres = None
        if need[0]:
            if dy.shape[0] >= 4096 and W.numel() <= (1 << 23):   # (autograd.LinearFn: many rows against a small weight)
                dx = ops.gemm(dy, ops.transpose_ex(W, 1, N, K, K, 0)[0])
            else:
                dx = ops.gemm_kmajor(dy, W, a_kmajor=False)
        if ctx.has_res and need[1]:
            dres = dy
        gw = [None] * nw
        if any(need[5:5 + nw]):
            dW = ops.gemm_kmajor(dy, x, a_kmajor=True)   # (N, K): the packed gradient
            o = 0
            for i, r in enumerate(ctx.rows):
                gw[i] = dW[o:o + r] if need[5 + i] else None
                o += r
        gb = [None] * (nw if ctx.has_b else 0)
        if ctx.has_b and any(need[5 + nw:]):
            db = ops.colsum(dy)
            o = 0
            for i, r in enumerate(ctx.rows):
                gb[i] = db[o:o + r] if need[5 + nw + i] else None
                o += r
        return (dx, dres, None, None, None, *gw, *gb)


def packed_linear(x, linears, W, b, res=None):
    params = [lin.weight for lin in linears] + ([lin.bias for lin in linears] if b is not None else [])
    return PackedLinearFn.apply(x, res, W, b, len(linears), *params)


@_bind_context
class LoraDeltaFn(Function):
    """y[:, o_i : o_i + N_i] += s_i (xd_i A_i^T) B_i^T for the n adapters of one packed product: `y` (rows, sum N) is the output
    of PackedLinearFn, `meta` = ((o_i, N_i, s_i), ...), then xd_0 .. xd_n-1 (rows, K: the product's input after each adapter's own
    dropout), A_0 .. A_n-1 (r, K) and B_0 .. B_n-1 (N_i, r), the adapters' Parameters.

    IN PLACE on y's memory, returned as a NEW tensor over it: PackedLinearFn hands its output on as a view made inside a Function,
    which autograd lets no later Function mark dirty, and a copy would double the branch's traffic.  The caller drops the old
    tensor (lora_delta rebinds the name), and nothing has saved it: PackedLinearFn saves its inputs, not its output.  The version
    counter the two tensors share is bumped, so autograd would refuse a backward that did read the old values.
    Rounding points: A and B in the element type (fp32 adapter weights get a 16-bit compute copy per call: they are r x K small),
    xd in the element type, u_i = xd_i A_i^T rounded to the element type (u2tok_lora_down), and ONE rounding of y: float(y) +
    s_i u_i B_i^T in fp32 (u2tok_lora_up, accumulate form) -- the stock wrapped layer rounds u, u B^T, the scaling and the sum.
    Backward: dy passes through to the base product; du_i = s_i dy_i B_i (u2tok_lora_down on a contiguous B^T), dB_i^T = s_i
    u_i^T dy_i and dA_i = du_i^T xd_i (u2tok_lora_wgrad; fp32 results for fp32 Parameters), d xd_i = du_i A_i (u2tok_lora_up on a
    contiguous A^T), which autograd carries back through torch's dropout."""

    @staticmethod
    def forward(ctx, y, meta, *ts):
        n = len(meta)
        xds, As, Bs = ts[:n], ts[n:2 * n], ts[2 * n:]
        y = y.detach()
        saved = []
        for (o, N, s), xd, A, B in zip(meta, xds, As, Bs):
            A16, B16 = A.detach().to(y.dtype), B.detach().to(y.dtype)
            u = ops.lora_down(xd, A16)
            ops.lora_up(u, B16, y[:, o:o + N], alpha=s, accumulate=True)
            saved += [xd, u, A16, B16]
        torch.autograd.graph.increment_version(y)   # (the kernels wrote through raw pointers: tell autograd)
        ctx.save_for_backward(*saved)
        ctx.meta = meta
        ctx.f32 = [(A.dtype == torch.float32, B.dtype == torch.float32) for A, B in zip(As, Bs)]
        return y

    @staticmethod
    def backward(ctx, dy):
        meta, n = ctx.meta, len(ctx.meta)
        need = ctx.needs_input_grad
        if dy.stride(1) != 1:
            dy = dy.contiguous()
        dxd, dA, dB = [None] * n, [None] * n, [None] * n
        saved = ctx.saved_tensors   # (read once: under checkpointing the first read runs the recompute)
        for i, (o, N, s) in enumerate(meta):
            xd, u, A16, B16 = saved[4 * i:4 * i + 4]
            a32, b32 = ctx.f32[i]
            dyi = dy[:, o:o + N]
            if need[2 + 2 * n + i]:
                dB[i] = ops.lora_wgrad(u, dyi, alpha=s, out_f32=b32).t()
            if need[2 + i] or need[2 + n + i]:
                du = ops.lora_down(dyi, B16.t().contiguous(), alpha=s)
                if need[2 + n + i]:
                    dA[i] = ops.lora_wgrad(du, xd, out_f32=a32)
                if need[2 + i]:
                    dxd[i] = ops.lora_up(du, A16.t().contiguous())
        return (dy, None, *dxd, *dA, *dB)


def lora_delta(y, x2, modules, B: int, S: int):
    """Add the adapter branches of the wrapped ones among `modules` (the projections of one packed product, in packing order: q, k,
    v / o / gate, up / down -- the order in which the stock layer calls them, so that the same seed draws the same dropout masks)
    to the product's output `y` (B S, sum N); x2 (B S, K) the product's input.  Each adapter's OWN dropout module is called on the
    input in its stock (B, S, K) shape and in the adapter weights' dtype, as the stock wrapped projection calls it.  Without a
    wrapped projection y comes back as it is."""
    meta, xds, As, Bs = [], [], [], []
    o = 0
    for m in modules:
        N = m.weight.shape[0]
        if type(m) is not torch.nn.Linear:
            ad = adapter_of(m)
            if ad is None:   # (route() admitted the layer: the module changed under the call)
                raise RuntimeError(f"decoder training route: {type(m).__name__} is not an adapter the route computes")
            xa = x2.view(B, S, -1)
            if ad.A.weight.dtype != xa.dtype:
                xa = xa.to(ad.A.weight.dtype)
            xd = ad.dropout(xa).to(x2.dtype).reshape(B * S, -1)
            meta.append((o, N, ad.scaling))
            xds.append(xd), As.append(ad.A.weight), Bs.append(ad.B.weight)
        o += N
    if not meta:
        return y
    return LoraDeltaFn.apply(y, tuple(meta), *xds, *As, *Bs)


@_bind_context
class RMSNormFn(Function):
    """y = bf16(x rstd) * w  (LlamaRMSNorm / Qwen3RMSNorm); backward u2tok_rmsnorm_bwd."""

    @staticmethod
    def forward(ctx, x, w, eps: float):
        ctx.save_for_backward(x, w)
        ctx.eps = eps
        return ops.rmsnorm(x, w, eps)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx, dw = ops.rmsnorm_bwd(x, w, dy, ctx.eps)
        return dx, (dw.to(w.dtype) if ctx.needs_input_grad[1] else None), None


@_bind_context
class HeadNormRopeFn(Function):
    """Per-head RMSNorm (Qwen3 q_norm / k_norm; none for Llama) + rotary embedding on the q / k columns of the packed q|k|v
    product (u2tok_qk_norm_rope on a copy); backward u2tok_qk_norm_rope_bwd (inverse rotation, then the norm's backward)."""

    @staticmethod
    def forward(ctx, qkv, wq, wk, cos, sin, Hq: int, Hkv: int, d: int, eps: float):
        out = qkv.clone()
        ops.qk_norm_rope(out, wq, wk, cos, sin, Hq, Hkv, d, eps)
        ctx.save_for_backward(qkv if wq is not None else None, wq, wk, cos, sin)
        ctx.cfg = (Hq, Hkv, d, eps)
        return out

    @staticmethod
    def backward(ctx, dy):
        pre, wq, wk, cos, sin = ctx.saved_tensors
        Hq, Hkv, d, eps = ctx.cfg
        g = dy.clone(memory_format=torch.contiguous_format)
        _, dwq, dwk = ops.qk_norm_rope_bwd(g, pre, wq, wk, cos, sin, Hq, Hkv, d, eps)
        gq = dwq.to(wq.dtype) if wq is not None and ctx.needs_input_grad[1] else None
        gk = dwk.to(wk.dtype) if wk is not None and ctx.needs_input_grad[2] else None
        return g, gq, gk, None, None, None, None, None, None


@_bind_context
class GqaAttentionFn(Function):
    """Causal grouped-query attention over the packed q|k|v rows (B * S, (Hq + 2 Hkv) d) with per-sequence key lengths;
    -> (B * S, Hq d).  Backward: the flash kernel pair, dq | dk | dv into one packed gradient."""

    @staticmethod
    def forward(ctx, qkv, kv_len, B: int, S: int, Hq: int, Hkv: int, d: int, scale: float):
        q3 = qkv.view(B, S, -1)
        out, lse = ops.attention_gqa_ex(q3[..., :Hq * d], q3[..., Hq * d:(Hq + Hkv) * d], q3[..., (Hq + Hkv) * d:], Hq, Hkv,
                                        scale, kv_len=kv_len, with_lse=True)
        ctx.save_for_backward(qkv, out, lse)
        ctx.kv_len = kv_len
        ctx.cfg = (B, S, Hq, Hkv, d, scale)
        return out.view(B * S, Hq * d)

    @staticmethod
    def backward(ctx, dy):
        qkv, out, lse = ctx.saved_tensors
        B, S, Hq, Hkv, d, scale = ctx.cfg
        dqkv = ops.attention_gqa_bwd(qkv.view(B, S, -1), out, dy.reshape(B, S, Hq * d), Hq, Hkv, scale, kv_len=ctx.kv_len,
                                     lse=lse)
        return dqkv.view(B * S, -1), None, None, None, None, None, None, None


@_bind_context
class SwiGLUFn(Function):
    """act = bf16(silu(gate)) * up from the packed gate|up product (the two-step form: the pre-activations are saved);
    backward: the packed [d_gate | d_up] (u2tok_swiglu_bwd)."""

    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        return ops.swiglu(gu)

    @staticmethod
    def backward(ctx, dact):
        (gu,) = ctx.saved_tensors
        return ops.swiglu_bwd(gu, dact)


# ------------------------------------------------------------------------------------------------ the layer
def layer_forward_train(layer, lo, x2, cos, sin, B: int, S: int, kv_len):
    """The layer's forward through the Functions above on its rows x2 (B S, E) -> (B, S, E); `lo` is the layer's layout
    (prefill.py, `product`: the four products' weights and the projections that own them -- three and two nn.Linear behind q|k|v
    and gate|up for Llama / Qwen3, Phi-3's single qkv_proj / gate_up_proj, whose Parameter receives the packed dW whole), cos /
    sin the rotary rows (B S, d),
    kv_len the key lengths or None.  Phi-3's stock layer rounds where Llama's does: the activation is up * bf16(silu(gate)) on
    the halves of the gate_up_proj output (gate rows first), its two residual dropouts are inactive on this route (lo.ready)
    and it has no head norm (HeadNormRopeFn's wq = None form)."""
    att = layer.self_attn
    cfg = att.config
    Hq, Hkv, d = cfg.num_attention_heads, cfg.num_key_value_heads, att.head_dim
    stats["layers"] += 1   # (counted on entry: a checkpoint recompute stops early, once the tensors it needs are back)
    pr = lo.projections(layer)
    n_ad = sum(type(m) is not torch.nn.Linear for m in pr)
    if n_ad:
        lora_stats["layers"] += 1
        lora_stats["adapters"] += n_ad

    def product(g: int, x, res=None):
        """product g of the layout (its modules, packed weight and bias: lo.product) on x, then its adapters' branch"""
        lins, W, b = lo.product(pr, g)
        return lora_delta(packed_linear(x, lins, W.detach(), None if b is None else b.detach(), res=res), x, lins, B, S)

    xn = RMSNormFn.apply(x2, layer.input_layernorm.weight, float(layer.input_layernorm.variance_epsilon))
    qkv = product(0, xn)
    qn, kn = getattr(att, "q_norm", None), getattr(att, "k_norm", None)
    qkv = HeadNormRopeFn.apply(qkv, None if qn is None else qn.weight, None if kn is None else kn.weight, cos, sin, Hq, Hkv,
                               d, float(qn.variance_epsilon) if qn is not None else 1e-6)
    ctx = GqaAttentionFn.apply(qkv, kv_len, B, S, Hq, Hkv, d, float(att.scaling))
    h = product(1, ctx, res=x2)
    hn = RMSNormFn.apply(h, layer.post_attention_layernorm.weight, float(layer.post_attention_layernorm.variance_epsilon))
    act = SwiGLUFn.apply(product(2, hn))
    return product(3, act, res=h).view(B, S, -1)
