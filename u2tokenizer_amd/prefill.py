"""Decoder prefill on the spliced embeddings through the HIP kernels (the step AFTER the path:
`LlamaForCausalLM / Qwen3ForCausalLM.forward(inputs_embeds=...)`, /root/reference/src/model/language_model/u2llama.py:76-87,
and the first forward of `generate`, u2llama.py:123-126).

The decoder stays the stock HuggingFace module tree: its parameters (names, shapes, state dict), its KV cache and its
`generate` loop are untouched.  `enable_fused_prefill(model)` replaces the `forward` of every decoder layer by one that,
for the PREFILL call (no grad, bf16 on the GPU, more than one position, empty cache for that layer, full attention, no
padding) runs the layer as

    RMSNorm -> ONE q|k|v GEMM -> per-head RMSNorm (Qwen3) + rotary embedding -> causal grouped-query attention
    -> out-projection GEMM with the residual in its epilogue -> RMSNorm -> ONE gate|up GEMM with SiLU(gate) * up in its
    epilogue -> down-projection GEMM with the residual in its epilogue

on the library's MFMA GEMMs (include/u2tok.h: u2tok_gemm_bf16), the fused attention kernel of tokattn.hip (grouped-query heads,
causal mask, scores never in HBM) and the row kernels of decoder.hip, and for a DECODE step (one new position per sequence, batch
<= 16, a plain HF DynamicCache) as two library calls around the cache update (`_decode_step`: weight-streaming few-rows products,
attention with the keys split over workgroups).  Everything else -- training, CPU tensors, padded batches, other cache types --
takes the layer's original forward, unless one of the opt-in switches widens a route: SWITCHES below lists them, one record
each (keyword of `enable_fused_prefill`, field of the stack's state, config attribute of a u2 causal LM, what it implies, what it
does); `enable_fused_prefill` and `language_model._maybe_fuse` both walk that table.  What the switches share:
  * padded: `pad_rule` turns the call's 2-D mask into a key range per sequence; the prefill hands it to the attention kernel, the
    decode step to the batched decode attention of csrc/decode_attn.hip (u2tok_decoder_decode_post with batched = 1).
  * continued: both of its calls go through the attention kernel's band form (K / V read in the cache's own (B, H_kv, capacity,
    d) layout, the lower edge of an attention window per query row).  Taken: no cache or a plain DynamicCache of DynamicLayer /
    append-in-place / DynamicSlidingWindowLayer layers, no mask or all ones, with `padded` also a LEFT-padded mask as wide as
    cache + call on layers without a window; stock: a right-padded continuation, holes, window + padding, offloaded / static /
    quantized caches.
  * fp8_decode, fp4_decode, lora: what they keep per layer beside the weights (e4m3 copies with a scale per row; e2m1 copies with a
    scale per block of 32; 16-bit adapter operands)
    lives in the layer's `_LayerState` with the decode step's descriptors, is rebuilt when a source changed and on nothing
    else, and goes when the switch goes off.  With `lora` the adapter branch follows each of the four products UNMERGED -- on
    many rows the down / up kernels of csrc/lora.hip, on a decode step the two-launch group product of csrc/lora_rows.hip
    inside the two library calls --, and a wrapper that is merged or disabled runs as its base layer.
  * stack_decode, head: the decoder STACK's forward is wrapped as well; a decode step `route` would hand to the fused step in every
    layer (`stack_route`) runs as one library call for all of them (`_stack_step`), with the bits of the per-layer route; a u2
    causal LM's call that `head_route` admits runs that step WITH its head (final RMSNorm, lm_head, fp32 logits) through
    `head_forward`; the head's descriptor and quantised copy live on the model (`_HeadState`), not in the stack's state.
  * kv8, kv8_continued, stack_kv8: the cache a fused prefill starts is a `Kv8Layer` (e4m3 codes and a scale per cached row) where
    the append-in-place layer would go; the decode step (u2tok_decoder_decode_post_kv8), with kv8_continued the continued prefill
    (u2tok_attention_kv8_rows; calls longer than KV8_EXTEND_MAX_ROWS stay stock) and with stack_kv8 the whole-stack step and the
    head (u2tok_decoder_decode_stack_kv8 / _stack_head_kv8) write and read the codes; every route that refuses the layer reads the
    same cache dequantised through the layer's `update`.
q|k|v and gate|up are packed the way the tokenizer packs its projections: the nn.Parameters keep their names and shapes,
their storage becomes a view of one buffer, so the stock modules keep working on them.

Phi-3 layers (`Phi3Attention.qkv_proj`, `Phi3MLP.gate_up_proj`: gate rows first, then up) already hold that packed layout and
are used as they are (`_PackedLayout`).  Their configs carry `sliding_window` = W (every Phi-3-4k build: 2047; query i sees
keys i - W + 1 .. i): a prefill of S <= W positions is the plain causal one, a longer prefill takes the stock layers (with
`continued`: the band inside the attention kernel), and a decode step attends over the last min(T, W) cached positions -- of a
plain DynamicCache, the append-in-place layer or the DynamicSlidingWindowLayer that `generate` builds for such a config.

`route` decides once per call which forward a patched layer takes: the opt-in training route of decoder_train.py, the decode
step, the prefill or the stock forward.  The patch state is one `_LayerState` per layer and one `_StackState` per decoder stack.

The cache-kind rule, once: WHAT a call's cache layer is, is `kv_cache.layer_kind`'s answer and nobody else's; the cache layers and
`_KVWrite` (where a step's rows go: T0, the first position of a window, the buffers, the commit) live in kv_cache.py and know no
switch.  WHICH kinds a call may take is decided here: `route` (the decode step: filled 16-bit layers, codes with kv8; the continued
prefill: those, nothing cached yet, codes with kv8_continued; the caps on a group's query heads and KV8_EXTEND_MAX_ROWS), which
leaves its answer on the layer's state for the step, and `stack_route` (one in-place kind for every layer; codes with stack_kv8).
The steps branch on that kind alone; what the whole-stack step does differently on codes is one record (`_STACK_KINDS`).
"""
from __future__ import annotations

import ctypes as C
import types
from collections import namedtuple
from dataclasses import dataclass, field
from typing import NamedTuple, Optional

import torch

from . import _lib, decoder_train, ops
from .kv_cache import (APPEND, APPEND_OTHER, DENSE, EMPTY, KERNEL_DTYPES, KERNEL_HEAD_DIMS, KV8, LAZY, NO_CACHE, SLIDING,  # noqa: F401
                       Kv8Layer, _append_layer_class, _KVWrite, _plain_layers, _prefill_append_layer, kv8_cache, layer_kind, window_first)
from .lora import _HOOK_TABLES, adapter_of, base_only_of, dropout_inactive

# What the kernels compute, per route: element types and head dims of the prefill / decode kernels, and of the backward
# kernels the training route needs (bf16 only; head dim 96 -- the flash backward's <96> kernels behind
# u2tok_attention_gqa_bwd_d96 -- with the train_phi3 switch, which also admits the packed Phi-3 layout)
INFER_DTYPES, INFER_HEAD_DIMS = KERNEL_DTYPES, KERNEL_HEAD_DIMS
TRAIN_DTYPES, TRAIN_HEAD_DIMS = (torch.bfloat16,), (64, 128)
TRAIN_PHI3_HEAD_DIMS = (64, 96, 128)


class Switch(NamedTuple):
    """One route switch: the keyword of `enable_fused_prefill`, the field of `_StackState` it sets (None: no state), the config
    attribute of a u2 causal LM that sets it (None: keyword only), its default, the keywords it implies, the keywords it does
    nothing without (the config attribute turns those on with it, the keyword does not), the fields of `_LayerState` that are
    dropped when it goes off, and what it does."""
    kw: str
    field: Optional[str]
    config: Optional[str]
    default: bool
    implies: tuple
    needs: tuple
    frees: tuple
    doc: str


SWITCHES = (
    Switch("decode", "decode", None, True, (), (), (), "the fused decode step (off: decode steps take the stock layers)"),
    Switch("strict", None, None, True, (), (), (),
           "refuse a decoder layer of another layout, or a Phi-3 layer the kernels do not compute (another activation, partial "
           "rotary, a head dim outside 64 / 96 / 128); off: such a layer is skipped and stays stock"),
    Switch("train", "train", "u2_fused_decoder_training", False, (), (), (),
           "a Llama / Qwen3 layer called with grad enabled takes the training route of decoder_train.py (head dims 64 / 128)"),
    Switch("prefill", "prefill", "u2_fused_prefill", True, (), (), (),
           "the fused prefill and decode step (off: the layers are patched for the training route only)"),
    Switch("padded", "padded", "u2_fused_padded_batches", False, (), (), (),
           "a LEFT- or RIGHT-padded batch (`pad_rule`) keeps the fused prefill, a left-padded one the fused decode step too -- what "
           "`generate` on prompts of different lengths calls; off, any mask with a zero sends the call to the stock layers"),
    Switch("continued", "continued", "u2_fused_continued_prefill", False, (), (), (),
           "more than one new position against a filled cache (a second turn, a prompt fed in chunks, `generate(..., "
           "past_key_values=cache)`, the verification step of assisted decoding) and a prefill longer than the window of a "
           "sliding-window layer stay on the HIP layers (u2tok_attention_gqa_band)"),
    Switch("fp8_decode", "fp8", "u2_fused_decode_fp8", False, (), (), ("w8",),
           "a layer whose E, Hq D and I are multiples of 64 runs the decode step's four products on e4m3 copies of its weights with "
           "one fp32 scale per row: half the weight bytes per step, half the layer's weights again in HBM; exact on the quantised "
           "weights, the quantiser's cost in accuracy is unmeasured on trained weights; `w8_stats`, `w8_weights(layer)`"),
    Switch("train_phi3", "train_phi3", "u2_fused_phi3_training", False, (), ("train",), (),
           "with `train`: the training route also takes head dim 96 (either layout) and the packed Phi-3 layout at head dims 64 / 96 / 128; a layer "
           "with a window W trains while the call has S <= W positions"),
    Switch("wide_decode", "wide", "u2_fused_wide_decode", False, (), (), (),
           "a decode step of 17 .. 64 sequences keeps the fused step (at most 16 query heads per kv head: always the batched decode "
           "attention; a left-padded one still needs `padded`); the weights are streamed once per step, each block of 16 sequences "
           "gets the bits of a step of its own (csrc/rows.h); `wide_stats`"),
    Switch("train_lora", "train_lora", "u2_fused_lora_training", False, ("train",), (), (),
           "the training route also takes LoRA-wrapped projections (`lora.adapter_of` lists what qualifies) and adds the adapter "
           "branch on the rank-r kernels of csrc/lora.hip; the no-grad routes stay as they are; `decoder_train.lora_stats`"),
    Switch("lora", "lora", "u2_fused_lora_inference", False, (), (), ("lora", "ads"),
           "the prefill, the continued prefill and the decode step take LoRA-wrapped projections with the adapters UNMERGED (a "
           "dropout that is the identity in the call; a merged or disabled wrapper counts as its base layer); `lora_stats`"),
    Switch("fp4_decode", "fp4", "u2_fused_decode_fp4", False, (), (), ("w4",),
           "a layer whose E, Hq D and I are multiples of 128 runs the decode step's four products on MXFP4 copies of its weights "
           "(OCP e2m1 codes, one power-of-two scale per block of 32): a quarter of the weight bytes per step, a quarter of the "
           "layer's weights again in HBM; exact on the quantised weights, the quantiser's cost in accuracy is unmeasured on trained "
           "weights; with `fp8_decode` as well a layer takes e2m1 where it qualifies, else e4m3 where it qualifies, else 16 bits; "
           "`w4_stats`, `w4_weights(layer)`"),
    Switch("stack_decode", "stack", "u2_fused_stack_decode", False, (), (), (),
           "a decode step the fused step would take layer by layer runs as ONE library call for the whole decoder stack "
           "(u2tok_decoder_decode_stack: the per-layer calls' launches in their order, the same bits, no Python between the "
           "layers; `stack_route` lists what it asks, everything else keeps the per-layer routes); `stack_stats`"),
    Switch("head", "head", "u2_fused_decode_head", False, ("stack_decode",), (), (),
           "a whole-stack step of a causal LM called without labels also runs its head -- the stack's final RMSNorm and lm_head, "
           "fp32 logits -- in the same library call (u2tok_decoder_decode_stack_head); `head_route` lists what it asks, every other "
           "call runs the module norm and nn.Linear as before; `config.u2_fused_head_form` (\"elem\", \"fp8\", \"fp4\") picks lm_head's "
           "weight form, the quantised ones unmeasured in accuracy on trained weights; `head_stats`"),
    Switch("stack_kv8", "stack8", "u2_fused_stack_kv_fp8", False, ("stack_decode", "kv8"), (), (),
           "a decode step on a cache of filled `Kv8Layer`s runs as ONE library call for the whole stack as well "
           "(u2tok_decoder_decode_stack_kv8; with `head`, u2tok_decoder_decode_stack_head_kv8): the rotary kernel writes the step's "
           "rows into the layers' buffers as codes (u2tok_qk_norm_rope_kv8), so a layer has as many launches as on the 16-bit "
           "stack step, and every hidden row, code, scale and logit has the bits of the per-layer step on that cache; every layer "
           "of the cache must be a filled `Kv8Layer` of this batch on the GPU with at most 16 query heads per kv head -- a cache "
           "that mixes them with append-in-place layers keeps the per-layer routes, which keep their two-launch quantiser; the "
           "continued prefill on codes and 17 .. 64 sequences are as `kv8_continued` and `wide_decode` have them; "
           "`stack_kv8_stats`"),
    Switch("kv8_continued", "kv8x", "u2_fused_kv_fp8_continued", False, ("kv8", "continued"), (), (),
           "more than one new position against a filled `Kv8Layer` stays on the HIP layers: the new rows are quantised into the "
           "layer's buffers and the new queries attend over the codes, the new rows' included (u2tok_attention_kv8_rows: 16 rows "
           "of (position, query head) per workgroup, so the cache is read once per 16 such rows -- the form for few new positions; "
           "at most 16 query heads per kv head; a call of more than `KV8_EXTEND_MAX_ROWS` positions stays stock); what the cache "
           "holds defines the semantics, as on the stock route; left-padded continuations with `padded`; the whole-stack and head "
           "calls on such a cache are `stack_kv8`'s, decode steps only; `kv8_extend_stats`"),
    Switch("kv8", "kv8", "u2_fused_kv_fp8", False, (), (), (),
           "the KV cache a fused prefill starts is FP8: a `Kv8Layer` (e4m3 codes, one fp32 scale per cached row of K and of V: half "
           "the cache's bytes in HBM and per decode step) where the append-in-place layer would go; the prefill commits through the "
           "layer's `update`, the decode step quantises its new rows and attends over the codes (u2tok_decoder_decode_post_kv8: "
           "always the batched decode attention, so at most 16 query heads per kv head); the continued prefill refuses the layer "
           "(stock layers on the dequantised cache) and the whole-stack and head calls keep off such a cache (`stack_route` answers "
           "\"layers\", `head_route` \"stock\") unless `stack_kv8` is on; exact on the quantised cache, the quantiser's cost in "
           "accuracy is unmeasured on trained weights; `kv8_stats`.  `kv8_continued` keeps the continued prefill on the codes as well"),
)

# layer calls per route of the no-grad routes (as decoder_train.stats / loss_head.stats: a route that fell back to the stock layers
# would pass every parity check); the padded counts are the calls whose mask carried a key range
stats = {"prefill": 0, "decode": 0, "padded_prefill": 0, "padded_decode": 0}
# ... and of the continued prefill (new positions against a filled cache, or a prefill past the window), in a dict of its own:
# `stats` keeps exactly its four routes
extend_stats = {"extend": 0, "padded_extend": 0}
# ... and the decode steps (counted in `stats` as well) that really ran on e4m3 weights (fp8_decode)
w8_stats = {"decode": 0, "padded_decode": 0}
# ... and those that ran on e2m1 weights (fp4_decode); a step moves the counter of the one form it ran in
w4_stats = {"decode": 0, "padded_decode": 0}
# ... and the decode steps (counted in `stats` as well) of more than 16 sequences (wide_decode), per layer call
wide_stats = {"decode": 0, "padded_decode": 0}
# ... and the layer calls of the no-grad routes (counted above as well) that computed at least one unmerged adapter (lora), per
# route, and the adapters they computed
lora_stats = {"prefill": 0, "extend": 0, "decode": 0, "adapters": 0}
# ... and the MODEL calls that ran as one whole-stack step (stack_decode); their layers are counted above as decode steps as well
stack_stats = {"decode": 0, "padded_decode": 0}
# ... and the causal-LM calls while the head switch is on: "head" took the step with the head, "fallback" ran the module norm and
# nn.Linear (`head_route` said no), "form_fallback" the head-route calls whose requested weight form the shape does not take (they ran
# on the element type)
head_stats = {"head": 0, "fallback": 0, "form_fallback": 0}
# ... and the decode steps (counted in `stats` as well) that ran on an e4m3 KV cache (kv8), per layer call
kv8_stats = {"decode": 0, "padded_decode": 0}
# ... and the continued prefills (counted in `extend_stats` as well) that attended over the codes of such a cache (kv8_continued)
kv8_extend_stats = {"extend": 0, "padded_extend": 0}
# ... and the MODEL calls (counted in `stack_stats` as well) that ran as one whole-stack step on such a cache (stack_kv8); their layers
# are counted in `stats` and `kv8_stats` as decode steps
stack_kv8_stats = {"decode": 0, "padded_decode": 0}
# the longest call (new positions per sequence) the continued prefill on an e4m3 cache takes, None: no cap.  The kernel streams the
# cache once per 16 rows of (position, query head), so a long call could lose to the stock route's one dequantisation; the value is
# the measurement's verdict (DESIGN f15: faster than the stock route at every measured length up to 1024, so no cap)
KV8_EXTEND_MAX_ROWS = None
# whether the whole-stack step asks for its three RMSNorms in the tail of the product before them (u2tok_gemm_rows_norm): the same
# bits either way; the default is the measurement's verdict (DESIGN f12)
STACK_TAIL_NORM = False


class _QForm(NamedTuple):
    """One quantised weight form of the decode step: its number (csrc/kernels.h: WForm), the `_StackState` field of its switch,
    the `_LayerState` field that holds a layer's copies, what E, Hq D and I must be multiples of, the quantiser (a 2-D weight -> a
    (codes, scales) pair), the counters of the steps that ran in it, and what u2tok_decode_config.wform says for it (None: the
    step's own config, wform 0 -- the four scales being set says e4m3)."""
    form: int
    switch: str
    copies: str
    multiple: int
    quantise: object
    stats: dict
    wform: Optional[int]


# in order of precedence: a layer takes the first form that is switched on and that it qualifies for, else the element type (form 0)
_QFORMS = (_QForm(2, "fp4", "w4", 128, ops.quantize_blocks_fp4, w4_stats, 2),
           _QForm(1, "fp8", "w8", 64, ops.quantize_rows_fp8, w8_stats, None))
_QFORM_OF = {q.form: q for q in _QFORMS}

# the kinds of cache layer the 16-bit steps take (sliding layers and codes: see `route`)
_DECODE_KINDS = (DENSE, APPEND, APPEND_OTHER)
_EXTEND_KINDS = _DECODE_KINDS + (NO_CACHE, LAZY, EMPTY)
_NO_PAD = ("none", None, None)   # the mask verdict of a call without padding (`pad_rule`, `_mask_hook`): compared by identity first


def _count(st, how: str, B: int, codes: bool = False, whole: bool = False) -> None:
    """One routed layer call (how: "prefill", "extend" or "decode") in the dicts above.  codes: it writes and reads an e4m3 cache
    layer in place (kind KV8); whole: it is the first layer of a whole-stack step, which is counted with it."""
    stack = st.stack
    pad = stack.pad   # (a routed call: the verdict is a tuple)
    key = how if pad is _NO_PAD or pad[0] == "none" else "padded_" + how
    if codes:
        (kv8_extend_stats if how == "extend" else kv8_stats)[key] += 1
    if whole:
        stack_stats[key] += 1
        if codes:
            stack_kv8_stats[key] += 1
    (extend_stats if how == "extend" else stats)[key] += 1
    if how == "decode" and (B > 16 or stack.fp8 or stack.fp4):
        for q in _QFORMS:   # (`_weight_form`: a layer keeps the copies of one form)
            if getattr(stack, q.switch) and getattr(st, q.copies) is not None:
                q.stats[key] += 1
                break
        if B > 16:
            wide_stats[key] += 1
    if st.ads is not None:
        lora_stats[how] += 1
        lora_stats["adapters"] += sum(a is not None for a in st.ads)


def pad_rule(mask):
    """What the fused inference routes make of a call's 2-D attention mask (next to decoder_train.train_mask_rule):
    ("none", None, None) for no mask or all ones; ("right", None, kv_len) when every row is ones then zeros; ("left", kv_start,
    None) when every row is zeros then ones -- at least one one per row, kv_start / kv_len int32 (B,) on the mask's device: key j
    of sequence b is visible iff kv_start[b] <= j < kv_len[b] --; None (stock layers) for holes, an empty row, padding on both
    sides or a mask that is not 2-D.  One host synchronisation (four flags in one transfer), none without a mask."""
    if mask is None:
        return _NO_PAD
    if not torch.is_tensor(mask) or mask.dim() != 2 or mask.shape[1] == 0:
        return None
    m = mask != 0
    S = m.shape[1]
    n = m.sum(1)
    pos = torch.arange(S, device=m.device)
    first = torch.where(m, pos, S).amin(1)          # first / last one of each row (S / -1: an empty row)
    last = torch.where(m, pos, -1).amax(1)
    whole = (n > 0) & (last - first + 1 == n)         # one run of ones, no holes
    full, runs, at0, at_end = torch.stack((n.eq(S).all(), whole.all(), first.eq(0).all(), last.eq(S - 1).all())).tolist()
    if full:
        return _NO_PAD
    if not runs:
        return None
    if at0:
        return "right", None, (last + 1).to(torch.int32)
    if at_end:
        return "left", first.to(torch.int32), None
    return None


def _pack(linears):
    """Lay the weights (and biases, if any) of `linears` back to back in one buffer; returns (W, b | None)."""
    linears = [getattr(lin, "base_layer", lin) for lin in linears]   # (an adapter-wrapped projection: its base layer)
    ws = [lin.weight for lin in linears]
    es = ws[0].element_size()
    st0 = ws[0].untyped_storage()
    adjacent = all(w.is_contiguous() and w.untyped_storage().data_ptr() == st0.data_ptr() for w in ws) and all(
        ws[i + 1].data_ptr() == ws[i].data_ptr() + ws[i].numel() * es for i in range(len(ws) - 1))  # (one storage: neighbours
    # in two allocations are not a packed buffer)
    if not adjacent:
        W = torch.cat([w.data for w in ws], 0).contiguous()
        o = 0
        for w in ws:
            w.data = W[o:o + w.shape[0]]
            o += w.shape[0]
    W = ws[0].data.as_strided((sum(w.shape[0] for w in ws), ws[0].shape[1]), (ws[0].shape[1], 1))
    b = None
    if all(lin.bias is not None for lin in linears):
        b = torch.cat([lin.bias.data for lin in linears], 0).contiguous()  # (biases are tiny: a copy, refreshed per call)
    elif any(lin.bias is not None for lin in linears):
        raise RuntimeError("mixed bias / no-bias projections cannot be packed")
    return W, b


_scratch = {}


def _ensure_gemm_scratch(device) -> None:
    """Split-K scratch of the calling stream (at S = 1024 the out projection is 256 tiles of 128 x 128: cut in two along K it puts
    two workgroups on every CU; q|k|v and the down projection take the big-tile kernel in 2 / 4 K slices, gemm_bt.hip:
    bt_pick_sliced), registered on the active context like the training path's."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, id(ops.active_context(device)))
    if key not in _scratch:
        buf = torch.empty(72 << 20, dtype=torch.uint8, device=device)  # 4 slices of (1024, 4096) fp32 sums + slack
        with torch.cuda.device(device):
            ops.set_gemm_scratch(buf)
        _scratch[key] = buf


def _base(lin):
    """The nn.Linear whose weight and bias a projection's product reads: the module, or an adapter wrapper's base layer."""
    return getattr(lin, "base_layer", lin)


class _Layout:
    """A decoder layer's projections as the four products read them.  GROUPS: the projections (indices into `projections(layer)`)
    of q|k|v, o, gate|up and down; everything else about the products follows from it (`product`)."""
    GROUPS = ()

    @classmethod
    def product(cls, pr, g: int):
        """Product g (0: q|k|v, 1: o, 2: gate|up, 3: down) of the projections `pr` -> (its modules, W, b): one module's own
        weight and bias, several modules' packed ones (`_pack`)."""
        idx = cls.GROUPS[g]
        if len(idx) == 1:
            m = pr[idx[0]]
            lin = getattr(m, "base_layer", m)   # (`_base`, written out: four calls per layer call on the host-bound steps)
            return (m,), lin.weight, lin.bias
        lins = pr[idx[0]:idx[-1] + 1]           # (the projections of one product are neighbours in `projections`)
        return (lins, *_pack(lins))

    @staticmethod
    def window(layer):
        return None


class _SplitLayout(_Layout):
    """Llama / Qwen3: separate q / k / v and gate / up projections, packed into one buffer each on first use."""
    GROUPS = ((0, 1, 2), (3,), (4, 5), (6,))
    TRAINS = True        # the training route computes this layout

    @staticmethod
    def projections(layer):
        att, mlp = layer.self_attn, layer.mlp
        return (att.q_proj, att.k_proj, att.v_proj, att.o_proj, mlp.gate_proj, mlp.up_proj, mlp.down_proj)

    @staticmethod
    def ready(layer, att) -> bool:
        return getattr(att, "sliding_window", None) is None


class _PackedLayout(_Layout):
    """Phi-3: one qkv_proj (q, k, v rows) and one gate_up_proj (gate rows, then up rows) -- the packed layout itself."""
    GROUPS = ((0,), (1,), (2,), (3,))
    TRAINS = False       # ... and this one only with the train_phi3 switch (route)

    @staticmethod
    def projections(layer):
        return (layer.self_attn.qkv_proj, layer.self_attn.o_proj, layer.mlp.gate_up_proj, layer.mlp.down_proj)

    @staticmethod
    def window(layer):
        return getattr(layer.self_attn.config, "sliding_window", None)   # (Phi3Attention has no attribute of its own)

    @staticmethod
    def ready(layer, att) -> bool:
        """No dropout that the fused forward would skip (training mode with resid_pdrop / attention_dropout > 0), weights as
        one dense matrix each."""
        for m in (layer.resid_attn_dropout, layer.resid_mlp_dropout):
            if m.training and m.p > 0:
                return False
        if att.training and att.attention_dropout > 0:
            return False
        return att.qkv_proj.weight.is_contiguous() and layer.mlp.gate_up_proj.weight.is_contiguous()

    @staticmethod
    def supported(layer) -> bool:
        """What the kernels compute: SiLU gate, rotary over the whole head (no partial_rotary_factor < 1, as in Phi-4-mini),
        head dim 64 / 96 / 128 (Phi-3-mini / -3.5-mini: 96, Phi-3-medium: 128)."""
        att = layer.self_attn
        cfg = att.config
        rp = getattr(cfg, "rope_parameters", None) or {}
        prf = rp.get("partial_rotary_factor", getattr(cfg, "partial_rotary_factor", 1.0))
        return (getattr(cfg, "hidden_act", None) == "silu" and float(prf if prf is not None else 1.0) == 1.0
                and att.head_dim in INFER_HEAD_DIMS)


def _layout_of(layer):
    """_SplitLayout / _PackedLayout for a decoder layer of a layout the fused forward runs, else None."""
    if not all(hasattr(layer, a) for a in ("self_attn", "mlp", "input_layernorm", "post_attention_layernorm")):
        return None
    att, mlp = layer.self_attn, layer.mlp
    if not all(hasattr(att, a) for a in ("o_proj", "head_dim", "scaling")) or not hasattr(mlp, "down_proj"):
        return None
    if all(hasattr(att, a) for a in ("q_proj", "k_proj", "v_proj")) and all(hasattr(mlp, a) for a in ("gate_proj", "up_proj")):
        return _SplitLayout
    if hasattr(att, "qkv_proj") and hasattr(mlp, "gate_up_proj") and hasattr(att, "config") \
            and hasattr(layer, "resid_attn_dropout") and hasattr(layer, "resid_mlp_dropout") and _PackedLayout.supported(layer):
        return _PackedLayout
    return None


_HOOKS_F, _HOOKS_FP, _HOOKS_B, _HOOKS_BP = _HOOK_TABLES


def _admit(layer, projections, lora: bool, grad: bool):
    """Whether the projections are what the call's route computes.  The fused forwards read the projections' `.weight` / `.bias`
    and never CALL the submodules.  That is only the same computation while every projection is exactly torch.nn.Linear and
    nothing hangs on the modules that are skipped: a peft lora.Linear exposes `.weight` as its BASE weight (the reference trains
    the decoder with LoRA, train_stage1.py:342-353: an unmerged adapter would be silently ignored), forward hooks
    (output_attentions recorders, activation probes) would not fire.  Checked on every call: adapters and hooks come and go after
    enable_fused_prefill (module attribute reads are what this costs per layer and step).
    lora (the call's switch: train_lora with grad, lora without) decides what else a projection may be: with grad an adapter the
    training route computes (lora.adapter_of: the layout of peft's lora.Linear, read attribute by attribute); without grad also a
    wrapper that computes its base layer alone (lora.base_only_of: merged or disabled, DPO's null-reference pass), and the
    adapter's dropout must be the identity in this call (peft applies dropout in train mode even under no_grad).
    -> the lora.Adapter per projection (None for a plain or base-only one; () when there is none at all), or None: the stock
    forward (hooks, rank outside RANKS, DoRA and the other variants, more than one active adapter, an unreadable attribute,
    active dropout)."""
    ads = ()
    for m in projections:
        if type(m) is torch.nn.Linear:
            continue
        a = adapter_of(m) if lora else None
        if a is None:
            if not lora or grad or base_only_of(m) is None:
                return None
            continue
        if not grad and not dropout_inactive(a.dropout):
            return None
        ads = ads or [None] * len(projections)
        ads[projections.index(m)] = a
    for m in (*projections, layer.self_attn, layer.mlp, layer.input_layernorm, layer.post_attention_layernorm):
        d = m.__dict__   # (nn.Module keeps its hook tables as instance attributes; 44 lookups per layer call, a third of the
        #                   Python of a decode step: no inner loop)
        if d.get(_HOOKS_F) or d.get(_HOOKS_FP) or d.get(_HOOKS_B) or d.get(_HOOKS_BP):
            return None
    return ads and tuple(ads)


@dataclass(slots=True, eq=False)
class _StackState:
    """enable_fused_prefill's state on a decoder stack: the route switches (SWITCHES), the pre-hook's verdict on the call's 2-D
    mask, the hook, and the decode steps' scratch ((B, device, stream) -> buffers)."""
    hook: object
    decode: bool = True
    train: bool = False
    train_phi3: bool = False
    train_lora: bool = False
    prefill: bool = True
    padded: bool = False
    continued: bool = False
    fp8: bool = False
    wide: bool = False
    lora: bool = False
    fp4: bool = False
    stack: bool = False
    head: bool = False
    stack8: bool = False
    kv8x: bool = False
    kv8: bool = False
    pad: tuple = _NO_PAD      # the verdict on the call's mask: pad_rule's (kind, kv_start, kv_len), or None = stock (`_mask_hook`)
    pad_shape: tuple = None    # ... and, for a mask with a key range, its (B, columns)
    scratch: dict = field(default_factory=dict)

    @property
    def mask_ok(self) -> bool:
        """No mask, or all ones."""
        return self.pad is not None and self.pad[0] == "none"


@dataclass(slots=True, eq=False)
class _LoraOps:
    """A layer's unmerged adapters as the kernels read them (`_lora_state`): per product (q|k|v, o, gate|up, down) the segments
    (A16 (r, K), B16 (N, r), col0, scaling) of its wrapped projections, their number, and for the decode step the
    u2tok_decode_lora built from them with the workspace bytes it needs per batch size."""
    key: tuple
    groups: tuple
    n: int
    desc: object = None
    need: dict = field(default_factory=dict)


@dataclass(slots=True, eq=False)
class _LayerState:
    """A patched layer: its original forward, its stack's state, its layout, and what the decode step keeps between calls: the
    16-bit descriptor (`dec`), the optional e4m3 pairs (`w8`), the optional e2m1 pairs (`w4`), the optional adapter operands
    (`lora`) and the DecodeLayer variants built from them (`variants`: one per (weight form, with adapters) that a step has asked
    for -- `_decode_layer`), dropped together (`_drop_variants`) whenever one of the four sources is rebuilt.  The ctypes
    structs and the references handed to the library live here."""
    orig: object
    stack: _StackState
    layout: type
    ads: tuple = None          # lora: the call's adapters per projection (`_admit`, set by route() for the step that follows)
    kind: object = None        # `layer_kind`'s answer for the call's cache layer (set by route(), taken by the step that follows)
    dec: object = None         # `_Decode16`
    w8: tuple = None           # fp8_decode: (key, the four (W8, scale) pairs)
    lora: _LoraOps = None
    variants: dict = field(default_factory=dict)   # (form, lora) -> `_decode_layer`'s tuple
    w4: tuple = None           # fp4_decode: (key, the four (codes, block scales) pairs)


def _drop_variants(st) -> None:
    st.variants.clear()


def is_patched(layer) -> bool:
    """True while enable_fused_prefill's forward is installed on `layer`."""
    return "_u2_prefill" in layer.__dict__


def _rows(x):
    return x.reshape(-1, x.shape[-1]).contiguous()   # (B, S, E) -> dense (B S, E) rows (no copy when they are already)


def _rotary_rows(pe, B: int, S: int, d: int, elem=None):
    """`position_embeddings` as (B S, d) rows of cos and sin.  With `elem` (decode, training): tables the kernels do not read as
    they are (two types, neither fp32 nor `elem`, rows not unit stride or not of one stride) become fp32 copies."""
    cos, sin = pe
    cos, sin = cos.expand(B, S, d).reshape(B * S, d), sin.expand(B, S, d).reshape(B * S, d)
    if elem is not None and (cos.dtype != sin.dtype or cos.dtype not in (torch.float32, elem) or cos.stride(1) != 1
                             or sin.stride(1) != 1 or cos.stride(0) != sin.stride(0)):
        cos, sin = cos.float().contiguous(), sin.float().contiguous()
    return cos, sin


def route(layer, shape, dtype, is_cuda: bool, args, kwargs, grad: bool, pr):
    """The forward a call of the patched `layer` takes, from the input's shape, dtype and device flag (no tensor needed):
    ("train", kv_len) or stock with grad enabled, else ("decode", W), ("prefill", W), ("extend", W) or stock; W = the attention
    window or None.  "extend" (stack.continued, opt-in): more than one position that the plain prefill refuses -- the layer's
    cache already holds positions, or the call is longer than the window -- with a cache layer of a kind the continued prefill takes (`kv_cache.layer_kind`).  Masks: decode,
    prefill and extend read the stack pre-hook's verdict on the call's 2-D mask, the training route the layer's own 4-D mask (layer_mask_kv_len: cached on the tensor, so a checkpoint recompute sees its own forward's).  `pr`: the
    layout's projections (read once per call)."""
    st = layer._u2_prefill
    stack, lo, att = st.stack, st.layout, layer.self_attn
    st.ads = st.kind = None
    if not (stack.train if grad else stack.prefill):
        return "stock", None
    pe = kwargs.get("position_embeddings")
    # every route: no `past_key_value` (singular: the 4.46 .. 4.5x protocol, never patched), a (B, S >= 1, E) GPU input in the
    # weights' type (bf16 weights under an fp16 autocast hand fp16 activations on), projections the route computes, no hooks
    if args or "past_key_value" in kwargs or kwargs.get("output_attentions") or not is_cuda or len(shape) != 3 \
            or shape[1] < 1 or pr[0].weight.dtype != dtype or pe is None or pe[0].shape[-1] != att.head_dim:
        return "stock", None
    ads = _admit(layer, pr, stack.train_lora if grad else stack.lora, grad)
    if ads is None or not lo.ready(layer, att):
        return "stock", None
    if grad:
        # a layout and a head dim the route computes (train_phi3: the packed Phi-3 layout and head dim 96 too), no KV cache, no
        # active attention dropout, widths the row kernels take, no more positions than the attention window, a mask the
        # attention computes
        phi3 = stack.train_phi3
        if not (lo.TRAINS or phi3) or dtype not in TRAIN_DTYPES \
                or att.head_dim not in (TRAIN_PHI3_HEAD_DIMS if phi3 else TRAIN_HEAD_DIMS) or kwargs.get("past_key_values") \
                is not None or (att.training and float(getattr(att, "attention_dropout", 0.0) or 0.0) > 0) \
                or shape[2] % 8 or shape[2] > 4096 or _base(pr[lo.GROUPS[3][0]]).weight.shape[1] % 8 \
                or layer.input_layernorm.weight.dtype not in TRAIN_DTYPES:
            return "stock", None
        W = lo.window(layer)
        if W is not None and shape[1] > W:   # (a call longer than the window: the band is not in the backward kernels)
            return "stock", None
        ok, kv_len = decoder_train.layer_mask_kv_len(kwargs.get("attention_mask"), shape[0], shape[1])
        return ("train", kv_len) if ok else ("stock", None)
    if ads:
        st.ads = ads   # (the step that follows computes them; no adapter at all: the base layers alone)
    if dtype not in INFER_DTYPES or att.head_dim not in INFER_HEAD_DIMS:
        return "stock", None
    W = lo.window(layer)
    cache = kwargs.get("past_key_values")
    pad = stack.pad
    ranged = pad is not _NO_PAD and (pad is None or pad[0] != "none")   # a padded call: "left" / "right" when the kernels take its key ranges
    if ranged:
        # a mask with zeros: stock, unless the padded routes are on, the mask is one run of ones per row as wide as this call's
        # keys (prefill: S columns, decode: cache + 1) and the layer has no attention window
        if pad is None or not stack.padded or W is not None or stack.pad_shape[0] != shape[0]:
            return "stock", None
        kind = pad[0]
        keys = shape[1] + (cache.get_seq_length(att.layer_idx) if cache is not None else 0)
        if stack.pad_shape[1] != keys or (shape[1] == 1 and kind != "left"):
            return "stock", None
        if keys != shape[1] and kind != "left":   # (a right-padded continuation: the new keys would not follow the old ones)
            return "stock", None
    if shape[1] == 1:   # one new position per sequence, batch <= 16 (wide_decode=True: <= 64), against a plain DynamicCache
        wide = shape[0] > 16   # (17 .. 64 sequences: the few-rows product on up to four blocks of 16 rows, always the batched attention)
        kind, lay = layer_kind(cache, att.layer_idx, shape[0])
        st.kind = kind
        # a filled 16-bit layer of a plain cache (sliding: under a window); kv8: codes the kernels take, always the batched attention
        ok = (shape[0] <= 64 and stack.wide if wide else True) and stack.decode and (
            kind in _DECODE_KINDS or (kind is KV8 and stack.kv8) or (kind is SLIDING and W is not None and lay.get_seq_length() > 0))
        if (ranged or wide or kind is KV8) and att.config.num_attention_heads // att.config.num_key_value_heads > 16:
            ok = False  # (the batched decode attention holds a group's query heads in one 16-row operand)
        return ("decode", W) if ok else ("stock", None)
    # an empty cache and no more positions than the window: the plain causal prefill
    if (W is None or shape[1] <= W) and (cache is None or cache.get_seq_length(att.layer_idx) == 0):
        return "prefill", W
    # continued=True: the band and the cache's layout inside the attention kernel (u2tok_attention_gqa_band), for every layer of a
    # plain cache the step can write; kv8_continued: codes the kernels take as well (u2tok_attention_kv8_rows, the two caps)
    if stack.continued:
        kind = st.kind = layer_kind(cache, att.layer_idx, shape[0])[0]
        if kind in _EXTEND_KINDS or (kind is SLIDING and W is not None) or (
                kind is KV8 and stack.kv8x and att.config.num_attention_heads // att.config.num_key_value_heads <= 16
                and (KV8_EXTEND_MAX_ROWS is None or shape[1] <= KV8_EXTEND_MAX_ROWS)):
            return "extend", W
    return "stock", None


def _layer_forward(self, hidden_states, *args, **kwargs):
    st = self._u2_prefill
    x = hidden_states
    pr = st.layout.projections(self)
    shape = x.shape
    how, arg = route(self, shape, x.dtype, x.is_cuda, args, kwargs, torch.is_grad_enabled(), pr)
    if how == "decode":
        codes = st.kind is KV8
        out = _decode_step(self, x, kwargs["position_embeddings"], kwargs.get("past_key_values"), arg, pr)
        if out is not None:
            _count(st, how, shape[0], codes)
            return out
    elif how == "prefill" or how == "extend":
        _count(st, how, shape[0], st.kind is KV8)
        return _prefill_step(self, st.layout, x, kwargs["position_embeddings"], kwargs.get("past_key_values"), arg, how == "extend")
    elif how == "train":
        return _train_step(self, st.layout, x, kwargs["position_embeddings"], arg)
    return st.orig(hidden_states, *args, **kwargs)


def _train_step(layer, lo, x, pe, kv_len):
    """The training route (decoder_train.layer_forward_train) on the layer's rows and rotary tables."""
    B, S, _ = x.shape
    _ensure_gemm_scratch(x.device)
    with ops.on_device(x):
        cos, sin = _rotary_rows(pe, B, S, layer.self_attn.head_dim, x.dtype)
        return decoder_train.layer_forward_train(layer, lo, _rows(x), cos.detach(), sin.detach(), B, S, kv_len)


def _lora_add(y, x2, segs):
    """The adapter branch of one packed product on many rows, for its wrapped projections: u = rnd(x A^T) (u2tok_lora_down), then
    y[:, col0:col0 + N] = rnd(float(y) + scale u B^T) in place (u2tok_lora_up, accumulate form) -- the kernels and the rounding
    points of the training route (decoder_train.LoraDeltaFn)."""
    for A16, B16, col0, scale in segs:
        u = ops.lora_down(x2, A16)
        ops.lora_up(u, B16, y[:, col0:col0 + B16.shape[0]], alpha=scale, accumulate=True)


def _prefill_step(self, lo, x, pe, cache, window=None, extend=False):
    """The prefill step of a layer.  extend (the "extend" route): the S new positions attend over a cache layer that holds T0 > 0
    -- the band form reads K / V where the cache keeps them (`_KVWrite.views`) --, or, with no position cached yet, the call is
    longer than `window` and its own keys get the band.  One attention entry: the C side picks the kernel form from which of
    window, kv_start (the first visible key of each sequence of a left-padded batch) and kv_len the call has; none of them is the
    plain causal kernel.  With unmerged adapters admitted for the call (the `lora` switch: st.ads) each of the four products is
    followed by its adapters' branch (`_lora_add`); the q|k|v branch precedes the rotary embedding, so the cache receives adapted
    keys and values.  The cache is committed once every launch of the layer is enqueued."""
    B, S, E = x.shape
    rows = B * S
    att = self.self_attn
    st = self._u2_prefill
    pr = lo.projections(self)
    g_qkv, g_o, g_gu, g_down = _lora_state(st, lo, pr, x.dtype, x.device).groups if st.ads is not None else ((), (), (), ())
    cfg = att.config
    Hq, Hkv, d = cfg.num_attention_heads, cfg.num_key_value_heads, att.head_dim
    _ensure_gemm_scratch(x.device)
    with ops.on_device(x):
        product = lo.product
        (_, Wqkv, bqkv), (_, Wo, bo), (_, Wgu, bgu), (_, Wdown, bdown) = product(pr, 0), product(pr, 1), product(pr, 2), product(pr, 3)
        x2 = _rows(x)
        cos, sin = _rotary_rows(pe, B, S, d)
        xn = ops.rmsnorm(x2, self.input_layernorm.weight, self.input_layernorm.variance_epsilon)
        qkv = ops.gemm(xn, Wqkv, bias=bqkv)
        _lora_add(qkv, xn, g_qkv)
        qn, kn = getattr(att, "q_norm", None), getattr(att, "k_norm", None)
        q3 = qkv.view(B, S, -1)
        _, kv_start, kv_len = st.stack.pad
        filled = extend and cache is not None and cache.get_seq_length(att.layer_idx) > 0
        kind, st.kind = st.kind, None   # (route()'s answer, where it routed this call)
        codes = kind is KV8       # an e4m3 cache (kv8_continued): the rotary kernel's new rows stay dense, `attend8` quantises them
        kv = _KVWrite(cache, att.layer_idx, B, S, window, like=x.new_empty((B, Hkv, 0, d)) if codes else None,
                      fresh=None if filled else (Hkv, d, x), kv8=st.stack.kv8, kind=kind)
        codes = kv.kind is KV8
        kv_out = kv.lay._buffers() if kv.kind is APPEND else None
        r = ops.qk_norm_rope(qkv, None if qn is None else qn.weight, None if kn is None else kn.weight, cos, sin, Hq, Hkv, d,
                             qn.variance_epsilon if qn is not None else 1e-6, kv_cache_seq=S if cache is not None else 0,
                             kv_out=kv_out, kv_pos=kv.T0)
        kc, vc = (r[1], r[2]) if cache is not None and kv_out is None else (None, None)
        if codes:   # over the codes, the quantised new rows included
            ctx = kv.attend8(q3[..., :Hq * d], kc, vc, Hq, float(att.scaling), kv_start)
        else:
            if filled:
                K, V, _ = kv.views(kc, vc)
            else:   # its own keys / values: columns of the q|k|v rows
                K, V = q3[..., Hq * d:(Hq + Hkv) * d], q3[..., (Hq + Hkv) * d:]
            # a padded batch: the key range of each sequence inside the kernel; padding rows come back as zeros.  extend: query i sees
            # its own key and the window - 1 before it
            ctx = ops.attention_gqa_band(q3[..., :Hq * d], K, V, Hq, Hkv, float(att.scaling), window=window if extend else None,
                                         kv_start=kv_start, kv_len=kv_len, causal=True)
        ctx2 = ctx.view(rows, Hq * d)
        h = ops.gemm(ctx2, Wo, bias=bo, residual=x2)
        _lora_add(h, ctx2, g_o)   # (after the residual epilogue: the same terms)
        hn = ops.rmsnorm(h, self.post_attention_layernorm.weight, self.post_attention_layernorm.variance_epsilon)
        if not g_gu and bgu is None and ops.gemm_swiglu_supported(rows, E, Wgu.shape[0] // 2):
            act = ops.gemm_swiglu(hn, Wgu)  # SiLU(gate) * up in the epilogue of the pair product: no (rows, 2 I) tensor
        else:   # (a gate or up adapter: its branch lands on the pair product before the SiLU)
            gu = ops.gemm(hn, Wgu, bias=bgu)
            _lora_add(gu, hn, g_gu)
            act = ops.swiglu(gu)
        out = ops.gemm(act, Wdown, bias=bdown, residual=h)
        _lora_add(out, act, g_down)
        kv.commit(kc, vc)
    return out.view(B, S, E)


@dataclass(slots=True, eq=False)
class _Decode16:
    """Per-layer constants of the decode step: the config struct, the 16-bit layer descriptor, the packed operands it points at."""
    key: tuple
    ok: bool
    cfg: object
    cfg_ref: object
    layer: object
    keep: tuple
    nq: int
    Hkv: int
    hd: int


def _decode_state(self, B: int, device, pr):
    """Per-layer constants of the decode step (weight pointers of the packed projections, the config struct), rebuilt when a
    weight moved or the batch size changed; per-model scratch (workspace, q|k|v row, new cache entries) shared by all layers."""
    st = self._u2_prefill
    lo = st.layout
    att = self.self_attn
    g = lo.GROUPS   # (the first projection of each product locates its buffer)
    key = (pr[g[0][0]].weight.data_ptr(), pr[g[1][0]].weight.data_ptr(), pr[g[2][0]].weight.data_ptr(), pr[g[3][0]].weight.data_ptr(), B)
    d = st.dec
    if d is None or d.key != key:
        cfg = att.config
        Hq, Hkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, att.head_dim
        product = lo.product
        (_, Wqkv, bqkv), (_, Wo, bo), (_, Wgu, bgu), (_, Wdown, bdown) = product(pr, 0), product(pr, 1), product(pr, 2), product(pr, 3)
        qn, kn = getattr(att, "q_norm", None), getattr(att, "k_norm", None)
        E, inter = Wqkv.shape[1], Wgu.shape[0] // 2
        c = _lib.DecodeConfig(B=B, E=E, Hq=Hq, Hkv=Hkv, D=hd, I=inter, eps=float(self.input_layernorm.variance_epsilon),
                              qk_eps=float(qn.variance_epsilon) if qn is not None else 1e-6, scale=float(att.scaling))
        ok = (E % 32 == 0 and inter % 32 == 0 and Wo.is_contiguous() and Wdown.is_contiguous()
              and self.post_attention_layernorm.variance_epsilon == self.input_layernorm.variance_epsilon)
        p = ops._ptr
        lay = _lib.DecodeLayer(w_in_norm=p(self.input_layernorm.weight), Wqkv=p(Wqkv), bqkv=p(bqkv),
                               wq_norm=p(None if qn is None else qn.weight), wk_norm=p(None if kn is None else kn.weight),
                               Wo=p(Wo), bo=p(bo), w_post_norm=p(self.post_attention_layernorm.weight),
                               Wgu=p(Wgu), bgu=p(bgu), Wdown=p(Wdown), bdown=p(bdown))
        d = st.dec = _Decode16(key, ok, c, C.byref(c), lay, (Wqkv, bqkv, Wgu, bgu), (Hq + 2 * Hkv) * hd, Hkv, hd)
        _drop_variants(st)
    # (per model, batch size AND stream: two generate() calls in flight on different streams must not share the step's scratch)
    stream = torch.cuda.current_stream(device).cuda_stream
    pool = st.stack.scratch
    edt = self.input_layernorm.weight.dtype      # bf16, or fp16 for a decoder loaded in float16 (the f16 build of the library)
    sc = pool.get((B, device, stream))
    if sc is not None and sc["qkv"].dtype != edt:
        sc = None
    if sc is None:
        if len(pool) >= 8:
            pool.clear()
        sc = {"B": B, "device": device, "ws": None, "T": 0,
              "qkv": torch.empty((B, d.nq), dtype=edt, device=device),
              "kc": torch.empty((B, d.Hkv, 1, d.hd), dtype=edt, device=device),
              "vc": torch.empty((B, d.Hkv, 1, d.hd), dtype=edt, device=device)}
        pool[(B, device, stream)] = sc
    return d, sc


def _quant_state(st, d, pr, q) -> bool:
    """The copies of a layer's four packed decode weights (q|k|v, o, gate|up, down) in the quantised form `q` -- fp8_decode: e4m3
    with a scale per row (ops.quantize_rows_fp8), half the layer's weights again in HBM; fp4_decode: MXFP4, e2m1 codes with an e8m0
    scale per block of 32 (ops.quantize_blocks_fp4), a quarter -- in the layer state's field `q.copies`; False for a layer the form
    does not take (E, Hq D or I not a multiple of `q.multiple`: the layer keeps the next form it qualifies for).  Built at the first
    qualifying step, rebuilt when a source weight's data_ptr() or _version changed (an optimiser step, load_state_dict,
    weight.mul_), freed with the patch state by disable_fused_prefill and when the switch goes off.  Parameters, state dict,
    prefill and training never see the copies; biases stay in the element type."""
    c = d.cfg
    if c.E % q.multiple or (c.Hq * c.D) % q.multiple or c.I % q.multiple:
        return False
    key = tuple((m.weight.data_ptr(), m.weight._version) for m in pr)
    have = getattr(st, q.copies)
    if have is None or have[0] != key:
        Wqkv, _, Wgu, _ = d.keep
        lo = st.layout
        setattr(st, q.copies, (key, tuple(q.quantise(w) for w in (Wqkv, lo.product(pr, 1)[1], Wgu, lo.product(pr, 3)[1]))))
        _drop_variants(st)
    return True


def _weight_form(st, d, pr) -> int:
    """The weight form of a layer's decode step under the stack's switches: the first of `_QFORMS` that is on and that the layer
    qualifies for -- 2 (e2m1) under fp4_decode, else 1 (e4m3) under fp8_decode --, else 0 (the element type).  Builds or refreshes
    the copies of the form it returns; copies of another form a layer once built are dropped, so `_count` sees the one that ran."""
    stack = st.stack
    if not (stack.fp4 or stack.fp8):
        return 0
    for q in _QFORMS:
        if getattr(stack, q.switch) and _quant_state(st, d, pr, q):
            for other in _QFORMS:
                if other is not q:
                    setattr(st, other.copies, None)
            return q.form
    return 0


def _op16(w, dtype, device):
    """An adapter weight as the kernels read it: itself when it already is a dense tensor of the element type on the device, else a
    16-bit compute copy (fp32 adapters: peft's default under autocast_adapter_dtype)."""
    w = w.detach()
    if w.dtype == dtype and w.device == device and w.is_contiguous():
        return w
    return w.to(device=device, dtype=dtype).contiguous()


def _lora_state(st, lo, pr, dtype, device) -> _LoraOps:
    """The call's unmerged adapters (st.ads: `_admit`) as the kernels read them, in st.lora -- the 16-bit compute copies of fp32
    adapters among them.  Rebuilt when an adapter weight's data_ptr() or _version, a scaling, the active adapter (its A / B modules)
    or a `merged` / `disable_adapters` flag (an entry of st.ads turning None) changed, and on nothing else: no step converts
    anything.  Freed with the patch state by disable_fused_prefill, and when the switch goes off."""
    ads = st.ads
    key = (dtype, device) + tuple(None if a is None else (id(a.A), a.A.weight.data_ptr(), a.A.weight._version, id(a.B),
                                                          a.B.weight.data_ptr(), a.B.weight._version, a.scaling, a.r) for a in ads)
    ls = st.lora
    if ls is None or ls.key != key:
        groups = []
        for idx in lo.GROUPS:
            col0, segs = 0, []
            for i in idx:
                a = ads[i]
                if a is not None:
                    segs.append((_op16(a.A.weight, dtype, device), _op16(a.B.weight, dtype, device), col0, a.scaling))
                col0 += _base(pr[i]).out_features
            groups.append(tuple(segs))
        ls = st.lora = _LoraOps(key, tuple(groups), sum(len(g) for g in groups))
        _drop_variants(st)
        lora_state_builds[0] += 1
    return ls


lora_state_builds = [0]   # how often `_lora_state` built its operands (tests: once per change, never per step)
_LORA_PRODUCTS = ("qkv", "o", "gu", "down")


def _lora_scratch(ls, B: int, sc, h) -> None:
    """Point the adapters' u2tok_decode_lora (built here on first use) at the calling stream's scratch for B rows: u, then the
    largest group workspace; shared by all layers like the step's other scratch."""
    desc = ls.desc
    if desc is None:
        desc = ls.desc = _lib.DecodeLora()
        for name, segs in zip(_LORA_PRODUCTS, ls.groups):
            for e, (A16, B16, col0, scale) in zip(getattr(desc, name), segs):
                e.A, e.B, e.r, e.col0, e.N, e.scale = A16.data_ptr(), B16.data_ptr(), A16.shape[0], col0, B16.shape[0], scale
            setattr(desc, "n_" + name, len(segs))
    need = ls.need.get(B)
    if need is None:
        need = ls.need[B] = _lib.DECODE_LORA_U_BYTES + max(
            h.u2tok_lora_rows_workspace_bytes(B, segs[0][0].shape[1], C.addressof(getattr(desc, name)), len(segs))
            for name, segs in zip(_LORA_PRODUCTS, ls.groups) if segs)
    buf = sc.get("lora")
    if buf is None or buf.numel() < need:
        buf = sc["lora"] = torch.empty(need, dtype=torch.uint8, device=sc["qkv"].device)
    desc.scratch, desc.scratch_bytes = buf.data_ptr(), buf.numel()


def _decode_layer(st, form: int, lora: bool):
    """The step's u2tok_decode_layer as (struct, reference to it, config reference, config): the 16-bit descriptor (st.dec) with,
    for a quantised form, the codes and the addresses of their scales in place of the four weights and in the four scale fields
    (norms and biases as the 16-bit step has them) -- for e2m1 with a copy of the step's u2tok_decode_config that says so
    (wform = 2) -- and, for lora, the adapters' u2tok_decode_lora.  One variant per (form, lora), built on first use from the
    sources as they are now; a rebuilt source drops all of them."""
    v = st.variants.get((form, lora))
    if v is None:
        lay = _lib.DecodeLayer.from_buffer_copy(st.dec.layer)
        cfg, cfg_ref = st.dec.cfg, st.dec.cfg_ref
        if form:
            q = _QFORM_OF[form]
            (lay.Wqkv, lay.scale_qkv), (lay.Wo, lay.scale_o), (lay.Wgu, lay.scale_gu), (lay.Wdown, lay.scale_down) = (
                (w.data_ptr(), s.data_ptr()) for w, s in getattr(st, q.copies)[1])
            if q.wform is not None:
                cfg = _lib.DecodeConfig.from_buffer_copy(cfg)   # (the batch size is part of st.dec's key: a change rebuilds both)
                cfg.wform = q.wform
                cfg_ref = C.byref(cfg)
        if lora:
            lay.lora = C.addressof(st.lora.desc)
        v = st.variants[(form, lora)] = (lay, C.byref(lay), cfg_ref, cfg)
    return v


def w8_weights(layer):
    """The four (W8, scale) pairs -- packed q|k|v, o, packed gate|up, down -- a patched layer's e4m3 decode step reads, or None
    (not patched, fp8_decode off, no qualifying step yet, a layer that keeps the 16-bit step)."""
    st = layer.__dict__.get("_u2_prefill")
    return None if st is None or st.w8 is None else st.w8[1]


def w4_weights(layer):
    """The four (codes uint8 (N, K / 2), block scales uint8 (N, K / 32)) pairs -- packed q|k|v, o, packed gate|up, down -- a patched
    layer's e2m1 decode step reads, or None (not patched, fp4_decode off, no qualifying step yet, a layer that keeps another form)."""
    st = layer.__dict__.get("_u2_prefill")
    return None if st is None or st.w4 is None else st.w4[1]


def _step_variant(st, d, pr, x, B: int, sc, h):
    """What a layer's decode step runs on: weight form -> adapter operands -> adapter scratch for B rows -> descriptor variant
    (found without a call once built).  -> (`_decode_layer`'s tuple, the `_LoraOps` or None)."""
    form = _weight_form(st, d, pr)
    ls = _lora_state(st, st.layout, pr, x.dtype, x.device) if st.ads is not None else None
    if ls is not None:
        _lora_scratch(ls, B, sc, h)
    v = st.variants.get((form, ls is not None))
    return (v if v is not None else _decode_layer(st, form, ls is not None)), ls


def _decode_step(self, x, pe, cache, window, pr):
    """One decode step of a layer (B <= 16 new tokens -- wide_decode: B <= 64 --, one each, against the KV cache): the step
    `generate` repeats up to 768 times per report (eval/mrg.py:74-77).  TWO library calls per layer (u2tok_decoder_decode_pre /
    _post, 10 launches) around the cache's own `update`: the products are the weight-streaming few-rows GEMM (gemm_rows.hip; 17 ..
    64 rows: its wide form, always with the batched attention), the attention is the fused kernel with the KEYS split over
    workgroups; with a Python call per kernel the step was bound by the host (7.9 ms against ~4 ms of kernels).
    window = W (a sliding-window layer): the query attends over the last min(T, W) positions -- an offset into the cache buffers.
    fp8_decode / fp4_decode / lora: the same two calls on another variant of the layer descriptor (`_step_variant`).
    Where the rows go is `_KVWrite`'s answer: the first call writes them into an append-in-place layer's buffers at T0, else onto
    the scratch rows; the second reads what `views` returns -- or, on codes (KV8), is u2tok_decoder_decode_post_kv8: it quantises
    the scratch rows into position T0 of the layer's buffers and attends over the codes, always with the batched kernel."""
    att = self.self_attn
    B, _, E = x.shape
    d, sc = _decode_state(self, B, x.device, pr)
    if not d.ok:
        return None                                   # (the caller takes the stock layer)
    st = self._u2_prefill
    with ops.on_device(x) as (h, stream):
        x2 = _rows(x)
        cos, sin = _rotary_rows(pe, B, 1, d.hd, x.dtype)
        T1 = cache.get_seq_length(att.layer_idx) + 1
        if sc["ws"] is None or sc["T"] < T1:
            Tcap = max(2048, 2 * T1)                      # (grows geometrically: the workspace depends on T through the key splits)
            d.cfg.B = B
            sc["ws"] = torch.empty(h.u2tok_decoder_decode_workspace_bytes(d.cfg_ref, Tcap), dtype=torch.uint8, device=x.device)
            sc["T"] = Tcap
        ws, nws = sc["ws"].data_ptr(), sc["ws"].numel()
        out = torch.empty((B, 1, E), dtype=x.dtype, device=x.device)
        # append in place: the rotary kernel writes the step's keys / values at position T0 of the layer's buffers; else into the
        # step's scratch rows -- for the cache's own `update`, or for the second call to quantise into position T0 of the codes
        kind, st.kind = st.kind, None   # (route()'s answer, where it routed this call)
        kv = _KVWrite(cache, att.layer_idx, B, 1, window, like=sc["kc"], kind=kind)
        if kv.kind is APPEND:
            kd, vd = kv.lay._buffers()
            kvs, s_off = kd.stride(1), kv.T0
        else:
            kd, vd, kvs, s_off = sc["kc"], sc["vc"], 0, 0
        (_, layer_ref, cfg_ref, _), _ = _step_variant(st, d, pr, x, B, sc, h)
        _lib.check(h.u2tok_decoder_decode_pre(cfg_ref, layer_ref, x2.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                              int(cos.dtype == torch.float32), cos.stride(0), sc["qkv"].data_ptr(), kd.data_ptr(),
                                              vd.data_ptr(), kvs, s_off, ws, nws, stream), "u2tok_decoder_decode_pre")
        _, kv_start, _ = st.stack.pad
        left = kv_start is not None   # a left-padded batch: the batched decode attention with each sequence's first visible position
        start = kv_start.data_ptr() if left else None
        if kv.kind is KV8:            # over the codes of positions `first` .. T0 (a window W: the last W)
            kc, vc, ks, vs = kv.lay._buffers()
            _lib.check(h.u2tok_decoder_decode_post_kv8(cfg_ref, layer_ref, x2.data_ptr(), sc["qkv"].data_ptr(), kd.data_ptr(), vd.data_ptr(),
                                                       kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), vs.data_ptr(), kc.shape[2], kv.first,
                                                       kv.T0, start, out.data_ptr(), ws, nws, stream), "u2tok_decoder_decode_post_kv8")
        else:
            K, V, kvs = kv.views(kd, vd, kvs)
            _lib.check(h.u2tok_decoder_decode_post(cfg_ref, layer_ref, x2.data_ptr(), sc["qkv"].data_ptr(), K.data_ptr(), V.data_ptr(),
                                                   K.shape[2], kvs, int(left or B > 16), start, out.data_ptr(), ws, nws, stream),
                       "u2tok_decoder_decode_post")
        kv.commit()
    return out


# ---------------------------------------------------------------------------------------------- the whole-stack decode step
_MISSING = object()
_STACK_ARGS = ("input_ids", "attention_mask", "position_ids", "past_key_values", "inputs_embeds", "use_cache")
_STACK_SCRATCH = ("stack_ws", "stack_T", "stack_arr", "stack_keep", "stack_head", "stack_arr8", "stack_keep8")   # what the step keeps in a (B, device, stream) scratch entry
_PE_STUBS = {}


# What the whole-stack step does differently per kind of cache: the struct of a layer's slot; the scratch keys of the slot array and
# of what each slot was filled from; the slot's fields for the addresses of `_buffers()`; its extent field and what it holds of the
# first buffer; the entry without and with the head, each sized by its name + "_workspace_bytes"; whether the entries take `batched`
# (on codes the attention is always the batched one)
_StackKind = namedtuple("_StackKind", "struct arr keep ptrs extent entry head_entry batched")
_STACK_KINDS = {
    APPEND: _StackKind(_lib.DecodeStackLayer, "stack_arr", "stack_keep", ("k_cache", "v_cache"), ("kv_stride", lambda kb: kb.stride(1)),
                       "u2tok_decoder_decode_stack", "u2tok_decoder_decode_stack_head", True),
    KV8: _StackKind(_lib.DecodeStackLayerKv8, "stack_arr8", "stack_keep8", ("k_codes", "v_codes", "k_scales", "v_scales"),
                    ("capacity", lambda kc: kc.shape[2]), "u2tok_decoder_decode_stack_kv8", "u2tok_decoder_decode_stack_head_kv8", False),
}


@dataclass(slots=True, eq=False)
class _StackRun:
    """The whole-stack route's own state, on the decoder stack as `_u2_stack_run` (outside `_StackState`: its fields are the
    switches): the forward the stack had (`had`: the instance attribute it was, or _MISSING for the class's method) and the per-layer
    plan of the call being admitted."""
    orig: object
    had: object
    plan: list = field(default_factory=list)


def _stack_wrap(base) -> None:
    if "_u2_stack_run" not in base.__dict__:
        base._u2_stack_run = _StackRun(base.forward, base.__dict__.get("forward", _MISSING))
        base.forward = types.MethodType(_stack_forward, base)


def _stack_unwrap(base) -> None:
    """Put the stack's own forward back and drop what the route kept: its state, and the workspaces, descriptor arrays and
    descriptor references in the decode steps' scratch."""
    run = base.__dict__.pop("_u2_stack_run", None)
    if run is None:
        return
    if run.had is _MISSING:
        del base.forward
    else:
        base.forward = run.had
    stack = base.__dict__.get("_u2_stack")
    for sc in (stack.scratch.values() if stack is not None else ()):
        for k in _STACK_SCRATCH:
            sc.pop(k, None)


def _no_hooks(m) -> bool:
    d = m.__dict__
    return not (d.get(_HOOKS_F) or d.get(_HOOKS_FP) or d.get(_HOOKS_B) or d.get(_HOOKS_BP))


def stack_route(base, B: int, S: int, dtype, is_cuda: bool, kw: dict, grad: bool, plan: list = None) -> str:
    """Whether a call of the patched decoder stack `base` runs as ONE whole-stack decode step ("stack") or goes on to the stack's
    own forward and the per-layer routes ("layers").  B, S, dtype, is_cuda: of the call's (B, S) ids or (B, S, E) embeddings (ids:
    the embedding table's type); kw: the call's keyword arguments by name, `use_cache`, `output_hidden_states` and
    `output_attentions` resolved against the config.  "stack" needs ALL of:
      * the switch on, grad off, one new position per sequence on the GPU, `use_cache`, a cache, no `output_hidden_states`, no
        `output_attentions`;
      * every layer of the stack patched, none with forward hooks, forward pre-hooks or any other hook table entry (the stack's
        final norm is called as the module it is);
      * `route()` answering "decode" for EVERY layer on this call's shape and keyword arguments -- it keeps deciding masks (the
        pre-hook's verdict: `stack.pad` is current), wide batches, adapters, windows, head dims, types;
      * `_decode_state(...).ok` for every layer, one head dim and one hidden size for all of them;
      * every layer's cache entry of ONE in-place kind (`kv_cache.layer_kind`): the append-in-place layer a fused prefill left,
        holding this batch -- or, with `stack_kv8` on, codes the kernels take (u2tok_decoder_decode_stack_kv8); a dense or sliding
        layer, a cache that mixes the two kinds and codes with the switch off send the call to the per-layer routes.
    plan (a list): receives one (layer, state, projections, `_Decode16`, scratch, window) per layer of a "stack" verdict."""
    stack = base.__dict__.get("_u2_stack")
    if stack is None or not stack.stack or grad or S != 1 or not is_cuda:
        return "layers"
    cache = kw.get("past_key_values")
    if not kw.get("use_cache") or cache is None or kw.get("output_hidden_states") or kw.get("output_attentions"):
        return "layers"
    layers = list(base.layers[:base.config.num_hidden_layers])
    if not layers or not hasattr(base, "norm"):
        return "layers"
    lkw = {k: v for k, v in kw.items() if k not in ("input_ids", "inputs_embeds", "attention_mask", "position_ids", "use_cache",
                                                    "output_hidden_states")}
    steps = []
    hd = E = kind0 = None
    for layer in layers:
        if not is_patched(layer) or not _no_hooks(layer):
            return "layers"
        st = layer._u2_prefill
        att = layer.self_attn
        pr = st.layout.projections(layer)
        E1 = _base(pr[0]).weight.shape[1]
        pe = _PE_STUBS.get(att.head_dim)
        if pe is None:   # (route() reads the tables' last dimension alone)
            pe = _PE_STUBS[att.head_dim] = (torch.empty(0, att.head_dim),) * 2
        lkw["position_embeddings"] = pe
        how, window = route(layer, (B, 1, E1), dtype, is_cuda, (), lkw, False, pr)
        if how != "decode" or (hd is not None and (att.head_dim != hd or E1 != E)):
            return "layers"
        hd, E = att.head_dim, E1
        kind = st.kind                                   # (route() said "decode": of the kinds it admits)
        if not (kind is APPEND or (kind is KV8 and stack.stack8)) or (kind0 is not None and kind is not kind0):
            return "layers"                              # (one in-place kind for the whole call; codes with `stack_kv8` alone)
        kind0 = kind
        d, sc = _decode_state(layer, B, _base(pr[0]).weight.device, pr)
        if not d.ok:
            return "layers"
        steps.append((layer, st, pr, d, sc, window))
    if plan is not None:
        plan[:] = steps
    return "stack"


def _stack_forward(self, *args, **kwargs):
    """The forward of a decoder stack while `stack_decode` is on: the whole-stack step for the calls `stack_route` admits, the
    stack's own forward -- and with it the per-layer routes -- unchanged for every other call.  (The `_mask_hook` pre-hook has run:
    `stack.pad` is this call's.)"""
    run = self._u2_stack_run
    if len(args) > len(_STACK_ARGS) or any(n in kwargs for n in _STACK_ARGS[:len(args)]):
        return run.orig(*args, **kwargs)
    kw = dict(zip(_STACK_ARGS, args), **kwargs)
    ids, x = kw.get("input_ids"), kw.get("inputs_embeds")
    t = x if x is not None else ids
    if (ids is None) == (x is None) or not torch.is_tensor(t) or t.dim() != (3 if x is not None else 2):
        return run.orig(*args, **kwargs)
    cfg = self.config
    for name in ("use_cache", "output_hidden_states", "output_attentions"):
        if kw.get(name) is None:
            kw[name] = getattr(cfg, name, False)
    dtype = x.dtype if x is not None else self.embed_tokens.weight.dtype
    plan = run.plan
    if stack_route(self, t.shape[0], t.shape[1], dtype, t.is_cuda, kw, torch.is_grad_enabled(), plan) != "stack":
        return run.orig(*args, **kwargs)
    try:
        return _stack_step(self, plan, ids, x, kw["past_key_values"], kw.get("position_ids"))
    finally:
        plan.clear()


def _stack_step(base, plan, ids, x, cache, position_ids, head=None):
    """One decode step of the whole decoder stack in ONE library call (u2tok_decoder_decode_stack; on a cache of `Kv8Layer`s
    u2tok_decoder_decode_stack_kv8, whose rotary kernel appends the step's rows as codes): per layer what `_decode_step` does
    around its two calls -- `_step_variant`, room for one more row in the layer's buffers --, then the call, then every layer's
    commit.  The rotary tables come from ONE call of the stack's `rotary_emb`, as the layers receive them from the stock forward.
    head (a `_HeadState`): the step with the head (u2tok_decoder_decode_stack_head) -- the stack's final norm and lm_head ride in
    the call, and the result is (last hidden rows un-normed (B, 1, E), fp32 logits (B, 1, V))."""
    from transformers.modeling_outputs import BaseModelOutputWithPast
    if x is None:
        x = base.embed_tokens(ids)
    B, _, E = x.shape
    if position_ids is None:
        position_ids = (torch.arange(1, device=x.device) + cache.get_seq_length()).unsqueeze(0)
    pe = base.rotary_emb(x, position_ids)
    n = len(plan)
    stack = plan[0][1].stack
    sc = plan[0][4]            # (one scratch entry per (B, device, stream): every layer's `_decode_state` returned the same)
    hd = plan[0][3].hd
    # (`stack_route`: one kind of cache per call -- append-in-place layers, or `Kv8Layer`s and the entries on codes)
    which = plan[0][1].kind or layer_kind(cache, plan[0][0].self_attn.layer_idx, B)[0]   # (route()'s answer)
    kind = _STACK_KINDS[which]
    layers, like = cache.layers, sc["kc"]
    with ops.on_device(x) as (h, stream):
        x2 = _rows(x)
        cos, sin = _rotary_rows(pe, B, 1, hd, x.dtype)
        arr = sc.get(kind.arr)
        if arr is None or len(arr) != n:
            arr = sc[kind.arr] = (kind.struct * n)()
            sc[kind.keep] = [None] * n
            sc["stack_ws"] = None
        keep = sc[kind.keep]
        rows, lss, Tmax = [], [], 0
        for i, (layer, st, pr, d, _, window) in enumerate(plan):
            v, ls = _step_variant(st, d, pr, x, B, sc, h)
            if ls is not None:
                lss.append(ls)
            lay = layers[layer.self_attn.layer_idx]   # (`_KVWrite`'s rule for an in-place layer, without the object)
            T0 = lay._room(1, like)
            first = window_first(T0, window)
            bufs = lay._buffers()
            slot, had = arr[i], keep[i]
            if had is None or had[0] is not v or had[1] is not bufs[0]:   # (rewrite what changed: a rebuilt variant, a re-homed buffer)
                slot.cfg, slot.layer = C.addressof(v[3]), C.addressof(v[0])
                for f, t in zip(kind.ptrs, bufs):
                    setattr(slot, f, t.data_ptr())
                setattr(slot, kind.extent[0], kind.extent[1](bufs[0]))
                keep[i] = (v,) + bufs
            T = T0 + 1 - first
            slot.s_off, slot.k_first, slot.T = T0, first, T
            if T > Tmax:
                Tmax = T
            rows.append((lay, T0 + 1, T))
        for ls in lss:   # (a later layer's larger group may have replaced the shared adapter scratch: all of them read the last one)
            ls.desc.scratch, ls.desc.scratch_bytes = sc["lora"].data_ptr(), sc["lora"].numel()
        name = kind.entry if head is None else kind.head_entry
        if sc["stack_ws"] is None or sc["stack_T"] < Tmax or (head is not None and not sc.get("stack_head")):
            Tcap = max(2048, 2 * Tmax, sc.get("stack_T", 0))   # (grows geometrically, as the per-layer step's workspace does)
            for i in range(n):
                arr[i].T = Tcap
            # (the head's normed rows lie behind the stack step's workspace, and the entries on codes size it as the 16-bit ones do on
            #  the same (cfg, T): a workspace once sized for the head serves all four entries)
            need = getattr(h, name + "_workspace_bytes")(arr, n, *(() if head is None else (head.ref,)))
            for i, row in enumerate(rows):
                arr[i].T = row[2]
            if need == 0:
                raise RuntimeError("u2tok_decoder_decode_stack_workspace_bytes refused the stack's descriptors")
            sc["stack_ws"] = torch.zeros(need, dtype=torch.uint8, device=x.device)   # (zeros: the tail norms' ticket, once)
            sc["stack_T"] = Tcap
            sc["stack_head"] = head is not None
        ws = sc["stack_ws"]
        out = torch.empty((B, 1, E), dtype=x.dtype, device=x.device)
        _, kv_start, _ = stack.pad
        left = kv_start is not None
        # (w_final_norm = NULL: the stack's final norm stays the module's own below, as on the per-layer routes -- the library's
        #  RMSNorm and the module's add a row's squares in another order, and one element in some ten thousand rounds the other way)
        front = (arr, n, x2.data_ptr(), cos.data_ptr(), sin.data_ptr(), int(cos.dtype == torch.float32), cos.stride(0))
        front += ((int(left or B > 16),) if kind.batched else ()) + (kv_start.data_ptr() if left else None,)
        if head is None:
            _lib.check(getattr(h, name)(*front, None, 0.0, int(STACK_TAIL_NORM), out.data_ptr(), ws.data_ptr(), ws.numel(), stream), name)
        else:
            logits = torch.empty((B, 1, head.desc.V), dtype=torch.float32, device=x.device)
            _lib.check(getattr(h, name)(*front, int(STACK_TAIL_NORM), out.data_ptr(), head.ref, logits.data_ptr(), head.desc.V,
                                        ws.data_ptr(), ws.numel(), stream), name)
        for lay, T1, _ in rows:
            lay._commit(T1)
    for i, step in enumerate(plan):
        _count(step[1], "decode", B, which is KV8, i == 0)
    if head is not None:
        return out, logits
    return BaseModelOutputWithPast(last_hidden_state=base.norm(out), past_key_values=cache)


# ---------------------------------------------------------------------------------------------- the head of the decode step
HEAD_FORMS = {"elem": 0, "fp8": 1, "fp4": 2}   # config.u2_fused_head_form -> the form number of u2tok_decode_head_desc


@dataclass(slots=True, eq=False)
class _HeadState:
    """What the head route keeps on the causal LM (`_u2_head`): the sources it was built from (`key`), the form lm_head runs in, its
    quantised copy ((codes, scales), None in the element type) -- the head's own: with tied embeddings `embed_tokens` keeps reading
    the 16-bit table --, the u2tok_decode_head_desc and the reference handed to the library."""
    key: tuple
    form: int
    copy: tuple
    desc: object
    ref: object


def head_form(requested: str, E: int) -> tuple:
    """(form number, fell back) of `config.u2_fused_head_form` for a hidden size E: "elem" -> 0; "fp8" -> 1 where E % 64 == 0; "fp4"
    -> 2 where E % 128 == 0 (what the few-rows product of that form asks of K); a shape the form does not take runs on the element
    type (0, True).  Another word than the three: ValueError."""
    if requested not in HEAD_FORMS:
        raise ValueError(f"u2_fused_head_form: expected one of {sorted(HEAD_FORMS)}, got {requested!r}")
    form = HEAD_FORMS[requested]
    if form and E % _QFORM_OF[form].multiple:
        return 0, True
    return form, False


def head_weights(model):
    """The (codes, scales) pair lm_head's quantised head reads -- ops.quantize_rows_fp8's or ops.quantize_blocks_fp4's --, or None
    (switch off, no head-route call yet, the element type)."""
    hs = model.__dict__.get("_u2_head")
    return None if hs is None else hs.copy


def _head_state(model, form: int) -> _HeadState:
    """The head's descriptor for `form`, built at the first head-route call and rebuilt when lm_head.weight's or the final norm
    weight's data_ptr() or _version changed (an optimiser step, load_state_dict, weight.mul_) or another form is asked for --
    as `_quant_state` has it for a layer."""
    w, norm = model.lm_head.weight, _stack_of(model).norm
    key = (w.data_ptr(), w._version, norm.weight.data_ptr(), norm.weight._version, float(norm.variance_epsilon), form)
    hs = model.__dict__.get("_u2_head")
    if hs is None or hs.key != key:
        copy = _QFORM_OF[form].quantise(w.detach()) if form else None
        desc = ops.head_desc(norm.weight.detach(), norm.variance_epsilon, *(copy if form else (w.detach(),)))
        hs = model.__dict__["_u2_head"] = _HeadState(key, form, copy, desc, C.byref(desc))
    return hs


def head_route(model, B: int, S: int, dtype, is_cuda: bool, kw: dict, grad: bool, labels=None, plan: list = None) -> str:
    """Whether a call of the causal LM `model` (its decoder stack patched) runs the whole-stack step WITH the head ("head": final
    norm, lm_head and fp32 logits in the stack's library call) or today's path ("stock": the stack's forward -- the whole-stack step
    where `stack_route` admits it -- then the module norm and nn.Linear).  B, S, dtype, is_cuda, kw, grad, plan: as `stack_route`
    takes them (kw: the STACK's keyword arguments, resolved against the config); "logits_to_keep" and "return_dict" of the model call
    ride in kw as well.  "head" needs ALL of:
      * the switch on, no `labels`, one position per sequence, every position's logits asked for (`logits_to_keep` 0, 1 or absent),
        a ModelOutput asked for;
      * lm_head exactly nn.Linear: no bias, no hooks, not adapter-wrapped; its weight in the call's element type (bf16 or fp16),
        rows of unit stride a multiple of 8 elements apart, on the device of the stack's weights;
      * the stack's `norm` of the class of the layers' input norm (the decoder's own RMSNorm), without hooks, its weight like
        lm_head's; no hook on the stack but the route's own mask hook;
      * shapes the norm and the product take: hidden size a multiple of 32 up to 8192, a vocabulary of at least 2, lm_head (V, E);
      * `stack_route` answering "stack" for this call."""
    base = _stack_of(model)
    stack = base.__dict__.get("_u2_stack")
    if stack is None or not stack.head or labels is not None or S != 1:
        return "stock"
    keep = kw.get("logits_to_keep", 0)
    if not (keep is None or (isinstance(keep, int) and not isinstance(keep, bool) and keep in (0, 1))) or kw.get("return_dict", True) is False:
        return "stock"
    head, norm = getattr(model, "lm_head", None), getattr(base, "norm", None)
    layers = base.layers[:base.config.num_hidden_layers]
    if type(head) is not torch.nn.Linear or head.bias is not None or not _no_hooks(head) or norm is None or not len(layers):
        return "stock"
    in_norm = getattr(layers[0], "input_layernorm", None)
    if in_norm is None or type(norm) is not type(in_norm) or not _no_hooks(norm) or not hasattr(norm, "variance_epsilon"):
        return "stock"
    hooks = base.__dict__
    if hooks.get(_HOOKS_F) or hooks.get(_HOOKS_B) or hooks.get(_HOOKS_BP) or list((hooks.get(_HOOKS_FP) or {}).values()) != [_mask_hook]:
        return "stock"
    w, nw = head.weight, getattr(norm, "weight", None)
    if nw is None or w.dtype != dtype or dtype not in INFER_DTYPES or nw.dtype != dtype or w.device != in_norm.weight.device \
            or nw.device != w.device:
        return "stock"
    V, E = w.shape
    if nw.shape != (E,) or not nw.is_contiguous() or E % 32 or E > 8192 or V < 2 or w.stride(1) != 1 or w.stride(0) < E or w.stride(0) % 8:
        return "stock"
    if w.data_ptr() % 16 or nw.data_ptr() % 16:   # (a view that starts inside a row)
        return "stock"
    skw = {k: v for k, v in kw.items() if k not in ("logits_to_keep", "return_dict")}
    if stack_route(base, B, S, dtype, is_cuda, skw, grad, plan) != "stack":
        return "stock"
    if plan is not None and plan and _base(plan[0][2][0]).weight.shape[1] != E:
        plan.clear()
        return "stock"
    return "head"


def head_forward(model, input_ids, attention_mask, position_ids, past_key_values, inputs_embeds, use_cache, labels, kwargs):
    """What `_u2CausalLMMixin.forward` asks while the decoder stack is patched: the CausalLMOutputWithPast of the head route --
    logits (B, 1, V) fp32 --, or None: the call goes on to the stock forward with its arguments as they came (counted in
    `head_stats` while the switch is on)."""
    base = _stack_of(model)
    stack = base.__dict__.get("_u2_stack")
    if stack is None or not stack.head:
        return None
    run = base.__dict__.get("_u2_stack_run")
    x = inputs_embeds
    t = x if x is not None else input_ids
    ok = run is not None and (input_ids is None) != (x is None) and torch.is_tensor(t) and t.dim() == (3 if x is not None else 2)
    if ok:
        kw = dict(kwargs, input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, past_key_values=past_key_values,
                  inputs_embeds=x, use_cache=use_cache)
        cfg = base.config
        for name in ("use_cache", "output_hidden_states", "output_attentions"):
            if kw.get(name) is None:
                kw[name] = getattr(cfg, name, False)
        dtype = x.dtype if x is not None else base.embed_tokens.weight.dtype
        # (the stack is not called as a module on this route: its mask pre-hook's verdict is asked for here)
        if t.shape[1] == 1 and labels is None:
            _mask_hook(base, (), {"attention_mask": attention_mask})
        plan = run.plan
        ok = head_route(model, t.shape[0], t.shape[1], dtype, t.is_cuda, kw, torch.is_grad_enabled(), labels, plan) == "head"
    if not ok:
        head_stats["fallback"] += 1
        return None
    from transformers.modeling_outputs import CausalLMOutputWithPast
    try:
        form, fell = head_form(str(getattr(model.config, "u2_fused_head_form", "elem")), model.lm_head.weight.shape[1])
        hs = _head_state(model, form)
        _, logits = _stack_step(base, plan, input_ids, x, kw["past_key_values"], kw.get("position_ids"), head=hs)
    finally:
        plan.clear()
    head_stats["head"] += 1
    head_stats["form_fallback"] += fell
    return CausalLMOutputWithPast(logits=logits, past_key_values=kw["past_key_values"])


def _mask_hook(module, args, kwargs):
    """Forward pre-hook of the decoder stack: the verdict on the call's 2-D mask for route().  The fused layers assume no padding
    (the path's prompts are left-aligned and the reference evaluates at batch 1, eval/mrg.py:74): a mask with zeros sends the
    whole call to the stock layers, unless `padded` is on and `pad_rule` finds a key range per sequence.  One synchronisation
    either way: off, the single `.all()`."""
    m = kwargs.get("attention_mask")
    stack = module._u2_stack
    if stack.padded:
        pad = pad_rule(m)
    else:
        pad = _NO_PAD if m is None or (torch.is_tensor(m) and m.dim() == 2 and bool(m.to(torch.bool).all())) else None
    stack.pad, stack.pad_shape = pad, (tuple(m.shape) if pad is not None and m is not None else None)
    return None


_warned_protocol = [False]


def _layer_protocol_ok(layer, base=None) -> bool:
    """_layer_forward is written against the decoder-layer protocol of transformers >= 4.56 / 5.x: the cache arrives as the
    keyword `past_key_values`, rotary tables as `position_embeddings`, and the layer returns the hidden-state TENSOR.  From
    4.46 (the reference's pin) up to that change the keyword is `past_key_value` and layers return tuples: there the cache
    would never be updated and `layer_outputs[0]` would slice the batch.  Such layers are left stock."""
    import inspect
    import warnings
    try:
        sig = inspect.signature(layer.forward)
        ok = "past_key_values" in sig.parameters and "position_embeddings" in sig.parameters
        ret = sig.return_annotation
        if ok and ret is not inspect.Signature.empty and "tuple" in str(ret).lower():
            # (Phi3DecoderLayer of transformers 5.x still announces a tuple and returns the tensor: the decoder stack that
            #  assigns the layer's result to its hidden states is the evidence)
            try:
                ok = base is not None and "hidden_states = decoder_layer(" in inspect.getsource(type(base).forward)
            except (TypeError, OSError):
                ok = False
    except (TypeError, ValueError):
        ok = False
    if not ok and not _warned_protocol[0]:
        _warned_protocol[0] = True
        import transformers
        warnings.warn(f"u2tokenizer_amd.prefill: decoder layer protocol of transformers {transformers.__version__} is not the one "
                      "the fused prefill is written for (past_key_values keyword, tensor return); layers stay stock")
    return ok


def enable_fused_prefill(model, decode: bool = True, strict: bool = True, train: bool = False, prefill: bool = True,
                         padded: bool = False, continued: bool = False, fp8_decode: bool = False,
                         train_phi3: bool = False, wide_decode: bool = False, train_lora: bool = False, lora: bool = False,
                         fp4_decode: bool = False, stack_decode: bool = False, head: bool = False, stack_kv8: bool = False,
                         kv8_continued: bool = False, kv8: bool = False) -> int:
    """Patch the decoder layers of an HF Llama / Qwen3 / Phi-3 causal LM (u2LlamaForCausalLM / u2Qwen3ForCausalLM /
    u2Phi3ForCausalLM included) for the fused prefill and the fused decode step.  Idempotent; returns the number of layers
    patched.  The keywords are the route switches: SWITCHES describes each once, the module docstring what they share.  Every
    call sets all of them anew, so a switch that is not named goes back to its default, and what it kept per layer is freed.
    `disable_fused_prefill` restores the stock forwards."""
    given = dict(decode=decode, strict=strict, train=train, prefill=prefill, padded=padded, continued=continued,
                 fp8_decode=fp8_decode, train_phi3=train_phi3, wide_decode=wide_decode, train_lora=train_lora, lora=lora,
                 fp4_decode=fp4_decode, stack_decode=stack_decode, head=head, stack_kv8=stack_kv8, kv8_continued=kv8_continued,
                 kv8=kv8)
    base = _stack_of(model)
    layers = getattr(base, "layers", None)
    if layers is None:
        raise RuntimeError("enable_fused_prefill: no decoder layers found (expected an HF Llama / Qwen3 / Phi-3 model)")
    todo = []
    for layer in layers:
        if is_patched(layer):
            continue
        layout = _layout_of(layer)
        if layout is None:
            if strict:
                raise RuntimeError(f"enable_fused_prefill: unsupported decoder layer {type(layer).__name__}")
            continue   # (another layer layout: stays stock)
        if _layer_protocol_ok(layer, base):
            todo.append((layer, layout))
    stack = base.__dict__.get("_u2_stack")
    if stack is None:
        stack = base._u2_stack = _StackState(base.register_forward_pre_hook(_mask_hook, with_kwargs=True))
    on = {s.kw: bool(given[s.kw]) for s in SWITCHES}
    for s in SWITCHES:
        if on[s.kw]:
            on.update(dict.fromkeys(s.implies, True))
    for s in SWITCHES:
        if s.field is not None:
            setattr(stack, s.field, on[s.kw])
        if s.frees and not on[s.kw]:   # (what the switch kept per layer goes with it, and the descriptors built from it)
            for layer in layers:
                if is_patched(layer):
                    for f in s.frees:
                        setattr(layer._u2_prefill, f, None)
                    _drop_variants(layer._u2_prefill)
    stack.pad, stack.pad_shape = _NO_PAD, None
    for layer, layout in todo:
        layer._u2_prefill = _LayerState(layer.forward, stack, layout)
        layer.forward = types.MethodType(_layer_forward, layer)
    (_stack_wrap if stack.stack else _stack_unwrap)(base)
    if not stack.head:
        model.__dict__.pop("_u2_head", None)   # (lm_head's copies and descriptor go with the switch)
    return len(todo)


def disable_fused_prefill(model) -> None:
    base = _stack_of(model)
    model.__dict__.pop("_u2_head", None)
    for layer in base.layers:
        st = layer.__dict__.pop("_u2_prefill", None)
        if st is not None:
            layer.forward = st.orig
    _stack_unwrap(base)
    stack = base.__dict__.pop("_u2_stack", None)
    if stack is not None:
        stack.hook.remove()


def _stack_of(model):
    return model.get_model() if hasattr(model, "get_model") else getattr(model, "model", model)
