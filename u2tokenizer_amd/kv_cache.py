"""The KV cache layers the fused decoder steps write in place -- append-in-place 16-bit buffers (`AppendLayer`) and e4m3 codes with
a scale per cached row (`Kv8Layer`); every other layer is written through the cache's own `update` -- and the one rule for what kind
of layer a call has (`layer_kind`) and where its rows go (`_KVWrite`).  The two in-place classes answer the same three questions
the same way: `_room(n, like)` -> the current length T0, with room for n more rows; `_buffers()` -> the tensors the kernels
address; `_commit(T)` -> the layer holds T positions.  Nothing here knows a route or a switch: prefill.py decides which kinds a
call may take."""
from __future__ import annotations

import torch
from transformers import cache_utils

from . import ops

# the HF cache classes the fused steps work with (None where this transformers lacks one: before 4.56 no per-layer caches)
_DYN_CACHE, _DYN_LAYER, _SLIDING_LAYER, _CACHE_LAYER = (getattr(cache_utils, n, None) for n in (
    "DynamicCache", "DynamicLayer", "DynamicSlidingWindowLayer", "CacheLayerMixin"))
# element types and head dims of the inference kernels (the row quantiser's among them)
KERNEL_DTYPES, KERNEL_HEAD_DIMS = (torch.bfloat16, torch.float16), (64, 96, 128)

_APPEND_LAYER = None


def _append_layer_class():
    """A DynamicLayer that APPENDS IN PLACE: keys / values are views [:, :, :T] of buffers with room to grow (doubling), so a decode
    step writes one row instead of re-copying the whole cache (DynamicLayer.update is a torch.cat: two launches and 2 x T rows per
    layer and step).  Everything else -- crop, batch selection, beam reordering, the stock attention reading `.keys` -- is
    DynamicLayer's: those reassign `.keys` / `.values`, after which the next update re-homes them."""
    global _APPEND_LAYER
    if _APPEND_LAYER is None:
        class AppendLayer(_DYN_LAYER):
            _kb = _vb = None

            @classmethod
            def _placed(cls, B: int, H: int, n: int, d: int, like: torch.Tensor):
                """A new empty layer for (B, H, *, d) rows of `like`'s type and device, with room for n positions."""
                lay = cls()
                proto = torch.empty((B, H, 0, d), dtype=like.dtype, device=like.device)
                lay.lazy_initialization(proto, proto)
                lay._room(n, torch.empty((B, H, 1, d), dtype=like.dtype, device=like.device))
                return lay

            def _room(self, n: int, like: torch.Tensor = None) -> int:
                """Make sure `n` more positions fit behind the current ones; returns the current length.  like: a (B, H, *, d)
                tensor of the rows' type and device (None: the layer's own keys)."""
                if like is None:
                    like = self.keys
                T0 = self.keys.shape[-2] if self.is_initialized and self.keys.numel() else 0
                kb = self._kb
                homed = kb is not None and (T0 == 0 or (self.keys.data_ptr() == kb.data_ptr() and self.values.data_ptr() == self._vb.data_ptr()
                                                        and self.keys.shape[:2] == kb.shape[:2]))
                if not homed or T0 + n > kb.shape[-2] or kb.shape[:2] != like.shape[:2]:
                    cap = max(256, 2 * (T0 + n))
                    shape = (like.shape[0], like.shape[1], cap, like.shape[3])
                    nk = torch.empty(shape, dtype=like.dtype, device=like.device)
                    nv = torch.empty(shape, dtype=like.dtype, device=like.device)
                    if T0:
                        nk[:, :, :T0].copy_(self.keys)
                        nv[:, :, :T0].copy_(self.values)
                    self._kb, self._vb = nk, nv
                    self.keys, self.values = nk[:, :, :T0], nv[:, :, :T0]
                return T0

            def _buffers(self) -> tuple:
                return self._kb, self._vb

            def _commit(self, T: int) -> None:
                self.keys, self.values = self._kb[:, :, :T], self._vb[:, :, :T]

            def update(self, key_states, value_states, *args, **kwargs):
                if not self.is_initialized:
                    self.lazy_initialization(key_states, value_states)
                n = key_states.shape[-2]
                T0 = self._room(n, key_states)
                self._kb[:, :, T0:T0 + n].copy_(key_states)
                self._vb[:, :, T0:T0 + n].copy_(value_states)
                self._commit(T0 + n)
                return self.keys, self.values

        _APPEND_LAYER = AppendLayer
    return _APPEND_LAYER


class Kv8Layer(_CACHE_LAYER if _CACHE_LAYER is not None else object):
    """A cache layer (CacheLayerMixin's protocol) that keeps K and V as FP8: e4m3 codes (B, H_kv, capacity, d) uint8 and one fp32
    scale per cached row (B, H_kv, capacity), K and V each (`ops.quantize_kv_fp8`: the format; value = code x scale), in buffers with
    room to grow -- they double, the old codes and scales are copied bit for bit.  What the cache HOLDS defines the semantics,
    whatever route reads it:
      * `update()` on an empty layer quantises its inputs and returns them as they came (HF's own quantized-cache rule: the
        prefill attends over what it computed); on a filled layer it quantises the new rows and returns the whole cache dequantised
        in the callers' type -- so the stock layers, and every route that refuses the layer, attend over the same quantised cache
        the fused decode step reads as codes (u2tok_decoder_decode_post_kv8);
      * length, mask sizes, crop, batch selection / repetition, beam reordering, reset, offload / prefetch work on codes and scales
        directly: nothing is ever dequantised and requantised (rnd(code x scale) does not requantise to the same codes);
      * `.keys` / `.values` are read-only, dequantised on demand for foreign readers; assigning them raises.
    Quantisation runs the kernel (u2tok_kv_quantize_rows) for 16-bit rows on the GPU that it takes, the torch reference elsewhere:
    the same bits; the layer works on the CPU."""
    is_sliding = False
    is_compileable = False

    def __init__(self, **kwargs):
        self._kc = self._vc = self._ks = self._vs = None
        self._T = 0
        self.dtype = self.device = None
        self.is_initialized = False

    def _dequant(self, codes, scales):
        if not self.is_initialized or codes is None:
            return None
        T = self._T
        return ops.dequantize_kv_fp8(codes[:, :, :T], scales[:, :, :T], self.dtype)

    @property
    def keys(self):
        return self._dequant(self._kc, self._ks)

    @keys.setter
    def keys(self, value):
        raise AttributeError("Kv8Layer.keys is read-only: the layer holds e4m3 codes and scales")

    @property
    def values(self):
        return self._dequant(self._vc, self._vs)

    @values.setter
    def values(self, value):
        raise AttributeError("Kv8Layer.values is read-only: the layer holds e4m3 codes and scales")

    def lazy_initialization(self, key_states, value_states) -> None:
        self.dtype, self.device = key_states.dtype, key_states.device
        self.is_initialized = True

    def codes(self):
        """(K codes, V codes, K scales, V scales) of the cached positions: views of the buffers (None while empty)"""
        if self._kc is None:
            return None
        T = self._T
        return self._kc[:, :, :T], self._vc[:, :, :T], self._ks[:, :, :T], self._vs[:, :, :T]

    def _room(self, n: int, like=None) -> int:
        """`n` more positions fit behind the current ones -> the current length.  like: (B, H, *, d) on the rows' device, or None."""
        T0, kc = self._T, self._kc
        t = kc if like is None else like
        B, H, d, device = t.shape[0], t.shape[1], t.shape[3], t.device
        if kc is None or T0 + n > kc.shape[2] or kc.shape[:2] != (B, H) or kc.shape[3] != d or kc.device != device:
            if kc is not None and T0 and (kc.shape[:2] != (B, H) or kc.shape[3] != d):
                raise RuntimeError(f"Kv8Layer: rows of shape {(B, H, n, d)} against a cache of {tuple(kc.shape)}")
            cap = max(256, 2 * (T0 + n))
            new = (torch.empty((B, H, cap, d), dtype=torch.uint8, device=device), torch.empty((B, H, cap, d), dtype=torch.uint8, device=device),
                   torch.empty((B, H, cap), dtype=torch.float32, device=device), torch.empty((B, H, cap), dtype=torch.float32, device=device))
            if T0:
                for dst, src in zip(new, (self._kc, self._vc, self._ks, self._vs)):
                    dst[:, :, :T0].copy_(src[:, :, :T0])
            self._kc, self._vc, self._ks, self._vs = new
        return T0

    def _buffers(self) -> tuple:
        return self._kc, self._vc, self._ks, self._vs

    def _commit(self, T: int) -> None:
        self._T = T

    def _quantise(self, k, v, T0: int) -> None:
        n, d = k.shape[2], k.shape[3]
        if k.is_cuda and k.dtype in KERNEL_DTYPES and v.dtype == k.dtype and d in KERNEL_HEAD_DIMS and k.stride(3) == 1 and v.stride(3) == 1 \
                and not any(s % 8 for t in (k, v) for s in t.stride()[:3]) and k.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0:
            ops.kv_quantize_rows(k, v, self._kc, self._vc, self._ks, self._vs, T0)
            return
        for x, codes, scales in ((k, self._kc, self._ks), (v, self._vc, self._vs)):
            c, s = ops.quantize_kv_fp8(x)
            codes[:, :, T0:T0 + n].copy_(c.view(torch.uint8))
            scales[:, :, T0:T0 + n].copy_(s)

    def update(self, key_states, value_states, *args, **kwargs):
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        n = key_states.shape[2]
        T0 = self._room(n, key_states)
        self._quantise(key_states, value_states, T0)
        self._T = T0 + n
        if T0 == 0:
            return key_states, value_states
        dt = key_states.dtype
        return (ops.dequantize_kv_fp8(self._kc[:, :, :self._T], self._ks[:, :, :self._T], dt),
                ops.dequantize_kv_fp8(self._vc[:, :, :self._T], self._vs[:, :, :self._T], dt))

    def get_seq_length(self) -> int:
        return self._T

    def get_mask_sizes(self, query_length) -> tuple:
        if not isinstance(query_length, int):      # (a cache_position tensor: earlier 4.5x protocol)
            query_length = query_length.shape[0]
        return self._T + query_length, 0

    def get_max_length(self) -> int:
        return -1

    def get_max_cache_shape(self) -> int:
        return -1

    def crop(self, tokens_to_remove: int) -> None:
        """DynamicLayer.crop's meaning: a negative number removes that many positions from the end, a positive one is the length to
        keep (nothing happens when it is not shorter than the cache)."""
        T = self._T
        if tokens_to_remove > 0:
            if tokens_to_remove >= T:
                return
            self._T = tokens_to_remove
        else:
            self._T = max(0, T + tokens_to_remove)

    def _each(self, fn) -> None:
        if self._kc is not None:
            self._kc, self._vc, self._ks, self._vs = (fn(t) for t in (self._kc, self._vc, self._ks, self._vs))

    def batch_repeat_interleave(self, repeats: int) -> None:
        if self._T > 0:
            self._each(lambda t: t.repeat_interleave(repeats, dim=0))

    def batch_select_indices(self, indices) -> None:
        if self._T > 0:
            self._each(lambda t: t[indices, ...].contiguous())

    def reorder_cache(self, beam_idx) -> None:
        if self._T > 0:
            self._each(lambda t: t.index_select(0, beam_idx.to(t.device)))

    def reset(self) -> None:
        self._T = 0

    def offload(self) -> None:
        self._each(lambda t: t.to("cpu", non_blocking=True))

    def prefetch(self) -> None:
        if self._kc is not None and self.device is not None and self._kc.device != self.device:
            self._each(lambda t: t.to(self.device, non_blocking=True))


def kv8_cache(n_layers: int):
    """A plain HF DynamicCache of `n_layers` empty `Kv8Layer`s: what `kv8` leaves behind a fused prefill, for a caller that wants
    the FP8 cache on the stock layers as well (any device)."""
    cache = _DYN_CACHE()
    cache.layers.extend(Kv8Layer() for _ in range(n_layers))
    return cache


def _plain_layers(cache):
    """The `layers` list of `cache` if it is a plain HF DynamicCache (no offloading), else None."""
    layers = getattr(cache, "layers", None)
    if type(cache) is not _DYN_CACHE or not isinstance(layers, list) or getattr(cache, "offloading", False):
        return None
    return layers


# What a call's cache layer is (`layer_kind`; compared by identity), and the kinds a step writes where the cache keeps them
NO_CACHE, FOREIGN, LAZY, EMPTY, DENSE, SLIDING = "no cache", "foreign", "lazy", "empty", "dense", "sliding"
APPEND, APPEND_OTHER, KV8, KV8_OTHER = "append", "append-other", "kv8", "kv8-other"
IN_PLACE = (APPEND, KV8)


def layer_kind(cache, layer_idx: int, B: int):
    """(kind, layer | None) of layer `layer_idx` of `cache` for a call of B sequences; the one place that tests cache and layer
    classes.  NO_CACHE; FOREIGN: not a plain DynamicCache, an offloaded one, a layer class unknown here; LAZY: the cache will still
    create the layer, as a DynamicLayer; EMPTY: a DynamicLayer or append-in-place layer without positions; DENSE: a filled
    DynamicLayer; SLIDING: a DynamicSlidingWindowLayer, empty or filled; APPEND / APPEND_OTHER: a filled append-in-place layer
    holding this batch / another (reordered, re-batched: its `update` re-homes it); KV8: a `Kv8Layer` the kernels take -- filled,
    this batch, codes on the GPU; KV8_OTHER: any other `Kv8Layer`."""
    if cache is None:
        return NO_CACHE, None
    layers = _plain_layers(cache)
    if layers is None:
        return FOREIGN, None
    if layer_idx >= len(layers):
        return (LAZY if getattr(cache, "layer_class_to_replicate", None) is _DYN_LAYER else FOREIGN), None
    lay = layers[layer_idx]
    t = type(lay)
    if t is _APPEND_LAYER or t is _DYN_LAYER:
        keys = lay.keys if lay.is_initialized else None
        if keys is None or keys.numel() == 0:   # (DynamicLayer.get_seq_length() == 0)
            return EMPTY, lay
        if t is _DYN_LAYER:
            return DENSE, lay
        return (APPEND if keys.shape[0] == B else APPEND_OTHER), lay
    if t is Kv8Layer:
        kc = lay._kc
        return (KV8 if lay._T > 0 and kc is not None and kc.shape[0] == B and kc.is_cuda else KV8_OTHER), lay
    return (SLIDING if t is _SLIDING_LAYER else FOREIGN), lay


def _prefill_append_layer(cache, layer_idx: int, B: int, Hkv: int, S: int, d: int, like: torch.Tensor, kv8: bool = False):
    """For a plain HF DynamicCache whose layer `layer_idx` is still empty: put an append-in-place layer there with room for S
    positions (and as many again for the decode steps) and return it; None for every other cache (its `update` is used).  kv8: a
    `Kv8Layer` is put there instead (an empty one stays) and None is returned: the caller commits through its quantising `update`."""
    kind, lay = layer_kind(cache, layer_idx, B)
    if kind is LAZY:
        layers = cache.layers
        while len(layers) <= layer_idx:
            layers.append(_DYN_LAYER())
        kind = EMPTY
    empty8 = kv8 and kind is KV8_OTHER and lay.get_seq_length() == 0
    if kind is not EMPTY and not empty8:
        return None
    if kv8:
        if _CACHE_LAYER is not None and not empty8:
            cache.layers[layer_idx] = Kv8Layer()
        return None
    try:
        lay = _append_layer_class()._placed(B, Hkv, S, d, like)
    except (TypeError, AttributeError):  # (another transformers version's layer protocol)
        return None
    cache.layers[layer_idx] = lay
    return lay


def window_first(T0: int, window) -> int:
    """First position a step under a window W reads of a layer holding T0: the last n + W - 1 of T0 + n start there, whatever n."""
    return 0 if window is None else max(0, T0 + 1 - window)


class _KVWrite:
    """Where the new keys / values of a step go and what it attends over -- the one KV-write rule of the prefill, the continued
    prefill and the decode steps.  `kind`: `layer_kind`'s answer (argument: where the caller has it already); `lay`: the layer when
    the step writes it in place (`IN_PLACE`), else None; `T0`: the positions it holds; `first`: `window_first` of T0.
      * APPEND: the rotary kernel writes behind the T0 old positions of the layer's buffers, `views` are of those buffers.
      * KV8: the step's rows become codes behind the T0 cached ones -- the decode steps' entries quantise them, the continued
        prefill does in `attend8` -- and the attention reads the codes.
      * everything else: dense tensors through the cache's own `update` -- in `views` when the step attends over the cache, else
        in `commit`.
    fresh = (H_kv, d, like): the first call into this layer; `_prefill_append_layer` puts an append-in-place layer there (APPEND,
    T0 = 0) or, kv8, a `Kv8Layer` that is written through its own `update` (`lay` stays None).  The whole-stack step, whose layers
    are all of one in-place kind, follows the rule without the object: `_room`, `window_first`, `_buffers`, `_commit`."""
    __slots__ = ("cache", "idx", "n", "window", "kind", "lay", "T0", "first")

    def __init__(self, cache, idx: int, B: int, n: int, window, like=None, fresh=None, kv8: bool = False, kind=None):
        self.n, self.window = n, window
        lay, T0 = None, 0
        if fresh is not None:
            if cache is not None:
                lay = _prefill_append_layer(cache, idx, B, fresh[0], n, fresh[1], fresh[2], kv8)
            kind = DENSE if lay is None else APPEND
        else:
            if kind is None:
                kind = layer_kind(cache, idx, B)[0]
            if kind in IN_PLACE:   # (a reordered or re-batched append layer: `_room` re-homes it)
                lay = cache.layers[idx]
                T0 = lay._room(n, like)
        if lay is None:
            self.cache, self.idx = cache, idx   # (for the cache's own `update`)
        self.kind, self.lay, self.T0, self.first = kind, lay, T0, window_first(T0, window)

    def views(self, kc, vc, stride=0):
        """(K, V, stride of one (batch, kv head) entry -- 0: dense) to attend over; kc / vc: the dense new keys / values for a cache
        that is not written in place, stride: the buffers' for one that is.  A window W: the last n + W - 1 positions of an
        in-place layer; of a dense cache the last W for a decode step (a longer call hands the band kernel what `update`
        returned: its masks are relative to the last key, and a DynamicSlidingWindowLayer returns its kept W - 1 positions and the
        new ones)."""
        n, W, lay = self.n, self.window, self.lay
        if lay is not None:
            lo, T1 = self.first, self.T0 + n
            return lay._kb[:, :, lo:T1], lay._vb[:, :, lo:T1], stride
        K, V = self.cache.update(kc, vc, self.idx)   # DynamicLayer: torch.cat -> dense (B, H_kv, T, d)
        self.cache = None                            # (updated: nothing left for `commit`)
        if n == 1:
            K, V = K.contiguous(), V.contiguous()
            if W is not None and K.shape[2] > W:     # (the last W positions: rows of each (batch, kv head) entry)
                return K[:, :, -W:], V[:, :, -W:], K.stride(1)
        elif K.stride() != V.stride() or K.stride(3) != 1 or K.stride(2) != K.shape[3] or K.stride(0) != K.shape[1] * K.stride(1):
            K, V = K.contiguous(), V.contiguous()    # (not a view the band kernel reads where it lies)
        return K, V, 0

    def attend8(self, q, kc, vc, heads: int, scale: float, kv_start):
        """KV8: the dense new rows kc / vc (B, H_kv, n, d) as codes and scales at positions T0 .. T0 + n - 1, then the n new queries
        q (B, n, heads d) over positions `first` .. T0 + n - 1 of the codes."""
        bufs = self.lay._buffers()
        ops.kv_quantize_rows(kc, vc, *bufs, self.T0)
        return ops.attention_kv8_rows(q, *bufs, self.T0 + self.n - self.first, heads, scale, window=self.window, kv_start=kv_start,
                                      k_first=self.first)

    def commit(self, kc=None, vc=None) -> None:
        if self.lay is not None:
            self.lay._commit(self.T0 + self.n)
        elif self.cache is not None:
            self.cache.update(kc, vc, self.idx)
