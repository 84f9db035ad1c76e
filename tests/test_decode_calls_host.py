"""CPU: the operands of the decode steps' library calls.  `prefill._decode_step` (two calls per layer) and `prefill._stack_step` (one
call per token) run on CPU tensors against a handle that records (entry name, arguments) instead of launching: `ops.on_device`
yields it, every `*_workspace_bytes` answers a fixed size, every entry 0, and the stream is a fake one (`_decode_state` asks torch
for it).  Every argument is then checked against what include/u2tok.h defines it to be -- which buffer an address lies in and at
which byte offset, the position the step's row is written at, the first position and the number of positions the attention reads,
the buffers' capacity and stride, the batched flag -- for each kind of cache layer (dense DynamicLayer, append-in-place, `Kv8Layer`),
with and without a binding attention window, for 2 and for 17 sequences, left-padded or not, and for the stack step with and
without the head.  Afterwards the layer holds one more position in the very buffers the call was given."""
import contextlib
import ctypes as C
import types

import pytest
import torch
from transformers.cache_utils import DynamicCache, DynamicLayer

from test_decoder_route_host import _FakeCuda, _model
from u2tokenizer_amd import _lib, ops, prefill

bf = torch.bfloat16
NL, T0, W, WS_BYTES, VOCAB = 2, 9, 4, 4096, 64


class _Handle:
    """the library handle's stand-in: records every call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return WS_BYTES if name.endswith("_workspace_bytes") else 0
        return entry

    def entries(self):
        return [c for c in self.calls if not c[0].endswith("_workspace_bytes")]


@pytest.fixture
def handle(monkeypatch):
    h = _Handle()
    monkeypatch.setattr(ops, "on_device", lambda *a, **k: contextlib.nullcontext((h, 0)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    return h


def _layer_of(kind, B, Hkv, d):
    kv = torch.arange(B * Hkv * T0 * d, dtype=torch.float32).view(B, Hkv, T0, d).mul(1e-3).to(bf)
    lay = {"dense": DynamicLayer, "append": prefill._append_layer_class(), "kv8": prefill.Kv8Layer}[kind]()
    lay.update(kv, -kv)
    if kind == "kv8":      # (the routes take codes on the GPU alone: the buffer says it is there)
        lay._kc = lay._kc.as_subclass(_FakeCuda)
    return lay


def _setup(kinds, B, left, **sw):
    """a patched two-layer Qwen3 stack (hidden 128, 2 query heads / 1 kv head of 64) and a plain cache of T0 positions per layer"""
    m = _model(num_hidden_layers=NL)
    prefill.enable_fused_prefill(m, kv8=True, padded=True, wide_decode=True, **sw)
    cache = DynamicCache()
    cache.layers.extend(_layer_of(k, B, 1, 64) for k in kinds)
    kv_start = torch.arange(B, dtype=torch.int32) % 3 if left else None
    m.model._u2_stack.pad = ("left", kv_start, None) if left else prefill._NO_PAD
    m.model._u2_stack.pad_shape = (B, T0 + 1) if left else None
    return m, cache, kv_start


def _within(addr, t):
    """byte offset of `addr` inside the storage of tensor `t`"""
    base = t.untyped_storage().data_ptr()
    assert base <= addr < base + t.untyped_storage().nbytes(), (addr, base)
    return addr - t.data_ptr()


CELLS = [(w, B, left) for w in (None, W) for B in (2, 17) for left in (False, True)]
IDS = [f"W{w}-B{B}-{'left' if left else 'nopad'}" for w, B, left in CELLS]


@pytest.mark.parametrize("window,B,left", CELLS, ids=IDS)
@pytest.mark.parametrize("kind", ["dense", "append", "kv8"])
def test_the_per_layer_step(handle, kind, window, B, left):
    m, cache, kv_start = _setup((kind, kind), B, left)
    k_first = 0 if window is None else max(0, T0 + 1 - window)
    T = T0 + 1 - k_first
    for layer in m.model.layers:
        idx = layer.self_attn.layer_idx
        lay = cache.layers[idx]
        pr = prefill._SplitLayout.projections(layer)
        x = torch.zeros(B, 1, 128, dtype=bf)
        pe = (torch.ones(B, 1, 64, dtype=bf), torch.zeros(B, 1, 64, dtype=bf))
        if kind == "kv8":
            bufs = (lay._kc, lay._vc, lay._ks, lay._vs)
        elif kind == "append":
            bufs = (lay._kb, lay._vb)
        handle.calls.clear()
        out = prefill._decode_step(layer, x, pe, cache, window, pr)
        assert out.shape == (B, 1, 128) and out.dtype == bf
        (n1, pre), (n2, post) = handle.entries()
        assert n1 == "u2tok_decoder_decode_pre" and n2 == ("u2tok_decoder_decode_post_kv8" if kind == "kv8" else "u2tok_decoder_decode_post")
        sc = next(iter(m.model._u2_stack.scratch.values()))
        # pre: cfg, layer, x, cos, sin, cos_sin_f32, cs_ld, qkv, k_cache, v_cache, kv_stride, s_off, workspace, bytes, stream
        assert len(pre) == 15 and pre[2] == x.data_ptr() and pre[5] == 0 and pre[6] == 64 and pre[7] == sc["qkv"].data_ptr()
        assert pre[12] == sc["ws"].data_ptr() and pre[13] == WS_BYTES == sc["ws"].numel() and pre[14] == 0
        if kind == "append":      # the row lands at position T0 of the layer's buffers
            assert pre[8:12] == (bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[0].stride(1), T0)
        else:                     # ... else in the step's dense scratch rows
            assert pre[8:12] == (sc["kc"].data_ptr(), sc["vc"].data_ptr(), 0, 0)
        assert post[:4] == (pre[0], pre[1], x.data_ptr(), sc["qkv"].data_ptr())
        assert post[-4:] == (out.data_ptr(), pre[12], WS_BYTES, 0)
        start = kv_start.data_ptr() if left else None
        if kind == "kv8":
            # post_kv8: ..., k_new, v_new, k_codes, v_codes, k_scales, v_scales, capacity, k_first, s_off, kv_start, out, ws, bytes, stream
            assert len(post) == 18 and post[4:6] == (sc["kc"].data_ptr(), sc["vc"].data_ptr())
            assert post[6:10] == tuple(t.data_ptr() for t in bufs)
            assert post[10:14] == (bufs[0].shape[2], k_first, T0, start)
            assert (lay._kc, lay._vc, lay._ks, lay._vs) == bufs and lay.codes()[0].shape[2] == T0 + 1
        else:
            # post: ..., K, V, T, kv_stride, batched, kv_start, out, ws, bytes, stream
            assert len(post) == 14
            if kind == "append":
                src = bufs
                assert lay._kb is bufs[0] and lay._vb is bufs[1] and lay.keys.data_ptr() == bufs[0].data_ptr()
                stride = bufs[0].stride(1)
            else:                 # what the cache's own `update` returned and keeps
                src = (lay.keys, lay.values)
                assert lay.keys.is_contiguous()
                stride = lay.keys.stride(1) if k_first else 0
            assert _within(post[4], src[0]) == _within(post[5], src[1]) == k_first * 64 * 2
            assert post[6:10] == (T, stride, int(left or B > 16), start)
        assert lay.get_seq_length() == T0 + 1 and cache.get_seq_length(idx) == T0 + 1


STACK_CELLS = [(w, B, left, head) for w, B, left in CELLS for head in (False, True)]


@pytest.mark.parametrize("window,B,left,head", STACK_CELLS, ids=[f"{i}-{'head' if h else 'nohead'}" for i in IDS for h in (False, True)])
@pytest.mark.parametrize("kind", ["append", "kv8"])
def test_the_stack_step(handle, kind, window, B, left, head):
    m, cache, kv_start = _setup((kind, kind), B, left, stack_kv8=True)
    q8 = kind == "kv8"
    k_first = 0 if window is None else max(0, T0 + 1 - window)
    T = T0 + 1 - k_first
    plan = []
    for layer in m.model.layers:
        pr = prefill._SplitLayout.projections(layer)
        d, sc = prefill._decode_state(layer, B, torch.device("cpu"), pr)
        plan.append((layer, layer._u2_prefill, pr, d, sc, window))
    hs = None
    if head:
        desc = _lib.DecodeHead(w_norm=1 << 20, W=1 << 20, scale=None, E=128, V=VOCAB, wform=0, eps=1e-6, ldw=0, lds=0)
        hs = prefill._HeadState((), 0, None, desc, C.byref(desc))
    bufs = [(lay._kc, lay._vc, lay._ks, lay._vs) if q8 else (lay._kb, lay._vb) for lay in cache.layers]
    x = torch.zeros(B, 1, 128, dtype=bf)
    n0 = {k: dict(getattr(prefill, k)) for k in ("stats", "stack_stats", "kv8_stats", "stack_kv8_stats")}
    res = prefill._stack_step(m.model, plan, None, x, cache, None, head=hs)
    (name, a), = handle.entries()
    assert name == "u2tok_decoder_decode_stack" + ("_head" if head else "") + ("_kv8" if q8 else "")
    sizing = [c for c in handle.calls if c[0].endswith("_workspace_bytes")]
    assert [c[0] for c in sizing] == [name + "_workspace_bytes"] and sizing[0][1][:2] == (a[0], NL)
    # layers, n, x, cos, sin, cos_sin_f32, cs_ld, [batched -- the 16-bit entries alone], kv_start, ...
    arr = a[0]
    assert a[1] == NL and a[2] == x.data_ptr() and a[5] in (0, 1) and a[6] in (0, 64)   # (one table row for all sequences, or one each)
    start = kv_start.data_ptr() if left else None
    if q8:
        rest = a[7:]
        assert rest[0] == start
    else:
        rest = a[8:]
        assert a[7:9] == (int(left or B > 16), start)
    rest = rest[1:]
    ws = sc["stack_ws"]
    if head:       # tail_norm, out, head, logits, ld_logits, workspace, bytes, stream
        out, logits = res
        assert len(rest) == 8 and rest[0] == int(prefill.STACK_TAIL_NORM) and rest[1] == out.data_ptr() and rest[2] is hs.ref
        assert rest[3:] == (logits.data_ptr(), VOCAB, ws.data_ptr(), WS_BYTES, 0)
        assert logits.shape == (B, 1, VOCAB) and logits.dtype == torch.float32 and out.shape == (B, 1, 128)
    else:          # w_final_norm, final_eps, tail_norm, out, workspace, bytes, stream
        assert len(rest) == 7 and rest[:3] == (None, 0.0, int(prefill.STACK_TAIL_NORM)) and rest[4:] == (ws.data_ptr(), WS_BYTES, 0)
        assert res.last_hidden_state.shape == (B, 1, 128) and res.past_key_values is cache
    assert ws.numel() == WS_BYTES and not ws.any()                           # (zeroed once: the tail norms' ticket)
    for i, (layer, st, pr, d, _, _) in enumerate(plan):
        slot, lay, b = arr[i], cache.layers[i], bufs[i]
        v = st.variants[(0, False)]
        assert slot.cfg == C.addressof(v[3]) and slot.layer == C.addressof(v[0])
        assert (slot.s_off, slot.k_first, slot.T) == (T0, k_first, T)
        if q8:
            assert (slot.k_codes, slot.v_codes, slot.k_scales, slot.v_scales) == tuple(t.data_ptr() for t in b)
            assert slot.capacity == b[0].shape[2] and (lay._kc, lay._vc, lay._ks, lay._vs) == b
            assert lay.codes()[0].shape[2] == T0 + 1
        else:
            assert (slot.k_cache, slot.v_cache, slot.kv_stride) == (b[0].data_ptr(), b[1].data_ptr(), b[0].stride(1))
            assert lay._kb is b[0] and lay._vb is b[1] and lay.keys.data_ptr() == b[0].data_ptr()
        assert lay.get_seq_length() == T0 + 1
    key = "padded_decode" if left else "decode"
    moved = {k: getattr(prefill, k)[key] - n0[k][key] for k in n0}
    assert moved == {"stats": NL, "stack_stats": 1, "kv8_stats": NL * q8, "stack_kv8_stats": int(q8)}


def test_a_second_step_rewrites_positions_alone(handle):
    """the next token's call: the same descriptor array, every slot one position on"""
    m, cache, _ = _setup(("append", "append"), 2, False, stack_decode=True)
    plan = []
    for layer in m.model.layers:
        pr = prefill._SplitLayout.projections(layer)
        d, sc = prefill._decode_state(layer, 2, torch.device("cpu"), pr)
        plan.append((layer, layer._u2_prefill, pr, d, sc, W))
    x = torch.zeros(2, 1, 128, dtype=bf)
    prefill._stack_step(m.model, plan, None, x, cache, None)
    prefill._stack_step(m.model, plan, None, x, cache, None)
    (_, a), (_, b) = handle.entries()
    assert a[0] is b[0] and len([c for c in handle.calls if c[0].endswith("_workspace_bytes")]) == 1
    for i in range(NL):
        assert (b[0][i].s_off, b[0][i].k_first, b[0][i].T) == (T0 + 1, T0 + 2 - W, W) and cache.layers[i].get_seq_length() == T0 + 2
