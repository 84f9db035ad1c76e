"""CPU: prefill._KVWrite, the one rule of the prefill, the continued prefill and the decode step for where new keys / values go,
what the step attends over and when the cache is committed -- on CPU tensors, nothing launched.  Pinned here: an append-in-place
layer is recognised by the batch of its `.keys` at every site, so a layer whose keys were reordered or re-batched between two
steps (beam search, batch selection: `.keys` reassigned, the buffers still the old ones) is re-homed by `_room` and written in
place at once; a batch that does not match, and every other layer class, goes through the cache's own `update`."""
import torch
from transformers.cache_utils import DynamicCache

from u2tokenizer_amd import prefill

B, H, D = 3, 2, 4


def _filled(T=5, batch=B):
    """a plain DynamicCache whose layer 0 is the append-in-place layer a fused prefill of T positions leaves"""
    cache = DynamicCache()
    lay = prefill._prefill_append_layer(cache, 0, batch, H, T, D, torch.zeros(1))
    assert type(lay) is prefill._append_layer_class() and cache.layers[0] is lay
    lay._kb.copy_(torch.arange(lay._kb.numel(), dtype=torch.float32).view_as(lay._kb))
    lay._vb.copy_(-lay._kb)
    lay._commit(T)
    return cache, lay


def _like(batch=B):
    return torch.empty(batch, H, 1, D)


def test_decode_step_writes_behind_the_old_positions_in_place():
    cache, lay = _filled()
    kb = lay._kb
    kv = prefill._KVWrite(cache, 0, B, 1, None, like=_like())
    assert kv.lay is lay and kv.T0 == 5 and lay._kb is kb                     # room was there: the same buffers
    K, V, stride = kv.views(None, None, kb.stride(1))
    assert K.shape == (B, H, 6, D) and K.data_ptr() == kb.data_ptr() and V.data_ptr() == lay._vb.data_ptr() and stride == kb.stride(1)
    assert lay.keys.shape[2] == 5
    kv.commit()
    assert lay.keys.shape[2] == 6 and lay.keys.data_ptr() == kb.data_ptr() and cache.get_seq_length(0) == 6


def test_window_views_of_an_in_place_layer():
    cache, lay = _filled(T=9)
    kv = prefill._KVWrite(cache, 0, B, 1, 4, like=_like())                    # a decode step: the last W positions
    K, _, _ = kv.views(None, None)
    assert K.shape[2] == 4 and torch.equal(K, lay._kb[:, :, 6:10])
    kv = prefill._KVWrite(cache, 0, B, 3, 4)                                  # 3 new positions: the last n + W - 1
    assert kv.T0 == 9
    K, _, _ = kv.views(None, None)
    assert K.shape[2] == 6 and torch.equal(K, lay._kb[:, :, 6:12])
    kv = prefill._KVWrite(cache, 0, B, 3, 40)                                 # a window longer than the cache: everything
    assert kv.views(None, None)[0].shape[2] == 12


def test_a_rebatched_layer_is_rehomed_and_written_in_place_at_once():
    cache, lay = _filled()
    old_kb, old_keys = lay._kb, lay.keys.clone()
    lay.keys, lay.values = lay.keys[[2, 0]], lay.values[[2, 0]]               # what batch selection / beam reordering do
    for n, like in ((1, _like(2)), (3, None)):                                # the decode step's call and the continued prefill's
        c, l = cache, lay
        kv = prefill._KVWrite(c, 0, 2, n, None, like=like)
        assert kv.lay is l and kv.T0 == 5
        assert l._kb is not old_kb and l._kb.shape[:2] == (2, H) and l._kb.shape[2] >= 5 + n
        assert torch.equal(l.keys, old_keys[[2, 0]]) and l.keys.data_ptr() == l._kb.data_ptr()
        assert kv.views(None, None)[0].shape == (2, H, 5 + n, D)
    # ... a reordered layer of the same batch as well (the buffers' batch still matches: only `.keys` tells)
    cache, lay = _filled()
    kb = lay._kb
    lay.keys, lay.values = lay.keys[[1, 2, 0]], lay.values[[1, 2, 0]]
    kv = prefill._KVWrite(cache, 0, B, 1, None, like=_like())
    assert kv.lay is lay and lay._kb is not kb and torch.equal(lay._kb[:, :, :5], kb[[1, 2, 0], :, :5])


class _Counting(DynamicCache):
    updates = 0

    def update(self, *a, **k):
        self.updates += 1
        return super().update(*a, **k)


def _dense(T=5, batch=B):
    cache = _Counting()
    kv = torch.arange(batch * H * T * D, dtype=torch.float32).view(batch, H, T, D)
    cache.update(kv, -kv, 0)
    cache.updates = 0
    return cache


def test_every_other_layer_goes_through_update_once():
    new = torch.ones(B, H, 1, D)
    for window, keys in ((None, 6), (4, 4), (40, 6)):
        cache = _dense()
        kv = prefill._KVWrite(cache, 0, B, 1, window, like=_like())
        assert kv.lay is None and kv.T0 == 0
        K, V, stride = kv.views(new, -new)
        assert cache.updates == 1 and K.shape == (B, H, keys, D) and torch.equal(K[:, :, -1:], new) and torch.equal(V, -K)
        assert stride == (0 if keys == 6 else 6 * D) and K.stride(2) == D and K.stride(3) == 1
        kv.commit(new, -new)
        assert cache.updates == 1                                             # (updated in `views`: nothing left)
    # several new positions: what `update` returned, whole, whatever the window (the band kernel masks relative to the last key)
    cache = _dense()
    new = torch.ones(B, H, 3, D)
    kv = prefill._KVWrite(cache, 0, B, 3, 4)
    K, _, stride = kv.views(new, -new)
    assert K.shape == (B, H, 8, D) and stride == 0 and K.is_contiguous() and K.data_ptr() == cache.layers[0].keys.data_ptr()
    # a batch that is not the layer's: not in place, T0 = 0
    cache, lay = _filled()
    assert prefill._KVWrite(cache, 0, B + 1, 1, None, like=_like(B + 1)).lay is None


def _codes(T=9, batch=B):
    """a plain DynamicCache whose layer 0 is a `Kv8Layer` of T positions whose codes say they are on the GPU"""
    from test_decoder_route_host import _FakeCuda
    cache = DynamicCache()
    lay = prefill.Kv8Layer()
    kv = torch.arange(batch * H * T * D, dtype=torch.float32).view(batch, H, T, D)
    lay.update(kv, -kv)
    lay._kc = lay._kc.as_subclass(_FakeCuda)
    cache.layers.append(lay)
    return cache, lay


def test_the_codes_kind():
    cache, lay = _codes()
    bufs = lay._buffers()
    for n, like in ((1, _like()), (3, None)):                                 # the decode step's call and the continued prefill's
        kv = prefill._KVWrite(cache, 0, B, n, 4, like=like)
        assert kv.kind is prefill.KV8 and kv.lay is lay and kv.T0 == 9 and lay._buffers() == bufs
        assert kv.first == 6                                                  # the last n + W - 1 of T0 + n: 9 + 1 - 4, whatever n
        assert lay.get_seq_length() == 9                                      # (nothing is the layer's before `commit`)
    kv = prefill._KVWrite(cache, 0, B, 1, None, like=_like())
    assert kv.first == 0 and kv.T0 == 9
    kv = prefill._KVWrite(cache, 0, B, 1, 40, like=_like())                   # a window longer than the cache: everything
    assert kv.first == 0
    kv.commit()
    assert lay.get_seq_length() == 10 and lay.codes()[0].shape[2] == 10 and lay._buffers() == bufs
    # a re-batched layer (batch selection: the codes now hold two sequences) is not written in place for a call of three ...
    lay.batch_select_indices(torch.tensor([2, 0]))
    kv = prefill._KVWrite(cache, 0, B, 1, None, like=_like())
    assert kv.kind is not prefill.KV8 and kv.lay is None and kv.T0 == 0
    new = torch.ones(B, H, 1, D)
    try:                                                                      # ... and its own `update` refuses the rows
        kv.views(new, -new)
        raise AssertionError("a Kv8Layer took rows of another batch")
    except RuntimeError as e:
        assert "against a cache of" in str(e)
    assert lay.get_seq_length() == 10
    # ... nor are codes on the CPU, or an empty layer
    cache, lay = _codes()
    lay._kc = lay._kc.as_subclass(torch.Tensor)
    assert prefill._KVWrite(cache, 0, B, 1, None, like=_like()).kind is not prefill.KV8
    cache.layers[0] = prefill.Kv8Layer()
    assert prefill._KVWrite(cache, 0, B, 1, None, like=_like()).lay is None


def test_first_call_into_a_layer():
    cache = DynamicCache()
    x = torch.zeros(1)
    kv = prefill._KVWrite(cache, 0, B, 7, None, fresh=(H, D, x))              # an empty plain cache: the append-in-place layer
    lay = kv.lay
    assert type(lay) is prefill._append_layer_class() and cache.layers[0] is lay and kv.T0 == 0 and lay._kb.shape[2] >= 14
    kv.commit()
    assert cache.get_seq_length(0) == 7
    cache = _Counting()                                                       # another cache class: dense, updated by `commit`
    kv = prefill._KVWrite(cache, 0, B, 7, None, fresh=(H, D, x))
    assert kv.lay is None and cache.updates == 0
    new = torch.ones(B, H, 7, D)
    kv.commit(new, new)
    assert cache.updates == 1 and cache.get_seq_length(0) == 7
    kv = prefill._KVWrite(None, 0, B, 7, None, fresh=(H, D, x))               # no cache: nothing to do
    assert kv.lay is None and kv.T0 == 0
    kv.commit(None, None)
