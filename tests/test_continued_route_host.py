"""CPU: the continued prefill's host side (`enable_fused_prefill(model, continued=True)`): `route()`'s decisions over stub layers
and caches -- switch off / on, cache empty / filled, S <= W / S > W, every cache kind, every mask kind, the combinations that
stay stock --, the config switch, the band rule of u2tok_attention_gqa_band against HF's own sliding-window causal mask, and the
C entry point's argument checks (no launch)."""
import contextlib
import types

import pytest
import torch

from u2tokenizer_amd import decoder_train, ops, prefill

bf = torch.bfloat16


class _FakeCuda(torch.Tensor):
    @property
    def is_cuda(self):
        return True


def _model(kind="qwen3", head_dim=64, hidden=128, inter=256, window=None):
    from transformers import LlamaConfig, LlamaForCausalLM, Phi3Config, Phi3ForCausalLM, Qwen3Config, Qwen3ForCausalLM
    c = dict(vocab_size=64, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=1, max_position_embeddings=256)
    if kind == "phi3":
        c.update(num_attention_heads=hidden // head_dim, num_key_value_heads=hidden // head_dim, sliding_window=window,
                 pad_token_id=0, bos_token_id=1, eos_token_id=2)
        cfg, cls = Phi3Config, Phi3ForCausalLM
    else:
        c.update(num_attention_heads=2, num_key_value_heads=1, head_dim=head_dim)
        cfg, cls = (Qwen3Config, Qwen3ForCausalLM) if kind == "qwen3" else (LlamaConfig, LlamaForCausalLM)
    torch.manual_seed(0)
    return cls(cfg(**c)).to(bf).eval()


def _stock(self, hidden_states, *args, past_key_values=None, position_embeddings=None, **kwargs) -> torch.Tensor:
    self._calls.append("stock")
    return hidden_states


@pytest.fixture
def recorder(monkeypatch):
    calls = []

    def decode(layer, x, pe, cache, window=None, pr=None):
        calls.append(("decode", window))
        return x

    def step(layer, lo, x, pe, cache, window=None, extend=False):
        calls.append(("extend", window) if extend else "prefill")
        return x

    monkeypatch.setattr(prefill, "_decode_step", decode)
    monkeypatch.setattr(prefill, "_prefill_step", step)
    monkeypatch.setattr(decoder_train, "layer_forward_train", lambda *a, **k: calls.append("train"))
    monkeypatch.setattr(ops, "on_device", lambda *a, **k: contextlib.nullcontext((None, None)))
    return calls


def _patch(m, calls, **flags):
    for layer in m.model.layers:
        layer._calls = calls
        layer.forward = types.MethodType(_stock, layer)
    prefill.enable_fused_prefill(m, **flags)


def _cache(m, B, T, kind):
    """A cache of `kind` holding T positions in layer 0 (T = 0: empty; kind None: no cache)."""
    from transformers import cache_utils as cu
    if kind is None:
        return None
    att = m.model.layers[0].self_attn
    kv = torch.zeros(B, m.config.num_key_value_heads, T, att.head_dim, dtype=bf)
    if kind == "config":      # what `generate` builds: DynamicSlidingWindowLayer for a windowed config, else DynamicLayer
        cache = cu.DynamicCache(config=m.config)
    elif kind == "plain":     # DynamicLayers created lazily
        cache = cu.DynamicCache()
    elif kind == "append":
        cache = cu.DynamicCache()
        cache.layers.append(prefill._append_layer_class()())
    elif kind == "sliding layer":   # a DynamicSlidingWindowLayer put there by hand
        cache = cu.DynamicCache()
        cache.layers.append(cu.DynamicSlidingWindowLayer(sliding_window=4))
    elif kind == "offloaded":
        cache = cu.DynamicCache()
        cache.offloading = True   # (the flag DynamicCache(offloading=True) sets; its constructor wants a device stream)
    elif kind == "static":
        cache = cu.StaticCache(config=m.config, max_cache_len=64)
    elif kind == "subclass":
        cache = type("MyCache", (cu.DynamicCache,), {})()
    elif kind == "other layer":
        cache = cu.DynamicCache()
        cache.layers.append(type("OtherLayer", (cu.DynamicLayer,), {})())   # (a class of its own: not what the route knows)
    if T:
        if kind == "offloaded":   # (no stream to prefetch on without a GPU: fill the layer itself)
            cache.layers.append(cu.DynamicLayer())
            cache.layers[0].update(kv, kv)
        else:
            cache.update(kv, kv, 0)
    return cache


def _route(m, calls, stack_mask, B=2, S=8, T=0, cache="plain"):
    """The route one call of layer 0 takes after the decoder stack's pre-hook has judged `stack_mask` (None: no mask)."""
    layer = m.model.layers[0]
    prefill._mask_hook(m.model, (), {"attention_mask": stack_mask})
    calls.clear()
    x = torch.zeros(B, S, m.config.hidden_size, dtype=bf).as_subclass(_FakeCuda)
    d = layer.self_attn.head_dim
    kwargs = dict(attention_mask=None, position_embeddings=(torch.ones(B, S, d, dtype=bf), torch.zeros(B, S, d, dtype=bf)),
                  past_key_values=_cache(m, B, T, cache))
    with torch.no_grad():
        layer(x, **kwargs)
    assert len(calls) == 1, calls
    return calls[0]


def _mask(kind, B=2, S=8):
    m = torch.ones(B, S, dtype=torch.int64)
    if kind == "left":
        m[-1, :3] = 0
    elif kind == "right":
        m[-1, S - 3:] = 0
    elif kind == "hole":
        m[-1, 2] = 0
    return m


PHI3W = dict(kind="phi3", hidden=192, head_dim=96, window=6)   # W = 6: the S = 8 calls below are longer than the window
ONES = "ones"

# name -> (model kwargs, stack mask (None / ONES / tensor), call kwargs, route with continued=True [, enable flags])
TABLE = {
    # cache filled, S > 1: every cache kind the route takes
    "second turn, plain DynamicLayer": ({}, None, dict(T=5), ("extend", None)),
    "second turn, config-built cache": ({}, None, dict(T=5, cache="config"), ("extend", None)),
    "second turn, append-in-place layer": ({}, None, dict(T=5, cache="append"), ("extend", None)),
    "second turn, llama": (dict(kind="llama"), None, dict(T=5), ("extend", None)),
    "second turn, head dim 96": (dict(head_dim=96), None, dict(T=5), ("extend", None)),
    "second turn, mask of ones over cache + call": ({}, ONES, dict(T=5), ("extend", None)),
    "second turn, two rows": ({}, None, dict(T=5, B=1, S=2), ("extend", None)),
    "second turn, batch 32": ({}, None, dict(T=5, B=32, S=3), ("extend", None)),
    # ... and those it leaves to the stock layers
    "second turn, offloaded cache": ({}, None, dict(T=5, cache="offloaded"), "stock"),
    "second turn, static cache": ({}, None, dict(T=5, cache="static"), "stock"),
    "second turn, DynamicCache subclass": ({}, None, dict(T=5, cache="subclass"), "stock"),
    "second turn, unknown layer class": ({}, None, dict(T=5, cache="other layer"), "stock"),
    "second turn, sliding layer under a layer without a window": (dict(kind="phi3", hidden=192, head_dim=96, window=None), None,
                                                                dict(T=5, cache="sliding layer"), "stock"),
    "second turn, head dim 32": (dict(head_dim=32), None, dict(T=5), "stock"),
    # masks on a continuation
    "second turn, left padding, padded off": ({}, _mask("left", S=13), dict(T=5), "stock"),
    "second turn, left padding": ({}, _mask("left", S=13), dict(T=5), ("extend", None), dict(padded=True)),
    "second turn, left padding, append layer": ({}, _mask("left", S=13), dict(T=5, cache="append"), ("extend", None), dict(padded=True)),
    "second turn, left padding of another width": ({}, _mask("left", S=8), dict(T=5), "stock", dict(padded=True)),
    "second turn, right padding": ({}, _mask("right", S=13), dict(T=5), "stock", dict(padded=True)),
    "second turn, hole": ({}, _mask("hole", S=13), dict(T=5), "stock", dict(padded=True)),
    "second turn, window + left padding": (PHI3W, _mask("left", S=13), dict(T=5), "stock", dict(padded=True)),
    # a layer with a window W = 6
    "window, S <= W, empty cache": (PHI3W, None, dict(S=6), "prefill"),
    "window, S > W, no cache": (PHI3W, None, dict(cache=None), ("extend", 6)),
    "window, S > W, empty plain cache": (PHI3W, None, {}, ("extend", 6)),
    "window, S > W, empty sliding cache": (PHI3W, None, dict(cache="config"), ("extend", 6)),
    "window, S > W, mask of ones": (PHI3W, ONES, dict(cache="config"), ("extend", 6)),
    "window, S > W, static cache": (PHI3W, None, dict(cache="static"), "stock"),
    "window, S > W, left padding": (PHI3W, _mask("left"), dict(cache=None), "stock", dict(padded=True)),
    "window, S <= W, filled sliding cache": (PHI3W, None, dict(S=4, T=9, cache="config"), ("extend", 6)),
    "window, S <= W, filled plain cache": (PHI3W, None, dict(S=4, T=9), ("extend", 6)),
    "window, S > W, filled append layer": (PHI3W, None, dict(T=9, cache="append"), ("extend", 6)),
    # what the other routes keep
    "first turn": ({}, None, {}, "prefill"),
    "first turn, no cache": ({}, None, dict(cache=None), "prefill"),
    "decode step": ({}, None, dict(S=1, T=5), ("decode", None)),
    "decode step, window": (PHI3W, None, dict(S=1, T=9, cache="config"), ("decode", 6)),
}


def _case(name, recorder, **flags):
    mk, mask, call, want, *extra = TABLE[name]
    m = _model(**mk)
    _patch(m, recorder, **{**(extra[0] if extra else {}), **flags})
    B, S, T = call.get("B", 2), call.get("S", 8), call.get("T", 0)
    if isinstance(mask, str):
        mask = torch.ones(B, S + T, dtype=torch.int64)
    return _route(m, recorder, mask, **call), want


@pytest.mark.parametrize("name", list(TABLE))
def test_continued_route(recorder, name):
    got, want = _case(name, recorder, continued=True)
    assert got == want


@pytest.mark.parametrize("name", list(TABLE))
def test_without_the_switch_every_call_routes_as_before(recorder, name):
    """continued=False (the default): what the table sends to the new route is stock, everything else is unchanged."""
    got, want = _case(name, recorder)
    assert got == ("stock" if isinstance(want, tuple) and want[0] == "extend" else want)


def test_switch_is_set_anew_by_every_enable_call(recorder):
    m = _model()
    _patch(m, recorder, continued=True)
    assert m.model._u2_stack.continued is True
    prefill.enable_fused_prefill(m)
    assert m.model._u2_stack.continued is False
    assert _route(m, recorder, None, T=5) == "stock"


def test_lm_config_switch_is_passed_on(monkeypatch):
    """`config.u2_fused_continued_prefill` reaches enable_fused_prefill as `continued` (default: not passed, so False)."""
    from u2tokenizer_amd import language_model as LM
    seen = []
    monkeypatch.setattr(prefill, "enable_fused_prefill", lambda model, **kw: seen.append(kw) or 0)
    for on in (None, True):
        cfg = LM.u2Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                               num_key_value_heads=2, head_dim=16)
        if on is not None:
            cfg.u2_fused_continued_prefill = on
        m = LM.u2Qwen3ForCausalLM(cfg).to(bf).eval()
        layer = m.model.layers[0]
        p0 = next(layer.parameters())
        layer.parameters = lambda *a, p0=p0, **k: iter([p0.detach().as_subclass(_FakeCuda)])
        with torch.no_grad():
            m(inputs_embeds=torch.zeros(1, 3, 64, dtype=bf))
    assert [kw.get("continued", False) for kw in seen] == [False, True]
    assert all("padded" not in kw for kw in seen)


def test_the_continued_counters_live_next_to_stats_not_in_it():
    assert set(prefill.stats) == {"prefill", "decode", "padded_prefill", "padded_decode"}
    assert prefill.extend_stats.keys() == {"extend", "padded_extend"}


# ------------------------------------------------------------------------------------------------------------ band rule
def band_visible(Sq: int, Skv: int, W, kv_start: int = 0, kv_len=None) -> torch.Tensor:
    """The kernel's rule as a (Sq, Skv) bool table: key j is visible to query i iff i + c_off - W < j <= i + c_off with
    c_off = Skv - Sq (W = 0 / None: no lower edge) and kv_start <= j < kv_len."""
    i, j = torch.arange(Sq)[:, None], torch.arange(Skv)[None, :]
    c = Skv - Sq
    vis = j <= i + c
    if W:
        vis = vis & (j > i + c - W)
    return vis & (j >= kv_start) & (j < (Skv if kv_len is None else kv_len))


def _hf_sliding_mask(Sq: int, Skv: int, W: int) -> torch.Tensor:
    """HF's own sliding-window causal mask for Sq queries at the end of Skv keys, as a (Sq, Skv) bool table; the rule
    `i - j < W` on absolute positions where this transformers has no masking utilities to import."""
    q_pos = torch.arange(Skv - Sq, Skv)
    try:
        from transformers.masking_utils import and_masks, causal_mask_function, sliding_window_overlay
        fn = and_masks(sliding_window_overlay(W), causal_mask_function)
        z = torch.zeros((), dtype=torch.long)
        return torch.tensor([[bool(fn(z, z, qi, kj)) for kj in torch.arange(Skv)] for qi in q_pos])
    except ImportError:
        j = torch.arange(Skv)[None, :]
        return (j <= q_pos[:, None]) & (q_pos[:, None] - j < W)


# (Sq, Skv, W): the shapes of tests/test_gpu_continued_prefill.py
@pytest.mark.parametrize("Sq,Skv,W", [(200, 200, 32), (200, 200, 64), (130, 130, 1), (70, 70, 500), (70, 200, 96), (37, 68, 32),
                                      (20, 51, 32), (70, 70, 32)])
def test_band_rule_is_hfs_sliding_window_mask(Sq, Skv, W):
    vis = band_visible(Sq, Skv, W)
    assert torch.equal(vis, _hf_sliding_mask(Sq, Skv, W))
    assert (vis.sum(1) == torch.clamp(torch.arange(Sq) + Skv - Sq + 1, max=W)).all()   # W keys, the query's own included
    assert vis[torch.arange(Sq), torch.arange(Sq) + Skv - Sq].all()


def test_band_rule_of_a_sliding_cache_operand_is_the_rule_on_absolute_positions():
    """A DynamicSlidingWindowLayer hands back its kept W - 1 positions plus the S new ones: the relative rule on that operand is
    the absolute rule on the whole history, columns before the operand being invisible anyway."""
    W, S, T0 = 32, 37, 90
    whole = band_visible(S, T0 + S, W)
    kept = band_visible(S, W - 1 + S, W)
    assert torch.equal(whole[:, T0 - (W - 1):], kept) and not whole[:, :T0 - (W - 1)].any()


def test_a_band_can_mask_a_rows_whole_first_tile():
    """The hazard the kernel handles: with 64-key tiles and 64-row query blocks, a block whose first row's band starts mid-tile
    loads a first tile in which its later rows see nothing although they see keys in the next one."""
    W, S = 32, 200
    vis = band_visible(S, S, W)
    q0 = 64
    kt0 = max(0, q0 - W + 1) // 64                                       # first tile the block loads
    rows = [i for i in range(q0, q0 + 64) if not vis[i, kt0 * 64:kt0 * 64 + 64].any()]
    assert rows and min(rows) == 95 and all(vis[i].any() for i in rows)


# ------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("elem", ["bf16", "f16"])
def test_attention_gqa_band_rejects_bad_arguments(elem):
    """u2tok_attention_gqa_band returns before any launch on arguments it cannot take."""
    from u2tokenizer_amd import _lib
    h = _lib.load_library(elem)
    P = 1 << 20   # an aligned address that is never dereferenced
    # q, k, v, out, nb, Sq, Skv, Hq, Hkv, d, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, scale, causal, kv_start, kv_len, lse,
    # lse_ld, k_hs, v_hs, window, stream: 8 new rows against a cache view of 24 positions in buffers of 64
    args = [P, P, P, P, 1, 8, 24, 4, 2, 64, 512, 64, 64, 256, 4096, 2 * 64 * 64, 2 * 64 * 64, 2048, 0.1, 1, None, None, None, 0,
            64 * 64, 64 * 64, 16, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return h.u2tok_attention_gqa_band(*a)

    for i in (0, 1, 2, 3):
        assert call(**{f"a{i}": None}) == -1, i
    assert call(a9=256) == -1 and call(a9=32) == -1            # head dims of the band kernel: 64 / 96 / 128
    assert call(a26=-1) == -1                                  # window
    assert call(a19=0) == -1                                   # a window without the causal mask
    assert call(a24=64 * 64 + 4) == -1 and call(a25=0) == -1   # head strides: positive multiples of 8
    assert call(a5=32) == -1                                   # causal with more queries than keys
    assert call(a20=P + 2) == -1                               # kv_start not 4-byte aligned
    assert call(a7=3) == -1                                    # Hq % Hkv
