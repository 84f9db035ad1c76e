"""GPU: the tokenizer's attention at head dim 384 (E = 3072: Phi-3-mini / Llama-3.2-3B as the decoder) on the fused kernels --
tok_attn_kernel<384> (u2tok_tok_attention, u2tok_attention_gqa), temporal_attention_kernel<6> (u2tok_temporal_attention) and
the routing of a whole tokenizer forward -- on both element builds.

Building blocks: the bound, the reference expression and the scale of tests/test_gpu_ops.py (imported: a bf16 / fp16 result
may be two roundings of the fp32 value of the same inputs away).  The float16 cases choose the build the way
tests/test_gpu_f16.py does: that module's element type and ulp are switched, and the library is picked by the tensors' dtype.
Whole forward: the three-distance gate of tests/test_gpu_configs.py (imported) against oracle/u2_oracle.py in fp32, with
the reference's own bf16 run as the yardstick.
"""
import ctypes as C
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import test_gpu_ops as T
from cases import TOKENIZER_CASES, tokenizer_inputs
from helpers import err_stats, tok_cfg
from oracle import u2_oracle as O
from test_gpu_configs import gate, three_way
from test_gpu_ops import _tok_attn_ref, close_bf16, rnd
from u2tokenizer_amd import synth

pytestmark = pytest.mark.gpu
D = "cuda"
PROF_TEMPORAL, PROF_TOKATTN = 2, 5   # kernels.h: the profile's launch classes


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


@pytest.fixture(params=["bf16", "f16"])
def elem(request, monkeypatch):
    """float16: rnd() draws fp16 inputs, close_bf16() allows two fp16 roundings and ops dispatches to libu2tok_hip_f16.so"""
    if request.param == "f16":
        monkeypatch.setattr(T, "bf", torch.float16)
        monkeypatch.setattr(T, "ULP", 2.0 ** -11)
    return request.param


def _launches(ops, device, fn):
    """fn() under option "profile" -> (its result, launches per class), as tests/test_gpu_path.py reads them"""
    from u2tokenizer_amd import _lib
    ops.set_option("profile", 1)
    try:
        out = fn()
        torch.cuda.synchronize()
        h = _lib.load_library()
        h.u2tok_ctx_set_current(ops.active_context(torch.device(device)).handle)
        ms, fl, by, cnt = (C.c_double * 6)(), (C.c_double * 6)(), (C.c_double * 6)(), (C.c_int64 * 6)()
        _lib.check(h.u2tok_profile_collect2(ms, fl, by, cnt, 6), "u2tok_profile_collect2")
    finally:
        ops.set_option("profile", 0)
    return out, list(cnt)


# ------------------------------------------------------------------------------------------------ u2tok_tok_attention
def _packed_qkv(nb, Sq, Skv, E):
    """q / k / v as column slices of packed buffers, as the pipeline passes them (host tensors, device views)"""
    if Sq == Skv:
        qkv = rnd(nb, Sq, 3 * E, seed=Sq + 384)
        dq = qkv.to(D)
        return (qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]), (dq[..., :E], dq[..., E:2 * E], dq[..., 2 * E:])
    q, kv = rnd(nb, Sq, E, seed=Sq), rnd(nb, Skv, 2 * E, seed=Skv)
    dkv = kv.to(D)
    return (q, kv[..., :E], kv[..., E:]), (q.to(D), dkv[..., :E], dkv[..., E:])


@pytest.mark.parametrize("nb,Sq,Skv,H,bias,splits", [
    (1, 1, 1, 1, True, 0),          # one key, one query
    (1, 16, 33, 1, False, 2),       # a one-key tail tile and a two-way merge
    (2, 37, 53, 2, True, 0),        # tails everywhere, a head offset of 384 inside E = 768, a batch stride
    (2, 37, 53, 2, True, 2),
    (1, 64, 96, 1, False, 0),       # whole blocks only
    (1, 130, 97, 2, True, 0),       # three query blocks
    (1, 64, 320, 1, False, 10)])    # the run-time merge behind eight splits
def test_tok_attention_d384(ops, elem, nb, Sq, Skv, H, bias, splits):
    """u2tok_tok_attention at d = 384 against the fp32 softmax(q k^T scale + bias) v of the same inputs; three launches agree
    bit for bit; option tok_wide = 0 and 2 give the same bits (there is no 8-wave form at 384: both run tok_attn_kernel<384>)."""
    d = 384
    E = H * d
    (q, k, v), (dq, dk, dv) = _packed_qkv(nb, Sq, Skv, E)
    tbl = rnd(1023, H, scale=0.5, seed=3) if bias else None
    dt = None if tbl is None else tbl.to(D)
    scale = 2.0 / math.sqrt(d)
    ref = _tok_attn_ref(q, k, v, H, scale, tbl)
    got = [ops.tok_attention(dq, dk, dv, H, scale, dt, 512, splits) for _ in range(3)]
    assert got[0].dtype == T.bf
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    close_bf16(got[0], ref)
    try:
        for wide in (0, 2):
            ops.set_option("tok_wide", wide)
            g = ops.tok_attention(dq, dk, dv, H, scale, dt, 512, splits)
            close_bf16(g, ref)
            assert torch.equal(g, got[0]), wide
    finally:
        ops.set_option("tok_wide", 2)


def test_tok_attention_d384_forced_rescale_and_split_merge(ops, elem):
    """One key row aligned with every query in the LAST tile (the running max jumps there), unsplit and with the keys cut so
    that it lies in the last split: the merge weights of the other splits are tiny."""
    nb, Sq, Skv, H, d = 1, 128, 160, 2, 384
    q, kv = rnd(nb, Sq, H * d, seed=5), rnd(nb, Skv, 2 * H * d, seed=6)
    for h in range(H):
        kv[0, 133, h * d:(h + 1) * d] = (q[0, :, h * d:(h + 1) * d].float().mean(0) * 40 + 3 * q[0, 7, h * d:(h + 1) * d].float()).to(T.bf)
    k, v = kv[..., :H * d], kv[..., H * d:]
    ref = _tok_attn_ref(q, k, v, H, 1 / math.sqrt(d))
    s = q[0, :, :d].float() @ k[0, :, :d].float().t() / math.sqrt(d) * 1.4427          # scores in log2 units
    assert s[7, 133] - s[7, :128].max() > 64   # the running max of row 7 (and with it its wave's rescale) does jump in the last tile
    dkv = kv.to(D)
    for splits in (1, 2, 5):              # 5 tiles of 32 keys: (3 | 2) and one tile each -- key 133 in the last split
        close_bf16(ops.tok_attention(q.to(D), dkv[..., :H * d], dkv[..., H * d:], H, 1 / math.sqrt(d), None, 512, splits), ref)


@pytest.mark.parametrize("causal,Sq,Skv,Hq,Hkv", [(True, 70, 70, 2, 1), (True, 5, 69, 1, 1), (False, 37, 53, 2, 2)])
def test_attention_gqa_d384(ops, elem, causal, Sq, Skv, Hq, Hkv):
    """u2tok_attention_gqa shares the kernel: grouped heads and the causal mask at d = 384 come with it"""
    d = 384
    q, kv = rnd(1, Sq, Hq * d, seed=21), rnd(1, Skv, 2 * Hkv * d, seed=22)
    k, v = kv[..., :Hkv * d], kv[..., Hkv * d:]
    qh = q.float().view(1, Sq, Hq, d).permute(0, 2, 1, 3)
    kh, vh = (t.float().view(1, Skv, Hkv, d).permute(0, 2, 1, 3).repeat_interleave(Hq // Hkv, 1) for t in (k, v))
    s = qh @ kh.transpose(-1, -2) * (2.0 / math.sqrt(d))
    if causal:
        s = s.masked_fill(torch.arange(Skv)[None, :] > torch.arange(Sq)[:, None] + (Skv - Sq), float("-inf"))
    ref = (F.softmax(s, dim=-1) @ vh).permute(0, 2, 1, 3).reshape(1, Sq, Hq * d)
    dkv = kv.to(D)
    got = ops.attention_gqa(q.to(D), dkv[..., :Hkv * d], dkv[..., Hkv * d:], Hq, Hkv, 2.0 / math.sqrt(d), causal=causal)
    close_bf16(got, ref)


# ------------------------------------------------------------------------------------------------ u2tok_temporal_attention
@pytest.mark.parametrize("B,T_,N,H", [(1, 8, 5, 2), (2, 1, 3, 1), (1, 16, 4, 8), (1, 3, 7, 2)])
def test_temporal_attention_d384(ops, elem, B, T_, N, H):
    d = 384
    E = H * d
    qkv, tbl = rnd(B * T_ * N, 3 * E, seed=d), rnd(1023, H, scale=0.5, seed=3)
    qd = qkv.to(D)
    got = ops.temporal_attention(qd[:, :E], qd[:, E:2 * E], qd[:, 2 * E:], B, T_, N, H, 1 / math.sqrt(d), tbl.to(D), 512)
    x = qkv.float().view(B, T_, N, 3, H, d).permute(3, 0, 2, 4, 1, 5)
    pos = torch.arange(T_)
    bias = tbl.float()[pos[None, :] - pos[:, None] + 511].permute(2, 0, 1)
    p = F.softmax(x[0] @ x[1].transpose(-1, -2) / math.sqrt(d) + bias[None, None], dim=-1)
    close_bf16(got, (p @ x[2]).permute(0, 3, 1, 2, 4).reshape(B * T_ * N, E))


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_points_without_a_384_form_refuse_it(ops, elem):
    """u2tok_attention_gqa_ex / _range with a key range or row statistics, _band with a window or a cache view and
    u2tok_decode_attention have no d = 384 kernel: U2TOK_ERR_ARG, and nothing is launched"""
    d, S = 384, 40
    q = rnd(2, S, d, seed=31).to(D)
    n = torch.full((2,), S - 3, dtype=torch.int32, device=D)
    z = torch.zeros((2,), dtype=torch.int32, device=D)
    cache = rnd(2, 1, 64, d, seed=32).to(D)
    calls = [lambda: ops.attention_gqa_ex(q, q, q, 1, 1, 0.05, kv_len=n),
             lambda: ops.attention_gqa_ex(q, q, q, 1, 1, 0.05, with_lse=True),
             lambda: ops.attention_gqa_range(q, q, q, 1, 1, 0.05, kv_start=z),
             lambda: ops.attention_gqa_range(q, q, q, 1, 1, 0.05, kv_len=n, causal=False),
             lambda: ops.attention_gqa_band(q, q, q, 1, 1, 0.05, window=8),
             lambda: ops.attention_gqa_band(q, cache[:, :, :S], cache[:, :, :S], 1, 1, 0.05),
             lambda: ops.decode_attention(q[:, 0], cache[:, :, :S], cache[:, :, :S], 1, 1, 0.05)]

    def run():
        for f in calls:
            with pytest.raises(RuntimeError, match="U2TOK_ERR_ARG"):
                f()
    _, cnt = _launches(ops, D, run)
    assert sum(cnt) == 0, cnt


# ------------------------------------------------------------------------------------------------ the tokenizer forward
QK_GAIN = 2.0
"""Query / key gain of the forward test's parameters (synth.lively_).  At gain 1 the two residual-free SVR layers collapse the
tokens onto their mean (diversity 2e-4 in the fp32 oracle), at the default 4 the chain is chaotic at this width (the reference's
own bf16 run is 116 % away from its fp32 run); at 2 the fp32 output keeps a token diversity of 0.3 and the bf16 reference
stays within 2 to 8 % of it over several draws (neither regime is asserted below), so the gate compares something."""


def _case(E, attn_type):
    return dict(TOKENIZER_CASES["hard_1l"], E=E, layers=2, attn_type=attn_type)   # the smallest configuration, two layers


def _module(c):
    from u2tokenizer_amd.tokenizer import u2Tokenizer
    with torch.device("meta"):
        m = u2Tokenizer(embed_size=c["E"], num_heads=c["heads"], num_layers=c["layers"], top_k=c["top_k"],
                        use_multi_scale=c["use_multi_scale"], num_3d_query_token=c["Q"], hidden_size=c["E"],
                        attn_type=c["attn_type"], enable_diffts=c["enable_diffts"], enable_dmtp=c["enable_dmtp"])
    return m


_WEIGHTS = {}


def _tensor(name, shape, seed):
    """Parameters by name (shared between the rma and the rope module, which differ only in the bias tables): the square
    projections -- 400 M values per module -- are drawn on the GPU with synth.synth_tensor's scale, everything else by
    synth.synth_tensor itself; then synth.lively_ at QK_GAIN."""
    key = (name, tuple(shape), seed)
    if key not in _WEIGHTS:
        if len(shape) == 2 and name.endswith(".weight") and shape[0] * shape[1] >= 1 << 20:
            g = torch.Generator(device=D).manual_seed(zlib.crc32(name.encode()) + seed)
            t = torch.randn(tuple(shape), generator=g, device=D) / math.sqrt(shape[1])
        else:
            t = synth.synth_tensor(name, shape, seed).to(D)
        _WEIGHTS[key] = synth.lively_(name, t, qk_gain=QK_GAIN)
    return _WEIGHTS[key]


def _load(c, dtype=torch.bfloat16):
    m = _module(c)
    sd = {k: _tensor("u2tokenizer." + k, v.shape, c["seed"]) for k, v in m.state_dict().items() if v.is_floating_point()}
    m = m.to(dtype).to_empty(device=D)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=False)
    return m, {"u2tokenizer." + k: v for k, v in sd.items()}


@pytest.fixture(scope="module")
def launches_at_2048(ops):
    """launch counts of the same configuration at E = 2048 (head dim 256), where every core is on the fused kernels"""
    out = {}
    for at in ("rma", "rope"):
        c = _case(2048, at)
        m, _ = _load(c)
        v, t = tokenizer_inputs(c)
        v, t = v.to(torch.bfloat16).to(D), t.to(torch.bfloat16).to(D)
        _, out[at] = _launches(ops, D, lambda: m(v_token=v, t_token=t))
    _WEIGHTS.clear()
    return out


@pytest.mark.parametrize("attn_type", ["rma", "rope"])
def test_tokenizer_forward_at_E3072_takes_the_fused_kernels(ops, launches_at_2048, attn_type):
    """Two tokenizer layers at E = 3072, heads 8, against the oracle in fp32 (gate of tests/test_gpu_configs.py); every
    attention core on the fused kernels -- as many launches in the fused-attention and chunk-axis classes as at E = 2048 --
    and the GEMM chain (option tok_flash = 0: none in the fused class) as the cross-check under the same gate."""
    c = _case(3072, attn_type)
    m, sd = _load(c)
    v, t = tokenizer_inputs(c)
    v16, t16 = v.to(torch.bfloat16), t.to(torch.bfloat16)
    sd32 = {k: x.cpu() for k, x in sd.items()}
    sd16 = {k: x.to(torch.bfloat16).cpu() for k, x in sd.items()}
    _WEIGHTS.clear()
    o32, i32 = O.tokenizer_forward(sd32, "u2tokenizer", v16.float(), t16.float(), tok_cfg(c))
    o16, i16 = O.tokenizer_forward(sd16, "u2tokenizer", v16, t16, tok_cfg(c))
    k_ = c["top_k"]
    overlap = lambda a, b: len(set(a[0].tolist()) & set(b[0].tolist())) / k_   # noqa: E731

    got, cnt = _launches(ops, D, lambda: m(v_token=v16.to(D), t_token=t16.to(D)))
    idx = m.last_topk_indices.cpu()
    want = launches_at_2048[attn_type]
    print(f"{attn_type}: launches per class at E = 3072 {cnt}, at E = 2048 {want}")
    assert cnt[PROF_TOKATTN] > 0 and cnt[PROF_TEMPORAL] > 0, cnt
    assert cnt[PROF_TOKATTN] == want[PROF_TOKATTN] and cnt[PROF_TEMPORAL] == want[PROF_TEMPORAL], (cnt, want)
    assert cnt == want, (cnt, want)           # ... and nothing else changed class either

    ops.set_option("tok_flash", 0)
    try:
        chain, cnt0 = _launches(ops, D, lambda: m(v_token=v16.to(D), t_token=t16.to(D)))
        idx0 = m.last_topk_indices.cpu()
    finally:
        ops.set_option("tok_flash", 1)
    assert cnt0[PROF_TOKATTN] == 0 and cnt0[PROF_TEMPORAL] == cnt[PROF_TEMPORAL], cnt0

    d, d0 = three_way(got, o32, o16), three_way(chain, o32, o16)
    print(f"{attn_type}: fused {d['hip_vs_o32']['rel_rms']:.3e} / chain {d0['hip_vs_o32']['rel_rms']:.3e} / bf16 oracle "
          f"{d['o16_vs_o32']['rel_rms']:.3e} relative RMS from fp32; diversity {d['diversity_o32']:.3f}; "
          f"fused vs chain {err_stats(got.float().cpu(), chain.float().cpu())['rel_rms']:.3e}")
    # neither collapsed (gain 1: diversity < 1e-2) nor chaotic (gain 3 and up: the bf16 reference > 60 % off)
    assert d["diversity_o32"] > 0.05 and d["o16_vs_o32"]["rel_rms"] < 0.3, d
    assert torch.isfinite(got.float()).all() and torch.isfinite(chain.float()).all()
    gate(d, f"E3072 {attn_type} fused")
    gate(d0, f"E3072 {attn_type} chain")
    # hard top-k: the same indices from both routes -- or, where rounding moved one, each route as close to the fp32
    # selection as the reference's own bf16 run is (one index of slack, as tests/test_gpu_configs.py)
    if not torch.equal(idx, idx0):
        n = int((idx != idx0).sum())
        print(f"{attn_type}: {n} of {k_} top-k indices differ between the fused and the chain route")
        for name, i in (("fused", idx), ("chain", idx0)):
            assert overlap(i, i32) >= overlap(i16, i32) - 1.0 / k_ - 1e-9, (name, n, i, i32, i16)
