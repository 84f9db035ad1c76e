"""GPU: the SVR folds (include/u2tok.h, "FOLD SLOTS") on the device -- the output projection of every SVR attention but the last
folded into the q | k | v projection behind it.

  * parity of the folded route: the folded HIP output is no further from the float64 oracle than 1.2 x what the oracle's own bf16 run
    is on the same inputs (gate() of tests/test_gpu_configs.py; the yardstick is the bf16 oracle, never the unfolded HIP route);
  * admission: a call that asks for SVR tensors, or option svr_fold = 0, launches and computes what it did before the folds; a plain
    forward makes exactly 2 L - 1 GEMM launches fewer and nothing else changes class;
  * staleness: a weight written in place is refolded; a checkpoint loaded into a packed model is refolded;
  * a weight table whose wq / wk / wv are separately allocated launches the unfolded sequence whatever its fold slots hold."""
import ctypes as C
import functools

import pytest
import torch

from helpers import err_stats, tok_cfg
from oracle import u2_oracle as O
from cases import tokenizer_inputs
from pipeline_cases import swapped_rows
from svr_fold_cases import DTYPES, case, make
from test_gpu_configs import gate, three_way

pytestmark = pytest.mark.gpu
D = "cuda"
NCAT, GEMM = 6, 0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from u2tokenizer_amd import ops
    ops.device_check()
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(False)
    yield ops
    torch.set_grad_enabled(prev)


@functools.lru_cache(maxsize=None)
def _model(attn, L, B, elem):
    c = case(attn, L, B)
    m, sd = make(c)
    return c, m.to(DTYPES[elem]).to(D), sd


def _inputs(c, elem):
    v, t = tokenizer_inputs(c)
    return v.to(DTYPES[elem]), t.to(DTYPES[elem])


@functools.lru_cache(maxsize=None)
def _oracles(attn, L, B, elem):
    """(float64 oracle on the weights and inputs the HIP route reads, the bf16 oracle's distance to ITS float64 oracle)"""
    c, _, sd = _model(attn, L, B, elem)
    v, t = _inputs(c, elem)
    cfg = tok_cfg(c)
    o64 = O.tokenizer_forward({k: x.to(DTYPES[elem]).double() for k, x in sd.items()}, "u2tokenizer", v.double(), t.double(), cfg)[0]
    vb, tb = _inputs(c, "bf16")
    sdb = {k: x.to(torch.bfloat16) for k, x in sd.items()}
    o16 = O.tokenizer_forward(sdb, "u2tokenizer", vb, tb, cfg)[0]
    o64b = o64 if elem == "bf16" else O.tokenizer_forward({k: x.double() for k, x in sdb.items()}, "u2tokenizer", vb.double(),
                                                          tb.double(), cfg)[0]
    return o64, o16, o64b


def _profiled(ops, elem, fn):
    """fn() under option "profile" -> (its result, launches per class)"""
    from u2tokenizer_amd import _lib
    ops.set_option("profile", 1)
    try:
        out = fn()
        torch.cuda.synchronize()
        h = _lib.load_library(elem)
        prev = h.u2tok_ctx_get_current()
        h.u2tok_ctx_set_current(ops.active_context(torch.device(D, torch.cuda.current_device())).handle_for(elem))
        ms, fl, by, cnt = (C.c_double * NCAT)(), (C.c_double * NCAT)(), (C.c_double * NCAT)(), (C.c_int64 * NCAT)()
        try:
            _lib.check(h.u2tok_profile_collect2(ms, fl, by, cnt, NCAT), "u2tok_profile_collect2")
        finally:
            h.u2tok_ctx_set_current(prev)
    finally:
        ops.set_option("profile", 0)
    return out, list(cnt)


PARITY = [("rma", 1, 1), ("rma", 2, 1), ("rma", 3, 1), ("rope", 2, 1), ("mha", 2, 1), ("mha", 2, 2)]


@pytest.mark.parametrize("elem", list(DTYPES))
@pytest.mark.parametrize("attn,L,B", PARITY)
def test_folded_route_parity(ops, attn, L, B, elem):
    """L = 1 has only the fold inside the layer, L = 2 adds the first one across layers; mha at B = 2 attends across the batch
    entries (the gather / scatter path of the temporal attention)."""
    c, m, _ = _model(attn, L, B, elem)
    v, t = _inputs(c, elem)
    o64, o16, o64b = _oracles(attn, L, B, elem)
    m.capture_svr_tokens = False
    assert all(s is not None for s in m._fold_slots()) and len(m._fold_slots()) == 2 * (2 * L - 1)
    got = m(v_token=v.to(D), t_token=t.to(D))
    d = three_way(got, o64, o16)
    d["o16_vs_o32"] = err_stats(o16.float(), o64b)           # the yardstick: the bf16 oracle against the float64 oracle of ITS inputs
    print(f"{elem} {attn} L={L} B={B}: folded HIP {d['hip_vs_o32']['rel_rms']:.3e}, bf16 oracle {d['o16_vs_o32']['rel_rms']:.3e} "
          f"relative RMS from float64 (ratio {d['hip_vs_o32']['rel_rms'] / d['o16_vs_o32']['rel_rms']:.2f}); diversity {d['diversity_o32']:.3f}")
    assert torch.isfinite(got.float()).all()
    if elem == "f16":   # gate()'s last clause, "as close to the 16-bit reference as that is to the exact one": the oracle run in fp16
        sdh = {k: x.to(torch.float16) for k, x in _model(attn, L, B, elem)[2].items()}
        d["hip_vs_o16"] = err_stats(got.float().cpu(), O.tokenizer_forward(sdh, "u2tokenizer", v, t, tok_cfg(c))[0].float())
    gate(d, f"{elem} {attn} L={L} B={B} folded")
    # exchanging two rows of v_token that differ in chunk and token position must move the output
    (b0, t0, n0), (b1, t1, n1) = swapped_rows(c)
    v2 = v.clone()
    v2[b0, t0, n0], v2[b1, t1, n1] = v[b1, t1, n1], v[b0, t0, n0]
    assert not torch.equal(m(v_token=v2.to(D), t_token=t.to(D)), got)


@pytest.mark.parametrize("elem", list(DTYPES))
@pytest.mark.parametrize("attn", ["rma", "mha"])
def test_fold_slots_against_float64(ops, attn, elem):
    """What u2tok_tokenizer_svr_fold left in every slot, element by element against W_qkv W_o and W_qkv b_o + b_qkv in float64 of the
    weights the device holds.  (The lively stacks above are chaotic from two layers on -- the bf16 oracle itself is ~80 % away from
    float64 there -- so this is what pins the pairing and the operand order at depth.)  Bound: one rounding to the element type,
    u |x| with u = 2^-8 (bf16) / 2^-11 (fp16), or half the smallest fp16 subnormal step, plus twice the fp32 accumulation bound
    (K + 1) 2^-24 sum |a| |b| (which may also carry x across a rounding boundary)."""
    from svr_fold_cases import _attention_names, _qkv_o
    L = 2
    c, m, sd = _model(attn, L, 1, elem)
    m(v_token=_inputs(c, elem)[0].to(D), t_token=_inputs(c, elem)[1].to(D))      # (folds current)
    sd64 = {k: x.to(DTYPES[elem]).double() for k, x in sd.items()}
    names, slots = _attention_names(L), m._fold_slots()
    u, floor, K = (2.0 ** -8, 0.0, c["E"]) if elem == "bf16" else (2.0 ** -11, 2.0 ** -25, c["E"])
    for j in range(1, len(names)):
        w_qkv, b_qkv = _qkv_o(sd64, names[j])[:2]
        w_o, b_o = _qkv_o(sd64, names[j - 1])[2:]
        for got, want, mag in ((slots[2 * (j - 1)], w_qkv @ w_o, w_qkv.abs() @ w_o.abs()),
                               (slots[2 * (j - 1) + 1], w_qkv @ b_o + b_qkv, w_qkv.abs() @ b_o.abs() + b_qkv.abs())):
            err = (got.double().cpu() - want).abs()
            bound = u * want.abs() + floor + 2 * (K + 1) * 2.0 ** -24 * mag
            assert got.shape == want.shape and bool((err <= bound).all()), (attn, elem, j, (err / bound).max().item())


@pytest.mark.parametrize("elem", list(DTYPES))
@pytest.mark.parametrize("attn,L,B", [("rma", 1, 1), ("rma", 3, 1), ("mha", 2, 2)])
def test_admission(ops, attn, L, B, elem):
    c, m, _ = _model(attn, L, B, elem)
    v, t = (x.to(D) for x in _inputs(c, elem))
    m.capture_svr_tokens = False
    m(v_token=v, t_token=t)                                   # (the folds are built: nothing but the forward under the profile)
    run = lambda: m(v_token=v, t_token=t).clone()             # noqa: E731
    try:
        folded, n_fold = _profiled(ops, elem, run)
        ops.set_option("svr_fold", 0)
        plain, n_plain = _profiled(ops, elem, run)
        ops.set_option("svr_fold", 1)
        m.capture_svr_tokens = True
        cap, n_cap = _profiled(ops, elem, run)
        ops.set_option("svr_fold", 0)
        cap0, n_cap0 = _profiled(ops, elem, run)
    finally:
        ops.set_option("svr_fold", 1)
        m.capture_svr_tokens = False
    print(f"{elem} {attn} L={L} B={B}: launches per class folded {n_fold}, svr_fold=0 {n_plain}, capturing {n_cap}")
    assert n_cap == n_plain == n_cap0                         # a call that asks for SVR tensors launches what it always did
    assert torch.equal(cap, plain) and torch.equal(cap, cap0)  # ... and computes the same bits
    assert n_fold[GEMM] == n_plain[GEMM] - (2 * L - 1), (n_fold, n_plain)
    assert n_fold[1:] == n_plain[1:], (n_fold, n_plain)       # nothing else changed class
    assert not torch.equal(folded, plain)                     # (the folded route rounds elsewhere: it did run)
    # forward_with_taps copies every SVR layer's output out: unfolded, with the fold slots in its table
    out, taps = m.forward_with_taps(v, t)
    assert torch.equal(out, plain) and len(taps["svr_out"]) == L


@pytest.mark.parametrize("elem", list(DTYPES))
def test_weight_written_in_place_is_refolded(ops, elem):
    c, m, sd = _model("rma", 2, 1, elem)
    v, t = (x.to(D) for x in _inputs(c, elem))
    m.capture_svr_tokens = False
    before = m(v_token=v, t_token=t).clone()
    name = "svt_module.attention_network.layers.0.spatial_attention.dense.weight"
    new = (sd["u2tokenizer." + name].flip(0) * 0.5).to(DTYPES[elem])
    old = m.get_parameter(name).detach().clone()
    try:
        m.get_parameter(name).copy_(new.to(D))
        after = m(v_token=v, t_token=t).clone()
        fresh, _ = make(c)
        fresh.load_state_dict({k[len("u2tokenizer."):]: x for k, x in dict(sd, **{"u2tokenizer." + name: new.float()}).items()})
        fresh = fresh.to(DTYPES[elem]).to(D)
        want = fresh(v_token=v, t_token=t)
        assert not torch.equal(after, before)
        assert torch.equal(after, want)
    finally:
        m.get_parameter(name).copy_(old)                      # (the cached model goes back to its weights, and refolds)
    assert torch.equal(m(v_token=v, t_token=t), before)


def test_training_forward_drops_the_folds(ops):
    """An optimiser that writes through param.data (dp.Zero1AdamW, DeepSpeed) advances no version counter: the forward on the
    autograd route drops the folds, and the next inference forward builds them from the weights it finds."""
    c = case("rma", 2)
    v, t = (x.to(D) for x in _inputs(c, "bf16"))
    name = "svt_module.attention_network.layers.1.spatial_attention.dense.weight"
    m, _ = make(c)
    m = m.to(torch.bfloat16).to(D)
    before = m(v_token=v, t_token=t).clone()
    assert m._folds is not None
    with torch.enable_grad():
        m(v_token=v, t_token=t)
    assert m._folds is None and m._fold_slots() == [None] * 6
    m.get_parameter(name).data.mul_(0.5)
    after = m(v_token=v, t_token=t)
    assert m._folds is not None
    fresh, _ = make(c)
    fresh.get_parameter(name).data.mul_(0.5)                   # (a power of two: the same bf16 values)
    fresh = fresh.to(torch.bfloat16).to(D)
    assert torch.equal(after, fresh(v_token=v, t_token=t)) and not torch.equal(after, before)


def test_checkpoint_loaded_into_a_packed_model_is_refolded(ops, tmp_path):
    from u2tokenizer_amd import checkpoint as CK
    c = case("rma", 2)
    v, t = (x.to(D) for x in _inputs(c, "bf16"))
    src, _ = make(dict(c, seed=c["seed"] + 100))
    src = src.to(torch.bfloat16).to(D)
    want = src(v_token=v, t_token=t).clone()
    keys = list(src.state_dict())
    path = CK.save_checkpoint(src, str(tmp_path / "ck"), safe_serialization=False)
    m, _ = make(c)
    m = m.to(torch.bfloat16).to(D)
    assert not torch.equal(m(v_token=v, t_token=t), want)      # other weights, folded
    CK.load_checkpoint(m, path, strict=True)
    assert list(m.state_dict()) == keys
    assert torch.equal(m(v_token=v, t_token=t), want)


@pytest.mark.parametrize("elem", list(DTYPES))
def test_unpacked_table_is_not_folded(ops, elem):
    """u2tok_tokenizer_forward on a weight table of separately allocated tensors (no wk starts where its wq ends), no svr_out: the
    three-launch q | k | v and two-launch k | v projections run, every output projection runs -- with null fold slots, and just the
    same with the packed model's folds in the slots (a fold needs its attention's q | k | v packed)."""
    from u2tokenizer_amd import _lib
    L = 2
    c, m, _ = _model("rma", L, 1, elem)
    dt = DTYPES[elem]
    v, t = (x.to(D) for x in _inputs(c, elem))
    m.capture_svr_tokens = False
    try:
        ops.set_option("svr_fold", 0)
        _, n_packed = _profiled(ops, elem, lambda: m(v_token=v, t_token=t))
    finally:
        ops.set_option("svr_fold", 1)
    B, T, N, E = v.shape
    bufs = []

    def own(p):
        if p is None:
            return None
        bufs.append(torch.empty(p.numel() + 64, dtype=dt, device=D))
        return bufs[-1][:p.numel()].view(p.shape).copy_(p.detach())

    weights = [own(p) for p in m._weights()]

    def direct(slots):
        with ops.on_device(v, elem=dt) as (h, stream):
            table = ops.weight_table(weights + slots)
            cfg = m._config(B, T, N, E, t.shape[1])
            nbytes = h.u2tok_tokenizer_workspace_bytes(C.byref(cfg))
            assert nbytes
            ws = torch.empty(nbytes, dtype=torch.uint8, device=D)
            out = torch.empty((B, c["Q"], E), dtype=dt, device=D)
            _lib.check(h.u2tok_tokenizer_forward(C.byref(cfg), table, v.data_ptr(), t.data_ptr(), out.data_ptr(), None, None,
                                                 ws.data_ptr(), ws.numel(), stream), "u2tok_tokenizer_forward")
            torch.cuda.synchronize()
        return out

    null, n_null = _profiled(ops, elem, lambda: direct([None] * (2 * (2 * L - 1))))
    full, n_full = _profiled(ops, elem, lambda: direct(m._fold_slots()))
    # per layer: 2 SVR attentions + the TTA self attention take 3 launches for their q | k | v instead of 1, the 2 cross attentions 2
    # for their k | v instead of 1
    assert n_null[GEMM] == n_packed[GEMM] + L * (3 * 2 + 2 * 1), (n_null, n_packed)
    assert n_null[1:] == n_packed[1:] and n_full == n_null
    assert torch.equal(full, null)
