"""GPU: the encoder attention forwards -- tok_attn_kernel<64 .. 512>, tok_attn2_kernel<256 | 512, MUBUF>, the bias window, the
key-split merges (u2tok_tok_attention), flash_d64_kernel and flash_dp2_kernel<0 | 1> (u2tok_flash_attention_d64 / _lse) and
temporal_attention_kernel (u2tok_temporal_attention) -- on the sweeps of tests/enc_attn_cases.py, element by element against the
float64 bound derived there (tests/test_enc_attn_bounds_host.py shows that the kernels' rounding model keeps it and that each mutant
breaks it more than 10-fold), on the bf16 and the f16 build.  The float64 reference is computed on the device.

Every call goes through the C entry: q | k | v are column views of packed buffers, the output is a view with gaps between rows and
batch entries of NaN-filled storage, the bias table sits between NaN guard rows and the split workspace is NaN-filled with a guard
tail.  Every call runs twice with equal bits; pads and guards must still be NaN and the inputs unchanged afterwards; no element is
left out.  The split count of a case is computed from the launcher's rule and asserted on the workspace (exactly ns splits' partial
results written).  Worst error / bound measured on the MI355X: DESIGN.md, "Encoder attention: length sweeps and bias edges"."""
import pytest
import torch

import attn_edge_cases as E
import enc_attn_cases as C

pytestmark = pytest.mark.gpu
D = "cuda"
ELEMS = [pytest.param(name, id=name) for name in C.ELEM]
NAN16 = {"bf16": 0x7FC1, "f16": 0x7E01}      # quiet NaNs with a payload no arithmetic produces
NAN32 = 0x7FC00001
GUARD = 8                                    # NaN rows in front of and behind the bias table
WS_GUARD = 64                                # fp32 words behind the workspace
ERR_ARG = -1


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    torch.set_grad_enabled(False)
    return _ops


def nan16(n, elem):
    return torch.full((n,), NAN16[elem], dtype=torch.int16, device=D).view(C.ELEM[elem][0])


def nan32(n):
    return torch.full((n,), NAN32, dtype=torch.int32, device=D).view(torch.float32)


def all_nan16(t, elem):
    return bool((t.view(torch.int16) == NAN16[elem]).all())


def all_nan32(t):
    return bool((t.view(torch.int32) == NAN32).all())


def entry(ops, anchor, name, *args):
    """u2tok_<name>(*args, stream) of the build of anchor's element type -> status, after the stream has drained"""
    with ops.on_device(anchor) as (h, st):
        got = getattr(h, name)(*args, st)
    torch.cuda.synchronize()
    return got


def padded_out(nb, S, Ew, pad, elem, off=0):
    """(storage, view (nb, S, Ew)): rows at stride Ew + pad, batch entries one spare row apart, `off` elements in front"""
    ld = Ew + pad
    st = nan16(off + nb * (S + 1) * ld, elem)
    return st, st[off:].view(nb, S + 1, ld)[:, :S, :Ew]


def pads_intact(st, view, elem):
    """everything of the storage outside the view is still NaN"""
    keep = st.clone()
    view_of_keep = keep[view.storage_offset():].view(view.shape[0], -1, view.stride(1))[:, :view.shape[1], :view.shape[2]]
    view_of_keep.view(torch.int16).fill_(NAN16[elem])
    return all_nan16(keep, elem)


def rows_of(t):
    """(nb, H, S, d) -> (nb, S, H d)"""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)


class Worst:
    def __init__(self):
        self.r, self.id, self.bad, self.n = 0.0, None, [], 0

    def hold(self, got, want, bound, cid):
        got = got.double()
        assert torch.isfinite(got).all(), cid
        r = E.ratio((got - want).abs(), bound)
        self.n += 1
        if r > self.r:
            self.r, self.id = r, cid
        if not r <= 1.0:
            self.bad.append((cid, r))

    def done(self, label):
        print(f"kernel error / bound, {label}: {self.r:.3f} over {self.n} calls ({self.id})")
        assert self.n and not self.bad, f"{len(self.bad)} of {self.n} calls outside the bound: {self.bad[:8]}"


# ------------------------------------------------------------------------------------------------------------ tok_attention
def tok_forms(d):
    return (0, 1, 2) if d in (256, 512) else (0,)


def _tok_buffers(c, o, elem):
    Ew = c.H * c.d
    qs = nan16(c.nb * c.Sq * (Ew + 8), elem).view(c.nb, c.Sq, Ew + 8)
    qs[..., :Ew] = rows_of(o["q"].to(D))
    kv = torch.cat([rows_of(o["k"].to(D)), rows_of(o["v"].to(D))], -1)
    tb = None
    if o["table"] is not None:
        tb = nan16((2 * c.max_len - 1 + 2 * GUARD) * c.H, elem).view(-1, c.H)
        tb[GUARD:GUARD + 2 * c.max_len - 1] = o["table"].to(D)
    return qs, kv, tb


def _tok_call(ops, c, o, elem, bufs, status=0):
    """one u2tok_tok_attention call on fresh NaN-filled output and workspace -> (output view, ns the workspace shows)"""
    qs, kv, tb = bufs
    Ew = c.H * c.d
    with ops.on_device(qs) as (h, _):
        ask = h.u2tok_tok_attention_workspace_bytes(c.nb, c.H, c.Sq, c.Skv, c.d)
    per = c.nb * c.Sq * (Ew * 4 + c.H * 8)                    # bytes of one split's partial results
    nbytes = max(ask, c.splits * per if c.splits > 1 else 0)
    ws = nan32(nbytes // 4 + WS_GUARD)
    ost, out = padded_out(c.nb, c.Sq, Ew, 8, elem)
    q, k, v = qs[..., :Ew], kv[..., :Ew], kv[..., Ew:]
    got = entry(ops, qs, "u2tok_tok_attention", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), c.nb, c.Sq, c.Skv, c.H, c.d,
                q.stride(1), k.stride(1), v.stride(1), out.stride(1), q.stride(0), k.stride(0), v.stride(0), out.stride(0),
                float(o["scale"]), None if tb is None else tb[GUARD:].data_ptr(), c.max_len or 0, c.splits,
                ws.data_ptr() if nbytes else None, nbytes)
    assert got == status, (C.case_id(c), got)
    assert pads_intact(ost, out, elem), C.case_id(c)
    if status:
        assert all_nan16(ost, elem) and all_nan32(ws), C.case_id(c)
        return None, 0
    # the first ns * per bytes hold the splits' partial outputs and (max, sum) pairs, nothing else is touched
    written = (ws.view(torch.int32) != NAN32)
    nw = int(written.sum())
    assert nw % (per // 4) == 0 and bool(written[:nw].all()), (C.case_id(c), nw, per)
    return out, nw // (per // 4)


def _tok_sweep(ops, elem, cases, label):
    assert cases
    worst = {f: Worst() for f in (0, 1, 2)}
    try:
        for c in cases:
            cid = C.case_id(c)
            o = C.operands(c, elem)
            bufs = _tok_buffers(c, o, elem)
            before = [b.clone() for b in bufs if b is not None]
            ns, _ = C.split_shape(c)
            m = C.reference(c, o, elem, D)
            want, bound = rows_of(m["out"]), rows_of(m["bound"])
            outs = {}
            for form in tok_forms(c.d):
                ops.set_option("tok_wide", form)
                out, got_ns = _tok_call(ops, c, o, elem, bufs)
                again, _ = _tok_call(ops, c, o, elem, bufs)
                assert got_ns == (ns if ns > 1 else 0), (cid, form, got_ns, ns)
                assert torch.equal(out.view(torch.int16), again.view(torch.int16)), (cid, form)
                worst[form].hold(out, want, bound, cid)
                outs[form] = out
            if 2 in outs:    # the FLAT-encoded and the buffer-addressed DMA of the 8-wave form move the same bytes
                assert torch.equal(outs[1].view(torch.int16), outs[2].view(torch.int16)), cid
            assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(before, [b for b in bufs if b is not None])), cid
    finally:
        ops.set_option("tok_wide", 2)
    for form in (0, 1, 2):
        if worst[form].n:
            worst[form].done(f"{label} tok_wide = {form} {elem}")
    assert worst[0].n == len(cases)


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("d", C.WIDE + C.NARROW)
def test_g_every_key_length(ops, elem, d):
    _tok_sweep(ops, elem, [c for c in C.cases("G") if c.d == d], f"G key length (d = {d})")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("table", ("exact", 512))
@pytest.mark.parametrize("d", C.WIDE + C.NARROW)
def test_h_every_query_length(ops, elem, d, table):
    _tok_sweep(ops, elem, [c for c in C.cases("H") if c.d == d and (c.max_len == 512) == (table == 512)], f"H query length (d = {d}, max_len {table})")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("Sq", (16, 70))
@pytest.mark.parametrize("d", (64, 256, 512))
def test_i_key_splits(ops, elem, d, Sq, bias):
    cases = [c for c in C.cases("I") if c.d == d and c.Sq == Sq and bool(c.max_len) == bias]
    assert {C.split_shape(c)[0] for c in cases} == set(range(1, 11 if d >= 256 else 7))      # (every merge kernel; asserted per call below)
    _tok_sweep(ops, elem, cases, f"I splits (d = {d}, Sq = {Sq}, {'bias' if bias else 'no bias'})")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("part", ("window-64", "window-256", "window-512", "unequal"))
def test_k_bias_table_and_window_edges(ops, elem, part):
    cases = [c for c in C.cases("K") if (c.Skv == 576 and part == f"window-{c.d}") or (c.Skv != 576 and part == "unequal")]
    _tok_sweep(ops, elem, cases, f"K bias edges ({part})")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("d", (64, 128, 256, 384, 512))
def test_k_one_key_past_the_bias_window_is_refused(ops, elem, d):
    """Skv = 577 needs 703 slots: the argument error, and neither the output nor the workspace is written"""
    try:
        for form in tok_forms(d):
            ops.set_option("tok_wide", form)
            for splits in (1, 0, 3):
                c = C.case("K", "tok", 2, 16, 577, 2, d, max_len=577, splits=splits)
                o = C.operands(c, elem)
                _tok_call(ops, c, o, elem, _tok_buffers(c, o, elem), status=ERR_ARG)
    finally:
        ops.set_option("tok_wide", 2)


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("data", ("rise", "first", "steps", "equal", "edge"))
def test_j_hard_softmax_data_wide_forms(ops, elem, data):
    _tok_sweep(ops, elem, [c for c in C.cases("J") if c.kern == "tok" and c.data == data and c.d != 384], f"J {data} (d = 256, 512)")
    _tok_sweep(ops, elem, [c for c in C.cases("J") if c.kern == "tok" and c.data == data and c.d == 384], f"J {data} (d = 384)")


# ------------------------------------------------------------------------------------------------------ flash_attention_d64
MODES = {"mode1": (1, 0), "mode7": (7, 0), "mode7-prescaled": (7, 1)}


def _flash_call(ops, c, qkv, elem, lse, narrow=False):
    """u2tok_flash_attention_d64[_lse] as ops.flash_attention_d64 calls it, into a padded NaN-filled output -> (storage, view, lse)"""
    nb, S, Hd = c.nb, c.Skv, c.H * 64
    Sm, es = C.n_main(c), 2
    S_pad = (Sm + 63) // 64 * 64
    vt = nan16(nb * Hd * S_pad, elem).view(nb, Hd, S_pad)
    assert entry(ops, qkv, "u2tok_transpose_bf16", qkv[:, :, 2 * Hd:].data_ptr(), vt.data_ptr(), nb, Sm, Hd, 3 * Hd, S_pad, S * 3 * Hd,
                 Hd * S_pad, 1) == 0
    ost, out = padded_out(nb, S, Hd, 4 if narrow else 8, elem, off=4 if narrow else 0)   # narrow: rows at 8-byte, not 16-byte, alignment
    x0 = qkv.data_ptr() + (S - 1) * 3 * Hd * es
    x = c.extra
    args = (qkv.data_ptr(), qkv.data_ptr() + Hd * es, vt.data_ptr(), out.data_ptr(), nb, Sm, c.H, 3 * Hd, S * 3 * Hd, out.stride(1),
            out.stride(0), S_pad, 0.125, x0 if x else None, x0 + Hd * es if x else None, x0 + 2 * Hd * es if x else None,
            out.data_ptr() + (S - 1) * out.stride(1) * es if x else None, S * 3 * Hd, out.stride(0), 1 if x else 0)
    stats = None
    if lse:
        lse_ld = (S + 63) // 64 * 64
        stats = nan32(nb * c.H * lse_ld).view(nb * c.H, lse_ld)
        assert entry(ops, qkv, "u2tok_flash_attention_d64_lse", *args, stats.data_ptr(), lse_ld) == 0
        assert all_nan32(stats[:, S:]), C.case_id(c)
    else:
        assert entry(ops, qkv, "u2tok_flash_attention_d64", *args) == 0
    assert pads_intact(ost, out, elem), C.case_id(c)
    return out, stats


def _flash_sweep(ops, elem, cases, mode, label, narrow=False):
    """each case: once through the _lse entry and once through the plain one with equal bits; out under the bound, every row's lse
    within 1e-5 max(1, |lse|) in natural-log units (the extra row's included)"""
    assert cases
    flash_mode, pre = MODES[mode]
    w, worst_lse = Worst(), 0.0
    try:
        ops.set_option("flash_mode", flash_mode)
        ops.set_option("flash_q_prescaled", pre)
        for c in cases:
            cid = C.case_id(c)
            o = C.operands(c, elem)
            if pre:
                o = C.prescaled(o, elem)
            qkv = torch.cat([rows_of(o[n].to(D)) for n in "qkv"], -1).contiguous()
            before = qkv.clone()
            out, lse = _flash_call(ops, c, qkv, elem, True, narrow)
            again, _ = _flash_call(ops, c, qkv, elem, False, narrow)
            assert torch.equal(out.view(torch.int16), again.view(torch.int16)), cid
            assert torch.equal(qkv.view(torch.int16), before.view(torch.int16)), cid
            m = C.reference(c, o, elem, D)
            w.hold(out, rows_of(m["out"]), rows_of(m["bound"]), cid)
            want = m["lse"].reshape(c.nb * c.H, c.Skv)
            r = ((lse[:, :c.Skv].double() * C.LN2 - want).abs() / (1e-5 * want.abs().clamp_min(1.0))).max().item()
            worst_lse = max(worst_lse, r)
            assert r <= 1.0, (cid, "lse", r)
    finally:
        ops.set_option("flash_mode", 0)
        ops.set_option("flash_q_prescaled", 0)
    print(f"lse error / (1e-5 max(1, |lse|)), {label} {mode} {elem}: {worst_lse:.3f}")
    w.done(f"{label} {mode} {elem}")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("extra", (False, True), ids=("plain", "extra"))
@pytest.mark.parametrize("lo,hi", [(1, 165), (166, 330), (511, 2049)])
@pytest.mark.parametrize("mode", list(MODES))
def test_l_vit_flash_at_every_length(ops, elem, mode, lo, hi, extra):
    cases = [c for c in C.cases("L") if c.extra == extra and lo <= C.n_main(c) <= hi]
    _flash_sweep(ops, elem, cases, mode, f"L flash S = {lo} .. {hi}{' + extra row' if extra else ''}")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("mode", list(MODES))
def test_l_flash_narrow_stores_under_the_bound(ops, elem, mode):
    """an output view at an 8-byte offset with 8-byte aligned rows takes the 8-byte store form"""
    _flash_sweep(ops, elem, [c for c in C.cases("L") if C.n_main(c) in (70, 330, 640 - 63) and not c.extra] +
                 [c for c in C.cases("L") if C.n_main(c) in (129, 513) and c.extra], mode, "L flash, 8-byte stores", narrow=True)


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("data,mode", [(da, mo) for da in ("rise", "first", "steps", "equal", "edge") for mo in MODES
                                       if (da, mo) != ("steps", "mode7-prescaled")])   # (pre-scaling rounds q once more: no exact steps)
def test_j_hard_softmax_data_flash(ops, elem, data, mode):
    """steps straddle FLASH_RESCALE_THR = 8 in mode 1 and, in mode 7, the row-sum piece's 2^64 (half: 2^15) for 16 equal keys"""
    cases = [c for c in C.cases("J") if c.kern == "flash" and c.data == data and (data == "edge" or isinstance(c.thr, tuple) == (mode != "mode1"))]
    _flash_sweep(ops, elem, cases, mode, f"J {data}")


# ------------------------------------------------------------------------------------------------------- temporal_attention
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("d", (64, 128, 256, 384, 512))
def test_t_temporal_attention_at_every_length(ops, elem, d):
    """q | k | v as column views at ld = 3 E + 8, the output at ld = E + 8; P stays in fp32: the bound's P weight is 0"""
    w = Worst()
    for c in [c for c in C.cases("T") if c.d == d]:
        cid = C.case_id(c)
        o = C.operands(c, elem)
        Ew, R = c.H * c.d, c.nb * c.Sq * c.N
        buf = nan16(R * (3 * Ew + 8), elem).view(R, 3 * Ew + 8)
        for n, name in enumerate("qkv"):
            buf[:, n * Ew:(n + 1) * Ew] = C.temporal_rows(o[name].to(D), c)
        before = buf.clone()
        tb = None
        if o["table"] is not None:
            tb = nan16((2 * c.max_len - 1 + 2 * GUARD) * c.H, elem).view(-1, c.H)
            tb[GUARD:GUARD + 2 * c.max_len - 1] = o["table"].to(D)
        outs = []
        for _ in range(2):
            ost = nan16(R * (Ew + 8), elem)
            out = ost.view(R, Ew + 8)[:, :Ew]
            got = entry(ops, buf, "u2tok_temporal_attention", buf.data_ptr(), buf[:, Ew:].data_ptr(), buf[:, 2 * Ew:].data_ptr(),
                        out.data_ptr(), c.nb, c.Sq, c.N, c.H, c.d, buf.stride(0), out.stride(0), float(o["scale"]),
                        None if tb is None else tb[GUARD:].data_ptr(), c.max_len or 512)
            assert got == 0, cid
            assert all_nan16(ost.view(R, Ew + 8)[:, Ew:], elem), cid
            outs.append(out)
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), cid
        assert torch.equal(buf.view(torch.int16), before.view(torch.int16)), cid
        m = C.reference(c, o, elem, D)
        w.hold(C.temporal_heads(outs[0], c), m["out"], m["bound"], cid)
    w.done(f"T temporal (d = {d}) {elem}")
