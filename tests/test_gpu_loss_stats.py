"""GPU: the loss head's statistics -- u2tok_ce_stats_update alone (the (m, l, zt) bits of u2tok_ce_lse_update whatever else is asked
for; the first index of the maximum through every level of its reduction; exact and float64-bounded sums; log sum exp(2 z)),
loss_head.token_stats against token_logprobs, the recomputed products and float64, and whole small causal LMs: the SFT evaluation's
token accuracy from `u2_fused_loss_head_predictions` and a DPO step's outputs from `model.token_stats`, each against the stock
model's full logits."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import decisive_decoder_
from u2tokenizer_amd import language_model as LM, loss_head, synth

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"
INF = float("inf")
INT64_MAX = (1 << 63) - 1
PAD = 3e38          # what the 8 columns past every slice hold: a read beyond Vs wins the maximum and wrecks the sum
FLAGS = list(itertools.product((False, True), repeat=3))       # (argmax, zsum, l2)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    return _ops


def chain(Vs):
    """Longest chain of dependent fp32 additions of zsum within one slice, as csrc/loss.hip states it above the kernel."""
    return -(-Vs // 2048) + 11


# slicings of V into widths that are multiples of 8 and unequal (V = 8 is one chunk: it cannot be split)
PLANS = {8: {1: (8,)},
         264: {1: (264,), 2: (200, 64), 5: (8, 120, 64, 16, 56)},
         2056: {1: (2056,), 2: (1792, 264), 5: (8, 264, 1512, 8, 264)}}


def _plan(widths):
    out, v0 = [], 0
    for w in widths:
        out.append((v0, w))
        v0 += w
    return out


def _padded(z, v0, vs):
    """The slice's columns in a buffer with leading dimension vs + 8, the padding holding PAD."""
    buf = torch.full((z.shape[0], vs + 8), PAD, dtype=bf, device=D)
    buf[:, :vs] = z[:, v0:v0 + vs]
    return buf[:, :vs]


def _run(ops, z, labels, plan, flags=None, base=0):
    """Feeds the slices of `plan` in the order given.  flags None: ops.ce_lse_update; else ops.ce_stats_update with (argmax, zsum, l2).
    -> dict of the state tensors."""
    rows = z.shape[0]
    st = {"m": torch.full((rows,), -INF, device=D), "l": torch.zeros(rows, device=D), "zt": torch.full((rows,), 777.0, device=D)}
    if flags is not None:
        if flags[0]:
            st["amax"], st["aidx"] = torch.full((rows,), -INF, device=D), torch.full((rows,), INT64_MAX, dtype=torch.int64, device=D)
        if flags[1]:
            st["zsum"] = torch.zeros(rows, device=D)
        if flags[2]:
            st["l2"] = torch.zeros(rows, device=D)
    for v0, vs in plan:
        blk = _padded(z, v0, vs)
        assert blk.stride(0) == vs + 8
        if flags is None:
            ops.ce_lse_update(blk, base + v0, labels, st["m"], st["l"], st["zt"])
        else:
            ops.ce_stats_update(blk, base + v0, labels, **st)
    return st


def _first_max(z):
    """(max, first column that holds it) per row, from the values themselves on the CPU."""
    zc = z.detach().cpu().float()
    mx = zc.max(-1).values
    cols = torch.arange(zc.shape[1]).expand_as(zc)
    return mx, torch.where(zc == mx[:, None], cols, torch.full_like(cols, zc.shape[1])).min(-1).values


def _quantised(rows, V, seed):
    """Multiples of 0.25 in [-4, 4]: every partial sum of a row is exact in fp32, and the maximum is held by many columns."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-16, 17, (rows, V), generator=g).float() * 0.25).to(bf).to(D)


def _gaussian(rows, V, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((rows, V), generator=g) * 6.5).clamp_(-30, 30).to(bf).to(D)


def _labels(rows, V, seed):
    lab = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(seed))
    lab[0], lab[-1] = V - 1, 0
    return lab.to(D)


def _check_stats(z, labels, st, flags, plan, name):
    """Every statistic of `st` against the CPU / float64 values of the same bf16 logits; prints each figure before it asserts."""
    zd = z.double()
    if flags[0]:
        mx, first = _first_max(z)
        assert torch.equal(st["aidx"].cpu(), first), (name, st["aidx"].tolist(), first.tolist())
        assert torch.equal(st["amax"].cpu(), mx), name
    if flags[1]:
        ref = zd.sum(-1)
        L = max(chain(vs) for _, vs in plan) + len(plan)
        assert L <= 160
        bound = L * 2.0 ** -24 * zd.abs().sum(-1)
        err = (st["zsum"].double() - ref).abs()
        print(f"  {name} zsum: max err {err.max().item():.3g}, bound {bound.min().item():.3g} (L = {L})")
        assert (err <= bound).all(), (name, err.max().item())
    if flags[2]:
        ref = torch.logsumexp(2 * zd, -1)
        got = 2.0 * st["m"].double() + torch.log(st["l2"].double())
        bound = 2e-5 * ref.abs().clamp_min(1.0)
        err = (got - ref).abs()
        print(f"  {name} lse2: max err {err.max().item():.3g}, bound {bound.min().item():.3g}")
        assert (err <= bound).all(), (name, err.max().item())


# ------------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("V", [8, 264, 2056])
def test_ce_stats_update_every_flavour(ops, rows, V):
    """For 1, 2 and 5 slices and all eight combinations of the optional statistics: (m, l, zt) bit-equal to ce_lse_update, lse
    within the project's bound of float64, the statistics right (argmax and amax exact; zsum EXACT on the quantised data, within
    L 2^-24 sum|z| on the gaussian; lse2 within 2e-5 max(1, |ref|)), a repeat bit-equal, and lse2 / zsum moved by the slice count
    by no more than their bounds."""
    for kind, z in (("quantised", _quantised(rows, V, 5)), ("gaussian", _gaussian(rows, V, 6))):
        labels = _labels(rows, V, 7)
        zd = z.double()
        lse_ref = torch.logsumexp(zd, -1)
        by_n = {}
        for n, widths in PLANS[V].items():
            plan = _plan(widths)
            base = _run(ops, z, labels, plan)
            lse = base["m"].double() + torch.log(base["l"].double())
            assert ((lse - lse_ref).abs() <= 1e-5 * lse_ref.abs().clamp_min(1.0)).all(), (kind, n)
            assert torch.equal(base["zt"], z.gather(1, labels[:, None])[:, 0].float())
            for flags in FLAGS:
                st = _run(ops, z, labels, plan, flags)
                again = _run(ops, z, labels, plan, flags)
                assert set(st) == set(again) and all(torch.equal(st[k], again[k]) for k in st), (kind, n, flags)
                for k in ("m", "l", "zt"):
                    assert torch.equal(st[k], base[k]), (kind, n, flags, k)
                _check_stats(z, labels, st, flags, plan, f"{kind} rows {rows} V {V} slices {n} {flags}")
                if kind == "quantised" and flags[1]:
                    assert torch.equal(st["zsum"].double(), zd.sum(-1)), (n, flags)
            by_n[n] = _run(ops, z, labels, plan, (True, True, True))
        for a, b in itertools.combinations(by_n, 2):
            assert torch.equal(by_n[a]["aidx"], by_n[b]["aidx"]) and torch.equal(by_n[a]["amax"], by_n[b]["amax"])
            l2a, l2b = (2.0 * s["m"].double() + torch.log(s["l2"].double()) for s in (by_n[a], by_n[b]))
            assert ((l2a - l2b).abs() <= 2e-5 * torch.logsumexp(2 * zd, -1).abs().clamp_min(1.0)).all(), (kind, a, b)


def _tie_rows():
    """Rows of V = 2056 (257 chunks of 8: chunk c belongs to thread c % 256, lane (c % 256) % 64, wave (c % 256) // 64 of a
    one-slice launch) whose maximum 25 is held twice; -> (z, expected first index)."""
    V = 2056
    g = torch.Generator().manual_seed(9)
    cases = [("one chunk", (8 * 40 + 2, 8 * 40 + 5)),
             ("two chunks of one thread", (3, 8 * 256 + 1)),
             ("two lanes", (8 * 5 + 5, 8 * 9)),
             ("two lanes, the first in the higher lane", (8 * 10 + 7, 8 * 256 + 2)),
             ("two waves", (8 * 70, 8 * 130 + 4)),
             ("two waves, the first in the higher wave, the second in the last column", (8 * 200, V - 1)),
             ("two slices", (100, 2000)),
             ("the last column alone", (V - 1,)),
             ("all equal", None),
             ("all -inf", None)]
    z = (torch.randn((len(cases), V), generator=g) * 3).clamp_(-20, 20)
    want = []
    for r, (name, cols) in enumerate(cases):
        if cols is None:
            z[r] = 1.5 if name == "all equal" else -INF
            want.append(0)
        else:
            z[r, list(cols)] = 25.0
            want.append(min(cols))
    return z.to(bf).to(D), torch.tensor(want), [c[0] for c in cases]


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("descending", [False, True])
def test_argmax_is_the_first_index_at_every_level_of_the_reduction(ops, n, descending):
    """The maximum held twice -- inside one chunk, in two chunks of one thread, in two lanes, in two waves, in two slices -- in the
    last column, by every column and by none (-inf throughout): the first column wins, in 5-row batches, for slices fed in
    ascending and in descending v0, and with every combination of the other statistics."""
    z, want, names = _tie_rows()
    assert torch.equal(_first_max(z)[1], want)
    plan = _plan(PLANS[2056][n])
    if descending:
        plan = plan[::-1]
    for r0 in (0, 5):
        zz, labels = z[r0:r0 + 5].contiguous(), _labels(5, 2056, 3)
        base = _run(ops, zz, labels, plan)
        for flags in FLAGS:
            if not flags[0]:
                continue
            st = _run(ops, zz, labels, plan, flags)
            got = st["aidx"].cpu()
            for i in range(5):
                assert got[i] == want[r0 + i], (names[r0 + i], flags, int(got[i]), int(want[r0 + i]))
            assert torch.equal(st["amax"].cpu(), _first_max(zz)[0])
            for k in ("m", "l", "zt"):
                assert torch.equal(st[k], base[k]), (flags, k)
    one = _run(ops, z[:1].contiguous(), _labels(1, 2056, 3), plan, (True, False, False))      # rows = 1
    assert one["aidx"].item() == want[0]


def test_first_column_above_32_bits(ops):
    """v0 = 2^31 + 8 (only the slice exists): indices and the label's column are 64-bit."""
    rows, Vs, v0 = 5, 264, 2 ** 31 + 8
    z = _quantised(rows, Vs, 13)
    labels = torch.tensor([v0, v0 + Vs - 1, v0 + 17, 5, v0 + Vs], dtype=torch.int64, device=D)   # the last two: not in this slice
    base = _run(ops, z, labels, [(0, Vs)], None, base=v0)
    st = _run(ops, z, labels, [(0, Vs)], (True, True, True), base=v0)
    mx, first = _first_max(z)
    assert torch.equal(st["aidx"].cpu(), first + v0) and (st["aidx"] > 2 ** 31).all()
    assert torch.equal(st["amax"].cpu(), mx) and torch.equal(st["zsum"].double(), z.double().sum(-1))
    want_zt = torch.tensor([z[0, 0].item(), z[1, Vs - 1].item(), z[2, 17].item(), 777.0, 777.0])
    assert torch.equal(st["zt"].cpu(), want_zt)
    for k in ("m", "l", "zt"):
        assert torch.equal(st[k], base[k])


def test_zsum_of_full_rows_at_the_training_vocabulary(ops):
    """rows = 5, V = 151 936 in 5 slices: on quantised logits the sum EQUALS float64's (no element dropped or counted twice), on
    gaussian logits it is within L 2^-24 sum|z|, L = the kernel's stated chain + the slice count (and L <= 160 even in one slice)."""
    rows, V = 5, 151936
    vs = (-(-V // 5) + 255) // 256 * 256
    plan = [(v0, min(vs, V - v0)) for v0 in range(0, V, vs)]
    assert len(plan) == 5 and chain(V) + 1 <= 160
    labels = _labels(rows, V, 17)
    z = _quantised(rows, V, 15)
    st = _run(ops, z, labels, plan, (True, True, True))
    assert torch.equal(st["zsum"].double(), z.double().sum(-1))
    _check_stats(z, labels, st, (True, True, True), plan, "quantised V 151936")
    z = _gaussian(rows, V, 16)
    st = _run(ops, z, labels, plan, (True, True, True))
    _check_stats(z, labels, st, (True, True, True), plan, "gaussian V 151936")
    base = _run(ops, z, labels, plan)
    for k in ("m", "l", "zt"):
        assert torch.equal(st[k], base[k])


def test_bad_arguments_launch_nothing(ops):
    """amax without aidx and the reverse, misaligned pointers, Vs % 8 != 0: U2_ERR_ARG from the library (raised by the wrapper's
    check), the state untouched."""
    from u2tokenizer_amd import _lib
    h = _lib.load_library()
    rows, Vs = 5, 264
    z = _quantised(rows, Vs, 19)
    labels = _labels(rows, Vs, 20)
    f32 = lambda v: torch.full((rows + 1,), v, device=D)
    m, l, zt, amax, zsum, l2 = f32(-INF), f32(0.0), f32(777.0), f32(-INF), f32(0.0), f32(0.0)
    aidx = torch.full((rows + 1,), INT64_MAX, dtype=torch.int64, device=D)
    p = lambda t, off=0: t.data_ptr() + off
    good = [p(z), Vs, rows, Vs, 0, p(labels), p(m), p(l), p(zt), p(amax), p(aidx), p(zsum), p(l2), None]

    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return h.u2tok_ce_stats_update(*a)

    assert call(a9=None) == -1 and call(a10=None) == -1
    assert call(a0=p(z, 8)) == -1 and call(a6=p(m, 2)) == -1 and call(a9=p(amax, 2)) == -1 and call(a10=p(aidx, 4)) == -1
    assert call(a11=p(zsum, 1)) == -1 and call(a12=p(l2, 2)) == -1 and call(a5=p(labels, 4)) == -1
    assert call(a3=260) == -1 and call(a1=268, a3=260) == -1
    torch.cuda.synchronize()
    assert (m == -INF).all() and not l.any() and (zt == 777.0).all() and (amax == -INF).all() and (aidx == INT64_MAX).all()
    assert not zsum.any() and not l2.any()
    with pytest.raises(RuntimeError):
        ops.ce_stats_update(z, 0, labels, m[:rows], l[:rows], zt[:rows], amax=amax[:rows])
    with pytest.raises(RuntimeError):
        ops.ce_stats_update(z[:, :260], 0, labels, m[:rows], l[:rows], zt[:rows])
    assert call() == 0                                                  # the same arguments, unbroken: it runs
    torch.cuda.synchronize()
    assert torch.equal(aidx[:rows].cpu(), _first_max(z)[1]) and aidx[rows] == INT64_MAX


# ------------------------------------------------------------------------------------------------ the Function
def _problem(R, E, V, ignored, seed):
    """h, w on the CPU generator (the float64 properties below were checked there), logits of std 4."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn((R, E), generator=g).to(bf)
    w = (torch.randn((V, E), generator=g) * (4.0 / E ** 0.5)).to(bf)
    labels = torch.randint(0, V, (R,), generator=g)
    if ignored > 0:
        labels[torch.rand(R, generator=g) < ignored] = -100
        labels[0] = 3                                                   # (at least one labelled row)
    return h.to(D), w.to(D), labels.to(D)


def _slice_bytes(kept, V, nslices):
    return loss_head.DEFAULT_SLICE_BYTES if nslices == 1 else kept * 2 * max(256, -(-V // nslices) // 256 * 256)


def _recomputed(ops, h, w, labels, slice_bytes):
    """The Z the head saw: the same compaction, the same plan, the same products."""
    idx, _ = loss_head.compact_rows(labels, w.shape[0])
    hp = h[idx].contiguous()
    plan = loss_head.plan_slices(idx.numel(), w.shape[0], slice_bytes)
    return idx, torch.cat([ops.gemm(hp, w[v0:v0 + vs].contiguous()) for v0, vs in plan], 1), plan


@pytest.mark.parametrize("R", [5, 300])
@pytest.mark.parametrize("V", [264, 8000])
@pytest.mark.parametrize("ignored", [0.0, 0.6])
@pytest.mark.parametrize("nslices", [1, 4])
def test_token_stats_function(ops, monkeypatch, R, V, ignored, nslices):
    """logprob and both gradients bit-equal to token_logprobs with and without extras, the same number of products; argmax = the
    first maximum of the recomputed products, and = float64's argmax wherever float64's top-1 margin exceeds 2^-7 max|z| (at least
    3/4 of the rows); logit_sum and lse2m against float64 over the recomputed products; rows without a label hold the fill values."""
    E = 64
    h, w, labels = _problem(R, E, V, ignored, 100 + R + V)
    kept = int((labels != -100).sum())
    sb = _slice_bytes(kept, V, nslices)
    gemms = [0]
    real_gemm = ops.gemm

    def counting(*a, **k):
        gemms[0] += 1
        return real_gemm(*a, **k)

    gw = torch.rand(R, generator=torch.Generator().manual_seed(1)).to(D) + 0.5

    def run(fn):
        hh, ww = h.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
        gemms[0] = 0
        monkeypatch.setattr(ops, "gemm", counting)
        n0 = dict(loss_head.stats)
        with torch.enable_grad():
            out = fn(hh, ww)
            lp = out if torch.is_tensor(out) else out.logprob
            (lp * gw).sum().backward()
        monkeypatch.setattr(ops, "gemm", real_gemm)
        assert loss_head.stats["calls"] == n0["calls"] + 1 and loss_head.stats["rows"] == n0["rows"] + kept
        assert loss_head.stats["rows_skipped"] == n0["rows_skipped"] + R - kept
        return out, lp.detach(), hh.grad, ww.grad, gemms[0]

    kw = dict(shift=False, slice_bytes=sb)
    ref = run(lambda hh, ww: loss_head.token_logprobs(hh, ww, labels, **kw))
    plain = run(lambda hh, ww: loss_head.token_stats(hh, ww, labels, **kw))
    full = run(lambda hh, ww: loss_head.token_stats(hh, ww, labels, want=("lse2", "logit_sum", "argmax"), **kw))
    one = run(lambda hh, ww: loss_head.token_stats(hh, ww, labels, want=("argmax",), **kw))
    for got in (plain, full, one):
        for i, name in ((1, "logprob"), (2, "dh"), (3, "dW")):
            assert torch.equal(got[i], ref[i]), name
        assert got[4] == ref[4] and got[4] > 0                          # the vocabulary is walked once, whatever is wanted
    st = full[0]
    assert plain[0].argmax is None and plain[0].logit_sum is None and plain[0].lse2m is None and one[0].lse2m is None
    assert st.logprob.requires_grad and not st.argmax.requires_grad and not st.logit_sum.requires_grad and not st.lse2m.requires_grad
    assert st.argmax.dtype == torch.int64 and st.logit_sum.dtype == torch.float32 and st.lse2m.dtype == torch.float32
    assert torch.equal(one[0].argmax, st.argmax) and torch.equal(st.labelled, labels != -100)
    off = labels == -100
    assert (st.argmax[off] == -100).all() and not st.logit_sum[off].any() and not st.lse2m[off].any() and not st.logprob[off].any()
    # against the products the head saw
    idx, Z, plan = _recomputed(ops, h, w, labels, sb)
    assert len(plan) == 1 if nslices == 1 else len(plan) >= min(nslices, -(-V // 256)) >= 2       # (V = 264: 256 + 8 columns)
    assert torch.equal(st.argmax[idx].cpu(), _first_max(Z)[1])
    zd = Z.double()
    L = max(chain(vs) for _, vs in plan) + len(plan)
    err = (st.logit_sum[idx].double() - zd.sum(-1)).abs()
    print(f"  R {R} V {V} slices {len(plan)}: logit_sum max err {err.max().item():.3g} (L = {L})")
    assert (err <= L * 2.0 ** -24 * zd.abs().sum(-1)).all()
    # lse2m = lse2 - 2 lse: the bound of lse2 (2e-5 max(1, |lse2|)) plus twice that of lse (1e-5 max(1, |lse|))
    lse2, lse = torch.logsumexp(2 * zd, -1), torch.logsumexp(zd, -1)
    err = (st.lse2m[idx].double() - (lse2 - 2 * lse)).abs()
    print(f"  lse2m max err {err.max().item():.3g}")
    assert (err <= 2e-5 * lse2.abs().clamp_min(1.0) + 2e-5 * lse.abs().clamp_min(1.0)).all()
    # against float64 logits of the same bf16 operands
    z64 = h[idx].double() @ w.double().t()
    top = z64.topk(2, -1)
    decisive = (top.values[:, 0] - top.values[:, 1]) > 2.0 ** -7 * z64.abs().max(-1).values
    print(f"  decisive rows: {int(decisive.sum())} of {idx.numel()}")
    assert 4 * int(decisive.sum()) >= 3 * idx.numel()
    assert torch.equal(st.argmax[idx][decisive], top.indices[:, 0][decisive])


def test_token_stats_without_any_label_launches_nothing(ops, monkeypatch):
    h, w, labels = _problem(5, 64, 264, 0.0, 41)
    labels[:] = -100

    def refuse(*a, **k):
        raise AssertionError("nothing is to be launched")

    for name in ("gemm", "ce_stats_update", "ce_lse_update", "gather_rows"):
        monkeypatch.setattr(ops, name, refuse)
    st = loss_head.token_stats(h.view(1, 5, 64), w, labels.view(1, 5), want=("argmax", "logit_sum", "lse2"), shift=False)
    assert st.logprob.shape == (1, 5) and not st.logprob.any() and (st.argmax == -100).all() and st.argmax.dtype == torch.int64
    assert not st.logit_sum.any() and not st.lse2m.any() and not st.labelled.any()


# ------------------------------------------------------------------------------------------------ whole models
def _lm(kind, dtype, seed=17, decisive=None, **switches):
    common = dict(vocab_size=512, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, max_position_embeddings=512,
                  pad_token_id=0, bos_token_id=1, eos_token_id=2)
    if kind == "qwen3":
        cfg = LM.u2Qwen3Config(num_attention_heads=4, num_key_value_heads=2, head_dim=128, tie_word_embeddings=False, **common)
        cls = LM.u2Qwen3ForCausalLM
    else:      # tied embeddings, as Llama-3.2-1B
        cfg = LM.u2Config(num_attention_heads=8, num_key_value_heads=2, head_dim=64, tie_word_embeddings=True,
                          rope_theta=500000.0, **common)
        cls = LM.u2LlamaForCausalLM
    for k, v in switches.items():
        setattr(cfg, k, v)
    m = cls(cfg)
    synth.fill_module_(m, seed=seed, prefix="decoder.")
    if decisive is not None:
        decisive_decoder_(m, decisive)
    return m.to(dtype).to(D)


def _sft_batch(B, S, lens, prompt, vocab, seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (B, S), generator=g)
    mask = torch.zeros((B, S), dtype=torch.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    ids[mask == 0] = 0
    labels = ids.clone()
    labels[mask == 0] = -100          # right padding
    labels[:, :prompt] = -100         # masked prompt
    return ids.to(D), mask.to(D), labels.to(D)


def _accuracy(pred_ids, label_ids, rows=None):
    """Token accuracy the way an SFT driver's compute_metrics has it: predictions [:, :-1] against labels [:, 1:] where the label
    is not -100 (`rows`: a further (B, S - 1) selection)."""
    preds, labels = pred_ids[:, :-1], label_ids[:, 1:]
    valid = labels != -100
    if rows is not None:
        valid = valid & rows
    return (preds[valid] == labels[valid]).double().mean().item(), valid


@pytest.mark.parametrize("kind", ["qwen3", "llama"])
def test_sft_evaluation_predictions(ops, kind):
    """Both switches on: out.logits is the (B, S) int64 argmax, the loss is the loss head's bit for bit, and the token accuracy from
    `predictions_for_metrics` equals the one from the stock model's argmax(logits) on the decisive rows (float64 top-1 margin of
    the stock model's final hidden states over 2^-7 max|z|: at least 3/4 of the labelled rows).  Predictions switch off: logits None.
    Loss head off: stock logits, whose argmax `predictions_for_metrics` takes."""
    B, S = 2, 96
    ids, mask, labels = _sft_batch(B, S, (96, 61), 20, 512)
    make = lambda **sw: _lm(kind, bf, decisive=5, **sw).eval()
    stock, head = make(), make(u2_fused_loss_head=True)
    both = make(u2_fused_loss_head=True, u2_fused_loss_head_predictions=True)
    only_pred = make(u2_fused_loss_head_predictions=True)
    with torch.no_grad():
        s = stock(input_ids=ids, attention_mask=mask, labels=labels)
        hidden = stock.model(input_ids=ids, attention_mask=mask).last_hidden_state
        n0 = dict(loss_head.stats)
        hd = head(input_ids=ids, attention_mask=mask, labels=labels)
        bt = both(input_ids=ids, attention_mask=mask, labels=labels)
        assert loss_head.stats["calls"] == n0["calls"] + 2
        op = only_pred(input_ids=ids, attention_mask=mask, labels=labels)
        assert loss_head.stats["calls"] == n0["calls"] + 2                 # (the predictions switch alone does nothing)
    assert hd.logits is None
    assert bt.logits.dtype == torch.int64 and bt.logits.shape == (B, S) and torch.equal(bt.loss, hd.loss)
    assert op.logits.shape == (B, S, 512) and torch.equal(op.logits, s.logits) and torch.equal(op.loss, s.loss)
    shifted = loss_head.shift_labels(labels)
    assert (bt.logits[shifted == -100] == -100).all() and (bt.logits[shifted != -100] >= 0).all()
    pred_head = loss_head.predictions_for_metrics(bt.logits, labels)
    pred_stock = loss_head.predictions_for_metrics(s.logits, labels)
    assert pred_head is bt.logits and torch.equal(pred_stock, s.logits.argmax(-1))
    z64 = hidden.double() @ stock.lm_head.weight.double().t()
    top = z64.topk(2, -1)
    decisive = ((top.values[..., 0] - top.values[..., 1]) > 2.0 ** -7 * z64.abs().amax(-1))[:, :-1]
    acc_head, rows = _accuracy(pred_head, labels, decisive)
    acc_stock, _ = _accuracy(pred_stock, labels, decisive)
    n_valid = int((labels[:, 1:] != -100).sum())
    print(f"  {kind}: {int(rows.sum())} decisive of {n_valid} labelled rows, accuracy {acc_head:.4f} (stock {acc_stock:.4f}), "
          f"all rows {_accuracy(pred_head, labels)[0]:.4f} (stock {_accuracy(pred_stock, labels)[0]:.4f})")
    assert 4 * int(rows.sum()) >= 3 * n_valid
    assert torch.equal(pred_head[:, :-1][rows], pred_stock[:, :-1][rows]) and acc_head == acc_stock
    assert torch.equal(pred_head[:, :-1][rows], top.indices[..., 0][:, :-1][rows])


def _err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-30)).item()


def _dpo_from_logits(logits, labels, n, V, ipo):
    """A DPO trainer's concatenated-forward outputs from full logits, in float64."""
    z, tgt = logits.double()[:, :-1], labels[:, 1:]
    on = tgt != -100
    lsm = z.log_softmax(-1)
    lp = torch.gather(lsm, 2, tgt.clamp_min(0)[..., None])[..., 0] * on
    logps = lp.sum(-1) / (on.sum(-1) if ipo else 1)
    w = ((lp - torch.logsumexp(2 * lsm, -1)) * on).sum(-1) / on.sum(-1)
    return {"chosen_logps": logps[:n], "rejected_logps": logps[n:], "mean_chosen_logits": z[:n][on[:n]].mean(),
            "mean_rejected_logits": z[n:][on[n:]].mean(), "policy_weights": torch.exp(w[:n] + w[n:]).clamp(max=1),
            "nll_loss": -lp[:n].sum() / on[:n].sum()}


@pytest.mark.parametrize("grad", [True, False])
@pytest.mark.parametrize("kind", ["qwen3", "llama"])
def test_dpo_outputs_from_model_token_stats(ops, kind, grad):
    """`model.token_stats(..., want=("logit_sum", "lse2"))` on a [chosen; rejected] batch -> `dpo_outputs`, against the same
    quantities from full logits in float64.  The log-probs (summed, and IPO's means) with the tolerance of test_gpu_loss_head.py's
    DPO test (against the fp32 stock model, no further than 1.5 x the bf16 stock model is, + 1e-3); mean logits, policy weights and
    the NLL against the bf16 stock model's own full logits with the kernel-level bounds."""
    B, S, V = 2, 80, 512
    ids_c, mask_c, lab_c = _sft_batch(B, S, (80, 52), 16, V, seed=5)
    ids_r, mask_r, lab_r = _sft_batch(B, S, (67, 80), 16, V, seed=6)
    ids_r[:, :16] = ids_c[:, :16]                      # the same prompt
    ids, mask, labels = torch.cat((ids_c, ids_r)), torch.cat((mask_c, mask_r)), torch.cat((lab_c, lab_r))
    with torch.set_grad_enabled(grad):
        ref_logits = _lm(kind, torch.float32)(input_ids=ids, attention_mask=mask, use_cache=False).logits.detach()
        stock_logits = _lm(kind, bf)(input_ids=ids, attention_mask=mask, use_cache=False).logits.detach()
        ref, stock = _dpo_from_logits(ref_logits, labels, B, V, False), _dpo_from_logits(stock_logits, labels, B, V, False)
        m = _lm(kind, bf)
        n0 = dict(loss_head.stats)
        st = m.token_stats(None, ids, labels, attention_mask=mask, want=("logit_sum", "lse2"))
        out = loss_head.dpo_outputs(st, B, vocab=V, use_weighting=True, rpo=True)
        ipo = loss_head.dpo_outputs(st, B, vocab=V, ipo=True)
    assert set(ipo) == {"chosen_logps", "rejected_logps", "mean_chosen_logits", "mean_rejected_logits"}
    ref_ipo, stock_ipo = _dpo_from_logits(ref_logits, labels, B, V, True), _dpo_from_logits(stock_logits, labels, B, V, True)
    for name in ("chosen_logps", "rejected_logps"):
        es, ef = _err(stock_ipo[name], ref_ipo[name]), _err(ipo[name].detach(), ref_ipo[name])
        print(f"  ipo {name}: fused {ef:.3g}, stock bf16 {es:.3g}")
        assert ef <= 1.5 * es + 1e-3, ("ipo", name, ef, es)
    shifted = loss_head.shift_labels(labels)
    assert loss_head.stats["calls"] == n0["calls"] + 1 and loss_head.stats["rows"] == n0["rows"] + int((shifted != -100).sum())
    assert set(out) == set(ref) and st.argmax is None and st.logprob.shape == (2 * B, S)
    assert st.logprob.requires_grad == grad and out["chosen_logps"].requires_grad == grad and out["nll_loss"].requires_grad == grad
    assert not out["policy_weights"].requires_grad and not out["mean_chosen_logits"].requires_grad
    if grad:
        with torch.enable_grad():
            (out["chosen_logps"].sum() - out["rejected_logps"].sum() + out["nll_loss"]).backward()
        assert m.lm_head.weight.grad is not None and torch.isfinite(m.lm_head.weight.grad.float()).all()
    for name in ("chosen_logps", "rejected_logps"):
        es, ef = _err(stock[name], ref[name]), _err(out[name].detach(), ref[name])
        print(f"  {name}: fused {ef:.3g}, stock bf16 {es:.3g}")
        assert ef <= 1.5 * es + 1e-3, (name, ef, es)
    assert ((out["policy_weights"] > 0) & (out["policy_weights"] <= 1)).all()
    # the rest, against the bf16 stock model's own logits z (float64 arithmetic on them) with the kernel-level bounds:
    #   mean logits: L 2^-24 sum|z| over the half's labelled rows / their count (L = chain(512) + 1 slice);
    #   nll: a mean of lse - z_label: the lse bound 1e-5 max(1, |lse|), taken at the largest |lse|;
    #   policy weights: exp of a sum of two means of (logprob - lse2m): in the exponent 2 x (lse bound + lse2m bound =
    #   2e-5 max(1, |lse2|) + 2e-5 max(1, |lse|)), as a relative bound on the weight.
    z = stock_logits.double()[:, :-1]
    on = labels[:, 1:] != -100
    L = chain(V) + 1
    lse_b = 1e-5 * torch.logsumexp(z, -1)[on].abs().max().clamp_min(1.0).item()
    lse2_b = 2e-5 * torch.logsumexp(2 * z, -1)[on].abs().max().clamp_min(1.0).item()
    for name, half in (("mean_chosen_logits", slice(0, B)), ("mean_rejected_logits", slice(B, 2 * B))):
        bound = L * 2.0 ** -24 * z[half][on[half]].abs().sum().item() / (int(on[half].sum()) * V)
        err = abs(out[name].item() - stock[name].item())
        print(f"  {name}: {out[name].item():.6g}, stock {stock[name].item():.6g}, |d| {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (name, err, bound)
    err = abs(out["nll_loss"].item() - stock["nll_loss"].item())
    print(f"  nll_loss: {out['nll_loss'].item():.6g}, stock {stock['nll_loss'].item():.6g}, |d| {err:.3g}, bound {lse_b:.3g}")
    assert err <= lse_b, ("nll_loss", err, lse_b)
    rel = ((out["policy_weights"].double() - stock["policy_weights"]).abs() / stock["policy_weights"]).max().item()
    wb = math.expm1(2 * (lse_b + lse2_b + 2 * lse_b))
    print(f"  policy_weights: {out['policy_weights'].tolist()}, stock {stock['policy_weights'].tolist()}, rel {rel:.3g}, bound {wb:.3g}")
    assert rel <= wb, ("policy_weights", rel, wb)
