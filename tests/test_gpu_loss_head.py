"""GPU: the loss head (u2tokenizer_amd/loss_head.py) -- its two row kernels against float64 / fp32 expressions on the same bf16
values, the autograd Function against float64 with torch's own bf16 path as the yardstick (check_grad of test_gpu_decoder_train.py),
its peak memory against one fp32 copy of the logits, whole small causal LMs with `u2_fused_loss_head` against the fp32 stock model,
and the two log-prob passes of a DPO step."""
import pytest
import torch
import torch.nn.functional as F

from u2tokenizer_amd import language_model as LM, loss_head, synth

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"
ULP = 2.0 ** -8


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    return _ops


def gen(seed):
    return torch.Generator(device=D).manual_seed(seed)


def rms(a, b):
    return (a.double() - b.double()).pow(2).mean().sqrt().item()


def check_grad(got, bf_ref, ref, name=""):
    """test_gpu_decoder_train.py::check_grad: got's rms error against float64 <= 1.5 x torch's bf16 path's + 1 bf16 ulp of the
    maximum.  Prints the ratio of the two errors (a CPU emulation of the head's algorithm gave 1.000 for nll, dh and dW).
    That floor is the rounding of a bf16 RESULT; nll and the loss are fp32 results, whose only error beyond the bf16 logits both
    paths share is the fp32 log-sum-exp: for them the floor is the lse kernel's own bound, 1e-5 max(1, max |ref|), a thousand
    times tighter (at max |nll| ~ 30: 3e-4 against 0.12), so that the 1.5 x is what decides."""
    ref = ref.double()
    assert torch.isfinite(got.float()).all(), name
    e_got, e_bf = rms(got, ref), rms(bf_ref, ref)
    floor = ULP * ref.abs().max().item()
    print(f"  {name}: error {e_got:.4g}, bf16 stock path {e_bf:.4g}, ratio {e_got / max(e_bf, 1e-300):.4f}")
    assert e_got <= 1.5 * e_bf + floor, (name, e_got, e_bf, floor)
    if got.dtype == torch.float32:
        floor32 = 1e-5 * max(1.0, ref.abs().max().item())
        assert e_got <= 1.5 * e_bf + floor32, (name, e_got, e_bf, floor32)


def _slices(V, n):
    vs = (-(-V // n) + 255) // 256 * 256
    return [(v0, min(vs, V - v0)) for v0 in range(0, V, vs)]


def _logits_and_labels(rows, V, seed):
    """bf16 logits reaching |z| = 30 and labels that sit on the first and the last column of every slice of the 1 / 2 / 5 plans."""
    z = (torch.randn((rows, V), device=D, generator=gen(seed)) * 6.5).clamp_(-30, 30).to(bf)
    z[0, 0], z[rows - 1, V - 1] = 30.0, -30.0
    labels = torch.randint(0, V, (rows,), device=D, generator=gen(seed + 1))
    edges = sorted({c for n in (1, 2, 5) for v0, vs in _slices(V, n) for c in (v0, v0 + vs - 1)})
    # (at most 14 edges: the rows = 300 / 1024 cases carry every one of them, for each V; a rows = 5 case only the five lowest)
    assert len(edges) <= rows or rows == 5
    for r, c in zip(range(rows), edges):
        labels[r] = c
    return z, labels


def _lse_run(ops, z, labels, n):
    rows, V = z.shape
    m = torch.full((rows,), float("-inf"), device=D)
    l, zt = torch.zeros(rows, device=D), torch.full((rows,), 777.0, device=D)
    for v0, vs in _slices(V, n):
        ops.ce_lse_update(z[:, v0:v0 + vs], v0, labels, m, l, zt)
    return m + torch.log(l), zt, (m, l)


# ------------------------------------------------------------------------------------------------ kernels alone
@pytest.mark.parametrize("rows,V", [(5, 151936), (300, 128256), (1024, 8000), (1024, 151936), (300, 8000), (5, 128256)])
def test_ce_lse_update_against_float64(ops, rows, V):
    """lse within 1e-5 max(1, |lse|) of float64 on the same bf16 values (room for ~600-term serial fp32 sums per thread), the
    label's logit exact, for 1, 2 and 5 slices; the slice count moves lse by no more than that bound; a repeat is bit-equal."""
    z, labels = _logits_and_labels(rows, V, 11)
    ref = torch.logsumexp(z.double(), -1)
    zt_ref = z.gather(1, labels[:, None])[:, 0].float()
    bound = 1e-5 * ref.abs().clamp_min(1.0)
    got = {}
    for n in (1, 2, 5):
        lse, zt, state = _lse_run(ops, z, labels, n)
        lse2, zt2, state2 = _lse_run(ops, z, labels, n)
        assert torch.equal(lse, lse2) and torch.equal(zt, zt2) and all(torch.equal(a, b) for a, b in zip(state, state2))
        err = (lse.double() - ref).abs()
        print(f"  rows {rows} V {V} slices {n}: max |d lse| {err.max().item():.3g} (max |lse| {ref.abs().max().item():.3g})")
        assert (err <= bound).all(), (n, err.max().item())
        assert torch.equal(zt, zt_ref), n
        got[n] = lse
    for a, b in ((1, 2), (1, 5), (2, 5)):
        assert ((got[a].double() - got[b].double()).abs() <= bound).all(), (a, b)


def _ordered(x):
    """bf16 -> integers whose difference counts representable values between two numbers."""
    i = x.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


@pytest.mark.parametrize("rows,V", [(5, 151936), (300, 128256), (1024, 8000), (300, 151936)])
def test_ce_grad_inplace_against_the_fp32_expression(ops, rows, V):
    """coef (exp(z - lse) - onehot) in fp32 rounded to bf16: equal up to 1 bf16 ulp everywhere, the label column included; rows
    with coef = 0 exactly zero; whatever the slicing; a repeat is bit-equal."""
    z, labels = _logits_and_labels(rows, V, 21)
    lse = torch.logsumexp(z.double(), -1).float()
    coef = torch.randn(rows, device=D, generator=gen(23)) * 0.01
    coef[1::3] = 0.0
    onehot = F.one_hot(labels, V).float()
    want = (coef[:, None] * (torch.exp(z.float() - lse[:, None]) - onehot)).to(bf)
    outs = []
    for n in (1, 5, 5):
        g = z.clone()
        for v0, vs in _slices(V, n):
            ops.ce_grad_inplace(g[:, v0:v0 + vs], v0, labels, lse, coef)
        assert torch.isfinite(g.float()).all()
        d = (_ordered(g) - _ordered(want)).abs()
        assert d.max().item() <= 1, (n, d.max().item())
        at = g.gather(1, labels[:, None])[:, 0]
        assert ((_ordered(at) - _ordered(want.gather(1, labels[:, None])[:, 0])).abs() <= 1).all()
        assert (at[coef > 0].float() <= 0).all() and (at[coef < 0].float() >= 0).all()    # (p - 1) <= 0 on the label column
        assert (g[1::3] == 0).all()
        outs.append(g)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])                # elementwise: slicing changes nothing


# ------------------------------------------------------------------------------------------------ the Function
def _problem(R, E, V, ignored, seed):
    h = torch.randn((R, E), device=D, generator=gen(seed)).to(bf)
    w = (torch.randn((V, E), device=D, generator=gen(seed + 1)) * (5.0 / E ** 0.5)).to(bf)     # logits of std 5: |z| beyond 20
    labels = torch.randint(0, V, (R,), device=D, generator=gen(seed + 2))
    if ignored >= 1.0:
        labels[:] = -100
    elif ignored > 0:
        labels[torch.rand(R, device=D, generator=gen(seed + 3)) < ignored] = -100
    gw = torch.rand(R, device=D, generator=gen(seed + 4)) + 0.5                                # upstream gradient per row
    return h, w, labels, gw


def _stock(h, w, labels, gw, dtype, block=None):
    """nll, dh, dW of F.cross_entropy((h W^T).float(), labels, reduction='none') . gw in `dtype` (bf16: the stock head's own
    rounding points; float64: the reference, in row blocks when `block` is given)."""
    R, (V, E) = h.shape[0], w.shape
    hh, ww = h.detach().clone().to(dtype), w.detach().clone().to(dtype)     # (fresh leaves: .to(bf16) alone would hand back h itself)
    if block is None:
        hh.requires_grad_(True), ww.requires_grad_(True)
        with torch.enable_grad():
            logits = hh @ ww.t()
            logits = logits.float() if dtype == bf else logits
            nll = F.cross_entropy(logits, labels, ignore_index=-100, reduction="none")
            (nll * gw.to(nll.dtype)).sum().backward()
        return nll.detach(), hh.grad, ww.grad
    nll, dh, dw = torch.zeros(R, dtype=dtype, device=D), torch.zeros_like(hh), torch.zeros_like(ww)
    for r0 in range(0, R, block):
        sl = slice(r0, min(R, r0 + block))
        lab = labels[sl]
        keep = lab != -100
        logits = hh[sl] @ ww.t()
        lse = torch.logsumexp(logits, -1)
        safe = lab.clamp_min(0)
        nll[sl] = torch.where(keep, lse - logits.gather(1, safe[:, None])[:, 0], torch.zeros_like(lse))
        p = torch.exp(logits - lse[:, None])
        p.scatter_add_(1, safe[:, None], -torch.ones_like(lse)[:, None])
        p *= (gw[sl].to(dtype) * keep)[:, None]
        dh[sl] = p @ ww
        dw += p.t() @ hh[sl]
    return nll, dh, dw


def _head(h, w, labels, gw, slice_bytes, need_w=True):
    hh, ww = h.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(need_w)
    n0 = dict(loss_head.stats)
    with torch.enable_grad():
        nll = loss_head.TokenNLLFn.apply(hh, ww, labels, -100, slice_bytes)
        (nll * gw).sum().backward()
    kept = int((labels != -100).sum())
    assert loss_head.stats["calls"] == n0["calls"] + 1 and loss_head.stats["rows"] == n0["rows"] + kept
    assert loss_head.stats["rows_skipped"] == n0["rows_skipped"] + labels.numel() - kept
    return nll.detach(), hh.grad, ww.grad


SMALL = [(77, 512, 32064), (300, 2048, 128256)]


@pytest.mark.parametrize("R,E,V", SMALL)
@pytest.mark.parametrize("ignored", [0.0, 0.6])
@pytest.mark.parametrize("nslices", [1, 4])
def test_token_nll_function_against_float64(ops, R, E, V, ignored, nslices):
    h, w, labels, gw = _problem(R, E, V, ignored, 31)
    kept = int((labels != -100).sum())
    slice_bytes = loss_head.DEFAULT_SLICE_BYTES if nslices == 1 else kept * 2 * (-(-V // nslices) // 256 * 256)
    assert len(loss_head.plan_slices(kept, V, slice_bytes)) >= nslices
    ref, stock = _stock(h, w, labels, gw, torch.float64), _stock(h, w, labels, gw, bf)
    got = _head(h, w, labels, gw, slice_bytes)
    again = _head(h, w, labels, gw, slice_bytes)
    assert got[0].dtype == torch.float32 and got[1].dtype == bf and got[2].dtype == bf
    print(f"(R, E, V) = ({R}, {E}, {V}), {ignored:.0%} ignored, {len(loss_head.plan_slices(kept, V, slice_bytes))} slices")
    for i, name in enumerate(("nll", "dh", "dW")):
        assert torch.equal(got[i], again[i]), name                 # no atomics anywhere in the head
        check_grad(got[i], stock[i], ref[i], name)
    assert (got[0][labels == -100] == 0).all() and (got[1][labels == -100] == 0).all()
    # a frozen lm_head: no weight gradient, the same dh
    frozen = _head(h, w, labels, gw, slice_bytes, need_w=False)
    assert frozen[2] is None and torch.equal(frozen[1], got[1]) and torch.equal(frozen[0], got[0])
    # the reference model of DPO: no grad at all
    with torch.no_grad():
        assert torch.equal(loss_head.TokenNLLFn.apply(h, w, labels, -100, slice_bytes), got[0])


@pytest.mark.parametrize("R,E,V", SMALL)
def test_token_nll_function_without_any_label(ops, R, E, V):
    h, w, labels, gw = _problem(R, E, V, 1.0, 41)
    nll, dh, dw = _head(h, w, labels, gw, loss_head.DEFAULT_SLICE_BYTES)
    assert nll.shape == (R,) and not nll.any() and dh.shape == h.shape and not dh.any() and dw.shape == w.shape and not dw.any()
    bad = labels.clone()
    bad[3] = V
    with pytest.raises(ValueError):
        loss_head.TokenNLLFn.apply(h, w, bad, -100, loss_head.DEFAULT_SLICE_BYTES)


@pytest.mark.parametrize("items", [None, 100, "tensor"])
def test_linear_cross_entropy_is_the_stock_causal_lm_loss(ops, items):
    """ForCausalLMLoss semantics: pad-and-shift, mean over the labelled rows or sum / num_items_in_batch; loss and both gradients
    against float64 with the stock bf16 expression as the yardstick."""
    from transformers.loss.loss_utils import ForCausalLMLoss
    B, S, E, V = 3, 50, 512, 32064
    h, w, labels, _ = _problem(B * S, E, V, 0.4, 51)
    labels = labels.view(B, S)
    n = torch.tensor(100, device=D) if items == "tensor" else items
    res = {}
    for name, dtype in (("ref", torch.float64), ("stock", bf)):
        hh, ww = h.detach().clone().to(dtype).view(B, S, E).requires_grad_(True), w.detach().clone().to(dtype).requires_grad_(True)
        with torch.enable_grad():
            logits = hh @ ww.t()
            if dtype == bf:
                loss = ForCausalLMLoss(logits, labels, V, num_items_in_batch=n)
            else:
                loss = F.cross_entropy(logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100,
                                       reduction="mean" if n is None else "sum") / (1 if n is None else 100)
            loss.backward()
        res[name] = (loss.detach(), hh.grad, ww.grad)
    hh, ww = h.detach().clone().view(B, S, E).requires_grad_(True), w.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        loss = loss_head.linear_cross_entropy(hh, ww, labels, num_items_in_batch=n, slice_bytes=1 << 20)
        loss.backward()
    for i, (name, t) in enumerate((("loss", loss.detach()), ("dh", hh.grad), ("dW", ww.grad))):
        check_grad(t, res["stock"][i], res["ref"][i], name)
    assert not hh.grad[:, -1].any()                                  # the last position predicts nothing


def test_token_nll_function_at_the_training_shape(ops):
    """(R, E, V) = (1024, 4096, 151 936): Qwen3-8B's head; the float64 reference in row blocks on the GPU."""
    R, E, V = 1024, 4096, 151936
    h, w, labels, gw = _problem(R, E, V, 0.0, 61)
    got = _head(h, w, labels, gw, loss_head.DEFAULT_SLICE_BYTES)
    again = _head(h, w, labels, gw, loss_head.DEFAULT_SLICE_BYTES)
    stock = _stock(h, w, labels, gw, bf)
    ref = _stock(h, w, labels, gw, torch.float64, block=128)
    print(f"(R, E, V) = ({R}, {E}, {V}), {len(loss_head.plan_slices(R, V))} slices")
    for i, name in enumerate(("nll", "dh", "dW")):
        assert torch.equal(got[i], again[i]), name
        check_grad(got[i], stock[i], ref[i], name)


def test_peak_memory_stays_below_one_fp32_copy_of_the_logits(ops):
    """(R, E, V) = (2048, 1024, 151 936), all rows labelled: forward + backward of the head allocates less than R V 4 bytes (1.24 GB)
    above what was held before the call; the stock head, measured the same way, more."""
    R, E, V = 2048, 1024, 151936
    h, w, labels, gw = _problem(R, E, V, 0.0, 71)
    limit = R * V * 4

    def peak(fn):
        hh, ww = h.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.enable_grad():
            fn(hh, ww).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    new = peak(lambda hh, ww: (loss_head.TokenNLLFn.apply(hh, ww, labels, -100, loss_head.DEFAULT_SLICE_BYTES) * gw).sum())
    old = peak(lambda hh, ww: (F.cross_entropy((hh @ ww.t()).float(), labels, reduction="none") * gw).sum())
    print(f"  peak above the inputs: loss head {new / 2**20:.0f} MiB, stock head {old / 2**20:.0f} MiB, limit {limit / 2**20:.0f} MiB")
    assert old > limit
    assert new < limit


# ------------------------------------------------------------------------------------------------ whole models
def _lm(kind, dtype, seed=17, **switches):
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
    if kind == "llama":
        assert m.lm_head.weight is m.model.embed_tokens.weight
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


def _err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-30)).item()


def _sft_step(m, ids, mask, labels, ckpt=False):
    m.train()
    if ckpt:
        m.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"use_reentrant": False})
    m.zero_grad(set_to_none=True)
    with torch.enable_grad():
        out = m(input_ids=ids, attention_mask=mask, labels=labels, use_cache=False)
        out.loss.backward()
    return out, {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("kind", ["qwen3", "llama"])
@pytest.mark.parametrize("layers_too", [False, True])
def test_model_with_the_loss_head_matches_the_stock_model(ops, kind, layers_too):
    """Loss and every parameter's gradient with `u2_fused_loss_head` (alone, and with `u2_fused_decoder_training` + gradient
    checkpointing) against the fp32 stock model: no further than 1.5 x the stock bf16 model is (+ 1e-3, the convention of
    test_gpu_decoder_train.py's whole-decoder test); the head ran once, on the labelled rows only; logits are None."""
    B, S = 2, 96
    ids, mask, labels = _sft_batch(B, S, (96, 61), 20, 512)
    ref = _sft_step(_lm(kind, torch.float32), ids, mask, labels)
    stock = _sft_step(_lm(kind, bf), ids, mask, labels)
    assert stock[0].logits is not None
    mg = _lm(kind, bf, u2_fused_loss_head=True, u2_fused_decoder_training=layers_too)
    n0 = dict(loss_head.stats)
    fused = _sft_step(mg, ids, mask, labels, ckpt=layers_too)
    kept = int((loss_head.shift_labels(labels) != -100).sum())
    assert loss_head.stats["calls"] == n0["calls"] + 1 and loss_head.stats["rows"] == n0["rows"] + kept
    assert loss_head.stats["rows_skipped"] == n0["rows_skipped"] + B * S - kept and 0 < kept < B * S - 40
    assert fused[0].logits is None and fused[0].loss.dtype == torch.float32
    es, ef = _err(stock[0].loss, ref[0].loss), _err(fused[0].loss, ref[0].loss)
    print(f"  {kind} loss: fused {ef:.3g}, stock bf16 {es:.3g}")
    assert ef <= 1.5 * es + 1e-3, ("loss", ef, es)
    assert fused[1].keys() == ref[1].keys()
    for n in ref[1]:
        es, ef = _err(stock[1][n], ref[1][n]), _err(fused[1][n], ref[1][n])
        assert ef <= 1.5 * es + 1e-3, (n, ef, es)
    # evaluation loss (no grad) takes the head too
    mg.eval()
    n1 = loss_head.stats["calls"]
    with torch.no_grad():
        ev = mg(input_ids=ids, attention_mask=mask, labels=labels)
    assert loss_head.stats["calls"] == n1 + 1 and ev.logits is None
    assert _err(ev.loss, ref[0].loss) <= 1.5 * _err(stock[0].loss, ref[0].loss) + 1e-3
    # num_items_in_batch (the Trainer's gradient accumulation): sum / n
    with torch.no_grad():
        scaled = mg(input_ids=ids, attention_mask=mask, labels=labels, num_items_in_batch=2 * kept)
    assert abs(scaled.loss.item() * 2 - ev.loss.item()) <= 1e-5 * abs(ev.loss.item())
    # without labels, or with the switch off, nothing changes: logits come back
    with torch.no_grad():
        assert mg(input_ids=ids, attention_mask=mask).logits.shape == (B, S, 512)
    assert loss_head.stats["calls"] == n1 + 2


def test_model_route_honours_shift_labels_and_ignore_index(ops):
    """The keywords ForCausalLMLoss takes besides the labels, through the model's forward on the head's route: `shift_labels=`
    (used as given, `labels` then only switches the loss on) and a non-default `ignore_index=`.  Each against the fp32 stock model
    called with the same keywords, the stock bf16 model as the yardstick (1.5 x + 1e-3, as above); the head ran on the rows those
    keywords leave."""
    B, S = 2, 64
    ids, mask, labels = _sft_batch(B, S, (64, 41), 12, 512)
    shifted = loss_head.shift_labels(labels)
    kept = int((shifted != -100).sum())
    other = labels.clone()
    other[other == -100] = -1
    cases = {"plain": dict(labels=labels),
             "shift_labels": dict(labels=torch.full_like(labels, 5), shift_labels=shifted),
             "ignore_index": dict(labels=other, ignore_index=-1)}
    ref, stock, mg = _lm("qwen3", torch.float32).eval(), _lm("qwen3", bf).eval(), _lm("qwen3", bf, u2_fused_loss_head=True).eval()
    got = {}
    with torch.no_grad():
        for name, kw in cases.items():
            n0 = dict(loss_head.stats)
            out = mg(input_ids=ids, attention_mask=mask, **kw)
            assert out.logits is None and loss_head.stats["calls"] == n0["calls"] + 1, name
            assert loss_head.stats["rows"] == n0["rows"] + kept and loss_head.stats["rows_skipped"] == n0["rows_skipped"] + B * S - kept
            want, yard = ref(input_ids=ids, attention_mask=mask, **kw).loss, stock(input_ids=ids, attention_mask=mask, **kw).loss
            assert loss_head.stats["calls"] == n0["calls"] + 1                       # (the other two models kept the stock head)
            es, ef = _err(yard, want), _err(out.loss, want)
            print(f"  {name}: fused {ef:.3g}, stock bf16 {es:.3g}")
            assert ef <= 1.5 * es + 1e-3, (name, ef, es)
            got[name] = out.loss
        # -100 is an ordinary (and invalid) label once ignore_index is another value
        with pytest.raises(ValueError):
            mg(input_ids=ids, attention_mask=mask, labels=labels, ignore_index=-1)
    assert torch.equal(got["plain"], got["shift_labels"]) and torch.equal(got["plain"], got["ignore_index"])   # the same rows


def test_dpo_logprob_passes(ops):
    """Policy (grad) and reference model (no_grad) `token_logprobs` of a chosen / rejected pair, the sigmoid DPO loss and the
    policy's gradients against the fp32 stock computation gather(log_softmax(logits.float())) * mask; yardstick: the stock bf16
    models through the same expression."""
    B, S, beta = 2, 80, 0.1
    ids_c, mask_c, lab_c = _sft_batch(B, S, (80, 52), 16, 512, seed=5)
    ids_r, mask_r, lab_r = _sft_batch(B, S, (67, 80), 16, 512, seed=6)
    ids_r[:, :16] = ids_c[:, :16]                      # the same prompt
    ids, mask, labels = torch.cat((ids_c, ids_r)), torch.cat((mask_c, mask_r)), torch.cat((lab_c, lab_r))

    def stock_logps(m):
        logits = m(input_ids=ids, attention_mask=mask, use_cache=False).logits.float()
        tgt = labels[:, 1:]
        keep = tgt != -100
        lp = torch.gather(logits[:, :-1].log_softmax(-1), 2, tgt.clamp_min(0)[..., None])[..., 0]
        return (lp * keep).sum(-1)

    def head_logps(m):
        lp = m.token_logprobs(None, ids, labels, attention_mask=mask)
        assert lp.shape == (2 * B, S) and lp.dtype == torch.float32 and not lp[labels_shifted == -100].any()
        return lp.sum(-1)

    labels_shifted = loss_head.shift_labels(labels)

    def dpo(policy, reference, logps):
        policy.train()
        policy.zero_grad(set_to_none=True)
        with torch.no_grad():
            ref_lp = logps(reference)
        with torch.enable_grad():
            pol_lp = logps(policy)
            margin = (pol_lp[:B] - pol_lp[B:]) - (ref_lp[:B] - ref_lp[B:])
            loss = -F.logsigmoid(beta * margin).mean()
            loss.backward()
        return loss.detach(), pol_lp.detach(), ref_lp, {n: p.grad.detach().clone() for n, p in policy.named_parameters()}

    ref = dpo(_lm("qwen3", torch.float32, 17), _lm("qwen3", torch.float32, 18).eval(), stock_logps)
    stock = dpo(_lm("qwen3", bf, 17), _lm("qwen3", bf, 18).eval(), stock_logps)
    n0 = dict(loss_head.stats)
    fused = dpo(_lm("qwen3", bf, 17), _lm("qwen3", bf, 18).eval(), head_logps)
    assert loss_head.stats["calls"] == n0["calls"] + 2
    assert loss_head.stats["rows"] == n0["rows"] + 2 * int((labels_shifted != -100).sum())
    for i, name in ((0, "dpo loss"), (1, "policy log-probs"), (2, "reference log-probs")):
        es, ef = _err(stock[i], ref[i]), _err(fused[i], ref[i])
        print(f"  {name}: fused {ef:.3g}, stock bf16 {es:.3g}")
        assert ef <= 1.5 * es + 1e-3, (name, ef, es)
    for n in ref[3]:
        es, ef = _err(stock[3][n], ref[3][n]), _err(fused[3][n], ref[3][n])
        assert ef <= 1.5 * es + 1e-3, (n, ef, es)
