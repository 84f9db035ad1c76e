"""CPU: the host side of the loss head's statistics (loss_head.token_stats and what is built on it) -- `predictions_for_metrics` on
both kinds of input, `dpo_outputs` against the float64 expressions on full logits, which calls of a u2 causal LM reach
`loss_head.token_stats` (replaced by a recorder) for each setting of the two config switches, the fill values of `TokenStats`, and the
argument checks of u2tok_ce_stats_update on both builds."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from u2tokenizer_amd import _lib, language_model as LM, loss_head

ERR_ARG = -1


# ------------------------------------------------------------------------------------------------ predictions_for_metrics
def test_predictions_for_metrics_passes_predictions_through_and_reduces_logits():
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.int64, torch.int32):
        pred = torch.randint(-100, 50, (3, 7), generator=g).to(dtype)
        assert loss_head.predictions_for_metrics(pred, None) is pred
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        logits = torch.randn(3, 7, 11, generator=g).to(dtype)
        logits[0, 0, 4] = logits[0, 0, 9] = 50.0                      # a tie: the first index, as torch.argmax
        got = loss_head.predictions_for_metrics(logits, torch.zeros(3, 7, dtype=torch.int64))
        assert got.dtype == torch.int64 and torch.equal(got, torch.argmax(logits, -1)) and got[0, 0] == 4
    assert torch.equal(loss_head.predictions_for_metrics(torch.zeros(2, 3, 5)), torch.zeros(2, 3, dtype=torch.int64))   # labels optional


# ------------------------------------------------------------------------------------------------ dpo_outputs
def _full_logit_stats(logits, labels):
    """A TokenStats in float64 from full logits (B, S, V), labels shifted inside: each field by its definition."""
    shifted = loss_head.shift_labels(labels)
    on = shifted != -100
    lsm = logits.log_softmax(-1)
    lp = torch.gather(lsm, 2, shifted.clamp_min(0)[..., None])[..., 0] * on
    return loss_head.TokenStats(lp, on, torch.where(on, logits.argmax(-1), torch.full_like(shifted, -100)),
                                logits.sum(-1) * on, (torch.logsumexp(2 * logits, -1) - 2 * torch.logsumexp(logits, -1)) * on)


@pytest.mark.parametrize("use_weighting,ipo,rpo", list(itertools.product((False, True), repeat=3)))
def test_dpo_outputs_against_float64_on_full_logits(use_weighting, ipo, rpo):
    B, S, V, n = 4, 6, 16, 2
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(B, S, V, generator=g, dtype=torch.float64) * 3
    labels = torch.randint(0, V, (B, S), generator=g)
    labels[:, :2] = -100
    labels[1, 4:] = -100
    labels[3, 5:] = -100
    st = _full_logit_stats(logits, labels)
    out = loss_head.dpo_outputs(st, n, vocab=V, use_weighting=use_weighting, ipo=ipo, rpo=rpo)
    keys = {"chosen_logps", "rejected_logps", "mean_chosen_logits", "mean_rejected_logits"}
    assert set(out) == keys | ({"policy_weights"} if use_weighting else set()) | ({"nll_loss"} if rpo else set())
    # the same quantities the long way: positions [:, :-1] scored against labels[:, 1:], everything from the logits tensor
    z, tgt = logits[:, :-1], labels[:, 1:]
    mask = tgt != -100
    lsm = z.log_softmax(-1)
    per_tok = torch.gather(lsm, 2, tgt.clamp_min(0)[..., None])[..., 0] * mask
    logps = per_tok.sum(-1) / (mask.sum(-1) if ipo else 1)
    tol = dict(rtol=1e-12, atol=1e-12)
    assert torch.allclose(out["chosen_logps"], logps[:n], **tol) and torch.allclose(out["rejected_logps"], logps[n:], **tol)
    assert torch.allclose(out["mean_chosen_logits"].double(), z[:n][mask[:n]].mean(), rtol=1e-6, atol=1e-7)      # (an fp32 output)
    assert torch.allclose(out["mean_rejected_logits"].double(), z[n:][mask[n:]].mean(), rtol=1e-6, atol=1e-7)
    if use_weighting:
        w = ((per_tok - torch.logsumexp(2 * lsm, -1)) * mask).sum(-1) / mask.sum(-1)
        want = torch.exp(w[:n] + w[n:]).clamp(max=1)
        assert torch.allclose(out["policy_weights"], want, **tol)
        assert ((out["policy_weights"] > 0) & (out["policy_weights"] <= 1)).all() and not out["policy_weights"].requires_grad
    if rpo:
        want = F.cross_entropy(z[:n].reshape(-1, V), tgt[:n].reshape(-1), ignore_index=-100)
        assert torch.allclose(out["nll_loss"], want, **tol)


def test_dpo_outputs_is_differentiable_where_the_logprobs_are_and_checks_its_input():
    B, S, V = 4, 6, 16
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(B, S, V, generator=g, dtype=torch.float64).requires_grad_(True)
    labels = torch.randint(0, V, (B, S), generator=g)
    with torch.enable_grad():
        st = _full_logit_stats(logits, labels)
        st = st._replace(argmax=None, logit_sum=st.logit_sum.detach(), lse2m=st.lse2m.detach())
        out = loss_head.dpo_outputs(st, 2, vocab=V, use_weighting=True, rpo=True)
    assert out["chosen_logps"].requires_grad and out["nll_loss"].requires_grad and not out["policy_weights"].requires_grad
    assert not out["mean_chosen_logits"].requires_grad
    with pytest.raises(ValueError):
        loss_head.dpo_outputs(st, 3, vocab=V)                                         # not a (2 x 3, S) batch
    with pytest.raises(ValueError):
        loss_head.dpo_outputs(st._replace(lse2m=None), 2, vocab=V, use_weighting=True)
    with pytest.raises(ValueError):
        loss_head.dpo_outputs(st._replace(logit_sum=None), 2, vocab=V)


# ------------------------------------------------------------------------------------------------ TokenStats
def test_token_stats_fill_values():
    on = torch.tensor([[True, False, True], [False, False, False]])
    st = loss_head.TokenStats.filled(on)
    assert st.logprob.shape == on.shape and st.logprob.dtype == torch.float32 and not st.logprob.any()
    assert st.labelled is on and st.argmax is None and st.logit_sum is None and st.lse2m is None
    st = loss_head.TokenStats.filled(on, want=("lse2", "argmax", "logit_sum"), ignore_index=-7)
    assert st.argmax.dtype == torch.int64 and st.argmax.shape == on.shape and (st.argmax == -7).all()
    for t in (st.logit_sum, st.lse2m):
        assert t.dtype == torch.float32 and t.shape == on.shape and not t.any()
    assert loss_head.TokenStats.filled(on, want="argmax").argmax.eq(-100).all()
    with pytest.raises(ValueError, match="unknown"):
        loss_head.TokenStats.filled(on, want=("entropy",))
    with pytest.raises(ValueError, match="unknown"):
        loss_head.token_stats(torch.zeros(2, 64), torch.zeros(8, 64), torch.zeros(2, dtype=torch.int64), want=("logits",))
    assert loss_head._want(("lse2", "argmax", "argmax")) == ("argmax", "lse2")       # canonical order, whatever the caller's


def test_stats_function_refuses_what_it_does_not_compute():
    h, w = torch.zeros(4, 64, dtype=torch.float16), torch.zeros(64, 64, dtype=torch.float16)
    lab = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="float16"):
        loss_head.TokenStatsFn.apply(h, w, lab, -100, 1 << 20, ("argmax",))
    with pytest.raises(RuntimeError, match="do not match"):
        loss_head.token_stats(torch.zeros(2, 3, 64, dtype=torch.bfloat16), w.to(torch.bfloat16), torch.zeros(2, 4, dtype=torch.int64),
                              want=("argmax",))


# ------------------------------------------------------------------------------------------------ which calls reach token_stats
class _Cuda(torch.Tensor):
    @property
    def is_cuda(self):
        return True


@pytest.mark.parametrize("head,predictions,with_labels,shift_kw", [c for c in itertools.product(
    (None, False, True), (None, False, True), (False, True), (False, True)) if c[2] or not c[3]])
def test_model_route_switch_matrix(monkeypatch, head, predictions, with_labels, shift_kw):
    """`loss_head.token_stats` is reached exactly when both switches are on and labels are given -- with want=("argmax",), the
    keywords of the loss passed on -- and its argmax becomes the output's `logits`; the predictions switch alone does nothing; the loss
    head alone keeps `logits=None`; without labels, or with the loss head off, the stock logits come back."""
    cfg = LM.u2Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=16)
    if head is not None:
        cfg.u2_fused_loss_head = head
    if predictions is not None:
        cfg.u2_fused_loss_head_predictions = predictions
    torch.manual_seed(0)
    m = LM.u2LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    m.lm_head.weight = nn.Parameter(m.lm_head.weight.detach().as_subclass(_Cuda), requires_grad=False)   # "on the GPU"
    stats_calls, ce_calls = [], []

    def fake_stats(hidden, weight, labels, *, want=(), ignore_index=-100, shift=True, slice_bytes=None):
        stats_calls.append(dict(want=tuple(want), ignore_index=ignore_index, shift=shift, labels=labels))
        assert weight is m.lm_head.weight and hidden.shape == (2, 9, 64)
        on = (loss_head.shift_labels(labels, ignore_index) if shift else labels) != ignore_index
        st = loss_head.TokenStats.filled(on, want=want, ignore_index=ignore_index)
        return st._replace(logprob=-2.5 * on.float(), argmax=torch.where(on, torch.full_like(st.argmax, 7), st.argmax))

    def fake_ce(hidden, weight, labels, **kw):
        ce_calls.append(kw)
        return torch.tensor(1.25)

    monkeypatch.setattr(loss_head, "token_stats", fake_stats)
    monkeypatch.setattr(loss_head, "linear_cross_entropy", fake_ce)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 64, (2, 9), generator=g)
    labels = ids.clone()
    labels[:, :4] = -100
    kw = {}
    if with_labels:
        kw["labels"] = labels
        if shift_kw:
            kw["shift_labels"] = loss_head.shift_labels(labels)
            kw["num_items_in_batch"] = 20
    with torch.no_grad():
        out = m(input_ids=ids, **kw)
    on_head = bool(head) and with_labels
    if on_head and predictions:
        assert len(stats_calls) == 1 and not ce_calls
        call = stats_calls[0]
        assert call["want"] == ("argmax",) and call["ignore_index"] == -100
        assert call["shift"] is (not shift_kw) and call["labels"] is (kw["shift_labels"] if shift_kw else labels)
        assert out.logits.dtype == torch.int64 and out.logits.shape == (2, 9)
        shifted = loss_head.shift_labels(labels)
        assert torch.equal(out.logits, torch.where(shifted != -100, torch.full_like(shifted, 7), torch.full_like(shifted, -100)))
        assert loss_head.predictions_for_metrics(out.logits, labels) is out.logits
        kept = int((shifted != -100).sum())
        assert out.loss.item() == pytest.approx(2.5 * kept / 20 if shift_kw else 2.5)
    elif on_head:
        assert len(ce_calls) == 1 and not stats_calls and out.logits is None and out.loss.item() == 1.25
    else:
        assert not stats_calls and not ce_calls
        assert out.logits.shape == (2, 9, 64) and out.logits.is_floating_point() and (out.loss is not None) == with_labels
        assert loss_head.predictions_for_metrics(out.logits, labels).shape == (2, 9)


def test_model_token_stats_refuses_a_head_that_does_not_qualify():
    cfg = LM.u2Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=16)
    m = LM.u2LlamaForCausalLM(cfg).eval()
    with pytest.raises(RuntimeError, match="token_stats"):             # no fallback: it says so
        m.token_stats(None, torch.ones(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64), want=("logit_sum",))


# ------------------------------------------------------------------------------------------------ C entry point
@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


def test_ce_stats_update_rejects_bad_arguments_before_any_launch(lib):
    P = 1 << 20   # a 256-byte aligned address that is never dereferenced
    # Z, ldz, rows, Vs, v0, labels, m, l, zt, amax, aidx, zsum, l2, stream
    args = [P, 512, 4, 512, 0, P, P, P, P, P, P, P, P, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.u2tok_ce_stats_update(*a)

    for i in (0, 5, 6, 7, 8):                                          # the required pointers, as u2tok_ce_lse_update
        assert call(**{f"a{i}": None}) == ERR_ARG, i
    assert call(a9=None) == ERR_ARG and call(a10=None) == ERR_ARG      # amax without aidx and the reverse
    assert call(a2=0) == ERR_ARG and call(a3=0) == ERR_ARG and call(a4=-8) == ERR_ARG
    assert call(a1=504) == ERR_ARG and call(a1=516) == ERR_ARG         # ldz < Vs, ldz not a multiple of 8
    assert call(a3=508) == ERR_ARG                                     # Vs not a multiple of 8
    assert call(a0=P + 8) == ERR_ARG                                   # Z not 16-byte aligned
    for i in (6, 7, 8, 9, 11, 12):                                     # fp32 state not 4-byte aligned
        assert call(**{f"a{i}": P + 2}) == ERR_ARG, i
    assert call(a10=P + 4) == ERR_ARG and call(a5=P + 4) == ERR_ARG    # int64 arrays not 8-byte aligned
    assert call(a4=(1 << 63) - 8) == ERR_ARG                           # v0 + Vs past int64


def test_ce_stats_update_is_declared_and_bound():
    res, args = _lib.SIGNATURES["u2tok_ce_stats_update"]
    assert res is C.c_int32 and args[1] is C.c_int64 and args[4] is C.c_int64 and len(args) == 14
