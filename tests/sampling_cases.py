"""Shared by the sampling-warper tests (not a test file): the float64 reference of the semantics in include/u2tok.h
(u2tok_sample_warp), the margin function that says which tokens a correct fp32 implementation may decide either way, and the
case table.

Reference, per row:  z = x / T in fp32 (one division; T = 1: z = x);  top-k: k = min(max(top_k, min_keep), V), z_i < (k-th largest z)
removed, ties kept;  top-p over the survivors: STABLE ascending sort (equal values: lower index first, so from the top the higher
index ranks higher), float64 softmax and cumsum, token removed iff its ascending cumulative mass (itself included) is <= 1 - top_p
and it is not among the last min_keep of the sort -- transformers' TopPLogitsWarper with the arithmetic in float64 and the sort
stable;  out = z where kept, -inf elsewhere."""
import math

import torch

NEG = -math.inf
DELTA = 1e-5          # a token whose float64 cumulative mass is this close to 1 - top_p may go either way (see `undecided`)
MAX_UNDECIDED = 4     # per row; a condition on the reference, asserted by the tests

# (temperature, top_k, top_p, min_keep)
PARAMS = {
    "T0.7_p0.9": (0.7, 0, 0.9, 1),
    "k50_p0.9": (1.0, 50, 0.9, 1),
    "T0.2_p0.7": (0.2, 0, 0.7, 1),
    "T1.3_k50_p0.95_keep2": (1.3, 50, 0.95, 2),
    "k5": (1.0, 5, 1.0, 1),
    "p0.9": (1.0, 0, 0.9, 1),
}
VOCABS = (2, 8, 63, 64, 65, 1000, 4097, 32064, 151936)
ROWS = (1, 3, 16, 17)
SHAPES = [(r, v) for v in VOCABS for r in ROWS if v < 151936 or r in (1, 16)]


def logits(rows, V, seed=0, bf16_values=False):
    """fp32 randn * 3 (a spread like trained logits'); bf16_values: rounded to bf16 values -- ties everywhere, what a bf16 lm_head gives"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + V)
    x = torch.randn(rows, V, generator=g) * 3
    return x.bfloat16().float() if bf16_values else x


def reference(x, temperature=1.0, top_k=0, top_p=1.0, min_keep=1):
    """x (rows, V) fp32 on the CPU -> (out fp32, cum float64 | None): cum[r, i] = the ascending cumulative mass of token i (itself
    included) among the survivors of top-k, the quantity the top-p rule compares with 1 - top_p; None without a top-p stage."""
    assert x.dtype == torch.float32 and x.dim() == 2 and not x.is_cuda
    rows, V = x.shape
    z = x / temperature if temperature != 1.0 else x.clone()
    keep = torch.ones(rows, V, dtype=torch.bool)
    if top_k > 0:
        k = min(max(top_k, min_keep), V)
        kth = torch.topk(z, k, dim=-1).values[:, -1:]
        keep &= ~(z < kth)
    cum = None
    if top_p < 1.0:
        zz = torch.where(keep, z, torch.full_like(z, NEG)).double()
        srt, idx = torch.sort(zz, dim=-1, descending=False, stable=True)
        c = torch.softmax(srt, dim=-1).cumsum(dim=-1)
        remove = c <= (1.0 - top_p)
        remove[:, -min_keep:] = False
        keep &= ~torch.zeros_like(remove).scatter(1, idx, remove)
        cum = torch.zeros_like(c).scatter(1, idx, c)
    return torch.where(keep, z, torch.full_like(z, NEG)), cum


def undecided(x, cum, top_p, min_keep=1, delta=DELTA):
    """(rows, V) bool: tokens that may be kept or removed.  fp32 exp of arguments up to ~30, one normalisation and a tree sum over 2^18
    terms give 2-3e-6 relative error in a cumulative mass; delta is that times ~4.  The last min_keep tokens of the stable sort are kept
    by rank, whatever their mass: they are decided.  Without a top-p stage nothing is undecided (top-k is exact)."""
    if cum is None:
        return torch.zeros(x.shape, dtype=torch.bool)
    und = (cum - (1.0 - top_p)).abs() <= delta
    # rank from the top in the stable order: (value desc, index desc); the top min_keep are decided
    order = torch.sort(x.double(), dim=-1, descending=False, stable=True).indices[:, -min_keep:]
    und.scatter_(1, order, False)
    return und


def check(out, x, params, what=""):
    """The acceptance rule: the reference stays inside the cap of undecided tokens per row, and every decided element of `out`
    equals the reference bit for bit (kept values and -inf alike).  -> number of undecided tokens."""
    T, k, p, mk = params
    ref, cum = reference(x, T, k, p, mk)
    # (min_keep ranks by the survivors' values: z, whose order is x's for T > 0 up to ties created by the division -- rank on z)
    z = x / T if T != 1.0 else x
    und = undecided(z, cum, p, mk)
    per_row = und.sum(-1)
    assert int(per_row.max()) <= MAX_UNDECIDED, f"{what}: the reference has {per_row.tolist()} undecided tokens per row"
    got = out.detach().float().cpu()
    same = (got.view(torch.int32) == ref.view(torch.int32)) | und
    bad = (~same).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} decided elements differ, first (row, col) {bad[0].tolist()}: got "
                              f"{got[tuple(bad[0])].item()!r}, reference {ref[tuple(bad[0])].item()!r}, "
                              f"cum {None if cum is None else cum[tuple(bad[0])].item()!r}")
    return int(und.sum())


def stock(x, temperature=1.0, top_k=0, top_p=1.0, min_keep=1):
    """the transformers warpers the fused one replaces, applied in order (on x's device)"""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    procs = []
    if temperature != 1.0:
        procs.append(TemperatureLogitsWarper(float(temperature)))
    if top_k > 0:
        procs.append(TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=min_keep))
    if top_p < 1.0:
        procs.append(TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=min_keep))
    s = x
    for p in procs:
        s = p(None, s)
    return s, procs
