"""The inference attention kernels' edge sweeps, shared by tests/test_attn_edges_host.py (CPU: the emulation and the mask mutants
against the bound) and tests/test_gpu_attn_edges.py (the kernels against the bound): the mask rule, the case tables, the data
builders and the per-element float64 bound.  Kernels: tok_attn_kernel<64|96|128, EX, BAND> (csrc/tokattn.hip, 64-key tiles, reached
through ops.attention_gqa, its split_keys form, attention_gqa_range and attention_gqa_band) and decode_attn_kernel<64|96|128> with
decode_attn_merge_kernel (csrc/decode_attn.hip, 32-key tiles, ops.decode_attention).

A case is a `Case` tuple; `operands(case, elem)` builds its inputs once per process on the CPU (never modified afterwards):
q (nb, Sq, Hq d) and K / V buffers (nb, Hkv, Skv + spare, d) in a KV cache's layout, of which positions >= Skv are spare capacity no
key of which is visible.  `model` / `emulate` run on whatever device their inputs are on.

Data sets (field `data`):
  normal   q, k, v ~ N(0, 1).
  poison   q = m + N(0, 1) with a fixed sign pattern m (|m|^2 = d), so that every query row has q . qbar ~ d for the sequence's mean
           query qbar; every key that NO row of the sequence may see (below kv_start[b], at or beyond kv_len[b], spare capacity) is
           k = 3 qbar: a score of ~ 3 sqrt(d) >= 24 in natural-log units against N(0, 2) for the visible keys, and v = +-64 there.
           All finite: the kernels multiply p = 0 into masked V rows.
  raised   poison, and the first and the last visible key of each sequence get + 4 m / (scale d): their scores rise by ~ 4.
  rise     scores rising by ~ 10 (> 8) log2 units per 32 keys (20 per 64-key tile): every tile rescales, the last keys carry all the weight.
  first    the first visible key of each sequence ~ 90 natural-log units (130 log2 units; > 100 above every other score): later tiles stay under the
           running max (the lazy branch) and their terms underflow against it.
  steps    all keys of a tile equal and all query rows equal (the lazy branch is a wave-uniform decision over 16 rows), consecutive
           tiles (of `tile` keys: 64 / 32) 7.9 and 8.1 log2 units apart in turn, built from values that are exact in both element
           types: a tile 7.9 above the running max stays under the threshold 8 (lazy), the next one, 16 above it, rescales.
  equal    every key equal and v = |N(0, 1)| + 0.5: each row is a mean of positive values.
  edge     one dominating key per sequence at position `edge[b]` (score + 30, v = +-8): placed just inside and just outside a mask
           edge, in the partial tile of that edge."""
import collections
import functools
import math

import torch

import test_decoder_train_bounds_host as B

u = 2.0 ** -24
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
# name -> (dtype, unit roundoff charged per rounding, half the spacing of the type's subnormals: a probability below the smallest
# normal is rounded absolutely, not relatively -- 2^-25 for IEEE half (normal range from 2^-14); bf16 has fp32's exponent range)
ELEM = {"bf16": (torch.bfloat16, 2.0 ** -8, 0.0), "f16": (torch.float16, 2.0 ** -11, 2.0 ** -25)}
STALE = 7.3   # log2 units the emulation's stale row max lies below the true one (the kernel's lazy branch allows up to 8)

Case = collections.namedtuple("Case", "sweep entry nb Sq Skv Hq Hkv d window kv_start kv_len causal spare layout data edge tile thr",
                              defaults=(8.0,))    # thr: the lazy-rescale threshold the `steps` data straddles, in log2 units


def case(sweep, entry, nb, Sq, Skv, Hq, Hkv, d, window=None, kv_start=None, kv_len=None, causal=True, spare=0, layout="cache",
         data="normal", edge=None, tile=64):
    return Case(sweep, entry, nb, Sq, Skv, Hq, Hkv, d, window, kv_start, kv_len, causal, spare, layout, data, edge, tile)


def case_id(c):
    """(long per-sequence tuples are cut to their first three entries)"""
    return "-".join(str(x[:3] + ("..",) if isinstance(x, tuple) and len(x) > 8 else x).replace(" ", "").replace("'", "") for x in c)


# ------------------------------------------------------------------------------------------------------------------- mask
def visible(Sq, Skv, window=None, kv_start=None, kv_len=None, causal=True, device=None):
    """(nb | 1, Sq, Skv) bool: query i of sequence b sees key j iff kv_start[b] <= j < kv_len[b] and, when causal,
    j <= i + Skv - Sq and (window W) j > i + Skv - Sq - W."""
    i = torch.arange(Sq, device=device)[:, None]
    j = torch.arange(Skv, device=device)[None, :]
    c = Skv - Sq
    vis = torch.ones(Sq, Skv, dtype=torch.bool, device=device)
    if causal:
        vis = vis & (j <= i + c)
        if window:
            vis = vis & (j > i + c - window)
    vis = vis[None]
    if kv_start is not None:
        vis = vis & (j[None] >= torch.tensor(kv_start, device=device)[:, None, None])
    if kv_len is not None:
        vis = vis & (j[None] < torch.tensor(kv_len, device=device)[:, None, None])
    return vis


def case_visible(c, device=None):
    return visible(c.Sq, c.Skv, c.window, c.kv_start, c.kv_len, c.causal, device)


# ----------------------------------------------------------------------------------------------------------- case tables
DS = (64, 96, 128)
GS = (1, 3, 5, 7, 8, 16)
LONG_T = (1023, 1024, 1025, 1792)


def sweep_a():
    """window: column layout, Sq = Skv = 150 (three query blocks, three 64-key tiles, the last partial), every W from 1 to 151"""
    return [case("A", "band", 1, 150, 150, 2, 1, d, window=W, layout="col") for d in DS for W in range(1, 152)]


def sweep_b():
    """continued prefill: Sq new rows behind c_off cached keys, views [:, :, :Skv] of buffers with 5 spare poisoned positions"""
    out, n = [], 0
    for c_off in (1, 31, 32, 63, 64, 65, 100):
        for Sq in (1, 15, 16, 17, 63, 64, 65, 70):
            for W in sorted({0, 1, 16, 17, 63, 64, 65, c_off, c_off + 1}):
                out.append(case("B", "band", 2, Sq, Sq + c_off, 3, 1, DS[n % 3], window=W or None, spare=5, data="poison"))
                n += 1
    return out


def sweep_c():
    """ranges: the edge in the batch dimension, S = 150, 151 sequences, kv_start[b] = b (the last one sees nothing)"""
    S, nb = 150, 151
    start = tuple(range(nb))
    out, n = [], 0
    for Sq in (S, 6):
        for L, W in ((None, None), (1, None), (64, None), (65, None), (None, 40)):
            ln = None if L is None else tuple(min(S, b + L) for b in range(nb))
            for entry in ("range", "band"):
                if W and entry == "range":
                    continue
                out.append(case("C", entry, nb, Sq, S, 2, 1, DS[n % 3], window=W, kv_start=start, kv_len=ln, spare=5 if entry == "band" else 0,
                                layout="cache" if entry == "band" else "col", data="poison"))
                n += 1
    return out


def decode_gd(T):
    """group size and head dim of decode length T: all 18 pairs occur within any 18 consecutive lengths"""
    return GS[T % 6], DS[(T + T // 6) % 3]


def sweep_d():
    """batched decode: every T from 1 to 300 (one tile, unsplit, split, the ntile < 8 threshold) and four long lengths; 8 sequences
    whose first visible key lies at 0, 1, 31, 32, 33, T // 2, T - 1 and T (none visible); strided cache views on odd T"""
    out = []
    for T in list(range(1, 301)) + list(LONG_T):
        g, d = decode_gd(T)
        start = tuple(min(max(s, 0), T) for s in (0, 1, 31, 32, 33, T // 2, T - 1, T))
        out.append(case("D", "decode", 8, 1, T, 2 * g, 2, d, kv_start=start, spare=7 if T % 2 else 0,
                        data="raised" if T > 300 else "poison", tile=32))
    return out


def sweep_e():
    """split form: attention_gqa(causal=False, split_keys=True), 3 sequences of 3 query rows, every T from 1 to 200 and the long ones"""
    out = []
    for T in list(range(1, 201)) + list(LONG_T):
        g = (1, 3, 8)[T % 3]
        out.append(case("E", "split", 3, 3, T, 2 * g, 2, DS[(T + T // 3) % 3], causal=False, spare=3 if T % 2 else 0, layout="col",
                        data="poison"))
    return out


def sweep_f():
    """hard softmax data through all five entry points: S = 150 (tok_attn_kernel), T = 300 and 1025 (the decode kernels)"""
    out = []
    for d in DS:
        for data in ("rise", "first", "steps", "equal"):
            out.append(case("F", "gqa", 2, 150, 150, 2, 1, d, layout="col", data=data))
            out.append(case("F", "range", 2, 150, 150, 2, 1, d, kv_start=(0, 70), kv_len=(150, 140), layout="col", data=data))
            out.append(case("F", "band", 2, 150, 150, 2, 1, d, kv_start=(0, 70), kv_len=(150, 140), spare=5, data=data))
            for T in (300, 1025):
                out.append(case("F", "split", 2, 3, T, 6, 2, d, causal=False, spare=T % 2, layout="col", data=data))
                out.append(case("F", "decode", 4, 1, T, 6, 2, d, kv_start=(0, 33, T // 2, T - 1), spare=T % 2, data=data, tile=32))
        # (v) the dominating key on each side of each edge: the diagonal and the window (row j0 sees it, row j0 - 1 does not; row
        # j0 + 39 does, row j0 + 40 does not), kv_start = 70 (69 | 70), kv_len = 140 (139 | 140), Skv (T - 1 | spare position T)
        for j0 in (63, 64, 69, 70, 100, 127, 128, 139, 140):
            out.append(case("F", "gqa", 1, 150, 150, 2, 1, d, layout="col", data="edge", edge=(j0,)))
            out.append(case("F", "range", 1, 150, 150, 2, 1, d, kv_start=(70,), kv_len=(140,), layout="col", data="edge", edge=(j0,)))
            out.append(case("F", "band", 1, 150, 150, 2, 1, d, window=40, kv_start=(70,), kv_len=(140,), spare=5, data="edge", edge=(j0,)))
        for T in (300, 1025):
            out.append(case("F", "split", 2, 3, T, 6, 2, d, causal=False, spare=1, layout="col", data="edge", edge=(T - 1, T)))
            out.append(case("F", "decode", 4, 1, T, 6, 2, d, kv_start=(33, 33, 0, 0), spare=1, data="edge", edge=(32, 33, T - 1, T), tile=32))
    return out


SWEEPS = {"A": sweep_a, "B": sweep_b, "C": sweep_c, "D": sweep_d, "E": sweep_e, "F": sweep_f}


@functools.lru_cache(maxsize=None)
def cases(sweep):
    return tuple(SWEEPS[sweep]())


# ----------------------------------------------------------------------------------------------------------- data builders
def _pattern(d):
    return torch.where(torch.rand(d, generator=B._gen(6, d)) < 0.5, -1.0, 1.0)


def _first_last(c):
    """per sequence: the first and the last key any row sees (None: no key visible)"""
    vis = case_visible(c).any(1).expand(c.nb, c.Skv)
    res = []
    for b in range(c.nb):
        idx = vis[b].nonzero().flatten()
        res.append((int(idx[0]), int(idx[-1])) if idx.numel() else None)
    return res


@functools.lru_cache(maxsize=None)
def _operands(key, elem):
    c = key
    dt = ELEM[elem][0]
    cap = c.Skv + c.spare
    g = B._gen(7, c.nb, c.Sq, c.Skv, c.Hq, c.Hkv, c.d, c.window or 0, len(c.data), c.tile, sum(c.edge or (0,)))   # (thr: steps draws nothing)
    m = _pattern(c.d)
    scale = c.d ** -0.5
    q = torch.randn(c.nb, c.Sq, c.Hq, c.d, generator=g)
    k = torch.randn(c.nb, c.Hkv, cap, c.d, generator=g)
    v = torch.randn(c.nb, c.Hkv, cap, c.d, generator=g)
    unit = m / (scale * c.d)          # a key's score rises by ~ x (natural log) per x * unit added to it
    if c.data in ("poison", "raised"):
        q = q + m
        qbar = q.mean((1, 2))                                                 # (nb, d)
        inv = torch.ones(c.nb, cap, dtype=torch.bool)
        inv[:, :c.Skv] = ~case_visible(c).any(1).expand(c.nb, c.Skv)
        sign = torch.where(torch.rand(c.nb, c.Hkv, cap, c.d, generator=g) < 0.5, -64.0, 64.0)
        k = torch.where(inv[:, None, :, None], 3.0 * qbar[:, None, None, :], k)
        v = torch.where(inv[:, None, :, None], sign, v)
        if c.data == "raised":
            for b, fl in enumerate(_first_last(c)):
                if fl is not None:
                    for j in set(fl):
                        k[b, :, j] += 4.0 * unit
    elif c.data != "normal":
        q = m + 0.25 * q
        j = torch.arange(cap)
        if c.data == "rise":
            k = 0.1 * k + (10.0 * LN2 * (j // 32))[None, None, :, None] * unit
        elif c.data == "first":
            for b, fl in enumerate(_first_last(c)):
                if fl is not None:
                    k[b, :, fl[0]] += 90.0 * unit
        elif c.data == "steps":
            # every row the same query, (q1 | q2) m over the two halves of the head dim; tile t's keys (t | +-2^-4) m: t, 2^-4 and
            # their products with q are exact in both element types, so tile t's score is t S1 +- S2 in log2 units with
            # S1 = scale (d / 2) q1 log2 e = 8 (to the 0.3 % of q1's rounding) and S2 = 0.05: steps of S1 - 0.1 and S1 + 0.1 in turn
            h, t = c.d // 2, j // c.tile
            per = scale * h * LOG2E
            q1, q2 = torch.tensor(c.thr / per).to(dt).float(), torch.tensor(0.05 / (per * 2.0 ** -4)).to(dt).float()
            q = torch.cat([q1.expand(h), q2.expand(h)])
            if c.thr != 8.0:   # (q1's own rounding, 0.4 % of S1, is more than 0.1 beyond S1 = 25: the half's last element takes it up)
                q[h - 1] = torch.tensor(c.thr / per * h - float(q1) * (h - 1)).to(dt).float()
            q = (q * m).expand(c.nb, c.Sq, c.Hq, c.d)
            k = torch.cat([t[:, None].float().expand(cap, h), torch.where(t % 2 == 0, 1.0, -1.0)[:, None].expand(cap, h) * 2.0 ** -4], 1) * m
            k = k[None, None].expand(c.nb, c.Hkv, cap, c.d)
        elif c.data == "equal":
            k = k[:, :, :1].expand(c.nb, c.Hkv, cap, c.d).clone()
            v = v.abs() + 0.5
        elif c.data == "edge":
            for b, j0 in enumerate(c.edge):
                k[b, :, j0] += 30.0 * unit
                v[b, :, j0] = 8.0 * m
        else:
            raise ValueError(c.data)
    return dict(q=q.reshape(c.nb, c.Sq, c.Hq * c.d).to(dt), K=k.to(dt), V=v.to(dt), scale=scale)


def operands(c, elem):
    """the inputs of a case (shared by its entry points: the entry is not part of the key)"""
    return _operands(c._replace(sweep="", entry="", layout=""), elem)


# ------------------------------------------------------------------------------------------------------------ bound model
def _scores(q, k, scale, vis, bias=None):
    G = q.shape[1] // k.shape[1]
    kk = k.repeat_interleave(G, 1)
    s = (q @ kk.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias
    s = s.masked_fill(~vis[:, None], float("-inf"))
    m = s.max(-1, keepdim=True).values
    return s, torch.where(m == float("-inf"), torch.zeros_like(m), m), kk


def model(q, k, v, scale, vis, U, tiny=0.0, bias=None, c_bias=0.0, pw=None):
    """q (nb, Hq, Sq, d), k / v (nb, Hkv, Skv, d) float64, vis (nb | 1, Sq, Skv) -> out (nb, Hq, Sq, d) and its per-element bound.
    A row that sees no key has out = 0 and bound = 0: the kernels must return exact zeros there.

    Terms (U: the element type's unit roundoff, u = 2^-24; P the exact probabilities):
      U |out|                         the output rounding                                       } attn_fwd_model's terms
      (U + (Skv + d) u) sum_j P_j |v_j|   P enters the P V product rounded; the fp32 accumulation   } (U = 2^-8 there)
      sum_j P_j e_ij (|v_j| + |out|)  the fp32 scores.  s_ij is a d-term fp32 dot product: off by at most d u A_ij,
                                      A_ij = scale sum_c |q_ic k_jc|; the exponent's argument fma(s, scale log2 e, -m) and exp2 add a few
                                      u of |s_ij| + |m_i| + 1 (m_i: the row max).  A score off by e changes p_j by the factor exp(e),
                                      so the normalised P_j' = P_j (1 + e_ij) / sum_k P_k (1 + e_ik): to first order the output moves
                                      by sum_j P_j e_ij v_j - out sum_j P_j e_ij.  e_ij = u (d A_ij + 4 (|s_ij| + |m_i|) + 8).
                                      At N(0, 1) data this is ~ 1e-5, far below U; at |s| ~ 200 it reaches U.
      tiny sum_j |v_j| / l_i          (IEEE half only) a probability below 2^-14 is rounded to a multiple of 2^-24: off by up to
                                      tiny = 2^-25 absolutely.  The kernel's p_j = exp(s_ij - m') with m' <= m_i, so its row sum
                                      is >= l_i = sum_j exp(s_ij - m_i) >= 1 and the absolute errors are scaled down at least as
                                      much as charged here.

    The encoder attention kernels (tests/enc_attn_cases.py, where both are derived) add two parameters:
      bias, c_bias   an additive score term (1 | nb, Hq, Sq, Skv), exact in float64: s_ij = scale q_i . k_j + bias_ij, and e_ij gains
                     c_bias u |bias_ij| for the fp32 operations that touch the bias alone.
      pw             the weight of sum_j P_j |v_j| that stands for P's rounding before the P V product (default U; 0 for a kernel
                     that keeps P in fp32).  Returns also lse = m_i + log l_i (natural log; -inf for a row that sees no key)."""
    d, Skv = q.shape[3], k.shape[2]
    pw = U if pw is None else pw
    s, m, kk = _scores(q, k, scale, vis, bias)
    G = q.shape[1] // k.shape[1]
    vv = v.repeat_interleave(G, 1)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    P = p / l.clamp_min(1e-300)
    out = P @ vv
    A = scale * (q.abs() @ kk.abs().transpose(-1, -2))
    e = u * (d * A + 4 * (s.masked_fill(~vis[:, None], 0.0).abs() + m.abs()) + 8)
    if bias is not None:
        e = e + c_bias * u * bias.abs()
    Pe = P * e
    bound = U * out.abs() + (pw + (Skv + d) * u) * (P @ vv.abs()) + Pe @ vv.abs() + Pe.sum(-1, keepdim=True) * out.abs()
    if tiny:
        bound = bound + tiny * (vis[:, None].to(torch.float64).expand(-1, q.shape[1], -1, -1) @ vv.abs()) / l.clamp_min(1.0)
    lse = torch.where(l > 0, m + torch.log(l.clamp_min(1e-300)), torch.full_like(l, float("-inf")))[..., 0]
    return dict(out=out, bound=bound, P=P, s=s, lse=lse)


def emulate(q, k, v, scale, vis, dt, stale=0.0, bias=None, round_p=True):
    """the kernels: p = exp(s - m') rounded to the element type for the P V product (round_p False: kept as it is, a kernel whose
    P stays in fp32), m' the row max or `stale` log2 units below it (the lazy branch keeps a running max up to 8 below a tile's),
    the row sum of the unrounded p divides, one output rounding"""
    def rnd(t):
        return t.float().to(dt).double()
    s, m, _ = _scores(q, k, scale, vis, bias)
    p = torch.exp(s - m + stale * LN2)
    l = p.sum(-1, keepdim=True)
    G = q.shape[1] // k.shape[1]
    o = (rnd(p) if round_p else p) @ v.repeat_interleave(G, 1)
    return rnd(torch.where(l > 0, o / l.clamp_min(1e-300), torch.zeros_like(o)))


def split_heads(c, ops_, device=None):
    """float64 q (nb, Hq, Sq, d) and k, v (nb, Hkv, Skv, d) of a case's operands"""
    q = ops_["q"].to(device).double().view(c.nb, c.Sq, c.Hq, c.d).permute(0, 2, 1, 3)
    return q, ops_["K"][:, :, :c.Skv].to(device).double(), ops_["V"][:, :, :c.Skv].to(device).double()


def rows(t):
    """(nb, Hq, Sq, d) -> (nb, Sq, Hq d)"""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)


def ratio(err, bound):
    """max of err / bound over ALL elements: 0 / 0 counts as 0, a nonzero error against a zero bound as inf"""
    r = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return r.max().item() if r.numel() else 0.0
