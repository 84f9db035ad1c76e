"""The encoder attention forwards' length sweeps and bias edges, shared by tests/test_enc_attn_bounds_host.py (CPU: the emulation and
the mutants against the bound) and tests/test_gpu_enc_attn_bounds.py (the kernels against the bound): case tables, data builders, the
per-element float64 bound, the emulation and the mutants.  Kernels: tok_attn_kernel<64 .. 512> and the 8-wave tok_attn2_kernel<256 |
512, MUBUF> with the relative-position bias window and the key-split merges tok_attn_combine_ns_kernel<2..8> / tok_attn_combine_kernel
(csrc/tokattn.hip, ops.tok_attention); flash_d64_kernel (mode 1) and flash_dp2_kernel<0 | 1> (mode 7, plain and pre-scaled q) with the
extra row / extra key; temporal_attention_kernel<VPL> (all csrc/attn.hip).

Everything is in HEAD FORM: q (nbe, H, Sq, d), k / v (nbe, H, Skv, d); the GPU module lays the rows out as each entry point reads them.
  tok       nbe = nb, rows (nb, S, H d).  Scale 1 / sqrt(d).  max_len None: no bias.
  flash     d = 64, Sq = Skv = S rows of which, with `extra`, the last one is the kernels' extra row (query AND key).  Scale 0.125.
  temporal  nbe = B N in (b, n) order, Sq = Skv = T; the kernel's rows are (b t n).  Scale 1 / sqrt(d).

The bound is attn_edge_cases.model with its four terms and two additions:

1. Bias.  The exact scores are scale q_i . k_j + bias[j - i + max_len - 1][h].  What the kernels do with a table value, in fp32
   (tok_attn_kernel: `bf16_to_f32(rel_bias[...]) * 1.4426...f` when the window is filled, then `fmaf(sc, c_scale, bb)` in the softmax
   block): the constant log2 e is itself a rounded fp32 number (<= u |bias| relative to the product), the product is rounded once
   (u |bias|), and the fused multiply-add rounds the sum once -- at most u |s_ij| <= u (|scale q . k| + |bias_ij|), of which model's
   4 u |s_ij| already holds the first part (its s now includes the bias) and the bias's share is charged here: c = 3 operations,
   e_ij += 3 u |bias_ij|.  temporal_attention_kernel adds the table value in natural units (`x += bf16_to_f32(rel_bias[...])`): one
   add, c = 1; __expf's product with log2 e acts on s_ij - m_i and sits in model's 4 u (|s_ij| + |m_i|).
2. P rounding.  The term (U + (Skv + d) u) sum_j P_j |v_j| charges U for P entering the P V MFMA in the element type.  The MFMA
   kernels keep U.  temporal_attention_kernel writes the normalised P to LDS as fp32 (`pl[wv][t1][t2b + r] = s[r] * inv`) and
   multiplies on the VALU in fp32 (`o[t1][j] += pw * vv[j]`): weight 0, leaving (T + d) u sum P |v| for the <= T fp32 FMAs, the
   division and the product with 1 / sum (4 + T <= 20 roundings against T + d >= 65).

Data.  `raised`: q = m + N(0, 1) for a fixed sign pattern m, k, v ~ N(0, 1); the first and the last key, the last key of every key
tile and the first of the next (32 keys on the wide heads, 64 on the narrow ones and the flash kernels) and the flash kernels' extra
key and last main key get + 8 m / (scale d): a score ~ 8 above the rest, so that each of them carries 1 / (number raised) of a row and
dropping, doubling or shifting one changes its weight by 1 / (number raised) -- up to 66 keys are raised, which with N(0, 1) values
alone is 3 to 9 bounds.  So the r-th raised key's v also gets + 64 in column r mod d: in that column the key holds nearly all of
out and of sum P |v|, and a relative change w of its weight is w / (2 U) bounds.  temporal: the sign of m alternates with the query
row t and every key carries + 4 m / (scale d), so that on odd rows all real keys sit 4 and the raised ones 12 BELOW a phantom key
of score 0 (the mutant that forgets t2 < T), which then takes most of the row.  The bias table is N(0, 1) per row and head, its two
extreme rows 3 and -2 (read only by the corner elements (Sq - 1, 0) and (0, Skv - 1) when max_len = Sq or Skv: a mutant that clips them
away moves a raised key's weight 20- or 7-fold), rounded to the element type.  Hard data (sweep J) comes from attn_edge_cases' builders."""
import collections
import functools
import math

import torch

import attn_edge_cases as E
import test_decoder_train_bounds_host as B

ELEM, LN2, LOG2E, u = E.ELEM, E.LN2, E.LOG2E, E.u
RAISE = 8.0
VMARK = 64.0                 # what the r-th raised key's v gets in column r mod d
EDGE_ROWS = (3.0, -2.0)      # the table's first and last row (unequal: i - j in place of j - i swaps them)
T_SHIFT = 4.0                # temporal: every key's common component along m
C_BIAS = {"tok": 3.0, "temporal": 1.0, "flash": 0.0}
TOK_STALE = 7.3              # TOKATTN_RESCALE_THR = 8 (csrc/tokattn.hip) and FLASH_RESCALE_THR = 8 (mode 1, csrc/attn.hip)
# mode 7: a row-sum piece of 16 probabilities above 2^64 (bf16; tools/gen_flash_dp2_asm.py THR_BITS = 0x5f800000) or 2^15 (half;
# tools/asm_elem_f16.py rewrites it to 0x47000000) sends the wave to the exact path: one probability stays below that
DP2_STALE = {"bf16": 59.7, "f16": 13.7}     # (no integers: a power of two would leave every rounding where it is)
# ... and 16 equal probabilities trip it at 2^(thr - 4) each: the `steps` data straddles that
DP2_STEP_THR = (("bf16", 60.0), ("f16", 11.0))

Case = collections.namedtuple("Case", "sweep kern nb Sq Skv H d max_len splits data edge tile extra N thr")


def tok_tile(d):
    return 32 if d >= 256 else 64      # tok_attn_kernel: BK


def case(sweep, kern, nb, Sq, Skv, H, d, max_len=None, splits=1, data="raised", edge=None, tile=None, extra=False, N=1, thr=8.0):
    if tile is None:
        tile = tok_tile(d) if kern == "tok" else 64
    return Case(sweep, kern, nb, Sq, Skv, H, d, max_len, splits, data, edge, tile, extra, N, thr)


def case_id(c):
    return "-".join(str(x).replace(" ", "").replace("'", "") for x in c)


# ----------------------------------------------------------------------------------------------------------- case tables
WIDE, NARROW = (256, 384, 512), (64, 128)
I_SKV = (33, 64, 65, 97, 129, 161, 193, 225, 257, 289, 321)   # (193, 225, 257: 7, 8 and 9 tiles of 32 keys -- see sweep_i)
L_LONG = (511, 512, 513, 577, 1024, 1025, 2049)
T_BNH = ((1, 1, 1), (2, 3, 3), (1, 5, 2))


def sweep_g():
    """key length: every Skv at Sq = 70 (one full, one partial query block), bias with max_len = max(Sq, Skv) exactly"""
    return [case("G", "tok", 2, 70, Skv, 2, d, max_len=max(70, Skv)) for d in WIDE + NARROW for Skv in range(1, 131 if d >= 256 else 201)]


def sweep_h():
    """query length: every Sq = 1 .. 130 at Skv = 70, bias with max_len = max(Sq, Skv) and once more with 512"""
    return [case("H", "tok", 2, Sq, 70, 2, d, max_len=L or max(Sq, 70)) for d in WIDE + NARROW for L in (0, 512) for Sq in range(1, 131)]


def sweep_i():
    """key splits: forced 1 .. 10 and 0 (the heuristic).  With the launcher's rule (tps = ceil(ntile / splits), ns = ceil(ntile / tps))
    the lengths {33, 64, 65, 97, 129, 161, 289, 321} reach ns in {1 .. 6, 10} only; 193, 225 and 257 (7, 8, 9 tiles of 32, the last of one
    key) add 7, 8 and 9: tok_attn_combine_ns_kernel<7 | 8> and the run-time merge at 9."""
    return [case("I", "tok", 2, Sq, Skv, 2, d, max_len=max(Sq, Skv) if bias else None, splits=sp)
            for d in (64, 256, 512) for Sq in (16, 70) for bias in (True, False) for Skv in I_SKV for sp in range(0, 11)]


def sweep_k():
    """bias table and window edges: Skv = 576 (639 of the 640 LDS slots) unsplit, by the heuristic and in 3 and 18 | 9 splits;
    Sq > Skv and Sq < Skv with max_len = max(Sq, Skv); three heads at d = 64 (the table's head column no power of two)"""
    out = [case("K", "tok", 2, Sq, 576, 2, d, max_len=576, splits=sp) for d in (64, 256, 512) for Sq in (1, 64, 65, 512)
           for sp in (1, 0, 3, 18)]
    for d in (64, 256, 384, 512):
        out += [case("K", "tok", 2, Sq, Skv, 2, d, max_len=max(Sq, Skv), splits=sp) for Sq, Skv in ((100, 37), (37, 100), (130, 129), (129, 130))
                for sp in (1, 2)]
    out += [case("K", "tok", 2, Sq, Skv, 3, 64, max_len=max(Sq, Skv), splits=sp) for Sq, Skv in ((70, 70), (37, 133), (133, 37)) for sp in (1, 2)]
    return out


def _pairs(pos):
    pos = sorted(set(pos))
    return [tuple(pos[i:i + 2]) if i + 1 < len(pos) else (pos[i], pos[0]) for i in range(0, len(pos), 2)]


def sweep_j():
    """hard softmax data (attn_edge_cases' builders) through the wide forms and the flash modes: S = 150 (five 32-key tiles, three
    64-key tiles, the last partial); `steps` at each kernel's tile and on both sides of its rescale threshold; `edge`: the dominating
    key at 0, tile - 1, tile, Skv - 2, Skv - 1 and on either side of every split boundary (three splits of two tiles: 63 | 64, 127 | 128)"""
    out, S = [], 150
    for d in WIDE:
        for sp in (1, 3):
            out += [case("J", "tok", 2, 70, S, 2, d, splits=sp, data=data) for data in ("rise", "first", "steps", "equal")]
            out += [case("J", "tok", 2, 70, S, 2, d, splits=sp, data="edge", edge=e) for e in _pairs((0, 31, 32, 63, 64, 127, 128, S - 2, S - 1))]
    for extra in (False, True):
        for thr in (8.0, DP2_STEP_THR):
            out += [case("J", "flash", 2, S, S, 2, 64, data=data, extra=extra, thr=thr) for data in ("rise", "first", "steps", "equal")]
        out += [case("J", "flash", 2, S, S, 2, 64, data="edge", edge=e, extra=extra) for e in _pairs((0, 63, 64, 127, 128, S - 3, S - 2, S - 1))]
    return out


def sweep_l():
    """ViT flash: every count of main rows 1 .. 330 (mode 1: 128-row units, mode 7: 256-row units, 64-key tiles) and the long ones,
    without and with the extra row"""
    return [case("L", "flash", 2, Sm + x, Sm + x, 2, 64, extra=bool(x)) for x in (0, 1) for Sm in list(range(1, 331)) + list(L_LONG)]


def sweep_t():
    """temporal: every T = 1 .. 16 at every head dim; (2, 3, 3) leaves two idle waves in the last block of four"""
    return [case("T", "temporal", Bn, T, T, H, d, max_len=L, N=N) for d in (64, 128, 256, 384, 512) for (Bn, N, H) in T_BNH
            for L in (None, 0, 512) for T in range(1, 17)]


SWEEPS = {"G": sweep_g, "H": sweep_h, "I": sweep_i, "K": sweep_k, "J": sweep_j, "L": sweep_l, "T": sweep_t}


@functools.lru_cache(maxsize=None)
def cases(sweep):
    out = tuple(SWEEPS[sweep]())
    if sweep == "T":   # (max_len 0 in the table above: exactly T)
        out = tuple(c._replace(max_len=c.Sq) if c.max_len == 0 else c for c in out)
    return out


def split_shape(c, ws_bytes=None):
    """(ns, tps) of a tok case by the launcher's rule (csrc/tokattn.hip: attn_shape, tok_attn_want_splits); ws_bytes None: a
    workspace that holds what is asked for"""
    ntile = -(-c.Skv // c.tile)
    per = c.nb * c.Sq * (c.H * c.d * 4 + c.H * 8)
    if c.splits > 0:
        ns = min(c.splits, ntile)
    else:
        base = c.nb * c.H * -(-c.Sq // 64)
        ns = 1 if base >= 192 or ntile < 4 else min(-(-256 // base), ntile // 2)
        if ws_bytes is not None:
            ns = max(min(ns, ws_bytes // per), 1)
    tps = -(-ntile // ns)
    return -(-ntile // tps), tps


def scale_of(c):
    return 0.125 if c.kern == "flash" else c.d ** -0.5


def n_main(c):
    return c.Skv - 1 if c.extra else c.Skv


def raised_keys(c):
    """the keys the `raised` data lifts"""
    Sm = n_main(c)
    pos = {0, Sm - 1, c.Skv - 1}
    if c.kern != "temporal":
        for t in range(c.tile, Sm, c.tile):
            pos |= {t - 1, t}
    return sorted(pos)


# ----------------------------------------------------------------------------------------------------------- data builders
_POOL_N = 1 << 23


@functools.lru_cache(maxsize=None)
def _pool():
    """N(0, 1) draws every case takes its tensors from (one generator call per process instead of three per case)"""
    return torch.randn(_POOL_N + (1 << 22), generator=B._gen(11))


def _draw(off, *shape):
    n = math.prod(shape)
    assert n <= 1 << 22
    off %= _POOL_N
    return _pool()[off:off + n].view(*shape).clone()


def _key(c):
    s = 0
    for x in (c.nb, c.Sq, c.Skv, c.H, c.d, c.N, int(c.extra), len(c.kern)):
        s = (s * 1000003 + int(x) * 7919 + 17) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=4)
def _operands(c, elem):
    dt = ELEM[elem][0]
    scale = scale_of(c)
    nbe = c.nb * c.N
    if c.data == "raised":
        k0 = _key(c)
        m = E._pattern(c.d)
        q = _draw(k0, nbe, c.H, c.Sq, c.d) + m
        k = _draw(k0 + 2796203, nbe, c.H, c.Skv, c.d)
        v = _draw(k0 + 5592407, nbe, c.H, c.Skv, c.d)
        if c.kern == "temporal":
            q = q - 2.0 * m * (torch.arange(c.Sq) % 2)[:, None]
        if c.kern == "temporal":
            k += T_SHIFT * m / (scale * c.d)
        rk = raised_keys(c)
        k[:, :, rk] += RAISE * m / (scale * c.d)
        for r, j in enumerate(rk):
            v[:, :, j, r % c.d] += VMARK
    else:   # attn_edge_cases' hard data: no mask, equal heads
        thr = dict(c.thr)[elem] if isinstance(c.thr, tuple) else c.thr
        ec = E.case("", "", nbe, c.Sq, c.Skv, c.H, c.H, c.d, causal=False, data=c.data, edge=c.edge, tile=c.tile)._replace(thr=thr)
        assert scale == c.d ** -0.5
        q, k, v = E.split_heads(ec, E.operands(ec, elem))
    tbl = None
    if c.max_len:
        tbl = _draw(_key(c) + 8388617 + c.max_len, 2 * c.max_len - 1, c.H)
        tbl[0], tbl[-1] = EDGE_ROWS
        tbl = tbl.to(dt)
    return dict(q=q.to(dt), k=k.to(dt), v=v.to(dt), table=tbl, scale=scale)


def operands(c, elem):
    """the inputs of a case in head form, in the element type (sweep, splits and thr of another build are not part of the key)"""
    return _operands(c._replace(sweep="", splits=1, max_len=c.max_len or 0), elem)


def prescaled(o, elem):
    """what the ViT's q|k|v product leaves in the q columns: q * scale * log2 e, rounded once; the kernel computes exp2(q' . k), i.e. the
    same attention at scale ln 2"""
    return dict(o, q=(o["q"].float() * (o["scale"] * LOG2E)).to(ELEM[elem][0]), scale=LN2)


# ---------------------------------------------------------------------------------------------------- bias, bound, emulation
def bias_matrix(table, Sq, Skv, max_len, shift=0, flip=False, kbeg=None):
    """(1, H, Sq, Skv) float64: table[j - i + max_len - 1 (+ shift) (+ kbeg[j])][h], a row outside the table reads as 0 (the kernel's
    clipping); flip: i - j.  `table` (2 max_len - 1, H)."""
    i = torch.arange(Sq, device=table.device)[:, None]
    j = torch.arange(Skv, device=table.device)[None, :]
    row = (i - j if flip else j - i) + max_len - 1 + shift
    if kbeg is not None:
        row = row + kbeg.to(table.device)[None, :]
    ok = (row >= 0) & (row < 2 * max_len - 1)
    b = table.double()[row.clamp(0, 2 * max_len - 2)] * ok[..., None]
    return b.permute(2, 0, 1)[None]


def heads64(o, device=None):
    return tuple(o[n].to(device).double() for n in "qkv")


def reference(c, o, elem, device=None):
    """float64 out (nbe, H, Sq, d), its per-element bound and lse (nbe, H, Sq; natural log) on `device`"""
    _, U, tiny = ELEM[elem]
    q, k, v = heads64(o, device)
    bias = None if o["table"] is None else bias_matrix(o["table"].to(device), c.Sq, c.Skv, c.max_len)
    vis = torch.ones(1, c.Sq, c.Skv, dtype=torch.bool, device=device)
    kw = dict(bias=bias, c_bias=C_BIAS[c.kern], pw=0.0 if c.kern == "temporal" else U)
    step = 1 if c.Sq * c.Skv > 1 << 19 else q.shape[0]       # (a long sequence: one batch entry at a time)
    parts = [E.model(q[b:b + step], k[b:b + step], v[b:b + step], o["scale"], vis, U, tiny, **kw) for b in range(0, q.shape[0], step)]
    return {n: torch.cat([p[n] for p in parts]) for n in ("out", "bound", "lse")}


def emulate(c, o, elem, stale=0.0, q=None, k=None, v=None, bias="own", vis=None):
    """the kernels' rounding points on the case (attn_edge_cases.emulate; temporal keeps P unrounded); q / k / v / bias / vis: a mutant's"""
    q0, k0, v0 = heads64(o)
    q, k, v = (q0 if q is None else q), (k0 if k is None else k), (v0 if v is None else v)
    if isinstance(bias, str):
        bias = None if o["table"] is None else bias_matrix(o["table"], c.Sq, c.Skv, c.max_len)
    if vis is None:
        vis = torch.ones(1, q.shape[2], k.shape[2], dtype=torch.bool)
    return E.emulate(q, k, v, o["scale"], vis, ELEM[elem][0], stale, bias=bias, round_p=c.kern != "temporal")


def stales(c, elem):
    """the stale-max distances (log2 units) a case's kernels can run at"""
    if c.kern == "temporal":
        return (0.0,)
    return (0.0, TOK_STALE) + ((DP2_STALE[elem],) if c.kern == "flash" else ())


# --------------------------------------------------------------------------------------------------------------- mutants
# mutant(c, o) -> keyword arguments of emulate() that restate the fault, or None where the case cannot show it
def _hide(c, cols):
    vis = torch.ones(1, c.Sq, c.Skv, dtype=torch.bool)
    vis[..., cols] = False
    return dict(vis=vis)


def _bias(c, o, **kw):
    if o["table"] is None or c.Skv == 1:     # (one key: the softmax does not see its score)
        return None
    return dict(bias=bias_matrix(o["table"], c.Sq, c.Skv, c.max_len, **kw))


def _kbeg(c):
    """first key of the split each key belongs to"""
    ns, tps = split_shape(c)
    return None if ns < 2 else (torch.arange(c.Skv) // (tps * c.tile)) * (tps * c.tile)


def m_row_plus(c, o):
    return _bias(c, o, shift=1)


def m_row_minus(c, o):
    return _bias(c, o, shift=-1)


def m_flip(c, o):
    return _bias(c, o, flip=True) if c.Sq > 1 or c.Skv > 1 else None


def m_next_head(c, o):
    return None if o["table"] is None or c.H < 2 or c.Skv == 1 else dict(bias=bias_matrix(o["table"].roll(1, 1), c.Sq, c.Skv, c.max_len))


def m_no_log2e(c, o):
    b = _bias(c, o)
    return b and dict(bias=b["bias"] * LN2)


def m_log2e_twice(c, o):
    b = _bias(c, o)
    return b and dict(bias=b["bias"] * LOG2E)


def m_no_bias(c, o):
    return None if o["table"] is None or c.Skv == 1 else dict(bias=None)


def m_no_kbeg(c, o):
    kb = _kbeg(c) if c.kern == "tok" else None
    return None if kb is None else _bias(c, o, kbeg=kb)


def m_extreme_rows(c, o):
    if o["table"] is None or c.Skv == 1 or c.max_len > max(c.Sq, c.Skv):
        return None
    t = o["table"].clone()
    t[0] = t[-1] = 0
    return dict(bias=bias_matrix(t, c.Sq, c.Skv, c.max_len))


def m_last_key(c, o):
    return _hide(c, [c.Skv - 1]) if c.Skv > 1 else None


def m_first_key(c, o):
    return _hide(c, [0]) if c.Skv > 1 else None


def m_last_twice(c, o):
    if c.Skv == 1:       # (the only key twice is the same row)
        return None
    q, k, v = heads64(o)
    out = dict(k=torch.cat([k, k[:, :, -1:]], 2), v=torch.cat([v, v[:, :, -1:]], 2))
    if o["table"] is not None:
        b = bias_matrix(o["table"], c.Sq, c.Skv, c.max_len)
        out["bias"] = torch.cat([b, b[..., -1:]], -1)
    return out


def m_tile_first(c, o):
    Sm = n_main(c)
    return _hide(c, [(Sm - 1) // c.tile * c.tile]) if Sm > c.tile else None


def m_tile_last(c, o):
    return _hide(c, [c.tile - 1]) if n_main(c) > c.tile else None


def m_split_first(c, o):
    kb = _kbeg(c) if c.kern == "tok" else None
    return None if kb is None else _hide(c, [int(kb[-1])])


def m_extra_key_dropped(c, o):
    return _hide(c, [c.Skv - 1]) if c.extra else None


def m_extra_key_twice(c, o):
    return m_last_twice(c, o) if c.extra else None


def m_extra_query(c, o):
    if not c.extra or c.Sq < 2:
        return None
    q = heads64(o)[0].clone()
    q[:, :, -1] = q[:, :, -2]
    return dict(q=q)


def m_phantom_key(c, o):
    if c.Skv >= 16 or c.Sq == 1:      # (the 16 x 16 tile has no row T; a lone even row sees its raised key 12 above the phantom)
        return None
    q, k, v = heads64(o)
    out = dict(k=torch.cat([k, torch.zeros_like(k[:, :, :1])], 2), v=torch.cat([v, torch.zeros_like(v[:, :, :1])], 2))
    if o["table"] is not None:
        b = bias_matrix(o["table"], c.Sq, c.Skv, c.max_len)
        out["bias"] = torch.cat([b, torch.zeros_like(b[..., :1])], -1)
    return out


def temporal_rows(x, c):
    """head form (B N, H, T, d) -> the kernel's rows (B T N, H d)"""
    return x.reshape(c.nb, c.N, c.H, c.Sq, c.d).permute(0, 3, 1, 2, 4).reshape(c.nb * c.Sq * c.N, c.H * c.d)


def temporal_heads(rows, c):
    return rows.reshape(c.nb, c.Sq, c.N, c.H, c.d).permute(0, 2, 3, 1, 4).reshape(c.nb * c.N, c.H, c.Sq, c.d)


def m_swap_n_t(c, o):
    """rows read as (b n t): the same storage under the other order (the output is written back through it as well, which the
    emulation leaves out: the inputs alone are wrong enough)"""
    if c.N < 2 or c.Sq < 2:
        return None

    def swap(x):
        return temporal_rows(x, c).reshape(c.nb, c.N, c.Sq, c.H, c.d).permute(0, 1, 3, 2, 4).reshape(c.nb * c.N, c.H, c.Sq, c.d)
    q, k, v = heads64(o)
    return dict(q=swap(q), k=swap(k), v=swap(v))


# (name, sweeps it belongs to, mutation)
MUTANTS = [("bias row index + 1", "GHKT", m_row_plus), ("bias row index - 1", "GHKT", m_row_minus), ("i - j in place of j - i", "GHKT", m_flip),
           ("the neighbouring head's bias column", "GHKT", m_next_head), ("bias not multiplied by log2 e", "GHK", m_no_log2e),
           ("bias multiplied by log2 e twice", "GHK", m_log2e_twice), ("bias dropped", "GHIKT", m_no_bias),
           ("a split's kbeg left out of the slot index", "IK", m_no_kbeg), ("the two extreme table rows read as 0", "GHK", m_extreme_rows),
           ("last key dropped", "GHIKLT", m_last_key), ("first key dropped", "GHIKLT", m_first_key),
           ("last key counted twice", "GHIKL", m_last_twice), ("first key of a tile dropped", "GHIKL", m_tile_first),
           ("last key of a tile dropped", "GHIKL", m_tile_last), ("first key of a split dropped", "IK", m_split_first),
           ("flash: extra key dropped", "L", m_extra_key_dropped), ("flash: extra key counted twice", "L", m_extra_key_twice),
           ("flash: the extra query row reads the last main row's q", "L", m_extra_query),
           ("temporal: a phantom key T with score 0", "T", m_phantom_key), ("temporal: n and t swapped in the row order", "T", m_swap_n_t)]
