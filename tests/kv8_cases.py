"""The FP8 (e4m3) KV cache, shared by tests/test_kv8_host.py (CPU) and tests/test_gpu_kv8.py (the kernels): the decode attention's
LDS image and operand maps (csrc/decode_attn.hip: decode_attn_kv8_kernel), the case tables, the quantised operands, the float64
bound and the CPU emulation of the kernel's rounding points.

The bound is attn_edge_cases.model on the DEQUANTISED float64 K / V (code x scale is the definition the kernels and the tests
share) plus three named terms:
  ks   s_j = ks[j] * sum_d q_d code(K_jd): one more fp32 rounding of the score, u |s_ij| on top of model's e_ij;
  vs   the P operand is rnd_elem(fl32(p_j vs[j])): the fp32 product costs one more u on the P term, u sum_j P_j |v_j|;
  sub  (IEEE half) rnd_f16 of p_j vs[j] PRE below 2^-14 is off by up to 2^-25 absolutely, in units of |code_j|: the output moves by
       at most 2^-25 / PRE * sum_j |code(V_j)| / l_i (the kernel's row sum is >= l_i >= 1, as in model's `tiny` term, which this one
       replaces: the probability itself is never rounded to half).  PRE = 2^8 is the kernel's pre-scale on P.
and one that the format of the accumulation brings with it, whatever the cache holds:
  f32  fp32 has no normal number below 2^-126: v_exp_f32 flushes a p_j below it to zero and the product p_j vs[j] PRE is flushed
       or rounded absolutely there, each off by at most 2^-126: the output moves by at most 2^-126 sum_j (|v_j| + |code(V_j)| / PRE
       + |out|) / l_i.  About 1e-35 on N(0, 1) data -- it matters only where the output itself is that small: a quantised row holds
       exact ZERO codes (|x| < 2^-10 scale), so an element whose dominating key has a zero code is the sum of the other keys'
       terms alone, which with the amax spread of the "normal" data are 90 natural-log units down (model's own terms are all
       relative to P_j |v_j| and give a bound of 1e-41 there).
  out  (IEEE half) the stored output has no finer grid than half's subnormals: below 2^-14 it is rounded absolutely, off by up to
       2^-25, where model's U |out| is smaller.  With the amax spread a V row of amax 2^-6 has elements of 1e-5, and a sequence
       that sees one key returns that row.  Rows that see no key keep a bound of 0: they must be exact zeros.
"""
import functools

import torch

import attn_edge_cases as A
import test_decoder_train_bounds_host as B

DS = (64, 96, 128)
BK = 64                      # keys per tile
PRE = {"bf16": 1.0, "f16": 256.0}
F16_SUB = 2.0 ** -25         # half the spacing of IEEE half's subnormals
F32_MIN = 2.0 ** -126        # the smallest normal fp32


# ------------------------------------------------------------------------------------------------ LDS image and operand maps
def swz(D, row):
    """the XOR on a row's 16-byte chunk index (da8_swz)"""
    if D == 128:
        return (((row >> 1) & 3) << 1) | ((row >> 3) & 1)
    if D == 64:
        return (((row >> 2) & 1) << 1) | ((row >> 3) & 1)
    return (row >> 3) & 1


def tile_off(D, row, byte):
    """byte offset inside a tile's LDS image of byte `byte` (= d) of key row `row`"""
    return row * D + (((byte >> 4) ^ swz(D, row)) << 4) + (byte & 15)


def dma_source(D, piece, lane):
    """(row, first byte) the LDS-DMA piece `piece` of `lane` fetches: its destination is the lane-linear chunk piece * 64 + lane"""
    c = piece * 64 + lane
    row, cp = divmod(c, D // 16)
    return row, (cp ^ swz(D, row)) << 4


def k_read(D, kb, ks, lane):
    """ds_read_b64 of the K fragment: -> (LDS byte offset, key row, first d) of the lane's 8 codes"""
    l15, g = lane & 15, lane >> 4
    row, d0 = 16 * kb + l15, 32 * ks + 8 * g
    return tile_off(D, row, d0), row, d0


def v_read(D, blk, r16, lane):
    """ds_read_b64_tr_b16 number r16 (rows + 16 r16) of d block blk: -> (LDS byte offset the lane SUPPLIES, key row, first d of its 8 bytes)"""
    l15, g = lane & 15, lane >> 4
    row, d0 = 16 * r16 + 4 * g + (l15 >> 2), 32 * blk + 8 * (l15 & 3)
    return tile_off(D, row, d0), row, d0


def v_received(D, blk, r16, lane):
    """what the transposed read hands the lane (T10: lane i of a 16-lane group receives 16-bit column i of the group's 4 rows, row q in
    element q; the group's lane 4 q + p supplies row q, columns 4 p .. 4 p + 3): -> [(key, d of the low byte)] of its 4 elements"""
    i, g = lane & 15, lane >> 4
    out = []
    for q in range(4):
        src = 16 * g + 4 * q + (i >> 2)                     # the lane whose 8 bytes hold column i
        _, row, d0 = v_read(D, blk, r16, src)
        out.append((row, d0 + 2 * (i & 3)))
    return out


def p_slot_key(hh, g, e):
    """key (inside the tile) of k-slot (g, e) of the P fragment of 32-key half hh"""
    return 32 * hh + 16 * (e >> 2) + 4 * g + (e & 3)


def o_row_d(blk, odd, g, r):
    """d of accumulator element r of lane group g of the even / odd MFMA of d block blk: what the store writes where"""
    return 32 * blk + 2 * (4 * g + r) + odd


def bank_ways(addresses):
    """worst number of distinct dwords on one of the 64 banks among the 8-byte reads of one 32-lane half"""
    banks = {}
    for a in addresses:
        for w in (a // 4, a // 4 + 1):
            banks.setdefault(w % 64, set()).add(w)
    return max(len(v) for v in banks.values())


# ----------------------------------------------------------------------------------------------------------- case tables
LENGTHS = tuple(range(1, 131)) + tuple(range(133, 301, 3)) + A.LONG_T
HOST_LENGTHS = (1, 2, 31, 63, 64, 65, 127, 128, 129, 130, 300, 1025)


def attn_case(T, data):
    """8 sequences whose first visible key lies at 0, 1, 31, 32, 33, T // 2, T - 1 and T (none visible), spare capacity on odd T (and
    one position for the "edge" data, whose dominating key sits on a mask edge: at the first visible key of the even sequences, one
    below it -- masked -- for the odd ones)"""
    g, d = A.decode_gd(T)
    start = tuple(min(max(s, 0), T) for s in (0, 1, 31, 32, 33, T // 2, T - 1, T))
    spare = 7 if T % 2 else int(data == "edge")
    edge = tuple(min(max(s - (b & 1), 0), T - 1 + min(spare, 1)) for b, s in enumerate(start)) if data == "edge" else None
    return A.case("K8", "decode", 8, 1, T, 2 * g, 2, d, kv_start=start, spare=spare, data=data, edge=edge, tile=BK)


@functools.lru_cache(maxsize=None)
def operands(c, elem):
    """attn_edge_cases' operands of the case -- "normal": every key's K row and V row scaled by its own 2^e, e in -6 .. 6 --, every
    position of the buffers quantised (masked keys and spare capacity too): q, K8 / V8 (codes), ks / vs, scale"""
    o = A.operands(c, elem)
    K, V = o["K"], o["V"]
    if c.data == "normal":
        g = B._gen(8, c.Skv, c.d)
        ek = torch.randint(-6, 7, K.shape[:3], generator=g).float()
        ev = torch.randint(-6, 7, V.shape[:3], generator=g).float()
        K, V = (K.float() * torch.exp2(ek)[..., None]).to(K.dtype), (V.float() * torch.exp2(ev)[..., None]).to(V.dtype)
    from u2tokenizer_amd import ops
    K8, ks = ops.quantize_kv_fp8(K)
    V8, vs = ops.quantize_kv_fp8(V)
    return dict(q=o["q"], K=K, V=V, K8=K8, V8=V8, ks=ks, vs=vs, scale=o["scale"])


def split(c, o, device=None):
    """float64: q (nb, Hq, 1, d), the codes of K and V (nb, Hkv, T, d) and their scales (nb, Hkv, T)"""
    q = o["q"].to(device).double().view(c.nb, c.Sq, c.Hq, c.d).permute(0, 2, 1, 3)
    return (q,) + tuple(o[n][:, :, :c.Skv].to(device).double() for n in ("K8", "V8", "ks", "vs"))


# ------------------------------------------------------------------------------------------------------------ bound, emulation
def model(q, kc, vc, ks, vs, scale, vis, elem):
    """out and its per-element bound (module docstring) for float64 codes and scales"""
    _, U, _ = A.ELEM[elem]
    k, v = kc * ks[..., None], vc * vs[..., None]
    m = A.model(q, k, v, scale, vis, U, 0.0)
    G = q.shape[1] // k.shape[1]
    P, out = m["P"], m["out"]
    va = v.abs().repeat_interleave(G, 1)
    Pe = P * (A.u * m["s"].masked_fill(~vis[:, None], 0.0).abs())
    bound = m["bound"] + Pe @ va + Pe.sum(-1, keepdim=True) * out.abs() + A.u * (P @ va)
    s, mx, _ = A._scores(q, k, scale, vis)
    l = torch.exp(s - mx).sum(-1, keepdim=True).clamp_min(1.0)
    seen = vis[:, None].to(torch.float64).expand(-1, q.shape[1], -1, -1)
    ca = vc.abs().repeat_interleave(G, 1)
    bound = bound + F32_MIN * (seen @ (va + ca / PRE[elem]) + seen.sum(-1, keepdim=True) * out.abs()) / l
    if elem == "f16":
        bound = bound + (F16_SUB / PRE[elem]) * (seen @ ca) / l + F16_SUB * seen.amax(-1, keepdim=True)
    return dict(out=out, bound=bound)


def emulate(q, kc, vc, ks, vs, scale, vis, elem, mutant=None):
    """the kernel's rounding points: the code dot product and its product with ks in fp32, p = exp(s - m), the row sum of the
    unrounded p, the P operand rnd_elem(fl32(p vs PRE)) against the codes of V, one output rounding.  mutant: "shift" reads every
    scale one key late, "swap" exchanges the K and the V scales."""
    dt = A.ELEM[elem][0]

    def f32(t):
        return t.float().double()

    def rnd(t):
        return t.float().to(dt).double()
    if mutant == "shift":
        ks, vs = ks.roll(1, -1), vs.roll(1, -1)
    elif mutant == "swap":
        ks, vs = vs, ks
    G = q.shape[1] // kc.shape[1]
    dot = f32(q @ kc.repeat_interleave(G, 1).transpose(-1, -2))
    s = f32(dot * ks.repeat_interleave(G, 1)[:, :, None, :]) * scale
    s = s.masked_fill(~vis[:, None], float("-inf"))
    mx = s.max(-1, keepdim=True).values
    mx = torch.where(mx == float("-inf"), torch.zeros_like(mx), mx)
    p = torch.exp(s - mx)
    l = p.sum(-1, keepdim=True)
    P = rnd(f32(p * (vs * PRE[elem]).repeat_interleave(G, 1)[:, :, None, :]))
    o = P @ vc.repeat_interleave(G, 1)
    return rnd(torch.where(l > 0, o / l.clamp_min(1e-300) / PRE[elem], torch.zeros_like(o)))
