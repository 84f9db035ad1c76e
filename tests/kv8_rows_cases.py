"""The rows form of the attention over an e4m3 KV cache (csrc/decode_attn.hip: decode_attn_kv8_kernel<D, true> behind
u2tok_attention_kv8_rows), shared by tests/test_kv8_rows_host.py (CPU) and tests/test_gpu_kv8_rows.py (the kernel): the row map and
the per-block tile range restated in Python, and the case table.

The bound is tests/kv8_cases.py's `model` on attn_edge_cases.case_visible(c), unchanged: it already takes Sq > 1, a window and
kv_start, and the rows form has the rounding points of the decode form (`K8.emulate`) -- the same score, probability, P operand and
output roundings per (row, key); only which keys a row sees differs.  No term is added.

Row map: a kv head's Sq G query rows (G = Hq / Hkv) are numbered f = i G + gh -- i the new position, gh the query head inside the
group -- and cut into blocks of 16; G need not divide 16.  With c = T - Sq row f sees key j iff kv_start[b] <= j <= i + c and, for a
window W > 0, j > i + c - W.  A block walks the 64-key tiles from the one holding its first row's lowest key to the one holding its
last row's diagonal, none when kv_start lies beyond that diagonal; inside a key split, the part of that range the split covers."""
import functools

import attn_edge_cases as A
import kv8_cases as K8

BK = K8.BK
ROWS = 16


# ------------------------------------------------------------------------------------------------------------------- row map
def row_blocks(G, Sq):
    """-> per block the (position, head in group) of its live rows, in operand row order; the last block's other rows are dead"""
    flat = [(f // G, f % G) for f in range(Sq * G)]
    return [flat[o:o + ROWS] for o in range(0, len(flat), ROWS)]


def row_keys(i, Sq, T, W, kvs):
    """(first, last) key row `i` sees (first > last: none)"""
    c = T - Sq
    kvs = max(0, min(kvs, T))
    return (max(kvs, i + c - W + 1) if W else kvs), i + c


def block_tiles(block, Sq, T, W, kvs):
    """-> (first tile, end tile, masked): the tiles [first, end) the block walks and, per such tile, whether it takes the masked
    path -- the kernel's wave-uniform expressions on the block's first and last live row"""
    i0, i1 = block[0][0], block[-1][0]
    lo0, hi0 = row_keys(i0, Sq, T, W, kvs)
    lo1, hi1 = row_keys(i1, Sq, T, W, kvs)
    first = lo0 // BK
    end = first if lo0 > hi1 else hi1 // BK + 1
    masked = {kt: kt * BK < lo1 or kt * BK + BK - 1 > hi0 for kt in range(first, end)}
    return first, end, masked


def asked_splits(B, Sq, Hq, Hkv, T):
    """dec_attn_splits on B x row blocks (enough workgroups for 256 CUs, a 32-key tile per wave of a split), at most one per 64-key tile"""
    nrb = -(-Sq * (Hq // Hkv) // ROWS)
    nt32 = -(-T // 32)
    ns = 1 if nt32 < 8 else max(1, min(-(-256 // (B * nrb * Hkv)), nt32 // 4))
    return min(ns, -(-T // BK))


def splits(B, Sq, Hq, Hkv, T):
    """-> (splits launched, 64-key tiles per split): no split beyond the last tile"""
    ntile = -(-T // BK)
    tps = -(-ntile // asked_splits(B, Sq, Hq, Hkv, T))
    return -(-ntile // tps), tps


def workspace_bytes(B, Sq, Hq, Hkv, T, D):
    ns = asked_splits(B, Sq, Hq, Hkv, T)
    return ns * B * Sq * Hq * (4 * D + 8) if ns > 1 else 0


# ----------------------------------------------------------------------------------------------------------- case tables
NB, HKV = 3, 2
C_OFFS = (1, 31, 63, 64, 65, 100)
SQS = (2, 5, 16, 17, 33)
PAIRS = tuple((g, d) for g in A.GS for d in A.DS)


def _case(n, Sq, T, W, data, edge=None, spare=None):
    g, d = PAIRS[n % len(PAIRS)]
    start = (0, min(33, T - 1), T)       # the last sequence sees nothing: exact zeros
    spare = (5 if n % 2 else 0) if spare is None else spare
    return A.case("K8R", "rows", NB, Sq, T, HKV * g, HKV, d, window=W, kv_start=start, spare=spare, data=data, edge=edge, tile=BK)


@functools.lru_cache(maxsize=None)
def sweep(data):
    """c_off cached positions x Sq new ones x the windows {none, 1, 17, 64, c_off + 1}, G and d rotating through A.GS x A.DS, spare
    capacity on every other case"""
    out, n = [], 0
    for c_off in C_OFFS:
        for Sq in SQS:
            for W in sorted({0, 1, 17, 64, c_off + 1}):
                out.append(_case(n, Sq, Sq + c_off, W or None, data))
                n += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def long_cases():
    """the split path: T in A.LONG_T, one and seven new positions, no window and one that ends inside the cache"""
    out = []
    for n, T in enumerate(A.LONG_T):
        out.append(_case(2 * n, 1, T, None, "normal"))
        out.append(_case(2 * n + 1, 7, T, 700 if n % 2 else None, "normal"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_cases():
    """the dominating key (score + 30, v = +-8) on row 1's diagonal (row 0 must not see it), on the last row's window edge (its lowest
    visible key: one row further down would not see it, and every row above does or does not by its own edge) and at kv_start
    (per sequence; the last sequence's lies in the spare position T: nobody sees it) -- on 8 shapes"""
    shapes = ((1, 2, 1), (31, 5, 17), (63, 16, 64), (64, 17, 17), (65, 33, 64), (100, 33, 101), (100, 5, 17), (31, 17, 32))
    out = []
    for n, (c_off, Sq, W) in enumerate(shapes):
        T = Sq + c_off
        start = (0, min(33, T - 1), T)
        for where in ((1 + c_off,) * NB, (max(0, Sq - 1 + c_off - W + 1),) * NB, start):
            out.append(_case(n, Sq, T, W, "edge", edge=where, spare=1))
    return tuple(out)


def gpu_operands(c, o, device):
    """q (nb, Sq, Hq d), the code and scale buffers at their full capacity, kv_start"""
    import torch
    kc, vc = (o[n].view(torch.uint8).to(device).contiguous() for n in ("K8", "V8"))
    return (o["q"].to(device), kc, vc, o["ks"].to(device).contiguous(), o["vs"].to(device).contiguous(),
            torch.tensor(c.kv_start, dtype=torch.int32, device=device))
