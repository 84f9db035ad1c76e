"""CPU: the LDS layout of the head-dim-384 attention tiles (tokattn.hip: tok_attn_kernel<384>, the tokenizer's own attention
at E = 3072), restated in Python (no GPU needed).

A tile is 32 keys x 768 bytes: 48 chunks of 16 bytes per row = three whole 16-chunk segments.  It is filled by LDS-DMA
(64 consecutive chunks per wave instruction, six pieces per thread, the permutation on the SOURCE chunk) and read as
ds_read_b128 K fragments (lane (l15, g) of 16-key block kb and k step ks: chunk 4 ks + g of row 16 kb + l15) and
ds_read_b64_tr_b16 V^T fragments (tests/test_lds_layouts.py: tr_read).  The swizzles are those of d = 256 / 512 -- the K
tile XORs the chunk index with row & 15, the V tile rotates the chunks of each segment by 2 (key & 3) + 8 ((key >> 2) & 1)
-- and both only touch the low four bits of the chunk index, so a chunk stays inside its segment and its row although 48
is no power of two; the 768-byte row pitch is a multiple of the 256-byte bank period, so a lane group's rows differ only
by what the swizzle adds.
"""
from test_lds_layouts import slots_of, tr_read
from test_phi3_decoder_host import B128_GROUPS   # ds_read_b128 lane groups (one LDS cycle each)

DH, BK, CPR, ROWB, SEG = 384, 32, 48, 768, 16
NP, KS, DB = BK * CPR // 256, DH // 32, DH // 16


def test_the_template_constants():
    assert (NP, KS, DB, BK * ROWB) == (6, 12, 24, 24 * 1024)
    assert CPR % SEG == 0 and ROWB % 256 == 0 and CPR & (CPR - 1)       # whole segments, whole bank periods, no power of two
    assert 4 * BK * ROWB + 640 * 4 <= 160 * 1024 < 2 * (4 * BK * ROWB)   # two stages of K and V + the bias window: one workgroup per CU


def tv_rot(k):
    return 2 * (k & 3) + 8 * ((k >> 2) & 1)


def k_src(row, cp):
    return cp ^ (row & (SEG - 1))


def v_src(row, cp):
    return (cp & ~(SEG - 1)) | (((cp & (SEG - 1)) - tv_rot(row)) & (SEG - 1))


def dma_image(src):
    """LDS chunk c -> (tile row, logical chunk) as dma_k / dma_v leave it: piece i of thread (w, lane) is chunk
    c = 256 i + 64 w + lane = (row c / 48, position c % 48) and reads the source chunk src(row, position)"""
    img = {}
    for i in range(NP):
        for w in range(4):
            for lane in range(64):
                c = i * 256 + w * 64 + lane
                row, cp = c // CPR, c % CPR
                img[c] = (row, src(row, cp))
    return img


def test_dma_source_permutation_is_a_bijection_that_stays_inside_the_row():
    for src in (k_src, v_src):
        img = dma_image(src)
        assert len(img) == BK * CPR == 32 * 48
        assert all(0 <= L < CPR for _, L in img.values())                                   # inside the row ...
        assert all(L // SEG == (c % CPR) // SEG for c, (_, L) in img.items())               # ... and inside its segment
        assert sorted(img.values()) == [(r, L) for r in range(BK) for L in range(CPR)]      # every chunk of the tile once
    # a swizzle over the whole row, as the one-segment widths may read it (& (CPR - 1) with CPR = 48), would not be one
    assert len({(cp + 5) & (CPR - 1) for cp in range(CPR)}) < CPR


def k_addr(kb, ks, lane):
    l15, g = lane & 15, lane >> 4
    return kb * 16 * ROWB + l15 * ROWB + (((ks * 4 + g) ^ (l15 & (SEG - 1))) << 4)


def test_k_fragments_receive_their_keys_and_chunks():
    img = dma_image(k_src)
    for kb in range(BK // 16):
        for ks in range(KS):
            for lane in range(64):
                a = k_addr(kb, ks, lane)
                assert a % 16 == 0 and a < BK * ROWB
                assert img[a // 16] == (16 * kb + (lane & 15), 4 * ks + (lane >> 4)), (kb, ks, lane)


def test_k_fragment_reads_are_conflict_free():
    groups = B128_GROUPS + [list(range(16 * g, 16 * g + 16)) for g in range(4)]   # the hardware's groups and the plain 16-lane ones
    for kb in range(BK // 16):
        for ks in range(KS):
            for grp in groups:
                slots = [(k_addr(kb, ks, l) % 256) // 16 for l in grp]
                assert len(set(slots)) == 16, (kb, ks, grp, slots)


def test_unswizzled_768_byte_rows_would_conflict_sixteen_ways():
    """what the XOR is for: the row pitch is a whole number of bank periods, so one logical chunk of 16 rows is ONE slot"""
    assert len({(row * ROWB + 16 * 5) % 256 // 16 for row in range(16)}) == 1


def v_addrs(db, second):
    """lane -> byte address of the transpose read of d block db (second: the +16 key rows); one P fragment per tile"""
    out = []
    for lane in range(64):
        l15, g = lane & 15, lane >> 4
        v_row = 4 * g + (l15 >> 2)
        cc = 2 * db + ((l15 & 3) >> 1)
        cp = (cc & ~(SEG - 1)) | (((cc & (SEG - 1)) + tv_rot(v_row)) & (SEG - 1))
        out.append(v_row * ROWB + (l15 & 1) * 8 + cp * 16 + (16 * ROWB if second else 0))
    return out


def test_v_transpose_reads_receive_their_rows_and_columns():
    img = dma_image(v_src)
    lds = {}
    for c, (row, L) in img.items():
        for e in range(8):
            lds[16 * c + 2 * e] = (row, 8 * L + e)   # element value = (key row, column)
    for db in range(DB):
        for second in (False, True):
            a = v_addrs(db, second)
            assert max(a) + 8 <= BK * ROWB
            got = tr_read(a, lds)
            for lane in range(64):
                l15, g = lane & 15, lane >> 4
                want = [(16 * second + 4 * g + r, 16 * db + l15) for r in range(4)]
                assert got[lane] == want, (db, second, lane)


def test_v_transpose_reads_are_conflict_free():
    for db in range(DB):
        for second in (False, True):
            a = v_addrs(db, second)
            for half in (a[:32], a[32:]):   # ds_read_b64_tr_b16: 2 x 32 lanes, 8 bytes each -> 64 banks
                assert len({(x % 256) // 8 for x in half}) == 32, (db, second)
                assert len(set(slots_of(half))) == 16
            for g in range(4):              # a 16-lane group: [4 keys][16 d], two lanes per 16-byte slot
                assert len(set(slots_of(a[16 * g:16 * g + 16]))) == 8, (db, second, g)


def test_key_split_partials_are_float4_aligned_per_head():
    """tok_attn_combine*: one thread merges 4 consecutive columns of E = H * 384; a float4 never straddles two heads"""
    for H in (1, 2, 8):
        E = H * DH
        assert E % 4 == 0 and DH % 4 == 0
        assert all((e // DH) == ((e + 3) // DH) for e in range(0, E, 4))
