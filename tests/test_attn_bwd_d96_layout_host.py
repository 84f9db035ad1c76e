"""CPU: executable statement of the LDS placement of csrc/attn_bwd.hip's head-dim-96 tiles (tile_off<96>; no GPU needed), next to
tests/test_lds_layouts.py, whose model of ds_read_b64_tr_b16 and of the 16-byte slots of the 256-byte bank row it uses.

A [64][96] bf16 tile has rows of 192 bytes = 12 chunks of 16 bytes.  Row r starts 12 r slots into the bank rows, so chunk c of row
r lies in slot 4 ((c >> 2) - r mod 4) + (c & 3): the group of four chunks picks the 64-byte quarter, and rows r, r + 4, r + 8,
r + 12 meet.  The placement XORs the chunk's low two bits with (row >> 2) & 3 -- it stays inside each group of four chunks --:

    tile_off<96>(row, chunk) = row * 192 + (chunk & ~3) * 16 + (((chunk & 3) ^ ((row >> 2) & 3)) * 16)

Checked here, with the kernels' index arithmetic restated in Python:
  * staging (thread tid carries chunks (tid & 3) + {0, 4, 8} of row tid >> 2) fills every (row, chunk) once, inside its row, and
    its ds_write_b128 groups of 8 consecutive lanes touch 8 different slots of a 128-byte bank row;
  * the 32 x 32 row fragments (ds_read_b128: lane l31 reads row 32 kbk + l31 at chunk 2 ks + hi) and both transpose reads of
    tr_frag (nb = 0..2, r0 = 0, 16, 32, 48) receive exactly the elements the MFMA operand order needs;
  * the conflict degree of both patterns -- 1: conflict-free -- is the number DESIGN.md records, for the 16-consecutive-rows model
    of tests/test_lds_layouts.py and for the lane groups the hardware serves a ds_read_b128 in;
  * the unmodified d = 64 / 128 formula on 12-chunk rows leaves the row (why the specialisation exists), and tokattn.hip's forward
    permutation L ^ ((r >> 1) & 2), derived for other reads, is a 2-way conflict for these row fragments."""
import itertools
import re
from pathlib import Path

import test_lds_layouts as L

ROW, CHUNKS, ROWS = 192, 12, 64
# the groups of 16 lanes a ds_read_b128 is served in (one LDS cycle each when conflict-free)
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]


def tile_off96(row, chunk):
    return row * ROW + ((chunk & ~3) << 4) + (((chunk & 3) ^ ((row >> 2) & 3)) << 4)


def tile_off_general(row, chunk, dh):
    """the d = 64 / 128 form: XOR over 8 chunks with the bit-reversed row-pair index"""
    return row * (dh * 2) + (((chunk & ~7) | ((chunk & 7) ^ L.rev3((row >> 1) & 7))) << 4)


def tile_off_forward(row, chunk):
    """tokattn.hip's d = 96 permutation"""
    return row * ROW + ((chunk ^ ((row >> 1) & 2)) << 4)


def staged(tid, i):
    """piece i of thread tid: (row, chunk)"""
    return tid >> 2, 4 * i + (tid & 3)


def image(off):
    lds = {}
    for tid, i in itertools.product(range(256), range(3)):
        row, chunk = staged(tid, i)
        for e in range(8):
            a = off(row, chunk) + 2 * e
            assert a not in lds
            lds[a] = (row, chunk * 8 + e)
    return lds


def row_frag_addrs(kbk, ks, off):
    return [off(32 * kbk + (lane & 31), 2 * ks + (lane >> 5)) for lane in range(64)]


def tr_addrs(nb, r0, second, off):
    addr = []
    for lane in range(64):
        a = lane & 15
        chunk = 4 * nb + 2 * ((lane >> 4) & 1) + ((a & 3) >> 1)
        row = r0 + 4 * (lane >> 5) + (a >> 2) + 8 * second
        addr.append(off(row, chunk) + (a & 1) * 8)
    return addr


def row_frag_degree(off):
    """most distinct 16-byte accesses on one slot, over 16 consecutive rows at one chunk (test_lds_layouts' model) and over the
    hardware's lane groups"""
    worst = 1
    for base, chunk in itertools.product(range(0, ROWS, 16), range(CHUNKS)):
        slots = [(off(base + r, chunk) % 256) // 16 for r in range(16)]
        worst = max(worst, max(slots.count(s) for s in slots))
    for kbk, ks in itertools.product(range(2), range(6)):
        addr = row_frag_addrs(kbk, ks, off)
        for g in B128_GROUPS:
            slots = [(addr[l] % 256) // 16 for l in g]
            worst = max(worst, max(slots.count(s) for s in slots))
    return worst


def transpose_degree(off):
    """test_lds_layouts' bank model: per half wave, distinct dwords per bank"""
    worst = 1
    for nb, r0, second in itertools.product(range(3), range(0, ROWS, 16), (0, 1)):
        addr = tr_addrs(nb, r0, second, off)
        for half in (0, 32):
            banks = {}
            for lane in range(half, half + 32):
                for w in range(2):
                    banks.setdefault((addr[lane] // 4 + w) % 64, set()).add(addr[lane] // 4 + w)
            worst = max(worst, max(len(v) for v in banks.values()))
    return worst


def test_staging_fills_every_chunk_once_inside_its_row():
    seen = {}
    for tid, i in itertools.product(range(256), range(3)):
        row, chunk = staged(tid, i)
        assert 0 <= row < ROWS and 0 <= chunk < CHUNKS
        a = tile_off96(row, chunk)
        assert a % 16 == 0 and row * ROW <= a <= row * ROW + ROW - 16, (row, chunk, a)
        assert a not in seen, (row, chunk, seen[a])
        seen[a] = (row, chunk)
    assert sorted(seen.values()) == [(r, c) for r in range(ROWS) for c in range(CHUNKS)]
    assert sorted(seen) == list(range(0, ROWS * ROW, 16))               # the tile, and nothing but the tile
    # ds_write_b128: groups of 8 consecutive lanes, banks (a / 4) mod 32 -> 8 slots of a 128-byte bank row
    for i, t0 in itertools.product(range(3), range(0, 256, 8)):
        slots = {(tile_off96(*staged(t, i)) % 128) // 16 for t in range(t0, t0 + 8)}
        assert len(slots) == 8, (i, t0, sorted(slots))


def test_row_fragments_receive_the_operand_rows():
    lds = image(tile_off96)
    for kbk, ks in itertools.product(range(2), range(6)):
        addr = row_frag_addrs(kbk, ks, tile_off96)
        for lane in range(64):
            hi, l31 = lane >> 5, lane & 31
            got = [lds[addr[lane] + 2 * e] for e in range(8)]
            # A operand of the 32x32x16 MFMA: row 32 kbk + l31, k = 16 ks + 8 hi + {0..7}
            assert got == [(32 * kbk + l31, 16 * ks + 8 * hi + e) for e in range(8)], (kbk, ks, lane)


def test_transpose_reads_receive_the_accumulator_order():
    lds = image(tile_off96)
    for nb, r0 in itertools.product(range(3), range(0, ROWS, 16)):
        for second in (0, 1):
            got = L.tr_read(tr_addrs(nb, r0, second, tile_off96), lds)
            for lane in range(64):
                rows = [r0 + 8 * second + 4 * (lane >> 5) + j for j in range(4)]
                assert got[lane] == [(r, nb * 32 + (lane & 31)) for r in rows], (nb, r0, second, lane)


def test_conflict_degree_is_the_one_design_md_records():
    text = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    m = re.search(r"`tile_off<96>`[^\n]*?conflict degree: row fragments (\d+), transpose reads (\d+)", text)
    assert m, "DESIGN.md does not record the conflict degree of tile_off<96>"
    assert (row_frag_degree(tile_off96), transpose_degree(tile_off96)) == (int(m.group(1)), int(m.group(2))) == (1, 1)
    # the forward kernel's d = 96 permutation was derived for other reads: it serves these transpose reads, not these row fragments
    assert row_frag_degree(tile_off_forward) == 2 and transpose_degree(tile_off_forward) == 1
    # ... and no swizzle at all: rows r and r + 4 share their slots
    assert row_frag_degree(lambda r, c: r * ROW + (c << 4)) == 4


def test_the_general_formula_leaves_a_12_chunk_row():
    out = [(r, c) for r in range(ROWS) for c in range(CHUNKS)
           if not r * ROW <= tile_off_general(r, c, 96) <= r * ROW + ROW - 16]
    assert out and all(c >= 8 for _, c in out)                          # chunks 8-11 of the rows whose XOR value has bit 2 set
    assert {c for _, c in out} == {8, 9, 10, 11} and len({r for r, _ in out}) == ROWS // 2
    assert max(tile_off_general(r, c, 96) for r, c in out) >= ROWS * ROW   # ... the last of them beyond the tile
    for dh in (64, 128):                                                # where it is used it stays inside
        assert all(r * dh * 2 <= tile_off_general(r, c, dh) <= r * dh * 2 + dh * 2 - 16 for r in range(ROWS) for c in range(dh // 8))
