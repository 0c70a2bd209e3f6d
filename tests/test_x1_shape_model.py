"""CPU models of the filter pass's two dump forms (vs_gemm_x1.hip): the LDS
bank pattern of the 16x16x64 form's fragment reads, and the slot -> (row, lane
list, dump order) arithmetic that both forms must share.

The LDS image of one 64-B step holds row r's 16-B data chunk c at position
c ^ ((r >> 2) & 3) of the row's 64 bytes.  A ds_read_b128 is served in four
groups of 16 lanes (MI355X_MICROARCH.md, LDS table); a group is conflict-free
when its 16 x 16 B cover the 64 banks once.  The 32x32 reads (32 rows x 2
chunks) do; the 16x16 reads (16 rows x 4 chunks: lane l reads row l & 15 for K
group l >> 4) do only when K group g takes data chunk pi(g) for one of eight
permutations — both operands use the same pi, and a product is a sum over K,
so any fixed pi computes the same sums."""

import itertools
import os
import random

# ds_read_b128: the four groups of 16 lanes served together
LANE_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
]
LANE_GROUPS += [[l + 32 for l in g] for g in LANE_GROUPS]

PI = (0, 3, 1, 2)  # the kernel's: (0x9C >> 2 g) & 3
GOOD = {(0, 3, 1, 2), (0, 3, 2, 1), (1, 2, 0, 3), (1, 2, 3, 0),
        (2, 1, 0, 3), (2, 1, 3, 0), (3, 0, 1, 2), (3, 0, 2, 1)}


def _ways(addr_of_lane):
    """The worst bank multiplicity over the four lane groups of one 16-B read
    per lane (bank = (address / 4) mod 64)."""
    worst = 0
    for grp in LANE_GROUPS:
        banks = {}
        for l in grp:
            a = addr_of_lane(l)
            assert a % 16 == 0
            for w in range(4):
                bk = (a // 4 + w) % 64
                banks[bk] = banks.get(bk, 0) + 1
        worst = max(worst, max(banks.values()))
    return worst


def _read16(base, pi):
    def addr(l):
        r, g = base + (l & 15), l >> 4
        return r * 64 + (pi[g] ^ ((r >> 2) & 3)) * 16
    return addr


def _read32(base, s2):
    def addr(l):
        r, h = base + (l & 31), l >> 5
        return r * 64 + ((2 * s2 + h) ^ ((r >> 2) & 3)) * 16
    return addr


def test_kernel_permutation_is_the_modelled_one():
    assert sum(p << (2 * g) for g, p in enumerate(PI)) == 0x9C
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                       "book-recommendation-engine_amd", "csrc", "vs_gemm_x1.hip")
    with open(src, encoding="utf-8") as f:
        assert "(0x9C >> (2 * (lane >> 4))) & 3" in f.read()


def test_16_row_reads_conflict_free_under_the_kernel_permutation():
    for base in range(0, 256, 16):
        assert _ways(_read16(base, PI)) == 1, base


def test_16_row_reads_identity_permutation_is_two_way():
    for base in range(0, 256, 16):
        assert _ways(_read16(base, (0, 1, 2, 3))) == 2, base


def test_the_eight_conflict_free_permutations():
    for pi in itertools.permutations(range(4)):
        w = {_ways(_read16(base, pi)) for base in range(0, 256, 16)}
        assert w == ({1} if pi in GOOD else {2}), (pi, w)


def test_32_row_reads_conflict_free():
    for base in range(0, 256, 32):
        for s2 in (0, 1):
            assert _ways(_read32(base, s2)) == 1, (base, s2)


# --- slots, rows, lists and dump order ------------------------------------

def tile_perm(t):
    return (((t * 2654435761) & 0xFFFFFFFF) >> 24) & 0xFC


def _dump32(t, wr, cand, ntotal, selfrow, dc0):
    """The 32x32 form's dump epilogue of wave (wr, any wq) on tile t: lane l
    holds query c = l & 31 of two 32-query blocks and rows 32 rb + 8 jj + 4 h +
    e (h = l >> 5); one lane owns a list.  cand(query, slot) -> the row's sum
    clears the threshold.  Returns {(query, list): [(slot index, row), ...]},
    the row and list of every (query, slot), and the lists' final counts."""
    f = tile_perm(t)
    out, where, cnt = {}, {}, {}
    for l in range(64):
        h, c32 = l >> 5, l & 31
        fh = (4 * h) ^ (f & 0x04)
        for qb in range(2):
            q = 32 * qb + c32
            lst = wr * 2 + h
            dc = dc0
            for rb in range(4):
                for bi in range(16):
                    jj, e = bi >> 2, bi & 3
                    slot = 128 * wr + 32 * rb + 8 * jj + 4 * h + e
                    row = t * 256 + ((128 * wr + 32 * rb) ^ (f & 0xE0)) + ((8 * jj) ^ (f & 0x18)) + fh + e
                    where[(q, slot)] = (row, lst)
                    if not cand(q, slot):
                        continue
                    if not (row < ntotal and row != selfrow.get(q, -1)):
                        continue
                    out.setdefault((q, lst), []).append((dc, row))
                    dc += 1
            cnt[(q, lst)] = dc
    return out, where, cnt


def _dump16(t, wr, cand, ntotal, selfrow, dc0):
    """The 16x16 form's: lane l holds query l & 15 of four 16-query blocks and
    rows 16 b + 4 g + e (g = l >> 4); lanes l and l ^ 32 share a list and, per
    16-row block, exchange the counts of the rows that take a slot: the lane
    below 32 stores first, both advance the count by the sum."""
    f = tile_perm(t)
    out, where, cnt = {}, {}, {}
    dc = {l: [dc0] * 4 for l in range(64)}
    for qb in range(4):
        for b in range(8):
            cm = {}
            for l in range(64):
                g, c16 = l >> 4, l & 15
                q = 16 * qb + c16
                fl = (4 * g) ^ (f & 0x0C)
                row0 = t * 256 + ((128 * wr + 16 * b) ^ (f & 0xF0)) + fl
                rows = []
                for e in range(4):
                    slot = 128 * wr + 16 * b + 4 * g + e
                    where[(q, slot)] = (row0 + e, wr * 2 + (g & 1))
                    if cand(q, slot) and row0 + e < ntotal and row0 + e != selfrow.get(q, -1):
                        rows.append(row0 + e)
                cm[l] = rows
            for l in range(64):
                g, c16 = l >> 4, l & 15
                q, lst = 16 * qb + c16, wr * 2 + (g & 1)
                n, npart = len(cm[l]), len(cm[l ^ 32])
                c = dc[l][qb] + (npart if l >= 32 else 0)
                dc[l][qb] += n + npart
                for row in cm[l]:
                    out.setdefault((q, lst), []).append((c, row))
                    c += 1
    for l in range(64):
        for qb in range(4):
            key = (16 * qb + (l & 15), wr * 2 + ((l >> 4) & 1))
            assert cnt.setdefault(key, dc[l][qb]) == dc[l][qb]  # the pair agree
    return out, where, cnt


def _check_tile(t, wr, density, ntotal, selfrow, seed):
    rng = random.Random(seed)
    table = {}

    def cand(q, slot):
        if (q, slot) not in table:
            table[(q, slot)] = rng.random() < density
        return table[(q, slot)]

    o32, w32, c32 = _dump32(t, wr, cand, ntotal, selfrow, 5)
    o16, w16, c16 = _dump16(t, wr, cand, ntotal, selfrow, 5)
    f = tile_perm(t)
    assert w32 == w16  # every (query, slot): the same row and the same list
    for (q, slot), (row, lst) in w32.items():
        assert row == t * 256 + (slot ^ f) and lst == wr * 2 + ((slot >> 2) & 1)
    assert c32 == c16
    assert set(o32) == set(o16)
    for key in o32:
        a, b = sorted(o32[key]), sorted(o16[key])
        assert a == b, (t, wr, key)  # the same row in the same slot of the list
        assert [c for c, _ in a] == list(range(5, 5 + len(a)))  # no slot twice, none skipped


def test_both_forms_fill_the_same_lists_in_the_same_order():
    tiles = [0, 1, 2, 3, 7, 100, 1171, 4882]
    assert len({tile_perm(t) for t in tiles}) >= 6
    for i, t in enumerate(tiles):
        for wr in (0, 1):
            for density in (1.0, 0.3, 0.02):
                _check_tile(t, wr, density, 1 << 30, {}, 10 * i + wr)


def test_rows_that_take_no_slot_are_not_counted():
    """The last tile's padding (rows >= ntotal) and the queries' own rows."""
    t = 1171
    ntotal = 300_000  # 224 rows of tile 1171
    selfrow = {q: t * 256 + ((q * 37) % 256) for q in range(64)}
    for wr in (0, 1):
        for density in (1.0, 0.3):
            _check_tile(t, wr, density, ntotal, selfrow, 99 + wr)
