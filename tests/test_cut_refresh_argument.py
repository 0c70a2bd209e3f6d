"""CPU model of the query cuts taken again after every replay (vs_x1_cuts.hip
"Query cuts", x1_replay_cut_kernel; vs_gemm_x1.hip x1_plan).

tests/test_filter_argument.py models ONE cut, a_M(snapshot) + 2.000001 B, taken
after the first launch of a pass.  The pass now takes it again after every
replay: cut = min(cut, a_M(lists now) + 2.000001 B).  a_M only falls while the
pass runs, so every cut is at or above the final a_M + 2B, the verification's
T = min(T, final cut) is a floor for every row any launch dropped (a row dropped
at launch c had key >= min(cut_c, last_c) >= min(cut_final, last_final)), and
both checks decide what they decided before.  This file restates the streaming
model with several snapshots, the dump / replay model with a cut per segment,
and the fused kernel's radix selection of a_M.  Statements about the algorithm:
the GPU tests check the kernels against the oracle."""

import numpy as np

from test_filter_argument import _accept, _mth_smallest_by_bits, _order_image, _stream_lists


def _cut_value(aM, B):
    """qcut_kernel / x1_replay_cut_kernel: a_M + 2.000001 B rounded up to fp32."""
    tp = float(aM) + 2.000001 * B
    t = np.float32(tp)
    if float(t) < tp:
        t = np.nextafter(t, np.float32(np.inf))
    return float(t)


def _refresh(cut, lists, a, B, M):
    """The cut after a snapshot of the lists: never above the stored one, -inf
    (a list of the query out of slots) stays, fewer than M entries: unchanged."""
    if cut == -np.inf:
        return cut
    ent = np.array([a[x] for lst in lists for x in lst])
    if len(ent) < M:
        return cut
    return min(cut, _cut_value(np.sort(ent)[M - 1], B))


def _stream_lists_recut(a, owner, P, L, order, cut_points, B, M, late):
    """test_filter_argument._stream_lists with a snapshot before each row index
    in `cut_points`: rows are admitted below min(the list's last entry, the cut
    then in force).  Returns the lists, the cut after every snapshot and the
    rows admitted from row `late` on."""
    lists = [[] for _ in range(P)]
    cut = np.inf
    cuts = []
    admitted = 0
    points = set(cut_points)
    for i, r in enumerate(order):
        if i in points:
            cut = _refresh(cut, lists, a, B, M)
            cuts.append(cut)
        lst = lists[owner[r]]
        lim = a[lst[-1]] if len(lst) == L else np.inf
        if a[r] < min(lim, cut):
            admitted += i >= late
            lst.append(r)
            lst.sort(key=lambda x: (a[x], x))
            del lst[L:]
    return [np.array(lst, dtype=np.int64) for lst in lists], cuts, admitted


def _verify(lists, cut, a, e, B, M, KF, L):
    """Both checks over the final lists with the final cut as the floor of the
    dropped rows (test_query_cut_keeps_both_checks_and_drops_admissions)."""
    n = a.shape[0]
    full = [lst for lst in lists if len(lst) == L]
    T = min((a[lst[-1]] for lst in full), default=np.inf)
    T = min(T, cut)
    entries = np.concatenate(lists)
    srt = entries[np.lexsort((entries, a[entries]))]
    aM = a[srt[M - 1]]
    merged = srt[:KF]
    T1 = min(a[merged[-1]] if len(merged) == KF else np.inf, T)
    ok1, top1 = _accept(list(merged), T1, e, B, M)
    Tp = min(T, aM + 2.000001 * B)
    S = sorted(r for r in entries if a[r] < Tp)
    ok2, top2 = _accept(S, Tp, e, B, M)
    exact = np.lexsort((np.arange(n), e))[:M]
    for ok, top in ((ok1, top1), (ok2, top2)):
        if ok:
            np.testing.assert_array_equal(top, exact)
    return ok1, ok2, Tp, S, aM


def test_refreshed_cuts_keep_both_checks_and_drop_more_admissions():
    """Snapshots at the replay points 1, 2, 4 and 8 of 10 parts: the checks'
    outcomes, T' and the rescored set equal those of the single snapshot (after
    part 1) and of no cut at all; the cut never rises and never falls below the
    final a_M + 2B; after the first snapshot the lists admit no more rows than
    with the single cut (fewer on average)."""
    rng = np.random.default_rng(15)
    B, M, KF, P, L = 1e-3, 19, 32, 128, 8
    ratio = []
    for q in range(40):
        n = 20000
        e = rng.standard_normal(n) * 0.01
        if q % 3 == 0:  # near-duplicates at the top
            e[rng.choice(n, 50, replace=False)] = -0.05 + rng.uniform(0, 4 * B, 50)
        a = e + rng.uniform(-B, B, n)
        owner = rng.integers(0, P, size=n)
        order = rng.permutation(n)
        first = n // 10
        points = [first, 2 * n // 10, 4 * n // 10, 8 * n // 10]
        none, _, _ = _stream_lists(a, owner, P, L, order, None, B, M, first)
        one, cut1, adm1 = _stream_lists(a, owner, P, L, order, first, B, M, first)
        many, cuts, admn = _stream_lists_recut(a, owner, P, L, order, points, B, M, first)
        r0 = _verify(none, np.inf, a, e, B, M, KF, L)
        r1 = _verify(one, cut1, a, e, B, M, KF, L)
        rn = _verify(many, cuts[-1], a, e, B, M, KF, L)
        for r in (r1, rn):
            assert r[:2] == r0[:2] and r[2] == r0[2] and r[3] == r0[3] and r[4] == r0[4]
        # the first snapshot is the single cut (_stream_lists always steps one
        # fp32 up, the kernels only when the rounding went down)
        assert cuts[0] <= cut1 <= np.nextafter(np.float32(cuts[0]), np.float32(np.inf))
        assert all(c1 <= c0 for c0, c1 in zip(cuts, cuts[1:]))
        assert cuts[-1] >= rn[4] + 2 * B  # never below the final a_M + 2B
        assert admn <= adm1
        ratio.append((admn, adm1))
    # a_M falls between the snapshots, so over 40 queries some rows are saved
    print("admitted after the first snapshot:", sum(r[0] for r in ratio), "of",
          sum(r[1] for r in ratio))
    assert sum(r[0] for r in ratio) < sum(r[1] for r in ratio)


def _dump_pass(a, a_lo, owner, P, L, R, B, M, parts, refresh):
    """A pass of `parts` equal launches over rows 0 .. n-1 in order: launch 0
    lists, the cut after it, launches 1 .. parts-1 dump (blocks of 16 rows: the
    block test, then one slot per row whose bound a_lo clears the floor =
    min(cut, the list's last entry at the segment's start)), a replay after
    launches 1, 3, 7, .. and the last (x1_launch), the cut taken again after
    every replay but the last when `refresh`.  Returns the lists, the cut in
    force at every launch, the final cut and the rows dumped."""
    n = a.shape[0]
    bounds = [n * p // parts for p in range(parts + 1)]
    lists, _, _ = _stream_lists(a[: bounds[1]], owner[: bounds[1]], P, L, np.arange(bounds[1]),
                                None, B, M, 0)
    lists = [list(lst) for lst in lists]
    cut = _refresh(np.inf, lists, a, B, M)
    cut_at = [np.inf]
    dumps = [[] for _ in range(P)]
    dumped = 0
    floors = None
    for c in range(1, parts):
        if floors is None:  # segment start: the lists as the last replay left them
            floors = [min(cut, a[lst[-1]] if len(lst) == L else np.inf) for lst in lists]
        cut_at.append(cut)
        for b0 in range(bounds[c], bounds[c + 1], 16):
            blk = np.arange(b0, min(b0 + 16, bounds[c + 1]))
            f = floors[owner[b0]]
            if a_lo[blk].min() < f:
                rows = [int(r) for r in blk if a_lo[r] < f]
                dumps[owner[b0]].extend(rows)
                dumped += len(rows)
        if ((c + 1) & c) == 0 or c + 1 == parts:  # x1_replay
            if any(len(d) > R for d in dumps):
                cut = -np.inf  # a list out of slots: the query fails
            for p in range(P):
                if len(dumps[p]) > R:
                    continue
                lst = lists[p]
                for r in dumps[p]:
                    lim = a[lst[-1]] if len(lst) == L else np.inf
                    if a[r] < min(lim, cut_at[-1]):
                        lst.append(r)
                        lst.sort(key=lambda x: (a[x], x))
                        del lst[L:]
            dumps = [[] for _ in range(P)]
            floors = None
            if refresh and c + 1 < parts:
                cut = _refresh(cut, lists, a, B, M)
    return lists, cut_at, cut, dumped


def test_dump_and_replay_with_refreshed_cuts():
    """The final lists of list launch + dump launches + replays, with the cut
    taken again after every replay, equal those of admitting every row
    in-kernel against min(list last, the cut in force at its launch); fewer rows
    are dumped than with the cut set once; a list out of slots turns its
    query's cut to -inf and no later refresh brings it back."""
    rng = np.random.default_rng(12)
    B, M, P, L, parts = 1e-3, 19, 64, 8, 10
    saved = []
    failed = 0
    for trial in range(16):
        n = 16 * 2560
        a = (rng.standard_normal(n) * 0.01).astype(np.float64)
        hard = trial % 4 == 0
        if hard:  # near-duplicates just above the top, late in the pass: more rows than slots
            a[n // 2 + rng.choice(n // 2, 1500, replace=False)] = -0.045 + rng.uniform(0, B, 1500)
        R = 16 if hard else 128
        a_lo = a - np.abs(rng.standard_normal(n)) * 2e-3  # the per-row test's bound
        owner = np.repeat(rng.integers(0, P, size=n // 16), 16)  # blocks of 16 rows
        lists, cut_at, cut, dumped = _dump_pass(a, a_lo, owner, P, L, R, B, M, parts, True)
        _, _, cut0, dumped0 = _dump_pass(a, a_lo, owner, P, L, R, B, M, parts, False)
        assert all(c1 <= c0 for c0, c1 in zip(cut_at, cut_at[1:]))  # never rises
        if cut == -np.inf:
            # failed at some replay: every cut after that launch is -inf too
            first = cut_at.index(-np.inf) if -np.inf in cut_at else len(cut_at)
            assert all(c == -np.inf for c in cut_at[first:])
            assert _refresh(cut, lists, a, B, M) == -np.inf
            failed += 1
            continue
        assert cut0 != -np.inf or hard
        # in-kernel admission with the cut in force at each launch
        bounds = [n * p // parts for p in range(parts + 1)]
        ref = [[] for _ in range(P)]
        for c in range(parts):
            for r in range(bounds[c], bounds[c + 1]):
                lst = ref[owner[r]]
                lim = a[lst[-1]] if len(lst) == L else np.inf
                if a[r] < min(lim, cut_at[c]):
                    lst.append(r)
                    lst.sort(key=lambda x: (a[x], x))
                    del lst[L:]
        for p in range(P):
            np.testing.assert_array_equal(np.array(lists[p], dtype=np.int64),
                                          np.array(ref[p], dtype=np.int64))
        if cut0 != -np.inf:
            assert dumped <= dumped0
            saved.append((dumped, dumped0))
    assert failed > 0 and len(saved) >= 8
    print("rows dumped:", sum(s[0] for s in saved), "of", sum(s[1] for s in saved))
    assert sum(s[0] for s in saved) < sum(s[1] for s in saved)


def _mth_smallest_by_radix(keys, valid, M):
    """x1_replay_cut_kernel's selection restated: over the valid keys' order
    images, byte by byte from the top, the histogram of the images that share
    the bytes chosen so far and the bin where the running count reaches the
    rank left."""
    img = _order_image(keys)[np.asarray(valid, bool)].astype(np.uint64)
    if len(img) < M:
        return None
    pre, want = 0, M
    for sh in (24, 16, 8, 0):
        live = img if sh == 24 else img[(img >> (sh + 8)) == (pre >> (sh + 8))]
        hist = np.bincount(((live >> sh) & 0xFF).astype(np.int64), minlength=256)
        inc = np.cumsum(hist)
        d = int(np.searchsorted(inc, want))  # the first bin with inc >= want
        want -= int(inc[d] - hist[d])
        pre |= d << sh
    assert 1 <= want
    u = np.uint32(pre)
    back = np.uint32(u & 0x7FFFFFFF) if u & 0x80000000 else np.uint32(~u)
    return np.array([back], np.uint32).view(np.float32)[0]


def test_radix_selection_is_the_mth_smallest_key():
    rng = np.random.default_rng(4)
    for trial in range(300):
        n = int(rng.integers(1, 300))
        keys = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 3)).astype(np.float32)
        if trial % 5 == 0:
            keys[: n // 2] = keys[0]                       # duplicates
        if trial % 7 == 0:
            keys[rng.random(n) < 0.2] = np.float32(-0.0)   # signed zeros
        if trial % 11 == 0:
            keys[rng.random(n) < 0.2] = np.float32(0.0)
        valid = rng.random(n) < 0.9
        M = int(rng.integers(1, 40))
        got = _mth_smallest_by_radix(keys, valid, M)
        v = np.sort(keys[valid])
        if len(v) < M:
            assert got is None
            assert _mth_smallest_by_bits(keys, valid, M) is None
        else:
            assert got == v[M - 1]  # -0.0 == 0.0: the order image ranks -0 first
            bits = _mth_smallest_by_bits(keys, valid, M)
            assert np.float32(got).view(np.uint32) == np.float32(bits).view(np.uint32)
