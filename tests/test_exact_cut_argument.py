"""CPU model of the exact-key cuts (vs_x1_cuts.hip "Exact-key cuts",
x1_ecut_kernel).

tests/test_cut_refresh_argument.py models cut = min(cut, a_M + 2.000001 B) taken
after the list launch and after every replay.  The int8 inner-product pass of an
fp32 index now also scores the query's M best-approximate list entries (and
their ties) exactly and takes

    cut = min(cut, a_M + 2.000001 B, e_M + 1.000001 B),

e_M the M-th smallest exact key over those entries and the M best exact keys
kept from the earlier cuts.  e_M is an exact key of M distinct admissible rows,
so e_M >= E_M (the true M-th best), and a row with approximate key >= e_M + B
has an exact key > e_M >= E_M: outside the exact top M, ties included.  This
file restates the pass (lane lists, a list launch, dump launches, replays with
both cuts) on adversarial keys and checks that argument end to end.  Statements
about the algorithm: tests/test_gpu_exact_cut.py checks the kernels against the
oracle."""

import numpy as np
import pytest

from test_cut_refresh_argument import _cut_value
from test_filter_argument import _accept

CAND = 64  # x1_ecut_kernel's kEcutCand


def _ecut_value(eM, B):
    """x1_ecut_kernel: e_M + 1.000001 B rounded up to fp32."""
    tp = float(eM) + 1.000001 * B
    t = np.float32(tp)
    if float(t) < tp:
        t = np.nextafter(t, np.float32(np.inf))
    return float(t)


def _refresh(cut, lists, a, e, B, M, kept, exact):
    """The cut after a snapshot of the lists.  `kept`: the rows of the M best
    exact keys scored so far (updated in place when `exact`).  -inf stays, fewer
    than M entries: unchanged, never above the stored cut."""
    if cut == -np.inf:
        return cut
    ent = [x for lst in lists for x in lst]  # (list, position) order
    if len(ent) < M:
        return cut
    aM = np.sort(a[ent])[M - 1]
    cut = min(cut, _cut_value(aM, B))
    if exact:
        cand = [r for r in ent if a[r] <= aM][:CAND]  # the M best and their ties
        assert len(cand) >= M
        union = sorted(set(kept) | set(cand), key=lambda r: (e[r], r))
        before = e[kept[M - 1]] if len(kept) >= M else np.inf
        kept[:] = union[:M]
        eM = e[kept[M - 1]]
        assert eM <= before  # e_M only falls
        cut = min(cut, _ecut_value(eM, B))
    return cut


def _pass(a, a_lo, e, owner, P, L, R, B, M, bounds, exact):
    """A pass over rows 0 .. n-1 in order, launch c over rows bounds[c] ..
    bounds[c + 1]: launch 0 lists, the cut after it, the later launches dump
    (blocks of 16 rows: the block test, then one slot per row whose bound a_lo
    clears the floor = min(cut, the list's last entry at the segment's start)),
    a replay after launches 1, 3, 7, .. and the last (x1_launch), the cut taken
    again after every replay but the last.  Returns the lists, the cut in force
    at every launch, the final cut, the rows dumped and the rows a cut dropped
    (rows at or above the cut in force that the list's own floor would have
    admitted are among them; every row at or above its launch's cut is)."""
    nl = len(bounds) - 1
    lists = [[] for _ in range(P)]
    for r in range(bounds[1]):
        lst = lists[owner[r]]
        if len(lst) < L or a[r] < a[lst[-1]]:
            lst.append(r)
            lst.sort(key=lambda x: (a[x], x))
            del lst[L:]
    kept = []
    cut = _refresh(np.inf, lists, a, e, B, M, kept, exact)
    cut_at = [np.inf]
    dumps = [[] for _ in range(P)]
    dumped = 0
    floors = None
    for c in range(1, nl):
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
        if ((c + 1) & c) == 0 or c + 1 == nl:  # x1_replay
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
            if c + 1 < nl:
                cut = _refresh(cut, lists, a, e, B, M, kept, exact)
    return lists, cut_at, cut, dumped


def _verify(lists, cut, a, e, B, M, KF, L):
    """verify_rescore_kernel and verify_wide_kernel with T = min(T, cut): the
    first check over the KF merged candidates, the wide check over the entries
    below T' = min(T, a_M + 2.000001 B, e1_M + 1.000001 B).  An accepted set must
    be the exact top M."""
    n = a.shape[0]
    full = [lst for lst in lists if len(lst) == L]
    T = min((a[lst[-1]] for lst in full), default=np.inf)
    T = min(T, cut)
    entries = np.array([x for lst in lists for x in lst], dtype=np.int64)
    srt = entries[np.lexsort((entries, a[entries]))]
    merged = srt[:KF]
    T1 = min(a[merged[-1]] if len(merged) == KF else np.inf, T)
    ok1, top1 = _accept(list(merged), T1, e, B, M)
    Tp = T
    if len(srt) >= M:
        Tp = min(Tp, _cut_value(a[srt[M - 1]], B))
        e1 = np.sort(e[merged])
        Tp = min(Tp, _ecut_value(e1[M - 1], B))
    S = sorted(r for r in entries if a[r] < Tp)
    ok2, top2 = _accept(S, Tp, e, B, M)
    exact = np.lexsort((np.arange(n), e))[:M]
    for ok, top in ((ok1, top1), (ok2, top2)):
        if ok:
            np.testing.assert_array_equal(top, exact)
    return ok1, ok2, T


def _keys(kind, rng, n, B, M):
    """Exact keys e and approximate keys a with |a - e| <= B."""
    e = rng.standard_normal(n) * 0.01
    if kind == "edge":  # every error at +B or -B
        a = e + B * rng.choice([-1.0, 1.0], n)
    elif kind == "cluster":  # near-duplicates at the top, closer than B
        e[rng.choice(n, 60, replace=False)] = -0.05 + rng.uniform(0, 4 * B, 60)
        a = e + rng.uniform(-B, B, n)
    elif kind == "ties":  # a run of exact ties around the M-th key
        srt = np.argsort(e)
        e[srt[M - 6:M + 12]] = e[srt[M - 1]]
        a = e + rng.uniform(-B, B, n)
    elif kind == "reorder":  # the top M pushed up, the next 2M pulled down
        srt = np.argsort(e)
        e[srt[:3 * M]] = e[srt[0]] + np.sort(rng.uniform(0, 1.5 * B, 3 * M))
        a = e.copy()
        a[srt[:M]] += B
        a[srt[M:3 * M]] -= B
        rest = np.ones(n, bool)
        rest[srt[:3 * M]] = False
        a[rest] += rng.uniform(-B, B, int(rest.sum()))
    else:
        a = e + rng.uniform(-B, B, n)
    assert np.all(np.abs(a - e) <= B * (1 + 1e-12))
    return e, a


@pytest.mark.parametrize("kind", ["plain", "edge", "cluster", "ties", "reorder"])
@pytest.mark.parametrize("share", [1, 4])
def test_exact_cuts_keep_the_top_m_and_dump_no_more(kind, share):
    """A list launch over 1/10 (share 1) or 1/40 (share 4: the quarter-length
    list launch) of the rows, dump launches, replays with both cuts."""
    rng = np.random.default_rng(90 + share)
    B, M, KF, P, L, R, parts = 1e-3, 19, 24, 64, 8, 128, 10
    total = total2 = 0
    for trial in range(6):
        n = 16 * 1280
        e, a = _keys(kind, rng, n, B, M)
        a_lo = a - np.abs(rng.standard_normal(n)) * 2e-3  # the per-row test's bound
        owner = np.repeat(rng.integers(0, P, size=n // 16), 16)  # blocks of 16 rows
        if share == 1:
            bounds = [n * p // parts for p in range(parts + 1)]
        else:  # x1_launch's quarter form: parts [0, 1), [1, F), then one chunk each
            first = n // parts
            bounds = [0, first // share // 16 * 16] + [n * p // parts for p in range(1, parts + 1)]
        lists, cut_at, cut, dumped = _pass(a, a_lo, e, owner, P, L, R, B, M, bounds, True)
        lists2, cut_at2, cut2, dumped2 = _pass(a, a_lo, e, owner, P, L, R, B, M, bounds, False)
        assert cut != -np.inf and cut2 != -np.inf
        # the cut never rises and is never above the a_M + 2B form's
        cuts = cut_at + [cut]
        assert all(c1 <= c0 for c0, c1 in zip(cuts, cuts[1:]))
        assert all(cx <= c2 for cx, c2 in zip(cuts, cut_at2 + [cut2]))
        # no row of the exact top M, ties included, is at or above any cut
        EM = np.sort(e)[M - 1]
        top = np.flatnonzero(e <= EM)
        assert np.all(a[top] < min(cuts))
        # the floor the verification takes is below every cut used
        ok1, ok2, T = _verify(lists, cut, a, e, B, M, KF, L)
        assert all(c >= T for c in cuts)
        _verify(lists2, cut2, a, e, B, M, KF, L)
        # a row dropped by a cut: its launch's cut <= its key, so >= T too
        for c in range(1, len(bounds) - 1):
            rows = np.arange(bounds[c], bounds[c + 1])
            assert np.all(a[rows[a[rows] >= cut_at[c]]] >= T)
        assert dumped <= dumped2, (dumped, dumped2)
        total += dumped
        total2 += dumped2
    print(f"{kind}, list share 1/{share}: rows dumped {total} (exact cuts) / {total2} (a_M + 2B)")
    assert total < total2


def test_exact_cut_window_is_b():
    """The argument alone, on keys with errors at the edges: over ANY M rows,
    e_M >= E_M, and no row with a >= e_M + 1.000001 B has e <= E_M."""
    rng = np.random.default_rng(7)
    B, M = 1e-3, 19
    for trial in range(200):
        n = 2000
        e, a = _keys(["edge", "ties", "reorder", "cluster"][trial % 4], rng, n, B, M)
        EM = np.sort(e)[M - 1]
        rows = rng.choice(n, int(rng.integers(M, 4 * M)), replace=False)
        if trial % 2:  # the M best approximate rows, as the kernel takes them
            rows = np.argsort(a)[:M]
        eM = np.sort(e[rows])[M - 1]
        assert eM >= EM
        cut = _ecut_value(eM, B)
        assert not np.any(e[a >= cut] <= EM)
        # and the M rows that gave e_M are below the cut: the wide check keeps them
        best = rows[np.argsort(e[rows])[:M]]
        assert np.all(a[best] < cut)


def test_lists_out_of_slots_stay_failed():
    rng = np.random.default_rng(3)
    B, M, P, L, parts = 1e-3, 19, 64, 8, 10
    n = 16 * 1280
    e, a = _keys("plain", rng, n, B, M)
    late = n // 2 + rng.choice(n // 2, 1500, replace=False)
    e[late] = -0.045 + rng.uniform(0, B, 1500)
    a[late] = e[late]
    a_lo = a - 2e-3
    owner = np.repeat(rng.integers(0, P, size=n // 16), 16)
    bounds = [n * p // parts for p in range(parts + 1)]
    lists, cut_at, cut, _ = _pass(a, a_lo, e, owner, P, L, 16, B, M, bounds, True)
    assert cut == -np.inf
    first = cut_at.index(-np.inf) if -np.inf in cut_at else len(cut_at)
    assert all(c == -np.inf for c in cut_at[first:])
    assert _refresh(cut, lists, a, e, B, M, [], True) == -np.inf
