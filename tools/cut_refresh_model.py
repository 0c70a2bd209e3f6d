#!/usr/bin/env python3
"""CPU model of the rows a cutting filter pass dumps, with the query cut set
once (after the list launch) and taken again after every replay (DESIGN.md §3,
vs_gemm_x1.hip x1_launch).

One query: its approximate keys over the corpus are N standard normals, dealt
at random to P lane lists of L entries; the pass is `chunks` equal launches,
the first a list launch, the rest dump launches with replays after launches
1, 3, 7, 15, .. and the last.  A dump launch stores a row when its key is below
min(cut, the list's last entry at the segment's start); a replay leaves each
list the L smallest of its entries and its dumped rows.  cut = a_M + 2B with a_M
the M-th smallest key over the lists, 2B given in units of the keys' sigma.

    python tools/cut_refresh_model.py [--n 10000000] [--lists 128] [--m 32]
                                      [--two-b 0.6] [--chunks 20] [--queries 3]
                                      [--list-share F] [--window-first W]
                                      [--window-later W]

C3 (10M rows, 128 lists, 20 launches) measured 2,849 rows per query with the cut
set once and 1,238 with refreshed cuts (0.43x); the model gives ~3,000 at
M = 32, 2B = 0.6 sigma, and about half of that with refreshed cuts.

Exact-key cuts (x1_ecut_kernel): cut = e_M + B, the M-th smallest exact key over
the M best-approximate entries plus ONE bound; e_M sits at a_M on average, so the
model takes them as a window of B above a_M where a_M + 2B has 2B.
--window-first / --window-later set the window (in sigma) of the cut after the
list launch and of the refreshed cuts (default: --two-b for both);
--list-share F makes the list launch 1/F of the first chunk, with one dump
launch over the rest of that chunk (x1_launch's quarter form, VS_X1_QUARTER=F).
--table prints the schedules of DESIGN.md §8 round 9 at M = 19, B = 0.32 sigma."""

import argparse

import numpy as np


def run(keys, owner, P, L, M, two_b, chunks, refresh, share=1, w_first=None, w_later=None):
    n = keys.shape[0]
    w_first = two_b if w_first is None else w_first
    w_later = two_b if w_later is None else w_later
    bounds = [n * c // chunks for c in range(chunks + 1)]
    if share > 1:  # the list launch over 1/share of the first chunk
        bounds.insert(1, bounds[1] // share)
    nl = len(bounds) - 1
    lists = np.full((P, L), np.inf)

    def fold(rows_key, rows_owner):
        for p in np.unique(rows_owner):
            merged = np.concatenate([lists[p], rows_key[rows_owner == p]])
            lists[p] = np.sort(merged)[:L]

    def a_m():
        v = np.sort(lists[np.isfinite(lists)])
        return v[M - 1] if len(v) >= M else np.inf

    # the list launch: every row against its list
    k0, o0 = keys[: bounds[1]], owner[: bounds[1]]
    order = np.lexsort((k0, o0))
    start = np.searchsorted(o0[order], np.arange(P))
    for p in range(P):
        lists[p] = np.sort(np.concatenate([lists[p], k0[order[start[p]: start[p] + L]]]))[:L]
    cut = a_m() + w_first
    span = int((keys < cut).sum())
    seg, per_seg = 0, []
    floors = None
    pend_k, pend_o = [], []
    for c in range(1, nl):
        if floors is None:
            floors = np.minimum(lists[:, L - 1], cut)
        kc, oc = keys[bounds[c]: bounds[c + 1]], owner[bounds[c]: bounds[c + 1]]
        hit = kc < floors[oc]
        pend_k.append(kc[hit])
        pend_o.append(oc[hit])
        seg += int(hit.sum())
        if ((c + 1) & c) == 0 or c + 1 == nl:
            fold(np.concatenate(pend_k), np.concatenate(pend_o))
            pend_k, pend_o, floors = [], [], None
            per_seg.append(seg)
            seg = 0
            if refresh and c + 1 < nl:
                cut = min(cut, a_m() + w_later)
    return span, per_seg


def table(a, rng, M=19, B=0.32):
    """Rows dumped per query for the list-launch shares and windows of DESIGN.md
    §8 round 9 (refreshed cuts; the same keys for every schedule)."""
    rows = [(1, 2 * B, 2 * B, "all cuts a_M + 2B"), (1, B, 2 * B, "first cut exact"),
            (1, B, B, "every cut exact"), (4, 2 * B, 2 * B, "all cuts a_M + 2B"),
            (4, B, 2 * B, "first cut exact"), (4, B, B, "every cut exact"),
            (8, B, B, "every cut exact")]
    tot = [[] for _ in rows]
    for q in range(a.queries):
        keys = rng.standard_normal(a.n)
        owner = rng.integers(0, a.lists, a.n)
        for i, (share, wf, wl, _) in enumerate(rows):
            tot[i].append(sum(run(keys, owner, a.lists, a.entries, M, 2 * B, a.chunks, True, share,
                                  wf, wl)[1]))
    for (share, _, _, name), t in zip(rows, tot):
        print(f"list launch 1/{share * a.chunks}, {name}: {np.mean(t):.0f} rows dumped per query")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--lists", type=int, default=128)
    ap.add_argument("--entries", type=int, default=8)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--two-b", type=float, default=0.6)
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--queries", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--list-share", type=int, default=1)
    ap.add_argument("--window-first", type=float, default=None)
    ap.add_argument("--window-later", type=float, default=None)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    if a.table:
        table(a, rng)
        return
    tot = {False: [], True: []}
    for q in range(a.queries):
        keys = rng.standard_normal(a.n)
        owner = rng.integers(0, a.lists, a.n)
        for refresh in (False, True):
            span, per_seg = run(keys, owner, a.lists, a.entries, a.m, a.two_b, a.chunks, refresh,
                                a.list_share, a.window_first, a.window_later)
            tot[refresh].append(sum(per_seg))
            print(f"query {q} {'refreshed' if refresh else 'set once '}: first cut spans {span} rows, "
                  f"dumped per segment {per_seg} = {sum(per_seg)}")
    once, again = np.mean(tot[False]), np.mean(tot[True])
    print(f"rows dumped per query: {once:.0f} set once, {again:.0f} refreshed ({again / once:.2f}x)")


if __name__ == "__main__":
    main()
