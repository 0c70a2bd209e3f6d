"""Distinct searches (vs_search_distinct) against their yardstick, one JSON line per case.

One index of --n x --d fp32 synthetic rows per metric (inner product, L2),
--batch queries, k = 10, device buffers.  Three groupings:

* "own":    every row its own group (the answer is the plain search's);
* "pairs":  random pairs of rows;
* "copies": every query's nearest row appended --copies times, all in one
  group (a re-ingested book with many rows): the first window holds one group
  and the query is searched again.  Runs of exactly equal keys are the staged
  engine's own worst case (its bounds cannot separate them, so the plain
  search slows down too); this case therefore searches the first
  --copies-queries queries only, and its yardstick the same ones.

For each: wall ms per search (median), the library's "distinct_topk" (the
engine's part) and "distinct_collapse" spans, rounds per search and the share
of queries searched again (vs_distinct_stats).  The yardstick is the plain
vs_search at VS_RAW_ORDER k = w_0 in the same run: the engine call round 0
makes, so with every row its own group the difference is the collapse and one
count read-back.
    python tools/bench_distinct.py [--n 10000000] [--d 1536] [--batch 4096] [--steps 7]
    python tools/bench_distinct.py --batch 1"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "book-recommendation-engine_amd"))

from vsearch import _lib  # noqa: E402
from vsearch import faiss as vfaiss  # noqa: E402

SEED = 1234


def median_ms(fn, steps, warmup=2):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    t.sort()
    return t[len(t) // 2] * 1e3


def main():
    import torch

    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=10_000_000)
    p.add_argument("--d", type=int, default=1536)
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--steps", type=int, default=7)
    p.add_argument("--copies", type=int, default=32)
    p.add_argument("--copies-queries", type=int, default=256)
    a = p.parse_args()
    n, d, k, B = a.n, a.d, a.k, a.batch
    xq = torch.empty((B, d), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().vs_fill_synthetic(xq.data_ptr(), B, d, SEED + 1, 50_000_000, None))
    torch.cuda.synchronize()
    D = torch.empty((B, k), dtype=torch.float32, device="cuda")
    I = torch.empty((B, k), dtype=torch.int64, device="cuda")

    for metric, mname in ((vfaiss.METRIC_INNER_PRODUCT, "ip"), (vfaiss.METRIC_L2, "l2")):
        index = vfaiss.IndexFlat(d, metric)
        index.reserve(n + a.copies * B)
        index.add_synthetic(n, seed=SEED)

        def yardstick(live, B=B):
            w0 = vfaiss.distinct_plan(k, metric, False, live)[0]
            Dw = torch.empty((B, w0), dtype=torch.float32, device="cuda")
            Iw = torch.empty((B, w0), dtype=torch.int64, device="cuda")
            flags = _lib.IN_DEVICE | _lib.OUT_DEVICE | _lib.RAW_ORDER
            lib = _lib.load()

            def plain():
                _lib.check(lib.vs_search(index._h, xq.data_ptr(), B, w0, Dw.data_ptr(),
                                         Iw.data_ptr(), flags, None))

            ms = median_ms(plain, a.steps)
            print(json.dumps({"case": "plain vs_search, raw k = w0", "metric": mname, "n": live,
                              "d": d, "batch": B, "w0": w0, "kernel": _lib.timer_kernel(),
                              "ms": round(ms, 3)}), flush=True)
            return ms

        def distinct(case, groups, plain_ms, B=B):
            with index.grouping(groups) as grp:
                def run():
                    index.search_distinct_device(xq.data_ptr(), B, k, grp, D.data_ptr(),
                                                 I.data_ptr())

                for _ in range(2):
                    run()
                _lib.timer_enable(True)
                _lib.timer_reset()
                vfaiss.distinct_stats(reset=True)
                ms = median_ms(run, a.steps, warmup=0)
                searches, rounds, again = vfaiss.distinct_stats()
                topk = _lib.timer_read_kernel("distinct_topk")[0] / a.steps
                coll = _lib.timer_read_kernel("distinct_collapse")[0] / a.steps
                _lib.timer_enable(False)
                _lib.timer_reset()
                print(json.dumps({"case": case, "metric": mname, "n": index.ntotal, "d": d,
                                  "batch": B, "k": k, "groups": grp.groups, "ms": round(ms, 3),
                                  "over_plain": round(ms / plain_ms, 3),
                                  "distinct_topk_ms": round(topk, 3),
                                  "distinct_collapse_ms": round(coll, 4),
                                  "rounds_per_search": round(rounds / a.steps, 2),
                                  "searched_again_share": round(again / max(searches, 1), 4)}),
                      flush=True)

        plain_ms = yardstick(n)
        distinct("own", np.full(n, -1, dtype=np.int32), plain_ms)
        distinct("pairs", (np.random.default_rng(7).permutation(n) // 2).astype(np.int32),
                 plain_ms)
        # every query's nearest row, appended --copies times in one group with it
        Bc = min(B, a.copies_queries)
        index.search_device(xq.data_ptr(), Bc, 1, D.data_ptr(), I.data_ptr())
        torch.cuda.synchronize()
        near = I.view(-1)[:Bc].cpu().numpy()  # (k = 1: the first Bc entries of the buffer)
        groups = np.full(n + a.copies * Bc, -1, dtype=np.int32)
        for q0 in range(0, Bc, 256):
            rows = np.stack([index.reconstruct(int(r)) for r in near[q0:q0 + 256]])
            index.add(np.repeat(rows, a.copies, axis=0))
        for q, r in enumerate(near):
            g = groups[r] if groups[r] >= 0 else q
            groups[r] = g
            groups[n + a.copies * q: n + a.copies * (q + 1)] = g
        plain_ms = yardstick(index.ntotal, Bc)
        distinct("copies", groups, plain_ms, Bc)
        del index


if __name__ == "__main__":
    main()
