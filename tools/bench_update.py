"""In-place updates (vs_update_rows) and row-list joins (vs_range_selfjoin_rows),
one JSON line per case.

Updates.  An fp32 inner-product index of --ntotal x --d rows from bench.py's
clustered feed (unit-norm rows, 1024 centres + 0.5 noise).  For m in --rows:
``update`` of m random labels with m new host vectors, timed --steps times
(other labels each time), then the path it replaces on the same index — same
size, same planes — ``remove_ids`` of m random labels and ``add`` of the m
vectors.  Both calls return synchronised, so the host clock around them is
the call's time.  Default sizes: 1,000,000 and 10,000,000 rows; 1, 100 and
10,000 rows per call.

Joins.  At --join-ntotal (1,000,000) rows: ``range_selfjoin(0.75, rows=...)``
of 1, 128 and 1,024 scattered rows, and the same rows as single-row window
calls (``q0=row, nq=1``), the form a list had to take before.  Results are
copied to the host in both forms; the hits must agree.

    python tools/bench_update.py [--ntotal 1000000 10000000] [--d 1536] [--steps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "book-recommendation-engine_amd"))

from bench import ClusteredRows  # noqa: E402
from vsearch import faiss as vfaiss  # noqa: E402

NEW_ROW0 = 1 << 40  # generator rows of the replacement vectors: far from the index's


def build(torch, gen, n, d):
    index = vfaiss.IndexFlatIP(d)
    index.reserve(n)
    for r0 in range(0, n, 1 << 20):
        x = gen.rows(r0, min(1 << 20, n - r0))
        index.add_device(x.data_ptr(), x.shape[0])
        torch.cuda.synchronize()
        del x
    return index


def median_time(fn, steps):
    import torch

    walls = []
    for s in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(s)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    walls.sort()
    return walls[len(walls) // 2], walls


def bench_updates(torch, gen, n, d, counts, steps):
    index = build(torch, gen, n, d)
    rng = np.random.default_rng(n)
    new = gen.rows(NEW_ROW0, max(counts)).cpu().numpy()
    index.update(rng.choice(n, 8, replace=False), new[:8])  # warm-up: scratch, code objects
    for m in counts:
        labels = [rng.choice(n, m, replace=False).astype(np.int64) for _ in range(steps)]
        t_upd, w_upd = median_time(lambda s: index.update(labels[s], new[:m]), steps)
        assert index.ntotal == n

        def remove_add(s):
            assert index.remove_ids(labels[s]) == m
            index.add(new[:m])

        t_old, w_old = median_time(remove_add, steps)
        assert index.ntotal == n
        print(json.dumps({"case": "update", "ntotal": n, "d": d, "rows": m,
                          "update_s": round(t_upd, 6), "remove_add_s": round(t_old, 6),
                          "remove_add_over_update": round(t_old / t_upd, 1),
                          "update_runs_s": [round(w, 6) for w in w_upd],
                          "remove_add_runs_s": [round(w, 6) for w in w_old]}), flush=True)
    return index


def bench_joins(torch, index, n, d, counts, t, steps):
    rng = np.random.default_rng(7)
    index.range_selfjoin(t, rows=[0])  # warm-up
    index.range_selfjoin(t, q0=0, nq=1)
    for m in counts:
        rows = rng.choice(n, m, replace=False).astype(np.int64)
        out = {}

        def listed(_):
            out["list"] = index.range_selfjoin(t, rows=rows)

        def singles(_):
            out["single"] = [index.range_selfjoin(t, q0=int(r), nq=1) for r in rows]

        t_list, w_list = median_time(listed, steps)
        t_single, w_single = median_time(singles, 1 if m > 128 else steps)
        hits = int(out["list"][0][-1])
        assert hits == sum(int(p[0][-1]) for p in out["single"])
        assert out["list"][1].tobytes() == b"".join(p[1].tobytes() for p in out["single"])
        print(json.dumps({"case": "join", "ntotal": n, "d": d, "rows": m, "threshold": t,
                          "hits": hits, "row_list_s": round(t_list, 6),
                          "single_row_calls_s": round(t_single, 6),
                          "single_over_row_list": round(t_single / t_list, 1),
                          "row_list_runs_s": [round(w, 6) for w in w_list],
                          "single_runs_s": [round(w, 6) for w in w_single]}), flush=True)


def main():
    import torch

    p = argparse.ArgumentParser()
    p.add_argument("--ntotal", type=int, nargs="+", default=[1_000_000, 10_000_000])
    p.add_argument("--d", type=int, default=1536)
    p.add_argument("--rows", type=int, nargs="+", default=[1, 100, 10_000])
    p.add_argument("--join-ntotal", type=int, default=1_000_000)
    p.add_argument("--join-rows", type=int, nargs="+", default=[1, 128, 1024])
    p.add_argument("--threshold", type=float, default=0.75)
    p.add_argument("--steps", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_update: no GPU")
    gen = ClusteredRows(torch, a.d, seed=1234)
    for n in a.ntotal:
        index = bench_updates(torch, gen, n, a.d, a.rows, a.steps)
        if n == a.join_ntotal and a.join_rows:
            bench_joins(torch, index, n, a.d, a.join_rows, a.threshold, a.steps)
            a.join_rows = []
        del index
        torch.cuda.empty_cache()
    if a.join_rows:
        index = build(torch, gen, a.join_ntotal, a.d)
        bench_joins(torch, index, a.join_ntotal, a.d, a.join_rows, a.threshold, a.steps)


if __name__ == "__main__":
    main()
