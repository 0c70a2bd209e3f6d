"""Where searches (vs_search_where) against their yardsticks, one JSON line per cell.

One index of --n x --d fp32 synthetic rows per metric (inner product, L2) with
one attribute column, a level uniform in [0, 1); k = 10, device buffers.  Query
q's predicate is a band of the level column that a fraction p of the rows
pass, p in --ps; batches --batches.

Per (batch, p), on the same build and the same index:

* "where":   the call as users make it (batches of at most 32 queries count
             first and choose a route per query);
* "windows": route A alone (VS_WHERE_CROSSOVER=0; small batches only);
* "scan":    route B alone (VS_WHERE_SCAN; small batches only, and the large
             batch at --scan-large-p alone: there it is the exact fp32 GEMM);
* "plain":   vs_search at the same k — the floor of a loose predicate;
* "sel":     vs_search_sel with ONE mask of the same selectivity for the whole
             batch — the nearest capability the library had.

Each line: wall ms per search (median), the route the counters show, window
rounds, queries scanned and rows the streaming kernel loaded per search
(vs_where_stats).  The small-batch crossover (vs_host.h kWhereCrossover) is
read off the "windows" and "scan" lines of batches 1 and 8.
    python tools/bench_where.py [--n 10000000] [--d 1536] [--metric ip] [--steps 5]"""
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


def median_ms(fn, steps, warmup=1):
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
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--metric", choices=("ip", "l2", "both"), default="both")
    p.add_argument("--batches", type=int, nargs="+", default=[1, 8, 4096])
    p.add_argument("--ps", type=float, nargs="+", default=[1, 0.3, 0.1, 0.03, 0.01, 0.001])
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--large-steps", type=int, default=2)
    p.add_argument("--scan-large-p", type=float, default=0.001)
    a = p.parse_args()
    n, d, k = a.n, a.d, a.k
    lib = _lib.load()
    Bmax = max(a.batches)
    xq = torch.empty((Bmax, d), dtype=torch.float32, device="cuda")
    _lib.check(lib.vs_fill_synthetic(xq.data_ptr(), Bmax, d, SEED + 1, 50_000_000, None))
    torch.cuda.synchronize()
    D = torch.empty((Bmax, k), dtype=torch.float32, device="cuda")
    I = torch.empty((Bmax, k), dtype=torch.int64, device="cuda")
    rng = np.random.default_rng(7)
    level = rng.random(n, dtype=np.float32)
    metrics = {"ip": [(vfaiss.METRIC_INNER_PRODUCT, "ip")], "l2": [(vfaiss.METRIC_L2, "l2")],
               "both": [(vfaiss.METRIC_INNER_PRODUCT, "ip"), (vfaiss.METRIC_L2, "l2")]}[a.metric]
    dflags = _lib.IN_DEVICE | _lib.OUT_DEVICE

    for metric, mname in metrics:
        index = vfaiss.IndexFlat(d, metric)
        index.reserve(n)
        index.add_synthetic(n, seed=SEED)
        attrs = index.attributes(level[None, :])
        print(json.dumps({"case": "plan", "metric": mname, "n": n, "d": d, "k": k,
                          "plan": vfaiss.where_plan(k, metric, False, n)}), flush=True)
        for B in a.batches:
            steps = a.steps if B <= 32 else a.large_steps

            def plain():
                index.search_device(xq.data_ptr(), B, k, D.data_ptr(), I.data_ptr())

            plain_ms = median_ms(plain, steps)
            print(json.dumps({"case": "plain", "metric": mname, "batch": B, "k": k,
                              "kernel": _lib.timer_kernel(), "ms": round(plain_ms, 3)}),
                  flush=True)
            for ps in a.ps:
                c = rng.uniform(ps / 2, 1 - ps / 2, B).astype(np.float32)
                lo = (c - np.float32(ps / 2)).reshape(B, 1)
                hi = (c + np.float32(ps / 2)).reshape(B, 1)
                where = (lo, hi, np.zeros((B, 3), dtype=np.uint64))
                runs = [("where", None, False)]
                if B <= 32:
                    runs += [("windows", "0", False), ("scan", None, True)]
                elif ps == a.scan_large_p:
                    runs += [("scan", None, True)]
                for case, cross, scan in runs:
                    if cross is None:
                        os.environ.pop("VS_WHERE_CROSSOVER", None)
                    else:
                        os.environ["VS_WHERE_CROSSOVER"] = cross

                    def run():
                        index.search_where_device(xq.data_ptr(), B, k, attrs, where,
                                                  D.data_ptr(), I.data_ptr(), scan=scan)

                    run()
                    vfaiss.where_stats(reset=True)
                    ms = median_ms(run, steps, warmup=0)
                    searches, rounds, again, scanned, streamed = vfaiss.where_stats(reset=True)
                    route = ("scan" if scanned == searches else
                             "windows" if scanned == 0 else "windows+scan")
                    print(json.dumps({
                        "case": case, "metric": mname, "batch": B, "p": ps, "ms": round(ms, 3),
                        "over_plain": round(ms / plain_ms, 3), "route": route,
                        "rounds_per_search": round(rounds / steps, 2),
                        "scanned_per_search": round(scanned / steps, 2),
                        "rows_streamed_per_search": int(streamed / steps)}), flush=True)
                os.environ.pop("VS_WHERE_CROSSOVER", None)
                # one shared mask of the same selectivity through the selector search
                mask = (level >= lo[0, 0]) & (level <= hi[0, 0])
                sel = index.selector(vfaiss.IDSelectorBitmap(n, np.packbits(mask,
                                                                            bitorder="little")))

                def selected():
                    _lib.check(lib.vs_search_sel(index._h, sel._h, xq.data_ptr(), B, k,
                                                 D.data_ptr(), I.data_ptr(), dflags, None))

                ms = median_ms(selected, steps)
                print(json.dumps({"case": "sel", "metric": mname, "batch": B, "p": ps,
                                  "selected": sel.count, "ms": round(ms, 3),
                                  "over_plain": round(ms / plain_ms, 3)}), flush=True)
                sel.close()
        attrs.close()
        del index


if __name__ == "__main__":
    main()
