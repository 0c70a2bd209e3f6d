"""Boosted searches (vs_search_boost) against their yardsticks, one JSON line per cell.

One index of --n x --d fp32 synthetic rows per metric (inner product, L2) with
one attribute column, a level uniform in [0, 10), and one tag bit set on a
twentieth of the rows; k = 10, device buffers.  Query q boosts rows near its
own level (near, scale 5) and rows that carry the tag.  Configurations:

* "weak":      near weight 0.008 + tag bonus 0.002 (U = 0.01);
* "reference": the reference's weights, near 0.4 (missing 0.2) + tag 0.05.

Per (batch, configuration), on the same build and the same index:

* "boost":      the call as users make it (windows, give-up rule, scan);
* "no_giveup":  every window before the scan (VS_BOOST_GIVEUP=-1; batches of
                at most 32 queries: the A/B of vs_host.h kBoostGiveUp);
* "scan":       route B alone (VS_BOOST_SCAN; small batches, and the large
                batch for the reference weights: there it is the exact fp32 GEMM);
* "plain":      vs_search at the same k — the floor of a boost that changes nothing.

Each line: wall ms per search (median), window rounds, queries searched again
and queries scanned per search (vs_boost_stats), from which the fraction of
queries each round settled follows.
    python tools/bench_boost.py [--n 10000000] [--d 1536] [--metric ip] [--steps 5]"""
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
CONFIGS = {"weak": (0.008, 0.004, 0.002), "reference": (0.4, 0.2, 0.05)}


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
    p.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--large-steps", type=int, default=2)
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
    level = (rng.random(n, dtype=np.float32) * np.float32(10)).astype(np.float32)
    tags = (rng.random(n) < 0.05).astype(np.uint64)
    metrics = {"ip": [(vfaiss.METRIC_INNER_PRODUCT, "ip")], "l2": [(vfaiss.METRIC_L2, "l2")],
               "both": [(vfaiss.METRIC_INNER_PRODUCT, "ip"), (vfaiss.METRIC_L2, "l2")]}[a.metric]

    for metric, mname in metrics:
        index = vfaiss.IndexFlat(d, metric)
        index.reserve(n)
        index.add_synthetic(n, seed=SEED)
        attrs = index.attributes(level[None, :], tags)
        print(json.dumps({"case": "plan", "metric": mname, "n": n, "d": d, "k": k,
                          "plan": vfaiss.where_plan(k, metric, True, n)}), flush=True)
        for B in a.batches:
            steps = a.steps if B <= 32 else a.large_steps

            def plain():
                index.search_device(xq.data_ptr(), B, k, D.data_ptr(), I.data_ptr(), raw=True)

            plain_ms = median_ms(plain, steps)
            print(json.dumps({"case": "plain", "metric": mname, "batch": B, "k": k,
                              "kernel": _lib.timer_kernel(), "ms": round(plain_ms, 3)}),
                  flush=True)
            for cname in a.configs:
                w, miss, bonus = CONFIGS[cname]
                kinds = np.ones((B, 1), dtype=np.int32)
                params = np.empty((B, 1, 4), dtype=np.float32)
                params[:, 0, 0] = rng.uniform(1, 9, B)
                params[:, 0, 1:] = (5.0, w, miss)
                tmask = np.zeros((B, 4), dtype=np.uint64)
                tmask[:, 0] = 1
                tbonus = np.zeros((B, 4), dtype=np.float32)
                tbonus[:, 0] = bonus
                boost = (kinds, params, tmask, tbonus)
                runs = [("boost", None, False)]
                if B <= 32:
                    runs += [("no_giveup", "-1", False), ("scan", None, True)]
                elif cname == "reference":
                    runs += [("scan", None, True)]
                for case, giveup, scan in runs:
                    if giveup is None:
                        os.environ.pop("VS_BOOST_GIVEUP", None)
                    else:
                        os.environ["VS_BOOST_GIVEUP"] = giveup

                    def run():
                        index.search_boost_device(xq.data_ptr(), B, k, attrs, boost, D.data_ptr(),
                                                  I.data_ptr(), scan=scan)

                    run()
                    vfaiss.boost_stats(reset=True)
                    ms = median_ms(run, steps, warmup=0)
                    searches, rounds, again, scanned = vfaiss.boost_stats(reset=True)
                    print(json.dumps({
                        "case": case, "config": cname, "metric": mname, "batch": B,
                        "ms": round(ms, 3), "over_plain": round(ms / plain_ms, 3),
                        "rounds_per_search": round(rounds / steps, 2),
                        "settled_in_first_window": round(1 - again / max(searches, 1), 4),
                        "scanned_fraction": round(scanned / max(searches, 1), 4)}), flush=True)
                os.environ.pop("VS_BOOST_GIVEUP", None)
        attrs.close()
        del index


if __name__ == "__main__":
    main()
