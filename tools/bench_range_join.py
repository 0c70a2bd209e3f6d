"""Range self-joins (vs_range_selfjoin), one JSON line per case.

A C4-shaped join: --ntotal x --d fp32 rows from bench.py's clustered feed
(unit-norm rows, 1024 centres + 0.5 noise) in an inner-product index, joined in
full at a threshold that gives about --degree hits per row — the median over
256 sample rows of their --degree-th best similarity, from a top-k self-join.
Default sizes: 65,536 and 1,000,000 rows.  Each size runs with ``upper`` off
and on.

Yardstick, same index, same process: ``range_search`` over the same rows given
as device-resident queries in 65,536-query batches at the same threshold (the
rows are unit norm, so the inner product is the cosine) — what the cost model
says the full join equals.  And ``upper`` on against off: about half the
candidate-pass time plus the triangle's imbalance.

Per line: hits, candidates, wall s of the whole join (every 65,536-row call,
results left on the device), the summed "gemm_range" kernel s (vs_timer), the
same for the yardstick, and the two ratios.
    python tools/bench_range_join.py [--ntotal 65536 1000000] [--d 1536] [--steps 1]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "book-recommendation-engine_amd"))

from bench import ClusteredRows  # noqa: E402
from vsearch import _lib  # noqa: E402
from vsearch import faiss as vfaiss  # noqa: E402

CHUNK = 65536


def _totals(lib, h):
    try:
        nq, total, cand = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(lib.vs_range_size(h, ctypes.byref(nq), ctypes.byref(total)), "vs_range_size")
        _lib.check(lib.vs_range_candidates(h, ctypes.byref(cand)), "vs_range_candidates")
    finally:
        lib.vs_range_destroy(h)
    return total.value, cand.value


def join(index, n, t, upper):
    """The whole join in calls of CHUNK rows: (hits, candidates); no copy out."""
    lib = index._lib
    hits = cand = 0
    for q0 in range(0, n, CHUNK):
        h = ctypes.c_void_p()
        _lib.check(lib.vs_range_selfjoin(index._h, q0, min(CHUNK, n - q0), ctypes.c_float(t), 1,
                                         1 if upper else 0, 0, None, ctypes.byref(h)),
                   "vs_range_selfjoin")
        a, b = _totals(lib, h)
        hits, cand = hits + a, cand + b
    return hits, cand


def search(index, X, n, t):
    """range_search of the same rows as device queries, CHUNK at a time."""
    lib = index._lib
    hits = cand = 0
    for q0 in range(0, n, CHUNK):
        h = ctypes.c_void_p()
        xq = X[q0:q0 + CHUNK]
        _lib.check(lib.vs_range_search(index._h, None, ctypes.c_void_p(xq.data_ptr()),
                                       xq.shape[0], ctypes.c_float(t), _lib.IN_DEVICE, None,
                                       ctypes.byref(h)), "vs_range_search")
        a, b = _totals(lib, h)
        hits, cand = hits + a, cand + b
    return hits, cand


def timed(fn, steps):
    """(result, median wall s, gemm_range kernel s per run) of fn()."""
    import torch

    walls, ks, res = [], 0.0, None
    for _ in range(steps):
        torch.cuda.synchronize()
        _lib.timer_enable(True)
        _lib.timer_reset()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        ks += _lib.timer_read_kernel("gemm_range")[0] * 1e-3
        _lib.timer_enable(False)
    walls.sort()
    return res, walls[len(walls) // 2], ks / steps


def main():
    import torch

    p = argparse.ArgumentParser()
    p.add_argument("--ntotal", type=int, nargs="+", default=[65536, 1_000_000])
    p.add_argument("--d", type=int, default=1536)
    p.add_argument("--degree", type=int, default=15)
    p.add_argument("--steps", type=int, default=1)
    p.add_argument("--no-yardstick", action="store_true")
    a = p.parse_args()
    for n in a.ntotal:
        gen = ClusteredRows(torch, a.d, seed=1234)
        X = torch.cat([gen.rows(r0, min(1 << 20, n - r0)) for r0 in range(0, n, 1 << 20)])
        index = vfaiss.IndexFlatIP(a.d)
        index.reserve(n)
        index.add_device(X.data_ptr(), n)
        torch.cuda.synchronize()
        # the threshold: the median degree-th best similarity of 256 sample rows
        S, _ = index.selfjoin(a.degree, q0=n // 2, nq=min(256, n - n // 2))
        t = float(np.median(S[:, a.degree - 1]))
        join(index, min(n, CHUNK), t, False)  # warm-up: scratch, code objects
        line = {"ntotal": n, "d": a.d, "threshold": t}
        for upper in (False, True):
            (hits, cand), wall, ks = timed(lambda: join(index, n, t, upper), a.steps)
            key = "upper" if upper else "full"
            line[key] = {"hits": hits, "hits_per_row": round(hits / n, 2), "candidates": cand,
                         "wall_s": round(wall, 4), "gemm_range_kernel_s": round(ks, 4)}
        line["upper_over_full_wall"] = round(line["upper"]["wall_s"] / line["full"]["wall_s"], 3)
        line["upper_over_full_kernel"] = round(
            line["upper"]["gemm_range_kernel_s"] / line["full"]["gemm_range_kernel_s"], 3)
        if not a.no_yardstick:
            (hits, cand), wall, ks = timed(lambda: search(index, X, n, t), a.steps)
            line["range_search"] = {"hits": hits, "candidates": cand, "wall_s": round(wall, 4),
                                    "gemm_range_kernel_s": round(ks, 4)}
            line["full_over_range_search_wall"] = round(line["full"]["wall_s"] / wall, 3)
            line["full_over_range_search_kernel"] = round(
                line["full"]["gemm_range_kernel_s"] / ks, 3)
        print(json.dumps(line), flush=True)
        del index, X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
