"""Range searches (vs_range_search) against the exact fp32 top-k search, one JSON
line per case.

One index of --ntotal x --d fp32 synthetic rows (--metric ip or l2),
device-resident queries, batches 4096, 128 and 1, each at two radii: one that
gives about 10 hits per query and one that gives about 1,000.  The radii come
from top-k searches of the same queries: the median over the batch of the
10th (1,000th) best score.

Yardstick, same index, same process, alternating with the range calls step by
step: ``set_engine("fp32")`` ``search(k = 10)`` of the same batch — one pass of
the exact fp32 engine.  A range call is two such passes (count, fill) plus the
verification of its candidates.

Per case: hits, candidates (rows the GEMM passes handed to the verification)
and their ratio; median wall ms per range call and per top-k call, the ratio
of the two, and the summed "gemm_range" kernel ms per call (vs_timer).  --passes
repeats the whole protocol (the clocks of a box drift: compare the passes).
    python tools/bench_range.py [--ntotal 10000000] [--d 1536] [--metric ip] [--steps 5]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "book-recommendation-engine_amd"))

from vsearch import _lib  # noqa: E402
from vsearch import faiss as vfaiss  # noqa: E402
from vsearch.synth import synthetic_rows  # noqa: E402

SEED = 1234


def range_call(index, ptr, n, radius):
    """One vs_range_search over device queries: (hits, candidates); no copy out."""
    lib = index._lib
    h = ctypes.c_void_p()
    _lib.check(lib.vs_range_search(index._h, None, ctypes.c_void_p(ptr), n,
                                   ctypes.c_float(radius), _lib.IN_DEVICE, None,
                                   ctypes.byref(h)), "vs_range_search")
    try:
        nq, total, cand = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(lib.vs_range_size(h, ctypes.byref(nq), ctypes.byref(total)), "vs_range_size")
        _lib.check(lib.vs_range_candidates(h, ctypes.byref(cand)), "vs_range_candidates")
    finally:
        lib.vs_range_destroy(h)
    return total.value, cand.value


def alternate(range_fn, topk_fn, steps, warmup=1):
    """Median wall ms of each, the two alternating step by step, and the
    gemm_range kernel ms per range call."""
    import torch

    for _ in range(warmup):
        range_fn()
        topk_fn()
    torch.cuda.synchronize()
    tr, tk, kms = [], [], 0.0
    for _ in range(steps):
        _lib.timer_enable(True)
        _lib.timer_reset()
        t0 = time.perf_counter()
        range_fn()
        torch.cuda.synchronize()
        tr.append(time.perf_counter() - t0)
        kms += _lib.timer_read_kernel("gemm_range")[0]
        _lib.timer_enable(False)
        _lib.timer_reset()
        t0 = time.perf_counter()
        topk_fn()
        torch.cuda.synchronize()
        tk.append(time.perf_counter() - t0)
    tr.sort()
    tk.sort()
    return tr[len(tr) // 2] * 1e3, tk[len(tk) // 2] * 1e3, kms / steps


def main():
    import torch

    p = argparse.ArgumentParser()
    p.add_argument("--ntotal", type=int, default=10_000_000)
    p.add_argument("--d", type=int, default=1536)
    p.add_argument("--metric", choices=("ip", "l2"), default="ip")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--passes", type=int, default=2)
    p.add_argument("--batches", type=int, nargs="+", default=[4096, 128, 1])
    a = p.parse_args()
    n, d = a.ntotal, a.d
    metric = vfaiss.METRIC_INNER_PRODUCT if a.metric == "ip" else vfaiss.METRIC_L2
    bmax = max(a.batches)
    xq = torch.from_numpy(synthetic_rows(50_000_000, bmax, d, 5678)).cuda()
    index = vfaiss.IndexFlat(d, metric)
    index.reserve(n)
    index.add_synthetic(n, seed=SEED)
    index.set_engine("fp32")
    torch.cuda.synchronize()

    def kth_scores(nq, k):
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        index.search_device(xq.data_ptr(), nq, k, D.data_ptr(), I.data_ptr())
        torch.cuda.synchronize()
        return D[:, k - 1].cpu().numpy()

    # the radii: medians of the k-th best score (1,000: over at most 128 queries)
    radii = {}
    for nq in a.batches:
        for want in (10, 1000):
            kk = min(want, n)
            radii[nq, want] = float(np.median(kth_scores(min(nq, 128), kk)))

    for rep in range(a.passes):
        for nq in a.batches:
            D = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
            I = torch.empty((nq, 10), dtype=torch.int64, device="cuda")

            def topk():
                index.search_device(xq.data_ptr(), nq, 10, D.data_ptr(), I.data_ptr())

            for want in (10, 1000):
                radius = radii[nq, want]
                hits, cand = range_call(index, xq.data_ptr(), nq, radius)
                rms, tms, kms = alternate(lambda: range_call(index, xq.data_ptr(), nq, radius),
                                          topk, a.steps)
                print(json.dumps({
                    "pass": rep, "metric": a.metric, "ntotal": n, "d": d, "batch": nq,
                    "target_hits_per_query": want, "radius": radius, "hits": hits,
                    "hits_per_query": round(hits / nq, 2), "candidates": cand,
                    "candidates_per_hit": round(cand / hits, 4) if hits else None,
                    "range_ms": round(rms, 3), "gemm_range_kernel_ms": round(kms, 3),
                    "fp32_topk10_ms": round(tms, 3),
                    "ratio": round(rms / tms, 3) if tms else None,
                    "topk_kernel": _lib.timer_kernel()}), flush=True)


if __name__ == "__main__":
    main()
