"""Example searches (vs_search_examples) against their floor, one JSON line per case.

One index of --n x --d fp32 synthetic rows per metric (inner product, L2);
--users users with --pos positive and --neg negative examples each, stored rows
drawn at random, k = 10, device outputs.

For each metric: the plain vs_search at VS_RAW_ORDER k = w_0 over the users'
positives as one batch of users x pos queries — the engine call round 0 of an
example search makes, the floor this design cannot beat — then the example
search itself: wall ms per call (median), users per second, the library's
"examples_topk" (the engine's part) and "examples_collapse" (merge, negative
keys, emit) spans, rounds per call and the share of users searched again
(vs_examples_stats).
    python tools/bench_examples.py [--n 1000000] [--d 1536] [--users 4096] [--steps 7]"""
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
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--d", type=int, default=1536)
    p.add_argument("--users", type=int, default=4096)
    p.add_argument("--pos", type=int, default=8)
    p.add_argument("--neg", type=int, default=2)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--steps", type=int, default=7)
    a = p.parse_args()
    n, d, k, U = a.n, a.d, a.k, a.users
    rng = np.random.default_rng(7)
    labels = rng.integers(0, n, size=(U, a.pos + a.neg))
    pos = [row[:a.pos] for row in labels]
    neg = [row[a.pos:] for row in labels]
    D = torch.empty((U, k), dtype=torch.float32, device="cuda")
    I = torch.empty((U, k), dtype=torch.int64, device="cuda")
    E = torch.empty((U, k), dtype=torch.int32, device="cuda")
    lib = _lib.load()

    for metric, mname in ((vfaiss.METRIC_INNER_PRODUCT, "ip"), (vfaiss.METRIC_L2, "l2")):
        index = vfaiss.IndexFlat(d, metric)
        index.add_synthetic(n, seed=SEED)
        # the floor: the positives as plain queries, raw order, k = the first window
        w0 = vfaiss.distinct_plan(k, metric, True, n)[0]
        B = U * a.pos
        xq = torch.empty((B, d), dtype=torch.float32, device="cuda")
        flat = np.ascontiguousarray(labels[:, :a.pos].reshape(-1), dtype=np.int64)
        for q0 in range(0, B, 4096):
            rows = np.stack([index.reconstruct(int(r)) for r in flat[q0:q0 + 4096]])
            xq[q0:q0 + rows.shape[0]] = torch.from_numpy(rows).cuda()
        Dw = torch.empty((B, w0), dtype=torch.float32, device="cuda")
        Iw = torch.empty((B, w0), dtype=torch.int64, device="cuda")
        flags = _lib.IN_DEVICE | _lib.OUT_DEVICE | _lib.RAW_ORDER

        def plain():
            _lib.check(lib.vs_search(index._h, xq.data_ptr(), B, w0, Dw.data_ptr(), Iw.data_ptr(),
                                     flags, None))

        plain_ms = median_ms(plain, a.steps)
        print(json.dumps({"case": "plain vs_search, raw k = w0", "metric": mname, "n": n, "d": d,
                          "batch": B, "w0": w0, "kernel": _lib.timer_kernel(),
                          "ms": round(plain_ms, 3)}), flush=True)

        def run():
            index.search_examples_device(pos, neg, k, D.data_ptr(), I.data_ptr(), E.data_ptr())

        for _ in range(2):
            run()
        _lib.timer_enable(True)
        _lib.timer_reset()
        vfaiss.examples_stats(reset=True)
        ms = median_ms(run, a.steps, warmup=0)
        users, rounds, again = vfaiss.examples_stats()
        topk = _lib.timer_read_kernel("examples_topk")[0] / a.steps
        coll = _lib.timer_read_kernel("examples_collapse")[0] / a.steps
        _lib.timer_enable(False)
        _lib.timer_reset()
        print(json.dumps({"case": "examples", "metric": mname, "n": n, "d": d, "users": U,
                          "pos": a.pos, "neg": a.neg, "k": k, "ms": round(ms, 3),
                          "users_per_s": round(U / ms * 1e3, 1),
                          "over_plain": round(ms / plain_ms, 3),
                          "examples_topk_ms": round(topk, 3),
                          "examples_collapse_ms": round(coll, 4),
                          "rounds_per_call": round(rounds / a.steps, 2),
                          "searched_again_share": round(again / max(users, 1), 4)}), flush=True)
        del index, xq, Dw, Iw


if __name__ == "__main__":
    main()
