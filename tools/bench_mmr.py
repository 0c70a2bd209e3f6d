"""MMR searches (vs_search_mmr) against their yardsticks, one JSON line per case.

One L2 index of --n x --d fp32 synthetic rows (the reference's stores are L2),
--batch queries, fetch_k in {20, 64, 256} and k in {4, 10}.

* "search_mmr": the whole call, device buffers in and out.  Wall ms per call
  (median), queries/s, and from the library's timer spans the ms of the
  re-rank's two kernels ("mmr_sims": the query cosines and candidate norms,
  "mmr_pick": the greedy selection with the picks' cosines computed on demand).
* "search": the plain vs_search for fetch_k alone at the same batch, device
  buffers: what the call spends before the re-rank.
* "host route": what a user of the library has without this call, LangChain's
  own steps, one query at a time: search(fetch_k), reconstruct every candidate
  on the host, numpy cosine matrices, the greedy loop in Python (LangChain's
  maximal_marginal_relevance, as recalled).  Measured over --host queries and
  scaled to the batch.
    python tools/bench_mmr.py [--n 1000000] [--d 1536] [--batch 4096] [--steps 5]"""
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
from vsearch.synth import synthetic_rows  # noqa: E402

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


def span_ms(name, steps):
    try:
        return _lib.timer_read_kernel(name)[0] / steps
    except _lib.VSearchError:
        return 0.0


def cosine_similarity(X, Y):
    """langchain_community.utils.math.cosine_similarity (numpy path), as recalled."""
    X = np.array(X)
    Y = np.array(Y)
    X_norm = np.linalg.norm(X, axis=1)
    Y_norm = np.linalg.norm(Y, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        similarity = np.dot(X, Y.T) / np.outer(X_norm, Y_norm)
    similarity[np.isnan(similarity) | np.isinf(similarity)] = 0.0
    return similarity


def maximal_marginal_relevance(query_embedding, embedding_list, lambda_mult=0.5, k=4):
    """langchain_community.vectorstores.utils.maximal_marginal_relevance, as recalled."""
    if min(k, len(embedding_list)) <= 0:
        return []
    if query_embedding.ndim == 1:
        query_embedding = np.expand_dims(query_embedding, axis=0)
    similarity_to_query = cosine_similarity(query_embedding, embedding_list)[0]
    most_similar = int(np.argmax(similarity_to_query))
    idxs = [most_similar]
    selected = np.array([embedding_list[most_similar]])
    while len(idxs) < min(k, len(embedding_list)):
        best_score = -np.inf
        idx_to_add = -1
        similarity_to_selected = cosine_similarity(embedding_list, selected)
        for i, query_score in enumerate(similarity_to_query):
            if i in idxs:
                continue
            redundant_score = max(similarity_to_selected[i])
            equation_score = lambda_mult * query_score - (1 - lambda_mult) * redundant_score
            if equation_score > best_score:
                best_score = equation_score
                idx_to_add = i
        idxs.append(idx_to_add)
        selected = np.append(selected, [embedding_list[idx_to_add]], axis=0)
    return idxs


def host_route(index, xq, k, fetch_k, lam, count):
    """Per query, LangChain's own steps on the calls the library had before:
    median ms of each part."""
    parts = {"search": [], "reconstruct": [], "rerank": [], "total": []}
    for q in xq[:count]:
        t0 = time.perf_counter()
        _, I = index.search(q[None, :], fetch_k)
        t1 = time.perf_counter()
        rows = [index.reconstruct(int(i)) for i in I[0] if i != -1]
        t2 = time.perf_counter()
        maximal_marginal_relevance(np.array(q, dtype=np.float32), rows, k=k, lambda_mult=lam)
        t3 = time.perf_counter()
        for name, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
            parts[name].append(dt * 1e3)
    return {name: round(float(np.median(v)), 4) for name, v in parts.items()}


def main():
    import torch

    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--d", type=int, default=1536)
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--host", type=int, default=64, help="queries served by the host route")
    p.add_argument("--lambda-mult", type=float, default=0.5)
    a = p.parse_args()
    n, d, B, lam = a.n, a.d, a.batch, a.lambda_mult
    index = vfaiss.IndexFlat(d, vfaiss.METRIC_L2)
    index.reserve(n)
    index.add_synthetic(n, seed=SEED)
    xq = synthetic_rows(10_000_000, B, d, seed=5678)
    xd = torch.from_numpy(xq).cuda()

    for fetch_k in (20, 64, 256):
        Dc = torch.empty((B, fetch_k), dtype=torch.float32, device="cuda")
        Ic = torch.empty((B, fetch_k), dtype=torch.int64, device="cuda")
        ms = median_ms(lambda: index.search_device(xd.data_ptr(), B, fetch_k, Dc.data_ptr(),
                                                   Ic.data_ptr()), a.steps)
        print(json.dumps({"case": "search", "n": n, "d": d, "batch": B, "fetch_k": fetch_k,
                          "kernel": _lib.timer_kernel(), "ms": round(ms, 3),
                          "qps": round(B / ms * 1e3, 1)}), flush=True)
        for k in (4, 10):
            D = torch.empty((B, k), dtype=torch.float32, device="cuda")
            I = torch.empty((B, k), dtype=torch.int64, device="cuda")

            def mmr():
                index.search_mmr_device(xd.data_ptr(), B, k, fetch_k, lam, D.data_ptr(),
                                        I.data_ptr())

            for _ in range(2):
                mmr()
            _lib.timer_enable(True)
            _lib.timer_reset()
            ms = median_ms(mmr, a.steps, warmup=0)
            sims, pick = span_ms("mmr_sims", a.steps), span_ms("mmr_pick", a.steps)
            _lib.timer_enable(False)
            _lib.timer_reset()
            print(json.dumps({"case": "search_mmr", "n": n, "d": d, "batch": B,
                              "fetch_k": fetch_k, "k": k, "lambda_mult": lam,
                              "ms": round(ms, 3), "qps": round(B / ms * 1e3, 1),
                              "mmr_sims_ms": round(sims, 4), "mmr_pick_ms": round(pick, 4)}),
                  flush=True)
            if a.host:
                parts = host_route(index, xq, k, fetch_k, lam, a.host)
                print(json.dumps({"case": "host route: search, reconstruct, numpy loop",
                                  "fetch_k": fetch_k, "k": k, "queries": min(a.host, B),
                                  "ms_per_query": parts,
                                  "ms_scaled_to_batch": round(parts["total"] * B, 1),
                                  "search_mmr_speedup": round(parts["total"] * B / ms, 1)}),
                      flush=True)


if __name__ == "__main__":
    main()
