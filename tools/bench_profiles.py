"""Profile searches (vs_search_profiles) against their yardsticks, one JSON line per case.

One L2 index of --n x --d fp32 synthetic rows (the reference's stores are L2),
--batch students, k = 10.  A student is a profile of 5-30 rated rows with the
reference's RATING_WEIGHTS and a list of rows already read, drawn so that most
lists are short (85 % at most 16 rows, 12 % up to 64, 3 % up to 256); the
profile's own rows are excluded too.

* "search_profiles": the batched call, host CSR in, host results out.  Wall ms
  per call (median) and queries/s; from the library's timer spans the mean
  kernel's ms and bytes/s (the rows it reads), the drop's ms, and the share of
  the step outside the engine (1 - engine spans / wall).
* "search_excl": the same with the means already on the device.
* "plain": vs_search of the same means at the same batch and k, device
  buffers: the ceiling.  Measured first, on an index no exclusion search has
  touched, and again at the end (the staged engine's adaptive plane order is
  kept per index, and the exclusion searches' deeper lists move it).
* --baseline S: the first S students served one at a time with what the
  library had before profile searches: reconstruct row by row, the mean on the
  host, a selector over every label, vs_search_sel at batch 1.  This mode uses
  no call of this change, so it also runs on an older build of the library.
    python tools/bench_profiles.py [--n 10000000] [--d 1536] [--batch 4096] [--steps 7]
    python tools/bench_profiles.py --baseline 64"""
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

SEED = 1234
RATING_WEIGHTS = (1.0, 0.7, 0.4, 0.2, 0.1)  # candidate_builder.py:45
CAPS = (0, 16, 64, 256, 1024)


def students(n, batch, seed=99):
    rng = np.random.default_rng(seed)
    profiles, read = [], []
    for _ in range(batch):
        size = int(rng.integers(5, 31))
        profiles.append((rng.choice(n, size, replace=False).astype(np.int64),
                         rng.choice(RATING_WEIGHTS, size).astype(np.float32)))
        u = rng.random()
        m = int(rng.integers(0, 17)) if u < 0.85 else \
            int(rng.integers(17, 65)) if u < 0.97 else int(rng.integers(65, 257))
        read.append(rng.choice(n, m, replace=False).astype(np.int64))
    return profiles, read


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


def baseline(index, profiles, read, k, count):
    """Per student, the calls the library had before: median ms of each part."""
    n = index.ntotal
    nbytes = (n + 7) // 8
    parts = {"reconstruct": [], "mean": [], "selector": [], "search": [], "total": []}
    for (labels, weights), seen in list(zip(profiles, read))[:count]:
        t0 = time.perf_counter()
        rows = [index.reconstruct(int(l)) for l in labels]
        t1 = time.perf_counter()
        total = 0.0
        for w in weights:
            total += float(w)
        q = np.sum([r * w for r, w in zip(rows, weights)], axis=0) / np.float32(total)
        t2 = time.perf_counter()
        bitmap = np.full(nbytes, 0xFF, dtype=np.uint8)
        for l in np.concatenate([labels, seen]):
            bitmap[l >> 3] &= ~np.uint8(1 << (l & 7))
        sel = vfaiss.Selector(index, bitmap, n)
        t3 = time.perf_counter()
        index.search(q[None, :], k, params=vfaiss.SearchParameters(sel=sel))
        t4 = time.perf_counter()
        sel.close()
        for name, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
            parts[name].append(dt * 1e3)
    out = {name: round(float(np.median(v)), 4) for name, v in parts.items()}
    return out


def main():
    import torch

    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=10_000_000)
    p.add_argument("--d", type=int, default=1536)
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--steps", type=int, default=7)
    p.add_argument("--baseline", type=int, default=0,
                   help="serve this many students one at a time, the earlier way, and stop")
    a = p.parse_args()
    n, d, k, B = a.n, a.d, a.k, a.batch
    index = vfaiss.IndexFlat(d, vfaiss.METRIC_L2)
    index.reserve(n)
    index.add_synthetic(n, seed=SEED)
    profiles, read = students(n, B)

    if a.baseline:
        parts = baseline(index, profiles, read, k, a.baseline)
        print(json.dumps({"case": "per student: reconstruct, host mean, selector, search_sel",
                          "n": n, "d": d, "k": k, "students": min(a.baseline, B),
                          "ms_per_student": parts,
                          "qps": round(1e3 / parts["total"], 1)}), flush=True)
        return

    sizes = np.asarray([np.unique(np.concatenate([pl, r])).size
                        for (pl, _), r in zip(profiles, read)])
    classes = {f"<={c}": int(((sizes <= c) & (sizes > lo)).sum())
               for lo, c in zip((-1,) + CAPS[:-1], CAPS)}
    profile_bytes = int(sum(pl.size for pl, _ in profiles)) * d * 4

    def timed(fn):
        _lib.timer_enable(True)
        _lib.timer_reset()
        ms = median_ms(fn, a.steps, warmup=0)
        spans = {s: span_ms(s, a.steps) for s in ("mean_rows", "excl_topk", "excl_drop")}
        _lib.timer_enable(False)
        _lib.timer_reset()
        return ms, spans

    # the ceiling first: plain vs_search of the same means, device buffers, on an
    # index no exclusion search has touched yet (the staged engine adapts its
    # plane order per index to the searches it has seen)
    means = torch.empty((B, d), dtype=torch.float32, device="cuda")
    index.mean_rows_device(profiles, means.data_ptr())
    torch.cuda.synchronize()
    offs, labels = vfaiss.exclusion_csr([np.concatenate([pl, r])
                                         for (pl, _), r in zip(profiles, read)], B)
    D = torch.empty((B, k), dtype=torch.float32, device="cuda")
    I = torch.empty((B, k), dtype=torch.int64, device="cuda")
    lib = _lib.load()
    flags = _lib.IN_DEVICE | _lib.OUT_DEVICE

    def plain():
        index.search_device(means.data_ptr(), B, k, D.data_ptr(), I.data_ptr())

    def report_plain(case):
        ms = median_ms(plain, a.steps)
        print(json.dumps({"case": case, "batch": B, "k": k, "kernel": _lib.timer_kernel(),
                          "ms": round(ms, 3), "qps": round(B / ms * 1e3, 1)}), flush=True)

    report_plain("plain vs_search of the same means")

    # the batched call, as a caller without device buffers makes it
    for _ in range(2):
        index.search_profiles(profiles, k, exclude=read)
    ms, sp = timed(lambda: index.search_profiles(profiles, k, exclude=read))
    out = {"case": "search_profiles", "n": n, "d": d, "batch": B, "k": k, "ms": round(ms, 3),
           "qps": round(B / ms * 1e3, 1), "exclusion_classes": classes,
           "mean_ms": round(sp["mean_rows"], 4), "drop_ms": round(sp["excl_drop"], 4),
           "engine_ms": round(sp["excl_topk"], 3),
           "outside_engine_share": round(1.0 - sp["excl_topk"] / ms, 4)}
    if sp["mean_rows"]:
        out["mean_TBps"] = round(profile_bytes / (sp["mean_rows"] * 1e-3) / 1e12, 3)
        out["mean_bytes"] = profile_bytes
    print(json.dumps(out), flush=True)

    def excl():
        _lib.check(lib.vs_search_excl(index._h, ctypes.c_void_p(means.data_ptr()), B, k,
                                      offs.ctypes.data, labels.ctypes.data,
                                      ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(I.data_ptr()),
                                      flags, None))

    for _ in range(2):
        excl()
    ms, sp = timed(excl)
    print(json.dumps({"case": "search_excl, means on the device", "batch": B, "k": k,
                      "ms": round(ms, 3), "qps": round(B / ms * 1e3, 1),
                      "drop_ms": round(sp["excl_drop"], 4),
                      "engine_ms": round(sp["excl_topk"], 3)}), flush=True)

    # the same plain search again: the exclusion searches' deeper lists hand more
    # queries from the int8 plane to the bf16 plane, and the index's adaptive
    # plane order carries that over to the searches that follow
    report_plain("plain vs_search again, after the exclusion searches")


if __name__ == "__main__":
    main()
