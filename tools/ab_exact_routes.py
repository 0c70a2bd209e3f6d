"""Bit-for-bit A/B of the exact routes between two builds of libvsearch.

    python3 tools/ab_exact_routes.py LIB_A LIB_B [--out FILE]

Each library runs in a fresh process of its own (selected with VSEARCH_LIB, as
tools/ab_x1.sh does), under its own timeout, the second only if the first ended
well.  A process runs a fixed list of calls on fixed seeds and prints one line
per call: the call's name, the kernel that served it and a sha256 of its D, I
(and lims for the range calls).  The parent writes both runs side by side and
marks every line equal or DIFFERENT; it exits 1 on any difference.  The first
HIP error ends a run (vsearch raises on it).

The shapes are small but reach every edge of the exact MFMA tile's loop
(csrc/vs_exact_tile.h): d = 64 (two stages for fp32, ONE for bf16) and d = 192;
300 rows (three tiles, the last with 44 live rows) and 3,000 rows (more than
one split); 130 queries (two query tiles, padded), 5 queries and 1 query.

`--child` is the per-library mode the parent starts."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "book-recommendation-engine_amd"))
sys.path.insert(0, ROOT)


def _sha(*arrays):
    import numpy as np

    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:32]


def child():
    import numpy as np

    from vsearch import _lib
    from vsearch import faiss as vf

    L2, IP = vf.METRIC_L2, vf.METRIC_INNER_PRODUCT
    mname = {L2: "L2", IP: "IP"}

    def rand(n, d, seed):
        return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)

    def say(name, *arrays):
        print(f"{name:58s} {_lib.timer_kernel():18s} {_sha(*arrays)}", flush=True)

    def index_of(xb, metric, dtype, engine="fp32"):
        index = vf.IndexFlat(xb.shape[1], metric, dtype=dtype)
        index.add(xb)
        index.set_engine(engine)
        return index

    shapes = [(d, n) for d in (64, 192) for n in (300, 3000)]
    # gemm_topk (130 queries) and gemv_topk (5 and 1 queries; batch 2 below)
    for d, n in shapes:
        xb = rand(n, d, 100 + d + n)
        for dtype in ("f32", "bf16"):
            for metric in (IP, L2):
                index = index_of(xb, metric, dtype)
                for nq in (130, 5, 2, 1):
                    xq = rand(nq, d, 7 + nq)
                    ks = (10, 40) if nq >= 5 else (10,)
                    for k in ks:
                        say(f"search d{d} n{n} {dtype} {mname[metric]} nq{nq} k{k}",
                            *index.search(xq, k))
                    if metric == IP or nq <= 2:  # the FLOOR pages
                        say(f"search d{d} n{n} {dtype} {mname[metric]} nq{nq} k100",
                            *index.search(xq, 100))
        # cosine self-join on an L2 index (gemm_topk MODE_COS, self0)
        index = index_of(xb, L2, "f32")
        say(f"selfjoin d{d} n{n} f32 k15", *index.selfjoin(15))

    # gemm_topk_rows / gemv_topk_rows: selector route (c), the gathered kernels
    # (more than 256 rows left out; fewer take the drop route (b) through the
    # unselected engine, which the searches above cover)
    for d, n, nsel in ((64, 300, 40), (192, 300, 40), (64, 3000, 1700), (192, 3000, 1700)):
        xb = rand(n, d, 200 + d + n)
        mask = np.zeros(n, dtype=bool)
        mask[np.random.default_rng(n).choice(n, nsel, replace=False)] = True
        for dtype in ("f32", "bf16"):
            for metric in (IP, L2):
                index = index_of(xb, metric, dtype, engine="auto")
                sel = index.selector(vf.IDSelectorBitmap(n, np.packbits(mask, bitorder="little")))
                for nq in (130, 5):
                    xq = rand(nq, d, 17 + nq)
                    for k in (10, 40) if metric == L2 else (10,):
                        say(f"search_sel d{d} {nsel}/{n} {dtype} {mname[metric]} nq{nq} k{k}",
                            *index.search(xq, k, params=vf.SearchParameters(sel=sel)))

    # gemm_range: range_search, and the range self-join on clustered rows
    for d, n in shapes:
        xb = rand(n, d, 300 + d + n)
        for dtype in ("f32", "bf16"):
            for metric in (IP, L2):
                index = index_of(xb, metric, dtype, engine="auto")
                for nq in (130, 1):
                    xq = rand(nq, d, 27 + nq)
                    thr = (0.25 * d) if metric == IP else (1.6 * d)
                    say(f"range_search d{d} n{n} {dtype} {mname[metric]} nq{nq}",
                        *index.range_search(xq, thr))
    rng = np.random.default_rng(1)
    centres = rng.standard_normal((40, 96))
    x = (centres[rng.integers(0, 40, 3000)] + 0.35 * rng.standard_normal((3000, 96)))
    for dtype in ("f32", "bf16"):
        index = vf.IndexFlatIP(96, dtype=dtype)
        index.add(np.ascontiguousarray(x.astype(np.float32)))
        for upper in (False, True):
            say(f"range_selfjoin clustered n3000 {dtype} upper={upper}",
                *index.range_selfjoin(0.8, upper=upper))

    # the qlist-gathered gemm_topk: staged default searches on 150,000 scaled
    # copies of one row (tests/test_gpu_dump.py).  Spaced 1 + 0.3 pos / N
    # (test_dump_slot_overflow_hands_queries_on) the exact fp32 stage answers
    # the queries handed to it: the hash is the gathered launch's output.
    # Spaced 1 + 1e-3 pos / N (test_dense_near_ties_reach_the_exact_stream)
    # its bound proves nothing and the exact-key stream rewrites its lists.
    N, D_, B = 300_000, 128, 4096
    os.environ["VS_X1_CHUNK_TILES"] = "8"
    for name, step in (("spaced copies", 0.3), ("dense near-ties", 1e-3)):
        rng = np.random.default_rng(77)
        xb = rng.uniform(-1, 1, (N, D_)).astype(np.float32)
        dup = rng.uniform(-1, 1, D_).astype(np.float32)
        pos = np.sort(rng.choice(N, 150_000, replace=False))
        xb[pos] = dup[None, :] * (1.0 + step * pos[:, None] / N).astype(np.float32)
        xq = (dup[None, :] + 0.3 * rng.uniform(-1, 1, (B, D_))).astype(np.float32)
        index = vf.IndexFlat(D_, IP)
        index.add(xb)
        _lib.filter_stats(reset=True)
        D, I = index.search(xq, 10)
        streamed = _lib.filter_exact_stats()
        staged, redone = _lib.filter_stats(reset=True)
        say(f"staged search, {name} n{N} nq{B} k10", D, I)
        print(f"staged search, {name}: {staged} queries, {redone} redone by the gathered "
              f"gemm_topk, {streamed} of them then streamed by exact key", flush=True)
        del index
    print("END", flush=True)


def run(lib, seconds):
    env = dict(os.environ, VSEARCH_LIB=os.path.abspath(lib))
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-u",
                        os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                       text=True)
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    ok = p.returncode == 0 and lines and lines[-1] == "END"
    return ok, p.returncode, lines[:-1] if ok else lines, p.stderr[-2000:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--labels", nargs=2, default=None, metavar=("A", "B"),
                    help="what to call the two libraries in the output (default: their paths)")
    a = ap.parse_args()
    if a.child:
        return child()
    if len(a.libs) != 2:
        ap.error("two libraries")
    la_, lb_ = a.labels or a.libs
    out = [f"# A = {la_}", f"# B = {lb_}"]
    oka, rca, la, erra = run(a.libs[0], a.timeout)
    if not oka:  # nothing more on the GPU after a run that did not end well
        out += [f"# A ended with status {rca}; B not started"] + la + [erra]
        status = 2
    else:
        okb, rcb, lb, errb = run(a.libs[1], a.timeout)
        ndiff = 0
        for i in range(max(len(la), len(lb))):
            x = la[i] if i < len(la) else "(missing)"
            y = lb[i] if i < len(lb) else "(missing)"
            same = x == y
            ndiff += not same
            out.append(f"{x}  {'equal' if same else 'DIFFERENT: B ' + y}")
        if not okb:
            out += [f"# B ended with status {rcb}", errb]
        out.append(f"# {len(la)} calls, {ndiff} different")
        status = 0 if okb and ndiff == 0 else 1
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return status


if __name__ == "__main__":
    sys.exit(main())
