"""GPU: the 65,536-query seam of the staged-query loop (vs_host.h
search_staged), under each of its callers.

``IndexFlat.search`` does not chunk, so one call of 65,536 + 40 queries makes
the library stage two chunks: a full one, and one of 40 queries padded to a
query tile.  d = 64 fills the staged rows (d == ld: only the padding rows are
zeroed); d = 24 leaves a column tail (the whole buffer is zeroed and the
copy is pitched).  bf16 indexes add the rounded copy of every chunk.

Oracle: ``flat.select_topk`` over the fp64 scores (``valid=`` a mask where the
case has one), compared with ``flat.mismatches_vec`` (``flat.mismatches``'s
checks on arrays: 65,576 queries) — the fp32 contract, as test_gpu_selector.py
and test_gpu_profiles.py.  Neither checks membership, so every returned label
is checked against its mask too.  The scores of one (metric, storage, d) are
computed once and shared by its four cases."""

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
CHUNK = 65536
NQ, N, K = CHUNK + 40, 600, 5
ROWS_KERNELS = ("gemv_topk_rows", "gemm_topk_rows")


class _Case:
    pass


@pytest.fixture(scope="module", params=[(m, t, d) for m in (IP, L2) for t in ("f32", "bf16")
                                        for d in (64, 24)],
                ids=lambda p: f"{'IP' if p[0] == IP else 'L2'}-{p[1]}-d{p[2]}")
def case(request):
    from vsearch import _lib
    from vsearch import faiss as vfaiss

    assert _lib.device_count() >= 1
    metric, dtype, d = request.param
    rng = np.random.default_rng(d)
    c = _Case()
    c.vf, c.metric = vfaiss, metric
    c.xb = rng.standard_normal((N, d)).astype(np.float32)
    c.xq = rng.standard_normal((NQ, d)).astype(np.float32)
    c.ob, c.oq = (flat.round_bf16(c.xb), flat.round_bf16(c.xq)) if dtype == "bf16" else (c.xb, c.xq)
    c.scores = flat.exact_scores(c.ob, c.oq, metric)
    c.plain = flat.select_topk(c.scores, K, metric)
    c.index = vfaiss.IndexFlat(d, metric, dtype=dtype)
    c.index.add(c.xb)
    for a in (c.xb, c.xq, c.scores, *c.plain):
        a.setflags(write=False)
    return c


def _parity(c, D, I, Dr, Ir):
    assert D.shape == (NQ, K) and I.shape == (NQ, K)
    bad = flat.mismatches_vec(D, I, Dr, Ir, c.metric, c.ob, c.oq)
    assert not bad, bad[:5]


def test_search_across_the_seam(case):
    D, I = case.index.search(case.xq, K)
    _parity(case, D, I, *case.plain)


@pytest.mark.parametrize("route", ["drop", "rows"])
def test_selector_search_across_the_seam(case, route):
    """"drop": 100 rows left out, route (b) (the unselected engine, then the
    drop); "rows": 300 rows kept, route (c) (the gathered MFMA kernel).  On an
    fp32 index "drop" takes ~16 s on one MI355X (65,576 queries at k + 100
    entries over 600 rows); every other case of this module is under a second."""
    from vsearch import _lib

    rng = np.random.default_rng(1)
    mask = np.zeros(N, dtype=bool)
    mask[rng.choice(N, 300 if route == "rows" else N - 100, replace=False)] = True
    vf = case.vf
    sel = case.index.selector(vf.IDSelectorBitmap(N, np.packbits(mask, bitorder="little")))
    assert sel.count == int(mask.sum())
    D, I = case.index.search(case.xq, K, params=vf.SearchParameters(sel=sel))
    name = _lib.timer_kernel()
    if route == "rows":
        assert name == "gemm_topk_rows", name
    else:
        assert name not in ROWS_KERNELS, name
    assert mask[I[I >= 0]].all(), "a label outside the selection"
    Dr, Ir = flat.select_topk(case.scores, K, case.metric,
                              valid=np.broadcast_to(mask[None, :], (NQ, N)))
    _parity(case, D, I, Dr, Ir)


def test_excluded_search_across_the_seam(case):
    """The last query of the first chunk and the first of the second carry
    different lists (their own nearest rows, so the drop changes the answer),
    as do the first and last queries of the call; every other list is empty
    (their oracle rows are the plain search's)."""
    rng = np.random.default_rng(2)
    near = {q: case.plain[1][q] for q in (0, CHUNK - 1, CHUNK, NQ - 1)}
    lists = {
        0: near[0][:2],
        CHUNK - 1: np.concatenate([near[CHUNK - 1][:3], [7, 11]]),
        # 20 rows: past the first class of the engine's cap table (16)
        CHUNK: np.union1d(near[CHUNK][:4], rng.choice(N, 16, replace=False))[:20],
        NQ - 1: near[NQ - 1][:1],
    }
    assert not np.array_equal(np.sort(lists[CHUNK - 1]), np.sort(lists[CHUNK]))
    offs = np.zeros(NQ + 1, dtype=np.int64)
    for q, rows in lists.items():
        offs[q + 1] = len(rows)
    offs = np.cumsum(offs)
    labels = np.concatenate([lists[q] for q in sorted(lists)]).astype(np.int64)
    D, I = case.index.search(case.xq, K, exclude=(offs, labels))
    Dr, Ir = (a.copy() for a in case.plain)
    for q, rows in lists.items():
        valid = np.ones((1, N), dtype=bool)
        valid[0, rows] = False
        Dr[q], Ir[q] = (a[0] for a in flat.select_topk(case.scores[q:q + 1], K, case.metric,
                                                        valid=valid))
        assert not np.isin(I[q], rows).any(), (q, "an excluded label came back")
        assert not np.array_equal(Ir[q], case.plain[1][q]), q  # the list matters
    _parity(case, D, I, Dr, Ir)
