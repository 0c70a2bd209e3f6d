"""CPU: the host side of range search (faiss range_search).

The C-ABI's argument checks run before any device call, so they are tested
without a GPU.  The store methods (``similarity_search_within_score*``) and the
chunk concatenation of ``IndexFlat.range_search`` are host logic: the store runs
over a test double (OracleIndex plus a numpy ``range_search``), the chunking
over a fake of the one C call it makes.  The arithmetic on the device is
test_gpu_range.py's."""

import ctypes

import numpy as np
import pytest

from helpers import OracleIndex
from oracle import flat
from vsearch import _lib
from vsearch import faiss as vfaiss
from vsearch import langchain as vlc
from vsearch.synth import SynthEmbeddings

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
RANGE_SYMBOLS = ("vs_range_search", "vs_range_size", "vs_range_candidates", "vs_range_copy",
                 "vs_range_destroy")


class RangeOracleIndex(OracleIndex):
    """OracleIndex with faiss's range_search in numpy: fp32 roundings of the
    fp64 scores, strict comparisons, ascending labels, params.sel honoured."""

    def range_search(self, x, thresh, *, params=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.shape[1] == self.d
        s = flat.exact_scores(self._x, x, self.metric_type).astype(np.float32)
        thresh = np.float32(thresh)
        hit = s > thresh if self.metric_type == IP else s < thresh
        sel = getattr(params, "sel", None) if params is not None else None
        if sel is not None:
            labels = np.arange(self.ntotal, dtype=np.int64) + self._base
            hit &= vfaiss._members(sel, labels)[None, :]
        lims = np.zeros(x.shape[0] + 1, dtype=np.uint64)
        lims[1:] = np.cumsum(hit.sum(axis=1))
        q, r = np.nonzero(hit)  # row-major: ascending labels inside each query
        return lims, s[q, r], r.astype(np.int64) + self._base


@pytest.fixture
def patched_indexes(monkeypatch):
    monkeypatch.setattr(vfaiss, "IndexFlatL2", lambda d, **kw: RangeOracleIndex(d, L2))
    monkeypatch.setattr(vfaiss, "IndexFlatIP", lambda d, **kw: RangeOracleIndex(d, IP))


def test_symbols_exported_and_in_signatures():
    lib = _lib.load()
    for name in RANGE_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int, name


def test_argument_checks_are_host_side():
    lib = _lib.load()
    out = ctypes.c_void_p()
    x = np.zeros((1, 8), dtype=np.float32)
    assert lib.vs_range_search(None, None, x.ctypes.data, 1, 1.0, 0, None,
                               ctypes.byref(out)) == _lib.E_INVALID
    assert "null index" in _lib.last_error()
    assert not out.value
    # a null `out` (checked before the index is looked at)
    assert lib.vs_range_search(None, None, x.ctypes.data, 1, 1.0, 0, None, None) == _lib.E_INVALID
    assert "null output" in _lib.last_error()
    assert lib.vs_range_search(None, None, x.ctypes.data, -1, 1.0, 0, None,
                               ctypes.byref(out)) == _lib.E_INVALID
    nq, total = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.vs_range_size(None, ctypes.byref(nq), ctypes.byref(total)) == _lib.E_INVALID
    assert lib.vs_range_copy(None, None, None, None, 0, None) == _lib.E_INVALID
    assert lib.vs_range_destroy(None) == 0


def _store(strategy, n=40, d=16):
    texts = [f"doc{i}" for i in range(n)]
    metas = [{"genre": "a" if i % 2 else "b", "level": i} for i in range(n)]
    store = vlc.FAISS.from_texts(texts, SynthEmbeddings(d), metadatas=metas,
                                 distance_strategy=strategy)
    return store, texts


@pytest.mark.parametrize("strategy,metric", [
    (vlc.DistanceStrategy.EUCLIDEAN_DISTANCE, L2),
    (vlc.DistanceStrategy.MAX_INNER_PRODUCT, IP),
])
def test_store_within_score_order_direction_and_strictness(patched_indexes, strategy, metric):
    store, texts = _store(strategy)
    assert store.index.metric_type == metric
    n = store.index.ntotal
    full = store.similarity_search_with_score("doc7", k=n)  # best first
    scores = np.array([s for _, s in full], dtype=np.float32)
    # a threshold equal to a score that occurs: the strict comparison leaves it out
    t = scores[9]
    want = [(d.page_content, s) for d, s in full if (s > t if metric == IP else s < t)]
    assert 0 < len(want) <= 9
    got = store.similarity_search_within_score("doc7", float(t))
    assert [(d.page_content, s) for d, s in got] == want
    assert got[0][0].page_content == "doc7"
    key = np.array([-s if metric == IP else s for _, s in got])
    assert (np.diff(key) >= 0).all(), "not best first"
    assert isinstance(got[0][1], np.floating)
    # one ulp past it: the document at the threshold is in
    t1 = np.nextafter(t, np.float32(-np.inf if metric == IP else np.inf))
    got1 = store.similarity_search_within_score("doc7", float(t1))
    assert len(got1) == int((scores >= t).sum() if metric == IP else (scores <= t).sum())
    assert len(got1) > len(got)
    # by_vector is the same search
    vec = store._embed_query("doc7")
    assert [(d.page_content, s) for d, s in
            store.similarity_search_within_score_by_vector(vec, float(t))] == want


def test_store_within_score_ties_come_by_label(patched_indexes):
    class Stub:
        def embed_documents(self, texts, **_):
            return [[float(i % 3)] * 3 for i, _ in enumerate(texts)]

        def embed_query(self, text):
            return [0.0, 0.0, 0.0]

    store = vlc.FAISS.from_texts([f"book {i}" for i in range(10)], Stub())
    got = store.similarity_search_within_score("anything", 3.5)
    # distances 0 (labels 0, 3, 6, 9) then 3 (labels 1, 4, 7); 12 is out
    assert [d.page_content for d, _ in got] == [f"book {i}" for i in (0, 3, 6, 9, 1, 4, 7)]
    assert [float(s) for _, s in got] == [0.0] * 4 + [3.0] * 3
    assert [d.page_content for d, _ in store.similarity_search_within_score("anything", 3.0)] == \
        [f"book {i}" for i in (0, 3, 6, 9)]


def test_store_within_score_filter_and_empty(patched_indexes):
    store, _ = _store(vlc.DistanceStrategy.EUCLIDEAN_DISTANCE)
    n = store.index.ntotal
    full = store.similarity_search_with_score("doc7", k=n)
    t = float(full[19][1])
    for flt, ok in (({"genre": "a"}, lambda m: m["genre"] == "a"),
                    ({"level": {"$gte": 20}}, lambda m: m["level"] >= 20),
                    (lambda m: m["level"] % 3 == 0, lambda m: m["level"] % 3 == 0)):
        want = [d.page_content for d, s in full if s < t and ok(d.metadata)]
        got = store.similarity_search_within_score("doc7", t, filter=flt)
        assert [d.page_content for d, _ in got] == want
        assert want, "the filter case is vacuous"
    assert store.similarity_search_within_score("doc7", 0.0) == []  # nothing is < 0
    assert store.similarity_search_within_score("doc7", t, filter={"genre": "none"}) == []


def _bare_index(d):
    """An IndexFlat without a device: range_search needs only _d, the chunk size
    and the one C call, which the tests replace."""
    index = object.__new__(vfaiss.IndexFlat)
    index._d = d
    index._h = None
    return index


def test_range_search_chunks_concatenate(monkeypatch):
    d, n = 4, 11
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, d)).astype(np.float32)
    calls = []

    def fake_call(self, xc, thresh, sel_handle):
        # query j (global) has j % 4 hits: labels 100 j + i, scores its first element + i
        q0 = int(np.nonzero((x == xc[0]).all(axis=1))[0][0])
        calls.append((q0, xc.shape[0], thresh, sel_handle))
        counts = [(q0 + j) % 4 for j in range(xc.shape[0])]
        lims = np.zeros(xc.shape[0] + 1, dtype=np.int64)
        lims[1:] = np.cumsum(counts)
        D = np.array([xc[j, 0] + i for j, c in enumerate(counts) for i in range(c)],
                     dtype=np.float32)
        I = np.array([100 * (q0 + j) + i for j, c in enumerate(counts) for i in range(c)],
                     dtype=np.int64)
        return lims, D, I

    monkeypatch.setattr(vfaiss.IndexFlat, "_RANGE_CHUNK", 4)
    monkeypatch.setattr(vfaiss.IndexFlat, "_range_call", fake_call)
    index = _bare_index(d)
    lims, D, I = index.range_search(x, 0.25)
    assert [(c[0], c[1]) for c in calls] == [(0, 4), (4, 4), (8, 3)]
    assert all(c[2] == 0.25 and c[3] is None for c in calls)
    assert lims.dtype == np.uint64 and D.dtype == np.float32 and I.dtype == np.int64
    counts = [j % 4 for j in range(n)]
    np.testing.assert_array_equal(lims, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64))
    for j in range(n):
        a, b = int(lims[j]), int(lims[j + 1])
        np.testing.assert_array_equal(I[a:b], 100 * j + np.arange(counts[j]))
        np.testing.assert_array_equal(D[a:b], x[j, 0] + np.arange(counts[j], dtype=np.float32))
    # one chunk: the call's arrays, lims as uint64
    calls.clear()
    monkeypatch.setattr(vfaiss.IndexFlat, "_RANGE_CHUNK", 65536)
    lims1, D1, I1 = index.range_search(x, 0.25)
    assert len(calls) == 1
    np.testing.assert_array_equal(lims1, lims)
    np.testing.assert_array_equal(D1, D)
    np.testing.assert_array_equal(I1, I)


def test_range_search_short_tail_borrows_and_empty_batch(monkeypatch):
    """A tail of fewer than 20 queries would switch the L2 key's formula (faiss
    decides on the call's size): it borrows 20 queries from the chunk before."""
    sizes = []

    def fake_call(self, xc, thresh, sel_handle):
        sizes.append(xc.shape[0])
        return (np.zeros(xc.shape[0] + 1, dtype=np.int64), np.empty(0, dtype=np.float32),
                np.empty(0, dtype=np.int64))

    monkeypatch.setattr(vfaiss.IndexFlat, "_RANGE_CHUNK", 100)
    monkeypatch.setattr(vfaiss.IndexFlat, "_range_call", fake_call)
    index = _bare_index(3)
    lims, D, I = index.range_search(np.zeros((205, 3), dtype=np.float32), 1.0)
    assert sizes == [100, 80, 25]
    assert lims.shape == (206,) and not lims.any() and D.size == 0 and I.size == 0
    sizes.clear()
    lims, D, I = index.range_search(np.zeros((0, 3), dtype=np.float32), 1.0)
    assert sizes == [] and lims.tolist() == [0] and lims.dtype == np.uint64
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.size == 0 and I.size == 0
