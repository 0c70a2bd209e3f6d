"""CPU: the host half of selector searches — the faiss IDSelector classes and
their label bitmap, the LangChain store's ``exact_filter`` and its passage
through the index service.  The index is the oracle-backed test double with a
``params=`` search that masks through ``flat.select_topk(valid=...)``; the same
calls run on the GPU in test_gpu_selector.py."""

import numpy as np
import pytest

from helpers import OracleIndex
from oracle import flat
from vsearch import faiss as vfaiss
from vsearch import langchain as vlc
from vsearch.service import IndexService, RemoteFAISS
from vsearch.synth import SynthEmbeddings

KEY = b"test-secret"
SIZES = [0, 1, 7, 8, 9, 1000]


class SelOracleIndex(OracleIndex):
    """OracleIndex whose search takes faiss's ``params=SearchParameters(sel=)``."""

    searches = 0

    def search(self, x, k, params=None, raw=False):
        sel = getattr(params, "sel", None) if params is not None else None
        if sel is None:
            return super().search(x, k, raw=raw)
        type(self).searches += 1
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.ntotal
        bits = vfaiss.selector_bitmap(sel, n, self._base)
        mask = np.unpackbits(bits, bitorder="little")[:n].astype(bool)
        valid = np.broadcast_to(mask, (x.shape[0], n))
        D, I = flat.select_topk(flat.exact_scores(self._x, x, self.metric_type), k,
                                self.metric_type, valid=valid, rule="lex" if raw else "faiss")
        return D, np.where(I >= 0, I + self._base, -1)


def _selectors(n, rng):
    ids = rng.integers(-3, n + 5, size=max(1, n // 3))
    bits = np.packbits(rng.random(n) < 0.4, bitorder="little")
    a = vfaiss.IDSelectorRange(n // 4, 3 * n // 4 + 1)
    b = vfaiss.IDSelectorArray(ids)
    c = vfaiss.IDSelectorBitmap(n, bits)
    d = vfaiss.IDSelectorBatch(ids[::2])
    return {
        "all": vfaiss.IDSelectorAll(),
        "range": a,
        "empty_range": vfaiss.IDSelectorRange(5, 5),
        "array": b,
        "bitmap": c,
        "batch": d,
        "not": vfaiss.IDSelectorNot(b),
        "and": vfaiss.IDSelectorAnd(a, c),
        "or": vfaiss.IDSelectorOr(b, c),
        "nested": vfaiss.IDSelectorOr(vfaiss.IDSelectorAnd(a, vfaiss.IDSelectorNot(c)),
                                      vfaiss.IDSelectorNot(vfaiss.IDSelectorOr(b, d))),
    }


@pytest.mark.parametrize("id_base", [0, 1000])
@pytest.mark.parametrize("n", SIZES)
def test_bitmap_equals_is_member(n, id_base):
    rng = np.random.default_rng(n + id_base)
    for name, sel in _selectors(n + id_base, rng).items():
        bits = vfaiss.selector_bitmap(sel, n, id_base)
        assert bits.dtype == np.uint8 and bits.size == (n + 7) // 8, name
        want = np.array([sel.is_member(id_base + i) for i in range(n)], dtype=bool)
        got = np.unpackbits(bits, bitorder="little")[:n].astype(bool)
        np.testing.assert_array_equal(got, want, err_msg=name)
        # the bits past n in the last byte are clear
        assert not np.unpackbits(bits, bitorder="little")[n:].any(), name


def test_range_is_half_open_and_array_keeps_duplicates():
    r = vfaiss.IDSelectorRange(3, 6)
    assert [r.is_member(i) for i in range(2, 8)] == [False, True, True, True, False, False]
    a = vfaiss.IDSelectorArray([4, 4, 9])
    assert a.is_member(4) and a.is_member(9) and not a.is_member(5)
    assert vfaiss.SearchParameters().sel is None
    assert vfaiss.SearchParameters(sel=r).sel is r


@pytest.mark.parametrize("n", SIZES)
def test_bitmap_round_trip(n):
    rng = np.random.default_rng(100 + n)
    mask = rng.random(n) < 0.5
    bits = np.packbits(mask, bitorder="little")
    sel = vfaiss.IDSelectorBitmap(n, bits)
    np.testing.assert_array_equal(vfaiss.selector_bitmap(sel, n), bits)
    # faiss's layout: label i is bit (i & 7) of byte (i >> 3)
    for i in range(min(n, 40)):
        assert sel.is_member(i) == bool((bits[i >> 3] >> (i & 7)) & 1)
    assert not sel.is_member(n) and not sel.is_member(-1)
    # a longer index than the bitmap: labels past n are not selected
    longer = vfaiss.selector_bitmap(sel, n + 13)
    got = np.unpackbits(longer, bitorder="little")[:n + 13].astype(bool)
    np.testing.assert_array_equal(got[:n], mask)
    assert not got[n:].any()


def test_oracle_is_deterministic_on_tied_integer_data():
    """The tie tests of test_gpu_selector.py demand exact equality with the
    masked select_topk: it must itself be a function of its inputs, and its L2
    order the plain (distance, label) order over the selected rows."""
    rng = np.random.default_rng(5)
    xb = rng.integers(-2, 3, size=(600, 3)).astype(np.float32)
    xq = rng.integers(-2, 3, size=(7, 3)).astype(np.float32)
    mask = rng.random(600) < 0.5
    valid = np.broadcast_to(mask, (7, 600))
    for metric in (flat.METRIC_L2, flat.METRIC_INNER_PRODUCT):
        s = flat.exact_scores(xb, xq, metric)
        for k in (1, 5, 16, 32):
            D1, I1 = flat.select_topk(s, k, metric, valid=valid)
            D2, I2 = flat.select_topk(s.copy(), k, metric, valid=valid.copy())
            np.testing.assert_array_equal(I1, I2)
            np.testing.assert_array_equal(D1, D2)
            assert mask[I1[I1 >= 0]].all()
            if metric == flat.METRIC_L2:
                for q in range(7):
                    rows = np.nonzero(mask)[0]
                    order = rows[np.lexsort((rows, s[q, rows]))][:k]
                    np.testing.assert_array_equal(I1[q], order)


# ---- the LangChain store -----------------------------------------------------------


@pytest.fixture
def store(monkeypatch):
    monkeypatch.setattr(vfaiss, "IndexFlatL2", lambda d, **kw: SelOracleIndex(d, flat.METRIC_L2))
    monkeypatch.setattr(vfaiss, "IndexFlatIP",
                        lambda d, **kw: SelOracleIndex(d, flat.METRIC_INNER_PRODUCT))
    emb = SynthEmbeddings(48)
    texts = [f"book {i}" for i in range(300)]
    metas = [{"book_id": f"B{i:03d}", "genre": ["fantasy", "mystery", "science"][i % 3],
              "level": i % 7} for i in range(300)]
    return vlc.FAISS.from_texts(texts, emb, metadatas=metas)


def _nearest_ids(store, vec, n):
    return [d.metadata["book_id"]
            for d in store.similarity_search_by_vector(vec, k=n)]


def test_exact_filter_returns_k_where_fetch_k_filtering_returns_fewer(store):
    vec = store.embedding_function.embed_query("book 17")
    read = _nearest_ids(store, vec, 25)  # a heavy reader: the 25 nearest books are read
    flt = {"book_id": {"$nin": read}}
    loose = store.similarity_search_by_vector(vec, k=10, filter=flt)  # fetch_k = 20
    assert len(loose) == 0
    exact = store.similarity_search_with_score_by_vector(vec, k=10, filter=flt,
                                                         exact_filter=True)
    assert len(exact) == 10
    assert not {d.metadata["book_id"] for d, _ in exact} & set(read)
    # they are the 10 nearest unread books: the unfiltered order with the read ones dropped
    want = [b for b in _nearest_ids(store, vec, 300) if b not in read][:10]
    assert [d.metadata["book_id"] for d, _ in exact] == want
    # fewer matches than k: exactly the matches
    few = store.similarity_search_by_vector(vec, k=10, filter={"book_id": ["B003", "B250", "nope"]},
                                            exact_filter=True)
    assert sorted(d.metadata["book_id"] for d in few) == ["B003", "B250"]
    # score_threshold still applies afterwards
    thr = float(exact[4][1])
    cut = store.similarity_search_with_score_by_vector(vec, k=10, filter=flt, exact_filter=True,
                                                       score_threshold=thr)
    assert [d.id for d, _ in cut] == [d.id for d, _ in exact[:len(cut)]]
    assert 5 <= len(cut) < 10 and all(s <= thr for _, s in cut)
    # the text-query forms pass it on
    docs = store.similarity_search("book 17", k=10, filter=flt, exact_filter=True)
    assert [d.id for d in docs] == [d.id for d, _ in exact]


@pytest.mark.parametrize("flt", [
    {"genre": "mystery"},
    {"genre": ["mystery", "science"]},
    {"genre": {"$eq": "fantasy"}},
    {"genre": {"$neq": "fantasy"}},
    {"level": {"$in": [1, 2, 99]}},
    {"level": {"$nin": [0, 3]}},
    {"book_id": {"$nin": []}},
    {"genre": "no such genre"},
])
def test_key_index_path_equals_scan_path(store, flt):
    assert vlc.FAISS._key_index_values(flt) is not None
    fast = store._filter_mask(flt, use_key_index=True)
    scan = store._filter_mask(flt, use_key_index=False)
    np.testing.assert_array_equal(fast, scan)
    fn = vlc._create_filter_func(flt)
    want = [fn(store.docstore.search(store.index_to_docstore_id[i]).metadata)
            for i in range(300)]
    np.testing.assert_array_equal(scan, want)


def test_other_filters_scan_once(store):
    for flt in ({"level": {"$gt": 4}}, {"genre": "mystery", "level": 2},
                {"$or": [{"genre": "science"}, {"level": 0}]}, {"genre": {"$eq": None}},
                lambda m: m["level"] == 3):
        if not callable(flt):
            assert vlc.FAISS._key_index_values(flt) is None
        fn = vlc._create_filter_func(flt)
        want = [fn(store.docstore.search(store.index_to_docstore_id[i]).metadata)
                for i in range(300)]
        np.testing.assert_array_equal(store._filter_mask(flt), want)
        vec = store.embedding_function.embed_query("book 40")
        docs = store.similarity_search_by_vector(vec, k=6, filter=flt, exact_filter=True)
        assert len(docs) == min(6, sum(want)) and all(fn(d.metadata) for d in docs)


def test_selector_cache_is_dropped_by_writes(store):
    vec = store.embedding_function.embed_query("book 5")
    flt = {"genre": "mystery"}
    store.similarity_search_by_vector(vec, k=3, filter=flt, exact_filter=True)
    assert len(store._sel_cache) == 1
    first = next(iter(store._sel_cache.values()))
    store.similarity_search_by_vector(vec, k=3, filter={"genre": "mystery"}, exact_filter=True)
    assert next(iter(store._sel_cache.values())) is first  # reused, keyed by the filter's JSON
    store.similarity_search_by_vector(vec, k=3, filter=lambda m: True, exact_filter=True)
    assert len(store._sel_cache) == 1  # a callable has no key
    new = store.add_texts(["a new mystery"], metadatas=[{"book_id": "N1", "genre": "mystery"}])
    assert store._sel_cache == {}
    docs = store.similarity_search("a new mystery", k=1, filter=flt, exact_filter=True)
    assert docs[0].metadata["book_id"] == "N1"  # the new row is selectable
    assert len(store._sel_cache) == 1
    store.delete(new)
    assert store._sel_cache == {}
    docs = store.similarity_search("a new mystery", k=400, filter=flt, exact_filter=True)
    assert len(docs) == 100 and all(d.metadata["genre"] == "mystery" for d in docs)


def test_exact_filter_false_is_todays_behaviour(store):
    vec = store.embedding_function.embed_query("book 77")
    before = SelOracleIndex.searches
    for flt in (None, {"genre": "science"}, {"level": {"$gt": 2}}):
        for fetch_k in (20, 60):
            a = store.similarity_search_with_score_by_vector(vec, k=5, filter=flt,
                                                             fetch_k=fetch_k)
            b = store.similarity_search_with_score_by_vector(vec, k=5, filter=flt,
                                                             fetch_k=fetch_k, exact_filter=False)
            # today's rule restated: the fetch_k (k without a filter) nearest, filtered on the host
            D, I = store.index.search(np.asarray([vec], dtype=np.float32),
                                      5 if flt is None else fetch_k)
            fn = vlc._create_filter_func(flt) if flt is not None else (lambda m: True)
            want = []
            for s, i in zip(D[0], I[0]):
                doc = store.docstore.search(store.index_to_docstore_id[int(i)])
                if fn(doc.metadata):
                    want.append((doc.id, float(s)))
            want = want[:5]
            assert [(d.id, float(s)) for d, s in a] == want
            assert [(d.id, float(s)) for d, s in b] == want
    assert SelOracleIndex.searches == before  # no selector search was made
    assert store._sel_cache == {}
    # exact_filter without a filter is a plain search
    a = store.similarity_search_with_score_by_vector(vec, k=5, exact_filter=True)
    b = store.similarity_search_with_score_by_vector(vec, k=5)
    assert [(d.id, float(s)) for d, s in a] == [(d.id, float(s)) for d, s in b]


# ---- the service --------------------------------------------------------------------


def test_service_passes_exact_filter(store):
    vec = store.embedding_function.embed_query("book 17")
    read = _nearest_ids(store, vec, 25)
    flt = {"book_id": {"$nin": read}}
    want = store.similarity_search_with_score_by_vector(vec, k=10, filter=flt, exact_filter=True)
    with IndexService(store, authkey=KEY) as svc, RemoteFAISS(svc.address, KEY) as cli:
        batches = svc.stats["search_batches"]
        got = cli.similarity_search_with_score_by_vector(vec, k=10, filter=flt, exact_filter=True)
        assert [(d.id, d.metadata, float(s)) for d, s in got] == \
               [(d.id, d.metadata, float(s)) for d, s in want]
        assert svc.stats["search_batches"] == batches  # not through the coalescer
        assert len(cli.similarity_search_by_vector(vec, k=10, filter=flt)) == 0
        docs = cli.similarity_search("book 17", k=10, filter=flt, exact_filter=True)
        assert [d.id for d in docs] == [d.id for d, _ in want]
        got = cli.similarity_search_with_score("book 17", k=10, filter=flt, exact_filter=True,
                                               score_threshold=float(want[3][1]))
        assert [d.id for d, _ in got] == [d.id for d, _ in want[:len(got)]] and len(got) >= 4
        # the flag off: the fetch_k path, coalesced as before
        loose = cli.similarity_search_with_score_by_vector(vec, k=4, filter={"genre": "mystery"},
                                                           fetch_k=30, exact_filter=False)
        local = store.similarity_search_with_score_by_vector(vec, k=4,
                                                             filter={"genre": "mystery"},
                                                             fetch_k=30)
        assert [(d.id, float(s)) for d, s in loose] == [(d.id, float(s)) for d, s in local]
        assert svc.stats["search_batches"] > batches
