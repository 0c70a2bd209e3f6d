"""CPU: the host side of in-place updates (vs_update_rows, vs_range_selfjoin_rows
and the Python layers above them) — what needs no device.

The C entries' argument checks answer before anything is read through a
pointer; the LangChain ``in_place`` bookkeeping runs on an oracle-backed index
that adds ``update``; ``StudentIndex.reembed``'s ordering and mirroring run on a
stub index whose join returns a fixed graph."""

import ctypes

import numpy as np
import pytest

from helpers import OracleIndex
from oracle import flat
from vsearch import faiss as vfaiss
from vsearch import langchain as vlc
from vsearch import students as vstudents
from vsearch.synth import SynthEmbeddings


# ---- the C entries --------------------------------------------------------------------------------
def test_update_rows_argument_messages():
    from vsearch import _lib

    lib = _lib.load()
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)

    def expect(args, tail):
        assert lib.vs_update_rows(*args) == _lib.E_INVALID, tail
        assert _lib.last_error() == "vs_update_rows: " + tail

    expect((None, buf, buf, 1, 0, None), "null index")
    expect((None, None, None, -1, 0, None), "null index")  # the index is checked first
    expect((fake, buf, buf, -1, 0, None), "n < 0")
    expect((fake, None, None, -1, 0, None), "n < 0")  # n before the buffers
    expect((fake, None, buf, 1, 0, None), "null labels")
    expect((fake, buf, None, 1, 0, None), "null vectors")
    # n == 0 is success, whatever the buffers
    assert lib.vs_update_rows(fake, None, None, 0, 0, None) == 0


def test_range_selfjoin_rows_argument_messages():
    from vsearch import _lib

    lib = _lib.load()
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    rows = np.zeros(4, dtype=np.int64)
    out = ctypes.c_void_p()

    def expect(code, args, tail):
        assert lib.vs_range_selfjoin_rows(*args) == code, tail
        assert _lib.last_error() == "vs_range_selfjoin_rows: " + tail

    inv = _lib.E_INVALID
    expect(inv, (fake, rows.ctypes.data, 1, 0.5, 1, 0, None, None), "null output")
    expect(inv, (None, rows.ctypes.data, 1, 0.5, 1, 0, None, ctypes.byref(out)), "null index")
    expect(inv, (fake, rows.ctypes.data, -1, 0.5, 1, 0, None, ctypes.byref(out)), "nq < 0")
    expect(inv, (fake, None, 1, 0.5, 1, 0, None, ctypes.byref(out)), "null buffer")
    expect(_lib.E_UNSUPPORTED, (fake, rows.ctypes.data, 65537, 0.5, 1, 0, None, ctypes.byref(out)),
           "more than 65536 query rows in one call")
    assert out.value is None
    # the window form's messages are as they were
    assert lib.vs_range_selfjoin(fake, -1, 1, 0.5, 1, 0, 0, None, ctypes.byref(out)) == inv
    assert _lib.last_error() == "vs_range_selfjoin: query rows out of range"


def test_range_selfjoin_rows_keyword_is_exclusive():
    index = vfaiss.IndexFlat.__new__(vfaiss.IndexFlat)  # no device: the checks come first
    index._h = ctypes.c_void_p()  # nothing to destroy
    for kw in ({"q0": 3}, {"nq": 2}, {"upper": True}):
        with pytest.raises(ValueError, match="rows= excludes"):
            index.range_selfjoin(0.5, rows=[1, 2], **kw)
    lims, S, I = index.range_selfjoin(0.5, rows=[])
    assert lims.tolist() == [0] and S.size == 0 and I.size == 0


# ---- the LangChain store --------------------------------------------------------------------------
class UpdatableOracleIndex(OracleIndex):
    """OracleIndex with IndexFlat.update's contract."""

    def __init__(self, d, metric=flat.METRIC_L2):
        super().__init__(d, metric)
        self.updates = []

    def update(self, labels, x):
        labels = np.asarray(labels, dtype=np.int64) - self._base
        x = np.ascontiguousarray(x, dtype=np.float32)
        if ((labels < 0) | (labels >= self.ntotal)).any() or np.unique(labels).size != labels.size:
            raise RuntimeError("vs_update_rows: bad labels")
        self._x = self._x.copy()
        self._x[labels] = x
        self.updates.append(labels.tolist())


@pytest.fixture
def updatable(monkeypatch):
    monkeypatch.setattr(vfaiss, "IndexFlatL2", lambda d, **kw: UpdatableOracleIndex(d, flat.METRIC_L2))
    monkeypatch.setattr(vfaiss, "IndexFlatIP",
                        lambda d, **kw: UpdatableOracleIndex(d, flat.METRIC_INNER_PRODUCT))


N_BOOKS = 12


def _start(emb):
    """One starting store: 12 books, B3 stored twice (a re-embedding the
    reference appended), SynthEmbeddings rows (distinct scores)."""
    texts = [f"book {i} text" for i in range(N_BOOKS)]
    metas = [{"book_id": f"B{i}", "level": i % 3} for i in range(N_BOOKS)]
    store = vlc.FAISS.from_texts(texts, emb, metadatas=metas,
                                 distance_strategy=vlc.DistanceStrategy.MAX_INNER_PRODUCT)
    store.add_texts(["book 3 again"], metadatas=[{"book_id": "B3", "level": 0}])
    return store


def _answers(store, queries, k):
    return [[(d.page_content, d.metadata, float(s))
             for d, s in store.similarity_search_with_score(q, k=k)] for q in queries]


BATCH = (["book 1 v2", "book 3 v3", "book 7 v2", "brand new", "no key"],
         [{"book_id": "B1", "level": 1}, {"book_id": "B3", "level": 0},
          {"book_id": "B7", "level": 1}, {"book_id": "B77", "level": 2}, {"level": 5}])
QUERIES = ["book 1 v2", "book 3 v3", "book 3 again", "book 7 text", "brand new", "no key",
           "book 5 text", "anything else"]


def test_in_place_upsert_answers_as_delete_then_add(updatable):
    emb = SynthEmbeddings(32)
    a, b = _start(emb), _start(emb)
    ids_a = a.upsert_texts(*BATCH)
    ids_b = b.upsert_texts(*BATCH, in_place=True)
    assert len(ids_a) == len(ids_b) == 5
    assert a.index.ntotal == b.index.ntotal == N_BOOKS + 1 - 1 + 2  # one B3 row gone, two appended
    k = b.index.ntotal
    assert _answers(a, QUERIES, k) == _answers(b, QUERIES, k)
    # one update call for the three stored keys, B3 at its lowest label
    assert b.index.updates == [[1, 3, 7]] and a.index.updates == []
    # every untouched label kept its document: labels below the deleted B3 row
    # (label 12) are where they were, the replaced ones hold the new documents
    for i in range(N_BOOKS):
        doc = b.docstore.search(b.index_to_docstore_id[i])
        assert doc.metadata["book_id"] == f"B{i}"
        want = {1: "book 1 v2", 3: "book 3 v3", 7: "book 7 v2"}.get(i, f"book {i} text")
        assert doc.page_content == want
    assert [b.docstore.search(b.index_to_docstore_id[i]).page_content for i in (12, 13)] == \
        ["brand new", "no key"]
    assert sorted(b.index_to_docstore_id) == list(range(k))
    assert b.index_to_docstore_id[1] == ids_b[0] and b.index_to_docstore_id[7] == ids_b[2]
    assert b.ids_for_key("B3") == [ids_b[1]] and b.ids_for_key("B77") == [ids_b[3]]
    np.testing.assert_array_equal(
        b.index.reconstruct_n(0, k)[[1, 3, 7, 12]],
        np.array(emb.embed_documents(["book 1 v2", "book 3 v3", "book 7 v2", "brand new"]),
                 dtype=np.float32))


def test_in_place_pure_reembedding_keeps_caches(updatable):
    emb = SynthEmbeddings(32)
    store = _start(emb)
    store.delete(store.ids_for_key("B3")[1:])  # one row per key
    sel = store._filter_selector({"level": 1})
    store._grp_cache["book_id"] = "a grouping"
    before = dict(store.index_to_docstore_id)
    ids = store.upsert_texts(["book 4 v2", "book 9 v2"],
                             [{"book_id": "B4", "level": 1}, {"book_id": "B9", "level": 0}],
                             ids=["new-4", "new-9"], in_place=True)
    assert ids == ["new-4", "new-9"]
    assert store.index.updates == [[4, 9]] and store.index.ntotal == N_BOOKS
    # same metadata, nothing appended or deleted: the handles stay
    assert store._filter_selector({"level": 1}) is sel
    assert store._grp_cache == {"book_id": "a grouping"}
    assert store._keylabels is not None
    after = dict(store.index_to_docstore_id)
    assert {i for i in before if before[i] != after[i]} == {4, 9}
    assert after[4] == "new-4" and after[9] == "new-9"
    assert store.docstore.search("new-4").page_content == "book 4 v2"
    assert not isinstance(store.docstore.search(before[4]), vlc.Document)  # the old entry is gone
    assert store.ids_for_key("B4") == ["new-4"]
    hit, _ = store.similarity_search_with_score("book 4 v2", k=1)[0]
    assert hit.page_content == "book 4 v2" and hit.metadata["book_id"] == "B4"
    # a second pure re-embedding through the kept key table
    store.upsert_texts(["book 4 v3"], [{"book_id": "B4", "level": 1}], in_place=True)
    assert store.index.updates[-1] == [4] and store._filter_selector({"level": 1}) is sel

    # a replaced document whose metadata differs: the caches go
    store.upsert_texts(["book 5 v2"], [{"book_id": "B5", "level": 1}], in_place=True)  # was level 2
    assert store._sel_cache == {} and store._grp_cache == {} and store._keylabels is None
    assert store.index.ntotal == N_BOOKS
    mask = store._filter_mask({"level": 1})
    assert mask[5] and mask.sum() == 5  # levels 1: books 1, 4, 7, 10 and now 5

    # an append clears them too
    sel = store._filter_selector({"level": 1})
    store.upsert_texts(["fresh"], [{"book_id": "B50", "level": 1}], in_place=True)
    assert store._sel_cache == {} and store.index.ntotal == N_BOOKS + 1


def test_in_place_several_rows_and_validation(updatable):
    emb = SynthEmbeddings(16)
    store = _start(emb)
    assert len(store.ids_for_key("B3")) == 2
    store.upsert_texts(["book 3 v3"], [{"book_id": "B3", "level": 0}], in_place=True)
    # the lowest label is updated, the other row deleted
    assert store.index.ntotal == N_BOOKS and store.index.updates == [[3]]
    assert len(store.ids_for_key("B3")) == 1
    assert store.docstore.search(store.index_to_docstore_id[3]).page_content == "book 3 v3"
    # the last row of a key in the batch wins; the id clash is found before anything changes
    with pytest.raises(ValueError):
        store.upsert_texts(["x"], [{"book_id": "B1", "level": 1}],
                           ids=[store.index_to_docstore_id[2]], in_place=True)
    assert store.index.updates == [[3]]
    store.upsert_texts(["b1 a", "b1 b"], [{"book_id": "B1", "level": 1}] * 2, in_place=True)
    assert store.docstore.search(store.index_to_docstore_id[1]).page_content == "b1 b"
    # the replaced row's own id may be given again
    own = store.index_to_docstore_id[2]
    assert store.upsert_texts(["b2"], [{"book_id": "B2", "level": 2}], ids=[own],
                              in_place=True) == [own]
    assert store.docstore.search(own).page_content == "b2"

    class Failing(SynthEmbeddings):
        def embed_documents(self, texts, **kw):
            raise RuntimeError("embedding service down")

    store.embedding_function = Failing(16)
    n_updates = len(store.index.updates)
    with pytest.raises(RuntimeError):
        store.upsert_texts(["y"], [{"book_id": "B1", "level": 1}], in_place=True)
    assert len(store.index.updates) == n_updates  # embedded before anything is mutated


def test_in_place_needs_an_index_with_update(monkeypatch):
    monkeypatch.setattr(vfaiss, "IndexFlatL2", lambda d, **kw: OracleIndex(d, flat.METRIC_L2))
    store = vlc.FAISS.from_texts(["a", "b"], SynthEmbeddings(8),
                                 metadatas=[{"book_id": 1}, {"book_id": 2}])
    with pytest.raises(ValueError, match="in_place=True needs an index with update"):
        store.upsert_texts(["a2"], [{"book_id": 1}], in_place=True)
    assert store.index.ntotal == 2
    assert store.docstore.search(store.index_to_docstore_id[0]).page_content == "a"
    store.upsert_texts(["a2"], [{"book_id": 1}])  # the default path needs none
    assert store.index.ntotal == 2


def test_service_passes_in_place_through(updatable):
    from vsearch.service import IndexService, RemoteFAISS

    key = b"test-secret"
    store = _start(SynthEmbeddings(32))
    with IndexService(store, authkey=key) as svc, RemoteFAISS(svc.address, key) as cli:
        before = dict(store.index_to_docstore_id)
        ids = cli.upsert_texts(["book 6 v2"], metadatas=[{"book_id": "B6", "level": 0}],
                               in_place=True)
        assert store.index.updates == [[6]] and store.index.ntotal == N_BOOKS + 1
        assert store.index_to_docstore_id[6] == ids[0]
        assert {i for i in before if before[i] != store.index_to_docstore_id[i]} == {6}
        assert cli.similarity_search("book 6 v2", k=1)[0].page_content == "book 6 v2"
        cli.upsert_texts(["book 6 v3"], metadatas=[{"book_id": "B6", "level": 0}])  # the default
        assert store.index.updates == [[6]] and store.index.ntotal == N_BOOKS + 1
        assert store.index_to_docstore_id[N_BOOKS] != before[N_BOOKS]  # deleted, then appended


# ---- StudentIndex.reembed ---------------------------------------------------------------------------
class StubStudentIndex:
    """update records its arguments; the join answers from a fixed symmetric
    similarity matrix, as the engine does: hits ascending by row, self left out."""

    def __init__(self, sims):
        self.sims = np.asarray(sims, dtype=np.float32)
        self.d = 4
        self.updated = []
        self.joins = []

    def update(self, labels, x):
        self.updated.append((np.asarray(labels).tolist(), np.asarray(x).shape))

    def range_selfjoin(self, min_sim, *, rows=None, exclude_self=True, **kw):
        assert not kw and exclude_self
        self.joins.append(np.asarray(rows).tolist())
        lims, S, I = [0], [], []
        for r in rows:
            hit = [j for j in range(self.sims.shape[0])
                   if j != r and self.sims[r, j] >= np.float32(min_sim)]
            I += hit
            S += [self.sims[r, j] for j in hit]
            lims.append(len(I))
        return (np.array(lims, dtype=np.uint64), np.array(S, dtype=np.float32),
                np.array(I, dtype=np.int64))


def _student_index(sims):
    si = vstudents.StudentIndex.__new__(vstudents.StudentIndex)
    si.keys = [f"s{i}" for i in range(len(sims))]
    si.quantize = False
    si.index = StubStudentIndex(sims)
    si._row = {k: i for i, k in enumerate(si.keys)}
    return si


def test_reembed_rows_are_ordered_and_mirrored():
    n = 6
    sims = np.zeros((n, n), dtype=np.float32)

    def edge(a, b, s):
        sims[a, b] = sims[b, a] = s

    edge(4, 1, 0.9)   # updated 4 - untouched 1
    edge(4, 2, 0.8)   # updated 4 - updated 2
    edge(2, 0, 0.85)  # updated 2 - untouched 0
    edge(2, 5, 0.5)   # below the threshold
    edge(0, 1, 0.95)  # names no updated student
    si = _student_index(sims)
    vec = np.ones(4, dtype=np.float32)
    rows = si.reembed([("s4", vec), ("s2", 2 * vec)], threshold=0.75)
    assert si.index.updated == [([4, 2], (2, 4))]  # one update, the list's order
    assert si.index.joins == [[4, 2]]              # one row-list join
    f = lambda v: float(np.float32(v))
    assert rows == [
        ("s0", "s2", f(0.85)),
        ("s1", "s4", f(0.9)),
        ("s2", "s0", f(0.85)), ("s2", "s4", f(0.8)),
        ("s4", "s1", f(0.9)), ("s4", "s2", f(0.8)),
    ]
    # a mapping is taken too; nothing to do is no call
    assert si.reembed({"s4": vec}, threshold=0.75) == [
        ("s1", "s4", f(0.9)), ("s2", "s4", f(0.8)), ("s4", "s1", f(0.9)), ("s4", "s2", f(0.8))]
    assert si.reembed([]) == [] and len(si.index.joins) == 2
    with pytest.raises(KeyError):
        si.reembed([("s4", vec), ("nobody", vec)])
    with pytest.raises(ValueError):
        si.reembed([("s4", vec), ("s4", vec)])
    assert len(si.index.updated) == 2  # both refused before the update
    # replace: in place, an unknown student is a KeyError
    si.replace("s3", vec)
    assert si.index.updated[-1] == ([3], (1, 4))
    with pytest.raises(KeyError):
        si.replace("nobody", vec)
    # edges_of_many: each student's rows in list order
    assert si.edges_of_many(["s4", "s0"], 0.75) == [
        ("s4", "s1", f(0.9)), ("s4", "s2", f(0.8)), ("s0", "s1", f(0.95)), ("s0", "s2", f(0.85))]
