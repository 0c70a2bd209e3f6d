"""CPU: distinct searches without a device — the oracle on hand-worked cases,
the argument checks of vs_search_distinct / vs_grouping_create over a zeroed
handle, the window schedule (vs_distinct_plan), group_ids, and the store's and
the service's plumbing over an oracle index."""

import ctypes

import numpy as np
import pytest

import distinct_oracle as do
from helpers import OracleIndex
from oracle import flat
from vsearch import _lib
from vsearch import faiss as vfaiss
from vsearch import langchain as vlc
from vsearch.service import IndexService, RemoteFAISS, _Pending
from vsearch.synth import SynthEmbeddings

KEY = b"test-secret"
L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
FMAX = np.finfo(np.float32).max


# ---- the oracle on hand-worked cases ---------------------------------------------------
def test_oracle_ties_inside_a_group_go_to_the_lowest_label():
    #           label 0    1    2    3    4    5
    scores = np.array([[3.0, 1.0, 1.0, 2.0, 1.0, 5.0]])
    groups = np.array([7, 4, 4, 7, 9, -1])
    rep = do.representatives(scores, groups, L2)
    assert rep[0].tolist() == [False, True, False, True, True, True]  # 1 (not 2), 3 (not 0)
    D, I = do.distinct_topk(scores, groups, 3, L2)
    assert I[0].tolist() == [1, 4, 3] and D[0].tolist() == [1.0, 1.0, 2.0]
    # inner product: larger is better, and faiss emits equal scores by descending label
    rep = do.representatives(scores, groups, IP)
    assert rep[0].tolist() == [True, True, False, False, True, True]
    D, I = do.distinct_topk(scores, groups, 4, IP)
    assert I[0].tolist() == [5, 0, 4, 1] and D[0].tolist() == [5.0, 3.0, 1.0, 1.0]
    D, I = do.distinct_topk(scores, groups, 4, IP, rule="lex")
    assert I[0].tolist() == [5, 0, 1, 4]


def test_oracle_exclusions_minus_one_rows_and_padding():
    scores = np.array([[1.0, 2.0, 3.0, 4.0, 5.0],
                       [1.0, 2.0, 3.0, 4.0, 5.0]])
    groups = np.array([0, 0, 1, -1, -1])
    valid = np.ones((2, 5), dtype=bool)
    valid[0, 0] = False          # query 0: the representative of group 0 is excluded
    valid[1, [0, 1]] = False     # query 1: group 0 is wholly excluded
    D, I = do.distinct_topk(scores, groups, 5, L2, valid=valid)
    assert I[0].tolist() == [1, 2, 3, 4, -1]  # label 1 is promoted; 4 groups, k = 5 pads
    assert I[1].tolist() == [2, 3, 4, -1, -1]
    assert D[0, 4] == FMAX and D[1, 3] == FMAX
    assert do.group_problems(I, scores, groups, valid) == []
    # the checker sees a group twice, and a representative that is not the lowest label
    assert do.group_problems(np.array([[0, 1]]), scores[:1], groups)
    tied = np.array([[1.0, 1.0, 3.0]])
    assert do.group_problems(np.array([[1]]), tied, np.array([0, 0, 1]))
    # every row its own group: the plain search
    own = do.distinct_topk(scores, np.full(5, -1), 3, L2)
    plain = flat.select_topk(scores, 3, L2)
    assert own[1].tolist() == plain[1].tolist()


def test_oracle_equals_the_plain_search_on_random_data_without_groups():
    rng = np.random.default_rng(0)
    scores = rng.integers(-3, 4, size=(7, 60)).astype(np.float64)  # many ties
    for metric in (L2, IP):
        for groups in (np.full(60, -1), np.arange(60)):
            for rule in ("faiss", "lex"):
                D, I = do.distinct_topk(scores, groups, 9, metric, rule=rule)
                Dr, Ir = flat.select_topk(scores, 9, metric, rule=rule)
                assert np.array_equal(I, Ir) and np.array_equal(D, Dr)


# ---- C entry points ---------------------------------------------------------------------
def _fake():
    return ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)


def test_search_distinct_argument_messages_in_order():
    """index, grouping, n, k, k's limit, the offsets, the buffers: each check
    answers only when the ones before it pass, and none of them reads the
    index or the grouping (zeroed handles)."""
    lib = _lib.load()
    fake, grp = _fake(), _fake()
    b = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)

    def call(idx, g, n, k, offs=None, labels=None, bufs=False):
        x = b if bufs else None
        return lib.vs_search_distinct(idx, g, x, n, k, offs, labels, x, x, 0, None)

    def expect(tail, *a, **kw):
        assert call(*a, **kw) == _lib.E_INVALID, tail
        assert _lib.last_error() == f"vs_search_distinct: {tail}"

    expect("null index", None, None, -1, 0)
    expect("null grouping", fake, None, -1, 0)
    expect("n < 0", fake, grp, -1, 0)
    expect("k must be > 0", fake, grp, 1, 0)
    expect("k must be > 0", fake, grp, 1, -3)
    expect("k too large", fake, grp, 1, 2**30)
    assert call(fake, grp, 1, 1025, bufs=True) == _lib.E_UNSUPPORTED
    assert _lib.last_error().startswith("vs_search_distinct: k > 1024")
    assert "2 x 2047 groups" in _lib.last_error()
    assert call(fake, grp, 0, 1025) == _lib.E_UNSUPPORTED  # before the empty call's success
    assert call(fake, grp, 0, 1024) == 0
    bad = np.asarray([1, 1], dtype=np.int64)
    expect("offsets must start at 0 and not decrease", fake, grp, 1, 1024, bad.ctypes.data)
    one = np.asarray([0, 1], dtype=np.int64)
    expect("null exclusion labels", fake, grp, 1, 1, one.ctypes.data)
    expect("null buffer", fake, grp, 1, 1024)
    expect("null buffer", fake, grp, 1, 1, one.ctypes.data, one.ctypes.data)


def test_grouping_create_argument_messages_in_order():
    lib = _lib.load()
    fake = _fake()  # a zeroed index: no rows
    out = ctypes.c_void_p()
    ids = np.asarray([0, 5, -1], dtype=np.int32)

    def expect(tail, idx, p, n, o=ctypes.byref(out)):
        assert lib.vs_grouping_create(idx, p, n, None, o) == _lib.E_INVALID, tail
        assert _lib.last_error() == f"vs_grouping_create: {tail}"

    expect("null output", fake, ids.ctypes.data, 3, None)
    expect("null index", None, ids.ctypes.data, 3)
    expect("n < 0", fake, ids.ctypes.data, -1)
    expect("null groups", fake, None, 3)
    bad = np.asarray([0, -2, 1], dtype=np.int32)
    expect("a group must be >= 0, or -1 for a row of its own", fake, bad.ctypes.data, 3)
    # the values are checked before the index is read: n != the live rows (0) comes last
    expect("n must equal the live row count", fake, ids.ctypes.data, 3)
    assert not out.value
    n = ctypes.c_int64(0)
    assert lib.vs_grouping_groups(None, ctypes.byref(n)) == _lib.E_INVALID
    assert lib.vs_grouping_destroy(None) == 0


# ---- the window schedule ------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("k", [1, 5, 10, 64, 170, 1024])
@pytest.mark.parametrize("live", [1, 7, 26, 27, 3000, 10_000_000, 2**31 - 600])
def test_plan_is_a_non_decreasing_schedule_that_ends_at_the_live_rows(metric, raw, k, live):
    need = 2 * k - 1 if metric == IP and not raw else k
    w = vfaiss.distinct_plan(k, metric, raw, live)
    assert len(w) >= 1 and w[-1] == live
    assert w[0] >= min(need, live)
    assert all(a < b for a, b in zip(w, w[1:]))  # every round but the last grows
    if live <= need:
        assert w == [live]
    assert len(w) <= 16  # x 4 per round


def test_plan_depends_on_need_alone():
    # raw k = 19 and ruled inner product k = 10 both read 19 entries
    assert vfaiss.distinct_plan(19, IP, True, 5000) == vfaiss.distinct_plan(10, IP, False, 5000)
    assert vfaiss.distinct_plan(19, L2, False, 5000) == vfaiss.distinct_plan(10, IP, False, 5000)
    assert vfaiss.distinct_plan(10, L2, False, 5000) == vfaiss.distinct_plan(10, L2, True, 5000)
    assert vfaiss.distinct_plan(10, L2, False, 0) == []
    lib = _lib.load()
    out = np.zeros(2, dtype=np.int64)
    # more rounds than the caller has room for: the count is the whole schedule's
    assert lib.vs_distinct_plan(10, L2, 0, 3000, out.ctypes.data, 2) == 5
    assert out.tolist() == [26, 104]
    for bad in ((0, L2, 0, 10), (1025, L2, 0, 10), (1, 7, 0, 10), (1, L2, 0, -1)):
        assert lib.vs_distinct_plan(*bad, out.ctypes.data, 2) == _lib.E_INVALID


def test_stats_start_at_zero_and_check_their_outputs():
    assert vfaiss.distinct_stats(reset=True)[0] >= 0
    assert vfaiss.distinct_stats() == (0, 0, 0)
    assert _lib.load().vs_distinct_stats(None, None, None, 0) == _lib.E_INVALID


# ---- group_ids ----------------------------------------------------------------------------
def test_group_ids():
    ints = np.array([5, -1, 5, 2**31 - 1, 0], dtype=np.int64)
    assert vfaiss.group_ids(ints).tolist() == ints.tolist()
    assert vfaiss.group_ids(ints).dtype == np.int32
    assert vfaiss.group_ids([3, -1, 3]).tolist() == [3, -1, 3]
    ids = vfaiss.group_ids(["b", None, "a", "b", ("x", 1), None, "a"])
    assert ids.tolist() == [0, -1, 1, 0, 2, -1, 1]  # equal keys equal ids, dense, None alone
    assert vfaiss.group_ids([]).size == 0
    for bad in (np.array([-2, 0]), np.array([2**31]), [0, -5]):
        with pytest.raises(ValueError):
            vfaiss.group_ids(bad)


# ---- store and service over an oracle index -------------------------------------------
class _OracleGrouping:
    def __init__(self, index, ids):
        self.index, self.ids, self.closed = index, np.asarray(ids), False
        self.groups = int(np.unique(self.ids[self.ids >= 0]).size + (self.ids < 0).sum())

    def close(self):
        self.closed = True


class DistinctOracleIndex(OracleIndex):
    """OracleIndex with the exclusion, profile and distinct surface of IndexFlat;
    the collapse is distinct_oracle's."""

    def __init__(self, d, metric=L2):
        super().__init__(d, metric)
        self.calls = []
        self.groupings = []

    def _valid(self, n, exclude):
        valid = np.ones((n, self.ntotal), dtype=bool)
        if exclude is not None:
            offs, labels = vfaiss.exclusion_csr(exclude, n)
            for q in range(n):
                seg = labels[offs[q]:offs[q + 1]]
                valid[q, seg[(seg >= 0) & (seg < self.ntotal)]] = False
        return valid

    def search(self, x, k, raw=False, exclude=None, params=None):
        assert params is None
        x = np.ascontiguousarray(x, dtype=np.float32)
        self.calls.append(("search", x.shape[0], k))
        return flat.select_topk(flat.exact_scores(self._x, x, self.metric_type), k,
                                self.metric_type, valid=self._valid(x.shape[0], exclude),
                                rule="lex" if raw else "faiss")

    def mean_rows(self, profiles):
        out = []
        for labels, weights in profiles:
            w = np.asarray(weights, dtype=np.float32)
            acc = np.sum([self._x[l] * v for l, v in zip(labels, w)], axis=0)
            out.append((acc / np.float32(sum(float(v) for v in w))).astype(np.float32))
        return np.stack(out)

    def search_profiles(self, profiles, k, *, exclude=None, exclude_profile=True):
        assert not exclude_profile
        return self.search(self.mean_rows(profiles), k, exclude=exclude)

    def grouping(self, keys):
        ids = vfaiss.group_ids(keys)
        assert ids.size == self.ntotal
        self.groupings.append(_OracleGrouping(self, ids))
        return self.groupings[-1]

    def search_distinct(self, x, k, grouping, *, exclude=None, raw=False):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert grouping.index is self and grouping.ids.size == self.ntotal
        self.calls.append(("search_distinct", x.shape[0], k, grouping.groups))
        return do.distinct_topk(flat.exact_scores(self._x, x, self.metric_type), grouping.ids, k,
                                self.metric_type, valid=self._valid(x.shape[0], exclude),
                                rule="lex" if raw else "faiss")


N_BOOKS = 60
N_AUTHORS = 12


def _meta(i):
    return {"book_id": f"B{i:03d}", "author": f"A{i % N_AUTHORS:02d}", "shelf": i % 3}


@pytest.fixture
def store(monkeypatch):
    """60 books of 12 authors; a third of them re-ingested as the reference
    does it (an appended, identical row), and two documents without an author."""
    monkeypatch.setattr(vfaiss, "IndexFlatL2", lambda d, **kw: DistinctOracleIndex(d, L2))
    emb = SynthEmbeddings(48)
    texts = [f"book {i}" for i in range(N_BOOKS)]
    metas = [_meta(i) for i in range(N_BOOKS)]
    st = vlc.FAISS.from_texts(texts, emb, metadatas=metas)
    st.add_texts([f"book {i}" for i in range(0, N_BOOKS, 3)],
                 metadatas=[_meta(i) for i in range(0, N_BOOKS, 3)])
    st.add_texts(["note 1", "note 2"], metadatas=[{"book_id": "N1"}, {"book_id": "N2"}])
    return st


def _query(store, *labels):
    v = np.sum([store.index._x[l] * w for l, w in zip(labels, (1.0, 0.6, 0.4))], axis=0)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _field(pairs, field="book_id"):
    return [d.metadata.get(field) for d, _ in pairs]


def test_store_returns_each_book_once(store):
    q = _query(store, 6, 40, 21)  # B006 and B021 are stored twice
    plain = store.similarity_search_with_score_by_vector(q, k=8)
    assert _field(plain)[:2] == ["B006", "B006"]
    got = store.similarity_search_with_score_by_vector(q, k=8, distinct="book_id")
    assert len(got) == 8 and len(set(_field(got))) == 8
    assert got[0] == plain[0]
    # the plain order with the later copies dropped
    seen, want = set(), []
    for d, s in store.similarity_search_with_score_by_vector(q, k=40):
        if d.metadata["book_id"] not in seen:
            seen.add(d.metadata["book_id"])
            want.append((d, s))
    assert got == want[:8]
    assert store.index.calls[-2][0] == "search_distinct"
    # the three methods over it, and the batch
    assert store.similarity_search_by_vector(q, k=8, distinct="book_id") == [d for d, _ in got]
    vec = np.asarray(store._embed_query("book 6"), dtype=np.float32)
    by_text = store.similarity_search_with_score("book 6", k=5, distinct="book_id")
    assert by_text == store.similarity_search_with_score_by_vector(vec, k=5, distinct="book_id")
    assert store.similarity_search("book 6", k=5, distinct="book_id") == [d for d, _ in by_text]
    assert _field(by_text).count("B006") == 1
    assert _field(store.similarity_search_with_score("book 6", k=5)).count("B006") == 2
    batch = store.similarity_search_batch_by_vector([q, vec], k=8, distinct="book_id")
    assert batch[0] == got and batch[1][:5] == by_text
    # one document per author; the two without the field count one by one
    authors = store.similarity_search_with_score_by_vector(q, k=40, distinct="author")
    assert len(authors) == N_AUTHORS + 2
    assert sorted(a for a in _field(authors, "author") if a) == [f"A{i:02d}"
                                                                   for i in range(N_AUTHORS)]
    assert _field(authors, "author").count(None) == 2


def test_store_distinct_with_filters_and_exclusions(store):
    q = _query(store, 6, 40, 21)
    with pytest.raises(ValueError, match="distinct and exact_filter"):
        store.similarity_search_with_score_by_vector(q, k=4, distinct="book_id",
                                                     filter={"shelf": 0}, exact_filter=True)
    with pytest.raises(ValueError, match="distinct and exact_filter"):
        store.similarity_search(  # through the methods over it too
            "book 6", k=4, distinct="book_id", exact_filter=True)
    # a host filter: the distinct search fetches fetch_k groups, the filter runs after it
    store.index.calls.clear()
    got = store.similarity_search_with_score_by_vector(q, k=3, distinct="book_id",
                                                       filter={"shelf": 0}, fetch_k=12)
    assert store.index.calls == [("search_distinct", 1, 12, N_BOOKS + 2)]
    assert len(got) == 3 and all(d.metadata["shelf"] == 0 for d, _ in got)
    assert len(set(_field(got))) == 3
    # exclude_ids leaves a representative out: its book's other row stands in
    first = store.similarity_search_with_score_by_vector(q, k=1, distinct="book_id")[0][0]
    assert first.metadata["book_id"] == "B006"
    got = store.similarity_search_with_score_by_vector(q, k=4, distinct="book_id",
                                                       exclude_ids=[first.id])
    assert got[0][0].metadata["book_id"] == "B006" and got[0][0].id != first.id
    assert len(set(_field(got))) == 4


def test_store_builds_a_grouping_once_per_field_and_drops_it_on_writes(store):
    q = _query(store, 6, 40, 21)
    made = store.index.groupings
    store.similarity_search_by_vector(q, k=3, distinct="book_id")
    store.similarity_search_by_vector(q, k=5, distinct="book_id")
    assert len(made) == 1 and made[0].groups == N_BOOKS + 2
    store.similarity_search_by_vector(q, k=3, distinct="author")
    store.similarity_search_batch_by_vector([q], k=3, distinct="author")
    assert len(made) == 2 and made[1].groups == N_AUTHORS + 2
    ids = store.add_texts(["book 6"], metadatas=[_meta(6)])
    assert store._grp_cache == {} and store._sel_cache == {}
    got = store.similarity_search_by_vector(q, k=5, distinct="book_id")
    assert len(made) == 3 and made[2].ids.size == store.index.ntotal
    assert [d.metadata["book_id"] for d in got].count("B006") == 1
    store.delete(ids)
    assert store._grp_cache == {}
    store.similarity_search_by_vector(q, k=5, distinct="book_id")
    assert len(made) == 4 and made[3].ids.size == store.index.ntotal


PROFILES = [[("B005", 1.0), ("B017", 0.5), ("nope", 0.8)],
            [("nope", 1.0)],
            [("B030", 0.3)],
            [(f"B{i:03d}", 0.1 + 0.1 * (i % 5)) for i in range(0, 40, 3)]]
READ = [["B006", "B007"], ["B001"], [], [f"B{i:03d}" for i in range(40, 50)]]


def test_store_recommend_for_profiles_distinct(store):
    base = store.recommend_for_profiles(PROFILES, k=8, exclude=READ)
    assert any(len(set(_field(r, "author"))) < len(r) for r in base)  # authors repeat
    got = store.recommend_for_profiles(PROFILES, k=8, exclude=READ, distinct="author")
    assert [len(r) for r in got] == [8, 0, 8, 8]
    kept, rows, lists = store.profile_requests(PROFILES, READ)
    vec = store.index.mean_rows(rows)
    authors = [store.docstore.search(store.index_to_docstore_id[i]).metadata.get("author")
               for i in range(store.index.ntotal)]
    D, I = do.distinct_topk(flat.exact_scores(store.index._x, vec, L2), vfaiss.group_ids(authors),
                            8, L2, valid=store.index._valid(len(kept), lists))
    for j, p in enumerate(kept):
        assert len(set(_field(got[p], "author"))) == 8
        barred = {b for b, _ in PROFILES[p]} | set(READ[p])
        assert not barred.intersection(_field(got[p]))
        assert [store.index_to_docstore_id[int(i)] for i in I[j]] == [d.id for d, _ in got[p]]
        assert [s for _, s in got[p]] == D[j].tolist()
    with pytest.raises(ValueError, match="distinct and mmr"):
        store.recommend_for_profiles(PROFILES, k=8, distinct="author", mmr=(20, 0.5))


def test_service_carries_the_field(store):
    q = _query(store, 6, 40, 21)
    with IndexService(store, authkey=KEY) as svc:
        with RemoteFAISS(svc.address, KEY) as cli:
            before = svc.stats["search_batches"]
            want = store.similarity_search_with_score_by_vector(q, k=6, distinct="book_id")
            got = cli.similarity_search_with_score_by_vector(q, k=6, distinct="book_id")
            assert [d for d, _ in got] == [d for d, _ in want]
            assert [np.float32(s) for _, s in got] == [np.float32(s) for _, s in want]
            assert len(set(_field(got))) == 6
            assert cli.similarity_search_by_vector(q, k=6, distinct="book_id") == \
                [d for d, _ in want]
            assert cli.similarity_search("book 6", k=5, distinct="book_id") == \
                store.similarity_search("book 6", k=5, distinct="book_id")
            assert cli.similarity_search_with_score("book 6", k=5, distinct="author") == \
                store.similarity_search_with_score("book 6", k=5, distinct="author")
            assert cli.similarity_search_by_vector(
                q, k=3, distinct="book_id", filter={"shelf": 0}, fetch_k=12) == \
                store.similarity_search_by_vector(
                    q, k=3, distinct="book_id", filter={"shelf": 0}, fetch_k=12)
            assert svc.stats["search_batches"] == before + 5  # through the coalescer
            with pytest.raises(ValueError, match="distinct and exact_filter"):
                cli.similarity_search_by_vector(q, k=3, distinct="book_id", exact_filter=True)
            want = store.recommend_for_profiles(PROFILES, k=8, exclude=READ, distinct="author")
            got = cli.recommend_for_profiles(PROFILES, k=8, exclude=READ, distinct="author")
            assert [[d for d, _ in r] for r in got] == [[d for d, _ in r] for r in want]
            assert [[np.float32(s) for _, s in r] for r in got] == \
                [[np.float32(s) for _, s in r] for r in want]
            assert svc.stats["search_batches"] == before + 6
            with pytest.raises(ValueError, match="distinct and mmr"):
                cli.recommend_for_profiles(PROFILES, k=8, distinct="author", mmr=(20, 0.5))
            # without the field the frames are what they always were
            assert cli.similarity_search_by_vector(q, k=6) == \
                store.similarity_search_by_vector(q, k=6)


def test_frames_are_unchanged_without_distinct():
    sent = []
    cli = RemoteFAISS.__new__(RemoteFAISS)
    cli._call = lambda header, payload=b"": (sent.append(header), ({"results": []}, b""))[1]
    cli.similarity_search_with_score("q", k=3)
    cli.similarity_search_with_score("q", k=3, distinct=None)
    cli.similarity_search_with_score("q", k=3, distinct="book_id")
    assert sent[0] == sent[1] and "distinct" not in sent[0]
    assert sent[2] == dict(sent[0], distinct="book_id")
    cli.recommend_for_profiles([[("B001", 1.0)]], k=3)
    cli.recommend_for_profiles([[("B001", 1.0)]], k=3, distinct="author")
    assert "distinct" not in sent[3] and sent[4] == dict(sent[3], distinct="author")


def test_coalescer_batches_requests_with_others_of_their_field_only(store):
    """Requests that wait together: the plain ones, the ones distinct by book
    and the one distinct by author each get a call of their own, and every
    caller its own rows."""
    q = np.stack([_query(store, 6, 40, 21), _query(store, 9, 3, 50), _query(store, 30, 12, 7)])
    with IndexService(store, authkey=KEY) as svc:
        co = svc._coalescer
        ps = [_Pending(q[0:1], 5, None, "book_id"), _Pending(q[1:2], 5, None, "author"),
              _Pending(q[2:3], 5, None, "book_id"), _Pending(q[0:1], 5), _Pending(q[1:2], 5),
              _Pending(q[1:2], 5, [[6, 7]], "book_id")]
        store.index.calls.clear()
        with co._cv:  # queued together: the dispatcher takes them as one round
            co._queue.extend(ps)
            co._cv.notify()
        for p in ps:
            assert p.done.wait(30) and p.err is None
        calls = sorted(store.index.calls)
        assert calls == [("search", 2, 5), ("search_distinct", 1, 5, N_AUTHORS + 2),
                         ("search_distinct", 3, 5, N_BOOKS + 2)]
        grp = store._distinct_grouping("book_id")
        for p, x in ((ps[0], q[0:1]), (ps[2], q[2:3])):
            D, I = store.index.search_distinct(x, 5, grp)
            assert np.array_equal(p.I, I) and np.array_equal(p.D, D)
        D, I = store.index.search_distinct(q[1:2], 5, grp, exclude=[[6, 7]])
        assert np.array_equal(ps[5].I, I)
        D, I = store.index.search_distinct(q[1:2], 5, store._distinct_grouping("author"))
        assert np.array_equal(ps[1].I, I)
        assert np.array_equal(ps[3].I, store.index.search(q[0:1], 5)[1])
