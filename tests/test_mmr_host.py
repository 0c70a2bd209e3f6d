"""CPU: the host side of the MMR searches — the argument checks of
vs_mmr_select / vs_search_mmr that need no device, the oracle module against
hand-worked cases, and the store's and the service's plumbing over an oracle
index."""

import ctypes

import numpy as np
import pytest

import mmr_oracle
from helpers import OracleIndex
from oracle import flat
from vsearch import _lib
from vsearch import faiss as vfaiss
from vsearch import langchain as vlc
from vsearch.service import IndexService, RemoteFAISS
from vsearch.synth import SynthEmbeddings

KEY = b"test-secret"
NAN = float("nan")
INF = float("inf")


# ---- C entry points -----------------------------------------------------------------
def _select(lib, idx, n, k, fetch_k, lam, bufs):
    b = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p) if bufs else None
    return lib.vs_mmr_select(idx, b, n, b, fetch_k, k, lam, b, 0, None)


def _search(lib, idx, n, k, fetch_k, lam, bufs):
    b = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p) if bufs else None
    return lib.vs_search_mmr(idx, b, n, k, fetch_k, lam, None, None, b, b, 0, None)


@pytest.mark.parametrize("name,call", [("vs_mmr_select", _select), ("vs_search_mmr", _search)])
def test_argument_messages_in_order(name, call):
    """index, n, k, fetch_k, lambda, buffers: each check answers only when the
    ones before it pass, and none of them reads the index (a zeroed handle)."""
    lib = _lib.load()
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)

    def expect(idx, n, k, fetch_k, lam, bufs, tail):
        assert call(lib, idx, n, k, fetch_k, lam, bufs) == _lib.E_INVALID, (name, tail)
        assert _lib.last_error() == f"{name}: {tail}"

    expect(None, -1, 0, 0, NAN, False, "null index")
    expect(fake, -1, 0, 0, NAN, False, "n < 0")
    expect(fake, 1, 0, 0, NAN, False, "k must be > 0")
    expect(fake, 1, -2, 0, NAN, False, "k must be > 0")
    expect(fake, 1, 1, 0, NAN, False, "fetch_k must be > 0")
    expect(fake, 1, 1, -5, NAN, False, "fetch_k must be > 0")
    expect(fake, 1, 1, 1, NAN, False, "lambda_mult is not finite")
    expect(fake, 1, 1, 1, INF, False, "lambda_mult is not finite")
    expect(fake, 1, 1, 1, -INF, False, "lambda_mult is not finite")
    expect(fake, 1, 1, 1, 0.5, False, "null buffer")
    expect(fake, 1, 5, 2, 0.5, False, "null buffer")  # k > fetch_k is legal
    # no queries: success without buffers, but only after the other checks
    assert call(lib, fake, 0, 1, 1, 0.5, False) == 0
    expect(fake, 0, 1, 0, 0.5, False, "fetch_k must be > 0")
    expect(fake, 0, 1, 1, NAN, False, "lambda_mult is not finite")


@pytest.mark.parametrize("name,call", [("vs_mmr_select", _select), ("vs_search_mmr", _search)])
def test_fetch_k_past_the_limit_is_unsupported(name, call):
    lib = _lib.load()
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    assert call(lib, fake, 1, 4, 1025, 0.5, True) == _lib.E_UNSUPPORTED
    assert _lib.last_error().startswith(f"{name}: fetch_k > 1024")


def test_search_mmr_checks_its_lists():
    lib = _lib.load()
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    b = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    offs = np.asarray([1, 1], dtype=np.int64)
    assert lib.vs_search_mmr(fake, b, 1, 2, 4, 0.5, offs.ctypes.data, None, b, b, 0,
                             None) == _lib.E_INVALID
    assert _lib.last_error() == "vs_search_mmr: offsets must start at 0 and not decrease"
    offs = np.asarray([0, 1], dtype=np.int64)
    assert lib.vs_search_mmr(fake, b, 1, 2, 4, 0.5, offs.ctypes.data, None, b, b, 0,
                             None) == _lib.E_INVALID
    assert _lib.last_error() == "vs_search_mmr: null exclusion labels"


def test_python_wrappers_check_before_the_library():
    index = vfaiss.IndexFlat.__new__(vfaiss.IndexFlat)
    index._d = 4
    index._h = None
    index._metric = vfaiss.METRIC_L2
    x = np.zeros((2, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="not both"):
        index.search_mmr(x, 3, exclude=[[1], []],
                         params=vfaiss.SearchParameters(sel=vfaiss.IDSelectorAll()))
    with pytest.raises(ValueError, match="cand_labels"):
        index.mmr_select(x, np.zeros((3, 5), dtype=np.int64), 2)
    with pytest.raises(AssertionError):
        index.mmr_select(x, np.zeros((2, 5), dtype=np.int64), 0)
    # no candidates at all: nothing to pick, no library call
    assert index.mmr_select(x, np.zeros((2, 0), dtype=np.int64), 3).tolist() == [[-1] * 3] * 2


def test_gather_picks_pads_like_a_search():
    D = np.asarray([[0.5, 1.5, 2.5]], dtype=np.float32)
    I = np.asarray([[7, 8, 9]], dtype=np.int64)
    pos = np.asarray([[2, 0, -1, -1]], dtype=np.int32)
    Dp, Ip = vfaiss.gather_picks(D, I, pos, vfaiss.METRIC_L2)
    assert Dp.dtype == np.float32 and Ip.dtype == np.int64
    assert Ip.tolist() == [[9, 7, -1, -1]]
    assert Dp[0, :2].tolist() == [2.5, 0.5] and Dp[0, 2] == np.finfo(np.float32).max
    Dp, _ = vfaiss.gather_picks(D, I, pos, vfaiss.METRIC_INNER_PRODUCT)
    assert Dp[0, 3] == -np.finfo(np.float32).max


# ---- the oracle against hand-worked cases ---------------------------------------------
def test_oracle_tie_goes_to_the_lowest_position():
    # q = c0: after c0 every score is lambda * s_i - (1 - lambda) * cos(c_i, c0)
    # with s_i == cos(c_i, c0) bit for bit: 0 for all at lambda = 0.5 -> list order
    q = [1.0, 0.0]
    E = [[1.0, 0.0], [1.0, 0.1], [0.0, 1.0]]
    assert mmr_oracle.mmr_positions(q, E, 3, 0.5).tolist() == [0, 1, 2]
    picks, gaps = mmr_oracle.Problem(q, E).select(3, 0.5)
    assert picks == [0, 1, 2] and gaps[1] == 0.0 and gaps[2] == INF


def test_oracle_lambda_one_sorts_by_cosine_and_lambda_zero_spreads():
    q = [1.0, 0.0]
    # cosines to q: 0, 1 / sqrt(2), 1
    assert mmr_oracle.mmr_positions(q, [[0.0, 1.0], [1.0, 1.0], [1.0, 0.0]], 3,
                                    1.0).tolist() == [2, 1, 0]
    # lambda = 0: the first pick is still the nearest (c0); then the score is
    # -max cos to the picks: c2 = -c0 scores +1; then c3 (0) before c1 (-0.99995)
    E = [[1.0, 0.0], [1.0, 0.01], [-1.0, 0.0], [0.0, 1.0]]
    assert mmr_oracle.mmr_positions(q, E, 4, 0.0).tolist() == [0, 2, 3, 1]
    # a hand-computed score: c1 after c0 at lambda = 0.25
    p = mmr_oracle.Problem(q, E)
    sc, _ = p.scores([0], 0.25)
    c = 1.0 / np.sqrt(1.0 + 1e-4)
    assert abs(sc[1] - (0.25 * c - 0.75 * c)) < 1e-15 and sc[0] == -INF


def test_oracle_empty_slots_zero_rows_and_padding():
    q = [1.0, 0.0]
    E = [[0.0, 0.0], [5.0, 5.0], [-1.0, 0.0]]
    valid = [True, False, True]
    # the zero row's cosines are 0 (not NaN): 0 > -1, so it is picked first;
    # position 1 is an empty slot and keeps its place; k = 5 pads with -1
    assert mmr_oracle.mmr_positions(q, E, 5, 0.5, valid).tolist() == [0, 2, -1, -1, -1]
    assert mmr_oracle.mmr_positions([0.0, 0.0], E, 2, 0.5, valid).tolist() == [0, 2]  # zero query
    assert mmr_oracle.mmr_positions(q, E, 2, 0.5, [False] * 3).tolist() == [-1, -1]
    assert np.isfinite(mmr_oracle.Problem(q, E, valid).G).all()
    rows = np.asarray(E, dtype=np.float32)
    got = mmr_oracle.mmr_select_labels(rows, np.asarray([q], dtype=np.float32),
                                       [[1002, -1, 1000]], 3, 0.5, id_base=1000)
    # positions, not labels: c_0 = row 2 = (-1, 0) scores -1, c_2 = the zero row 0
    assert got.tolist() == [[2, 0, -1]]
    assert mmr_oracle.replay(mmr_oracle.Problem(q, E, valid), [0, 2, -1], 3, 0.5, 2) == []
    with pytest.raises(AssertionError):
        mmr_oracle.replay(mmr_oracle.Problem(q, E, valid), [2, 0, -1], 3, 0.5, 2)
    with pytest.raises(AssertionError):
        mmr_oracle.replay(mmr_oracle.Problem(q, E, valid), [0, 1, -1], 3, 0.5, 2)


def test_issue_precondition_holds_on_the_gpu_tests_inputs():
    """The smallest gap between the oracle's best and second-best score dwarfs
    the slack on the kind of rows the GPU tests use."""
    rng = np.random.default_rng(11)
    d, F = 100, 64
    centres = rng.standard_normal((4, d))
    E = (centres[rng.integers(0, 4, F)] + 0.3 * rng.standard_normal((F, d))).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    for lam in (0.0, 0.5, 1.0):
        _, gaps = mmr_oracle.Problem(q, E).select(10, lam)
        assert min(gaps) > 2 * mmr_oracle.slack(d)


# ---- store and service over an oracle index -------------------------------------------
class MmrOracleIndex(OracleIndex):
    """OracleIndex with the MMR, exclusion, selector and profile surface of
    IndexFlat; the re-rank is the oracle's."""

    def __init__(self, d, metric=flat.METRIC_L2):
        super().__init__(d, metric)
        self.calls = []

    def search(self, x, k, raw=False, exclude=None, params=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self.calls.append(("search", x.shape[0], k))
        valid = np.ones((x.shape[0], self.ntotal), dtype=bool)
        sel = getattr(params, "sel", None)
        if sel is not None:
            valid &= np.asarray(sel.members(np.arange(self.ntotal)), dtype=bool)[None, :]
        if exclude is not None:
            offs, labels = vfaiss.exclusion_csr(exclude, x.shape[0])
            for q in range(x.shape[0]):
                seg = labels[offs[q]:offs[q + 1]]
                valid[q, seg[(seg >= 0) & (seg < self.ntotal)]] = False
        return flat.select_topk(flat.exact_scores(self._x, x, self.metric_type), k,
                                self.metric_type, valid=valid, rule="lex" if raw else "faiss")

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

    def mmr_select(self, x, cand_labels, k, lambda_mult=0.5):
        self.calls.append(("mmr_select", np.asarray(cand_labels).shape, k))
        return mmr_oracle.mmr_select_labels(self._x, x, cand_labels, k, lambda_mult, self._base)

    def search_mmr(self, x, k, fetch_k=20, lambda_mult=0.5, *, params=None, exclude=None):
        self.calls.append(("search_mmr", np.asarray(x).shape[0], k, fetch_k, lambda_mult))
        D, I = self.search(x, fetch_k, params=params, exclude=exclude)
        return vfaiss.gather_picks(D, I, self.mmr_select(x, I, k, lambda_mult), self.metric_type)


N_BOOKS = 90


@pytest.fixture
def store(monkeypatch):
    monkeypatch.setattr(vfaiss, "IndexFlatL2", lambda d, **kw: MmrOracleIndex(d, flat.METRIC_L2))
    emb = SynthEmbeddings(48)
    texts = [f"book {i}" for i in range(N_BOOKS)]
    metas = [{"book_id": f"B{i:03d}", "shelf": i % 3} for i in range(N_BOOKS)]
    # B005 re-ingested: the reference appends a second, identical row
    texts.append("book 5")
    metas.append({"book_id": "B005", "shelf": 5 % 3})
    return vlc.FAISS.from_texts(texts, emb, metadatas=metas)


def _query(store, *labels):
    """A query between the given stored rows (not any row itself)."""
    v = np.sum([store.index._x[l] * w for l, w in zip(labels, (1.0, 0.6, 0.4))], axis=0)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _ids(pairs):
    return [d.metadata["book_id"] for d, _ in pairs]


def test_store_mmr_methods_on_oracle(store):
    q = _query(store, 11, 40, 63)
    X = store.index._x
    D, I = store.index.search(q[None, :], 20)
    want = mmr_oracle.mmr_positions(q, X[I[0]], 4, 0.5)
    got = store.max_marginal_relevance_search_with_score_by_vector(q)  # LangChain's defaults
    assert _ids(got) == [f"B{int(I[0][p]):03d}" for p in want]
    # the score is the search's faiss score, not the MMR score
    assert [s for _, s in got] == [D[0][p] for p in want]
    assert ("search_mmr", 1, 4, 20, 0.5) in store.index.calls
    docs = store.max_marginal_relevance_search_by_vector(q, k=6, fetch_k=30, lambda_mult=0.2)
    want = mmr_oracle.mmr_positions(q, X[store.index.search(q[None, :], 30)[1][0]], 6, 0.2)
    assert [d.metadata["book_id"] for d in docs] == [
        f"B{int(store.index.search(q[None, :], 30)[1][0][p]):03d}" for p in want]
    by_text = store.max_marginal_relevance_search("book 11", k=3, fetch_k=10)
    vec = np.asarray(store._embed_query("book 11"), dtype=np.float32)
    assert by_text == store.max_marginal_relevance_search_by_vector(vec, k=3, fetch_k=10)
    # lambda = 1 is the plain search order; k > fetch_k returns fetch_k documents
    plain = store.similarity_search_with_score_by_vector(q, k=5)
    assert _ids(store.max_marginal_relevance_search_with_score_by_vector(
        q, k=5, lambda_mult=1.0)) == _ids(plain)
    assert len(store.max_marginal_relevance_search_by_vector(q, k=9, fetch_k=5)) == 5
    batch = store.max_marginal_relevance_search_batch_by_vector([q, X[3]], k=4)
    assert _ids(batch[0]) == _ids(got) and len(batch[1]) == 4
    assert not hasattr(store, "as_retriever")


def test_store_mmr_filters_on_oracle(store):
    q = _query(store, 11, 40, 63)
    X = store.index._x
    flt = {"shelf": 1}
    # LangChain's route: search fetch_k * 2, filter on the host, re-rank the rest
    store.index.calls.clear()
    got = store.max_marginal_relevance_search_with_score_by_vector(q, k=3, fetch_k=12, filter=flt)
    assert store.index.calls[0] == ("search", 1, 24) and store.index.calls[1][0] == "mmr_select"
    D, I = store.index.search(q[None, :], 24)
    keep = [j for j, i in enumerate(I[0]) if i < N_BOOKS and i % 3 == 1]  # (the copy: shelf 2)
    want = mmr_oracle.mmr_positions(q, X[I[0][keep]], 3, 0.5)
    assert _ids(got) == [f"B{int(I[0][keep[p]]):03d}" for p in want]
    assert [s for _, s in got] == [D[0][keep[p]] for p in want]
    assert all(d.metadata["shelf"] == 1 for d, _ in got)
    assert store.max_marginal_relevance_search_by_vector(q, filter={"shelf": 77}) == []
    # exact_filter: the filter is a selector, exactly min(fetch_k, matches) candidates
    store.index.calls.clear()
    got = store.max_marginal_relevance_search_with_score_by_vector(q, k=3, fetch_k=12, filter=flt,
                                                                   exact_filter=True)
    assert store.index.calls[0] == ("search_mmr", 1, 3, 12, 0.5)
    members = np.asarray([i for i in range(N_BOOKS) if i % 3 == 1])
    order = members[np.argsort(flat.exact_scores(X[members], q[None, :], flat.METRIC_L2)[0],
                               kind="stable")][:12]
    want = mmr_oracle.mmr_positions(q, X[order], 3, 0.5)
    assert _ids(got) == [f"B{int(order[p]):03d}" for p in want]
    # more picks asked than documents match: every match, once
    few = store.max_marginal_relevance_search_by_vector(q, k=50, fetch_k=60,
                                                        filter={"book_id": ["B001", "B004"]},
                                                        exact_filter=True)
    assert sorted(d.metadata["book_id"] for d in few) == ["B001", "B004"]


def test_store_mmr_pushes_the_reingested_copy_back(store):
    q = _query(store, 5, 40, 63)
    plain = store.similarity_search_by_vector(q, k=4)
    assert [d.metadata["book_id"] for d in plain[:2]] == ["B005", "B005"]
    mmr = store.max_marginal_relevance_search_by_vector(q, k=4, fetch_k=20, lambda_mult=0.5)
    assert [d.metadata["book_id"] for d in mmr].count("B005") == 1
    assert mmr[0].metadata["book_id"] == "B005"
    # the copy is still a candidate: it scores 0.5 * s - 0.5 * 1 and comes out later
    every = store.max_marginal_relevance_search_by_vector(q, k=20, fetch_k=20)
    assert [d.metadata["book_id"] for d in every].count("B005") == 2 and len(every) == 20


PROFILES = [[("B005", 1.0), ("B017", 0.5), ("nope", 0.8)],
            [("nope", 1.0)],
            [("B070", 0.3)],
            [(f"B{i:03d}", 0.1 + 0.1 * (i % 5)) for i in range(0, 60, 3)]]
READ = [["B006", "B007"], ["B001"], [], [f"B{i:03d}" for i in range(60, 80)]]


def test_store_recommend_for_profiles_mmr_on_oracle(store):
    index = store.index
    base = store.recommend_for_profiles(PROFILES, k=5, exclude=READ)
    index.calls.clear()
    assert store.recommend_for_profiles(PROFILES, k=5, exclude=READ, mmr=None) == base
    assert not any(c[0] in ("search_mmr", "mmr_select") for c in index.calls)
    got = store.recommend_for_profiles(PROFILES, k=5, exclude=READ, mmr=(20, 0.5))
    assert [len(r) for r in got] == [5, 0, 5, 5]
    kept, rows, lists = store.profile_requests(PROFILES, READ)
    vec = index.mean_rows(rows)
    D, I = index.search(vec, 20, exclude=lists)
    for j, p in enumerate(kept):
        want = mmr_oracle.mmr_positions(vec[j], index._x[I[j]], 5, 0.5)
        assert _ids(got[p]) == [store.docstore.search(store.index_to_docstore_id[int(I[j][w])])
                                .metadata["book_id"] for w in want]
        assert [s for _, s in got[p]] == [D[j][w] for w in want]
        barred = {b for b, _ in PROFILES[p]} | set(READ[p])
        assert not barred.intersection(_ids(got[p]))
    # lambda = 1 keeps the search order
    assert [_ids(r) for r in store.recommend_for_profiles(PROFILES, k=5, exclude=READ,
                                                          mmr=(5, 1.0))] == [_ids(r) for r in base]


def test_service_mmr_requests(store):
    # (before a service is started: a build without the methods fails here)
    assert hasattr(RemoteFAISS, "max_marginal_relevance_search_with_score_by_vector")
    assert hasattr(store, "max_marginal_relevance_search_with_score_by_vector")
    q = _query(store, 11, 40, 63)
    with IndexService(store, authkey=KEY) as svc:
        with RemoteFAISS(svc.address, KEY) as cli:
            before = svc.stats["search_batches"]
            want = store.max_marginal_relevance_search_with_score_by_vector(q, k=5, fetch_k=15,
                                                                            lambda_mult=0.3)
            got = cli.max_marginal_relevance_search_with_score_by_vector(q, k=5, fetch_k=15,
                                                                         lambda_mult=0.3)
            assert _ids(got) == _ids(want)
            assert [np.float32(s) for _, s in got] == [np.float32(s) for _, s in want]
            assert cli.max_marginal_relevance_search_by_vector(q) == \
                store.max_marginal_relevance_search_by_vector(q)
            assert cli.max_marginal_relevance_search("book 11", k=3) == \
                store.max_marginal_relevance_search("book 11", k=3)
            for exact in (False, True):
                assert cli.max_marginal_relevance_search_by_vector(
                    q, k=3, fetch_k=12, filter={"shelf": 1}, exact_filter=exact) == \
                    store.max_marginal_relevance_search_by_vector(
                        q, k=3, fetch_k=12, filter={"shelf": 1}, exact_filter=exact)
            with pytest.raises(ValueError):
                cli.max_marginal_relevance_search_by_vector(q, filter=lambda m: True)
            want = store.recommend_for_profiles(PROFILES, k=5, exclude=READ, mmr=(20, 0.5))
            got = cli.recommend_for_profiles(PROFILES, k=5, exclude=READ, mmr=(20, 0.5))
            assert [_ids(r) for r in got] == [_ids(r) for r in want]
            assert [[np.float32(s) for _, s in r] for r in got] == \
                [[np.float32(s) for _, s in r] for r in want]
            # MMR requests run on their own: none of them went through the coalescer
            assert svc.stats["search_batches"] == before
            plain = cli.recommend_for_profiles(PROFILES, k=5, exclude=READ)
            assert [_ids(r) for r in plain] == [
                _ids(r) for r in store.recommend_for_profiles(PROFILES, k=5, exclude=READ)]
            assert svc.stats["search_batches"] == before + 1


def test_recommend_frame_is_unchanged_without_mmr():
    """mmr=None sends the frame recommend_for_profiles always sent."""
    sent = []
    cli = RemoteFAISS.__new__(RemoteFAISS)
    cli._call = lambda header, payload=b"": (sent.append((header, payload)),
                                              ({"results": []}, b""))[1]
    cli.recommend_for_profiles([[("B001", 1.0)]], k=3, exclude=[["B002"]])
    cli.recommend_for_profiles([[("B001", 1.0)]], k=3, exclude=[["B002"]], mmr=None)
    old = {"op": "recommend_for_profiles", "k": 3, "key": "book_id",
           "profiles": [[["B001", 1.0]]], "exclude": [["B002"]]}
    assert sent[0] == (old, b"") and sent[1] == (old, b"")
    assert list(sent[0][0]) == list(old)  # key order too: the JSON bytes are the same
    cli.recommend_for_profiles([[("B001", 1.0)]], k=3, exclude=[["B002"]], mmr=(20, 0.25))
    assert sent[2] == (dict(old, mmr=[20, 0.25]), b"")
