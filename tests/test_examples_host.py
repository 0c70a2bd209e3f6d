"""CPU: example searches without a device — the oracle on a hand-worked case, a
numpy model of the engine's rounds (truncated lists, F, S) against the
definition, the argument checks of vs_search_examples / vs_search_examples_x
over a zeroed handle, the CSR building, and the store's request assembly over
an oracle index."""

import ctypes

import numpy as np
import pytest

import examples_oracle as eo
from helpers import OracleIndex
from oracle import flat
from vsearch import _lib
from vsearch import faiss as vfaiss
from vsearch import langchain as vlc
from vsearch.synth import SynthEmbeddings

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
FMAX = np.finfo(np.float32).max


# ---- the oracle on a hand-worked case ------------------------------------------------------
def test_oracle_on_a_hand_worked_case():
    # one coordinate; rows at 0, 1, 2, 3, 10, 11; liked 1 and 10 (in that order), disliked 3
    xb = np.array([[0.0], [1.0], [2.0], [3.0], [10.0], [11.0]], dtype=np.float32)
    pos = np.array([[1.0], [10.0]], dtype=np.float32)
    neg = np.array([[3.0]], dtype=np.float32)
    # L2 keys   row:  0   1   2   3   4   5
    #   to 1:         1   0   1   4  81 100
    #   to 10:      100  81  64  49   0   1      p = 1 0 1 4 0 1, deciding 0 0 0 0 1 1
    #   to 3:         9   4   1   0  49  64      n = 9 4 1 0 49 64
    # favoured (p < n): rows 0, 1, 4, 5; row 2 ties p == n and is dropped; row 3 is nearer 3
    D, I, E = eo.search(xb, [(pos, neg)], 5, L2)
    assert I[0].tolist() == [1, 4, 0, 5, -1]
    assert D[0].tolist() == [0.0, 0.0, 1.0, 1.0, FMAX]
    assert E[0].tolist() == [0, 1, 0, 1, -1]
    # without the negative every row is favoured, ties by label
    D, I, E = eo.search(xb, [(pos, None)], 6, L2)
    assert I[0].tolist() == [1, 4, 0, 2, 5, 3] and E[0].tolist() == [0, 1, 0, 0, 1, 0]
    # exclusions come off before the cut at k
    D, I, E = eo.search(xb, [(pos, neg)], 2, L2, exclude=[[1, 4]])
    assert I[0].tolist() == [0, 5]
    # inner product: score = x * e; liked 1, disliked 10 -> p = -x, n = -10 x: favoured iff x < 0
    xs = np.array([[-2.0], [-1.0], [0.0], [1.0]], dtype=np.float32)
    D, I, E = eo.search(xs, [(pos[:1], pos[1:])], 3, IP)
    assert I[0].tolist() == [1, 0, -1] and D[0].tolist() == [-1.0, -2.0, -FMAX]
    # two equal positives: the lower position decides
    D, I, E = eo.search(xb, [(np.array([[2.0], [2.0]], np.float32), None)], 2, L2)
    assert I[0].tolist() == [2, 1] and E[0].tolist() == [0, 0]


def test_checker_accepts_the_oracle_and_sees_planted_faults():
    rng = np.random.default_rng(1)
    xb = rng.standard_normal((200, 16)).astype(np.float32)
    users = [(xb[[3, 50]], xb[[7]]), (xb[[9]], None)]
    excl = [[3, 50, 7], [9]]
    for metric in (L2, IP):
        D, I, E = eo.search(xb, users, 12, metric, exclude=excl)
        assert eo.problems(D, I, E, xb, users, 12, metric, exclude=excl) == []
        bad = I.copy()
        bad[0, 3] = 3  # an excluded label
        assert eo.problems(D, bad, E, xb, users, 12, metric, exclude=excl)
        swapped = I.copy()
        swapped[1, [0, 1]] = swapped[1, [1, 0]]  # D no longer belongs to the labels
        assert eo.problems(D, swapped, E, xb, users, 12, metric, exclude=excl)
        short = (D.copy(), I.copy(), E.copy())
        short[0][0, 11], short[1][0, 11], short[2][0, 11] = flat.neutral(metric), -1, -1
        assert eo.problems(*short, xb, users, 12, metric, exclude=excl)  # a favoured row missing
        # a row nearer the negative than any positive must not come back
        kp = eo.user_keys(xb, users[0][0], metric).min(axis=0)
        kn = eo.user_keys(xb, users[0][1], metric).min(axis=0)
        worst = int(np.argmax(kp - kn))
        planted = I.copy()
        planted[0, 11] = worst
        assert eo.problems(D, planted, E, xb, users, 12, metric, exclude=excl)


# ---- the rounds: truncated lists, F and S ---------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_rounds_model_equals_the_definition(metric):
    """The exactness argument on small cases with many ties and duplicate rows:
    whatever the window, the rows at or before F are known exactly."""
    rng = np.random.default_rng(5)
    seen_rounds = set()
    for case in range(120):
        n = int(rng.integers(1, 160))
        d = 3
        xb = rng.integers(-1, 2, size=(n, d)).astype(np.float32)
        if n > 4:
            xb[n // 2] = xb[0]  # duplicate rows
        a, b = int(rng.integers(1, 5)), int(rng.integers(0, 4))
        pos = rng.integers(-1, 2, size=(a, d)).astype(np.float32)
        if a > 1 and case % 3 == 0:
            pos[1] = pos[0]
        neg = rng.integers(-1, 2, size=(b, d)).astype(np.float32)
        if b and case % 4 == 0:
            neg[0] = pos[0]  # liked and disliked at once: every row ties or loses
        excl = rng.choice(n, size=int(rng.integers(0, n // 2 + 1)), replace=False)
        allowed = eo.allowed_mask(n, excl)
        k = int(rng.integers(1, 12))
        kp, kn = eo.user_keys(xb, pos, metric), eo.user_keys(xb, neg, metric)
        want = eo.from_keys(kp, kn, allowed, k, metric)
        got, rounds = eo.rounds_model(kp, kn, allowed, k, metric)
        seen_rounds.add(rounds)
        for w, g in zip(want, got):
            assert np.array_equal(w, g), (case, w, g)
    assert len(seen_rounds) > 1  # some cases needed a longer window


def test_window_schedule_is_the_distinct_searches():
    for k in (1, 10, 40, 1024):
        for live in (1, 50, 3000, 10**6):
            assert [eo.window(k, r, live) for r in range(len(vfaiss.distinct_plan(k, L2, True,
                                                                                  live)))] \
                == vfaiss.distinct_plan(k, L2, True, live)
    assert [eo.window(10, r, 3000) for r in range(3)] == [26, 104, 416]


# ---- C entry points --------------------------------------------------------------------------
def _fake():
    return ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)


@pytest.mark.parametrize("form", ["labels", "vectors"])
def test_search_examples_argument_messages_in_order(form):
    """index, n, k, k's limit, the offsets, a positive per user, the list
    limit, the exclusion offsets, the buffers: each check answers only when the
    ones before it pass, and none of them reads the index (a zeroed handle)."""
    lib = _lib.load()
    fake = _fake()
    b = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    name = "vs_search_examples" if form == "labels" else "vs_search_examples_x"

    def call(idx, n, k, poffs=None, noffs=None, eoffs=None, elab=None, bufs=False):
        x = b if bufs else None
        po = poffs.ctypes.data if poffs is not None else None
        no = noffs.ctypes.data if noffs is not None else None
        eo_ = eoffs.ctypes.data if eoffs is not None else None
        if form == "labels":
            return lib.vs_search_examples(idx, po, x, no, x, n, k, eo_, elab, 1, x, x, x, 0, None)
        return lib.vs_search_examples_x(idx, po, x, no, x, n, k, eo_, elab, x, x, x, 0, None)

    def expect(tail, *a, code=_lib.E_INVALID, **kw):
        assert call(*a, **kw) == code, tail
        assert _lib.last_error().startswith(f"{name}: {tail}"), _lib.last_error()

    i64 = lambda *v: np.asarray(v, dtype=np.int64)  # noqa: E731
    expect("null index", None, -1, 0)
    expect("n < 0", fake, -1, 0)
    expect("k must be > 0", fake, 1, 0)
    expect("k > 1024", fake, 1, 1025, code=_lib.E_UNSUPPORTED)
    assert call(fake, 0, 1025) == _lib.E_UNSUPPORTED  # before the empty call's success
    assert call(fake, 0, 1024) == 0
    expect("null offsets", fake, 1, 1)
    expect("offsets must start at 0 and not decrease", fake, 1, 1, i64(1, 1))
    expect("offsets must start at 0 and not decrease", fake, 2, 1, i64(0, 2, 1))
    expect("offsets must start at 0 and not decrease", fake, 1, 1, i64(0, 1), i64(0, -1))
    expect("a user without a positive example", fake, 2, 1, i64(0, 1, 1))
    expect("more than 64 positive or 64 negative examples of one user", fake, 2, 1, i64(0, 1, 66),
           code=_lib.E_UNSUPPORTED)
    expect("more than 64 positive or 64 negative examples of one user", fake, 1, 1, i64(0, 64),
           i64(0, 65), code=_lib.E_UNSUPPORTED)
    # a user without a positive is reported before another user's long list
    expect("a user without a positive example", fake, 2, 1, i64(0, 65, 65))
    expect("offsets must start at 0 and not decrease", fake, 1, 1, i64(0, 64), i64(0, 64),
           i64(1, 1))
    expect("null exclusion labels", fake, 1, 1, i64(0, 1), None, i64(0, 1))
    expect("null buffer", fake, 1, 1, i64(0, 64), i64(0, 64))
    expect("null buffer", fake, 1, 1, i64(0, 1), None, i64(0, 0))


def test_examples_stats_check_their_outputs():
    lib = _lib.load()
    a = ctypes.c_int64(-1)
    assert lib.vs_examples_stats(ctypes.byref(a), None, None, 0) == _lib.E_INVALID
    assert _lib.last_error() == "vs_examples_stats: null output"
    users, rounds, requeried = vfaiss.examples_stats(reset=True)
    assert vfaiss.examples_stats() == (0, 0, 0)


# ---- CSR building -----------------------------------------------------------------------------
def test_examples_csr_label_and_vector_forms():
    offs, labels, vec = vfaiss.examples_csr([[3, 4], (), [7]])
    assert offs.tolist() == [0, 2, 2, 3] and labels.tolist() == [3, 4, 7] and vec is None
    assert labels.dtype == np.int64 and offs.dtype == np.int64
    offs, labels, vec = vfaiss.examples_csr(None, 2)
    assert offs.tolist() == [0, 0, 0] and labels.size == 0 and vec is None
    a = np.arange(6, dtype=np.float64).reshape(2, 3)
    offs, labels, vec = vfaiss.examples_csr([a, None, a[:1]], 3, 3)
    assert labels is None and offs.tolist() == [0, 2, 2, 3]
    assert vec.dtype == np.float32 and vec.shape == (3, 3) and vec.flags.c_contiguous
    assert vec[2].tolist() == [0.0, 1.0, 2.0]
    with pytest.raises(ValueError):
        vfaiss.examples_csr([a, [1, 2]])  # mixed forms
    with pytest.raises(ValueError):
        vfaiss.examples_csr([a], 1, 4)  # wrong width
    with pytest.raises(ValueError):
        vfaiss.examples_csr([[1]], 2)  # wrong user count


# ---- the store's request assembly --------------------------------------------------------------
class ExamplesOracleIndex(OracleIndex):
    """OracleIndex with IndexFlat.search_examples, answered by examples_oracle."""

    def __init__(self, d, metric=L2):
        super().__init__(d, metric)
        self.calls = []

    def search_examples(self, positive, negative=None, k=10, *, exclude=None,
                        exclude_examples=True, return_example=False):
        self.calls.append((positive, negative, k, exclude, exclude_examples))
        vec = lambda e: e if isinstance(e, np.ndarray) and e.ndim == 2 else self._x[list(e)]  # noqa: E731
        users = [(vec(p), vec(n) if negative is not None else None)
                 for p, n in zip(positive, negative if negative is not None else positive)]
        D, I, E = eo.search(self._x, users, k, self.metric_type, exclude=exclude)
        return (D, I, E) if return_example else (D, I)


N_BOOKS = 30


def _meta(i):
    return {"book_id": f"B{i:03d}", "author": f"A{i % 7}"}


@pytest.fixture()
def store(monkeypatch):
    monkeypatch.setattr(vfaiss, "IndexFlatL2", lambda d, **kw: ExamplesOracleIndex(d, L2))
    emb = SynthEmbeddings(48)
    st = vlc.FAISS.from_texts([f"book {i}" for i in range(N_BOOKS)], emb,
                              metadatas=[_meta(i) for i in range(N_BOOKS)])
    # re-embedded copies: a second row for every third book
    st.add_texts([f"book {i} again" for i in range(0, N_BOOKS, 3)],
                 metadatas=[_meta(i) for i in range(0, N_BOOKS, 3)])
    return st


def test_example_requests_assembly(store):
    liked = [["B000", "B004", "nope"], ["nope"], ["B005"]]
    disliked = [["B003", "gone"], ["B001"], []]
    exclude = [["B006"], [], ["B009", "absent"]]
    kept, pos, neg, lists, names = store.example_requests(liked, disliked, exclude)
    assert kept == [0, 2]
    # a key's first row stands for it; B000, B003, B006 and B009 have a second row (30 + i / 3)
    assert pos == [[0, 4], [5]] and neg == [[3], []]
    assert names == [["B000", "B004"], ["B005"]]
    assert sorted(lists[0]) == [0, 3, 4, 6, 30, 31, 32] and sorted(lists[1]) == [5, 9, 33]


def test_recommend_from_examples_over_an_oracle_index(store):
    liked = [["B000", "B004"], ["nope"], ["B005"]]
    disliked = [["B003"], ["B001"], None]
    disliked[2] = []
    exclude = [["B006"], [], ["B009"]]
    res = store.recommend_from_examples(liked, disliked, 5, exclude=exclude, with_reason=True)
    assert res[1] == [] and len(store.index.calls) == 1
    positive, negative, k, lists, exclude_examples = store.index.calls[0]
    assert k == 5 and exclude_examples is False and positive == [[0, 4], [5]]
    for u, banned in ((0, {"B000", "B004", "B003", "B006"}), (2, {"B005", "B009"})):
        assert len(res[u]) == 5
        ids = [doc.metadata["book_id"] for doc, _, _ in res[u]]
        assert not banned & set(ids)
        scores = [s for _, s, _ in res[u]]
        assert scores == sorted(scores)
        assert all(reason in liked[u] for _, _, reason in res[u])
    plain = store.recommend_from_examples(liked, disliked, 5, exclude=exclude)
    assert [[(d.metadata["book_id"], s) for d, s in r] for r in plain] == \
        [[(d.metadata["book_id"], s) for d, s, _ in r] for r in res]
    # a store that normalises its vectors hands the examples over as vectors
    store._normalize_L2 = True
    store.recommend_from_examples(liked, disliked, 3, exclude=exclude)
    positive, negative, k, lists, _ = store.index.calls[-1]
    assert isinstance(positive[0], np.ndarray) and positive[0].shape == (2, 48)
    assert negative[1].shape == (0, 48)
    np.testing.assert_allclose(np.linalg.norm(positive[0], axis=1), 1.0, rtol=1e-6)
    with pytest.raises(ValueError):
        store.recommend_from_examples(liked, disliked[:2], 3)
