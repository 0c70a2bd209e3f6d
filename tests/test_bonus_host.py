"""CPU: bonus searches without a device — the oracle on a hand-derived case,
``bonus_csr``'s shapes, defaults and errors, ``neighbour_bonus`` against a
literal restatement of the reference's loop, the store's ``bonus=`` grammar and
the argument checks that need no device."""

import ctypes

import numpy as np
import pytest

import bonus_oracle as bno
from helpers import OracleIndex
from oracle import flat
from vsearch import _lib
from vsearch import faiss as vfaiss
from vsearch import langchain as vlc
from vsearch import students
from vsearch.synth import SynthEmbeddings

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
f32 = np.float32


# ---- the oracle itself ------------------------------------------------------------------
def test_oracle_on_a_hand_derived_case():
    # inner-product scores of 6 rows for one query, nearest first
    scores = np.array([[1.0, 0.875, 0.75, 0.5, 0.25, 0.125]])
    # row 5 (the farthest) is promoted past everything, row 0 (the nearest) is
    # demoted to 0.25 where it ties the unlisted row 4, and row 3 is lifted to
    # 0.75 where it ties the unlisted row 2: the lower label wins both ties
    lists = [{5: 1.0, 0: -0.75, 3: 0.25, 99: 5.0, -1: 5.0}]
    s, listed = bno.dense_lists(lists, 1, 6)
    assert listed.tolist() == [[True, False, False, True, False, True]]
    assert s.tolist() == [[-0.75, 0.0, 0.0, 0.25, 0.0, 1.0]]
    fin = bno.final_keys(scores, None, s, listed, IP)
    assert fin.dtype == np.float32
    assert fin.tolist() == [[-0.25, -0.875, -0.75, -0.75, -0.25, -1.125]]
    D, I = bno.bonus_topk(scores, None, s, listed, None, 6, IP)
    assert I.tolist() == [[5, 1, 2, 3, 0, 4]]
    assert D.tolist() == [[1.125, 0.875, 0.75, 0.75, 0.25, 0.25]]
    D, I = bno.bonus_topk(scores, None, s, listed, None, 2, IP)
    assert I.tolist() == [[5, 1]]
    # a listed row that is masked or excluded is no candidate, whatever its bonus
    mask = np.array([[True, True, True, True, True, False]])
    D, I = bno.bonus_topk(scores, None, s, listed, mask, 6, IP, exclude=[[1]])
    assert I.tolist() == [[2, 3, 0, 4, -1, -1]] and D[0, 4] == flat.neutral(IP)
    # a boost composes: b lifts row 4 to 0.5, above the demoted row 0
    b = np.array([[0, 0, 0, 0, 0.25, 0]], dtype=np.float32)
    D, I = bno.bonus_topk(scores, b, s, listed, None, 6, IP)
    assert I.tolist() == [[5, 1, 2, 3, 4, 0]] and D[0, 4] == 0.5
    # L2: the bonus is subtracted from the distance, and D may be negative
    D, I = bno.bonus_topk(scores, None, s, listed, None, 3, L2)
    assert I.tolist() == [[5, 3, 4]] and D.tolist() == [[-0.875, 0.25, 0.25]]
    # s = +0 on a listed row changes nothing
    s0, l0 = bno.dense_lists([{2: 0.0}], 1, 6)
    assert np.array_equal(bno.final_keys(scores, b, s0, l0, IP).view(np.uint32),
                          bno.final_keys(scores, b, s0 * 0, l0 & False, IP).view(np.uint32))


def test_oracle_rounds_twice():
    # key - b and (key - b) - s are rounded separately: 1 - 2^-25 rounds to 1
    # (a tie, to even), and then 1 - 2^-25 does again; one rounding of the
    # exact 1 - 2^-24 would give the float below 1
    scores = np.array([[1.0]])
    b = np.array([[2.0 ** -25]], dtype=np.float32)
    s, listed = bno.dense_lists([{0: 2.0 ** -25}], 1, 1)
    assert bno.final_keys(scores, b, s, listed, L2)[0, 0] == f32(1.0)
    assert f32(1.0 - 2.0 ** -24) < f32(1.0)


def test_oracle_mismatches_tolerance():
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((50, 8)).astype(np.float32)
    xq = rng.standard_normal((2, 8)).astype(np.float32)
    b = rng.uniform(0, 0.5, size=(2, 50)).astype(np.float32)
    s, listed = bno.dense_lists([{3: 1.5, 7: -2.0, 11: 0.25}, {4: -1.0}], 2, 50)
    for metric in (IP, L2):
        sc = flat.exact_scores(xb, xq, metric)
        Dr, Ir = bno.bonus_topk(sc, b, s, listed, None, 5, metric)
        assert bno.mismatches(Dr, Ir, Dr, Ir, metric, xb, xq, b, s, listed) == []
        D = Dr.copy()
        D[0, 0] += 1e-3
        assert [p[2] for p in bno.mismatches(D, Ir, Dr, Ir, metric, xb, xq, b, s, listed)] == \
            ["score"]
        I = Ir.copy()
        I[1, 0], I[1, 4] = Ir[1, 4], Ir[1, 0]
        assert any(p[2] == "label"
                   for p in bno.mismatches(Dr, I, Dr, Ir, metric, xb, xq, b, s, listed))


# ---- bonus_csr --------------------------------------------------------------------------
def test_bonus_csr_shapes_defaults_and_errors():
    offs, labels, vals = vfaiss.bonus_csr(None, 3)
    assert offs.tolist() == [0, 0, 0, 0] and offs.dtype == np.int64
    assert labels.size == 0 and labels.dtype == np.int64
    assert vals.size == 0 and vals.dtype == np.float32
    offs, labels, vals = vfaiss.bonus_csr([{7: 0.5, 2: -1}, None, ([4, 9, 1], [1, 2, 3]), {}], 4)
    assert offs.tolist() == [0, 2, 2, 5, 5]
    assert labels.tolist() == [7, 2, 4, 9, 1] and vals.tolist() == [0.5, -1.0, 1.0, 2.0, 3.0]
    assert vals.dtype == np.float32 and labels.dtype == np.int64
    again = vfaiss.bonus_csr((offs, labels, vals), 4)  # a ready CSR passes through
    assert all(np.array_equal(a, b) for a, b in zip(again, (offs, labels, vals)))
    # unknown labels and -1 are the search's business, not an error here
    assert vfaiss.bonus_csr([{-1: 1.0, 10 ** 12: 2.0}], 1)[1].tolist() == [-1, 10 ** 12]
    full = (np.arange(1024), np.ones(1024))
    assert vfaiss.bonus_csr([full], 1)[0].tolist() == [0, 1024]
    assert vfaiss.MAX_BONUS_LIST == 1024
    for bad, n, msg in [
        ([{1: 1.0}], 2, "expected 2 lists, got 1"),
        ({1: 1.0}, 1, "one entry per query"),
        ([([1, 2], [1.0])], 1, "as many values as labels"),
        ([([1, 2], [1.0, 2.0], [3])], 1, "a list is a dict"),
        ([{1: np.nan}], 1, "not finite"),
        ([{1: np.inf}], 1, "not finite"),
        ([([1, 2], [1.0, -np.inf])], 1, "not finite"),
        ([([3, 5, 3], [1.0, 2.0, 3.0])], 1, "a label twice"),
        ([(np.arange(1025), np.ones(1025))], 1, "longer than 1024"),
        ((np.array([0, 2]), np.array([1]), np.array([1.0], dtype=np.float32)), 1,
         "offsets must rise"),
        ((np.array([0, 2, 1]), np.array([1, 2]), np.array([1.0, 2.0], dtype=np.float32)), 2,
         "offsets must rise"),
    ]:
        with pytest.raises(ValueError, match=msg):
            vfaiss.bonus_csr(bad, n)


# ---- neighbour_bonus --------------------------------------------------------------------
def _reference_social(neighbours, checkouts, student, weight, top=5):
    """candidate_builder.py:394-412 as a literal loop: the `top` rows of
    student_similarity WHERE a = student ORDER BY sim DESC, then one count per
    checkout row of those neighbours."""
    rows_sim = sorted([(b, sim) for a, b, sim in neighbours if a == student],
                      key=lambda r: -r[1])[:top]
    nbr_ids = [r[0] for r in rows_sim]
    nbr_recent_counts = {}
    if nbr_ids:
        for s, bid in checkouts:
            if s in nbr_ids:
                nbr_recent_counts[bid] = nbr_recent_counts.get(bid, 0) + 1
    return {bid: f32(weight) * f32(c) for bid, c in nbr_recent_counts.items()}


def test_neighbour_bonus_equals_the_reference_loop():
    neighbours = [
        ("s1", "n1", 0.99), ("s1", "n2", 0.95), ("s1", "n3", 0.91), ("s1", "n4", 0.90),
        ("s1", "n5", 0.80), ("s1", "n6", 0.80),  # an equal sim at the cut: n5 (earlier) stays
        ("s1", "n7", 0.79),
        ("s2", "n1", 0.5), ("s2", "s1", 0.7),
        ("s3", "n8", 0.9),  # n8 checked nothing out: s3 has no entry
    ]
    checkouts = [("n1", "B1"), ("n2", "B1"), ("n1", "B1"),  # a repeated row counts again
                 ("n5", "B2"), ("n6", "B3"), ("n7", "B4"), ("s1", "B5"), ("zz", "B1"),
                 ("n4", "B2")]
    got = students.neighbour_bonus(neighbours, checkouts)
    assert set(got) == {"s1", "s2"}
    for st in ("s1", "s2", "s3"):
        ref = _reference_social(neighbours, checkouts, st, 0.2)
        assert got.get(st, {}) == ref
    assert got["s1"] == {"B1": f32(0.2) * f32(3), "B2": f32(0.2) * f32(2)}  # no B3: n6 is cut
    assert all(isinstance(v, np.float32) for v in got["s1"].values())
    assert got["s2"] == {"B1": f32(0.2) * f32(2), "B5": f32(0.2)}
    one = students.neighbour_bonus(neighbours, checkouts, weight=0.5, top=1)
    assert one == {"s1": {"B1": f32(1.0)}, "s2": {"B5": f32(0.5)}}
    assert one["s1"] == _reference_social(neighbours, checkouts, "s1", 0.5, top=1)
    assert students.neighbour_bonus([], checkouts) == {}
    assert students.neighbour_bonus(neighbours, []) == {}


# ---- the store grammar ------------------------------------------------------------------
@pytest.fixture
def store(monkeypatch):
    monkeypatch.setattr(vfaiss, "IndexFlatL2", lambda d, **kw: OracleIndex(d, flat.METRIC_L2))
    texts = [f"book {i}" for i in range(6)]
    metas = [{"book_id": f"B{i % 4}", "isbn": i} for i in range(6)]  # B0 and B1 hold two rows
    return vlc.FAISS.from_texts(texts, SynthEmbeddings(8), metadatas=metas)


def test_store_bonus_lists_and_errors(store):
    lists = store._bonus_lists({"B0": 0.5, "B3": -1, "nope": 9.0}, 2, "book_id")
    assert lists == [{0: 0.5, 4: 0.5, 3: -1.0}] * 2  # every row of a re-embedded book
    lists = store._bonus_lists([None, {"B1": f32(0.25)}, {}], 3, "book_id")
    assert lists == [{}, {1: 0.25, 5: 0.25}, {}]
    assert store._bonus_lists({2: 1.5}, 1, "isbn") == [{2: 1.5}]
    assert store._bonus_lists(None, 2, "book_id") == [{}, {}]
    for bad, n, msg in [
        ([{"B0": 1.0}], 2, "1 lists for 2 queries"),
        ([[("B0", 1.0)]], 1, "a dict from book_id values to numbers"),
        ({"B0": "high"}, 1, "needs a finite number"),
        ({"B0": float("nan")}, 1, "needs a finite number"),
        ({"B0": float("inf")}, 1, "needs a finite number"),
        ({"B0": True}, 1, "needs a finite number"),
    ]:
        with pytest.raises(ValueError, match=msg):
            store._bonus_lists(bad, n, "book_id")
    b = {"B0": 1.0}
    vec = [0.0] * 8
    profiles = [[("B0", 1.0)]]
    for call, msg in [
        (lambda: store.similarity_search("x", k=2, bonus=b, distinct="book_id"), "not built"),
        (lambda: store.similarity_search("x", k=2, bonus=b, filter={"book_id": "B0"}),
         "not built"),
        (lambda: store.similarity_search_by_vector(vec, k=2, bonus=b, filter={"isbn": 1},
                                                   exact_filter=True), "not built"),
        (lambda: store.max_marginal_relevance_search("x", k=2, bonus=b), "not built"),
        (lambda: store.max_marginal_relevance_search_by_vector(vec, k=2, bonus=b), "not built"),
        (lambda: store.similarity_search_batch_by_vector([vec], k=2, bonus=b,
                                                         distinct="book_id"), "not built"),
        (lambda: store.recommend_for_profiles(profiles, k=2, bonus=b, mmr=(4, 0.5)),
         "not built"),
        (lambda: store.recommend_for_profiles(profiles, k=2, bonus=b, distinct="book_id"),
         "not built"),
        (lambda: store.recommend_for_profiles(profiles, k=2, bonus=[b, b]), "bonus"),
    ]:
        with pytest.raises(ValueError, match=msg):
            call()


# ---- the C-ABI's checks that need no device ---------------------------------------------
def test_argument_checks_without_a_device():
    lib = _lib.load()
    z = ctypes.c_void_p(None)
    assert lib.vs_search_bonus(z, z, None, 1, 1, None, None, None, None, None, None, None, None,
                               None, None, None, None, None, None, 0, None) == _lib.E_INVALID
    assert b"vs_search_bonus: null index" in lib.vs_last_error()
    assert lib.vs_bonus_stats(None, None, None, None, 0) == _lib.E_INVALID
    assert b"vs_bonus_stats" in lib.vs_last_error()
    one = ctypes.c_int64(0)
    assert lib.vs_bonus_stats(ctypes.byref(one), None, ctypes.byref(one), ctypes.byref(one),
                              0) == _lib.E_INVALID
    s = vfaiss.bonus_stats()
    assert len(s) == 4 and all(isinstance(v, int) for v in s)
