"""CPU: where searches without a device — the store's predicate grammar and its
mapping to the arrays of vs_search_where, the window plan (vs_where_plan)
against a restated schedule, the argument checks of the new entry points over
null and zeroed handles, and the oracle on a hand-derived case."""

import ctypes

import numpy as np
import pytest

import where_oracle as wo
from oracle import flat
from vsearch import _lib
from vsearch import faiss as vfaiss
from vsearch import langchain as vlc

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
FMAX = np.finfo(np.float32).max
INF = np.inf
f32 = np.float32


# ---- the grammar -----------------------------------------------------------------------
NUMERIC = {"level", "pages", "year", "rating", "price"}


def _numeric(field):
    return field in NUMERIC


def _compile(pred):
    nums, pairs = vlc.where_layout([pred], _numeric)
    return nums, pairs, vlc.where_predicate(pred, nums, pairs)


def test_numeric_operators_map_to_closed_float32_ranges():
    nums, pairs, p = _compile({"level": {"$gte": 3.2, "$lte": 5.2}, "pages": {"$gt": 100},
                               "year": {"$lt": 2000}, "rating": 4})
    assert nums == ("level", "pages", "rating", "year") and pairs == ()
    lo, hi, masks = vfaiss.where_arrays(p, 4, 1)
    assert lo.dtype == hi.dtype == np.float32 and masks.dtype == np.uint64
    assert lo[0].tolist() == [f32(3.2), np.nextafter(f32(100), f32(INF)), f32(4), -INF]
    assert hi[0].tolist() == [f32(5.2), INF, f32(4), np.nextafter(f32(2000), f32(-INF))]
    assert masks.tolist() == [[0, 0, 0]]
    # a strict bound excludes the value itself and admits its float32 neighbour
    assert lo[0, 1] > f32(100) and hi[0, 3] < f32(2000)
    # conditions on one field intersect
    _, _, p = _compile({"level": {"$gte": 2, "$gt": 3, "$lte": 9, "$lt": 8}})
    assert p["lo"] == [float(np.nextafter(f32(3), f32(INF)))]
    assert p["hi"] == [float(np.nextafter(f32(8), f32(-INF)))]


def test_categorical_operators_map_to_tag_masks():
    pred = {"genre": {"$in": ["fantasy", "adventure"]}, "lang": "en",
            "topics": {"$all": ["dragons", "maps"]}, "format": {"$nin": ["audio"], "$neq": "braille"}}
    nums, pairs, p = _compile(pred)
    assert nums == ()
    bit = {pair: 1 << j for j, pair in enumerate(pairs)}
    assert len(bit) == 7
    assert p["any_of"] == bit[("genre", "fantasy")] | bit[("genre", "adventure")]
    # a single required value is tested through all_of (the same test)
    assert p["all_of"] == bit[("lang", "en")] | bit[("topics", "dragons")] | bit[("topics", "maps")]
    assert p["none_of"] == bit[("format", "audio")] | bit[("format", "braille")]
    assert p["lo"] == [] and p["hi"] == []
    _, _, p1 = _compile({"genre": {"$in": ["fantasy"]}})
    assert p1["any_of"] == 0 and p1["all_of"] == 1
    _, _, p0 = _compile({"genre": {"$in": []}})  # matches nothing
    assert p0["any_of"] & p0["none_of"]
    with pytest.raises(ValueError, match="more than one field"):
        _compile({"genre": {"$in": ["a", "b"]}, "lang": {"$in": ["en", "fr"]}})
    assert vlc.where_predicate(None, (), ()) is None


def test_layout_is_shared_by_the_predicates_of_a_batch():
    preds = [{"level": {"$lte": 3}, "genre": "fantasy"}, None,
             {"pages": {"$gte": 10}, "genre": {"$in": ["scifi", "fantasy"]}}]
    nums, pairs = vlc.where_layout(preds, _numeric)
    assert nums == ("level", "pages")
    assert pairs == (("genre", "fantasy"), ("genre", "scifi"))
    arr = [vlc.where_predicate(p, nums, pairs) for p in preds]
    lo, hi, masks = vfaiss.where_arrays(arr, 2, 3)
    assert lo.tolist() == [[-INF, -INF], [-INF, -INF], [-INF, 10.0]]
    assert hi.tolist() == [[3.0, INF], [INF, INF], [INF, INF]]
    assert masks.tolist() == [[0, 1, 0], [0, 0, 0], [3, 0, 0]]


def test_limits_and_bad_operators_name_the_general_route():
    five = {f: {"$gte": 0} for f in sorted(NUMERIC)}
    with pytest.raises(ValueError, match=r"more than 4 numeric fields.*exact_filter=True"):
        vlc.where_layout([five], _numeric)
    four = dict(list(five.items())[:4])
    assert len(vlc.where_layout([four], _numeric)[0]) == 4
    ok = {"genre": {"$in": [f"g{i}" for i in range(64)]}}
    assert len(vlc.where_layout([ok], _numeric)[1]) == 64
    with pytest.raises(ValueError, match=r"more than 64 \(field, value\) pairs.*exact_filter=True"):
        vlc.where_layout([ok, {"genre": "one more"}], _numeric)
    for bad in ({"level": {"$in": [1, 2]}}, {"level": {"$regex": "x"}}, {"genre": {"$gte": "a"}},
                {"genre": {"$like": "a"}}, {"$or": [{"genre": "a"}]}):
        with pytest.raises(ValueError, match=r"not supported.*filter= with exact_filter=True"):
            vlc.where_layout([bad], _numeric)
    with pytest.raises(ValueError, match="takes a number"):
        vlc.where_layout([{"level": {"$gte": "three"}}], _numeric)
    with pytest.raises(ValueError, match="takes a list"):
        vlc.where_layout([{"genre": {"$in": "fantasy"}}], _numeric)
    with pytest.raises(ValueError, match="a predicate is a dict"):
        vlc.where_layout([["genre", "a"]], _numeric)


def test_where_arrays_forms_and_checks():
    lo, hi, masks = vfaiss.where_arrays(None, 2, 3)
    assert lo.shape == hi.shape == (3, 2) and masks.shape == (3, 3)
    assert (lo == -INF).all() and (hi == INF).all() and not masks.any()
    one = dict(lo=[1, None], hi=[None, 2.5], any_of=5, none_of=2**63)
    lo, hi, masks = vfaiss.where_arrays(one, 2, 2)  # one predicate for every query
    assert lo.tolist() == [[1, -INF]] * 2 and hi.tolist() == [[INF, 2.5]] * 2
    assert masks.tolist() == [[5, 0, 2**63]] * 2
    lo2, hi2, m2 = vfaiss.where_arrays((lo, hi, masks), 2, 2)  # arrays pass through
    assert np.array_equal(lo2, lo) and np.array_equal(hi2, hi) and np.array_equal(m2, masks)
    lo, hi, masks = vfaiss.where_arrays(dict(all_of=3), 0, 1)  # tags only
    assert lo.shape == (1, 0) and masks.tolist() == [[0, 3, 0]]
    with pytest.raises(ValueError, match="2 predicates for 3 queries"):
        vfaiss.where_arrays([None, None], 1, 3)
    with pytest.raises(ValueError, match="lo holds 1 values for 2 columns"):
        vfaiss.where_arrays(dict(lo=[1]), 2, 1)
    with pytest.raises(ValueError, match="unknown keys"):
        vfaiss.where_arrays(dict(low=[1]), 1, 1)
    with pytest.raises(ValueError, match="NaN bound"):
        vfaiss.where_arrays(dict(lo=[float("nan")]), 1, 1)


def test_store_refuses_the_combinations():
    store = vlc.FAISS.__new__(vlc.FAISS)
    store._normalize_L2 = False
    q = [0.0] * 4
    for kw, msg in ((dict(distinct="book_id"), "where and distinct"),
                    (dict(exact_filter=True), "where and exact_filter")):
        with pytest.raises(ValueError, match=msg):
            store.similarity_search_with_score_by_vector(q, k=3, where={"level": 1}, **kw)
    with pytest.raises(ValueError, match="where and distinct"):
        store.similarity_search_batch_by_vector([q], k=3, where={"level": 1}, distinct="a")
    with pytest.raises(ValueError, match="where and mmr"):
        store.max_marginal_relevance_search_by_vector(q, k=3, where={"level": 1})
    with pytest.raises(ValueError, match="where and mmr"):
        store.recommend_for_profiles([], k=3, where=[], mmr=(20, 0.5))
    with pytest.raises(ValueError, match="where and distinct"):
        store.recommend_for_profiles([], k=3, where=[], distinct="author")


# ---- the window plan -------------------------------------------------------------------
def _schedule(k, metric, raw, live):
    """The plan restated: windows need + max(16, need / 2), four times longer
    every round, clipped to the live rows; a window is run while it is at most
    1,023 entries or every live row; what is left goes to the scan (0)."""
    need = 2 * k - 1 if metric == IP and not raw else k
    out = []
    if live == 0:
        return out
    w = need + max(16, need // 2)
    while True:
        w = min(w, live)
        if w < live and w > 1023:
            return out + [0]
        out.append(w)
        if w >= live:
            return out
        w *= 4


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("k", [1, 5, 10, 40, 64, 170, 400, 1024, 5000])
@pytest.mark.parametrize("live", [0, 1, 7, 26, 27, 1023, 1024, 3000, 4999, 10_000_000])
def test_plan_is_the_restated_schedule(metric, raw, k, live):
    plan = vfaiss.where_plan(k, metric, raw, live)
    assert plan == _schedule(k, metric, raw, live)
    windows = [w for w in plan if w]
    assert all(b == min(4 * a, live) for a, b in zip(windows, windows[1:]))  # x 4
    assert all(w <= 1023 or w == live for w in windows)
    if plan:
        assert plan[-1] == 0 or plan[-1] == live  # the scan, unless a window reached every row
        assert 0 not in plan[:-1]


def test_plan_examples_and_checks():
    assert vfaiss.where_plan(10, L2, False, 5000) == [26, 104, 416, 0]
    assert vfaiss.where_plan(10, IP, False, 5000) == [35, 140, 560, 0]
    assert vfaiss.where_plan(10, IP, True, 5000) == vfaiss.where_plan(10, L2, False, 5000)
    assert vfaiss.where_plan(10, L2, False, 400) == [26, 104, 400]
    assert vfaiss.where_plan(1000, L2, False, 5000) == [0]  # the first window is past 1,023
    assert vfaiss.where_plan(1000, L2, False, 1200) == [1200]
    lib = _lib.load()
    out = np.zeros(2, dtype=np.int64)
    # more entries than the caller has room for: the count is the whole plan's
    assert lib.vs_where_plan(10, L2, 0, 5000, out.ctypes.data, 2) == 4
    assert out.tolist() == [26, 104]
    for bad in ((0, L2, 0, 10), (2**30, L2, 0, 10), (1, 7, 0, 10), (1, L2, 0, -1)):
        assert lib.vs_where_plan(*bad, out.ctypes.data, 2) == _lib.E_INVALID


def test_stats_start_at_zero_and_check_their_outputs():
    assert vfaiss.where_stats(reset=True)[0] >= 0
    assert vfaiss.where_stats() == (0, 0, 0, 0, 0)
    assert _lib.load().vs_where_stats(None, None, None, None, None, 0) == _lib.E_INVALID
    assert _lib.last_error() == "vs_where_stats: null output"


# ---- C entry points --------------------------------------------------------------------
def _fake():
    return ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)


def test_search_where_argument_messages_in_order():
    """index, handle, n, k, k's bound, the bounds, the offsets, the buffers: each
    check answers only when the ones before it pass, and none of them reads the
    index (a zeroed handle has no columns, so no bound is read through it: the
    NaN-bound check is exercised on a real handle, tests/test_gpu_where.py)."""
    lib = _lib.load()
    fake, at = _fake(), _fake()
    b = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)

    def call(idx, a, n, k, lo=None, offs=None, labels=None, bufs=False):
        x = b if bufs else None
        return lib.vs_search_where(idx, a, x, n, k, lo, None, None, offs, labels, x, x, 0, None)

    def expect(tail, *a, **kw):
        assert call(*a, **kw) == _lib.E_INVALID, tail
        assert _lib.last_error() == f"vs_search_where: {tail}"

    expect("null index", None, None, -1, 0)
    expect("null attributes", fake, None, -1, 0)
    expect("n < 0", fake, at, -1, 0)
    expect("k must be > 0", fake, at, 1, 0)
    expect("k must be > 0", fake, at, 1, -3)
    expect("k too large", fake, at, 1, 2**30)
    assert call(fake, at, 0, 1) == 0  # no queries: success, before the arrays are looked at
    assert call(fake, at, 0, 0) == _lib.E_INVALID  # but after k
    bad = np.asarray([1, 1], dtype=np.int64)
    expect("offsets must start at 0 and not decrease", fake, at, 1, 5, None, bad.ctypes.data)
    one = np.asarray([0, 1], dtype=np.int64)
    expect("null exclusion labels", fake, at, 1, 1, None, one.ctypes.data)
    expect("null buffer", fake, at, 1, 5)
    expect("null buffer", fake, at, 1, 1, None, one.ctypes.data, one.ctypes.data)


def test_attrs_argument_messages_in_order():
    lib = _lib.load()
    fake = _fake()  # a zeroed index: no rows
    out = ctypes.c_void_p()
    cols = np.zeros(3, dtype=np.float32)

    def expect(tail, idx, ncol, p, n, o=ctypes.byref(out)):
        assert lib.vs_attrs_create(idx, ncol, p, None, n, None, o) == _lib.E_INVALID, tail
        assert _lib.last_error() == f"vs_attrs_create: {tail}"

    expect("null output", fake, 1, cols.ctypes.data, 3, None)
    expect("null index", None, 1, cols.ctypes.data, 3)
    expect("ncol must be in 0 .. 4", fake, 5, cols.ctypes.data, 3)
    expect("ncol must be in 0 .. 4", fake, -1, cols.ctypes.data, 3)
    expect("n < 0", fake, 1, cols.ctypes.data, -1)
    expect("null columns", fake, 1, None, 3)
    expect("n must equal the live row count", fake, 1, cols.ctypes.data, 3)
    expect("n must equal the live row count", fake, 0, None, 3)  # tags only, no columns
    assert not out.value
    assert lib.vs_attrs_destroy(None) == 0
    # an empty index takes an empty handle, which counts nothing and needs no device
    assert lib.vs_attrs_create(fake, 0, None, None, 0, None, ctypes.byref(out)) == 0
    assert out.value
    assert lib.vs_attrs_destroy(out) == 0

    cnt = np.zeros(1, dtype=np.int64)

    def count(a, nq, o):
        return lib.vs_attrs_count(a, None, None, None, nq, o, None)

    assert count(None, 1, cnt.ctypes.data) == _lib.E_INVALID
    assert _lib.last_error() == "vs_attrs_count: null attributes"
    assert count(_fake(), -1, cnt.ctypes.data) == _lib.E_INVALID
    assert _lib.last_error() == "vs_attrs_count: nq < 0"
    assert count(_fake(), 0, None) == 0
    assert count(_fake(), 1, None) == _lib.E_INVALID
    assert _lib.last_error() == "vs_attrs_count: null output"


# ---- the oracle on a hand-derived case -------------------------------------------------
def test_oracle_on_a_hand_derived_case():
    #         label   0    1    2      3    4    5
    level = np.array([1.0, 2.0, np.nan, 3.0, 4.0, 2.0], dtype=np.float32)
    tags = np.array([0b01, 0b11, 0b01, 0b10, 0b00, 0b01], dtype=np.uint64)
    scores = np.array([[6.0, 5.0, 4.0, 3.0, 2.0, 1.0]] * 4)
    lo = np.array([[2.0], [-INF], [-INF], [3.0]], dtype=np.float32)
    hi = np.array([[3.0], [INF], [INF], [2.0]], dtype=np.float32)
    masks = np.array([[0, 0, 0],          # level in [2, 3]
                      [0b01, 0, 0b10],    # has bit 0, not bit 1; the column is not tested
                      [0, 0b11, 0],       # both bits
                      [0, 0, 0]],         # lo > hi: nothing
                     dtype=np.uint64)
    mask = wo.pass_mask(level[None, :], tags, lo, hi, masks)
    assert mask.tolist() == [[False, True, False, True, False, True],   # NaN fails a tested column
                             [True, False, True, False, False, True],  # ... and passes an untested one
                             [False, True, False, False, False, False],
                             [False] * 6]
    D, I = wo.where_topk(scores, mask, 3, L2)
    assert I.tolist() == [[5, 3, 1], [5, 2, 0], [1, -1, -1], [-1, -1, -1]]
    assert D[0].tolist() == [1.0, 3.0, 5.0] and D[2, 1] == FMAX
    D, I = wo.where_topk(scores, mask, 2, IP, exclude=[[1], [], None, [0]])
    assert I.tolist() == [[3, 5], [0, 2], [1, -1], [-1, -1]]
    assert D[3, 0] == -FMAX
    # ties: faiss emits equal inner products by descending label, raw order ascending
    tied = np.ones((1, 6))
    m = np.array([[True, False, True, True, False, True]])
    assert wo.where_topk(tied, m, 4, IP)[1].tolist() == [[5, 3, 2, 0]]
    assert wo.where_topk(tied, m, 3, IP, rule="lex")[1].tolist() == [[0, 2, 3]]
    # no columns, no tags: every row passes
    assert wo.pass_mask(None, None, np.zeros((2, 0)), np.zeros((2, 0)),
                        np.zeros((2, 3), dtype=np.uint64), n=4).all()
