"""GPU: where searches (vs_search_where): exact top-k under a predicate that
differs per query, through both routes (the windows and the predicated scan).

Oracle: ``where_oracle.where_topk`` — the boolean mask of the definition, then
``flat.select_topk`` over ``flat.exact_scores`` — compared with
``flat.mismatches`` at its default tolerance; on small-integer rows
(``rng.integers(-2, 3)``, every score exact in fp32) I and D are compared for
equality.  d = 96; 3,000 or 4,999 rows, so the last tile is partial."""

import numpy as np
import pytest

import where_oracle as wo
from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
DIM = 96
INF = np.inf


@pytest.fixture(scope="module")
def vf():
    from vsearch import _lib
    from vsearch import faiss as vfaiss

    assert _lib.device_count() >= 1
    return vfaiss


def _data(nq, n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, DIM)).astype(np.float32),
            rng.standard_normal((nq, DIM)).astype(np.float32))


def _int_data(nq, n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(-2, 3, size=(n, DIM)).astype(np.float32),
            rng.integers(-2, 3, size=(nq, DIM)).astype(np.float32))


def _attr_data(n, seed=1):
    """Two columns — a uniform level in [0, 10), a page count with a tenth of
    the values unknown — and six tag bits."""
    rng = np.random.default_rng(seed)
    level = rng.uniform(0, 10, n).astype(np.float32)
    pages = rng.integers(50, 900, n).astype(np.float32)
    pages[rng.random(n) < 0.1] = np.nan
    tags = rng.integers(0, 64, n).astype(np.uint64)
    return np.stack([level, pages]), tags


def _bands(nq, targets, seed=2):
    """One band of the level column per query: about targets[q % len] of the rows
    pass; a target of None is lo > hi (nothing)."""
    rng = np.random.default_rng(seed)
    lo = np.full((nq, 2), -INF, dtype=np.float32)
    hi = np.full((nq, 2), INF, dtype=np.float32)
    for q in range(nq):
        p = targets[q % len(targets)]
        if p is None:
            lo[q, 0], hi[q, 0] = 6.0, 4.0
        elif p < 1:
            c = rng.uniform(5 * p, 10 - 5 * p)
            lo[q, 0], hi[q, 0] = c - 5 * p, c + 5 * p
    return lo, hi, np.zeros((nq, 3), dtype=np.uint64)


def _check(index, attrs, xb, xq, cols, tags, where, k, *, raw=False, scan=False, exclude=None,
           exact=False):
    """One where search against the oracle; xb / xq are the values the index
    and the call hold (rounded for a bf16 index).  Returns (D, I, mask)."""
    metric = index.metric_type
    nq, n = xq.shape[0], xb.shape[0]
    lo, hi, masks = where
    mask = wo.pass_mask(cols, tags, lo, hi, masks, n=n)
    scores = flat.exact_scores(xb, xq, metric)
    Dr, Ir = wo.where_topk(scores, mask, k, metric, exclude=exclude,
                           rule="lex" if raw else "faiss")
    D, I = index.search_where(xq, k, attrs, where, exclude=exclude, raw=raw, scan=scan)
    allowed = mask & ~wo.excluded_mask(exclude, nq, n)
    for q in range(nq):
        got = I[q][I[q] >= 0]
        assert allowed[q][got].all(), ("a row that fails its predicate came back", q)
        assert got.size == min(k, int(allowed[q].sum())), (q, got.size, int(allowed[q].sum()))
    if exact:
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_array_equal(D, Dr)
    else:
        bad = flat.mismatches(D, I, Dr, Ir, metric, xb, xq)
        assert not bad, bad[:5]
    return D, I, mask


# ---- 1. the predicate that tests nothing ---------------------------------------------
@pytest.fixture(scope="module")
def int_indexes(vf):
    xb, _ = _int_data(1, 3000)
    cols, tags = _attr_data(3000)
    out = {}
    for metric in (L2, IP):
        index = vf.IndexFlat(DIM, metric)
        index.add(xb)
        out[metric] = (index, index.attributes(cols, tags))
    return xb, cols, tags, out


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 40, 129])
def test_no_predicate_is_the_plain_search(vf, int_indexes, metric, nq):
    xb, cols, tags, idx = int_indexes
    index, attrs = idx[metric]
    _, xq = _int_data(nq, 3000, seed=3)
    for raw in (False, True):
        D0, I0 = index.search(xq, 10, raw=raw)
        for where in (None, vf.where_arrays(None, 2, nq), dict(lo=[-INF, None], hi=[INF, INF])):
            D, I = index.search_where(xq, 10, attrs, where, raw=raw)  # route A: bit for bit
            np.testing.assert_array_equal(I, I0)
            np.testing.assert_array_equal(D.view(np.uint32), D0.view(np.uint32))
        D, I = index.search_where(xq, 10, attrs, None, raw=raw, scan=True)
        np.testing.assert_array_equal(I, I0)
        np.testing.assert_array_equal(D, D0)


# ---- 2. random per-query predicates --------------------------------------------------
@pytest.fixture(scope="module")
def normal_indexes(vf):
    xb, _ = _data(1, 4999)
    cols, tags = _attr_data(4999)
    out = {}
    for metric in (L2, IP):
        index = vf.IndexFlat(DIM, metric)
        index.add(xb)
        out[metric] = (index, index.attributes(cols, tags))
    return xb, cols, tags, out


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("scan", [False, True])
def test_random_predicates_of_every_selectivity(vf, normal_indexes, metric, scan):
    xb, cols, tags, idx = normal_indexes
    index, attrs = idx[metric]
    nq = 40
    _, xq = _data(nq, 4999, seed=4)
    where = _bands(nq, [1, 0.3, 0.03, 0.003, None])
    D, I, mask = _check(index, attrs, xb, xq, cols, tags, where, 10, scan=scan)
    matches = mask.sum(axis=1)
    np.testing.assert_array_equal(attrs.count(where), matches)
    assert (matches[4::5] == 0).all() and (I[4::5] == -1).all()  # "nothing" is all padding
    assert (D[4::5] == flat.neutral(metric)).all()
    assert matches[3::5].max() < 60 < matches[2::5].min()  # 0.003 and 0.03 of 4,999 rows
    assert ((I >= 0).sum(axis=1) == np.minimum(10, matches)).all()


# ---- 3. the scan: kernels, pages, dtypes ---------------------------------------------
@pytest.fixture(scope="module")
def scan_indexes(vf):
    xb, _ = _data(1, 4999, seed=5)
    cols, tags = _attr_data(4999, seed=6)
    out = {}
    for dtype in ("f32", "bf16"):
        for metric in (L2, IP):
            index = vf.IndexFlat(DIM, metric, dtype=dtype)
            index.add(xb)
            out[dtype, metric] = (index, index.attributes(cols, tags))
    return xb, cols, tags, out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nq", [1, 8, 9, 33, 129])
def test_scan_over_batches_pages_and_dtypes(vf, scan_indexes, dtype, nq):
    """nq 1 .. 33: the GEMV / GEMM switch (at most 32 queries stream, 8 per
    pass) and padded query tiles; k = 40 under the inner-product rule reads 79
    entries and k = 70 reads 70: two pages."""
    xb, cols, tags, idx = scan_indexes
    _, xq = _data(nq, 4999, seed=7)
    if dtype == "bf16":
        xb, xq = flat.round_bf16(xb), flat.round_bf16(xq)
    where = _bands(nq, [0.5, 0.1, 1, 0.02])
    where[2][:, 0] = np.uint64(0b101)  # and any of two tag bits
    for metric in (L2, IP):
        index, attrs = idx[dtype, metric]
        for k in (1, 10, 40, 70):
            _check(index, attrs, xb, xq, cols, tags, where, k, scan=True)
    _check(idx[dtype, IP][0], idx[dtype, IP][1], xb, xq, cols, tags, where, 40, scan=True, raw=True)


# ---- 4. the automatic route ----------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_auto_route_reaches_the_scan(vf, metric):
    n, k = 5000, 10
    xb, xq = _data(40, n, seed=8)
    rng = np.random.default_rng(9)
    level = np.full(n, 5.0, dtype=np.float32)
    level[rng.choice(n, 12, replace=False)] = 1.0
    level[rng.choice(np.nonzero(level == 5.0)[0], 2000, replace=False)] = 3.0  # 40 %
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    plan = vf.where_plan(k, metric, False, n)
    assert plan[-1] == 0 and len(plan) >= 3
    with index.attributes(level[None, :]) as attrs:
        few = dict(lo=[1.0], hi=[1.0])
        many = dict(lo=[3.0], hi=[3.0])
        assert attrs.count(few).tolist() == [12] and attrs.count(many).tolist() == [2000]
        cols = level[None, :]
        # 40 queries do not count: every window of the plan runs, then the scan
        vf.where_stats(reset=True)
        _check(index, attrs, xb, xq, cols, None, vf.where_arrays(few, 1, 40), k)
        searches, rounds, requeried, scanned, _ = vf.where_stats(reset=True)
        assert (searches, rounds, requeried, scanned) == (40, len(plan) - 1, 40, 40)
        # 8 queries count first: 12 of 5,000 rows is below the crossover, no window runs
        _check(index, attrs, xb, xq[:8], cols, None, vf.where_arrays(few, 1, 8), k)
        searches, rounds, requeried, scanned, streamed = vf.where_stats(reset=True)
        assert (searches, rounds, requeried, scanned) == (8, 0, 0, 8)
        # a predicate 40 % of the rows pass never reaches the scan
        for nq in (8, 40):
            _check(index, attrs, xb, xq[:nq], cols, None, vf.where_arrays(many, 1, nq), k)
            searches, rounds, requeried, scanned, streamed = vf.where_stats(reset=True)
            assert searches == nq and scanned == 0 and streamed == 0
            assert 1 <= rounds <= len(plan) - 1


# ---- 5. ties -------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [9, 40])
def test_ties_across_the_page_boundary(vf, metric, nq):
    """71 integer rows, each stored 70 times (and 29 more rows): every key is
    a 70-fold tie, and the predicate keeps every other copy, so 35 equal keys
    straddle the end of a 64-entry page and k itself."""
    rng = np.random.default_rng(10)
    base = rng.integers(-2, 3, size=(71, DIM)).astype(np.float32)
    xb = np.concatenate([np.repeat(base, 70, axis=0),
                         rng.integers(-2, 3, size=(29, DIM)).astype(np.float32)])
    assert xb.shape[0] == 4999
    xb = xb[rng.permutation(4999)]
    xq = rng.integers(-2, 3, size=(nq, DIM)).astype(np.float32)
    copy = np.zeros(4999, dtype=np.uint64)
    for row in np.unique(xb, axis=0):
        same = np.nonzero((xb == row).all(axis=1))[0]
        copy[same] = np.arange(same.size) % 2
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    with index.attributes(None, copy) as attrs:
        where = vf.where_arrays(dict(any_of=1), 0, nq)
        for k in (40, 70):
            for raw in (False, True):
                for scan in (False, True):
                    _check(index, attrs, xb, xq, None, copy, where, k, raw=raw, scan=scan,
                           exact=True)


# ---- 6. generations and tombstones ---------------------------------------------------
def test_generations_and_tombstones(vf):
    n = 3000
    xb, xq = _data(40, n, seed=11)
    xb, xq = flat.round_bf16(xb), flat.round_bf16(xq)
    cols, tags = _attr_data(n, seed=12)
    index = vf.IndexFlat(DIM, L2, dtype="bf16")
    index.add(xb)
    before = index.attributes(cols, tags)
    gone = np.random.default_rng(13).choice(n, 150, replace=False)
    assert index.remove_ids(gone) == 150  # a bf16 index keeps tombstones
    where = _bands(40, [0.3, 0.02, 1])
    with pytest.raises(RuntimeError, match="stale attributes"):
        index.search_where(xq, 5, before, where)
    with pytest.raises(RuntimeError, match="stale attributes"):
        before.count(where)
    keep = np.setdiff1d(np.arange(n), gone)
    xk, ck, tk = xb[keep], cols[:, keep], tags[keep]
    with pytest.raises(RuntimeError, match="n must equal the live row count"):
        index.attributes(cols, tags)
    with index.attributes(ck, tk) as attrs:
        np.testing.assert_array_equal(attrs.count(where), wo.pass_mask(ck, tk, *where).sum(axis=1))
        for scan in (False, True):
            _check(index, attrs, xk, xq, ck, tk, where, 10, scan=scan)
            _check(index, attrs, xk, xq[:3], ck, tk, tuple(a[:3] for a in where), 10, scan=scan)
        # an in-place update keeps the handle valid, and the new vectors are searched
        lab = np.array([5, 1700, 2849], dtype=np.int64)
        xk = xk.copy()
        xk[lab] = xq[:3]
        index.update(lab, xq[:3])
        ck = ck.copy()
        ck[0, lab] = 5.0
        with index.attributes(ck, tk) as attrs2:  # same generation: both handles serve
            w3 = vf.where_arrays(dict(lo=[4.5, None], hi=[5.5, None]), 2, 3)
            for scan in (False, True):
                _, I, _ = _check(index, attrs2, xk, xq[:3], ck, tk, w3, 10, scan=scan)
                assert I[:, 0].tolist() == lab.tolist()
                _check(index, attrs, xk, xq, cols[:, keep], tk, where, 10, scan=scan)
    # an fp32 index compacts at once: no tombstones, the same contract
    index = vf.IndexFlat(DIM, IP)
    index.add(xb)
    before = index.attributes(cols, tags)
    index.remove_ids(gone)
    with pytest.raises(RuntimeError, match="stale attributes"):
        index.search_where(xq, 5, before, where)
    with index.attributes(cols[:, keep], tk) as attrs:
        for scan in (False, True):
            _check(index, attrs, xb[keep], xq, cols[:, keep], tk, where, 10, scan=scan)


# ---- 7. exclusions -------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [5, 40])
def test_exclude_together_with_where(vf, normal_indexes, metric, nq):
    xb, cols, tags, idx = normal_indexes
    index, attrs = idx[metric]
    _, xq = _data(nq, 4999, seed=14)
    where = _bands(nq, [0.3, 0.05, 1])
    mask = wo.pass_mask(cols, tags, *where)
    _, I0 = wo.where_topk(flat.exact_scores(xb, xq, metric), mask, 100, metric, rule="lex")
    rng = np.random.default_rng(15)
    exclude = []
    for q in range(nq):
        m = (0, 1, 7, 100, 300)[q % 5]  # none, the best match alone, ..., lists past 64 entries
        best = I0[q][I0[q] >= 0][:max(m // 3, 1 if m else 0)]  # the best matches lead the list
        exclude.append(np.concatenate([best, rng.choice(4999, m - best.size, replace=False),
                                       [-1, 10**7]]).astype(np.int64) if m else [])
    for scan in (False, True):
        for raw in (False, True):
            D, I, _ = _check(index, attrs, xb, xq, cols, tags, where, 10, scan=scan, raw=raw,
                             exclude=exclude)
            for q in range(nq):
                if len(exclude[q]):
                    assert I0[q, 0] not in I[q]  # what would have been the best match


# ---- 8. attribute edge cases ---------------------------------------------------------
def test_attribute_edge_cases(vf, normal_indexes):
    xb, cols, tags, idx = normal_indexes
    index, attrs = idx[L2]
    _, xq = _data(9, 4999, seed=16)
    nan_rows = np.isnan(cols[1])
    assert nan_rows.sum() > 100
    preds = [
        dict(lo=[None, 100], hi=[None, 500]),      # a tested column: its NaN rows fail
        dict(lo=[2, None], hi=[4, None]),          # an untested one: they pass
        dict(lo=[None, -INF], hi=[None, 500]),     # one infinite bound still tests
        dict(lo=[None, 100], hi=[None, INF]),
        dict(lo=[-INF, -INF], hi=[INF, INF]),      # both infinite: no test, NaN rows pass
        dict(lo=[6, None], hi=[4, None]),          # lo > hi: nothing, a legal call
        dict(any_of=0b000110, all_of=0b101000, none_of=0b010000),
        dict(all_of=0b111111),
        dict(lo=[1, 60], hi=[9, 880], any_of=0b11, none_of=0b100000),
    ]
    where = vf.where_arrays(preds, 2, 9)
    for scan in (False, True):
        D, I, mask = _check(index, attrs, xb, xq, cols, tags, where, 10, scan=scan)
        assert not mask[0][nan_rows].any() and not mask[2][nan_rows].any()
        assert mask[1][nan_rows].any() and mask[4].all()
        assert not mask[5].any() and (I[5] == -1).all()
        assert 0 < mask[6].sum() < 700 and 0 < mask[7].sum() < 200
    np.testing.assert_array_equal(attrs.count(where), mask.sum(axis=1))
    # tags only (no columns), and no tags at all
    with index.attributes(None, tags) as only_tags:
        w = vf.where_arrays([dict(any_of=1), dict(none_of=63), None], 0, 3)
        for scan in (False, True):
            _check(index, only_tags, xb, xq[:3], None, tags, w, 10, scan=scan)
        np.testing.assert_array_equal(only_tags.count(w), wo.pass_mask(None, tags, *w).sum(axis=1))
    with index.attributes(cols[:1]) as no_tags:  # every row's tags are 0
        w = vf.where_arrays([dict(lo=[3], hi=[3.5]), dict(any_of=1), dict(none_of=1, all_of=0)],
                            1, 3)
        for scan in (False, True):
            _, I, mask = _check(index, no_tags, xb, xq[:3], cols[:1], None, w, 10, scan=scan)
            assert not mask[1].any() and mask[2].all()
    # a NaN bound is refused by the library itself (the wrapper refuses it earlier)
    from vsearch import _lib
    lib = _lib.load()
    lo = np.array([[0.0, np.nan]], dtype=np.float32)
    out = np.zeros(1, dtype=np.int64)
    assert lib.vs_attrs_count(attrs._h, lo.ctypes.data, None, None, 1, out.ctypes.data,
                              None) == _lib.E_INVALID
    assert _lib.last_error() == "vs_attrs_count: a NaN bound"
    buf = np.zeros(DIM * 10, dtype=np.float32)
    ibuf = np.zeros(10, dtype=np.int64)
    bad = np.array([1, 1], dtype=np.int64)
    assert lib.vs_search_where(index._h, attrs._h, buf.ctypes.data, 1, 10, None, lo.ctypes.data,
                               None, bad.ctypes.data, None, buf.ctypes.data, ibuf.ctypes.data, 0,
                               None) == _lib.E_INVALID
    assert _lib.last_error() == "vs_search_where: a NaN bound"  # before the offsets
    other = vf.IndexFlat(DIM, L2)
    other.add(xb[:10])
    with pytest.raises(ValueError, match="another index"):
        other.search_where(xq, 5, attrs, None)


# ---- 9. row skipping -----------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_row_skipping_counts_the_steps_it_loads(vf, normal_indexes, metric):
    xb, cols, tags, idx = normal_indexes
    index, attrs = idx[metric]
    _, xq = _data(1, 4999, seed=17)
    rng = np.random.default_rng(18)
    level = np.full(4999, 9.0, dtype=np.float32)
    level[rng.choice(1000, 60, replace=False)] = 2.0  # the passing rows: all in rows [0, 1000)
    with index.attributes(level[None, :]) as at:
        where = vf.where_arrays(dict(lo=[2.0], hi=[2.0]), 1, 1)
        vf.where_stats(reset=True)
        _check(index, at, xb, xq, level[None, :], None, where, 10, scan=True)
        *_, scanned, streamed = vf.where_stats(reset=True)
        steps = np.unique(np.nonzero(level == 2.0)[0] // 4).size
        assert scanned == 1 and streamed == 4 * steps and steps > 50
        # the predicate that tests nothing loads every step once
        _check(index, at, xb, xq, level[None, :], None, vf.where_arrays(None, 1, 1), 10, scan=True)
        assert vf.where_stats(reset=True)[4] == 4 * ((4999 + 3) // 4)


# ---- 10. the store -------------------------------------------------------------------
GENRES = ["fantasy", "adventure", "mystery", "science", "history", "poetry"]


@pytest.fixture(scope="module")
def store(vf):
    from vsearch import langchain as vlc
    from vsearch.synth import SynthEmbeddings

    n = 3000
    rng = np.random.default_rng(19)
    level = np.round(rng.uniform(1, 9, n), 1)
    metas = [{"book_id": f"B{i:04d}", "level": float(level[i]), "genre": GENRES[i % 6],
              "topics": [GENRES[(i // 6) % 6], "maps"] if i % 4 else ["maps"]} for i in range(n)]
    metas[7].pop("level")  # unknown: passes no test of the field
    texts = [f"book {i} about {m['genre']}" for i, m in enumerate(metas)]
    return vlc.FAISS.from_texts(texts, SynthEmbeddings(DIM), metadatas=metas), metas


def _passes(m, lo, hi, genres):
    return "level" in m and lo <= m["level"] <= hi and m["genre"] in genres


def test_store_where_returns_k_documents_that_all_pass(vf, store):
    st, metas = store
    k = 8
    where = {"level": {"$gte": 3.2, "$lte": 3.6}, "genre": {"$in": ["fantasy", "adventure"]}}
    matches = sum(_passes(m, 3.2, 3.6, ("fantasy", "adventure")) for m in metas)
    assert matches > 3 * k
    got = st.similarity_search("book 12 about fantasy", k=k, where=where)
    assert len(got) == k
    assert all(_passes(d.metadata, 3.2, 3.6, ("fantasy", "adventure")) for d in got)
    # the host filter over the default fetch_k returns fewer: the gap this closes
    def host(m):
        return _passes(m, 3.2, 3.6, ("fantasy", "adventure"))
    assert len(st.similarity_search("book 12 about fantasy", k=k, filter=host)) < k
    # and exact_filter agrees with where, document by document
    assert got == st.similarity_search("book 12 about fantasy", k=k, filter=host,
                                       exact_filter=True)
    assert len(st._attr_cache) == 3  # two field kinds and one handle
    st.similarity_search("book 99", k=k, where=where)
    assert len(st._attr_cache) == 3
    # fewer matches than k: exactly those
    rare = {"level": {"$gt": 7.5}, "genre": "poetry", "topics": {"$all": ["maps", "science"]}}
    want = [m for m in metas if "level" in m and np.float32(m["level"]) > np.float32(7.5)
            and m["genre"] == "poetry" and {"maps", "science"} <= set(m["topics"])]
    got = st.similarity_search_with_score("book 5", k=50, where=rare)
    assert 0 < len(want) < 50 and len(got) == len(want)
    assert sorted(d.metadata["book_id"] for d, _ in got) == sorted(m["book_id"] for m in want)
    # one predicate per query of a batch
    vecs = [st._embed_query(f"book {i}") for i in (3, 4, 5)]
    rows = st.similarity_search_batch_by_vector(
        vecs, k=k, where=[{"genre": g, "level": {"$lt": 5}} for g in GENRES[:3]])
    for g, row in zip(GENRES, rows):
        assert len(row) == k and all(d.metadata["genre"] == g and d.metadata["level"] < 5
                                     for d, _ in row)


def test_store_recommend_for_profiles_where(vf, store):
    st, metas = store
    k = 6
    profiles = [[(metas[(7 * s + j) % 3000]["book_id"], 1.0 - 0.2 * j) for j in range(4)]
                for s in range(12)]
    profiles[5] = [("nope", 1.0)]
    read = [[metas[(11 * s + j) % 3000]["book_id"] for j in range(5)] for s in range(12)]
    bands = [(1.0 + 0.5 * s, 3.0 + 0.5 * s) for s in range(12)]
    where = [{"level": {"$gte": a, "$lte": b}, "genre": {"$nin": ["poetry"]}} for a, b in bands]
    rows = st.recommend_for_profiles(profiles, k=k, exclude=read, where=where)
    assert rows[5] == []
    for s, row in enumerate(rows):
        if s == 5:
            continue
        assert len(row) == k
        barred = {b for b, _ in profiles[s]} | set(read[s])
        for d, _ in row:
            m = d.metadata
            assert bands[s][0] <= m["level"] <= bands[s][1] and m["genre"] != "poetry"
            assert m["book_id"] not in barred
    # a write drops the handle; the next search builds one over the new rows
    st.add_texts(["a new book"], metadatas=[{"book_id": "NEW", "level": 2.0, "genre": "poetry"}])
    assert st._attr_cache == {}
    got = st.similarity_search("a new book", k=3, where={"genre": "poetry", "level": 2.0})
    assert got[0].metadata["book_id"] == "NEW"
    st.delete([got[0].id])
    assert st._attr_cache == {}


# ---- 11. device pointers -------------------------------------------------------------
def test_device_outputs_and_a_capturing_stream(vf, normal_indexes):
    import torch

    from vsearch import _lib

    xb, cols, tags, idx = normal_indexes
    index, attrs = idx[IP]
    _, xq = _data(40, 4999, seed=20)
    where = _bands(40, [0.3, 0.01, 1, None])
    k = 10
    q = torch.from_numpy(xq).cuda()
    D = torch.empty((40, k), dtype=torch.float32, device="cuda")
    I = torch.empty((40, k), dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    for scan in (False, True):
        Dh, Ih = index.search_where(xq, k, attrs, where, scan=scan)
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            index.search_where_device(q.data_ptr(), 40, k, attrs, where, D.data_ptr(),
                                      I.data_ptr(), stream=st.cuda_stream, scan=scan)
        st.synchronize()
        np.testing.assert_array_equal(I.cpu().numpy(), Ih)
        np.testing.assert_array_equal(D.cpu().numpy().view(np.uint32), Dh.view(np.uint32))
    # a capturing stream is refused before anything is enqueued
    g = torch.cuda.CUDAGraph()
    buf = torch.zeros(8, device="cuda")
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        g.capture_begin(capture_error_mode="thread_local")
        try:
            buf.add_(1.0)
            with pytest.raises(_lib.VSearchError, match="capturing stream") as ei:
                index.search_where_device(q.data_ptr(), 40, k, attrs, where, D.data_ptr(),
                                          I.data_ptr(), stream=st.cuda_stream)
        finally:
            g.capture_end()
    assert ei.value.code == _lib.E_UNSUPPORTED
    del g
