"""GPU: boosted searches (vs_search_boost): exact top-k by similarity plus a
per-query boost of the row's attributes, through both routes (the windows with
their sufficiency test, and the boosted scan).

Oracle: ``boost_oracle`` — the numpy float32 restatement of b, then
``flat.select_topk(rule="lex")`` over fp64 ``score +- b`` — compared with
``boost_oracle.mismatches``; on small-integer rows with boosts that are
multiples of 1/32 every final key is exact in fp32, and I and D are compared
for equality.  d = 96; 3,000 or 4,999 rows, so the last tile is partial."""

import numpy as np
import pytest

import boost_oracle as bo
import where_oracle as wo
from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
DIM = 96
INF = np.inf
f32 = np.float32


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


def _half_levels(n, seed=1):
    """A level column of multiples of 0.5 in [0, 10) with a tenth unknown, and
    six tag bits."""
    rng = np.random.default_rng(seed)
    level = (rng.integers(0, 20, n) * 0.5).astype(np.float32)
    level[rng.random(n) < 0.1] = np.nan
    tags = rng.integers(0, 64, n).astype(np.uint64)
    return level[None, :], tags


def _oracle_b(vf, cols, tags, boost, nq):
    ncol = 0 if cols is None else cols.shape[0]
    arrays = vf.boost_arrays(boost, ncol, nq)
    b, bounds = bo.boost_values(cols, tags, *arrays, nrows=None if tags is None else tags.size)
    return b, bounds


# ---- 1. no boost is the raw search -----------------------------------------------------
@pytest.fixture(scope="module")
def int_indexes(vf):
    xb, _ = _int_data(1, 3000)
    cols, tags = _half_levels(3000)
    out = {}
    for metric in (L2, IP):
        index = vf.IndexFlat(DIM, metric)
        index.add(xb)
        out[metric] = (index, index.attributes(cols, tags))
    return xb, cols, tags, out


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 40, 129])
def test_no_boost_is_the_raw_search(vf, int_indexes, metric, nq):
    xb, cols, tags, idx = int_indexes
    index, attrs = idx[metric]
    _, xq = _int_data(nq, 3000, seed=3)
    D0, I0 = index.search(xq, 10, raw=True)
    for boost in (None, {"columns": [None]}, vf.boost_arrays(None, 1, nq)):
        D, I = index.search_boost(xq, 10, attrs, boost)  # the windows: bit for bit
        np.testing.assert_array_equal(I, I0)
        np.testing.assert_array_equal(D.view(np.uint32), D0.view(np.uint32))
    D, I = index.search_boost(xq, 10, attrs, None, scan=True)
    np.testing.assert_array_equal(I, I0)


# ---- 2. exact on exact data, both routes ------------------------------------------------
def _dyadic_specs(nq, w=0.25):
    """near with t a multiple of 0.5, s = 4, miss 0.125; one tag term of 0.125:
    every b is a multiple of 1/32."""
    return [{"columns": [("near", 0.5 * ((3 * q) % 20), 4.0, w, 0.125)],
             "tags": [(1 << (q % 6), 0.125)]} for q in range(nq)]


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 9, 40, 129])
def test_exact_on_exact_data_both_routes(vf, int_indexes, metric, nq):
    xb, cols, tags, idx = int_indexes
    index, attrs = idx[metric]
    _, xq = _int_data(nq, 3000, seed=3)
    scores = flat.exact_scores(xb, xq, metric)
    key = np.sort(scores if metric == L2 else -scores, axis=1)
    # the precondition of the counts below, a property of the fixture: the raw
    # rank-10 key is well below the rank-26 and rank-104 keys for every query
    assert (key[:, 25] - key[:, 9]).min() >= (7 if metric == L2 else 3)
    assert (key[:, 103] - key[:, 9]).min() >= (28 if metric == L2 else 13)
    specs = _dyadic_specs(nq)
    b, bounds = _oracle_b(vf, cols, tags, specs, nq)
    assert np.array_equal(b * 32, np.round(b * 32)) and (bounds == [0.0, 0.375]).all()
    for k in (10, 70):
        Dr, Ir = bo.boost_topk(scores, b, None, k, metric)
        for scan in (False, True):
            vf.boost_stats(reset=True)
            D, I = index.search_boost(xq, k, attrs, specs, scan=scan)
            np.testing.assert_array_equal(I, Ir)
            np.testing.assert_array_equal(D, Dr)
            searches, rounds, requeried, scanned = vf.boost_stats(reset=True)
            assert searches == nq
            if scan:
                assert (rounds, scanned) == (0, nq)
            elif k == 10:  # U = 0.375 is below every gap: the first window settles all
                assert (rounds, requeried, scanned) == (1, 0, 0)


@pytest.mark.parametrize("nq", [1, 9, 40, 129])
def test_a_strong_boost_settles_in_the_second_window(vf, int_indexes, nq):
    xb, cols, tags, idx = int_indexes
    index, attrs = idx[IP]
    _, xq = _int_data(nq, 3000, seed=3)
    scores = flat.exact_scores(xb, xq, IP)
    key = np.sort(-scores, axis=1)
    assert (key[:, 103] - key[:, 9]).min() >= 13  # above U = 8.125
    specs = _dyadic_specs(nq, w=8.0)
    b, bounds = _oracle_b(vf, cols, tags, specs, nq)
    assert (bounds == [0.0, 8.125]).all()
    Dr, Ir = bo.boost_topk(scores, b, None, 10, IP)
    vf.boost_stats(reset=True)
    D, I = index.search_boost(xq, 10, attrs, specs)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)
    searches, rounds, requeried, scanned = vf.boost_stats(reset=True)
    assert requeried > 0 and scanned == 0 and rounds == 2


# ---- 3. the row that no over-fetch finds ------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_the_row_no_over_fetch_finds(vf, metric):
    n, nq = 3000, 9
    xb, xq = _data(nq, n, seed=7)
    # row 0 is far from every query: its raw rank is beyond any window
    xb[0] = -0.5 * xq.sum(axis=0)
    scores = flat.exact_scores(xb, xq, metric)
    key = scores if metric == L2 else -scores
    assert ((key < key[:, :1]).sum(axis=1) > 1023).all()
    tags = np.zeros(n, dtype=np.uint64)
    tags[0] = 1 << 17
    tags[1::2] |= np.uint64(1)
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    spec = {"tags": [(1 << 17, 1000.0), (1, 0.01)]}
    b, _ = _oracle_b(vf, None, tags, spec, nq)
    with index.attributes(None, tags) as attrs:
        Dr, Ir = bo.boost_topk(scores, b, None, 10, metric)
        assert (Ir[:, 0] == 0).all()
        vf.boost_stats(reset=True)
        D, I = index.search_boost(xq, 10, attrs, spec)
        assert (I[:, 0] == 0).all()
        assert not bo.mismatches(D, I, Dr, Ir, metric, xb, xq, b)
        assert vf.boost_stats(reset=True)[3] == nq  # every query went to the scan
        Dr, Ir = bo.boost_topk(scores, b, None, 10, metric, exclude=[[0]] * nq)
        D, I = index.search_boost(xq, 10, attrs, spec, exclude=[[0]] * nq)
        assert not (I == 0).any()
        assert not bo.mismatches(D, I, Dr, Ir, metric, xb, xq, b)


# ---- 4. the boost's bits on the device --------------------------------------------------
@pytest.mark.parametrize("nq", [1, 5, 40])
def test_the_bits_of_b_on_the_device(vf, nq):
    """Zero queries under inner product: every score is 0, so D is b itself."""
    n, k = 300, 64
    rng = np.random.default_rng(23)
    cols = rng.uniform(-2.0, 12.0, size=(4, n)).astype(np.float32)
    cols[rng.random((4, n)) < 0.1] = np.nan
    cols[0, 0] = np.nan
    tags = rng.integers(0, 64, n).astype(np.uint64)
    index = vf.IndexFlat(DIM, IP)
    index.add(rng.standard_normal((n, DIM)).astype(np.float32))
    kinds = np.array([[1, 2, 1, 2], [2, 1, 0, 1], [0, 2, 2, 1]], dtype=np.int32)
    specs = []
    for q in range(nq):
        r = np.random.default_rng(100 + q)
        terms = []
        for c in range(4):
            kd = kinds[q % 3, c]
            terms.append(None if kd == 0 else (
                "near" if kd == 1 else "ramp", float(r.uniform(0, 9)) + 0.1,
                float(r.uniform(0.3, 7.0)), float(r.uniform(-0.7, 0.9)), float(r.uniform(-1, 1))))
        specs.append({"columns": terms,
                      "tags": [(int(r.integers(1, 64)), float(r.uniform(-0.2, 0.3)))
                               for _ in range(1 + q % 4)]})
    b, bounds = _oracle_b(vf, cols, tags, specs, nq)
    assert any(t is not None and t[3] < 0 for sp in specs for t in sp["columns"]) or nq == 1
    xq = np.zeros((nq, DIM), dtype=np.float32)
    with index.attributes(cols, tags) as attrs:
        D, I = index.search_boost(xq, k, attrs, specs, scan=True)
    for q in range(nq):
        order = np.lexsort((np.arange(n), -b[q].astype(np.float64)))[:k]
        np.testing.assert_array_equal(I[q], order)
        np.testing.assert_array_equal(D[q].view(np.uint32), b[q][order].view(np.uint32))


# ---- 5. random data ---------------------------------------------------------------------
def _attr_data(n, seed=1):
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


def _weighted_specs(nq):
    """Weights from 0.001 to 2 across the queries."""
    ws = np.geomspace(0.001, 2.0, max(nq, 2))
    return [{"columns": [("near", 1.3 + 0.17 * q, 5.0, float(ws[q]), float(ws[q]) / 2),
                         ("ramp", 100.0, 650.0, float(ws[q]) / 3, 0.0) if q % 2 else None],
             "tags": [(1 << (q % 6), float(ws[q]) / 8)]} for q in range(nq)]


@pytest.fixture(scope="module")
def normal_indexes(vf):
    xb, _ = _data(1, 4999, seed=5)
    cols, tags = _attr_data(4999, seed=6)
    out = {}
    for dtype in ("f32", "bf16"):
        for metric in (L2, IP):
            index = vf.IndexFlat(DIM, metric, dtype=dtype)
            index.add(xb)
            out[dtype, metric] = (index, index.attributes(cols, tags))
    return xb, cols, tags, out


def _check(vf, index, attrs, xb, xq, cols, tags, specs, k, *, where=None, exclude=None,
           scan=False):
    metric = index.metric_type
    nq, n = xq.shape[0], xb.shape[0]
    b, bounds = _oracle_b(vf, cols, tags, specs, nq)
    mask = np.ones((nq, n), dtype=bool) if where is None else \
        wo.pass_mask(cols, tags, *where, n=n)
    scores = flat.exact_scores(xb, xq, metric)
    Dr, Ir = bo.boost_topk(scores, b, mask, k, metric, exclude=exclude)
    D, I = index.search_boost(xq, k, attrs, specs, where=where, exclude=exclude, scan=scan)
    allowed = mask & ~wo.excluded_mask(exclude, nq, n)
    for q in range(nq):
        got = I[q][I[q] >= 0]
        assert allowed[q][got].all(), ("a row that is not allowed came back", q)
        assert got.size == min(k, int(allowed[q].sum())), (q, got.size, int(allowed[q].sum()))
    bad = bo.mismatches(D, I, Dr, Ir, metric, xb, xq, b)
    assert not bad, bad[:5]
    return D, I


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [3, 40])
def test_random_data_with_predicates_and_exclusions(vf, normal_indexes, dtype, metric, nq):
    xb, cols, tags, idx = normal_indexes
    index, attrs = idx[dtype, metric]
    _, xq = _data(nq, 4999, seed=8)
    if dtype == "bf16":
        xb, xq = flat.round_bf16(xb), flat.round_bf16(xq)
    specs = _weighted_specs(nq)
    where = _bands(nq, [1, 0.3, 0.03, None])
    rng = np.random.default_rng(9)
    D0, I0 = index.search(xq, 12, raw=True)
    exclude = [[int(v) for v in I0[q, :6]] + [int(v) for v in rng.integers(0, 4999, 5)] if q % 3 else []
               for q in range(nq)]
    routes = set()
    for k in (10, 70):
        for scan in (False, True):
            vf.boost_stats(reset=True)
            _check(vf, index, attrs, xb, xq, cols, tags, specs, k, scan=scan)
            s = vf.boost_stats(reset=True)
            routes.add(("scan" if s[3] else "") + ("windows" if s[1] else ""))
            _check(vf, index, attrs, xb, xq, cols, tags, specs, k, where=where, exclude=exclude,
                   scan=scan)
    assert "scan" in routes and routes & {"windows", "scanwindows"}


# ---- 5b. no boost under predicates is the raw where search ------------------------------
@pytest.fixture(scope="module")
def pinned_indexes(vf):
    xb, _ = _int_data(1, 4999, seed=13)
    cols, tags = _attr_data(4999, seed=6)
    out = {}
    for dtype in ("f32", "bf16"):  # the rows are small integers: exact in bf16 too
        for metric in (L2, IP):
            index = vf.IndexFlat(DIM, metric, dtype=dtype)
            index.add(xb)
            out[dtype, metric] = (index, index.attributes(cols, tags))
    return cols, tags, out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 8, 9, 33, 129])
def test_no_boost_under_predicates_is_the_raw_where_search(vf, pinned_indexes, dtype, metric, nq):
    """The two kinds of the shared route driver and scan kernels, pinned to each
    other: with boost None b = +0, so fl32(key - b) is the key's own bits, and a
    boosted search with per-query predicates and exclusions returns what
    search_where(raw=True) returns: I equal, D bit for bit.  Once through the
    scan (the streaming kernel at nq = 1, 8, 9, the MFMA kernel at 33, 129; k =
    70 takes two pages and the floor) and once by the default routes."""
    cols, tags, idx = pinned_indexes
    index, attrs = idx[dtype, metric]
    _, xq = _int_data(nq, 4999, seed=14)
    # bands of mixed selectivity; 0.001 is about five rows, None passes nothing
    where = _bands(nq, [0.3, None, 0.001, 1, 0.03], seed=15)
    if nq >= 8:  # a property of the fixture: a query passes nothing, one fewer than 10 rows
        counts = wo.pass_mask(cols, tags, *where, n=4999).sum(axis=1)
        assert (counts == 0).any() and ((counts > 0) & (counts < 10)).any(), counts[:8]
    _, I0 = index.search(xq, 8, raw=True)
    exclude = [[int(v) for v in I0[q, :3 + q % 3]] for q in range(nq)]
    for k in (10, 70):
        for scan in (True, False):
            Dw, Iw = index.search_where(xq, k, attrs, where, exclude=exclude, raw=True, scan=scan)
            Db, Ib = index.search_boost(xq, k, attrs, None, where=where, exclude=exclude,
                                        scan=scan)
            np.testing.assert_array_equal(Ib, Iw)
            np.testing.assert_array_equal(Db.view(np.uint32), Dw.view(np.uint32))


# ---- 6. tombstones and staleness --------------------------------------------------------
def test_tombstones_and_staleness(vf):
    n, nq = 3000, 40
    xb, xq = _data(nq, n, seed=11)
    xb, xq = flat.round_bf16(xb), flat.round_bf16(xq)
    cols, tags = _attr_data(n, seed=12)
    specs = _weighted_specs(nq)
    index = vf.IndexFlat(DIM, L2, dtype="bf16")
    index.add(xb)
    before = index.attributes(cols, tags)
    _check(vf, index, before, xb, xq, cols, tags, specs, 10)
    gone = np.random.default_rng(13).choice(n, 150, replace=False)
    assert index.remove_ids(gone) == 150  # a bf16 index keeps tombstones
    with pytest.raises(RuntimeError, match="stale attributes"):
        index.search_boost(xq, 5, before, specs)
    keep = np.setdiff1d(np.arange(n), gone)
    xk, ck, tk = xb[keep], cols[:, keep], tags[keep]
    with index.attributes(ck, tk) as attrs:
        for scan in (False, True):  # labels are positions among the live rows
            _check(vf, index, attrs, xk, xq, ck, tk, specs, 10, scan=scan)
            _check(vf, index, attrs, xk, xq[:3], ck, tk, specs[:3], 70, scan=scan)
        # an in-place update keeps the handle valid, and the new vectors are searched
        lab = np.array([5, 1700, 2849], dtype=np.int64)
        xk = xk.copy()
        xk[lab] = xq[:3]
        index.update(lab, xq[:3])
        for scan in (False, True):
            _, I = _check(vf, index, attrs, xk, xq, ck, tk, None, 10, scan=scan)
            assert I[:3, 0].tolist() == lab.tolist()
            _check(vf, index, attrs, xk, xq, ck, tk, specs, 10, scan=scan)
    other = vf.IndexFlat(DIM, L2)
    other.add(xb[:10])
    with pytest.raises(ValueError, match="another index"):
        other.search_boost(xq, 5, before, specs)


# ---- 7. the store -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def catalog(golden):
    """The golden CSV catalogue with its level as a number and its genres as a list."""
    from vsearch import langchain as vlc
    from vsearch.synth import SynthEmbeddings

    inputs, _ = golden
    metas = []
    for i, m in enumerate(inputs["book_metadata"]):
        m = dict(m)
        try:
            m["level"] = float(m["level"])
        except (KeyError, TypeError, ValueError):
            m.pop("level", None)
        if i % 11 == 3:
            m.pop("level", None)  # unknown reading level: the "missing" term
        m["genre"] = [g.strip() for g in str(m.get("genre", "")).split(",") if g.strip()]
        metas.append(m)
    st = vlc.FAISS.from_texts(inputs["book_texts"], SynthEmbeddings(), metadatas=metas)
    return st, metas, inputs["keywords"]


def _store_boost(level):
    return {"level": {"$near": level, "scale": 5, "weight": 0.4, "missing": 0.2},
            "genre": {"$in": ["fantasy", "adventure"], "weight": 0.05}}


def _store_b(metas, level):
    col = np.array([[m.get("level", np.nan) for m in metas]], dtype=np.float32)
    tags = np.array([1 if {"fantasy", "adventure"} & set(m["genre"]) else 0 for m in metas],
                    dtype=np.uint64)
    kinds = np.array([[1]], dtype=np.int32)
    params = np.array([[[level, 5, 0.4, 0.2]]], dtype=np.float32)
    b, _ = bo.boost_values(col, tags, kinds, params, np.array([[1, 0, 0, 0]], dtype=np.uint64),
                           np.array([[0.05, 0, 0, 0]], dtype=np.float32))
    return b[0]


def test_store_boost_ranks_every_document(vf, catalog):
    st, metas, keywords = catalog
    n, k = len(metas), 5
    pos = {m["book_id"]: i for i, m in enumerate(metas)}
    assert st.index.metric_type == L2
    found = None
    for kw in keywords:
        plain = st.similarity_search_with_score(kw, k=n)  # the store's own scores
        dist = np.empty(n, dtype=np.float32)
        for d, s in plain:
            dist[pos[d.metadata["book_id"]]] = s
        assert len(plain) == n
        for level in (1.5, 3.0, 4.2, 6.0, 8.5):
            final = (dist - _store_b(metas, level)).astype(np.float32)
            exact = np.lexsort((np.arange(n), final))[:k]
            near = np.array([pos[d.metadata["book_id"]] for d, _ in plain[:2 * k]])
            rerank = near[np.lexsort((near, final[near]))][:k]
            if found is None and exact.tolist() != rerank.tolist():
                found = (kw, level, exact, final, rerank)
    # the point of the feature: a re-rank of the k * 2 nearest misses a book
    assert found is not None
    kw, level, exact, final, rerank = found
    got = st.similarity_search_with_score(kw, k=k, boost=_store_boost(level))
    ids = [pos[d.metadata["book_id"]] for d, _ in got]
    assert ids == exact.tolist() and ids != rerank.tolist()
    np.testing.assert_allclose([s for _, s in got], final[exact], rtol=1e-5, atol=1e-5)
    assert [d.metadata["book_id"] for d in st.similarity_search(kw, k=k, boost=_store_boost(level))] \
        == [metas[i]["book_id"] for i in ids]
    # every (keyword, level) agrees with the host ranking of all documents
    for kw in keywords[:6]:
        plain = st.similarity_search_with_score(kw, k=n)
        dist = np.empty(n, dtype=np.float32)
        for d, s in plain:
            dist[pos[d.metadata["book_id"]]] = s
        final = (dist - _store_b(metas, 4.2)).astype(np.float32)
        got = st.similarity_search_with_score(kw, k=k, boost=_store_boost(4.2))
        assert [pos[d.metadata["book_id"]] for d, _ in got] == \
            np.lexsort((np.arange(n), final))[:k].tolist()


def test_store_profiles_and_errors(vf, catalog):
    st, metas, keywords = catalog
    k = 6
    n = len(metas)
    profiles = [[(metas[(7 * s + j) % n]["book_id"], 1.0 - 0.2 * j) for j in range(4)]
                for s in range(8)]
    profiles[5] = [("nope", 1.0)]
    read = [[metas[(11 * s + j) % n]["book_id"] for j in range(5)] for s in range(8)]
    boosts = [_store_boost(2.0 + 0.7 * s) for s in range(8)]
    where = [{"level": {"$gte": 1.0 + 0.5 * s, "$lte": 4.0 + 0.5 * s}} for s in range(8)]
    where[2] = {"level": {"$gte": 3.0, "$lte": 3.2}, "genre": {"$in": ["poetry"]}}  # few pass
    rows = st.recommend_for_profiles(profiles, k=k, exclude=read, boost=boosts, where=where)
    assert rows[5] == []
    for s, row in enumerate(rows):
        if s == 5:
            continue
        barred = {b for b, _ in profiles[s]} | set(read[s])
        lo, hi = where[s]["level"]["$gte"], where[s]["level"]["$lte"]
        allowed = [m for m in metas if "level" in m and f32(lo) <= f32(m["level"]) <= f32(hi)
                   and m["book_id"] not in barred and (s != 2 or "poetry" in m["genre"])]
        assert len(row) == min(k, len(allowed))
        ok = {m["book_id"] for m in allowed}
        assert all(d.metadata["book_id"] in ok for d, _ in row)
        one = st.recommend_for_profiles([profiles[s]], k=k, exclude=[read[s]], boost=boosts[s],
                                        where=where[s])[0]
        assert [d.metadata["book_id"] for d, _ in one] == [d.metadata["book_id"] for d, _ in row]
    assert len(rows[2]) < k
    vec = st._embed_query(keywords[0])
    batch = st.similarity_search_batch_by_vector([vec, vec], k=k, boost=[boosts[0], None])
    assert [d.metadata["book_id"] for d, _ in batch[1]] == \
        [d.metadata["book_id"] for d in st.similarity_search_by_vector(vec, k=k)]
    assert [d.metadata["book_id"] for d, _ in batch[0]] == \
        [d.metadata["book_id"] for d in st.similarity_search_by_vector(vec, k=k, boost=boosts[0])]
    b = boosts[0]
    for call in (lambda: st.similarity_search("x", k=k, boost=b, distinct="book_id"),
                 lambda: st.similarity_search("x", k=k, boost=b, filter={"book_id": "B001"}),
                 lambda: st.max_marginal_relevance_search("x", k=k, boost=b),
                 lambda: st.recommend_for_profiles(profiles, k=k, boost=b, mmr=(20, 0.5)),
                 lambda: st.recommend_for_profiles(profiles, k=k, boost=b, distinct="book_id"),
                 lambda: st.similarity_search_batch_by_vector([vec], k=k, boost=b,
                                                              distinct="book_id"),
                 lambda: st.similarity_search("x", k=k, boost={"level": {"$exp": 1, "weight": 1}}),
                 lambda: st.similarity_search("x", k=k, boost={
                     f"g{i}": {"$eq": 1, "weight": 0.1} for i in range(5)})):
        with pytest.raises(ValueError):
            call()


# ---- 8. device pointers -----------------------------------------------------------------
def test_device_outputs_and_a_capturing_stream(vf, normal_indexes):
    import torch

    from vsearch import _lib

    xb, cols, tags, idx = normal_indexes
    index, attrs = idx["f32", IP]
    _, xq = _data(40, 4999, seed=20)
    specs = _weighted_specs(40)
    k = 10
    q = torch.from_numpy(xq).cuda()
    D = torch.empty((40, k), dtype=torch.float32, device="cuda")
    I = torch.empty((40, k), dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    for scan in (False, True):
        Dh, Ih = index.search_boost(xq, k, attrs, specs, scan=scan)
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            index.search_boost_device(q.data_ptr(), 40, k, attrs, specs, D.data_ptr(),
                                      I.data_ptr(), stream=st.cuda_stream, scan=scan)
        st.synchronize()
        np.testing.assert_array_equal(I.cpu().numpy(), Ih)
        np.testing.assert_array_equal(D.cpu().numpy().view(np.uint32), Dh.view(np.uint32))
    g = torch.cuda.CUDAGraph()
    buf = torch.zeros(8, device="cuda")
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        g.capture_begin(capture_error_mode="thread_local")
        try:
            buf.add_(1.0)
            with pytest.raises(_lib.VSearchError, match="capturing stream") as ei:
                index.search_boost_device(q.data_ptr(), 40, k, attrs, specs, D.data_ptr(),
                                          I.data_ptr(), stream=st.cuda_stream)
        finally:
            g.capture_end()
    assert ei.value.code == _lib.E_UNSUPPORTED
