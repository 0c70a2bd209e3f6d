"""GPU: bonus searches (vs_search_bonus): exact top-k under per-query, per-row
score bonuses, with and without an attribute handle (the boosted search's base
through both of its routes, and the raw plain search).

Oracle: ``bonus_oracle`` — final keys in float32 numpy on top of
``boost_oracle.boost_values``, ranked by (final key, label) — compared for
equality on small-integer rows with boosts that are multiples of 1/32 and
bonuses that are multiples of 1/4 (every final key is exact in fp32), and with
``bonus_oracle.mismatches`` on random rows.  d = 96; 3,000 rows, so the last
tile is partial."""

import numpy as np
import pytest

import bonus_oracle as bno
import boost_oracle as bo
import where_oracle as wo
from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
DIM = 96
N = 3000
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


def _half_levels(n, seed=1):
    """A level column of multiples of 0.5 in [0, 10) with a tenth unknown, and
    six tag bits."""
    rng = np.random.default_rng(seed)
    level = (rng.integers(0, 20, n) * 0.5).astype(np.float32)
    level[rng.random(n) < 0.1] = np.nan
    tags = rng.integers(0, 64, n).astype(np.uint64)
    return level[None, :], tags


def _dyadic_specs(nq, w=0.25):
    """near with t a multiple of 0.5, s = 4, miss 0.125; one tag term of 0.125:
    every b is a multiple of 1/32."""
    return [{"columns": [("near", 0.5 * ((3 * q) % 20), 4.0, w, 0.125)],
             "tags": [(1 << (q % 6), 0.125)]} for q in range(nq)]


def _oracle_b(vf, cols, tags, boost, nq):
    ncol = 0 if cols is None else cols.shape[0]
    arrays = vf.boost_arrays(boost, ncol, nq)
    b, _ = bo.boost_values(cols, tags, *arrays, nrows=None if tags is None else tags.size)
    return b


def _quarter_lists(nq, n, seed, lengths=(0, 1, 17, 64, 300, 1024), signed=True):
    """Per query a list over random labels whose length is drawn from
    `lengths`, values multiples of 1/4 in [-8, 8] ([0, 8] when not signed)."""
    rng = np.random.default_rng(seed)
    lists = []
    for q in range(nq):
        m = int(lengths[(q + int(rng.integers(0, len(lengths)))) % len(lengths)])
        labels = rng.choice(n, m, replace=False).astype(np.int64)
        vals = (rng.integers(-32 if signed else 0, 33, m) * 0.25).astype(np.float32)
        lists.append((labels, vals))
    return lists


@pytest.fixture(scope="module")
def int_indexes(vf):
    xb, _ = _int_data(1, N)
    cols, tags = _half_levels(N)
    out = {}
    for metric in (L2, IP):
        index = vf.IndexFlat(DIM, metric)
        index.add(xb)
        out[metric] = (index, index.attributes(cols, tags))
    return xb, cols, tags, out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. no lists is the base search -----------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 40, 129])
def test_no_lists_is_the_base_search(vf, int_indexes, metric, nq):
    xb, cols, tags, idx = int_indexes
    index, attrs = idx[metric]
    _, xq = _data(nq, 8, seed=3)  # real-valued queries: the bits are the engines' own
    specs = _dyadic_specs(nq)
    Db, Ib = index.search_boost(xq, 10, attrs, specs)
    D0, I0 = index.search(xq, 10, raw=True)
    unknown = [{-1: 1.0, 10 ** 9: -2.0, N: 3.0}] * nq  # no live label: no list either
    for bonus in (None, [None] * nq, [{}] * nq, unknown):
        D, I = index.search_bonus(xq, 10, bonus, attrs=attrs, boost=specs)
        np.testing.assert_array_equal(I, Ib)
        np.testing.assert_array_equal(_bits(D), _bits(Db))
        D, I = index.search_bonus(xq, 10, bonus)
        np.testing.assert_array_equal(I, I0)
        np.testing.assert_array_equal(_bits(D), _bits(D0))


# ---- 2. exact on exact data -------------------------------------------------------------
def _exact_case(vf, xb, xq, cols, tags, specs, lists, metric):
    nq = xq.shape[0]
    scores = flat.exact_scores(xb, xq, metric)
    b = _oracle_b(vf, cols, tags, specs, nq) if specs is not None else \
        np.zeros(scores.shape, dtype=np.float32)
    s, listed = bno.dense_lists(lists, nq, xb.shape[0])
    # every final key is exactly representable: |key| <= 1,536, and b and s
    # are multiples of 1/32, so no subtraction rounds
    fin = bno.final_keys(scores, b, s, listed, metric)
    assert np.abs(scores).max() <= 1536
    assert np.array_equal(b * 32, np.round(b * 32)) and np.array_equal(s * 4, np.round(s * 4))
    key64 = scores if metric == L2 else -scores
    assert np.array_equal(fin.astype(np.float64), key64 - b.astype(np.float64) - s)
    return scores, b, s, listed


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 9, 40, 129])
def test_exact_on_exact_data(vf, int_indexes, metric, nq):
    xb, cols, tags, idx = int_indexes
    index, attrs = idx[metric]
    _, xq = _int_data(nq, N, seed=3)
    specs = _dyadic_specs(nq)
    lists = _quarter_lists(nq, N, seed=100 + nq)
    scores, b, s, listed = _exact_case(vf, xb, xq, cols, tags, specs, lists, metric)
    total = sum(l.size for l, _ in lists)
    negative = sum(1 for _, v in lists if (v < 0).any())
    for k in (10, 70, 1500):
        Dr, Ir = bno.bonus_topk(scores, b, s, listed, None, k, metric)
        for scan in (False, True):
            vf.bonus_stats(reset=True)
            D, I = index.search_bonus(xq, k, lists, attrs=attrs, boost=specs, scan=scan)
            np.testing.assert_array_equal(I, Ir)
            np.testing.assert_array_equal(D, Dr)
            searches, nlisted, demoted, entered = vf.bonus_stats(reset=True)
            assert (searches, nlisted, demoted) == (nq, total, negative)
            assert entered == int(np.take_along_axis(listed, np.maximum(Ir, 0), axis=1)
                                  [Ir >= 0].sum())
        # without a handle: the raw search is the base
        Dr, Ir = bno.bonus_topk(scores, None, s, listed, None, k, metric)
        D, I = index.search_bonus(xq, k, lists)
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_array_equal(D, Dr)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [9, 129])
def test_promotions_alone_demote_nobody(vf, int_indexes, metric, nq):
    xb, cols, tags, idx = int_indexes
    index, attrs = idx[metric]
    _, xq = _int_data(nq, N, seed=4)
    specs = _dyadic_specs(nq)
    lists = _quarter_lists(nq, N, seed=200 + nq, signed=False)
    lists[0] = (lists[0][0], -0.0 * lists[0][1])  # -0 counts as not negative
    scores, b, s, listed = _exact_case(vf, xb, xq, cols, tags, specs, lists, metric)
    for k, with_attrs in ((10, True), (70, False)):
        Dr, Ir = bno.bonus_topk(scores, b if with_attrs else None, s, listed, None, k, metric)
        vf.bonus_stats(reset=True)
        D, I = index.search_bonus(xq, k, lists, attrs=attrs, boost=specs) if with_attrs else \
            index.search_bonus(xq, k, lists)
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_array_equal(D, Dr)
        searches, nlisted, demoted, _ = vf.bonus_stats(reset=True)
        assert (searches, nlisted, demoted) == (nq, sum(l.size for l, _ in lists), 0)


# ---- 3. the row that no over-fetch finds ------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", [L2, IP])
def test_the_row_no_over_fetch_finds(vf, metric, dtype):
    nq, k = 9, 10
    xb, xq = _data(nq, N, seed=10)
    if dtype == "bf16":
        xb, xq = flat.round_bf16(xb), flat.round_bf16(xq)
    scores = flat.exact_scores(xb, xq, metric)
    key = scores if metric == L2 else -scores
    order = np.argsort(key, axis=1, kind="stable")
    # a property of the fixture: the gaps between the first raw keys are above
    # twice the engines' tolerance, so the raw order has one answer
    skey = np.take_along_axis(key, order, axis=1)
    tol = flat.score_tolerance(metric, skey[:, :k + 2], (xq.astype(np.float64) ** 2).sum(1).max(),
                               (xb.astype(np.float64) ** 2).sum(1).max())
    assert np.diff(skey[:, :k + 2], axis=1).min() > 2 * np.max(tol)
    index = vf.IndexFlat(DIM, metric, dtype=dtype)
    index.add(xb)
    lists = []
    for q in range(nq):
        last, first = int(order[q, -1]), int(order[q, 0])
        up = float(skey[q, -1] - skey[q, 0]) + 5.0      # the farthest row: to the front
        down = -(float(skey[q, k + 1] - skey[q, 0]) + 5.0)  # the nearest row: past rank k
        lists.append({last: up, first: down})
    D, I = index.search_bonus(xq, k, lists)
    assert I[:, 0].tolist() == order[:, -1].tolist()
    for q in range(nq):
        assert int(order[q, 0]) not in I[q].tolist()
    np.testing.assert_array_equal(I[:, 1:], order[:, 1:k])  # the raw order, shifted
    s, listed = bno.dense_lists(lists, nq, N)
    Dr, Ir = bno.bonus_topk(scores, None, s, listed, None, k, metric)
    zero = np.zeros(scores.shape, dtype=np.float32)
    assert not bno.mismatches(D, I, Dr, Ir, metric, xb, xq, zero, s, listed)
    # a search of k * 2 rows never sees the promoted row
    _, I2 = index.search(xq, 2 * k, raw=True)
    assert not (I2 == order[:, -1:]).any()


# ---- 4. ties by label, across the two sets ----------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_ties_by_label_across_the_two_sets(vf, metric):
    xb, xq = _int_data(1, N, seed=31)
    scores = flat.exact_scores(xb, xq, metric)
    key = (scores if metric == L2 else -scores)[0]
    order = np.lexsort((np.arange(N), key))
    r0, r3 = int(order[0]), int(order[3])
    copies = [1, 5, 2500]  # three more copies of the nearest row
    assert 5 < r3 < 2500 and r0 not in copies and key[order[3]] > key[order[2]] > key[r0]
    xb[copies] = xb[r0]
    scores = flat.exact_scores(xb, np.repeat(xq, 2, axis=0), metric)
    key = (scores if metric == L2 else -scores)[0]
    gap = float(key[r0] - key[r3])  # negative: the copy is demoted onto row r3's key
    # query 0: copy 5 listed with +0 (it still ties r0 and copy 1), copy 2500
    # tied with r3 from above r3's label; query 1: copy 1 tied with r3 from below
    lists = [{5: 0.0, 2500: gap}, {5: 0.0, 1: gap}]
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    s, listed = bno.dense_lists(lists, 2, N)
    k = 8
    Dr, Ir = bno.bonus_topk(scores, None, s, listed, None, k, metric)
    top = sorted([r0, 1, 5])
    assert Ir[0, :3].tolist() == top and Ir[1, :3].tolist() == sorted([r0, 5, 2500])
    pos0, pos1 = Ir[0].tolist(), Ir[1].tolist()
    assert pos0.index(r3) + 1 == pos0.index(2500) and pos1.index(1) + 1 == pos1.index(r3)
    assert Dr[0, pos0.index(r3)] == Dr[0, pos0.index(2500)]
    D, I = index.search_bonus(np.repeat(xq, 2, axis=0), k, lists)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)


# ---- 5. composition ---------------------------------------------------------------------
def _attr_data(n, seed=1):
    rng = np.random.default_rng(seed)
    level = rng.uniform(0, 10, n).astype(np.float32)
    pages = rng.integers(50, 900, n).astype(np.float32)
    pages[rng.random(n) < 0.1] = np.nan
    tags = rng.integers(0, 64, n).astype(np.uint64)
    return np.stack([level, pages]), tags


def _third_bands(nq, seed=2):
    """One band of the level column per query that about a third of the rows pass."""
    rng = np.random.default_rng(seed)
    lo = np.full((nq, 2), -INF, dtype=np.float32)
    hi = np.full((nq, 2), INF, dtype=np.float32)
    c = rng.uniform(2.0, 8.0, nq)
    lo[:, 0], hi[:, 0] = c - 5.0 / 3, c + 5.0 / 3
    return lo, hi, np.zeros((nq, 3), dtype=np.uint64)


def _weighted_specs(nq):
    """Weights from 0.01 to 4 across the queries."""
    ws = np.geomspace(0.01, 4.0, max(nq, 2))
    return [{"columns": [("near", 1.3 + 0.17 * q, 5.0, float(ws[q]), float(ws[q]) / 2),
                         ("ramp", 100.0, 650.0, float(ws[q]) / 3, 0.0) if q % 2 else None],
             "tags": [(1 << (q % 6), float(ws[q]) / 8)]} for q in range(nq)]


@pytest.fixture(scope="module")
def normal_indexes(vf):
    xb, _ = _data(1, N, seed=5)
    cols, tags = _attr_data(N, seed=6)
    out = {}
    for dtype in ("f32", "bf16"):
        for metric in (L2, IP):
            index = vf.IndexFlat(DIM, metric, dtype=dtype)
            index.add(xb)
            out[dtype, metric] = (index, index.attributes(cols, tags))
    return xb, cols, tags, out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [3, 40])
def test_composition(vf, normal_indexes, dtype, metric, nq):
    xb, cols, tags, idx = normal_indexes
    index, attrs = idx[dtype, metric]
    _, xq = _data(nq, N, seed=8)
    if dtype == "bf16":
        xb, xq = flat.round_bf16(xb), flat.round_bf16(xq)
    specs = _weighted_specs(nq)
    where = _third_bands(nq)
    mask = wo.pass_mask(cols, tags, *where, n=N)
    assert 0.25 < mask.mean() < 0.42
    rng = np.random.default_rng(9)
    scores = flat.exact_scores(xb, xq, metric)
    key = scores if metric == L2 else -scores
    spread = float(np.std(key))
    exclude, lists = [], []
    for q in range(nq):
        passing = np.nonzero(mask[q])[0]
        failing = np.nonzero(~mask[q])[0]
        near = passing[np.argsort(key[q, passing])[:24]]  # the allowed raw top
        ex = [int(v) for v in near[:4]] + [int(v) for v in rng.choice(N, 5, replace=False)]
        exclude.append(ex if q % 3 else [])
        # listed: allowed near rows of both signs, far passing rows, rows that
        # fail the predicate, and excluded rows — the last two with a bonus
        # that would put them first
        labels = np.unique(np.concatenate([
            near[2:16], rng.choice(passing, 20, replace=False), failing[:6],
            np.asarray(ex[:3], dtype=np.int64)]))
        vals = rng.uniform(-1.5, 1.5, labels.size) * spread
        vals[np.isin(labels, failing[:6]) | np.isin(labels, ex[:3])] = 50.0 * spread
        lists.append((labels.astype(np.int64), vals.astype(np.float32)))
    b = _oracle_b(vf, cols, tags, specs, nq)
    s, listed = bno.dense_lists(lists, nq, N)
    allowed = mask & ~wo.excluded_mask(exclude, nq, N)
    assert (listed & ~mask).any() and (listed & wo.excluded_mask(exclude, nq, N)).any()
    for k in (10, 70):
        Dr, Ir = bno.bonus_topk(scores, b, s, listed, mask, k, metric, exclude=exclude)
        for scan in (False, True):
            D, I = index.search_bonus(xq, k, lists, attrs=attrs, boost=specs, where=where,
                                      exclude=exclude, scan=scan)
            for q in range(nq):
                got = I[q][I[q] >= 0]
                assert allowed[q][got].all(), ("a row that is not allowed came back", q)
                assert got.size == min(k, int(allowed[q].sum()))
            bad = bno.mismatches(D, I, Dr, Ir, metric, xb, xq, b, s, listed)
            assert bad == [], bad[:5]
    assert (np.take_along_axis(listed, np.maximum(Ir, 0), axis=1) & (Ir >= 0)).any()


# ---- 6. liveness ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", [L2, IP])
def test_liveness(vf, metric, dtype):
    nq, k = 9, 20
    xb, xq = _int_data(nq, N, seed=41)  # small integers: exact in bf16 too
    cols, tags = _half_levels(N, seed=42)
    index = vf.IndexFlat(DIM, metric, dtype=dtype)
    index.add(xb)
    rng = np.random.default_rng(43)
    listed_rows = [rng.choice(N, 60, replace=False) for _ in range(nq)]
    gone = np.unique(np.concatenate([lr[:10] for lr in listed_rows] +
                                    [rng.choice(N, 100, replace=False)]))
    assert index.remove_ids(gone) == gone.size  # bf16: tombstones; fp32: the rows move
    keep = np.setdiff1d(np.arange(N), gone)
    live = keep.size
    label_of = {int(r): i for i, r in enumerate(keep)}  # labels: positions among the live rows
    xk, ck, tk = xb[keep].copy(), cols[:, keep], tags[keep]
    lists = []
    for q in range(nq):
        labels = [label_of[int(r)] for r in listed_rows[q] if int(r) in label_of]  # the removed
        # rows have no label any more; labels past the live rows and -1 name nothing
        labels += [live, live + 7, N - 1, 10 ** 12, -1]
        vals = (rng.integers(-32, 33, len(labels)) * 0.25).astype(np.float32)
        lists.append((np.asarray(labels, dtype=np.int64), vals))
    # some listed rows get new vectors in place
    upd = np.unique(np.concatenate([l[:3] for l, _ in lists]))
    xk[upd] = rng.integers(-2, 3, size=(upd.size, DIM)).astype(np.float32)
    xk[upd[:nq]] = xq[:upd[:nq].size]  # and some become a query itself
    index.update(upd, xk[upd])
    assert index.ntotal == live
    specs = _dyadic_specs(nq)
    with index.attributes(ck, tk) as attrs:
        for sp, at in ((None, None), (specs, attrs)):
            scores, b, s, listed = _exact_case(vf, xk, xq, ck, tk, sp, lists, metric)
            assert listed.sum() == sum(l.size for l, _ in lists) - 5 * nq
            Dr, Ir = bno.bonus_topk(scores, b, s, listed, None, k, metric)
            vf.bonus_stats(reset=True)
            D, I = index.search_bonus(xq, k, lists, attrs=at, boost=sp)
            np.testing.assert_array_equal(I, Ir)
            np.testing.assert_array_equal(D, Dr)
            assert vf.bonus_stats(reset=True)[1] == int(listed.sum())


# ---- 7. limits and errors on the device path --------------------------------------------
def _raw_call(index, xq, k, offs, labels, vals):
    from vsearch import _lib

    n = xq.shape[0]
    D = np.empty((n, k), dtype=np.float32)
    I = np.empty((n, k), dtype=np.int64)
    rc = _lib.load().vs_search_bonus(
        index._h, None, xq.ctypes.data, n, k, offs.ctypes.data, labels.ctypes.data,
        vals.ctypes.data, None, None, None, None, None, None, None, None, None, D.ctypes.data,
        I.ctypes.data, 0, None)
    return rc, _lib.load().vs_last_error().decode(), D, I


def test_limits_and_errors(vf, int_indexes):
    from vsearch import _lib

    xb, cols, tags, idx = int_indexes
    index, attrs = idx[IP]
    nq = 3
    _, xq = _int_data(nq, N, seed=51)
    rng = np.random.default_rng(52)
    full = [(rng.choice(N, 1024, replace=False).astype(np.int64),
             (rng.integers(-32, 33, 1024) * 0.25).astype(np.float32)) for _ in range(nq)]
    scores, b, s, listed = _exact_case(vf, xb, xq, None, None, None, full, IP)
    Dr, Ir = bno.bonus_topk(scores, None, s, listed, None, 10, IP)
    D, I = index.search_bonus(xq, 10, full)  # a list of 1,024 works
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)
    offs, labels, vals = vf.bonus_csr(full, nq)
    rc, msg, D, I = _raw_call(index, xq, 10, offs, labels, vals)
    assert rc == 0
    np.testing.assert_array_equal(I, Ir)
    # 1,025 entries: the wrapper and the library both name the limit
    with pytest.raises(ValueError, match="1024"):
        index.search_bonus(xq[:1], 10, [(np.arange(1025), np.ones(1025))])
    one = xq[:1]
    rc, msg, _, _ = _raw_call(index, one, 10, np.array([0, 1025], dtype=np.int64),
                              np.arange(1025, dtype=np.int64), np.ones(1025, dtype=np.float32))
    assert rc == _lib.E_UNSUPPORTED and "1024" in msg and "vs_search_bonus" in msg
    # a duplicate label, a NaN, offsets that fall
    with pytest.raises(ValueError, match="twice"):
        index.search_bonus(one, 10, [([4, 9, 4], [1.0, 2.0, 3.0])])
    rc, msg, _, _ = _raw_call(index, one, 10, np.array([0, 3], dtype=np.int64),
                              np.array([4, 9, 4], dtype=np.int64), np.ones(3, dtype=np.float32))
    assert rc == _lib.E_INVALID and "twice" in msg
    with pytest.raises(ValueError, match="not finite"):
        index.search_bonus(one, 10, [{4: np.nan}])
    rc, msg, _, _ = _raw_call(index, one, 10, np.array([0, 2], dtype=np.int64),
                              np.array([4, 9], dtype=np.int64),
                              np.array([1.0, np.nan], dtype=np.float32))
    assert rc == _lib.E_INVALID and "not finite" in msg
    rc, msg, _, _ = _raw_call(index, xq[:2], 10, np.array([0, 2, 1], dtype=np.int64),
                              np.array([4, 9], dtype=np.int64), np.ones(2, dtype=np.float32))
    assert rc == _lib.E_INVALID and "offsets" in msg
    # boost or where without a handle
    with pytest.raises(ValueError, match="need attrs"):
        index.search_bonus(one, 10, None, boost=_dyadic_specs(1))
    lo = np.zeros((1, 1), dtype=np.float32)
    rc = _lib.load().vs_search_bonus(index._h, None, one.ctypes.data, 1, 10, None, None, None, None,
                                     None, None, None, lo.ctypes.data, None, None, None, None,
                                     D.ctypes.data, I.ctypes.data, 0, None)
    assert rc == _lib.E_INVALID and b"without attributes" in _lib.load().vs_last_error()


def test_k_above_the_allowed_rows_pads(vf):
    n, nq = 300, 5
    xb, xq = _int_data(nq, n, seed=61)
    cols, tags = _half_levels(n, seed=62)
    rng = np.random.default_rng(63)
    lists = [(rng.choice(n, 40, replace=False).astype(np.int64),
              (rng.integers(-32, 33, 40) * 0.25).astype(np.float32)) for _ in range(nq)]
    exclude = [[int(v) for v in lists[q][0][:5]] + [7, 8] for q in range(nq)]
    lo = np.full((nq, 1), 2.0, dtype=np.float32)
    hi = np.full((nq, 1), 7.0, dtype=np.float32)
    where = (lo, hi, np.zeros((nq, 3), dtype=np.uint64))
    mask = wo.pass_mask(cols, tags, *where, n=n)
    specs = _dyadic_specs(nq)
    for metric in (L2, IP):
        index = vf.IndexFlat(DIM, metric)
        index.add(xb)
        with index.attributes(cols, tags) as attrs:
            scores, b, s, listed = _exact_case(vf, xb, xq, cols, tags, specs, lists, metric)
            k = n + 10
            for m, kw in ((None, {}), (mask, {"attrs": attrs, "boost": specs, "where": where})):
                Dr, Ir = bno.bonus_topk(scores, b if m is not None else None, s, listed, m, k,
                                        metric, exclude=exclude)
                assert (Ir[:, -1] == -1).all() and (Ir[:, 0] >= 0).all()
                D, I = index.search_bonus(xq, k, lists, exclude=exclude, **kw)
                np.testing.assert_array_equal(I, Ir)
                np.testing.assert_array_equal(D, Dr)


def test_device_outputs_and_a_capturing_stream(vf, int_indexes):
    import torch

    from vsearch import _lib

    xb, cols, tags, idx = int_indexes
    index, attrs = idx[L2]
    nq, k = 40, 10
    _, xq = _int_data(nq, N, seed=71)
    specs = _dyadic_specs(nq)
    lists = _quarter_lists(nq, N, seed=72)
    q = torch.from_numpy(xq).cuda()
    D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    for kw in ({}, {"attrs": attrs, "boost": specs}, {"attrs": attrs, "boost": specs,
                                                      "scan": True}):
        Dh, Ih = index.search_bonus(xq, k, lists, **kw)
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            index.search_bonus_device(q.data_ptr(), nq, k, lists, D.data_ptr(), I.data_ptr(),
                                      stream=st.cuda_stream, **kw)
        st.synchronize()
        np.testing.assert_array_equal(I.cpu().numpy(), Ih)
        np.testing.assert_array_equal(_bits(D.cpu().numpy()), _bits(Dh))
    g = torch.cuda.CUDAGraph()
    buf = torch.zeros(8, device="cuda")
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        g.capture_begin(capture_error_mode="thread_local")
        try:
            buf.add_(1.0)
            with pytest.raises(_lib.VSearchError, match="capturing stream") as ei:
                index.search_bonus_device(q.data_ptr(), nq, k, lists, D.data_ptr(), I.data_ptr(),
                                          stream=st.cuda_stream)
        finally:
            g.capture_end()
    assert ei.value.code == _lib.E_UNSUPPORTED


# ---- 8. the store -----------------------------------------------------------------------
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


def test_store_bonus_ranks_every_document(vf, catalog):
    st, metas, keywords = catalog
    n, k = len(metas), 5
    assert n == 341 and st.index.metric_type == L2
    ids = [m["book_id"] for m in metas]
    assert len(set(ids)) == n
    xb = st.index.reconstruct_n(0, n)
    for kw in keywords[:6]:
        xq = np.asarray([st._embed_query(kw)], dtype=np.float32)
        scores = flat.exact_scores(xb, xq, L2)
        order = np.argsort(scores[0], kind="stable")
        far, near = int(order[-1]), int(order[0])
        bonus = {ids[far]: float(scores[0, far]) + 1.0,    # the farthest book: first
                 ids[near]: -(float(scores[0, order[k + 2]]) + 1.0),  # the nearest: out
                 ids[int(order[3])]: 0.01, ids[int(order[40])]: 0.02, "no such book": 9.0}
        s, listed = bno.dense_lists([{ids.index(key): v for key, v in bonus.items()
                                      if key in ids}], 1, n)
        zero = np.zeros((1, n), dtype=np.float32)
        Dr, Ir = bno.bonus_topk(scores, None, s, listed, None, k, L2)
        got = st.similarity_search_with_score(kw, k=k, bonus=bonus)
        I = np.array([[ids.index(d.metadata["book_id"]) for d, _ in got]], dtype=np.int64)
        D = np.array([[sc for _, sc in got]], dtype=np.float32)
        assert I[0, 0] == far and near not in I[0].tolist()
        assert not bno.mismatches(D, I, Dr, Ir, L2, xb, xq, zero, s, listed)
        assert [d.metadata["book_id"] for d in st.similarity_search(kw, k=k, bonus=bonus)] == \
            [ids[i] for i in I[0]]
        # a search of k * 2 rows plus the bonus on the host never finds the promoted book
        plain = st.similarity_search_with_score(kw, k=2 * k)
        assert ids[far] not in [d.metadata["book_id"] for d, _ in plain]


def test_store_profiles_with_the_social_term(vf, catalog):
    from vsearch import students

    st, metas, keywords = catalog
    n, k = len(metas), 6
    ids = [m["book_id"] for m in metas]
    names = [f"student{i}" for i in range(6)]
    profiles = [[(ids[(7 * s + j) % n], 1.0 - 0.2 * j) for j in range(4)] for s in range(6)]
    read = [[ids[(11 * s + j) % n] for j in range(5)] for s in range(6)]
    boosts = [_store_boost(2.0 + 0.7 * s) for s in range(6)]
    # the neighbour graph and the recent checkouts of the neighbours
    rng = np.random.default_rng(81)
    neighbours = [(names[a], names[(a + d) % 6], 0.95 - 0.03 * d) for a in range(6)
                  for d in range(1, 6) if a != 4]  # student4 has no neighbours
    checkouts = [(names[int(rng.integers(0, 6))], ids[int(rng.integers(0, n))])
                 for _ in range(120)]
    checkouts += [(names[1], read[0][0]), (names[2], profiles[0][0][0])]  # a read and a rated book
    social = students.neighbour_bonus(neighbours, checkouts, weight=0.2, top=5)
    assert names[4] not in social and len(social[names[0]]) > 10
    bonus = [social.get(name) for name in names]
    rows = st.recommend_for_profiles(profiles, k=k, exclude=read, boost=boosts, bonus=bonus)
    # the same formula in numpy: distance - b - s over every allowed document
    kept, prows, lists = st.profile_requests(profiles, read, "book_id")
    assert kept == list(range(6))
    vec = st.index.mean_rows(prows)
    xb = st.index.reconstruct_n(0, n)
    scores = flat.exact_scores(xb, vec, L2)
    b = np.stack([_store_b(metas, 2.0 + 0.7 * s) for s in range(6)])
    s, listed = bno.dense_lists([None if e is None else {ids.index(key): v for key, v in e.items()}
                                 for e in bonus], 6, n)
    Dr, Ir = bno.bonus_topk(scores, b, s, listed, None, k, L2, exclude=lists)
    I = np.array([[ids.index(d.metadata["book_id"]) for d, _ in row] for row in rows])
    D = np.array([[sc for _, sc in row] for row in rows], dtype=np.float32)
    assert I.shape == (6, k)
    assert not bno.mismatches(D, I, Dr, Ir, L2, xb, vec, b, s, listed)
    for q in range(6):
        barred = {v for v, _ in profiles[q]} | set(read[q])
        assert not barred & {ids[i] for i in I[q]}
    # the social term changes at least one list, and one profile alone gives its own row
    plain = st.recommend_for_profiles(profiles, k=k, exclude=read, boost=boosts)
    assert any([d.metadata["book_id"] for d, _ in rows[q]] !=
               [d.metadata["book_id"] for d, _ in plain[q]] for q in range(6))
    one = st.recommend_for_profiles([profiles[2]], k=k, exclude=[read[2]], boost=boosts[2],
                                    bonus=bonus[2])[0]
    assert [d.metadata["book_id"] for d, _ in one] == [d.metadata["book_id"] for d, _ in rows[2]]
    vec0 = st._embed_query(keywords[0])
    batch = st.similarity_search_batch_by_vector([vec0, vec0], k=k, bonus=[bonus[0], None])
    assert [d.metadata["book_id"] for d, _ in batch[1]] == \
        [d.metadata["book_id"] for d in st.similarity_search_by_vector(vec0, k=k)]
    assert [d.metadata["book_id"] for d, _ in batch[0]] == \
        [d.metadata["book_id"] for d in st.similarity_search_by_vector(vec0, k=k, bonus=bonus[0])]
    with pytest.raises(ValueError, match="not built"):
        st.similarity_search("x", k=k, bonus=bonus[0], distinct="book_id")
