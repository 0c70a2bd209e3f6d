"""CPU: the row families of tests/test_gpu_row_families.py are admissible inputs.

The strict checkers (flat.mismatches / flat.selfjoin_mismatches with
strict=True) accept either label where two exact scores lie within the sum of
their rounding windows.  On data where many ranks tie they would pass anything,
so every family, metric and shape the GPU file searches must keep that share
(helpers.free_share, from the fp64 oracle alone) at or below 2 %.  This is a
condition on the inputs, not a measurement of the engine: another seed or shape
is admissible exactly when it passes here.

Shares at n = 6000, nq = 100, k = 10 (cosine over 300 query rows), d = 100 seed
7 and d = 64 seed 11: 0 for the inner product everywhere; at most 0.001 for L2
and the cosine on ladder, spike, sparse, late and pow2; offset 0.011 / 0.0083
(d = 100) and 0.009 / 0.0077 (d = 64) for L2 / cosine; ladder at d = 1024,
n = 3000: 0.002 for L2.  "zeros" under L2 has 0.2 (the two exact ties among the
three zero rows at ranks 0 to 2 of every query) until those rows are skipped;
they are checked on their own on the GPU."""

import numpy as np
import pytest

from helpers import (BAND_BASE, BAND_QUERIES, BAND_RADIUS, BAND_ROWS, FAMILY_JOIN_ROWS,
                     FAMILY_SHAPE, FAMILY_WIDE, FAMILY_WIDEST_K, JOIN_QUANTILES, RANGE_NQ,
                     RANGE_QUANTILES, ROW_FAMILIES, ZERO_QUERIES, bound_band_case, family_case,
                     family_half_mask, family_skip, family_tombstones, free_share,
                     free_share_cosine, join_reference, join_threshold, join_valid, range_cap,
                     range_classes, range_contract, range_counts, range_radius, range_reference,
                     row_family, zero_rows)
from oracle import flat

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
CAP = 0.02
SHAPES = [FAMILY_SHAPE, (6000, 64, 100, 10, 11)]


@pytest.fixture(scope="module")
def cases():
    memo = {}

    def get(name, shape):
        key = (name, shape)
        if key not in memo:
            n, d, nq, _, seed = shape
            memo[key] = family_case(name, n, d, nq, seed)
        return memo[key]

    return get


@pytest.mark.parametrize("name", ROW_FAMILIES)
def test_generators_are_deterministic_and_finite(name):
    n, d, nq, seed = 500, 100, 40, 7
    xb, xq = row_family(name, n, d, nq, seed)
    xb2, xq2 = row_family(name, n, d, nq, seed)
    assert xb.dtype == xq.dtype == np.float32
    assert xb.shape == (n, d) and xq.shape == (nq, d)
    np.testing.assert_array_equal(xb, xb2)
    np.testing.assert_array_equal(xq, xq2)
    assert np.isfinite(xb).all() and np.isfinite(xq).all()
    xb3, _ = row_family(name, n, d, nq, seed + 1)
    assert not np.array_equal(xb, xb3)


def test_families_have_the_structure_they_name():
    n, d, nq, seed = 2000, 100, 100, 7
    nrm = lambda x: np.sqrt(np.einsum("ij,ij->i", x.astype(np.float64), x.astype(np.float64)))
    xb, xq = row_family("ladder", n, d, nq, seed)
    assert nrm(xb).max() / nrm(xb).min() > 1e3 and nrm(xq).max() / nrm(xq).min() > 1e2
    xb, xq = row_family("spike", n, d, nq, seed)
    top2 = np.sort(np.abs(xb), axis=1)[:, -2:]
    assert np.median(top2[:, 1] / top2[:, 0]) > 10
    xb, xq = row_family("offset", n, d, nq, seed)
    assert (np.abs(xb.mean(axis=0)) > 7.5).all() and (np.sign(xb.mean(0)) == np.sign(xq.mean(0))).all()
    xb, xq = row_family("sparse", n, d, nq, seed)
    assert ((xb != 0).sum(axis=1) == 4).all() and (xq != 0).all()
    xb, xq = row_family("zeros", n, d, nq, seed)
    assert np.nonzero(~xb.any(axis=1))[0].tolist() == list(zero_rows(n)) and xq.any(axis=1).all()
    _, xq = family_case("zeros", n, d, nq, seed)
    assert np.nonzero(~xq.any(axis=1))[0].tolist() == list(ZERO_QUERIES)
    xb, xq = row_family("late", n, d, nq, seed)
    assert nrm(xb[n - n // 10:]).min() > 50 * nrm(xb[:n - n // 10]).max()
    x0, q0 = row_family("pow2:0", n, d, nq, seed)
    for e in (-40, 40):  # exact scalings of the same draw
        xe, qe = row_family(f"pow2:{e}", n, d, nq, seed)
        np.testing.assert_array_equal(xe, np.ldexp(x0, e))
        np.testing.assert_array_equal(qe, np.ldexp(q0, e))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"d{s[1]}")
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("name", ROW_FAMILIES)
def test_search_inputs_have_few_free_ranks(cases, name, metric, shape):
    n, d, nq, k, _ = shape
    xb, xq = cases(name, shape)
    share = free_share(xb, xq, metric, k, skip=family_skip(name, n))
    assert share <= CAP, (name, metric, share)
    # the small calls of the fp32-accumulating routes search the leading queries
    for sub in (1, 20):
        assert free_share(xb, xq[:sub], metric, k, skip=family_skip(name, n)) <= CAP, (name, sub)


def test_zero_rows_are_the_only_l2_ties_of_zeros(cases):
    """Unskipped, "zeros" has two free ranks of ten under L2 for every query:
    the exact ties among its three zero rows, which are every query's nearest."""
    n, d, nq, k, _ = FAMILY_SHAPE
    xb, xq = cases("zeros", FAMILY_SHAPE)
    assert free_share(xb, xq, L2, k) == pytest.approx(0.2, abs=0.002)
    _, Ir = flat.knn_exact(xb, xq, 3, L2)
    assert (np.sort(Ir, axis=1) == np.array(zero_rows(n))).all()
    assert free_share(xb, xq, L2, k, skip=family_skip("zeros", n)) <= CAP


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"d{s[1]}")
@pytest.mark.parametrize("name", ROW_FAMILIES)
def test_selfjoin_inputs_have_few_free_ranks(cases, name, shape):
    n, d, nq, k, _ = shape
    xb, _ = cases(name, shape)
    skip = zero_rows(n) if name == "zeros" else None
    share = free_share_cosine(xb, k, np.arange(FAMILY_JOIN_ROWS), skip=skip)
    assert share <= CAP, (name, share)


def test_late_first_add_has_few_free_ranks(cases):
    n, d, nq, k, _ = FAMILY_SHAPE
    xb, xq = cases("late", FAMILY_SHAPE)
    first = xb[:n - n // 10]
    for metric in (IP, L2):
        assert free_share(first, xq, metric, k) <= CAP
    assert free_share_cosine(first, k, np.arange(FAMILY_JOIN_ROWS)) <= CAP


def test_ladder_extra_shapes_have_few_free_ranks(cases):
    n, d, nq, k, _ = FAMILY_SHAPE
    xb, xq = cases("ladder", FAMILY_SHAPE)
    for metric, kw in FAMILY_WIDEST_K.items():
        assert free_share(xb, xq, metric, kw) <= CAP, (metric, kw)
    xb, xq = cases("ladder", FAMILY_WIDE)
    for metric in (IP, L2):
        assert free_share(xb, xq, metric, FAMILY_WIDE[3]) <= CAP, metric


# ---- range searches and range self-joins (tests/test_gpu_range_families.py) ---------------------
# The range contract accepts either answer for a pair whose fp64 score lies
# within its window of the radius.  Every (family, storage, batch, metric,
# quantile) the GPU file searches must keep those pairs at or below
# helpers.range_cap of the oracle's own hit count, have hits at all, and, over
# a family's cases, have one query without a hit and one with more than 128
# (a 128-row tile), so that the count and fill passes see empty and multi-tile
# segments.  Conditions on the inputs, from the fp64 oracle alone.
#
# Measured (6000 x 100, seed 7): every search case has at most 2 undecided
# pairs except "offset" under L2: 68 (f32) / 54 (bf16) of ~120,000 hits at
# quantile 0.2 with 100 queries, 12 / 16 of ~22,800 with 19, and 8 / 9 of
# ~6,000 at 0.01; the worst undecided / cap is 0.67.  The joins (about 89,985,
# 17,997 and 1,800 hits at cosine quantiles 0.95, 0.99 and 0.999; "zeros"
# 17,929 and 1,793 at the last two) have at most 3, "offset" 93 / 29 / 4 as
# f32 and 119 / 29 / 8 as bf16 rows (caps 449 / 89 / 9).  Only "offset" has a
# query row with more than 128 hits at 0.99; 0.95 (about 300 a row) gives every
# family one, which is why the joins have that third quantile.
STORAGE = {"f32": lambda x: x, "bf16": flat.round_bf16}


@pytest.fixture(scope="module")
def range_refs(cases):
    memo = {}

    def get(name, storage, metric):
        key = (name, storage, metric)
        if key not in memo:
            xb, xq = cases(name, FAMILY_SHAPE)
            memo[key] = range_reference(STORAGE[storage](xb), STORAGE[storage](xq), metric)
        return memo[key]

    return get


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", ROW_FAMILIES)
def test_range_search_cases_are_decided_by_the_oracle(range_refs, name, storage):
    empty = crowded = False
    for metric in (IP, L2):
        s100, w100 = range_refs(name, storage, metric)
        for nq in RANGE_NQ:
            s, w = s100[:nq], w100[:nq]
            for quantile in RANGE_QUANTILES:
                radius = range_radius(s, metric, quantile)
                assert np.isfinite(radius)
                hits, undecided, per_query = range_counts(s, w, radius, metric)
                print(f"range {name} {storage} {'IP' if metric == IP else 'L2'} nq={nq} "
                      f"q={quantile}: hits {hits} undecided {undecided} cap {range_cap(hits)} "
                      f"per query {per_query.min()}..{per_query.max()}")
                assert hits > 0, (name, metric, nq, quantile)
                assert undecided <= range_cap(hits), (name, metric, nq, quantile, undecided, hits)
                empty |= bool((per_query == 0).any())
                crowded |= bool((per_query > 128).any())
    assert empty, (name, storage, "no case has a query without a hit")
    assert crowded, (name, storage, "no case has a query with more than 128 hits")


def test_range_late_first_add_is_decided_by_the_oracle(cases):
    """The "late" family is searched after its first add too (nine tenths of
    the rows), with a radius of that add's own scores."""
    n = FAMILY_SHAPE[0]
    xb, xq = cases("late", FAMILY_SHAPE)
    n1 = n - n // 10
    for storage, rnd in STORAGE.items():
        for metric in (IP, L2):
            s100, w100 = range_reference(rnd(xb[:n1]), rnd(xq), metric)
            for nq in RANGE_NQ:
                s, w = s100[:nq], w100[:nq]
                for quantile in RANGE_QUANTILES:
                    radius = range_radius(s, metric, quantile)
                    hits, undecided, _ = range_counts(s, w, radius, metric)
                    print(f"range late[:{n1}] {storage} {'IP' if metric == IP else 'L2'} nq={nq} "
                          f"q={quantile}: hits {hits} undecided {undecided} cap {range_cap(hits)}")
                    assert hits > 0 and undecided <= range_cap(hits), (storage, metric, nq,
                                                                       quantile, undecided, hits)


def test_range_selected_half_is_decided_by_the_oracle(range_refs):
    """"ladder" with the random half family_half_mask selects."""
    mask = family_half_mask(FAMILY_SHAPE[0])
    assert 0.45 * mask.size < mask.sum() < 0.55 * mask.size
    for metric in (IP, L2):
        s, w = range_refs("ladder", "f32", metric)
        radius = range_radius(s, metric, 0.01)
        hits, undecided, _ = range_counts(s, w, radius, metric, valid=mask[None, :])
        print(f"range ladder half {'IP' if metric == IP else 'L2'}: hits {hits} "
              f"undecided {undecided} cap {range_cap(hits)}")
        assert hits > 0 and undecided <= range_cap(hits)


def test_range_tombstone_case_is_decided_by_the_oracle(cases):
    """"ladder" as a bf16 index after the removal of 50 planted query copies."""
    xb, xq = cases("ladder", FAMILY_SHAPE)
    _, ids, live = family_tombstones(xb, xq)
    assert ids.size == 50 == np.unique(ids).size and live.shape[0] == xb.shape[0] - 50
    s, w = range_reference(flat.round_bf16(live), flat.round_bf16(xq), L2)
    radius = range_radius(s, L2, 0.01)
    hits, undecided, _ = range_counts(s, w, radius, L2)
    print(f"range ladder bf16 tombstones L2: hits {hits} undecided {undecided} "
          f"cap {range_cap(hits)}")
    assert hits > 0 and undecided <= range_cap(hits)
    # each removed row would have been a hit: a copy of a query, at distance 0
    planted = flat.round_bf16(xq[np.arange(50) % xq.shape[0]])
    gone = flat.exact_scores(planted, flat.round_bf16(xq), L2)
    assert (gone[np.arange(50) % xq.shape[0], np.arange(50)] == 0).all() and radius > 0


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", ROW_FAMILIES)
def test_range_join_cases_are_decided_by_the_oracle(cases, name, storage):
    n = FAMILY_SHAPE[0]
    xb, _ = cases(name, FAMILY_SHAPE)
    s, w = join_reference(STORAGE[storage](xb), FAMILY_JOIN_ROWS)
    empty = crowded = False
    for quantile in JOIN_QUANTILES:
        t = join_threshold(s, quantile)
        assert 0 < t < 1
        for upper in (False, True):
            valid = join_valid(FAMILY_JOIN_ROWS, n, upper=upper)
            hits, undecided, per_query = range_counts(s, w, t, "cosine", valid)
            print(f"join {name} {storage} q={quantile} upper={upper}: t {t:.6f} hits {hits} "
                  f"undecided {undecided} cap {range_cap(hits)} "
                  f"per query {per_query.min()}..{per_query.max()}")
            assert hits > 0
            assert undecided <= range_cap(hits), (name, quantile, upper, undecided, hits)
            empty |= bool((per_query == 0).any())
            crowded |= bool((per_query > 128).any())
    assert empty, (name, storage, "no case has a query row without a hit")
    assert crowded, (name, storage, "no case has a query row with more than 128 hits")
    if name == "zeros":  # a zero row matches nothing and is matched by nothing
        assert np.isnan(s[0]).all() and np.isnan(s[1:, list(zero_rows(n))]).all()


def test_range_join_late_first_add_is_decided_by_the_oracle(cases):
    n = FAMILY_SHAPE[0]
    xb, _ = cases("late", FAMILY_SHAPE)
    n1 = n - n // 10
    for storage, rnd in STORAGE.items():
        s, w = join_reference(rnd(xb[:n1]), FAMILY_JOIN_ROWS)
        for quantile in JOIN_QUANTILES:
            t = join_threshold(s, quantile)
            for upper in (False, True):
                hits, undecided, _ = range_counts(s, w, t, "cosine",
                                                  join_valid(FAMILY_JOIN_ROWS, n1, upper=upper))
                print(f"join late[:{n1}] {storage} q={quantile} upper={upper}: hits {hits} "
                      f"undecided {undecided} cap {range_cap(hits)}")
                assert hits > 0 and undecided <= range_cap(hits)


def test_band_case_lets_the_bound_decide():
    """helpers.bound_band_case, from the oracle and a CPU fp32 sgemm alone: few
    undecided pairs; about half of the band's own pairs are hits; every one of
    them lies within 2e-4 of the radius, which is thousands of windows and about
    the error an fp32 accumulation makes on such a row (numpy's sgemm, as a
    stand-in for the candidate GEMM, used as the only test would drop more than
    100 of the hits); and the second add's norms are 10,000 times the first's,
    so maxima that did not grow give a bound far below that error."""
    base, band, xq = bound_band_case()
    xb = np.concatenate([base, band])
    s, w = range_reference(xb, xq, IP)
    hits, undecided, _ = range_counts(s, w, BAND_RADIUS, IP)
    print(f"range band IP: hits {hits} undecided {undecided} cap {range_cap(hits)}")
    assert hits > 70000 and undecided <= range_cap(hits)
    rows = np.arange(BAND_ROWS)
    own = np.zeros(s.shape, dtype=bool)
    own[rows % BAND_QUERIES, BAND_BASE + rows] = True
    hit, inside, outside = range_classes(s, w, BAND_RADIUS, IP)
    assert 600 < (hit & own).sum() < 1000 and (~(inside | outside) & own).sum() <= 2
    gap = np.abs(s[own] - float(BAND_RADIUS))
    assert gap.max() < 2e-4 and np.median(gap) > 1000 * w[own].max()
    approx = (xq @ xb.T).astype(np.float64)  # fp32 sgemm
    assert np.abs(approx[own] - s[own]).std() > 3 * gap.std()
    dropped = int((inside & own & ~(approx > float(BAND_RADIUS))).sum())
    print(f"range band IP: an fp32 sgemm alone drops {dropped} of {int((inside & own).sum())}")
    assert dropped > 100
    nrm = np.sqrt(np.einsum("ij,ij->i", xb.astype(np.float64), xb.astype(np.float64)))
    assert nrm[BAND_BASE:].min() > 1e4 * nrm[:BAND_BASE].max()


def test_range_classes_fail_on_nan_and_respect_valid():
    """range_classes: the oracle's hit rule per kind, NaN scores outside, and
    `valid` removing pairs from hit / inside."""
    s = np.array([[0.0, 1.0, 2.0, np.nan]])
    w = np.full_like(s, 0.25)
    hit, inside, outside = range_classes(s, w, 1.0, L2)
    assert hit.tolist() == [[True, False, False, False]]
    assert inside.tolist() == [[True, False, False, False]]
    assert outside.tolist() == [[False, False, True, True]]
    hit, inside, outside = range_classes(s, w, 1.0, IP)
    assert hit.tolist() == [[False, False, True, False]]
    assert outside.tolist() == [[True, False, False, True]]
    hit, inside, outside = range_classes(s, w, 1.0, "cosine", valid=np.array([[True, True, False,
                                                                               True]]))
    assert hit.tolist() == [[False, True, False, False]]
    assert inside.tolist() == [[False, False, False, False]]
    assert outside.tolist() == [[True, False, True, True]]
    assert range_cap(0) == 2 and range_cap(399) == 2 and range_cap(120000) == 600


def _oracle_result(s, hit):
    """The (lims, D, I) a correct engine returns for the hit matrix `hit`."""
    lims = np.zeros(s.shape[0] + 1, dtype=np.uint64)
    lims[1:] = np.cumsum(hit.sum(axis=1))
    q, r = np.nonzero(hit)
    return lims, s[q, r].astype(np.float32), r.astype(np.int64)


@pytest.mark.parametrize("kind", [L2, IP, "cosine"])
def test_range_contract_accepts_the_oracle_and_reports_each_fault(kind):
    """helpers.range_contract on a small case: the oracle's own answer passes;
    a missing hit, an extra row, a wrong or NaN D, unsorted labels and a
    broken lims each fail it."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((400, 24)).astype(np.float32)
    if kind == "cosine":
        s, w = join_reference(x, 30)
        valid = join_valid(30, 400)
        radius = join_threshold(s, 0.95, nq=30)
    else:
        s, w = range_reference(x, x[:30] + np.float32(0.5), kind)
        valid = None
        radius = range_radius(s, kind, 0.05)
    hit, inside, outside = range_classes(s, w, radius, kind, valid)
    assert int((~(inside | outside)).sum()) == 0 and hit.sum() > 60
    good = _oracle_result(s, hit)
    args = dict(valid=valid, timer=False)
    assert range_contract(good, s, w, radius, kind, **args) == (int(hit.sum()), 0)

    def fails(result):
        with pytest.raises(AssertionError):
            range_contract(result, s, w, radius, kind, **args)

    q, r = np.nonzero(hit)
    drop = hit.copy()
    drop[q[7], r[7]] = False
    fails(_oracle_result(s, drop))
    extra = hit.copy()
    q0, r0 = np.argwhere(outside & (valid if valid is not None else True))[0]
    extra[q0, r0] = True
    fails(_oracle_result(s, extra))
    for value in (np.nan, np.inf, good[1][5] * np.float32(1.001) + np.float32(1e-3)):
        D = good[1].copy()
        D[5] = value
        fails((good[0], D, good[2]))
    seg = np.nonzero(hit.sum(axis=1) >= 2)[0][0]
    a = int(good[0][seg])
    I = good[2].copy()
    I[[a, a + 1]] = I[[a + 1, a]]
    D = good[1].copy()
    D[[a, a + 1]] = D[[a + 1, a]]
    fails((good[0], D, I))
    lims = good[0].copy()
    lims[-1] -= 1
    fails((lims, good[1], good[2]))
    fails((good[0].astype(np.int64), good[1], good[2]))


def test_skip_removes_rows_and_queries():
    """free_share's skip: three planted duplicate rows make every query's top
    ranks free; left out, the share is that of the rows that remain."""
    rng = np.random.default_rng(1)
    xb = rng.standard_normal((400, 32)).astype(np.float32)
    xq = rng.standard_normal((10, 32)).astype(np.float32)
    base = free_share(xb, xq, IP, 5)
    big = 50.0 * xq[3]
    xd = np.concatenate([xb, np.stack([big, big, big])])
    assert free_share(xd, xq[3:4], IP, 5) == pytest.approx(0.4)  # ranks 0 and 1 of 5
    assert free_share(xd, xq, IP, 5, skip=((400, 401, 402), ())) == base
    assert free_share(xd, xq, IP, 5, skip=((401, 402), (3,))) == free_share(
        np.concatenate([xb, big[None]]), np.delete(xq, 3, axis=0), IP, 5)
