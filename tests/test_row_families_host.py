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

from helpers import (FAMILY_JOIN_ROWS, FAMILY_SHAPE, FAMILY_WIDE, FAMILY_WIDEST_K, ROW_FAMILIES,
                     ZERO_QUERIES, family_case, family_skip, free_share, free_share_cosine,
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
