"""GPU: the staged filter-and-verify engine on rows that stress its bounds.

The engine's exactness rests on data-dependent quantities:
per-row int8 scales, rounded-up residual norms, the index maxima of
bound_stats_kernel, the L2 augmentation l2aug_params fixes at the first add,
the bf16 plane's extra block, the cuts, the wide check and the exact-key
stream.  A wrong bound does not crash: it drops a true neighbour silently.  The
rest of the suite feeds the engine rows of one scale; here every family of
helpers.row_family (norms over four decades, one dominant coordinate, a large
common component, sparse rows, zero rows and queries, late rows 100x larger
than those that fixed the augmentation, the whole problem at 2^-40 and 2^+40)
goes through every staged engine and is compared STRICTLY with the fp64 oracle
on every query (flat.mismatches / flat.selfjoin_mismatches, strict=True: D is
the fp32 rounding of the label's exact score, another label only inside both
rounding windows).  tests/test_row_families_host.py shows that on these inputs
at most 2 % of the ranks are such ties, so the strict check cannot pass by
tolerance.

Every search prints the stage counters (filter_stats, filter_wide_stats,
filter_second_stats, filter_exact_stats); they are recorded in
profiles/row_families/filter_stats.txt and not asserted."""

import numpy as np
import pytest

from helpers import (FAMILY_JOIN_ROWS, FAMILY_SHAPE, FAMILY_WIDE, FAMILY_WIDEST_K, ROW_FAMILIES,
                     ZERO_QUERIES, family_case, zero_rows)
from oracle import cfaiss, flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
METRICS = [IP, L2]
ENGINES = ["auto", "i8v", "bf16v"]
N, DIM, NQ, K, SEED = FAMILY_SHAPE
MNAME = {IP: "IP", L2: "L2"}


@pytest.fixture(scope="module")
def vf():
    from vsearch import _lib
    from vsearch import faiss as vfaiss

    assert _lib.device_count() >= 1, "gpu tests need a visible MI355X"
    return vfaiss


class _Memo:
    """Inputs, oracle results and engine results, each computed once per module
    and never modified (arrays are handed out read-only)."""

    def __init__(self, vf):
        self.vf = vf
        self._rows, self._ref, self._join_ref, self._run, self._join = {}, {}, {}, {}, {}

    def rows(self, name, shape=FAMILY_SHAPE):
        key = (name, shape)
        if key not in self._rows:
            n, d, nq, _, seed = shape
            xb, xq = family_case(name, n, d, nq, seed)
            xb.setflags(write=False)
            xq.setflags(write=False)
            self._rows[key] = (xb, xq)
        return self._rows[key]

    def ref(self, name, metric, k=K, shape=FAMILY_SHAPE, nrows=None):
        key = (name, metric, k, shape, nrows)
        if key not in self._ref:
            xb, xq = self.rows(name, shape)
            self._ref[key] = flat.knn_exact(xb[:nrows], xq, k, metric)
        return self._ref[key]

    def join_ref(self, name, nrows=None):
        key = (name, nrows)
        if key not in self._join_ref:
            xb, _ = self.rows(name)
            self._join_ref[key] = flat.pgvector_cosine_topk(xb[:nrows], K,
                                                            q_rows=np.arange(FAMILY_JOIN_ROWS))
        return self._join_ref[key]

    def search(self, index, xq, k, tag):
        """One search with the stage counters around it; the staged engine must
        have counted the whole batch."""
        from vsearch import _lib

        _lib.filter_stats(reset=True)
        D, I = index.search(xq, k)
        wide, second, exact = (_lib.filter_wide_stats(), _lib.filter_second_stats(),
                               _lib.filter_exact_stats())
        fq, ff = _lib.filter_stats(reset=True)
        print(f"stages {tag}: filter=({fq}, {ff}) wide={wide} second={second} exact={exact}")
        assert fq == xq.shape[0], (tag, fq, ff)
        return D, I

    def run(self, name, metric, engine):
        """The family's (D, I) at the matrix shape; for "late" the result after
        the second add (the first add's search is checked on the way)."""
        key = (name, metric, engine)
        if key in self._run:
            return self._run[key]
        xb, xq = self.rows(name)
        index = self.vf.IndexFlat(DIM, metric)
        assert index.filter_planes == ("i8", "bf16")
        index.set_engine(engine)
        tag = f"{name} {MNAME[metric]} {engine} k={K}"
        if name == "late":
            # nine tenths first: they fix an L2 index's augmentation; the last
            # tenth (100x larger) does not double the index, so it stays
            n1 = N - N // 10
            index.add(xb[:n1])
            D, I = self.search(index, xq, K, tag + " first add")
            Dr, Ir = self.ref(name, metric, nrows=n1)
            bad = flat.mismatches(D, I, Dr, Ir, metric, xb[:n1], xq, strict=True)
            assert not bad, (tag, "first add", bad[:5])
            index.add(xb[n1:])
        else:
            index.add(xb)
        assert index.ntotal == N
        D, I = self.search(index, xq, K, tag)
        D.setflags(write=False)
        I.setflags(write=False)
        self._run[key] = (D, I)
        return D, I

    def join(self, name, metric, engine):
        key = (name, metric, engine)
        if key in self._join:
            return self._join[key]
        xb, _ = self.rows(name)
        index = self.vf.IndexFlat(DIM, metric)
        index.set_engine(engine)
        if name == "late":
            n1 = N - N // 10
            index.add(xb[:n1])
            S, I = index.selfjoin(K, q0=0, nq=FAMILY_JOIN_ROWS)
            Sr, Ir = self.join_ref(name, nrows=n1)
            bad = flat.selfjoin_mismatches(S, I, Sr, Ir, xb[:n1], np.arange(FAMILY_JOIN_ROWS),
                                           strict=True)
            assert not bad, (name, engine, "first add", bad[:5])
            index.add(xb[n1:])
        else:
            index.add(xb)
        S, I = index.selfjoin(K, q0=0, nq=FAMILY_JOIN_ROWS)
        self._join[key] = (S, I)
        return S, I


@pytest.fixture(scope="module")
def memo(vf):
    return _Memo(vf)


def _strict(memo, name, metric, D, I, k=K, shape=FAMILY_SHAPE):
    xb, xq = memo.rows(name, shape)
    Dr, Ir = memo.ref(name, metric, k, shape)
    return flat.mismatches(D, I, Dr, Ir, metric, xb, xq, strict=True)


@pytest.mark.parametrize("name", ROW_FAMILIES)
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("metric", METRICS)
def test_search_matrix(memo, metric, engine, name):
    """Every family through every staged engine, both metrics: strict parity on
    every query, and the staged engine counted the whole batch."""
    D, I = memo.run(name, metric, engine)
    bad = _strict(memo, name, metric, D, I)
    assert not bad, (name, metric, engine, len(bad), bad[:5])


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("metric", METRICS)
def test_ladder_widest_lists(memo, vf, metric, engine):
    """k = 28 (inner product, 2k - 1 = 55 candidates) and k = 56 (L2): the widest
    lists the staged engine takes, on norms over four decades."""
    k = FAMILY_WIDEST_K[metric]
    xb, xq = memo.rows("ladder")
    index = vf.IndexFlat(DIM, metric)
    index.set_engine(engine)
    index.add(xb)
    D, I = memo.search(index, xq, k, f"ladder {MNAME[metric]} {engine} k={k}")
    bad = _strict(memo, "ladder", metric, D, I, k=k)
    assert not bad, (metric, engine, k, len(bad), bad[:5])


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("metric", METRICS)
def test_ladder_wide_rows(memo, vf, metric, engine):
    """d = 1024 with norms over four decades: by l2aug_params' formula the L2
    augmentation's extra block reaches its cap of 128 columns."""
    n, d, nq, k, _ = FAMILY_WIDE
    xb, xq = memo.rows("ladder", FAMILY_WIDE)
    index = vf.IndexFlat(d, metric)
    index.set_engine(engine)
    index.add(xb)
    D, I = memo.search(index, xq, k, f"ladder {MNAME[metric]} {engine} k={k} d={d} n={n}")
    bad = _strict(memo, "ladder", metric, D, I, k=k, shape=FAMILY_WIDE)
    assert not bad, (metric, engine, len(bad), bad[:5])


@pytest.mark.parametrize("engine", ENGINES)
def test_zero_rows_tie_as_every_l2_querys_nearest(memo, engine):
    """Under L2 the three zero rows are every query's three nearest (the oracle
    says so first) at the same distance |q|^2: exact ties, in label order."""
    zr = np.array(zero_rows(N))
    _, Ir = memo.ref("zeros", L2)
    assert (np.sort(Ir[:, :3], axis=1) == zr).all()
    D, I = memo.run("zeros", L2, engine)
    assert (I[:, :3] == zr).all(), I[(I[:, :3] != zr).any(axis=1)][:5]
    assert (D[:, 0] == D[:, 1]).all() and (D[:, 1] == D[:, 2]).all()
    zq = list(ZERO_QUERIES)
    assert (D[zq, :3] == 0).all()


@pytest.mark.parametrize("engine", ENGINES)
def test_zero_queries_ip_follow_the_faiss_tie_rule(memo, engine):
    """For an all-zero query every inner product is exactly 0: D == 0 and the
    labels are those of faiss's heap (cfaiss.knn_seq), as
    test_ties_match_faiss_heap promises for the staged engine."""
    xb, xq = memo.rows("zeros")
    zq = list(ZERO_QUERIES)
    assert not xq[zq].any()
    D, I = memo.run("zeros", IP, engine)
    assert (D[zq] == 0).all(), D[zq]
    Dc, Ic = cfaiss.knn_seq(xb, xq[zq], K, IP)
    np.testing.assert_array_equal(I[zq], Ic)
    np.testing.assert_array_equal(D[zq], Dc)


JOIN_CASES = [(IP, "i8v"), (IP, "bf16v"), (L2, "auto")]  # an L2 index joins on its bf16 plane


@pytest.mark.parametrize("name", ROW_FAMILIES)
@pytest.mark.parametrize("metric,engine", JOIN_CASES)
def test_selfjoin_matrix(memo, metric, engine, name):
    """Cosine self-join of the first 300 stored rows against pgvector's rule,
    strictly, on every row."""
    xb, _ = memo.rows(name)
    S, I = memo.join(name, metric, engine)
    Sr, Ir = memo.join_ref(name)
    bad = flat.selfjoin_mismatches(S, I, Sr, Ir, xb, np.arange(FAMILY_JOIN_ROWS), strict=True)
    assert not bad, (name, metric, engine, len(bad), bad[:5])
    if name == "zeros":  # a zero row has no neighbours and is nobody's neighbour
        zr = zero_rows(N)
        assert (Ir[0] == -1).all()
        assert (I[0] == -1).all(), I[0]
        assert not np.isin(I, zr).any()
        assert (I[1:] >= 0).all()


@pytest.mark.parametrize("e", [-40, 40])
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("metric", METRICS)
def test_scale_invariance_search(memo, metric, engine, e):
    """Rows and queries scaled by 2^e: every score scales by 2^(2e) exactly.
    Each emitted key is one rounding of an exact sum (§4.2) and nothing under-
    or overflows at e = +-40, so the labels are those of e = 0 and D is
    ldexp(D0, 2e) bit for bit."""
    D0, I0 = memo.run("pow2:0", metric, engine)
    D, I = memo.run(f"pow2:{e}", metric, engine)
    np.testing.assert_array_equal(I, I0)
    want = np.ldexp(D0, 2 * e)
    assert want.dtype == np.float32 and np.isfinite(want).all() and (want != 0).all()
    np.testing.assert_array_equal(D, want)


@pytest.mark.parametrize("e", [-40, 40])
@pytest.mark.parametrize("metric,engine", JOIN_CASES)
def test_scale_invariance_selfjoin(memo, metric, engine, e):
    """The cosine does not scale: similarities and labels equal those of e = 0
    bit for bit."""
    S0, I0 = memo.join("pow2:0", metric, engine)
    S, I = memo.join(f"pow2:{e}", metric, engine)
    np.testing.assert_array_equal(I, I0)
    np.testing.assert_array_equal(S, S0)


# pow2:-40 is left out: every score there is ~2^-80 d, far below the fp32
# contract's absolute floor of 1e-5, so that check would accept any answer.
FP32_FAMILIES = [f for f in ROW_FAMILIES if f != "pow2:-40"]


@pytest.mark.parametrize("name", FP32_FAMILIES)
@pytest.mark.parametrize("metric", METRICS)
def test_fp32_accumulating_routes(memo, vf, metric, name):
    """The same families through the routes that accumulate in fp32: the fp32
    MFMA engine at nq = 100 and the small calls (nq = 1: GEMV, nq = 20: skinny),
    at the fp32 contract (strict=False)."""
    xb, xq = memo.rows(name)
    Dr, Ir = memo.ref(name, metric)
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    for nq in (1, 20):
        D, I = index.search(xq[:nq], K)
        bad = flat.mismatches(D, I, Dr[:nq], Ir[:nq], metric, xb, xq[:nq])
        assert not bad, (name, metric, nq, len(bad), bad[:5])
    index.set_engine("fp32")
    D, I = index.search(xq, K)
    bad = flat.mismatches(D, I, Dr, Ir, metric, xb, xq)
    assert not bad, (name, metric, "fp32", len(bad), bad[:5])
