"""GPU: range searches, range self-joins and the gathered / paged exact kernels
on the row families that stress data-dependent bounds.

The range search and the range self-join preselect candidates with an fp32 or
bf16 MFMA GEMM and widen the radius by a bound (vs_api_range.hip run_range:
bound_key / qbound_kernel with rows_exact, range_thr_kernel) whose inputs are
the largest stored norm (a plane's maxima, range_norm_max_kernel without a
plane, the augmented int8 maxima of an L2 index that kept only that plane), the
query's norm and ld.  A bound that is too small does not crash: it leaves a
true hit out of lims.  On rows of one scale the bound is never the deciding
term; here every family of helpers.row_family goes through the range contract
(helpers.range_contract) against the fp64 oracle: every pair farther than its
rounding window from the radius is classified as its fp64 score says, D is the
once-rounded exact key of its label, and the pairs inside the window are
counted against helpers.range_cap of the oracle's own hit count.
tests/test_row_families_host.py admits every case from the oracle alone.

The gathered selector kernels (gemm_topk_rows, gemv_topk_rows) and the paged
exact engine past the staged engine's k see the same families at the fp32
contract (flat.mismatches / flat.mismatches_vec, non-strict).

Inputs, references and indexes are computed once per module (_Memo) and never
modified.  Every contract prints its hits / undecided line; they are recorded
in profiles/range_families/gpu_tests_tail.txt and not asserted beyond the cap."""

import numpy as np
import pytest

from helpers import (BAND_BASE, BAND_RADIUS, BAND_ROWS, FAMILY_JOIN_ROWS, FAMILY_SHAPE,
                     JOIN_QUANTILES, RANGE_NQ, RANGE_QUANTILES, ROW_FAMILIES, ZERO_QUERIES,
                     bound_band_case, family_case, family_half_mask, family_tombstones,
                     join_reference, join_threshold, join_valid, plant_unselected, range_contract,
                     range_radius, range_reference, zero_rows)
from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
METRICS = [IP, L2]
N, DIM, NQ, K, SEED = FAMILY_SHAPE
N1 = N - N // 10  # the first add of "late"
MNAME = {IP: "IP", L2: "L2"}
ROUND = {"f32": lambda x: x, "bf16": flat.round_bf16}


@pytest.fixture(scope="module")
def vf():
    from vsearch import _lib
    from vsearch import faiss as vfaiss

    assert _lib.device_count() >= 1, "gpu tests need a visible MI355X"
    return vfaiss


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


class _Memo:
    """Inputs, oracle references and indexes, each computed once per module and
    never modified (arrays are handed out read-only)."""

    def __init__(self, vf):
        self.vf = vf
        self._rows, self._ref, self._join_ref, self._index = {}, {}, {}, {}

    def rows(self, name, dtype="f32"):
        """(xb, xq) as the index of that storage holds them."""
        key = (name, dtype)
        if key not in self._rows:
            xb, xq = family_case(name, N, DIM, NQ, SEED)
            self._rows[key] = _frozen(ROUND[dtype](xb), ROUND[dtype](xq))
        return self._rows[key]

    def ref(self, name, metric, dtype="f32", nrows=None):
        """(s, w) of the 100 queries over the first nrows rows."""
        key = (name, metric, dtype, nrows)
        if key not in self._ref:
            xb, xq = self.rows(name, dtype)
            self._ref[key] = _frozen(*range_reference(xb[:nrows], xq, metric))
        return self._ref[key]

    def join_ref(self, name, dtype="f32", nrows=None):
        """(s, w) of the cosines of the first FAMILY_JOIN_ROWS rows."""
        key = (name, dtype, nrows)
        if key not in self._join_ref:
            xb, _ = self.rows(name, dtype)
            self._join_ref[key] = _frozen(*join_reference(xb[:nrows], FAMILY_JOIN_ROWS))
        return self._join_ref[key]

    def check_searches(self, index, name, metric, dtype, nrows, tag, quantiles=RANGE_QUANTILES,
                       **kw):
        """The range contract at every batch size and quantile."""
        _, xq = self.rows(name)
        s100, w100 = self.ref(name, metric, dtype, nrows)
        for nq in RANGE_NQ:
            s, w = s100[:nq], w100[:nq]
            for quantile in quantiles:
                radius = range_radius(s, metric, quantile)
                range_contract(index.range_search(xq[:nq], radius, **kw), s, w, radius, metric,
                               tag=f"{tag} nq={nq} q={quantile}")

    def check_joins(self, index, name, dtype, nrows, tag):
        s, w = self.join_ref(name, dtype, nrows)
        n = s.shape[1]
        for quantile in JOIN_QUANTILES:
            t = join_threshold(s, quantile)
            for upper in (False, True):
                res = index.range_selfjoin(t, q0=0, nq=FAMILY_JOIN_ROWS, upper=upper)
                range_contract(res, s, w, t, "cosine",
                               valid=join_valid(FAMILY_JOIN_ROWS, n, upper=upper),
                               tag=f"{tag} join q={quantile} upper={upper}")

    def build(self, name, metric, dtype="f32"):
        """A fresh index of the family; "late" in two adds (nine tenths, then the
        100x tenth: the index maxima have to grow), with the contract checked
        after the first add on the way (searches, and the join for an inner-
        product index)."""
        xb, _ = self.rows(name)  # a bf16 index rounds what it is given itself
        index = self.vf.IndexFlat(DIM, metric, dtype=dtype)
        if name == "late":
            index.add(xb[:N1])
            tag = f"late[:{N1}] {MNAME[metric]} {dtype}"
            self.check_searches(index, name, metric, dtype, N1, tag)
            if metric == IP:
                self.check_joins(index, name, dtype, N1, tag)
            index.add(xb[N1:])
        else:
            index.add(xb)
        assert index.ntotal == N
        return index

    def index(self, name, metric, dtype="f32"):
        """One index per (family, metric, storage), created with the default
        planes."""
        key = (name, metric, dtype)
        if key not in self._index:
            index = self.build(name, metric, dtype)
            if dtype == "f32":
                assert index.filter_planes == ("i8", "bf16")
            self._index[key] = index
        return self._index[key]


@pytest.fixture(scope="module")
def memo(vf):
    return _Memo(vf)


def _search_case(memo, index, name, metric, dtype, nq, quantile, tag="", **kw):
    """One range search of the first nq queries at their own radius, through
    the contract; returns (result, radius)."""
    _, xq = memo.rows(name)
    s100, w100 = memo.ref(name, metric, dtype)
    s, w = s100[:nq], w100[:nq]
    radius = range_radius(s, metric, quantile)
    res = index.range_search(xq[:nq], radius, **kw)
    range_contract(res, s, w, radius, metric,
                   tag=f"{name} {MNAME[metric]} {dtype}{tag} nq={nq} q={quantile}")
    return res, radius


def _same(a, b):
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert u.tobytes() == v.tobytes()


# ---- the search matrix ----------------------------------------------------------------------------
@pytest.mark.parametrize("quantile", RANGE_QUANTILES)
@pytest.mark.parametrize("nq", RANGE_NQ)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ROW_FAMILIES)
def test_search_matrix(memo, name, metric, nq, quantile):
    """Every family, both metrics; 100 queries (faiss's BLAS L2 key) and the
    first 19 with their own radius (the sequential key, MODE_L2D); radii that
    take in 0.1 %, 1 % and 20 % of the pairs."""
    _search_case(memo, memo.index(name, metric), name, metric, "f32", nq, quantile)


@pytest.mark.parametrize("metric", METRICS)
def test_late_rows_by_update_equal_two_adds(memo, vf, metric):
    """The 100x rows written over the last tenth of "pow2:0" by index.update
    (the base rows of both families are the same draw): the result is that of
    the index built in two adds, byte for byte.  A condition of the contract
    (the exact key decides, whatever the maxima's history), not parity
    evidence: the two-add index is checked against the oracle by the matrix."""
    x0, _ = memo.rows("pow2:0")
    xl, xq = memo.rows("late")
    assert x0[:N1].tobytes() == xl[:N1].tobytes()
    index = vf.IndexFlat(DIM, metric)
    index.add(x0)
    index.update(np.arange(N1, N, dtype=np.int64), xl[N1:])
    assert index.reconstruct_n(0, N).tobytes() == xl.tobytes()
    two = memo.index("late", metric)
    for nq in RANGE_NQ:
        res, radius = _search_case(memo, index, "late", metric, "f32", nq, 0.01, tag=" update")
        _same(res, two.range_search(xq[:nq], radius))


# ---- planes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder", "late"])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("filt,planes", [("i8", ("i8",)), ("none", ())])
def test_planes(memo, monkeypatch, filt, planes, metric, name):
    """VS_FILTER=i8: the bound takes the int8 plane's maxima (an L2 index's are
    those of the augmented rows); none: range_norm_max_kernel over the stored
    norms.  "late" in two adds, checked after each."""
    monkeypatch.setenv("VS_FILTER", filt)
    index = memo.build(name, metric)
    assert index.filter_planes == planes and index.notice == ""
    memo.check_searches(index, name, metric, "f32", None, f"{name} {MNAME[metric]} planes={filt}",
                        quantiles=(0.01,))


# ---- bf16 indexes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", RANGE_NQ)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["ladder", "offset", "late"])
def test_bf16_index(memo, name, metric, nq):
    """Rows and queries rounded to bf16; the exact key is over the stored values
    and the bound's maximum comes from range_norm_max_kernel."""
    _search_case(memo, memo.index(name, metric, "bf16"), name, metric, "bf16", nq, 0.01)


def test_bf16_tombstones(memo, vf):
    """50 planted copies of queries, removed: a bf16 index keeps them in place
    as tombstones; they are never a hit and labels are positions among the live
    rows."""
    xb, xq = memo.rows("ladder")
    planted, ids, live = family_tombstones(xb, xq)
    index = vf.IndexFlat(DIM, L2, dtype="bf16")
    index.add(planted)
    assert index.remove_ids(ids) == 50 and index.ntotal == N - 50
    s, w = range_reference(flat.round_bf16(live), flat.round_bf16(xq), L2)
    radius = range_radius(s, L2, 0.01)
    range_contract(index.range_search(xq, radius), s, w, radius, L2, tag="ladder L2 bf16 tombstones")


# ---- selector -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", RANGE_NQ)
@pytest.mark.parametrize("metric", METRICS)
def test_selected_half(memo, vf, metric, nq):
    mask = family_half_mask(N)
    _, xq = memo.rows("ladder")
    s100, w100 = memo.ref("ladder", metric)
    s, w = s100[:nq], w100[:nq]
    radius = range_radius(s, metric, 0.01)
    sel = vf.IDSelectorBitmap(N, np.packbits(mask, bitorder="little"))
    res = memo.index("ladder", metric).range_search(xq[:nq], radius,
                                                    params=vf.SearchParameters(sel=sel))
    hits, _ = range_contract(res, s, w, radius, metric, valid=mask[None, :],
                             tag=f"ladder {MNAME[metric]} half nq={nq}")
    assert hits > 0 and mask[res[2]].all()


# ---- scale invariance -----------------------------------------------------------------------------
@pytest.mark.parametrize("nq", RANGE_NQ)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("e", [-40, 40])
def test_scale_invariance_search(memo, e, metric, nq):
    """Rows, queries and radius scaled by powers of two: every emitted key is one
    rounding of an exact sum and the exact key decides, so lims and I are those
    of e = 0 and D is ldexp(D0, 2e) bit for bit.  A condition of the contract,
    not parity evidence (the matrix checks both families against the oracle)."""
    _, x0 = memo.rows("pow2:0")
    _, xe = memo.rows(f"pow2:{e}")
    s, _ = memo.ref("pow2:0", metric)
    for quantile in RANGE_QUANTILES:
        r0 = range_radius(s[:nq], metric, quantile)
        re = np.ldexp(r0, 2 * e)
        assert re.dtype == np.float32 and np.isfinite(re) and re != 0
        lims0, D0, I0 = memo.index("pow2:0", metric).range_search(x0[:nq], r0)
        lims, D, I = memo.index(f"pow2:{e}", metric).range_search(xe[:nq], re)
        want = np.ldexp(D0, 2 * e)
        assert want.dtype == np.float32 and np.isfinite(want).all() and (want != 0).all()
        assert len(D0) > 0
        np.testing.assert_array_equal(lims, lims0)
        np.testing.assert_array_equal(I, I0)
        assert D.tobytes() == want.tobytes()


# ---- zeros ----------------------------------------------------------------------------------------
def test_zero_queries_inner_product(memo):
    """Every inner product of a zero query is exactly 0: nothing is > 0, and
    every one of the 6000 rows is > -1e-30 (a full-row segment) with D == 0."""
    _, xq = memo.rows("zeros")
    zq = list(ZERO_QUERIES)
    assert not xq[zq].any()
    index = memo.index("zeros", IP)
    lims, D, I = index.range_search(xq[zq], 0.0)
    assert lims.tolist() == [0, 0, 0] and len(D) == 0 and len(I) == 0
    lims, D, I = index.range_search(xq[zq], -np.float32(1e-30))
    assert lims.tolist() == [0, N, 2 * N]
    np.testing.assert_array_equal(I, np.tile(np.arange(N), 2))
    assert (D == 0).all()


def test_zero_queries_l2(memo):
    """A zero query's distance to a zero row is exactly 0 and to any other row
    |x|^2 > 0: at the smallest positive radius it hits exactly the three zero
    rows, with D == 0, alone (the sequential key) and inside the whole batch
    (the BLAS key), where no other query has a hit."""
    xb, xq = memo.rows("zeros")
    zq = list(ZERO_QUERIES)
    zr = list(zero_rows(N))
    radius = np.nextafter(np.float32(0), np.float32(1))
    assert radius > 0
    s, _ = memo.ref("zeros", L2)
    assert int((s < float(radius)).sum()) == 6 and (s[zq][:, zr] == 0).all()
    index = memo.index("zeros", L2)
    lims, D, I = index.range_search(xq[zq], radius)
    assert lims.tolist() == [0, 3, 6]
    assert I.tolist() == zr + zr and (D == 0).all()
    lims, D, I = index.range_search(xq, radius)
    per_query = np.diff(lims.astype(np.int64))
    want = np.zeros(NQ, dtype=np.int64)
    want[zq] = 3
    np.testing.assert_array_equal(per_query, want)
    assert I.tolist() == zr + zr and (D == 0).all()


# ---- the join matrix ------------------------------------------------------------------------------
JOIN_STORAGE = [(name, "f32") for name in ROW_FAMILIES] + [(name, "bf16")
                                                           for name in ("ladder", "offset", "late")]


@pytest.mark.parametrize("quantile", JOIN_QUANTILES)
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("name,dtype", JOIN_STORAGE)
def test_join_matrix(memo, name, dtype, upper, quantile):
    """The cosine range self-join of the first 300 stored rows of an inner-
    product index, thresholds at cosine quantiles of those rows' pairs."""
    s, w = memo.join_ref(name, dtype)
    t = join_threshold(s, quantile)
    index = memo.index(name, IP, dtype)
    res = index.range_selfjoin(t, q0=0, nq=FAMILY_JOIN_ROWS, upper=upper)
    range_contract(res, s, w, t, "cosine", valid=join_valid(FAMILY_JOIN_ROWS, N, upper=upper),
                   tag=f"{name} {dtype} join q={quantile} upper={upper}")
    if name == "zeros":  # a zero row has an empty range and is in nobody's
        lims, _, I = res
        assert lims[0] == lims[1] == 0
        assert not np.isin(I, zero_rows(N)).any()
        assert np.isnan(s[0]).all()


@pytest.mark.parametrize("quantile", JOIN_QUANTILES)
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("e", [-40, 40])
def test_scale_invariance_join(memo, e, upper, quantile):
    """The cosine does not scale: lims, S and I are those of e = 0 byte for
    byte at the same threshold.  A condition of the contract, not parity
    evidence."""
    s, _ = memo.join_ref("pow2:0")
    t = join_threshold(s, quantile)
    base = memo.index("pow2:0", IP).range_selfjoin(t, q0=0, nq=FAMILY_JOIN_ROWS, upper=upper)
    res = memo.index(f"pow2:{e}", IP).range_selfjoin(t, q0=0, nq=FAMILY_JOIN_ROWS, upper=upper)
    assert len(base[1]) > 0
    _same(res, base)


# ---- gathered and paged kernels -------------------------------------------------------------------
# pow2:-40 is left out: every score there is ~2^-80 d, far below the fp32
# contract's absolute floor of 1e-5, so that check would accept any answer.
FP32_FAMILIES = [f for f in ROW_FAMILIES if f != "pow2:-40"]


@pytest.mark.parametrize("nq,kernel", [(1, "gemv_topk_rows"), (40, "gemm_topk_rows")])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", FP32_FAMILIES)
def test_gathered_selector_kernels(memo, vf, name, metric, nq, kernel):
    """A random half selected, copies of the queries planted in unselected rows
    (the unfiltered nearest rows lie outside the selection), through the
    streaming (nq = 1) and the MFMA (nq = 40) gathered kernel, against the
    masked oracle at the fp32 contract; every label inside the mask."""
    from vsearch import _lib

    xb0, xq100 = memo.rows(name)
    xq = xq100[:nq]
    mask = family_half_mask(N)
    xb = plant_unselected(xb0, xq, mask)
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    sel = index.selector(vf.IDSelectorBitmap(N, np.packbits(mask, bitorder="little")))
    assert sel.count == int(mask.sum())
    D, I = index.search(xq, K, params=vf.SearchParameters(sel=sel))
    assert _lib.timer_kernel() == kernel
    Dr, Ir = flat.select_topk(flat.exact_scores(xb, xq, metric), K, metric,
                              valid=mask[None, :].repeat(nq, 0))
    assert (I >= 0).all() and mask[I].all(), "a label outside the selection"
    bad = flat.mismatches(D, I, Dr, Ir, metric, xb, xq)
    assert not bad, (name, metric, nq, len(bad), bad[:5])


# "late" under inner product is left out: past the ~300 late rows with large
# positive scores, a query's ranks up to 600 are late rows (|x| ~ 1000) whose
# products with the query (|q| ~ 10) cancel to scores of 10 to 30, and the fp32
# contract's tolerance for an inner product is 1e-5 |s| with no norm term.  Any
# fp32 accumulation of 100 products misses it there (numpy's sgemm does on 19
# of those entries, by up to 1.9 tolerances; the paged engine on 14, all "score",
# and set_engine("fp32") returns the same bytes): a limit of the fp32 contract on
# that family, not of the paged engine.  Its L2 case stays (the L2 tolerance
# scales with |q|^2 + |x|^2).
PAGED_CASES = ([(name, IP, 600) for name in ("ladder", "spike", "offset")] +
               [(name, L2, 1100) for name in ("ladder", "spike", "offset", "late")])


@pytest.mark.parametrize("name,metric,k", PAGED_CASES)
def test_paged_exact_engine(memo, name, metric, k):
    """k past the staged engine's lists: the paged exact engine pages through
    each query's order 64 entries at a time."""
    xb, xq = memo.rows(name)
    D, I = memo.index(name, metric).search(xq, k)
    assert D.shape == (NQ, k)
    Dr, Ir = flat.knn_exact(xb, xq, k, metric)
    bad = flat.mismatches_vec(D, I, Dr, Ir, metric, xb, xq)
    assert not bad, (name, metric, k, len(bad), bad[:5])


# ---- a case the bound decides ---------------------------------------------------------------------
@pytest.mark.parametrize("how", ["planes", "i8", "none", "update"])
def test_bound_decides_band(vf, monkeypatch, how):
    """helpers.bound_band_case: 1600 rows of norm ~1000, after 2000 of norm
    ~0.01, whose inner products with their query scatter about the radius by
    less than the candidate GEMM's own error on them: the GEMM alone drops a
    good part of the ~800 hits, so they are all there only if the bound took
    the large rows' norm, from the planes' maxima grown by the second add
    ("planes", "i8"), from range_norm_max_kernel ("none") or from the maxima
    grown by index.update ("update": the large rows written over small ones).
    Against the fp64 oracle, as every other case."""
    if how in ("i8", "none"):
        monkeypatch.setenv("VS_FILTER", how)
    base, band, xq = bound_band_case()
    xb = np.concatenate([base, band])
    index = vf.IndexFlat(DIM, IP)
    index.add(base)
    if how == "update":
        index.add(base[:BAND_ROWS])
        index.update(np.arange(BAND_BASE, BAND_BASE + BAND_ROWS, dtype=np.int64), band)
    else:
        index.add(band)
    assert index.filter_planes == {"i8": ("i8",), "none": ()}.get(how, ("i8", "bf16"))
    assert index.reconstruct_n(0, len(xb)).tobytes() == xb.tobytes()
    s, w = range_reference(xb, xq, IP)
    hits, _ = range_contract(index.range_search(xq, BAND_RADIUS), s, w, BAND_RADIUS, IP,
                             tag=f"band {how}")
    assert hits > 70000
