"""Test doubles built on the CPU oracle (test infrastructure only).

OracleIndex implements the faiss-index surface that the host logic (LangChain
store, persistence, sharding) uses, with the oracle as its arithmetic, so the
host logic is testable on CPU.  It is never used by product code."""

from __future__ import annotations

import numpy as np

from oracle import flat


class OracleIndex:
    is_trained = True

    def __init__(self, d: int, metric: int = flat.METRIC_L2):
        self.d = int(d)
        self.metric_type = int(metric)
        self._x = np.zeros((0, self.d), dtype=np.float32)
        self._base = 0
        self.device = 0

    @property
    def ntotal(self) -> int:
        return self._x.shape[0]

    def add(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.shape[1] == self.d
        self._x = np.concatenate([self._x, x])

    def search(self, x, k, raw=False):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.shape[1] == self.d
        assert k > 0
        if raw:  # VS_RAW_ORDER: lexicographic (key, label), no IP tie rule
            D, I = flat.knn_lex(self._x, x, k, self.metric_type)
        else:
            D, I = flat.knn_exact(self._x, x, k, self.metric_type)
        I = np.where(I >= 0, I + self._base, -1)
        return D, I

    def reconstruct(self, i):
        if not 0 <= i < self.ntotal:
            raise RuntimeError("key out of range")
        return self._x[i].copy()

    def reconstruct_n(self, n0=0, ni=-1):
        if ni == -1:
            ni = self.ntotal - n0
        return self._x[n0:n0 + ni].copy()

    def remove_ids(self, ids):
        ids = np.asarray(ids, dtype=np.int64) - self._base
        self._x, n = flat.remove_ids(self._x, ids)
        return n

    def set_id_base(self, base):
        self._base = int(base)

    def reset(self):
        self._x = np.zeros((0, self.d), dtype=np.float32)


def oracle_merge(Dall, Iall, metric, k):
    """Merge gathered shard lists [G][nq][k_in] with the oracle's tie rule."""
    G, nq, kin = Dall.shape
    D = np.full((nq, k), flat.neutral(metric), dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        s = Dall[:, q, :].ravel()
        ids = Iall[:, q, :].ravel()
        keep = ids >= 0
        s, ids = s[keep], ids[keep]
        if ids.size == 0:
            continue
        key = s if metric == flat.METRIC_L2 else -s
        sel = flat.faiss_order(ids, key, k, metric)
        pos = {int(i): j for j, i in enumerate(ids)}
        D[q, :sel.size] = [s[pos[int(i)]] for i in sel]
        I[q, :sel.size] = sel
    return D, I


def assert_against_candidates(D, I, cand, metric, k, d, strict):
    """One query's result (D, I) against its proven candidate set cand =
    (ids, fp64 scores, fp64 |x|^2, |q|^2): a set that provably holds the exact
    top-k (every other row strictly worse).  Every returned label must be a
    candidate, D[j] within the window of ITS OWN exact score, and a label that
    differs from the oracle's j-th only inside both windows (a tie).  Window:
    strict = the rounding of an exactly rescored key (flat.key_window), else the
    north star's fp32 contract (flat.score_tolerance)."""
    ids, exact, xn2, qn2 = cand
    pos = {int(i): j for j, i in enumerate(ids)}
    key = exact if metric == flat.METRIC_L2 else -exact
    ref_i = flat.faiss_order(np.asarray(ids, dtype=np.int64), key, k, metric)
    assert len(set(np.asarray(I).tolist())) == k

    def window(r):
        p = pos[int(r)]
        if strict:
            return float(flat.key_window(metric, exact[p], qn2, xn2[p], d))
        return float(flat.score_tolerance(metric, exact[p], qn2, xn2[p]))

    for j in range(k):
        assert int(I[j]) in pos, (j, int(I[j]), "not among the proven candidates")
        s_got = exact[pos[int(I[j])]]
        assert abs(float(D[j]) - s_got) <= window(I[j]), (j, int(I[j]), float(D[j]), s_got,
                                                          window(I[j]))
        if I[j] != ref_i[j]:
            s_ref = exact[pos[int(ref_i[j])]]
            assert abs(s_got - s_ref) <= window(I[j]) + window(ref_i[j]), (
                j, int(I[j]), int(ref_i[j]), s_got, s_ref)


def proven_candidates(index, xs, metric, N, K, m=64, chunk=1_000_000):
    """Per query of xs: the m best of the index's N rows (read back in chunks by
    reconstruct_n, bit-exact) by fp32 sgemm, with their fp64 exact scores and
    norms.  The margin between the K-th and the m-th sgemm score is checked
    against the worst-case fp32 sgemm error (gamma(d) |q| max|x|), so the set
    provably holds the exact top-K.  Returns (ids, exact, |x|^2, |q|^2) per
    query (the form assert_against_candidates takes)."""
    D_ = xs.shape[1]
    nq = xs.shape[0]
    best_s = np.full((nq, 0), -np.inf, np.float32)
    best_i = np.zeros((nq, 0), np.int64)
    xmax = 0.0
    rows = {}
    for r0 in range(0, N, chunk):
        xb = index.reconstruct_n(r0, min(chunk, N - r0))
        xmax = max(xmax, float(np.sqrt(np.einsum("ij,ij->i", xb, xb, dtype=np.float64).max())))
        s = xs @ xb.T  # fp32 sgemm
        if metric == flat.METRIC_L2:  # larger = better: 2 q.x - |x|^2 (|q|^2 is constant)
            s = 2.0 * s - np.einsum("ij,ij->i", xb, xb, dtype=np.float64)[None, :]
        s = np.asarray(s, np.float32)
        allv = np.concatenate([best_s, s], axis=1)
        alli = np.concatenate([best_i, np.broadcast_to(np.arange(r0, r0 + xb.shape[0]), s.shape)],
                              axis=1)
        part = np.argpartition(-allv, m - 1, axis=1)[:, :m]
        best_s = np.take_along_axis(allv, part, axis=1)
        best_i = np.take_along_axis(alli, part, axis=1)
        for q in range(nq):  # keep the candidate rows for the exact rescoring
            for r in best_i[q]:
                if r0 <= r < r0 + xb.shape[0]:
                    rows[int(r)] = xb[r - r0].copy()
    res = []
    u = 2.0 ** -24
    gam = D_ * u / (1 - D_ * u)
    for q in range(nq):
        ids = best_i[q]
        order = np.argsort(-best_s[q], kind="stable")
        s_sorted = best_s[q][order]
        qn = float(np.sqrt(np.dot(xs[q].astype(np.float64), xs[q].astype(np.float64))))
        bound = 2.0 * gam * qn * xmax * (2.0 if metric == flat.METRIC_L2 else 1.0) + 1e-3
        # fp32 preselection can only be wrong inside this margin
        assert s_sorted[K - 1] - s_sorted[m - 1] > 2 * bound, (q, s_sorted[K - 1], s_sorted[-1])
        xb = np.stack([rows[int(r)] for r in ids])
        exact = flat.exact_scores(xb, xs[q:q + 1], metric)[0]
        xn2 = np.einsum("ij,ij->i", xb.astype(np.float64), xb.astype(np.float64))
        res.append((ids, exact, xn2, qn * qn))
    return res


# Row families that stress the staged engine's data-dependent bounds (DESIGN.md
# §4.3): per-row int8 scales, residual norms, the index maxima, the L2
# augmentation and the absolute constants.  Every value is finite.
ROW_FAMILIES = ("ladder", "spike", "offset", "sparse", "zeros", "late",
                "pow2:-40", "pow2:0", "pow2:40")
# The shapes tests/test_gpu_row_families.py searches and
# tests/test_row_families_host.py admits: (n, d, nq, k, seed).  d = 100 pads to
# ld = 128, nq = 100 is one full and one ragged query tile; FAMILY_WIDE is the
# ladder at ld = 1024, where l2aug_params' cap lets m reach 128.
FAMILY_SHAPE = (6000, 100, 100, 10, 7)
FAMILY_WIDE = (3000, 1024, 100, 10, 7)
FAMILY_JOIN_ROWS = 300  # stored rows the cosine self-joins query
FAMILY_WIDEST_K = {0: 28, 1: 56}  # metric -> the widest list the staged engine takes
ZERO_QUERIES = (5, 70)  # queries the "zeros" searches also set to zero


def zero_rows(n):
    """The rows row_family("zeros", n, ...) sets to zero."""
    return (0, n // 2, n - 1)


def family_case(name, n, d, nq, seed):
    """row_family as the searches use it: the "zeros" batch also has its
    ZERO_QUERIES set to zero."""
    xb, xq = row_family(name, n, d, nq, seed)
    if name == "zeros":
        xq[[q for q in ZERO_QUERIES if q < nq]] = 0.0
    return xb, xq


def family_skip(name, n):
    """(rows, queries) free_share leaves out for a family: the zero rows and
    zero queries of "zeros" (checked on their own), nothing otherwise."""
    return (zero_rows(n), ZERO_QUERIES) if name == "zeros" else None


def row_family(name, n, d, nq, seed):
    """Deterministic (xb (n, d), xq (nq, d)) float32 rows of one family, drawn
    with g(m) = rng.standard_normal((m, d)) on one default_rng(seed):
      ladder   g * 10**U(-2, 2) per row and per query: norms log-uniform over
               four decades;
      spike    one coordinate per row and per query (random position) times 64;
      offset   mu + g, mu = 8 sign(g(1)) shared by rows and queries;
      sparse   rows of four non-zero standard-normal entries at random
               positions, dense queries;
      zeros    g with rows 0, n // 2, n - 1 set to zero;
      late     g with the last n // 10 rows times 100;
      pow2:e   ldexp(g, e) for rows and queries."""
    rng = np.random.default_rng(seed)

    def g(m):
        return rng.standard_normal((m, d))

    if name == "ladder":
        xb = g(n) * 10.0 ** rng.uniform(-2, 2, (n, 1))
        xq = g(nq) * 10.0 ** rng.uniform(-2, 2, (nq, 1))
    elif name == "spike":
        xb, xq = g(n), g(nq)
        xb[np.arange(n), rng.integers(0, d, n)] *= 64.0
        xq[np.arange(nq), rng.integers(0, d, nq)] *= 64.0
    elif name == "offset":
        mu = 8.0 * np.sign(g(1))
        xb, xq = mu + g(n), mu + g(nq)
    elif name == "sparse":
        xb = np.zeros((n, d))
        for i in range(n):
            xb[i, rng.choice(d, 4, replace=False)] = rng.standard_normal(4)
        xq = g(nq)
    elif name == "zeros":
        xb, xq = g(n), g(nq)
        xb[[0, n // 2, n - 1]] = 0.0
    elif name == "late":
        xb, xq = g(n), g(nq)
        xb[n - n // 10:] *= 100.0
    elif name.startswith("pow2:"):
        e = int(name[5:])
        xb, xq = np.ldexp(g(n), e), np.ldexp(g(nq), e)
    else:
        raise ValueError(name)
    return xb.astype(np.float32), xq.astype(np.float32)


def _share(sorted_scores, windows, k):
    """Share of (query, rank j < k) positions whose j-th and (j+1)-th sorted
    scores lie within the sum of their two windows."""
    gap = np.abs(sorted_scores[:, 1:k + 1] - sorted_scores[:, :k])
    free = gap <= windows[:, 1:k + 1] + windows[:, :k]
    return float(free.mean()) if free.size else 0.0


def free_share(xb, xq, metric, k, skip=None):
    """From the oracle alone: the share of (query, rank j < k) positions where
    the oracle's j-th and (j+1)-th scores lie within the sum of their two
    strict windows (flat.key_window), i.e. where flat.mismatches(strict=True)
    would accept either label.  skip = (rows, queries) left out of the count."""
    xb = np.asarray(xb, dtype=np.float32)
    xq = np.asarray(xq, dtype=np.float32)
    rows, queries = skip if skip is not None else ((), ())
    keep_r = np.setdiff1d(np.arange(xb.shape[0]), np.asarray(rows, dtype=np.int64))
    keep_q = np.setdiff1d(np.arange(xq.shape[0]), np.asarray(queries, dtype=np.int64))
    xb, xq = xb[keep_r], xq[keep_q]
    s = flat.exact_scores(xb, xq, metric)
    xn2 = np.einsum("ij,ij->i", xb.astype(np.float64), xb.astype(np.float64))
    qn2 = np.einsum("ij,ij->i", xq.astype(np.float64), xq.astype(np.float64))
    w = flat.key_window(metric, s, qn2[:, None], xn2[None, :], xb.shape[1])
    key = s if metric == flat.METRIC_L2 else -s
    order = np.argsort(key, axis=1, kind="stable")[:, :k + 1]
    return _share(np.take_along_axis(s, order, axis=1), np.take_along_axis(w, order, axis=1), k)


def free_share_cosine(x, k, q_rows, skip=None):
    """free_share for the cosine self-join of stored rows q_rows of x (self
    excluded, zero-norm rows never match): windows from
    flat.key_window(..., cosine=True).  skip = rows left out, as rows and as
    queries."""
    x64 = np.asarray(x, dtype=np.float64)
    q_rows = np.asarray(q_rows, dtype=np.int64)
    if skip is not None:
        q_rows = np.setdiff1d(q_rows, np.asarray(skip, dtype=np.int64))
    nrm = np.sqrt(np.einsum("ij,ij->i", x64, x64))
    with np.errstate(divide="ignore", invalid="ignore"):
        sims = (x64[q_rows] @ x64.T) / (nrm[q_rows, None] * nrm[None, :])
    sims[np.arange(q_rows.size), q_rows] = -np.inf
    if skip is not None:
        sims[:, np.asarray(skip, dtype=np.int64)] = -np.inf
    sims[~np.isfinite(sims)] = -np.inf
    order = np.argsort(-sims, axis=1, kind="stable")[:, :k + 1]
    s = np.take_along_axis(sims, order, axis=1)
    assert np.isfinite(s).all()
    w = flat.key_window(0, s, 0, 0, x64.shape[1], cosine=True)
    return _share(s, w, k)


# ---- range searches and range self-joins on the row families ------------------------------------
# The oracle side of tests/test_gpu_range_families.py; tests/test_row_families_host.py
# admits every case from these functions alone.
RANGE_QUANTILES = (0.001, 0.01, 0.2)  # the share of all pairs a search radius takes in
RANGE_NQ = (100, 19)  # faiss's BLAS L2 key, and its sequential one (the first 19 queries)
# Cosine quantiles of the join thresholds.  At 0.99 and 0.999 a query row of an
# i.i.d. family has 60 +- 8 and 6 +- 3 hits of 6000, so no segment spans a
# 128-row tile; 0.95 (about 300 hits a row) is there for that.
JOIN_QUANTILES = (0.95, 0.99, 0.999)


def family_half_mask(n, seed=1):
    """The random half of n rows the selector cases select (bool mask)."""
    return np.random.default_rng(seed).random(n) < 0.5


def family_tombstones(xb, xq, count=50, seed=5):
    """(rows to add, labels to remove, the rows then live): `count` random rows
    of xb replaced by copies of the leading queries, each of which would be a
    hit of its query."""
    ids = np.random.default_rng(seed).choice(xb.shape[0], count, replace=False)
    planted = np.array(xb)
    planted[ids] = xq[np.arange(count) % xq.shape[0]]
    return planted, ids, np.delete(planted, ids, axis=0)


def plant_unselected(xb, xq, mask):
    """Copies of the queries into unselected rows (three per query where they
    fit): the unfiltered nearest rows then lie outside the selection."""
    xb = np.array(xb)
    out = np.nonzero(~mask)[0]
    for j, r in enumerate(out[: 3 * xq.shape[0]]):
        xb[r] = xq[j % xq.shape[0]]
    return xb


# A case in which the range search's bound decides (the quantile radii above
# never do: at ld = 128 the bound is some hundred times the candidate GEMM's
# actual error, so that no pair of theirs lies between the two).  BAND_ROWS
# large rows (|x| ~ 1000), added after BAND_BASE small ones (|x| ~ 0.01), are
# each built orthogonal to one of the first BAND_QUERIES queries (|q| ~ 10) up
# to an inner product of BAND_RADIUS: their exact scores scatter about the
# radius by the rounding of their coordinates (~3e-5), far more than the window
# (U |s| ~ 1.5e-8) and less than the fp32 GEMM's error on such a row (~1e-4).
# About half are hits, and the GEMM alone misclassifies a good part of them:
# only a bound that knows the large rows' norm keeps them as candidates.
BAND_BASE, BAND_ROWS, BAND_QUERIES, BAND_RADIUS = 2000, 1600, 8, np.float32(0.25)


def bound_band_case(seed=7):
    """(first add, second add, queries) of the band case, d = FAMILY_SHAPE[1]."""
    d, nq = FAMILY_SHAPE[1], FAMILY_SHAPE[2]
    rng = np.random.default_rng(seed)
    base = np.ldexp(rng.standard_normal((BAND_BASE, d)), -10).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    q = xq[np.arange(BAND_ROWS) % BAND_QUERIES].astype(np.float64)
    x = 100.0 * rng.standard_normal((BAND_ROWS, d))
    qq = np.einsum("ij,ij->i", q, q)[:, None]
    x += (float(BAND_RADIUS) - np.einsum("ij,ij->i", x, q)[:, None]) / qq * q
    return base, x.astype(np.float32), xq


def _norms2(x):
    x64 = np.asarray(x, dtype=np.float64)
    return np.einsum("ij,ij->i", x64, x64)


def range_reference(xb, xq, metric):
    """(s, w): the fp64 scores of every (query, row) pair and the window
    flat.key_window an exactly computed, once-rounded key can sit in."""
    s = flat.exact_scores(xb, xq, metric)
    return s, flat.key_window(metric, s, _norms2(xq)[:, None], _norms2(xb)[None, :], xb.shape[1])


def range_radius(s, metric, quantile):
    """The radius that takes in the share `quantile` of the pairs of s."""
    return np.float32(np.quantile(s, quantile if metric == flat.METRIC_L2 else 1.0 - quantile))


def range_cap(hits):
    """How many undecided pairs (|s - radius| <= w) a case of `hits` oracle hits
    may have: a condition on the inputs, so that a case cannot pass because
    everything was "undecided"."""
    return max(2, int(hits) // 200)


def join_reference(x, nq=None):
    """(s, w): the fp64 cosines of the ordered pairs (q, r) of rows, q among
    the first nq (default: all), NaN for a zero row, and their windows
    flat.key_window(..., cosine=True)."""
    x64 = np.asarray(x, dtype=np.float64)
    n2 = np.einsum("ij,ij->i", x64, x64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (x64[:nq] @ x64.T) / np.sqrt(np.outer(n2[:nq], n2))
    return s, flat.key_window(0, s, 0, 0, x64.shape[1], cosine=True)


def join_threshold(s, quantile, nq=FAMILY_JOIN_ROWS):
    """The cosine at `quantile` of the pairs the first nq rows query (s of
    join_reference): self pairs and zero rows (NaN already) left out."""
    c = np.array(s[:nq], dtype=np.float64)
    c[np.arange(nq), np.arange(nq)] = np.nan
    return np.float32(np.nanquantile(c, quantile))


def join_valid(nq, n, *, q0=0, exclude_self=True, upper=False):
    """The pairs a self-join of rows q0 .. q0 + nq may return."""
    rows = np.arange(n)[None, :]
    qrow = np.arange(q0, q0 + nq)[:, None]
    valid = np.ones((nq, n), dtype=bool)
    if exclude_self:
        valid &= rows != qrow
    if upper:
        valid &= rows > qrow
    return valid


def range_classes(s, w, radius, kind, valid=None):
    """(hit, inside, outside) over the pairs of s for a threshold `radius`.
    kind: flat.METRIC_L2 (a hit is s < radius), flat.METRIC_INNER_PRODUCT
    (s > radius) or "cosine" (s >= radius).  hit is the fp64 oracle's own
    answer; inside / outside are the pairs farther than their window from the
    threshold, which every correct engine classifies the same way.  A NaN score
    (a zero row's cosine) is outside; `valid` (bool, broadcastable) marks the
    pairs that may be returned at all."""
    r = float(radius)
    with np.errstate(invalid="ignore"):
        if kind == flat.METRIC_L2:
            hit, inside, outside = s < r, s < r - w, ~(s <= r + w)
        elif kind == flat.METRIC_INNER_PRODUCT:
            hit, inside, outside = s > r, s > r + w, ~(s >= r - w)
        elif kind == "cosine":
            hit, inside, outside = s >= r, s >= r + w, ~(s >= r - w)
        else:
            raise ValueError(kind)
    if valid is not None:
        valid = np.broadcast_to(valid, s.shape)
        hit, inside, outside = hit & valid, inside & valid, outside | ~valid
    return hit, inside, outside


def range_counts(s, w, radius, kind, valid=None):
    """From the oracle alone: (hits, undecided, hits per query)."""
    hit, inside, outside = range_classes(s, w, radius, kind, valid)
    return int(hit.sum()), int((~(inside | outside)).sum()), hit.sum(axis=1)


def range_contract(result, s, w, radius, kind, *, valid=None, base=0, timer=True, tag=""):
    """The contract of a range search or range self-join result (lims, D, I)
    against the oracle's (s, w) for its queries: lims well formed; labels
    strictly ascending per query and inside the index; every pair inside the
    threshold by more than its window present; none outside by more than its
    window (or outside `valid`) returned; D within the window of the returned
    label's fp64 score; at most range_cap(oracle hits) undecided pairs; and the
    candidate pass was gemm_range.  Every comparison is written so that a NaN
    fails it.  Returns (hits, undecided)."""
    lims, D, I = result
    nq, n = s.shape
    if timer:
        from vsearch import _lib

        assert _lib.timer_kernel() == "gemm_range"
    assert lims.dtype == np.uint64 and D.dtype == np.float32 and I.dtype == np.int64
    assert lims.shape == (nq + 1,)
    assert lims[0] == 0 and lims[-1] == len(D) == len(I)
    li = lims.astype(np.int64)
    assert (np.diff(li) >= 0).all()
    q = np.repeat(np.arange(nq), np.diff(li))
    r = I - base
    assert ((r >= 0) & (r < n)).all(), "a label outside the index"
    if len(I) > 1:  # strictly ascending between neighbours of one query's segment
        same = q[1:] == q[:-1]
        assert (np.diff(r)[same] > 0).all(), "labels not strictly ascending inside a query"
    got = np.zeros((nq, n), dtype=bool)
    got[q, r] = True
    hit, inside, outside = range_classes(s, w, radius, kind, valid)
    hits, undecided = int(hit.sum()), int((~(inside | outside)).sum())
    print(f"range {tag}: hits {len(D)} oracle {hits} undecided {undecided} cap {range_cap(hits)}")
    assert undecided <= range_cap(hits), (tag, undecided, hits)
    assert got[inside].all(), (tag, "a pair inside the threshold is missing",
                               int((inside & ~got).sum()))
    assert not got[outside].any(), (tag, "a pair outside the threshold (or the selection) "
                                    "was returned", int((outside & got).sum()))
    err = np.abs(D.astype(np.float64) - s[q, r])
    assert (err <= w[q, r]).all(), (tag, "D is not the exact key")
    assert abs(len(D) - hits) <= undecided, (tag, len(D), hits, undecided)
    return len(D), undecided
