"""The oracle of the boosted searches (DESIGN.md "Boosted searches"): the
numpy float32 restatement of b(q, r), bit for bit, the exact top-k by boosted
score, and the parity checker for boosted keys."""

from __future__ import annotations

import numpy as np

from oracle import flat

METRIC_L2 = flat.METRIC_L2
F32 = np.float32


def boost_terms(columns, kinds, params):
    """c[q, c, r] float32: every operation one float32 numpy operation."""
    cols = np.ascontiguousarray(columns, dtype=F32)
    ncol, n = cols.shape if cols.ndim == 2 else (0, 0)
    kinds = np.asarray(kinds, dtype=np.int32).reshape(-1, ncol)
    nq = kinds.shape[0]
    params = np.asarray(params, dtype=F32).reshape(nq, ncol, 4)
    out = np.zeros((nq, ncol, n), dtype=F32)
    zero, one = F32(0), F32(1)
    with np.errstate(all="ignore"):
        for q in range(nq):
            for c in range(ncol):
                kd = int(kinds[q, c])
                if kd == 0:
                    continue
                t, s, w, miss = (F32(v) for v in params[q, c])
                v = cols[c]
                d = (v - t).astype(F32)
                if kd == 1:
                    x = (one - (np.abs(d) / s).astype(F32)).astype(F32)
                    term = (w * np.where(x > zero, x, zero).astype(F32)).astype(F32)
                else:
                    y = (d / s).astype(F32)
                    z = np.where(y > zero, y, zero).astype(F32)
                    term = (w * np.where(z < one, z, one).astype(F32)).astype(F32)
                out[q, c] = np.where(np.isnan(v), miss, term).astype(F32)
    return out


def boost_values(columns, tags, kinds, params, tag_masks, tag_bonus, nrows=None):
    """(b float32 (nq, nrows), bounds float32 (nq, 2) = L, U): the definition.

    b = (((c0 + c1) + c2) + c3) + g0 + g1 + g2 + g3 with absent columns +0,
    summed left to right in float32; the bounds are the same sum over each
    term's smallest / largest value."""
    cols = np.zeros((0, 0), dtype=F32) if columns is None else \
        np.ascontiguousarray(columns, dtype=F32)
    if cols.ndim == 1:
        cols = cols.reshape(1, -1) if cols.size else cols.reshape(0, 0)
    ncol = cols.shape[0]
    n = cols.shape[1] if ncol else (len(tags) if tags is not None else int(nrows or 0))
    kinds = np.asarray(kinds, dtype=np.int32).reshape(-1, ncol) if ncol else None
    tag_masks = None if tag_masks is None else np.asarray(tag_masks, dtype=np.uint64).reshape(-1, 4)
    tag_bonus = None if tag_bonus is None else np.asarray(tag_bonus, dtype=F32).reshape(-1, 4)
    nq = kinds.shape[0] if ncol else tag_masks.shape[0]
    params = np.asarray(params, dtype=F32).reshape(nq, ncol, 4) if ncol else None
    tg = np.zeros(n, dtype=np.uint64) if tags is None else np.asarray(tags, dtype=np.uint64)
    terms = boost_terms(cols, kinds, params) if ncol else np.zeros((nq, 0, n), dtype=F32)
    b = np.zeros((nq, n), dtype=F32)
    bounds = np.zeros((nq, 2), dtype=F32)
    zero = F32(0)
    for q in range(nq):
        acc = terms[q, 0].copy() if ncol else np.zeros(n, dtype=F32)
        for c in range(1, 4):
            acc = (acc + (terms[q, c] if c < ncol else zero)).astype(F32)
        U, L = zero, zero
        for c in range(4):
            hi = lo = zero
            if c < ncol and kinds[q, c] != 0:
                w, miss = F32(params[q, c, 2]), F32(params[q, c, 3])
                hi = max(zero, w, miss)
                lo = min(zero, w, miss)
            U = F32(U + hi)
            L = F32(L + lo)
        for j in range(4):
            g = zero if tag_bonus is None else F32(tag_bonus[q, j])
            m = np.uint64(0) if tag_masks is None else tag_masks[q, j]
            acc = (acc + np.where((tg & m) != 0, g, zero).astype(F32)).astype(F32)
            U = F32(U + max(zero, g))
            L = F32(L + min(zero, g))
        b[q] = acc
        bounds[q] = (L, U)
    return b, bounds


def boosted_scores(scores, b, metric):
    """fp64 boosted score: score + b (inner product), distance - b (L2)."""
    s = np.asarray(scores, dtype=np.float64)
    b64 = np.asarray(b, dtype=np.float64)
    return s - b64 if metric == METRIC_L2 else s + b64


def boost_topk(scores, b, mask, k, metric, exclude=None):
    """(D, I): the k best rows by (boosted key, label) over fp64 scores among
    the rows mask allows (None: all) that are not in the query's exclusion
    list; flat.select_topk's lexicographic rule."""
    fs = boosted_scores(scores, b, metric)
    nq, n = fs.shape
    valid = np.ones((nq, n), dtype=bool) if mask is None else np.array(mask, dtype=bool)
    if valid.ndim == 1:
        valid = np.broadcast_to(valid, (nq, n)).copy()
    if exclude is not None:
        for q, ex in enumerate(exclude):
            ex = np.asarray(list(ex), dtype=np.int64)
            ex = ex[(ex >= 0) & (ex < n)]
            valid[q, ex] = False
    return flat.select_topk(fs, k, metric, valid=valid, rule="lex")


def mismatches(D, I, Dr, Ir, metric, xb, xq, b):
    """flat.mismatches for boosted keys.  D within flat.score_tolerance(metric,
    s, |q|^2, |x|^2) + 2^-23 (|s| + |b|) of the returned label's exact boosted
    score (the engines' fp32 contract plus the one more rounding of the
    subtraction); a label other than the oracle's j-th is a tie only if the two
    exact boosted scores are within the sum of their two tolerances."""
    xb = np.asarray(xb, dtype=np.float32)
    xq = np.asarray(xq, dtype=np.float32)
    D = np.asarray(D)
    I = np.asarray(I)
    b = np.asarray(b, dtype=np.float64)
    bad = []
    nq, k = Ir.shape
    nb2 = np.einsum("ij,ij->i", xb.astype(np.float64), xb.astype(np.float64))
    nq2 = np.einsum("ij,ij->i", xq.astype(np.float64), xq.astype(np.float64))

    def one(q, r):
        s = flat.exact_scores(xb[r:r + 1], xq[q:q + 1], metric)[0, 0]
        tol = float(flat.score_tolerance(metric, s, nq2[q], nb2[r])) + \
            2.0 ** -23 * (abs(s) + abs(b[q, r]))
        return float(boosted_scores(s, b[q, r], metric)), tol

    for q in range(nq):
        ids = I[q]
        real = ids[ids >= 0]
        if len(set(real.tolist())) != real.size:
            bad.append((q, "duplicate labels", ids.tolist()))
            continue
        if not np.array_equal(ids < 0, Ir[q] < 0):
            bad.append((q, "padding differs", ids.tolist(), Ir[q].tolist()))
            continue
        if np.any(ids >= xb.shape[0]):
            bad.append((q, "label out of range", ids.tolist()))
            continue
        for j in range(k):
            if ids[j] < 0:
                if D[q, j] != flat.neutral(metric):
                    bad.append((q, j, "padding score", float(D[q, j])))
                continue
            f_got, tol = one(q, int(ids[j]))
            if not abs(float(D[q, j]) - f_got) <= tol:  # a NaN is not within
                bad.append((q, j, "score", float(D[q, j]), f_got, tol))
            if ids[j] != Ir[q, j]:
                f_ref, tol_ref = one(q, int(Ir[q, j]))
                if not abs(f_got - f_ref) <= tol + tol_ref:
                    bad.append((q, j, "label", int(ids[j]), int(Ir[q, j]), f_got, f_ref,
                                tol + tol_ref))
    return bad
