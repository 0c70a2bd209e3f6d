"""The oracle of the bonus searches (DESIGN.md "Bonus searches"): the final
keys in float32 numpy, one numpy operation per rounding, on top of
``boost_oracle.boost_values``; the full ranking by (final key, label); and the
parity checker for final keys."""

from __future__ import annotations

import numpy as np

from oracle import flat

METRIC_L2 = flat.METRIC_L2
F32 = np.float32


def dense_lists(lists, nq, n):
    """Per-query bonus lists (a dict label -> value, a (labels, values) pair
    or None each) as dense arrays: (s float32 (nq, n), listed bool (nq, n)).
    Labels outside [0, n) are ignored, as the search ignores them."""
    s = np.zeros((nq, n), dtype=F32)
    listed = np.zeros((nq, n), dtype=bool)
    for q, e in enumerate(lists if lists is not None else [None] * nq):
        if e is None:
            continue
        labels, vals = (list(e.keys()), list(e.values())) if isinstance(e, dict) else e
        labels = np.asarray(labels, dtype=np.int64).ravel()
        vals = np.asarray(vals, dtype=F32).ravel()
        ok = (labels >= 0) & (labels < n)
        s[q, labels[ok]] = vals[ok]
        listed[q, labels[ok]] = True
    return s, listed


def final_keys(scores, b, s, listed, metric):
    """final_key float32 (nq, n): key = fl32(score) (L2) or fl32(-score) (inner
    product), then fl32(key - b), then for the listed rows fl32(. - s)."""
    sc = np.asarray(scores, dtype=np.float64)
    key = (sc if metric == METRIC_L2 else -sc).astype(F32)
    bb = np.zeros(key.shape, dtype=F32) if b is None else np.asarray(b, dtype=F32)
    f1 = (key - bb).astype(F32)
    f2 = (f1 - np.asarray(s, dtype=F32)).astype(F32)
    return np.where(np.asarray(listed, dtype=bool), f2, f1).astype(F32)


def bonus_topk(scores, b, s, listed, mask, k, metric, exclude=None):
    """(D, I): the k allowed rows with the smallest (final key, label), D =
    final key (L2) or its negative (inner product), padded with (neutral, -1).
    Allowed: mask (None: all) and not in the query's exclusion list."""
    fin = final_keys(scores, b, s, listed, metric)
    nq, n = fin.shape
    valid = np.ones((nq, n), dtype=bool) if mask is None else np.array(mask, dtype=bool)
    if valid.ndim == 1:
        valid = np.broadcast_to(valid, (nq, n)).copy()
    if exclude is not None:
        for q, ex in enumerate(exclude):
            ex = np.asarray(list(ex), dtype=np.int64)
            ex = ex[(ex >= 0) & (ex < n)]
            valid[q, ex] = False
    dvals = fin.astype(np.float64) if metric == METRIC_L2 else -fin.astype(np.float64)
    return flat.select_topk(dvals, k, metric, valid=valid, rule="lex")


def final_scores(scores, b, s, listed, metric):
    """fp64 final score: score + b + s (inner product), distance - b - s (L2)."""
    sc = np.asarray(scores, dtype=np.float64)
    add = np.asarray(b, dtype=np.float64) + \
        np.where(np.asarray(listed, dtype=bool), np.asarray(s, dtype=np.float64), 0.0)
    return sc - add if metric == METRIC_L2 else sc + add


def mismatches(D, I, Dr, Ir, metric, xb, xq, b, s, listed):
    """boost_oracle.mismatches for final keys.  D within
    flat.score_tolerance(metric, score, |q|^2, |x|^2) + 2^-23 (|score| + |b|) +
    2^-23 (|score| + |b| + |s|) of the returned label's exact final score (the
    engines' fp32 contract plus the two roundings of the two subtractions); a
    label other than the oracle's j-th is a tie only if the two exact final
    scores are within the sum of their two tolerances."""
    xb = np.asarray(xb, dtype=np.float32)
    xq = np.asarray(xq, dtype=np.float32)
    D = np.asarray(D)
    I = np.asarray(I)
    b = np.asarray(b, dtype=np.float64)
    s = np.where(np.asarray(listed, dtype=bool), np.asarray(s, dtype=np.float64), 0.0)
    bad = []
    nq, k = Ir.shape
    nb2 = np.einsum("ij,ij->i", xb.astype(np.float64), xb.astype(np.float64))
    nq2 = np.einsum("ij,ij->i", xq.astype(np.float64), xq.astype(np.float64))

    def one(q, r):
        sc = flat.exact_scores(xb[r:r + 1], xq[q:q + 1], metric)[0, 0]
        tol = float(flat.score_tolerance(metric, sc, nq2[q], nb2[r])) + \
            2.0 ** -23 * (abs(sc) + abs(b[q, r])) + \
            2.0 ** -23 * (abs(sc) + abs(b[q, r]) + abs(s[q, r]))
        add = b[q, r] + s[q, r]
        return float(sc - add if metric == METRIC_L2 else sc + add), tol

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
