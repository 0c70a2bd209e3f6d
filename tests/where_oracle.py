"""numpy oracle of the where searches (vs_search_where): the boolean mask of
the definition — row j passes query q's predicate — and the top-k over the
rows that pass and are not excluded, through ``flat.select_topk``."""

import numpy as np

from oracle import flat


def pass_mask(columns, tags, lo, hi, masks, n=None):
    """(nq, n) bool: row j passes predicate q.  columns (ncol, n) float (NaN:
    unknown) or None, tags (n,) uint64 or None (all 0; n then says how many
    rows there are when there are no columns either); lo / hi (nq, ncol),
    masks (nq, 3) = any_of, all_of, none_of.  Column c is tested unless
    lo == -inf and hi == +inf; a tested column passes iff lo <= v <= hi, so a
    NaN value fails it."""
    lo = np.asarray(lo, dtype=np.float32)
    hi = np.asarray(hi, dtype=np.float32)
    masks = np.asarray(masks, dtype=np.uint64)
    nq = masks.shape[0]
    cols = np.zeros((0, 0), dtype=np.float32) if columns is None else \
        np.asarray(columns, dtype=np.float32).reshape(lo.shape[1] if lo.ndim == 2 else 0, -1)
    if n is None:
        n = cols.shape[1] if cols.shape[0] else (0 if tags is None else np.asarray(tags).size)
    t = np.zeros(n, dtype=np.uint64) if tags is None else np.asarray(tags, dtype=np.uint64)
    ok = np.ones((nq, n), dtype=bool)
    for c in range(cols.shape[0]):
        tested = ~((lo[:, c] == -np.inf) & (hi[:, c] == np.inf))
        with np.errstate(invalid="ignore"):
            inside = (lo[:, c, None] <= cols[c][None, :]) & (cols[c][None, :] <= hi[:, c, None])
        ok &= inside | ~tested[:, None]
    any_of, all_of, none_of = masks[:, 0, None], masks[:, 1, None], masks[:, 2, None]
    ok &= (any_of == 0) | ((t[None, :] & any_of) != 0)
    ok &= (t[None, :] & all_of) == all_of
    ok &= (t[None, :] & none_of) == 0
    return ok


def excluded_mask(exclude, nq, n):
    """(nq, n) bool from per-query label lists (None: nothing excluded)."""
    out = np.zeros((nq, n), dtype=bool)
    if exclude is not None:
        for q, e in enumerate(exclude):
            e = np.asarray(e if e is not None else (), dtype=np.int64)
            out[q, e[(e >= 0) & (e < n)]] = True
    return out


def where_topk(scores, mask, k, metric, exclude=None, rule="faiss"):
    """(D, I) of the definition: the plain top-k over the rows that pass and
    are not excluded."""
    nq, n = scores.shape
    valid = mask & ~excluded_mask(exclude, nq, n)
    return flat.select_topk(scores, k, metric, valid=valid, rule=rule)
