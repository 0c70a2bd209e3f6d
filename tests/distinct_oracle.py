"""The oracle of the distinct searches (test infrastructure only).

A grouping gives every row a group (an int >= 0, or -1: the row is its own
group).  For a query, the allowed rows ordered by (key, label) — key =
distance (L2) or -score (inner product), smaller is better — give every group
a representative: its first row in that order.  A distinct search returns what
a plain search would return over the representatives alone."""

from __future__ import annotations

import numpy as np

from oracle import flat


def representatives(scores: np.ndarray, groups, metric: int, valid=None) -> np.ndarray:
    """bool (nq, n): row r is the representative of its group for query q."""
    scores = np.asarray(scores, dtype=np.float64)
    groups = np.asarray(groups, dtype=np.int64)
    nq, n = scores.shape
    assert groups.shape == (n,)
    key = scores if metric == flat.METRIC_L2 else -scores
    labels = np.arange(n)
    # a row of its own gets a group id no other row has
    gid = np.where(groups >= 0, groups, groups.max(initial=0) + 1 + labels)
    rep = np.zeros((nq, n), dtype=bool)
    for q in range(nq):
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(key[q]) & (key[q] < float(flat.FLT_MAX))
        if valid is not None:
            ok &= np.asarray(valid[q], dtype=bool)
        rows = labels[ok]
        order = rows[np.lexsort((rows, key[q][rows]))]
        _, first = np.unique(gid[order], return_index=True)
        rep[q, order[first]] = True
    return rep


def distinct_topk(scores, groups, k: int, metric: int, valid=None, rule: str = "faiss"):
    """(D float32 (nq, k), I int64 (nq, k)): the top-k of the representatives,
    in faiss's order (rule="faiss") or plain (key, label) order (rule="lex",
    VS_RAW_ORDER), padded with (neutral, -1)."""
    rep = representatives(scores, groups, metric, valid)
    return flat.select_topk(np.asarray(scores, dtype=np.float64), int(k), metric, valid=rep,
                            rule=rule)


def group_problems(I, scores, groups, valid=None):
    """What flat.mismatches does not look at: no two returned labels of a query
    share a group, and every returned label is the lowest label of its group
    among that group's allowed rows with the returned label's own exact score
    (copies of a row score the same in fp64 as in the engine).  Returns a list
    of problems (empty: none)."""
    groups = np.asarray(groups, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float64)
    bad = []
    for q in range(I.shape[0]):
        ids = I[q][I[q] >= 0]
        g = groups[ids]
        g = g[g >= 0]
        if np.unique(g).size != g.size:
            bad.append((q, "a group twice", ids.tolist()))
        for r in ids:
            if groups[r] < 0:
                continue
            same = (groups == groups[r]) & (scores[q] == scores[q, r])
            if valid is not None:
                same &= np.asarray(valid[q], dtype=bool)
            low = int(np.nonzero(same)[0][0])
            if low != int(r):
                bad.append((q, "not the lowest label of its group at that score", int(r), low))
    return bad
