"""The oracle of the example searches (test infrastructure only).

A user has positive examples P (at least one), negative examples N (possibly
none) and allowed rows A.  With key = distance (L2) or -score (inner product),
smaller is better: p(r) = min over P of key(e, r), its deciding example the
lowest position attaining it; n(r) = min over N (+inf without negatives); r is
favoured iff p(r) < n(r), strictly.  The answer is the first k favoured rows of
A in ascending (p, label) order, D = p as a score, E = the deciding position,
padded with (neutral, -1, -1).

``search`` is that definition in fp64 over ``flat.exact_scores``; ``problems``
is the checker for data whose fp32 keys round (every leniency is a
``flat.key_window``); ``rounds_model`` is a numpy model of the engine's rounds
(truncated lists, F, S) that must equal the definition."""

from __future__ import annotations

import numpy as np

from oracle import flat


def user_keys(xb, examples, metric: int, bf16: bool = False) -> np.ndarray:
    """fp64 keys (len(examples), n) of example vectors against the rows."""
    ex = np.asarray(examples, dtype=np.float32).reshape(-1, np.asarray(xb).shape[1])
    if bf16:
        xb, ex = flat.round_bf16(xb), flat.round_bf16(ex)
    s = flat.exact_scores(xb, ex, metric)
    return s if metric == flat.METRIC_L2 else -s


def allowed_mask(n: int, exclude) -> np.ndarray:
    a = np.ones(n, dtype=bool)
    if exclude is not None:
        e = np.asarray(exclude, dtype=np.int64).ravel()
        a[e[(e >= 0) & (e < n)]] = False
    return a


def from_keys(kp, kn, allowed, k: int, metric: int):
    """The definition over key matrices kp (a, n) and kn (b, n): (D, I, E) rows."""
    kp = np.asarray(kp, dtype=np.float64)
    n = kp.shape[1]
    p = kp.min(axis=0)
    e = kp.argmin(axis=0)  # the first (lowest) position among equal keys
    kn = np.asarray(kn, dtype=np.float64).reshape(-1, n)
    nn = kn.min(axis=0) if kn.shape[0] else np.full(n, np.inf)
    fav = np.nonzero(np.asarray(allowed, dtype=bool) & (p < nn))[0]
    order = fav[np.lexsort((fav, p[fav]))][:k]
    D = np.full(k, flat.neutral(metric), dtype=np.float32)
    I = np.full(k, -1, dtype=np.int64)
    E = np.full(k, -1, dtype=np.int32)
    m = order.size
    D[:m] = (p[order] if metric == flat.METRIC_L2 else -p[order]).astype(np.float32)
    I[:m] = order
    E[:m] = e[order]
    return D, I, E


def search(xb, users, k: int, metric: int, exclude=None, bf16: bool = False):
    """``users``: a sequence of (positive vectors (a, d), negative vectors (b, d)
    or None); ``exclude``: per-user label lists or None.  Returns (D, I, E)."""
    n = np.asarray(xb).shape[0]
    out = []
    for u, (pos, neg) in enumerate(users):
        kp = user_keys(xb, pos, metric, bf16)
        kn = user_keys(xb, neg, metric, bf16) if neg is not None and len(neg) else np.zeros((0, n))
        out.append(from_keys(kp, kn, allowed_mask(n, None if exclude is None else exclude[u]),
                             k, metric))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def _windows(xb, ex, keys, metric, bf16):
    """flat.key_window of every (example, row) pair."""
    xb = np.asarray(xb, dtype=np.float32)
    ex = np.asarray(ex, dtype=np.float32).reshape(-1, xb.shape[1])
    if bf16:
        xb, ex = flat.round_bf16(xb), flat.round_bf16(ex)
    xn2 = np.einsum("ij,ij->i", xb.astype(np.float64), xb.astype(np.float64))
    qn2 = np.einsum("ij,ij->i", ex.astype(np.float64), ex.astype(np.float64))
    return flat.key_window(metric, keys, qn2[:, None], xn2[None, :], xb.shape[1])


def user_state(xb, pos, neg, metric: int, bf16: bool = False):
    """(kp, p, wp, nn, wn): the positive keys, p and n with the key windows of
    the pairs that attain them (wn = 0 and n = +inf without negatives)."""
    n = np.asarray(xb).shape[0]
    kp = user_keys(xb, pos, metric, bf16)
    wp_all = _windows(xb, pos, kp, metric, bf16)
    ip = kp.argmin(axis=0)
    p, wp = kp[ip, np.arange(n)], wp_all[ip, np.arange(n)]
    if neg is None or len(neg) == 0:
        return kp, p, wp, np.full(n, np.inf), np.zeros(n)
    kn = user_keys(xb, neg, metric, bf16)
    wn_all = _windows(xb, neg, kn, metric, bf16)
    i_n = kn.argmin(axis=0)
    return kp, p, wp, kn[i_n, np.arange(n)], wn_all[i_n, np.arange(n)]


def undecided(xb, pos, neg, metric: int, allowed=None, bf16: bool = False) -> np.ndarray:
    """The allowed rows with |p - n| <= key_window(p) + key_window(n)."""
    _, p, wp, nn, wn = user_state(xb, pos, neg, metric, bf16)
    und = np.abs(p - nn) <= wp + wn
    if allowed is not None:
        und &= np.asarray(allowed, dtype=bool)
    return np.nonzero(und)[0]


def problems(D, I, E, xb, users, k: int, metric: int, exclude=None, bf16: bool = False):
    """Checks a result on data whose keys round.  Every returned row must be
    allowed, unique and not definitely disfavoured, its D within key_window of
    its fp64 p and D in raw order, its E a positive that attains p within the
    window; every definitely favoured allowed row better than the last returned
    entry by more than the windows must be present, and a padded list must hold
    every definitely favoured row.  Returns a list of problems (empty: none)."""
    bad = []
    n = np.asarray(xb).shape[0]
    neutral = flat.neutral(metric)
    for u, (pos, neg) in enumerate(users):
        allowed = allowed_mask(n, None if exclude is None else exclude[u])
        kp, p, wp, nn, wn = user_state(xb, pos, neg, metric, bf16)
        fav_sure = allowed & (p < nn - (wp + wn))
        dis_sure = p > nn + (wp + wn)
        ids = I[u]
        m = int((ids >= 0).sum())
        if (ids[:m] < 0).any() or (ids[m:] != -1).any():
            bad.append((u, "padding inside the list"))
            continue
        if (D[u, m:] != neutral).any() or (E[u, m:] != -1).any():
            bad.append((u, "padding is not (neutral, -1, -1)"))
        got = ids[:m]
        if (got >= n).any():
            bad.append((u, "label out of range"))
            continue
        if np.unique(got).size != m:
            bad.append((u, "a label twice"))
        if not allowed[got].all():
            bad.append((u, "an excluded label"))
        if dis_sure[got].any():
            bad.append((u, "a definitely disfavoured row", got[dis_sure[got]].tolist()))
        key = (D[u, :m] if metric == flat.METRIC_L2 else -D[u, :m]).astype(np.float64)
        off = np.abs(key - p[got]) > wp[got]
        if off.any():
            bad.append((u, "D outside the key window", got[off].tolist()))
        for j in range(1, m):
            if key[j] < key[j - 1] or (key[j] == key[j - 1] and got[j] < got[j - 1]):
                bad.append((u, "not in (key, label) order", j))
        ee = E[u, :m]
        if ((ee < 0) | (ee >= kp.shape[0])).any():
            bad.append((u, "E out of range"))
        elif (kp[ee, got] > p[got] + wp[got]).any():
            bad.append((u, "E does not attain p"))
        present = np.zeros(n, dtype=bool)
        present[got] = True
        if m < k:
            missing = np.nonzero(fav_sure & ~present)[0]
        else:
            last = int(got[-1])
            missing = np.nonzero(fav_sure & ~present & (p < p[last] - (wp + wp[last])))[0]
        if missing.size:
            bad.append((u, "a definitely favoured row is missing", missing[:5].tolist()))
        if m < min(k, int(fav_sure.sum())):
            bad.append((u, "too few rows"))
    return bad


# ---- the engine's rounds as a numpy model -------------------------------------------------
def window(need: int, rnd: int, live: int) -> int:
    """The window of round ``rnd`` (vs_host.h distinct_window)."""
    w = need + max(16, need // 2)
    for _ in range(rnd):
        if w >= live:
            break
        w *= 4
    return min(w, live)


def rounds_model(kp, kn, allowed, k: int, metric: int, live: int | None = None):
    """The rounds of DESIGN.md "Example searches" over exact key matrices: per
    positive the first w allowed rows in (key, label) order; F = the smallest
    last entry of the full lists; S = the union's rows with (p^, label) <= F;
    settled when S holds k favoured rows or every list reached the end.
    Returns ((D, I, E), rounds)."""
    kp = np.asarray(kp, dtype=np.float64)
    a, n = kp.shape
    kn = np.asarray(kn, dtype=np.float64).reshape(-1, n)
    nn = kn.min(axis=0) if kn.shape[0] else np.full(n, np.inf)
    rows = np.nonzero(np.asarray(allowed, dtype=bool))[0]
    live = n if live is None else live
    lists = [rows[np.lexsort((rows, kp[j][rows]))] for j in range(a)]
    for rnd in range(64):
        w = window(k, rnd, live)
        F = (np.inf, -1)
        best = {}
        for j in range(a):
            L = lists[j][:w]
            if L.size == w and w < live:  # a full window that is not every live row
                F = min(F, (kp[j, L[-1]], int(L[-1])))
            for r in map(int, L):
                c = (kp[j, r], j)
                if r not in best or c < best[r]:
                    best[r] = c
        S = sorted((key, r, j) for r, (key, j) in best.items() if (key, r) <= F)
        fav = [(key, r, j) for key, r, j in S if key < nn[r]]
        if len(fav) >= k or F[0] == np.inf:
            fav = fav[:k]
            D = np.full(k, flat.neutral(metric), dtype=np.float32)
            I = np.full(k, -1, dtype=np.int64)
            E = np.full(k, -1, dtype=np.int32)
            for i, (key, r, j) in enumerate(fav):
                D[i] = key if metric == flat.METRIC_L2 else -key
                I[i], E[i] = r, j
            return (D, I, E), rnd + 1
    raise AssertionError("the schedule did not end")
