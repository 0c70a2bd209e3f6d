"""A plain numpy fp64 restatement of the MMR definition in include/vsearch.h
("MMR searches"): LangChain's maximal_marginal_relevance / cosine_similarity
(langchain_community.vectorstores.utils, 0.3.x, as recalled: langchain is not
vendored).  Test infrastructure only; tests/test_mmr_host.py and
tests/test_gpu_mmr.py use it."""

from __future__ import annotations

import numpy as np


def slack(d: int) -> float:
    """The fp64 rounding slack between two evaluations of one MMR score over
    d-dimensional rows: each of the three fp64 sums of a cosine carries at most
    d * 2^-53 relative to |a||b|, the quotient, square root and score
    arithmetic a few units more: (2d + 8) * 2^-53 a side, both sides counted."""
    return (4 * d + 16) * 2.0 ** -53


def cosines(A, B) -> np.ndarray:
    """cos(a, b) = dot(a, b) / sqrt(dot(a, a) * dot(b, b)) for every row a of A
    and b of B, the sums in float64 (the Gram as A @ B.T), a non-finite
    quotient counting as 0."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    dots = A @ B.T
    na = np.einsum("ij,ij->i", A, A)
    nb = np.einsum("ij,ij->i", B, B)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = dots / np.sqrt(na[:, None] * nb[None, :])
    c[~np.isfinite(c)] = 0.0
    return c


class Problem:
    """One query and its candidate list: rows E (F, d; any row for an empty
    slot), valid (F,) bool.  Holds s = cos(q, c_i) and the Gram of cosines."""

    def __init__(self, q, E, valid=None):
        E = np.asarray(E, dtype=np.float64).reshape(len(E), -1)
        self.F = E.shape[0]
        self.valid = (np.ones(self.F, dtype=bool) if valid is None
                      else np.asarray(valid, dtype=bool))
        self.s = cosines(np.asarray(q, dtype=np.float64)[None, :], E)[0] if self.F else np.zeros(0)
        self.G = cosines(E, E) if self.F else np.zeros((0, 0))
        self.GT = np.ascontiguousarray(self.G.T)  # GT[p] = G[:, p], contiguous

    def _scores(self, red, free, lambda_mult: float) -> np.ndarray:
        # red: every position's largest cosine to the picks so far (None: no pick yet)
        lam = float(lambda_mult)
        sc = self.s if red is None else lam * self.s - (1.0 - lam) * red
        return np.where(free, sc, -np.inf)

    def scores(self, picked, lambda_mult: float):
        """(scores, free): the score of every position given the picks so far
        (-inf where the position is no free candidate)."""
        picked = list(picked)
        free = self.valid.copy()
        free[picked] = False
        red = self.G[:, picked].max(axis=1) if picked else None
        return self._scores(red, free, lambda_mult), free

    def select(self, k: int, lambda_mult: float):
        """(picks, gaps): the positions in pick order (the best score, the
        lowest position among equals) and at each step the gap between the
        best and the second-best free score (inf when only one is free).  The
        picks for k are a prefix of the picks for any larger k."""
        picks, gaps = [], []
        nfree = int(self.valid.sum())
        steps = min(int(k), nfree)
        lam = float(lambda_mult)
        # the same values as scores() recomputes, kept up to date: red = the
        # running maximum (max is exact), bar = 0 for a free position, -inf else
        bar = np.where(self.valid, 0.0, -np.inf)
        red = None
        for _ in range(steps):
            sc = (self.s if red is None else lam * self.s - (1.0 - lam) * red) + bar
            p = int(np.argmax(sc))  # the first of equal maxima
            best = sc[p]
            sc[p] = -np.inf
            gaps.append(float(best - sc.max()) if nfree > 1 else float("inf"))
            picks.append(p)
            bar[p] = -np.inf
            nfree -= 1
            red = self.GT[p].copy() if red is None else np.maximum(red, self.GT[p], out=red)
        return picks, gaps


def mmr_positions(q, E, k: int, lambda_mult: float, valid=None) -> np.ndarray:
    """int32 (k,): the picks' positions in pick order, -1 past them."""
    picks, _ = Problem(q, E, valid).select(k, lambda_mult)
    out = np.full(int(k), -1, dtype=np.int32)
    out[:len(picks)] = picks
    return out


def mmr_select_labels(rows, x, cand, k: int, lambda_mult: float, id_base: int = 0) -> np.ndarray:
    """index.mmr_select over the array `rows` (label l = row l - id_base):
    cand int64 (n, F) labels, -1 an empty slot.  Returns int32 (n, k)."""
    x = np.asarray(x, dtype=np.float32)
    cand = np.asarray(cand, dtype=np.int64)
    out = np.full((x.shape[0], int(k)), -1, dtype=np.int32)
    for i in range(x.shape[0]):
        valid = cand[i] != -1
        if not valid.any():
            continue
        E = np.asarray(rows)[np.where(valid, cand[i] - id_base, 0)]
        out[i] = mmr_positions(x[i], E, k, lambda_mult, valid)
    return out


def replay(problem: Problem, picks, k: int, lambda_mult: float, d: int):
    """The checking rule of the GPU tests: replays `picks` (a device's pos row,
    -1 padded) step by step.  At each step the pick must be a free candidate
    whose oracle score, for the device's own prefix, is within slack(d) of the
    maximum.  Returns the list of steps at which the pick is not the oracle's
    own (lowest position of the maximum), after asserting the rule."""
    picks = [int(p) for p in picks]
    steps = min(int(k), int(problem.valid.sum()))
    assert all(p == -1 for p in picks[steps:]), ("padding", picks, steps)
    assert len(picks) >= steps
    differ = []
    prefix = []
    for t in range(steps):
        p = picks[t]
        sc, free = problem.scores(prefix, lambda_mult)
        assert 0 <= p < problem.F and free[p], (t, p, "not a free candidate")
        best = float(sc.max())
        assert sc[p] >= best - slack(d), (t, p, float(sc[p]), best)
        if p != int(np.argmax(sc)):
            differ.append(t)
        prefix.append(p)
    return differ
