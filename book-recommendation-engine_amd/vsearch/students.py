"""Student-neighbour self-join on the MI355X engine.

Replaces the per-student pgvector loop of the graph refresher
(src/graph_refresher/main.py:299-354) and the single-student query of the
similarity worker (src/incremental_workers/similarity/main.py:80-94):

    vectors -> "[%.6f,...]" pgvector literals (main.py:301)
    for each student s:  SELECT student_id, 1-(vec <=> src.vec) AS sim ...
                         WHERE student_id <> s ORDER BY vec <=> src.vec LIMIT 15
    keep rows with sim >= S.similarity_threshold (0.75; main.py:350-354, settings.py:139)

Here all students are one ``vs_selfjoin`` launch (cosine, exclude self by row,
top-k), with the %.6f quantisation applied on the host exactly as the text
round-trip does.  Output rows are the ``student_similarity(a, b, sim)`` tuples
(sql/00_init_schema.sql:105-111) the refresher would insert.

The graph itself is a threshold graph — every pair with ``sim >= threshold``;
the ``LIMIT 15`` is there because SQL needs a k, and in a dense cluster it drops
every neighbour past the 15th.  ``student_edges`` / ``StudentIndex.edges`` /
``StudentIndex.edges_of`` answer that question directly: one range self-join
(``vs_range_selfjoin``), as many rows as pass.  The top-15 forms above remain
the drop-in replacement.

A re-embedded student (student_embedding/main.py:137-145 upserts the vector,
the similarity worker then recomputes that student's rows) is
``StudentIndex.replace`` — the vector changes where it is stored — and a batch
of them ``StudentIndex.reembed``: one in-place update, one row-list join, and
the rows that name an updated student, which are the graph's complete diff.

Semantics notes: ties (equal similarity) are ordered by lower row; SQL leaves
them unspecified.  Zero-norm vectors never match; pgvector returns NaN for them
and the refresher's ``sim >= threshold`` test drops NaN too.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import faiss as vfaiss

DEFAULT_K = 15  # LIMIT 15 (graph_refresher/main.py:346, similarity/main.py:86)
DEFAULT_THRESHOLD = 0.75  # S.similarity_threshold (src/common/settings.py:139)


def pgvector_quantize(vectors) -> np.ndarray:
    """The f"{x:.6f}" text literal (graph_refresher/main.py:301) parsed back to float32."""
    v = np.asarray(vectors, dtype=np.float64)
    txt = np.char.mod("%.6f", v)
    return txt.astype(np.float64).astype(np.float32)


def build_student_index(vectors, *, quantize: bool = True, device: Optional[int] = None):
    x = pgvector_quantize(vectors) if quantize else np.ascontiguousarray(vectors, np.float32)
    index = vfaiss.IndexFlatIP(x.shape[1], device=device)
    index.add(x)
    return index


def student_neighbours(keys: Sequence[str], vectors, *, k: int = DEFAULT_K,
                       threshold: Optional[float] = DEFAULT_THRESHOLD, quantize: bool = True,
                       device: Optional[int] = None) -> List[Tuple[str, str, float]]:
    """All-students top-k cosine neighbours as (a, b, sim) rows.

    ``threshold=None`` keeps all k (the similarity worker's behaviour,
    similarity/main.py:89-94); a number applies the refresher's filter.
    """
    keys = list(keys)
    if len(keys) == 0:
        return []
    index = build_student_index(vectors, quantize=quantize, device=device)
    min_sim = -np.inf if threshold is None else float(threshold)
    S, I = index.selfjoin(k, exclude_self=True, min_sim=min_sim)
    rows = []
    for a in range(len(keys)):
        for j in range(S.shape[1]):
            b = int(I[a, j])
            if b < 0:
                continue
            rows.append((keys[a], keys[b], float(S[a, j])))
    return rows


def _edge_rows(keys, lims, S, I, q0: int, directed: bool, mirror: bool):
    """(a, b, sim) rows of a join result over query rows q0 ..: ordered by a's
    position, then b's.  ``mirror``: the result is an upper join (b > a); the
    directed rows add each pair's (b, a) with the same sim."""
    counts = np.diff(np.asarray(lims).astype(np.int64))
    a = np.repeat(np.arange(q0, q0 + counts.size, dtype=np.int64), counts)
    b = np.asarray(I, dtype=np.int64)
    s = np.asarray(S, dtype=np.float32)
    if directed and mirror:
        a, b, s = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([s, s])
        order = np.lexsort((b, a))
        a, b, s = a[order], b[order], s[order]
    return [(keys[int(x)], keys[int(y)], float(v)) for x, y, v in zip(a, b, s)]


def student_edges(keys: Sequence[str], vectors, *, threshold: float = DEFAULT_THRESHOLD,
                  quantize: bool = True, device: Optional[int] = None,
                  directed: bool = True) -> List[Tuple[str, str, float]]:
    """The threshold graph: (a, b, sim) for EVERY pair of students with
    ``sim >= threshold``, ordered by a's position, then b's — what the
    refresher's filter (graph_refresher/main.py:350-354) means without its
    ``LIMIT 15``.

    ``directed=True`` emits both (a, b) and (b, a), the shape of the
    ``student_similarity`` table; ``directed=False`` each pair once, a before b.
    Both come from one upper-triangle join (the similarity is symmetric bit for
    bit), mirrored on the host for the directed form."""
    keys = list(keys)
    if len(keys) == 0:
        return []
    index = build_student_index(vectors, quantize=quantize, device=device)
    lims, S, I = index.range_selfjoin(float(threshold), exclude_self=True, upper=True)
    return _edge_rows(keys, lims, S, I, 0, directed, True)


class StudentIndex:
    """Resident student vectors for per-event similarity (the similarity worker,
    src/incremental_workers/similarity/main.py:57-102, runs one student's query
    per STUDENT_EMBEDDING event).  The matrix is uploaded once; each event is one
    single-row self-join on the kept index (an HBM-bound scan, no re-upload), and
    a re-embedded student replaces its own row (the student_embeddings upsert of
    student_embedding/main.py:120-146)."""

    def __init__(self, keys: Sequence[str], vectors, *, quantize: bool = True,
                 device: Optional[int] = None):
        self.keys: List[str] = list(keys)
        if len(set(self.keys)) != len(self.keys):
            raise ValueError("StudentIndex: duplicate student keys")
        self.quantize = quantize
        self.index = build_student_index(vectors, quantize=quantize, device=device)
        self._row = {key: i for i, key in enumerate(self.keys)}

    def __len__(self) -> int:
        return len(self.keys)

    def neighbours_of(self, student: str, k: int = DEFAULT_K) -> List[Tuple[str, str, float]]:
        q = self._row[student]
        S, I = self.index.selfjoin(k, q0=q, nq=1, exclude_self=True)
        return [(student, self.keys[int(b)], float(s)) for s, b in zip(S[0], I[0]) if b >= 0]

    def neighbours(self, k: int = DEFAULT_K,
                   threshold: Optional[float] = DEFAULT_THRESHOLD) -> List[Tuple[str, str, float]]:
        min_sim = -np.inf if threshold is None else float(threshold)
        S, I = self.index.selfjoin(k, exclude_self=True, min_sim=min_sim)
        return [(self.keys[a], self.keys[int(b)], float(S[a, j]))
                for a in range(S.shape[0]) for j, b in enumerate(I[a]) if b >= 0]

    def edges(self, threshold: float = DEFAULT_THRESHOLD,
              directed: bool = True) -> List[Tuple[str, str, float]]:
        """``student_edges`` over the resident index."""
        if not self.keys:
            return []
        lims, S, I = self.index.range_selfjoin(float(threshold), exclude_self=True, upper=True)
        return _edge_rows(self.keys, lims, S, I, 0, directed, True)

    def edges_of(self, student: str,
                 threshold: float = DEFAULT_THRESHOLD) -> List[Tuple[str, str, float]]:
        """One student's edges, every one at or above the threshold (the
        similarity worker's event, similarity/main.py:80-94, without its
        LIMIT), ordered by the neighbour's position."""
        q = self._row[student]
        lims, S, I = self.index.range_selfjoin(float(threshold), q0=q, nq=1, exclude_self=True)
        return _edge_rows(self.keys, lims, S, I, q, True, False)

    def edges_of_many(self, students: Sequence[str],
                      threshold: float = DEFAULT_THRESHOLD) -> List[Tuple[str, str, float]]:
        """``edges_of`` for a list of students in one row-list join (one pass
        over the rows per 128 students, not one per student): each student's
        rows in list order, ordered by the neighbour's position."""
        rows = np.array([self._row[s] for s in students], dtype=np.int64)
        if rows.size == 0:
            return []
        lims, S, I = self.index.range_selfjoin(float(threshold), rows=rows, exclude_self=True)
        counts = np.diff(np.asarray(lims).astype(np.int64))
        a = np.repeat(rows, counts)
        return [(self.keys[int(x)], self.keys[int(y)], float(v)) for x, y, v in zip(a, I, S)]

    def _prepare(self, vectors) -> np.ndarray:
        v = np.asarray(vectors, dtype=np.float32).reshape(-1, self.index.d)
        return pgvector_quantize(v) if self.quantize else np.ascontiguousarray(v)

    def replace(self, student: str, vector) -> None:
        """Replace one student's vector in place (the ``ON CONFLICT ... DO
        UPDATE SET vec`` of student_embedding/main.py:137-145): no row moves,
        keys and positions stay.  An unknown student raises ``KeyError``."""
        r = self._row[student]
        self.index.update(np.array([r], dtype=np.int64), self._prepare(vector))

    def reembed(self, updates, threshold: float = DEFAULT_THRESHOLD
                ) -> List[Tuple[str, str, float]]:
        """Re-embed a batch of students and return their diff of the graph.

        ``updates``: a mapping student -> vector or a list of (student,
        vector), every student known (``KeyError`` otherwise, before anything
        changes) and named once.  One in-place ``update``, then one row-list
        join.  Returns the directed (a, b, sim) rows that name an updated
        student — (u, r) and the mirrored (r, u), a pair of two updated
        students once per direction — ordered by a's position, then b's.  The
        caller deletes every ``student_similarity`` row naming an updated
        student and inserts these (the similarity is the same bits in both
        directions, so the updated students' edges are the complete diff)."""
        items = list(updates.items()) if hasattr(updates, "items") else list(updates)
        if not items:
            return []
        rows = np.array([self._row[s] for s, _ in items], dtype=np.int64)
        if np.unique(rows).size != rows.size:
            raise ValueError("StudentIndex.reembed: a student named twice")
        self.index.update(rows, self._prepare([v for _, v in items]))
        lims, S, I = self.index.range_selfjoin(float(threshold), rows=rows, exclude_self=True)
        counts = np.diff(np.asarray(lims).astype(np.int64))
        u = np.repeat(rows, counts)
        r = np.asarray(I, dtype=np.int64)
        s = np.asarray(S, dtype=np.float32)
        # (u, r) as found; (r, u) mirrored unless r is updated too (its own
        # segment holds that direction already)
        other = ~np.isin(r, rows)
        a = np.concatenate([u, r[other]])
        b = np.concatenate([r, u[other]])
        s = np.concatenate([s, s[other]])
        order = np.lexsort((b, a))
        return [(self.keys[int(x)], self.keys[int(y)], float(v))
                for x, y, v in zip(a[order], b[order], s[order])]

    def upsert(self, student: str, vector) -> None:
        """Insert or replace one student's vector (a removed row compacts the
        later rows, faiss remove_ids semantics; the key list follows)."""
        v = np.asarray(vector, dtype=np.float32).reshape(1, -1)
        v = pgvector_quantize(v) if self.quantize else v
        if student in self._row:
            r = self._row.pop(student)
            self.index.remove_ids(np.array([r], dtype=np.int64))
            del self.keys[r]
            self._row = {key: i for i, key in enumerate(self.keys)}
        self.index.add(v)
        self._row[student] = len(self.keys)
        self.keys.append(student)


def student_neighbours_of(student: str, keys: Sequence[str], vectors, *, k: int = DEFAULT_K,
                          quantize: bool = True, device: Optional[int] = None,
                          index: Optional[StudentIndex] = None):
    """One student's rows (the similarity worker's compute_similarity).  Pass a
    resident ``StudentIndex`` to avoid uploading the matrix on every event."""
    if index is None:
        index = StudentIndex(keys, vectors, quantize=quantize, device=device)
    return index.neighbours_of(student, k)


def neighbour_bonus(neighbours, checkouts, weight: float = 0.2, top: int = 5):
    """The social term of the reference's ranking formula (scoring.py:116-119,
    ``social_boost_weight * neighbour_recent``) as the ``bonus=`` lists of
    ``FAISS.recommend_for_profiles``: ``{a: {book_id: float32(weight) *
    float32(count)}}``.

    ``neighbours`` are ``(a, b, sim)`` rows as ``student_neighbours`` /
    ``StudentIndex.neighbours`` return them; per student a the ``top`` rows of
    the greatest sim are kept (candidate_builder.py:395's ``ORDER BY sim DESC
    LIMIT 5``; an equal sim keeps the earlier row).  ``checkouts`` are
    ``(student, book_id)`` rows the caller has already cut to its recency
    window; ``count`` is the number of those rows whose student is one of a's
    kept neighbours, a repeated row counted again (the loop at
    candidate_builder.py:410-412).  A student none of whose neighbours checked
    anything out has no entry.  Plain host code: a sort of a few rows per
    student."""
    rows_of = {}
    for a, b, sim in neighbours:
        rows_of.setdefault(a, []).append((float(sim), b))
    books_of = {}
    for student, book in checkouts:
        books_of.setdefault(student, []).append(book)
    w = np.float32(weight)
    out = {}
    for a, rows in rows_of.items():
        order = sorted(range(len(rows)), key=lambda i: -rows[i][0])  # stable: ties keep their order
        kept = []
        for i in order[:int(top)]:
            if rows[i][1] not in kept:
                kept.append(rows[i][1])
        counts = {}
        for b in kept:
            for book in books_of.get(b, ()):
                counts[book] = counts.get(book, 0) + 1
        if counts:
            out[a] = {book: w * np.float32(c) for book, c in counts.items()}
    return out
