"""faiss-compatible flat indexes backed by the MI355X engine (libvsearch.so).

Drop-in for the subset of faiss-cpu 1.11.0 (/root/reference/poetry.lock:866-867,
not vendored) that the reference reaches through LangChain's ``FAISS`` store:

* ``IndexFlatL2(d)`` / ``IndexFlatIP(d)`` — built by ``FAISS.from_texts``
  (src/ingestion_service/pipeline.py:359, src/incremental_workers/book_vector/main.py:121,469)
* ``index.add`` (via ``FAISS.add_texts``, pipeline.py:363, book_vector/main.py:148)
* ``index.search`` (the only search call, inside
  ``similarity_search_with_score_by_vector``; reached from
  src/recommendation_api/mcp_book_server.py:142, candidate_builder.py:187,321, service.py:529,627)
* ``index.ntotal`` (pipeline.py:186,524; book_vector/main.py:162-170,349-410)
* ``index.reconstruct(i)`` (candidate_builder.py:166-168, service.py:490-494)
* ``index.remove_ids`` (via ``FAISS.delete``)
* ``write_index`` / ``read_index`` (via ``save_local`` / ``load_local``)
* ``normalize_L2`` (LangChain's ``normalize_L2=True`` option)
* ``index.search(x, k, params=SearchParameters(sel=IDSelector...))`` — the k
  nearest rows among the selected labels, in place of the reference's
  search-``k * 2``-then-drop loops (candidate_builder.py:187-203,
  service.py:529-542,627-640)
* ``index.range_search(x, thresh)`` — every row within a radius, in place of
  the reference's thresholds applied after a k-bounded search
  (graph_refresher/main.py:339-354, mcp_book_server.py:818-896)
* ``index.range_selfjoin(min_sim)`` — every stored pair at or above a cosine
  threshold (the student graph without its ``LIMIT 15``,
  graph_refresher/main.py:339-354)
* ``index.search(x, k, exclude=...)``, ``index.mean_rows(profiles)`` and
  ``index.search_profiles(profiles, k)`` — the reference's per-student
  candidate path (reconstruct the rated books, weighted mean, search, drop the
  books already read: candidate_builder.py:138-203) for many students in one
  call, every query with its own exclusion list
* ``index.search_mmr(x, k, fetch_k, lambda_mult)`` and ``index.mmr_select`` —
  LangChain's maximal-marginal-relevance re-rank of the ``fetch_k`` nearest
  rows (``FAISS.max_marginal_relevance_search*``), on the device instead of
  ``fetch_k`` reconstructs and a Python loop per query

Argument checks mirror faiss's python wrapper (``assert d == self.d``,
``assert k > 0``); library failures raise ``RuntimeError`` subclasses.
The rows live in HBM of one device; there is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import os
import struct

import numpy as np

from . import _lib
from ._lib import METRIC_INNER_PRODUCT, METRIC_L2, VSearchError

__all__ = [
    "METRIC_INNER_PRODUCT",
    "METRIC_L2",
    "Index",
    "IndexFlat",
    "IndexFlatIP",
    "IndexFlatL2",
    "IDSelector",
    "IDSelectorAll",
    "IDSelectorAnd",
    "IDSelectorArray",
    "IDSelectorBatch",
    "IDSelectorBitmap",
    "IDSelectorNot",
    "IDSelectorOr",
    "IDSelectorRange",
    "SearchParameters",
    "Selector",
    "selector_bitmap",
    "exclusion_csr",
    "profile_csr",
    "examples_csr",
    "examples_stats",
    "bonus_csr",
    "bonus_stats",
    "gather_picks",
    "normalize_L2",
    "read_index",
    "write_index",
    "default_device",
]


def default_device() -> int:
    """Device used by indexes created without an explicit ``device``: $VS_DEVICE,
    else $LOCAL_RANK (one process per GPU), else 0."""
    for var in ("VS_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(var)
        if v is not None and v.strip() != "":
            return int(v)
    return 0


def _as_f32_rows(x, d=None):
    x = np.ascontiguousarray(x, dtype="float32")
    if x.ndim != 2:
        raise ValueError(f"expected a 2-D array, got shape {x.shape}")
    if d is not None:
        assert x.shape[1] == d
    return x


class IDSelectorBatch:
    """faiss.IDSelectorBatch: a set of labels (duplicates collapse)."""

    def __init__(self, ids):
        self.ids = np.unique(np.ascontiguousarray(ids, dtype="int64").ravel())

    def is_member(self, i: int) -> bool:
        return bool(np.isin(i, self.ids))


class IDSelector:
    """faiss.IDSelector: a predicate over labels.  ``is_member(i)`` as faiss;
    ``members(labels)`` is the same over an int64 array (a bool array)."""

    def members(self, labels: np.ndarray) -> np.ndarray:
        raise NotImplementedError

    def is_member(self, i: int) -> bool:
        return bool(self.members(np.asarray([i], dtype=np.int64))[0])


def _members(sel, labels: np.ndarray) -> np.ndarray:
    if hasattr(sel, "members"):
        return np.asarray(sel.members(labels), dtype=bool)
    if isinstance(sel, IDSelectorBatch):
        return np.isin(labels, sel.ids)
    return np.fromiter((bool(sel.is_member(int(i))) for i in labels), dtype=bool,
                       count=len(labels))


class IDSelectorAll(IDSelector):
    """faiss.IDSelectorAll: every label."""

    def members(self, labels):
        return np.ones(len(labels), dtype=bool)


class IDSelectorRange(IDSelector):
    """faiss.IDSelectorRange: labels in [imin, imax) (half-open, as faiss)."""

    def __init__(self, imin: int, imax: int, assume_sorted: bool = False):
        self.imin = int(imin)
        self.imax = int(imax)
        self.assume_sorted = bool(assume_sorted)

    def members(self, labels):
        labels = np.asarray(labels, dtype=np.int64)
        return (labels >= self.imin) & (labels < self.imax)


class IDSelectorArray(IDSelector):
    """faiss.IDSelectorArray: the labels of an array (duplicates allowed)."""

    def __init__(self, ids):
        self.ids = np.ascontiguousarray(ids, dtype="int64").ravel()

    def members(self, labels):
        return np.isin(np.asarray(labels, dtype=np.int64), self.ids)


class IDSelectorBitmap(IDSelector):
    """faiss.IDSelectorBitmap: label i is selected iff bit (i & 7) of byte
    (i >> 3) is set; n is the number of bits given (labels past it are not
    selected)."""

    def __init__(self, n: int, bitmap):
        self.n = int(n)
        self.bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8).ravel()
        assert self.bitmap.size * 8 >= self.n

    def members(self, labels):
        labels = np.asarray(labels, dtype=np.int64)
        ok = (labels >= 0) & (labels < self.n)
        safe = np.where(ok, labels, 0)
        if self.bitmap.size == 0:
            return np.zeros(len(labels), dtype=bool)
        bits = (self.bitmap[safe >> 3] >> (safe & 7).astype(np.uint8)) & 1
        return ok & (bits != 0)


class IDSelectorNot(IDSelector):
    """faiss.IDSelectorNot."""

    def __init__(self, sel):
        self.sel = sel

    def members(self, labels):
        return ~_members(self.sel, labels)


class IDSelectorAnd(IDSelector):
    """faiss.IDSelectorAnd."""

    def __init__(self, lhs, rhs):
        self.lhs = lhs
        self.rhs = rhs

    def members(self, labels):
        return _members(self.lhs, labels) & _members(self.rhs, labels)


class IDSelectorOr(IDSelector):
    """faiss.IDSelectorOr."""

    def __init__(self, lhs, rhs):
        self.lhs = lhs
        self.rhs = rhs

    def members(self, labels):
        return _members(self.lhs, labels) | _members(self.rhs, labels)


def selector_bitmap(sel, ntotal: int, id_base: int = 0) -> np.ndarray:
    """The label bitmap of a selector tree for an index of ``ntotal`` rows whose
    labels start at ``id_base``: uint8, (ntotal + 7) // 8 bytes, bit i (faiss
    IDSelectorBitmap layout) set iff ``sel.is_member(id_base + i)``."""
    ntotal = int(ntotal)
    labels = np.arange(int(id_base), int(id_base) + ntotal, dtype=np.int64)
    mask = _members(sel, labels) if ntotal else np.zeros(0, dtype=bool)
    return np.packbits(mask, bitorder="little")


def exclusion_csr(exclude, n: int):
    """Per-query label lists as a CSR: (offs int64 (n + 1), labels int64).

    ``exclude`` is a sequence of n label sequences (any of them empty), or an
    ``(offs, labels)`` pair already in that form; ``None`` is n empty lists."""
    n = int(n)
    if exclude is None:
        return np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    # a pair of arrays whose first has n + 1 entries from 0 to len(second) is the
    # CSR form (two label lists for n == 2 would have to look exactly like that)
    if (isinstance(exclude, tuple) and len(exclude) == 2
            and all(isinstance(e, np.ndarray) and e.ndim == 1 for e in exclude)
            and exclude[0].size == n + 1 and exclude[0][0] == 0
            and exclude[0][-1] == exclude[1].size):
        offs = np.ascontiguousarray(exclude[0], dtype=np.int64)
        labels = np.ascontiguousarray(exclude[1], dtype=np.int64).ravel()
        if offs[0] != 0 or np.any(np.diff(offs) < 0) or offs[-1] != labels.size:
            raise ValueError("exclude: offsets must rise from 0 to len(labels)")
        return offs, labels
    lists = [np.asarray(e if e is not None else (), dtype=np.int64).ravel() for e in exclude]
    if len(lists) != n:
        raise ValueError(f"exclude: expected {n} lists, got {len(lists)}")
    offs = np.zeros(n + 1, dtype=np.int64)
    if n:
        np.cumsum([e.size for e in lists], out=offs[1:])
    labels = np.concatenate(lists) if n and offs[-1] else np.zeros(0, dtype=np.int64)
    return offs, np.ascontiguousarray(labels, dtype=np.int64)


def profile_csr(profiles):
    """A sequence of ``(labels, weights)`` profiles as a CSR: (offs int64
    (n + 1), labels int64, weights float32)."""
    labs, wts = [], []
    for p in profiles:
        l, w = p
        l = np.asarray(l, dtype=np.int64).ravel()
        w = np.asarray(w, dtype=np.float32).ravel()
        if l.size != w.size:
            raise ValueError("profile: as many weights as labels")
        labs.append(l)
        wts.append(w)
    n = len(labs)
    offs = np.zeros(n + 1, dtype=np.int64)
    if n:
        np.cumsum([l.size for l in labs], out=offs[1:])
    labels = np.concatenate(labs) if n else np.zeros(0, dtype=np.int64)
    weights = np.concatenate(wts) if n else np.zeros(0, dtype=np.float32)
    return (offs, np.ascontiguousarray(labels, dtype=np.int64),
            np.ascontiguousarray(weights, dtype=np.float32))


def examples_csr(examples, n: int | None = None, d: int | None = None):
    """Per-user example lists as a CSR for ``search_examples``: ``(offs, labels,
    vectors)`` with offs int64 (n + 1) and exactly one of labels (int64) and
    vectors (float32, (offs[-1], d)) not None.

    ``examples`` is a sequence of per-user lists of labels, or of per-user 2-D
    float arrays (the vector form; an empty list may stand for a user without
    examples in either form).  ``None`` is n empty label lists."""
    if examples is None:
        if n is None:
            raise ValueError("examples: None needs the number of users")
        return np.zeros(int(n) + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), None
    items = list(examples)
    if n is not None and len(items) != int(n):
        raise ValueError(f"examples: expected {int(n)} lists, got {len(items)}")
    vec = [isinstance(e, np.ndarray) and e.ndim == 2 and e.dtype.kind == "f" for e in items]
    empty = [e is None or np.size(e) == 0 for e in items]
    if any(vec) and not all(v or z for v, z in zip(vec, empty)):
        raise ValueError("examples: every user's examples must be labels, or every user's vectors")
    offs = np.zeros(len(items) + 1, dtype=np.int64)
    if any(vec):
        dd = int(d) if d is not None else next(e.shape[1] for e, v in zip(items, vec) if v)
        rows = [np.ascontiguousarray(e, dtype=np.float32) if v else np.zeros((0, dd), np.float32)
                for e, v in zip(items, vec)]
        if any(r.shape[1] != dd for r in rows):
            raise ValueError(f"examples: vectors must have {dd} columns")
        np.cumsum([r.shape[0] for r in rows], out=offs[1:])
        return offs, None, np.ascontiguousarray(np.concatenate(rows, axis=0), dtype=np.float32)
    lists = [np.asarray(e if e is not None else (), dtype=np.int64).ravel() for e in items]
    if items:
        np.cumsum([l.size for l in lists], out=offs[1:])
    labels = np.concatenate(lists) if items and offs[-1] else np.zeros(0, dtype=np.int64)
    return offs, np.ascontiguousarray(labels, dtype=np.int64), None


def examples_stats(reset: bool = False):
    """(users searched, rounds run, users searched again) of the example
    searches of this process since the last reset."""
    a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().vs_examples_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                             1 if reset else 0), "vs_examples_stats")
    return a.value, b.value, c.value


def gather_picks(D, I, pos, metric: int):
    """The entries of a search's (D, I) at the positions ``pos`` (``mmr_select``'s
    result; -1 = no pick) as (D float32, I int64) of pos's shape, padded the way
    a search pads: (+FLT_MAX for L2 | -FLT_MAX for inner product, -1)."""
    D = np.asarray(D, dtype=np.float32)
    I = np.asarray(I, dtype=np.int64)
    pos = np.asarray(pos)
    fmax = np.finfo(np.float32).max
    pad = np.float32(fmax if metric == METRIC_L2 else -fmax)
    if D.shape[1] == 0:
        return (np.full(pos.shape, pad, dtype=np.float32), np.full(pos.shape, -1, dtype=np.int64))
    safe = np.where(pos >= 0, pos, 0).astype(np.int64)
    Dp = np.where(pos >= 0, np.take_along_axis(D, safe, axis=1), pad).astype(np.float32)
    Ip = np.where(pos >= 0, np.take_along_axis(I, safe, axis=1), -1).astype(np.int64)
    return Dp, Ip


def _ptr(a: np.ndarray):
    return a.ctypes.data if a.size else None


class SearchParameters:
    """faiss.SearchParameters: ``sel`` restricts a search to the selected labels
    (an IDSelector tree, or a ``Selector`` built once by ``index.selector``)."""

    def __init__(self, sel=None):
        self.sel = sel


class Selector:
    """Device handle of a selection of one index (``IndexFlat.selector``):
    reusable across searches until the index changes (add, remove_ids, reset),
    after which searching with it raises RuntimeError ("stale selector")."""

    def __init__(self, index: "IndexFlat", bitmap: np.ndarray, nbits: int):
        self._lib = index._lib
        self._h = ctypes.c_void_p()
        self.index = index
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8)
        assert bitmap.size * 8 >= nbits
        _lib.check(self._lib.vs_selector_create(index._h, bitmap.ctypes.data if bitmap.size else None,
                                                int(nbits), None, ctypes.byref(self._h)),
                   "vs_selector_create")
        n = ctypes.c_int64(0)
        _lib.check(self._lib.vs_selector_count(self._h, ctypes.byref(n)), "vs_selector_count")
        self.count = int(n.value)

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is None or not h.value:
            return
        try:
            self._lib.vs_selector_destroy(h)
        except Exception:  # interpreter shutdown: the library may be gone
            pass
        h.value = None

    def __del__(self):
        self.close()


def group_ids(keys) -> np.ndarray:
    """Group keys factorised to the int32 ids of a grouping: an integer array
    passes through (values >= -1; -1 is "this row is its own group"); any other
    sequence of hashables gets dense ids 0, 1, ... in order of first
    appearance, equal keys equal ids, and ``None`` gives -1."""
    if isinstance(keys, np.ndarray) and keys.dtype.kind in "iu":
        ids = keys.ravel()
        if ids.size and (ids.min() < -1 or ids.max() > np.iinfo(np.int32).max):
            raise ValueError("group_ids: integer keys must lie in [-1, 2^31)")
        return np.ascontiguousarray(ids, dtype=np.int32)
    keys = list(keys)
    if keys and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in keys):
        return group_ids(np.asarray(keys, dtype=np.int64))
    seen: dict = {}
    out = np.empty(len(keys), dtype=np.int32)
    for i, v in enumerate(keys):
        out[i] = -1 if v is None else seen.setdefault(v, len(seen))
    return out


class Grouping:
    """Device handle of a grouping of one index (``IndexFlat.grouping``): one
    group id per label.  Reusable across ``search_distinct`` calls until the
    index changes (add, remove_ids, reset), after which searching with it
    raises RuntimeError ("stale grouping").  ``.groups`` is the number of
    distinct groups, every row that is its own group counted as one."""

    def __init__(self, index: "IndexFlat", ids: np.ndarray):
        self._lib = index._lib
        self._h = ctypes.c_void_p()
        self.index = index
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        _lib.check(self._lib.vs_grouping_create(index._h, _ptr(ids), int(ids.size), None,
                                                ctypes.byref(self._h)), "vs_grouping_create")
        n = ctypes.c_int64(0)
        _lib.check(self._lib.vs_grouping_groups(self._h, ctypes.byref(n)), "vs_grouping_groups")
        self.groups = int(n.value)

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is None or not h.value:
            return
        try:
            self._lib.vs_grouping_destroy(h)
        except Exception:  # interpreter shutdown: the library may be gone
            pass
        h.value = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def distinct_plan(k: int, metric: int, raw: bool, live: int):
    """The windows (raw entries per query) of a distinct search for k over
    ``live`` rows, round by round (vs_distinct_plan; touches no device)."""
    lib = _lib.load()
    out = np.zeros(64, dtype=np.int64)
    n = lib.vs_distinct_plan(int(k), int(metric), 1 if raw else 0, int(live), out.ctypes.data,
                             out.size)
    _lib.check(min(n, 0), "vs_distinct_plan")
    return [int(v) for v in out[:n]]


def distinct_stats(reset: bool = False):
    """(queries searched, rounds run, queries searched again) of the distinct
    searches of this process since the last reset."""
    a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().vs_distinct_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                             1 if reset else 0), "vs_distinct_stats")
    return a.value, b.value, c.value


MAX_WHERE_COLUMNS = 4


def where_arrays(where, ncol: int, nq: int):
    """The arrays of ``vs_search_where`` for ``nq`` queries over ``ncol``
    numeric columns: ``(lo, hi, masks)`` = float32 (nq, ncol), float32
    (nq, ncol), uint64 (nq, 3) with any_of, all_of, none_of.

    ``where`` is one predicate for every query or a sequence of ``nq`` of them.
    A predicate is ``None`` (no test) or a mapping with the optional keys
    ``"lo"`` / ``"hi"`` (``ncol`` values, ``None`` = unbounded: the closed
    range a column must lie in) and ``"any_of"`` / ``"all_of"`` / ``"none_of"``
    (tag bit masks).  An ``(lo, hi, masks)`` triple of arrays of those shapes
    passes through."""
    ncol, nq = int(ncol), int(nq)
    if isinstance(where, tuple) and len(where) == 3 and not isinstance(where[0], (dict, type(None))):
        lo = np.ascontiguousarray(where[0], dtype=np.float32).reshape(nq, ncol)
        hi = np.ascontiguousarray(where[1], dtype=np.float32).reshape(nq, ncol)
        masks = np.ascontiguousarray(where[2], dtype=np.uint64).reshape(nq, 3)
    else:
        preds = [where] * nq if where is None or isinstance(where, dict) else list(where)
        if len(preds) != nq:
            raise ValueError(f"where: {len(preds)} predicates for {nq} queries")
        lo = np.full((nq, ncol), -np.inf, dtype=np.float32)
        hi = np.full((nq, ncol), np.inf, dtype=np.float32)
        masks = np.zeros((nq, 3), dtype=np.uint64)
        for q, p in enumerate(preds):
            if p is None:
                continue
            unknown = set(p) - {"lo", "hi", "any_of", "all_of", "none_of"}
            if unknown:
                raise ValueError(f"where: unknown keys {sorted(unknown)}")
            for key, arr, dflt in (("lo", lo, -np.inf), ("hi", hi, np.inf)):
                vals = p.get(key)
                if vals is None:
                    continue
                vals = list(vals)
                if len(vals) != ncol:
                    raise ValueError(f"where: {key} holds {len(vals)} values for {ncol} columns")
                arr[q] = [dflt if v is None else v for v in vals]
            for j, key in enumerate(("any_of", "all_of", "none_of")):
                masks[q, j] = np.uint64(int(p.get(key, 0)) & (2**64 - 1))
    if np.isnan(lo).any() or np.isnan(hi).any():
        raise ValueError("where: a NaN bound")
    return lo, hi, masks


class Attributes:
    """Device handle of the attributes of one index (``IndexFlat.attributes``):
    up to four float32 columns and one 64-bit tag word per label.  Reusable
    across ``search_where`` calls until the index changes (add, remove_ids,
    reset), after which searching with it raises RuntimeError ("stale
    attributes"); ``index.update`` leaves it valid."""

    def __init__(self, index: "IndexFlat", columns, tags=None):
        self._lib = index._lib
        self._h = ctypes.c_void_p()
        self.index = index
        cols = np.zeros((0, 0), dtype=np.float32) if columns is None else \
            np.ascontiguousarray(columns, dtype=np.float32)
        if cols.ndim == 1:
            cols = cols.reshape(1, -1) if cols.size else cols.reshape(0, 0)
        if cols.ndim != 2 or cols.shape[0] > MAX_WHERE_COLUMNS:
            raise ValueError(f"attributes: at most {MAX_WHERE_COLUMNS} columns of one value per label")
        self.ncol = int(cols.shape[0])
        if tags is not None:
            tags = np.ascontiguousarray(tags, dtype=np.uint64).reshape(-1)
        n = int(cols.shape[1]) if self.ncol else (int(tags.size) if tags is not None
                                                  else index.ntotal)
        if tags is not None and tags.size != n:
            raise ValueError(f"attributes: {tags.size} tags for {n} labels")
        self.n = n
        _lib.check(self._lib.vs_attrs_create(index._h, self.ncol, _ptr(cols),
                                             _ptr(tags) if tags is not None else None, n, None,
                                             ctypes.byref(self._h)), "vs_attrs_create")

    def count(self, where, nq: int | None = None) -> np.ndarray:
        """The live rows that pass each predicate (int64; ``where`` as in
        ``where_arrays``: one predicate, or a sequence of them)."""
        if nq is None:
            nq = 1 if where is None or isinstance(where, dict) else \
                (np.asarray(where[2]).reshape(-1, 3).shape[0] if isinstance(where, tuple)
                 else len(where))
        lo, hi, masks = where_arrays(where, self.ncol, nq)
        out = np.zeros(nq, dtype=np.int64)
        _lib.check(self._lib.vs_attrs_count(self._h, _ptr(lo), _ptr(hi), _ptr(masks), nq,
                                            _ptr(out), None), "vs_attrs_count")
        return out

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is None or not h.value:
            return
        try:
            self._lib.vs_attrs_destroy(h)
        except Exception:  # interpreter shutdown: the library may be gone
            pass
        h.value = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def where_plan(k: int, metric: int, raw: bool, live: int):
    """The windows of a where search for k over ``live`` rows, round by round,
    then 0 when what they leave goes to the scan (vs_where_plan; touches no
    device)."""
    lib = _lib.load()
    out = np.zeros(64, dtype=np.int64)
    n = lib.vs_where_plan(int(k), int(metric), 1 if raw else 0, int(live), out.ctypes.data,
                          out.size)
    _lib.check(min(n, 0), "vs_where_plan")
    return [int(v) for v in out[:n]]


def where_stats(reset: bool = False):
    """(queries searched, window rounds run, queries searched again, queries
    answered by the scan, rows the scan's streaming kernel loaded) of the
    where searches of this process since the last reset."""
    v = [ctypes.c_int64(0) for _ in range(5)]
    _lib.check(_lib.load().vs_where_stats(*[ctypes.byref(x) for x in v], 1 if reset else 0),
               "vs_where_stats")
    return tuple(x.value for x in v)


MAX_BOOST_TAGS = 4
BOOST_KINDS = {"near": 1, "ramp": 2}


def boost_arrays(boost, ncol: int, nq: int):
    """The arrays of ``vs_search_boost`` for ``nq`` queries over ``ncol``
    numeric columns: ``(kinds, params, tag_masks, tag_bonus)`` = int32
    (nq, ncol), float32 (nq, ncol, 4) holding t, s, w, miss, uint64 (nq, 4),
    float32 (nq, 4).

    ``boost`` is one spec for every query or a sequence of ``nq`` of them.  A
    spec is ``None`` (no boost) or a mapping with the optional keys
    ``"columns"`` — one entry per column: ``None``, ``("near", t, s, w[, miss])``
    = ``w * max(0, 1 - |v - t| / s)`` or ``("ramp", t, s, w[, miss])`` =
    ``w * min(1, max(0, (v - t) / s))``, ``miss`` (default 0) the term of a NaN
    value — and ``"tags"`` — up to four ``(mask, bonus)`` pairs, ``bonus`` added
    when the row's tag word shares a bit with ``mask``.  A 4-tuple of arrays of
    those shapes passes through."""
    ncol, nq = int(ncol), int(nq)
    if isinstance(boost, tuple) and len(boost) == 4 and isinstance(boost[0], np.ndarray):
        kinds = np.ascontiguousarray(boost[0], dtype=np.int32).reshape(nq, ncol)
        params = np.ascontiguousarray(boost[1], dtype=np.float32).reshape(nq, ncol, 4)
        tag_masks = np.ascontiguousarray(boost[2], dtype=np.uint64).reshape(nq, MAX_BOOST_TAGS)
        tag_bonus = np.ascontiguousarray(boost[3], dtype=np.float32).reshape(nq, MAX_BOOST_TAGS)
    else:
        specs = [boost] * nq if boost is None or isinstance(boost, dict) else list(boost)
        if len(specs) != nq:
            raise ValueError(f"boost: {len(specs)} specs for {nq} queries")
        kinds = np.zeros((nq, ncol), dtype=np.int32)
        params = np.zeros((nq, ncol, 4), dtype=np.float32)
        params[:, :, 1] = 1.0
        tag_masks = np.zeros((nq, MAX_BOOST_TAGS), dtype=np.uint64)
        tag_bonus = np.zeros((nq, MAX_BOOST_TAGS), dtype=np.float32)
        for q, sp in enumerate(specs):
            if sp is None:
                continue
            unknown = set(sp) - {"columns", "tags"}
            if unknown:
                raise ValueError(f"boost: unknown keys {sorted(unknown)}")
            cols = sp.get("columns")
            if cols is not None:
                cols = list(cols)
                if len(cols) != ncol:
                    raise ValueError(f"boost: columns holds {len(cols)} entries for {ncol} columns")
                for c, term in enumerate(cols):
                    if term is None:
                        continue
                    term = tuple(term)
                    if len(term) not in (4, 5) or term[0] not in BOOST_KINDS:
                        raise ValueError("boost: a column term is None, (\"near\", t, s, w[, miss]) "
                                         "or (\"ramp\", t, s, w[, miss])")
                    kinds[q, c] = BOOST_KINDS[term[0]]
                    params[q, c, :3] = term[1:4]
                    params[q, c, 3] = term[4] if len(term) == 5 else 0.0
            tags = list(sp.get("tags") or ())
            if len(tags) > MAX_BOOST_TAGS:
                raise ValueError(f"boost: more than {MAX_BOOST_TAGS} tag terms")
            for j, (mask, bonus) in enumerate(tags):
                tag_masks[q, j] = np.uint64(int(mask) & (2**64 - 1))
                tag_bonus[q, j] = bonus
    if not (np.isfinite(params).all() and np.isfinite(tag_bonus).all()):
        raise ValueError("boost: a parameter that is not finite")
    if not (params[:, :, 1] > 0).all():
        raise ValueError("boost: a scale s must be > 0")
    if ((kinds < 0) | (kinds > 2)).any():
        raise ValueError("boost: a kind must be 0, 1 or 2")
    return kinds, params, tag_masks, tag_bonus


def boost_eval(columns, tags, boost, nq: int | None = None):
    """``(b, bounds)``: the boost of every (query, row) as the device computes
    it, float32 (nq, nrows), and each query's ``(L, U)`` with ``L <= b <= U``,
    float32 (nq, 2) (vs_boost_eval; touches no device).  ``columns``: up to
    four sequences of one value per row (NaN: unknown) or ``None``; ``tags``:
    one 64-bit word per row or ``None``; ``boost`` as in ``boost_arrays``."""
    cols = np.zeros((0, 0), dtype=np.float32) if columns is None else \
        np.ascontiguousarray(columns, dtype=np.float32)
    if cols.ndim == 1:
        cols = cols.reshape(1, -1) if cols.size else cols.reshape(0, 0)
    if cols.ndim != 2 or cols.shape[0] > MAX_WHERE_COLUMNS:
        raise ValueError(f"boost_eval: at most {MAX_WHERE_COLUMNS} columns of one value per row")
    ncol = int(cols.shape[0])
    if tags is not None:
        tags = np.ascontiguousarray(tags, dtype=np.uint64).reshape(-1)
    nrows = int(cols.shape[1]) if ncol else (int(tags.size) if tags is not None else 0)
    if tags is not None and tags.size != nrows:
        raise ValueError(f"boost_eval: {tags.size} tags for {nrows} rows")
    if nq is None:
        nq = 1 if boost is None or isinstance(boost, dict) else \
            (int(np.asarray(boost[2]).reshape(-1, MAX_BOOST_TAGS).shape[0])
             if isinstance(boost, tuple) else len(boost))
    kinds, params, tag_masks, tag_bonus = boost_arrays(boost, ncol, nq)
    b = np.zeros((nq, nrows), dtype=np.float32)
    bounds = np.zeros((nq, 2), dtype=np.float32)
    _lib.check(_lib.load().vs_boost_eval(
        ncol, _ptr(cols), _ptr(tags) if tags is not None else None, nrows, _ptr(kinds),
        _ptr(params), _ptr(tag_masks), _ptr(tag_bonus), nq, _ptr(b), _ptr(bounds)),
        "vs_boost_eval")
    return b, bounds


def boost_stats(reset: bool = False):
    """(queries searched, window rounds run, queries searched again, queries
    answered by the scan) of the boosted searches of this process since the
    last reset."""
    v = [ctypes.c_int64(0) for _ in range(4)]
    _lib.check(_lib.load().vs_boost_stats(*[ctypes.byref(x) for x in v], 1 if reset else 0),
               "vs_boost_stats")
    return tuple(x.value for x in v)


MAX_BONUS_LIST = 1024


def bonus_csr(bonus, n: int):
    """Per-query bonus lists as a CSR: ``(offs int64 (n + 1), labels int64,
    values float32)``, checked as ``vs_search_bonus`` checks them.

    ``bonus`` is ``None`` (n empty lists), a sequence of n entries — each a
    mapping ``label -> value``, a pair ``(labels, values)`` or ``None`` — or an
    ``(offs, labels, values)`` triple of arrays already in that form.  Every
    value must be finite, the labels of one list distinct, and a list holds at
    most ``MAX_BONUS_LIST`` entries; labels the index does not hold are
    ignored by the search."""
    n = int(n)
    if bonus is None:
        return (np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64),
                np.zeros(0, dtype=np.float32))
    if (isinstance(bonus, tuple) and len(bonus) == 3
            and all(isinstance(e, np.ndarray) and e.ndim == 1 for e in bonus)
            and bonus[0].size == n + 1):
        offs = np.ascontiguousarray(bonus[0], dtype=np.int64)
        labels = np.ascontiguousarray(bonus[1], dtype=np.int64)
        vals = np.ascontiguousarray(bonus[2], dtype=np.float32)
        if (offs[0] != 0 or np.any(np.diff(offs) < 0) or offs[-1] != labels.size
                or labels.size != vals.size):
            raise ValueError("bonus: offsets must rise from 0 to len(labels) == len(values)")
    else:
        if isinstance(bonus, dict):
            raise ValueError("bonus: one entry per query (a dict, a (labels, values) pair or None)")
        entries = list(bonus)
        if len(entries) != n:
            raise ValueError(f"bonus: expected {n} lists, got {len(entries)}")
        labs, vs = [], []
        for e in entries:
            if e is None:
                l, v = (), ()
            elif isinstance(e, dict):
                l, v = list(e.keys()), list(e.values())
            else:
                if len(e) != 2:
                    raise ValueError("bonus: a list is a dict, a (labels, values) pair or None")
                l, v = e
            l = np.asarray(l, dtype=np.int64).ravel()
            v = np.asarray(v, dtype=np.float32).ravel()
            if l.size != v.size:
                raise ValueError("bonus: as many values as labels")
            labs.append(l)
            vs.append(v)
        offs = np.zeros(n + 1, dtype=np.int64)
        if n:
            np.cumsum([l.size for l in labs], out=offs[1:])
        labels = np.ascontiguousarray(np.concatenate(labs) if n and offs[-1] else
                                      np.zeros(0, dtype=np.int64), dtype=np.int64)
        vals = np.ascontiguousarray(np.concatenate(vs) if n and offs[-1] else
                                    np.zeros(0, dtype=np.float32), dtype=np.float32)
    if not np.isfinite(vals).all():
        raise ValueError("bonus: a value that is not finite")
    if labels.size > 1:  # one sort by (query, label) for every list
        qs = np.repeat(np.arange(n, dtype=np.int64), np.diff(offs))
        order = np.lexsort((labels, qs))
        ls, qs = labels[order], qs[order]
        if np.any((ls[1:] == ls[:-1]) & (qs[1:] == qs[:-1])):
            raise ValueError("bonus: a label twice in one list")
    if n and np.diff(offs).max() > MAX_BONUS_LIST:
        raise ValueError(f"bonus: a list longer than {MAX_BONUS_LIST} entries")
    return offs, labels, vals


def bonus_stats(reset: bool = False):
    """(queries searched, listed live rows scored, queries whose base search
    carried an extra exclusion, result entries that are listed rows) of the
    bonus searches of this process since the last reset."""
    v = [ctypes.c_int64(0) for _ in range(4)]
    _lib.check(_lib.load().vs_bonus_stats(*[ctypes.byref(x) for x in v], 1 if reset else 0),
               "vs_bonus_stats")
    return tuple(x.value for x in v)


class Index:
    """Common base (faiss.Index)."""

    is_trained = True


class IndexFlat(Index):
    """Exact flat index (faiss::IndexFlat) on one GPU.

    ``dtype="bf16"`` stores rows as bf16 (round to nearest even) — half the HBM
    of fp32, for corpora that do not fit otherwise (BASELINE config 5).  Queries
    are rounded to bf16 as well and products accumulate in fp32, so the search is
    exact over the rounded vectors; against fp32 vectors it is reported as
    recall@k.  ``reconstruct`` returns the stored (rounded) values.
    """

    def __init__(self, d: int, metric: int = METRIC_L2, *, device: int | None = None,
                 dtype: str = "f32"):
        d = int(d)
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        self._device = default_device() if device is None else int(device)
        code = {"f32": _lib.DTYPE_F32, "float32": _lib.DTYPE_F32,
                "bf16": _lib.DTYPE_BF16, "bfloat16": _lib.DTYPE_BF16}[dtype]
        _lib.check(self._lib.vs_create(d, int(metric), code, self._device, ctypes.byref(self._h)),
                   "vs_create")
        self._d = d
        self._metric = int(metric)
        self._dtype = "bf16" if code == _lib.DTYPE_BF16 else "f32"
        self._id_base = 0

    # -- attributes faiss exposes -------------------------------------------------
    @property
    def d(self) -> int:
        return self._d

    @property
    def metric_type(self) -> int:
        return self._metric

    @property
    def device(self) -> int:
        return self._device

    @property
    def dtype(self) -> str:
        return self._dtype

    @property
    def ntotal(self) -> int:
        n = ctypes.c_int64(0)
        _lib.check(self._lib.vs_ntotal(self._h, ctypes.byref(n)), "vs_ntotal")
        return n.value

    def __len__(self) -> int:  # convenience; faiss has no __len__
        return self.ntotal

    def __del__(self):
        # no module-global lookups here: at interpreter exit `ctypes` may already
        # be torn down; the handle object itself is cleared in place
        h = getattr(self, "_h", None)
        if h is None or not h.value:
            return
        try:
            self._lib.vs_destroy(h)
        except Exception:  # interpreter shutdown: the library may be gone
            pass
        h.value = None

    # -- mutation ---------------------------------------------------------------------
    def add(self, x) -> None:
        """faiss Index.add: append rows (labels ntotal, ntotal+1, ...)."""
        x = _as_f32_rows(x, self._d)
        n = x.shape[0]
        if n == 0:
            return
        _lib.check(self._lib.vs_add(self._h, x.ctypes.data, n, 0, None), "vs_add")

    def add_device(self, ptr: int, n: int, stream: int = 0) -> None:
        """Append n rows already in device memory (row-major float32, stride d)."""
        _lib.check(self._lib.vs_add(self._h, ctypes.c_void_p(ptr), int(n), _lib.IN_DEVICE,
                                    ctypes.c_void_p(stream)), "vs_add")

    def update(self, labels, x) -> None:
        """In-place update (no faiss equivalent; faiss-cpu users remove and
        add): the live row with label ``labels[i]`` takes the value ``x[i]``,
        exactly as if it had been added there.  Rows do not move and labels do
        not change, so ``Selector`` and ``Grouping`` handles stay valid.  A
        label that is not live, or one given twice, raises and leaves the
        index unchanged."""
        labels = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        x = _as_f32_rows(x, self._d)
        if x.shape[0] != labels.size:
            raise ValueError(f"update: {labels.size} labels for {x.shape[0]} vectors")
        _lib.check(self._lib.vs_update_rows(self._h, labels.ctypes.data, x.ctypes.data,
                                            labels.size, 0, None), "vs_update_rows")

    def add_synthetic(self, n: int, seed: int, row0: int = 0, stream: int = 0) -> None:
        """Append the counter-based synthetic rows row0..row0+n-1 (see vsearch.synth)."""
        _lib.check(self._lib.vs_add_synthetic(self._h, int(n), ctypes.c_uint64(seed),
                                              int(row0), ctypes.c_void_p(stream)),
                   "vs_add_synthetic")

    def add_synthetic_ids(self, ids, seed: int, stream: int = 0) -> None:
        """Append the synthetic corpus rows with generator row numbers `ids`."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if ids.size:
            _lib.check(self._lib.vs_add_synthetic_ids(self._h, ids.ctypes.data, ids.size,
                                                      ctypes.c_uint64(seed),
                                                      ctypes.c_void_p(stream)),
                       "vs_add_synthetic_ids")

    def reserve(self, n: int) -> None:
        _lib.check(self._lib.vs_reserve(self._h, int(n)), "vs_reserve")

    def reset(self) -> None:
        _lib.check(self._lib.vs_reset(self._h), "vs_reset")

    def remove_ids(self, x) -> int:
        """faiss IndexFlat.remove_ids: stable compaction; returns #removed."""
        if isinstance(x, IDSelectorBatch):
            ids = x.ids
        else:
            ids = np.ascontiguousarray(x, dtype="int64")
            assert ids.ndim == 1
        nrem = ctypes.c_int64(0)
        if ids.size == 0:
            return 0
        _lib.check(self._lib.vs_remove_ids(self._h, ids.ctypes.data, ids.size,
                                           ctypes.byref(nrem)), "vs_remove_ids")
        return int(nrem.value)

    def set_engine(self, engine: str) -> None:
        """Large-batch arithmetic of fp32 indexes: "auto" (filter and verify in
        stages: the int8 plane, then the bf16 plane for what int8 cannot settle,
        then the exact fp32 engine), "fp32" (the exact fp32 MFMA engine), "i8v"
        or "bf16v" (filter and verify on that plane alone, then fp32)."""
        code = {"auto": _lib.ENGINE_AUTO, "fp32": _lib.ENGINE_FP32_MFMA,
                "bf16v": _lib.ENGINE_BF16_VERIFY, "i8v": _lib.ENGINE_I8_VERIFY}[engine]
        _lib.check(self._lib.vs_set_engine(self._h, code), "vs_set_engine")

    @property
    def filter_planes(self):
        """The filter planes of this index, in the order the staged engine runs
        them: ("i8", "bf16") for inner-product and L2 fp32 indexes (L2 as an
        augmented inner product), ("bf16",) for cosine, () for bf16 indexes
        (which search their stored values exactly)."""
        v = ctypes.c_int(0)
        _lib.check(self._lib.vs_filter_plane(self._h, ctypes.byref(v)), "vs_filter_plane")
        return tuple(n for bit, n in ((1, "i8"), (2, "bf16")) if v.value & bit)

    @property
    def notice(self) -> str:
        """The library's last notice for this index ("" if none): a filter plane
        dropped because HBM ran short while the storage grew."""
        v = self._lib.vs_notice(self._h)
        return v.decode() if v else ""

    def set_id_base(self, base: int) -> None:
        _lib.check(self._lib.vs_set_id_base(self._h, int(base)), "vs_set_id_base")
        self._id_base = int(base)

    def selector(self, sel) -> Selector:
        """The device handle of a selection: ``sel`` is an IDSelector tree over
        this index's labels.  ``.count`` is the number of selected rows."""
        if isinstance(sel, Selector):
            return sel
        ntotal = self.ntotal
        return Selector(self, selector_bitmap(sel, ntotal, self._id_base), ntotal)

    def _resolve_selector(self, sel):
        """(handle, owned): a Selector as it is, a selector tree built for this call."""
        if isinstance(sel, Selector):
            if sel.index is not self:
                raise ValueError("the Selector belongs to another index")
            return sel, False
        return self.selector(sel), True

    # -- queries -----------------------------------------------------------------------
    def search(self, x, k, *, params=None, D=None, I=None, raw: bool = False, exclude=None):
        """faiss Index.search: returns (D float32 (n,k), I int64 (n,k)).

        ``exclude`` gives every query its own list of labels to leave out: a
        sequence of n label sequences, or an ``(offs, labels)`` CSR pair
        (``exclusion_csr``).  The k nearest rows among the others come back
        (fewer than k pad with label -1); labels the index does not hold are
        ignored.  Not together with ``params.sel``.

        ``params=SearchParameters(sel=...)`` restricts the search to the selected
        labels (an IDSelector tree, built and freed in this call, or a
        ``Selector`` from ``index.selector``, reused); fewer than k selected
        rows pad with label -1.

        ``raw=True`` returns the k lexicographically best (key, label) entries
        instead of faiss's inner-product tie order (VS_RAW_ORDER; the per-shard
        half of an exact sharded search, see vsearch.sharded)."""
        x = _as_f32_rows(x)
        n, d = x.shape
        assert d == self._d
        k = int(k)
        assert k > 0
        if D is None:
            D = np.empty((n, k), dtype=np.float32)
        else:
            assert D.shape == (n, k)
        if I is None:
            I = np.empty((n, k), dtype=np.int64)
        else:
            assert I.shape == (n, k)
        sel = getattr(params, "sel", None) if params is not None else None
        if exclude is not None:
            if sel is not None:
                raise ValueError("search: pass exclude or params.sel, not both")
            offs, labels = exclusion_csr(exclude, n)
            if n == 0:
                return D, I
            _lib.check(self._lib.vs_search_excl(self._h, x.ctypes.data, n, k, offs.ctypes.data,
                                                _ptr(labels), D.ctypes.data, I.ctypes.data,
                                                _lib.RAW_ORDER if raw else 0, None),
                       "vs_search_excl")
            return D, I
        if n == 0:
            return D, I
        if sel is not None:
            handle, owned = self._resolve_selector(sel)
            try:
                _lib.check(self._lib.vs_search_sel(self._h, handle._h, x.ctypes.data, n, k,
                                                   D.ctypes.data, I.ctypes.data,
                                                   _lib.RAW_ORDER if raw else 0, None),
                           "vs_search_sel")
            finally:
                if owned:
                    handle.close()
            return D, I
        _lib.check(self._lib.vs_search(self._h, x.ctypes.data, n, k, D.ctypes.data,
                                       I.ctypes.data, _lib.RAW_ORDER if raw else 0, None),
                   "vs_search")
        return D, I

    def grouping(self, keys) -> Grouping:
        """The device handle of a grouping: ``keys`` holds one key per label
        (``ntotal`` of them): ints (-1: its own group) or any hashables
        (``None``: its own group), factorised by ``group_ids``."""
        if isinstance(keys, Grouping):
            return keys
        return Grouping(self, group_ids(keys))

    def search_distinct(self, x, k, grouping, *, exclude=None, raw: bool = False):
        """The k nearest groups, one best row per group: what ``search`` would
        return on an index that held only each group's best row (its lowest
        label among equally good ones).  ``grouping`` is a ``Grouping`` from
        ``index.grouping``, or the keys of one (built and freed in this call);
        ``exclude`` and ``raw`` as in ``search``.  Fewer than k groups among
        the allowed rows pad with label -1.  Exact for any grouping; k <= 1024."""
        x = _as_f32_rows(x)
        n, d = x.shape
        assert d == self._d
        k = int(k)
        assert k > 0
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        owned = not isinstance(grouping, Grouping)
        grp = self.grouping(grouping)
        if grp.index is not self:
            raise ValueError("the Grouping belongs to another index")
        try:
            offs, labels = (None, None) if exclude is None else exclusion_csr(exclude, n)
            _lib.check(self._lib.vs_search_distinct(
                self._h, grp._h, _ptr(x), n, k,
                offs.ctypes.data if offs is not None else None,
                _ptr(labels) if labels is not None else None, _ptr(D), _ptr(I),
                _lib.RAW_ORDER if raw else 0, None), "vs_search_distinct")
        finally:
            if owned:
                grp.close()
        return D, I

    def search_distinct_device(self, xq_ptr: int, n: int, k: int, grouping: Grouping, D_ptr: int,
                               I_ptr: int, stream: int = 0, raw: bool = False) -> None:
        """``search_distinct`` with every buffer on this index's device, on
        `stream` (the call waits for the stream after every round but the
        last; a capturing stream is refused)."""
        flags = _lib.IN_DEVICE | _lib.OUT_DEVICE | (_lib.RAW_ORDER if raw else 0)
        _lib.check(self._lib.vs_search_distinct(
            self._h, grouping._h, ctypes.c_void_p(xq_ptr), int(n), int(k), None, None,
            ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr), flags, ctypes.c_void_p(stream)),
            "vs_search_distinct")

    def attributes(self, columns, tags=None) -> Attributes:
        """The device handle of per-label attributes: ``columns`` holds up to
        four sequences of ``ntotal`` numbers (NaN: unknown; ``None``: no
        columns), ``tags`` one 64-bit word per label (``None``: all 0)."""
        if isinstance(columns, Attributes):
            return columns
        return Attributes(self, columns, tags)

    def search_where(self, x, k, attrs: Attributes, where, *, exclude=None, raw: bool = False,
                     scan: bool = False):
        """What ``search`` would return on an index that held only the rows
        that pass the query's predicate: ``where`` is one predicate for every
        query or one per query (``where_arrays``), over the columns and tags of
        ``attrs`` (``index.attributes``); ``exclude`` and ``raw`` as in
        ``search``.  Fewer than k matches pad with label -1.  ``scan=True``
        skips the windows and answers every query with the predicated scan."""
        x = _as_f32_rows(x)
        n, d = x.shape
        assert d == self._d
        k = int(k)
        assert k > 0
        if attrs.index is not self:
            raise ValueError("the Attributes belong to another index")
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        lo, hi, masks = where_arrays(where, attrs.ncol, n)
        offs, labels = (None, None) if exclude is None else exclusion_csr(exclude, n)
        flags = (_lib.RAW_ORDER if raw else 0) | (_lib.WHERE_SCAN if scan else 0)
        _lib.check(self._lib.vs_search_where(
            self._h, attrs._h, _ptr(x), n, k, _ptr(lo), _ptr(hi), _ptr(masks),
            offs.ctypes.data if offs is not None else None,
            _ptr(labels) if labels is not None else None, _ptr(D), _ptr(I), flags, None),
            "vs_search_where")
        return D, I

    def search_where_device(self, xq_ptr: int, n: int, k: int, attrs: Attributes, where,
                            D_ptr: int, I_ptr: int, stream: int = 0, raw: bool = False,
                            scan: bool = False) -> None:
        """``search_where`` with the queries and the results on this index's
        device, on `stream` (the call waits for the stream after every round; a
        capturing stream is refused).  The predicates stay host arrays."""
        lo, hi, masks = where_arrays(where, attrs.ncol, n)
        flags = (_lib.IN_DEVICE | _lib.OUT_DEVICE | (_lib.RAW_ORDER if raw else 0)
                 | (_lib.WHERE_SCAN if scan else 0))
        _lib.check(self._lib.vs_search_where(
            self._h, attrs._h, ctypes.c_void_p(xq_ptr), int(n), int(k), _ptr(lo), _ptr(hi),
            _ptr(masks), None, None, ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr), flags,
            ctypes.c_void_p(stream)), "vs_search_where")

    def search_boost(self, x, k, attrs: Attributes, boost, *, where=None, exclude=None,
                     scan: bool = False):
        """The k rows with the best boosted score, exactly: every live row is
        ranked by ``fl32(key - b)``, key the engine's key (-score for inner
        product, the squared distance for L2) and b the query's boost of the
        row's attributes (``boost_arrays``; ``boost_eval`` returns its bits),
        ties to the lower label.  D is ``score + b`` for inner product and
        ``distance - b`` for L2 (it may be negative).  ``where`` (as in
        ``search_where``) and ``exclude`` (as in ``search``) remove rows from
        the candidates.  ``scan=True`` skips the windows and answers every
        query with the boosted scan."""
        x = _as_f32_rows(x)
        n, d = x.shape
        assert d == self._d
        k = int(k)
        assert k > 0
        if attrs.index is not self:
            raise ValueError("the Attributes belong to another index")
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        kinds, params, tmasks, tbonus = boost_arrays(boost, attrs.ncol, n)
        lo, hi, masks = (None, None, None) if where is None else where_arrays(where, attrs.ncol, n)
        offs, labels = (None, None) if exclude is None else exclusion_csr(exclude, n)
        _lib.check(self._lib.vs_search_boost(
            self._h, attrs._h, _ptr(x), n, k, _ptr(kinds), _ptr(params), _ptr(tmasks), _ptr(tbonus),
            _ptr(lo) if lo is not None else None, _ptr(hi) if hi is not None else None,
            _ptr(masks) if masks is not None else None,
            offs.ctypes.data if offs is not None else None,
            _ptr(labels) if labels is not None else None, _ptr(D), _ptr(I),
            _lib.BOOST_SCAN if scan else 0, None), "vs_search_boost")
        return D, I

    def search_boost_device(self, xq_ptr: int, n: int, k: int, attrs: Attributes, boost,
                            D_ptr: int, I_ptr: int, stream: int = 0, where=None,
                            scan: bool = False) -> None:
        """``search_boost`` with the queries and the results on this index's
        device, on `stream` (the call waits for the stream after every round; a
        capturing stream is refused).  The boosts and predicates stay host
        arrays."""
        kinds, params, tmasks, tbonus = boost_arrays(boost, attrs.ncol, n)
        lo, hi, masks = (None, None, None) if where is None else where_arrays(where, attrs.ncol, n)
        flags = _lib.IN_DEVICE | _lib.OUT_DEVICE | (_lib.BOOST_SCAN if scan else 0)
        _lib.check(self._lib.vs_search_boost(
            self._h, attrs._h, ctypes.c_void_p(xq_ptr), int(n), int(k), _ptr(kinds), _ptr(params),
            _ptr(tmasks), _ptr(tbonus), _ptr(lo) if lo is not None else None,
            _ptr(hi) if hi is not None else None, _ptr(masks) if masks is not None else None,
            None, None, ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr), flags,
            ctypes.c_void_p(stream)), "vs_search_boost")

    def _bonus_call(self, x_ptr, n, k, bonus, attrs, boost, where, exclude, D_ptr, I_ptr, flags,
                    stream):
        if attrs is None:
            if boost is not None or where is not None:
                raise ValueError("search_bonus: boost= and where= need attrs=")
            kinds = params = tmasks = tbonus = lo = hi = masks = None
        else:
            if attrs.index is not self:
                raise ValueError("the Attributes belong to another index")
            kinds, params, tmasks, tbonus = boost_arrays(boost, attrs.ncol, n)
            lo, hi, masks = (None, None, None) if where is None else \
                where_arrays(where, attrs.ncol, n)
        boffs, blabels, bvals = bonus_csr(bonus, n)
        offs, labels = (None, None) if exclude is None else exclusion_csr(exclude, n)

        def p(a):
            return _ptr(a) if a is not None else None

        _lib.check(self._lib.vs_search_bonus(
            self._h, attrs._h if attrs is not None else None, x_ptr, n, k,
            boffs.ctypes.data, p(blabels), p(bvals), p(kinds), p(params), p(tmasks), p(tbonus),
            p(lo), p(hi), p(masks), offs.ctypes.data if offs is not None else None, p(labels),
            D_ptr, I_ptr, flags, stream), "vs_search_bonus")

    def search_bonus(self, x, k, bonus, *, attrs: Attributes | None = None, boost=None, where=None,
                     exclude=None, scan: bool = False):
        """The k rows with the best score after per-query, per-row bonuses,
        exactly: ``bonus`` lists per query up to 1,024 ``(label, s)`` pairs
        (``bonus_csr``), and every allowed row is ranked by
        ``fl32(fl32(key - b) - s)``, s = 0 for a row the query does not list,
        key and b as in ``search_boost`` (b = 0 without ``attrs``), ties to the
        lower label.  D is ``score + b + s`` for inner product and
        ``distance - b - s`` for L2.  ``boost`` and ``where`` need ``attrs``
        (``index.attributes``); ``exclude`` as in ``search``.  A listed row
        that fails its predicate or is excluded is not returned.  Without any
        list the answer is ``search_boost``'s (with ``attrs``) or
        ``search(raw=True)``'s, bit for bit."""
        x = _as_f32_rows(x)
        n, d = x.shape
        assert d == self._d
        k = int(k)
        assert k > 0
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        self._bonus_call(_ptr(x), n, k, bonus, attrs, boost, where, exclude, _ptr(D), _ptr(I),
                         _lib.BOOST_SCAN if scan else 0, None)
        return D, I

    def search_bonus_device(self, xq_ptr: int, n: int, k: int, bonus, D_ptr: int, I_ptr: int,
                            stream: int = 0, attrs: Attributes | None = None, boost=None,
                            where=None, exclude=None, scan: bool = False) -> None:
        """``search_bonus`` with the queries and the results on this index's
        device, on `stream` (the call waits for the stream; a capturing stream
        is refused).  The lists, boosts and predicates stay host arrays."""
        flags = _lib.IN_DEVICE | _lib.OUT_DEVICE | (_lib.BOOST_SCAN if scan else 0)
        self._bonus_call(ctypes.c_void_p(xq_ptr), int(n), int(k), bonus, attrs, boost, where,
                         exclude, ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr), flags,
                         ctypes.c_void_p(stream))

    def _examples_args(self, positive, negative):
        poffs, plab, pvec = examples_csr(positive, None, self._d)
        n = poffs.size - 1
        noffs = nlab = nvec = None
        if negative is not None:
            noffs, nlab, nvec = examples_csr(negative, n, self._d)
            if noffs[-1] == 0:
                noffs = nlab = nvec = None
        if noffs is not None and (pvec is None) != (nvec is None):
            raise ValueError("positive and negative examples must take the same form")
        return n, poffs, plab, pvec, noffs, nlab, nvec

    def _examples_call(self, n, k, poffs, plab, pvec, noffs, nlab, nvec, eoffs, elabels,
                       exclude_examples, D, I, E, flags, stream):
        op = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        pp = lambda a: _ptr(a) if a is not None else None  # noqa: E731
        if pvec is not None:
            _lib.check(self._lib.vs_search_examples_x(
                self._h, op(poffs), pp(pvec), op(noffs), pp(nvec), n, k, op(eoffs), pp(elabels),
                D, I, E, flags, stream), "vs_search_examples_x")
        else:
            _lib.check(self._lib.vs_search_examples(
                self._h, op(poffs), pp(plab), op(noffs), pp(nlab), n, k, op(eoffs), pp(elabels),
                1 if exclude_examples else 0, D, I, E, flags, stream), "vs_search_examples")

    def search_examples(self, positive, negative=None, k=10, *, exclude=None,
                        exclude_examples: bool = True, return_example: bool = False):
        """Recommendation from examples (Qdrant ``recommend`` with
        ``strategy="best_score"``): for every user the k rows nearest to ANY of
        its positive examples that no negative example is at least as near to,
        in ascending (key, label) order.  ``positive`` / ``negative`` hold one
        list of labels per user (stored rows), or one 2-D float array per user
        (the vector form); every user needs a positive, ``negative`` may be
        None.  ``exclude`` as in ``search``; ``exclude_examples`` also excludes
        a user's own example labels (label form only: vectors name no rows).
        Returns (D, I), D the score to the nearest positive; with
        ``return_example`` also E (int32), that positive's position in the
        user's list (-1 on padding).  Fewer than k such rows pad with label -1.
        Exact; k <= 1024, at most 64 positives and 64 negatives per user."""
        n, poffs, plab, pvec, noffs, nlab, nvec = self._examples_args(positive, negative)
        k = int(k)
        assert k > 0
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        E = np.empty((n, k), dtype=np.int32)
        if n:
            eoffs, elabels = (None, None) if exclude is None else exclusion_csr(exclude, n)
            self._examples_call(n, k, poffs, plab, pvec, noffs, nlab, nvec, eoffs, elabels,
                                exclude_examples, D.ctypes.data, I.ctypes.data, E.ctypes.data, 0,
                                None)
        return (D, I, E) if return_example else (D, I)

    def search_examples_device(self, positive, negative, k: int, D_ptr: int, I_ptr: int,
                               E_ptr: int = 0, *, exclude=None, exclude_examples: bool = True,
                               stream: int = 0) -> None:
        """``search_examples`` with D, I (and E, 0: not wanted) on this index's
        device, on ``stream`` (the call waits for the stream after every round;
        a capturing stream is refused).  The example lists are host lists."""
        n, poffs, plab, pvec, noffs, nlab, nvec = self._examples_args(positive, negative)
        if n == 0:
            return
        eoffs, elabels = (None, None) if exclude is None else exclusion_csr(exclude, n)
        self._examples_call(n, int(k), poffs, plab, pvec, noffs, nlab, nvec, eoffs, elabels,
                            exclude_examples, ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
                            ctypes.c_void_p(E_ptr) if E_ptr else None, _lib.OUT_DEVICE,
                            ctypes.c_void_p(stream))

    def mean_rows(self, profiles) -> np.ndarray:
        """The weighted means of stored rows, computed on the device: profile
        i is ``(labels, weights)`` and row i of the result (float32 (n, d)) is
        ``np.sum([reconstruct(l) * w ...], axis=0) / sum(weights)`` bit for bit
        (fp32, list order; the weights as float32, their sum taken in double
        and rounded once).  A label the index does not hold, an empty profile
        or a zero weight sum raise RuntimeError."""
        offs, labels, weights = profile_csr(profiles)
        n = offs.size - 1
        out = np.empty((n, self._d), dtype=np.float32)
        if n:
            _lib.check(self._lib.vs_mean_rows(self._h, offs.ctypes.data, _ptr(labels),
                                              _ptr(weights), n, out.ctypes.data, 0, None),
                       "vs_mean_rows")
        return out

    def mean_rows_device(self, profiles, out_ptr: int, stream: int = 0) -> None:
        """``mean_rows`` into a device buffer of n * d float32 on this index's
        device, stream-ordered on ``stream``."""
        offs, labels, weights = profile_csr(profiles)
        n = offs.size - 1
        if n:
            _lib.check(self._lib.vs_mean_rows(self._h, offs.ctypes.data, _ptr(labels),
                                              _ptr(weights), n, ctypes.c_void_p(out_ptr),
                                              _lib.OUT_DEVICE, ctypes.c_void_p(stream)),
                       "vs_mean_rows")

    def search_profiles(self, profiles, k, *, exclude=None, exclude_profile: bool = True,
                        raw: bool = False):
        """``search(mean_rows(profiles), k, exclude=...)`` in one call, the
        means staying on the device: returns (D, I) as ``search``.  With
        ``exclude_profile`` every profile's own labels are excluded from its
        result too (the rated books are the mean's nearest rows)."""
        offs, labels, weights = profile_csr(profiles)
        n = offs.size - 1
        k = int(k)
        assert k > 0
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        if n == 0:
            return D, I
        eoffs, elabels = (None, None) if exclude is None else exclusion_csr(exclude, n)
        _lib.check(self._lib.vs_search_profiles(
            self._h, offs.ctypes.data, _ptr(labels), _ptr(weights), n, k,
            eoffs.ctypes.data if eoffs is not None else None,
            _ptr(elabels) if elabels is not None else None, 1 if exclude_profile else 0,
            D.ctypes.data, I.ctypes.data, _lib.RAW_ORDER if raw else 0, None),
            "vs_search_profiles")
        return D, I

    def mmr_select(self, x, cand_labels, k, lambda_mult: float = 0.5) -> np.ndarray:
        """LangChain's ``maximal_marginal_relevance`` over stored rows, on the
        device: ``cand_labels`` (int64 (n, fetch_k), -1 = an empty slot that
        keeps its position) are query i's candidates, and row i of the result
        (int32 (n, k)) holds the positions into that list of the min(k,
        candidates) picks in pick order, -1 after them.  Cosines and scores
        are fp64 (include/vsearch.h, "MMR searches").  A label the index does
        not hold raises RuntimeError."""
        x = _as_f32_rows(x, self._d)
        n = x.shape[0]
        cand = np.ascontiguousarray(cand_labels, dtype=np.int64)
        if cand.ndim != 2 or cand.shape[0] != n:
            raise ValueError(f"cand_labels: expected shape ({n}, fetch_k), got {cand.shape}")
        k = int(k)
        assert k > 0
        pos = np.empty((n, k), dtype=np.int32)
        if n == 0:
            return pos
        if cand.shape[1] == 0:
            pos.fill(-1)
            return pos
        _lib.check(self._lib.vs_mmr_select(self._h, x.ctypes.data, n, cand.ctypes.data,
                                           cand.shape[1], k, float(lambda_mult), pos.ctypes.data,
                                           0, None), "vs_mmr_select")
        return pos

    def search_mmr(self, x, k, fetch_k: int = 20, lambda_mult: float = 0.5, *, params=None,
                   exclude=None):
        """``search(x, fetch_k)`` re-ranked by maximal marginal relevance, the
        candidates staying on the device: returns (D float32 (n, k), I int64
        (n, k)), the picks' faiss scores and labels in pick order, padded with
        label -1 after min(k, candidates).  ``exclude`` as in ``search``; with
        ``params=SearchParameters(sel=...)`` the candidates come from the
        selector search and ``mmr_select`` re-ranks them (not both)."""
        x = _as_f32_rows(x, self._d)
        n = x.shape[0]
        k = int(k)
        fetch_k = int(fetch_k)
        assert k > 0 and fetch_k > 0
        sel = getattr(params, "sel", None) if params is not None else None
        if sel is not None:
            if exclude is not None:
                raise ValueError("search_mmr: pass exclude or params.sel, not both")
            Dc, Ic = self.search(x, fetch_k, params=params)
            return gather_picks(Dc, Ic, self.mmr_select(x, Ic, k, lambda_mult),
                                self._metric)
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        if n == 0:
            return D, I
        offs, labels = (None, None) if exclude is None else exclusion_csr(exclude, n)
        _lib.check(self._lib.vs_search_mmr(
            self._h, x.ctypes.data, n, k, fetch_k, float(lambda_mult),
            offs.ctypes.data if offs is not None else None,
            _ptr(labels) if labels is not None else None, D.ctypes.data, I.ctypes.data, 0, None),
            "vs_search_mmr")
        return D, I

    def search_mmr_device(self, xq_ptr: int, n: int, k: int, fetch_k: int, lambda_mult: float,
                          D_ptr: int, I_ptr: int, stream: int = 0) -> None:
        """``search_mmr`` with every buffer on this index's device,
        stream-ordered on `stream`."""
        _lib.check(self._lib.vs_search_mmr(
            self._h, ctypes.c_void_p(xq_ptr), int(n), int(k), int(fetch_k), float(lambda_mult),
            None, None, ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
            _lib.IN_DEVICE | _lib.OUT_DEVICE, ctypes.c_void_p(stream)), "vs_search_mmr")

    # queries per vs_range_search call (the C-ABI's limit); larger batches are
    # searched in chunks and the parts concatenated
    _RANGE_CHUNK = 65536

    def _range_take(self, h):
        """Copies a vs_range handle out as (lims int64 (nq+1), D, I) numpy
        arrays and destroys it."""
        try:
            nq = ctypes.c_int64(0)
            total = ctypes.c_int64(0)
            _lib.check(self._lib.vs_range_size(h, ctypes.byref(nq), ctypes.byref(total)),
                       "vs_range_size")
            lims = np.empty(nq.value + 1, dtype=np.int64)
            D = np.empty(total.value, dtype=np.float32)
            I = np.empty(total.value, dtype=np.int64)
            _lib.check(self._lib.vs_range_copy(h, lims.ctypes.data,
                                               D.ctypes.data if total.value else None,
                                               I.ctypes.data if total.value else None, 0, None),
                       "vs_range_copy")
        finally:
            self._lib.vs_range_destroy(h)
        return lims, D, I

    def _range_call(self, x, thresh, sel_handle):
        """One vs_range_search call: (lims int64 (n+1), D, I) as numpy arrays."""
        n = x.shape[0]
        h = ctypes.c_void_p()
        _lib.check(self._lib.vs_range_search(self._h, sel_handle, x.ctypes.data, n,
                                             ctypes.c_float(thresh), 0, None, ctypes.byref(h)),
                   "vs_range_search")
        return self._range_take(h)

    def _range_join_call(self, q0, nq, min_sim, exclude_self, upper):
        """One vs_range_selfjoin call: (lims int64 (nq+1), S, I) as numpy arrays."""
        h = ctypes.c_void_p()
        _lib.check(self._lib.vs_range_selfjoin(self._h, int(q0), int(nq), ctypes.c_float(min_sim),
                                               1 if exclude_self else 0, 1 if upper else 0, 0,
                                               None, ctypes.byref(h)),
                   "vs_range_selfjoin")
        return self._range_take(h)

    @staticmethod
    def _range_concat(parts, n):
        """The (lims, D, I) parts of consecutive query chunks as one result of n
        queries: lims uint64 (n+1), D, I."""
        lims = np.zeros(n + 1, dtype=np.uint64)
        base, q0 = 0, 0
        for pl, _, _ in parts:
            m = len(pl) - 1
            lims[q0 + 1:q0 + m + 1] = (pl[1:] + base).astype(np.uint64)
            base += int(pl[-1])
            q0 += m
        D = np.concatenate([p[1] for p in parts]) if len(parts) > 1 else parts[0][1]
        I = np.concatenate([p[2] for p in parts]) if len(parts) > 1 else parts[0][2]
        return lims, D, I

    def range_search(self, x, thresh, *, params=None):
        """faiss Index.range_search: every row within the radius, as many as
        there are.  Returns (lims uint64 (n+1), D float32, I int64): query i's
        hits are D[lims[i]:lims[i+1]] / I[lims[i]:lims[i+1]], in ascending label
        order (faiss leaves the order unspecified).

        The comparison is faiss's strict one — L2: squared distance < thresh,
        inner product: score > thresh — decided for every row by its exact key
        (the key a search returns after rescoring), which is also what D holds.
        ``params=SearchParameters(sel=...)`` restricts the hits to the selected
        labels, as in ``search``."""
        x = _as_f32_rows(x)
        n, d = x.shape
        assert d == self._d
        thresh = float(thresh)
        if n == 0:
            return (np.zeros(1, dtype=np.uint64), np.empty(0, dtype=np.float32),
                    np.empty(0, dtype=np.int64))
        sel = getattr(params, "sel", None) if params is not None else None
        handle, owned = self._resolve_selector(sel) if sel is not None else (None, False)
        try:
            sh = handle._h if handle is not None else None
            step = self._RANGE_CHUNK
            cuts = list(range(0, n, step)) + [n]
            # the L2 key follows the call's size (fewer than 20 queries: faiss's
            # sequential sum): a short tail borrows from the chunk before it
            if len(cuts) > 2 and n - cuts[-2] < 20 < step // 2:
                cuts[-2] -= 20
            parts = [self._range_call(x[c0:c1], thresh, sh) for c0, c1 in zip(cuts, cuts[1:])]
        finally:
            if owned:
                handle.close()
        return self._range_concat(parts, n)

    def search_device(self, xq_ptr: int, n: int, k: int, D_ptr: int, I_ptr: int,
                      stream: int = 0, raw: bool = False, selector=None) -> None:
        """Device-resident search: all buffers are device pointers on this index's
        device; stream-ordered on `stream` (a hipStream_t, 0 = default stream).
        Returns once the first filter stage's count of unsettled queries is read
        (later stages are enqueued only for queries left; VS_TAIL_WAIT=0 keeps
        the call fully asynchronous)."""
        flags = _lib.IN_DEVICE | _lib.OUT_DEVICE | (_lib.RAW_ORDER if raw else 0)
        if selector is not None:
            # a Selector only: a handle built for this call could not be freed
            # before the stream has run the search
            if not isinstance(selector, Selector) or selector.index is not self:
                raise ValueError("search_device takes a Selector of this index")
            _lib.check(self._lib.vs_search_sel(self._h, selector._h, ctypes.c_void_p(xq_ptr),
                                               int(n), int(k), ctypes.c_void_p(D_ptr),
                                               ctypes.c_void_p(I_ptr), flags,
                                               ctypes.c_void_p(stream)), "vs_search_sel")
            return
        _lib.check(self._lib.vs_search(self._h, ctypes.c_void_p(xq_ptr), int(n), int(k),
                                       ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr), flags,
                                       ctypes.c_void_p(stream)), "vs_search")

    def reconstruct(self, key) -> np.ndarray:
        """faiss Index.reconstruct(key) -> float32 (d,)."""
        key = int(key)
        out = np.empty((1, self._d), dtype=np.float32)
        _lib.check(self._lib.vs_reconstruct_n(self._h, key, 1, out.ctypes.data, 0, None),
                   "vs_reconstruct_n")
        return out[0]

    def reconstruct_n(self, n0: int = 0, ni: int = -1) -> np.ndarray:
        """faiss Index.reconstruct_n(n0, ni) -> float32 (ni, d)."""
        if ni == -1:
            ni = self.ntotal - int(n0)
        out = np.empty((int(ni), self._d), dtype=np.float32)
        if ni:
            _lib.check(self._lib.vs_reconstruct_n(self._h, int(n0), int(ni), out.ctypes.data, 0,
                                                  None), "vs_reconstruct_n")
        return out

    def selfjoin(self, k: int, *, q0: int = 0, nq: int | None = None,
                 exclude_self: bool = True, min_sim: float = -np.inf):
        """Cosine self-join over stored rows [q0, q0+nq) (pgvector `<=>` semantics):
        returns (S float32 (nq,k) similarities, I int64 (nq,k) labels, -1 = none)."""
        ntotal = self.ntotal
        nq = ntotal - q0 if nq is None else int(nq)
        k = int(k)
        assert k > 0
        S = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        if nq == 0:
            return S, I
        _lib.check(self._lib.vs_selfjoin(self._h, int(q0), nq, k, 1 if exclude_self else 0,
                                         ctypes.c_float(min_sim), S.ctypes.data, I.ctypes.data,
                                         0, None), "vs_selfjoin")
        return S, I

    def _range_join_rows_call(self, rows, min_sim, exclude_self):
        """One vs_range_selfjoin_rows call: (lims int64 (len(rows)+1), S, I)."""
        h = ctypes.c_void_p()
        _lib.check(self._lib.vs_range_selfjoin_rows(self._h, rows.ctypes.data, rows.size,
                                                    ctypes.c_float(min_sim),
                                                    1 if exclude_self else 0, 0, None,
                                                    ctypes.byref(h)),
                   "vs_range_selfjoin_rows")
        return self._range_take(h)

    def range_selfjoin(self, min_sim, *, q0: int = 0, nq: int | None = None,
                       exclude_self: bool = True, upper: bool = False, chunk: int = 65536,
                       rows=None):
        """Cosine range self-join over stored rows [q0, q0+nq): every row whose
        similarity with the query row is >= ``min_sim``, as many as there are
        (``selfjoin`` without its k).  Returns (lims uint64 (nq+1), S float32,
        I int64): row q0 + i's hits are S[lims[i]:lims[i+1]] /
        I[lims[i]:lims[i+1]], in ascending label order.

        Every pair is decided by its exact key, which is the same bits for
        (a, b) and (b, a): the full join is symmetric.  ``upper=True`` keeps, for
        each query row q, only the rows r > q — each unordered pair once, for
        about half the work — whether or not ``exclude_self`` is set (a row is
        never after itself).  Zero-norm rows and a NaN ``min_sim`` match
        nothing.  One C call per ``chunk`` query rows (at most 65536).

        ``rows=`` gives the query rows as a list of row positions instead of a
        window (any order, duplicates allowed; exclusive with ``q0`` / ``nq`` /
        ``upper=True``): entry i's hits are segment i, bit for bit the segment
        of the single-row window ``q0=rows[i], nq=1``."""
        chunk = int(chunk)
        assert 0 < chunk <= 65536
        if rows is not None:
            if q0 != 0 or nq is not None or upper:
                raise ValueError("range_selfjoin: rows= excludes q0, nq and upper=True")
            rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
            if rows.size == 0:
                return (np.zeros(1, dtype=np.uint64), np.empty(0, dtype=np.float32),
                        np.empty(0, dtype=np.int64))
            parts = [self._range_join_rows_call(rows[c0:c0 + chunk], float(min_sim), exclude_self)
                     for c0 in range(0, rows.size, chunk)]
            return self._range_concat(parts, rows.size)
        q0 = int(q0)
        nq = self.ntotal - q0 if nq is None else int(nq)
        min_sim = float(min_sim)
        if nq <= 0:
            if nq < 0:
                raise ValueError("range_selfjoin: query rows out of range")
            return (np.zeros(1, dtype=np.uint64), np.empty(0, dtype=np.float32),
                    np.empty(0, dtype=np.int64))
        parts = [self._range_join_call(q0 + c0, min(chunk, nq - c0), min_sim, exclude_self, upper)
                 for c0 in range(0, nq, chunk)]
        return self._range_concat(parts, nq)

    def selfjoin_device(self, k: int, q0: int, nq: int, D_ptr: int, I_ptr: int, *,
                        exclude_self: bool = True, min_sim: float = -np.inf,
                        stream: int = 0) -> None:
        _lib.check(self._lib.vs_selfjoin(self._h, int(q0), int(nq), int(k),
                                         1 if exclude_self else 0, ctypes.c_float(min_sim),
                                         ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
                                         _lib.OUT_DEVICE, ctypes.c_void_p(stream)),
                   "vs_selfjoin")


class IndexFlatL2(IndexFlat):
    def __init__(self, d: int, **kw):
        super().__init__(d, METRIC_L2, **kw)


class IndexFlatIP(IndexFlat):
    def __init__(self, d: int, **kw):
        super().__init__(d, METRIC_INNER_PRODUCT, **kw)


def normalize_L2(x: np.ndarray) -> None:
    """faiss.normalize_L2 (fvec_renorm_L2): in place, rows with zero norm untouched."""
    if not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.flags.c_contiguous):
        raise TypeError("normalize_L2 expects a C-contiguous float32 numpy array")
    nr = np.einsum("ij,ij->i", x, x, dtype=np.float32)
    inv = np.ones_like(nr)
    pos = nr > 0
    inv[pos] = (1.0 / np.sqrt(nr[pos].astype(np.float32))).astype(np.float32)
    x *= inv[:, None]


# ---- persistence: faiss flat binary format ------------------------------------------
# faiss index_write.cpp for IndexFlat [upstream]: fourcc ("IxF2" L2 / "IxFI" IP), then
# write_index_header: d:int32, ntotal:int64, dummy:int64 (1<<20) x2, is_trained:uint8,
# metric_type:int32 (metric_arg:float32 only when metric_type > 1), then the codes
# vector as size:uint64 (= #floats) followed by the raw float32 rows.
_FOURCC = {METRIC_L2: b"IxF2", METRIC_INNER_PRODUCT: b"IxFI"}


def write_index(index: IndexFlat, fname) -> None:
    """faiss.write_index for flat indexes (streams rows out in bounded chunks)."""
    if not all(hasattr(index, a) for a in ("d", "ntotal", "metric_type", "reconstruct_n")) \
            or index.metric_type not in _FOURCC:
        raise TypeError("write_index: only flat L2 / inner-product indexes are supported")
    ntotal = index.ntotal
    with open(fname, "wb") as f:
        f.write(_FOURCC[index.metric_type])
        f.write(struct.pack("<iqqq?i", index.d, ntotal, 1 << 20, 1 << 20, True,
                            index.metric_type))
        f.write(struct.pack("<Q", ntotal * index.d))
        step = max(1, (64 << 20) // (4 * index.d))
        for i0 in range(0, ntotal, step):
            f.write(index.reconstruct_n(i0, min(step, ntotal - i0)).tobytes())


def read_index(fname, *, device: int | None = None, index_factory=None) -> IndexFlat:
    """faiss.read_index for flat indexes (IxF2 / IxFI / IxFl with metric 0|1).
    `index_factory(d, metric)` overrides the GPU index constructor (tests)."""
    with open(fname, "rb") as f:
        h = f.read(4)
        if h not in (b"IxF2", b"IxFI", b"IxFl"):
            raise RuntimeError(f"read_index: unsupported index type {h!r} (flat indexes only)")
        d, ntotal, _, _, _, metric = struct.unpack("<iqqq?i", f.read(4 + 8 * 3 + 1 + 4))
        if metric > 1:
            f.read(4)  # metric_arg
            raise RuntimeError(f"read_index: metric {metric} not supported")
        (size,) = struct.unpack("<Q", f.read(8))
        if size != ntotal * d:
            raise RuntimeError("read_index: codes size does not match d*ntotal")
        if index_factory is not None:
            index = index_factory(d, metric)
        else:
            index = IndexFlat(d, metric, device=device)
            if ntotal:
                index.reserve(ntotal)
        step = max(1, (64 << 20) // (4 * d))
        left = ntotal
        while left > 0:
            m = min(step, left)
            buf = f.read(4 * d * m)
            if len(buf) != 4 * d * m:
                raise RuntimeError("read_index: truncated file")
            index.add(np.frombuffer(buf, dtype="<f4").reshape(m, d))
            left -= m
    return index
