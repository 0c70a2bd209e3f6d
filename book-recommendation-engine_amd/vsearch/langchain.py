"""Drop-in for ``langchain_community.vectorstores.FAISS`` on the MI355X engine.

The reference hard-imports ``from langchain_community.vectorstores import FAISS``
(src/ingestion_service/pipeline.py:15, ingestion_service/main.py:51,
incremental_workers/book_vector/main.py:53,432, recommendation_api/candidate_builder.py:31,
service.py:31, mcp_book_server.py:24).  langchain-community 0.3.26
(/root/reference/poetry.lock:1577-1578) is not vendored; this module restates the
method surface those call sites use, with the same argument meaning, return
types and error behaviour:

* ``FAISS.from_texts`` / ``from_embeddings`` — IndexFlatIP for
  ``DistanceStrategy.MAX_INNER_PRODUCT``, IndexFlatL2 otherwise (the reference
  never passes a strategy, so its stores are L2: SURVEY.md §0.2).
* ``add_texts`` / ``add_embeddings`` — uuid4 ids by default, ``ValueError`` on
  duplicate ids, labels continue at ``len(index_to_docstore_id)``.
* ``similarity_search[_with_score][_by_vector]`` — ``index.search(vec, k or
  fetch_k)``, skip label -1, docstore lookup, optional metadata filter and
  ``score_threshold`` (``<=`` for L2, ``>=`` for inner product), ``docs[:k]``;
  the score is faiss's D value (squared L2 / inner product) as ``np.float32``.
* ``max_marginal_relevance_search[_by_vector]`` /
  ``max_marginal_relevance_search_with_score_by_vector`` — LangChain's
  signatures and defaults (``k=4, fetch_k=20, lambda_mult=0.5, filter=None``);
  ``maximal_marginal_relevance`` as recalled (langchain is not vendored), the
  re-rank on the device (``index.search_mmr`` / ``index.mmr_select``).
* ``delete`` — ``ValueError`` for unknown ids, then ``index.remove_ids`` and
  contiguous renumbering of ``index_to_docstore_id``.
* ``save_local`` / ``load_local`` — ``index.faiss`` in faiss's flat binary
  format plus a JSON docstore sidecar (``index.docstore.json``; LangChain's
  ``index.pkl`` needs LangChain's classes to unpickle and is not read);
  ``load_local`` still demands ``allow_dangerous_deserialization=True``.
* ``recommend_for_profiles`` (library-specific) — the per-student candidate
  path of candidate_builder.py:138-203 (weighted mean of the rated books'
  embeddings, search, drop the books already read) for many students in one
  device call; ``similarity_search_with_score_by_vector(..., exclude_ids=)``
  for one query.
* ``where=`` (library-specific) — a metadata predicate per query run inside
  the search on the device (``index.search_where``), where the reference
  filters an over-fetch on the host (candidate_builder.py:187-203,
  service.py:529-542, mcp_book_server.py:615-682).
* ``boost=`` (library-specific) — similarity plus a per-query boost of the
  documents' metadata (reading-level match, staff pick), ranked over every
  document on the device (``index.search_boost``), where the reference adds
  those terms to the ``k * 2`` nearest only (scoring.py:78-131).
* ``bonus=`` (library-specific) — a number per (query, ``metadata[bonus_key]``
  value) added to the score of every document with that value, ranked over
  every document on the device (``index.search_bonus``): the reference's
  social and recency terms (scoring.py:116-125), which are numbers per
  (student, book) and not functions of a book's metadata.
"""

from __future__ import annotations

import enum
import json
import logging
import math
import operator
import uuid
import warnings
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import faiss as vfaiss

logger = logging.getLogger(__name__)

__all__ = ["Document", "InMemoryDocstore", "DistanceStrategy", "FAISS",
           "migrate_reference_store", "full_faiss_rebuild"]


class Document:
    """langchain_core.documents.Document (page_content, metadata, id)."""

    __slots__ = ("page_content", "metadata", "id")

    def __init__(self, page_content: str, metadata: Optional[dict] = None,
                 id: Optional[str] = None, **_ignored):
        if not isinstance(page_content, str):
            raise TypeError("page_content must be a str")
        self.page_content = page_content
        self.metadata = {} if metadata is None else metadata
        self.id = id

    @property
    def type(self) -> str:
        return "Document"

    def __eq__(self, other):
        return (isinstance(other, Document) and self.page_content == other.page_content
                and self.metadata == other.metadata and self.id == other.id)

    def __repr__(self):
        idp = f"id='{self.id}', " if self.id is not None else ""
        return f"Document({idp}metadata={self.metadata!r}, page_content={self.page_content!r})"

    def to_json(self) -> dict:
        return {"page_content": self.page_content, "metadata": self.metadata, "id": self.id}

    @classmethod
    def from_json(cls, obj: dict) -> "Document":
        return cls(page_content=obj["page_content"], metadata=obj.get("metadata") or {},
                   id=obj.get("id"))


class InMemoryDocstore:
    """langchain_community.docstore.in_memory.InMemoryDocstore."""

    def __init__(self, _dict: Optional[Dict[str, Document]] = None):
        self._dict = _dict if _dict is not None else {}

    def add(self, texts: Dict[str, Document]) -> None:
        overlapping = set(texts).intersection(self._dict)
        if overlapping:
            raise ValueError(f"Tried to add ids that already exist: {overlapping}")
        self._dict = {**self._dict, **texts}

    def delete(self, ids: List) -> None:
        overlapping = set(ids).intersection(self._dict)
        if not overlapping:
            raise ValueError(f"Tried to delete ids that does not  exist: {ids}")
        for _id in ids:
            self._dict.pop(_id)

    def search(self, search: str):
        if search not in self._dict:
            return f"ID {search} not found."
        return self._dict[search]


class DistanceStrategy(str, enum.Enum):
    """langchain_community.vectorstores.utils.DistanceStrategy."""

    EUCLIDEAN_DISTANCE = "EUCLIDEAN_DISTANCE"
    MAX_INNER_PRODUCT = "MAX_INNER_PRODUCT"
    DOT_PRODUCT = "DOT_PRODUCT"
    JACCARD = "JACCARD"
    COSINE = "COSINE"


def _len_check_if_sized(x: Any, y: Any, x_name: str, y_name: str) -> None:
    if hasattr(x, "__len__") and hasattr(y, "__len__") and len(x) != len(y):
        raise ValueError(
            f"{x_name} and {y_name} expected to be equal length but "
            f"len({x_name})={len(x)} and len({y_name})={len(y)}"
        )


_FILTER_OPS: Dict[str, Callable[[Any, Any], bool]] = {
    "$eq": operator.eq,
    "$neq": operator.ne,
    "$gt": operator.gt,
    "$lt": operator.lt,
    "$gte": operator.ge,
    "$lte": operator.le,
    "$in": lambda a, b: a in b,
    "$nin": lambda a, b: a not in b,
}


def _create_filter_func(filter: Any) -> Callable[[Dict[str, Any]], bool]:
    """Metadata filter: callable, or MongoDB-style dict ($eq/$neq/$gt/$lt/$gte/$lte/
    $in/$nin/$and/$or/$not; a bare list value means membership)."""
    if callable(filter):
        return filter
    if not isinstance(filter, dict):
        raise ValueError(f"filter must be a dict of metadata or a callable, not {type(filter)}")

    def filter_func_cond(field: str, condition: Any) -> Callable[[Dict[str, Any]], bool]:
        if isinstance(condition, dict):
            ops = []
            for op, value in condition.items():
                if op not in _FILTER_OPS:
                    raise ValueError(f"filter contains unsupported operator: {op}")
                ops.append((_FILTER_OPS[op], value))

            def cond(doc, ops=ops):
                try:
                    return all(fn(doc.get(field), value) for fn, value in ops)
                except TypeError:  # e.g. None > 3
                    return False

            return cond
        if isinstance(condition, list):
            return lambda doc: doc.get(field) in condition
        return lambda doc: doc.get(field) == condition

    def build(f: Dict[str, Any]) -> Callable[[Dict[str, Any]], bool]:
        parts = []
        for key, value in f.items():
            if key == "$and":
                subs = [build(x) for x in value]
                parts.append(lambda doc, subs=subs: all(s(doc) for s in subs))
            elif key == "$or":
                subs = [build(x) for x in value]
                parts.append(lambda doc, subs=subs: any(s(doc) for s in subs))
            elif key == "$not":
                sub = build(value)
                parts.append(lambda doc, sub=sub: not sub(doc))
            else:
                parts.append(filter_func_cond(key, value))
        return lambda doc: all(p(doc) for p in parts)

    return build(filter)


# ``where=``: the predicate grammar of the device-side filtered search
# (``index.search_where``).  A predicate is a dict over metadata fields; a
# numeric field takes $gte $lte $gt $lt $eq (closed float32 ranges: a strict
# bound becomes np.nextafter in float32), a categorical or list-valued field
# $in $all $nin $neq $eq (tag bits); a bare value is $eq.
_WHERE_NUM_OPS = ("$gte", "$lte", "$gt", "$lt", "$eq")
_WHERE_TAG_OPS = ("$in", "$all", "$nin", "$neq", "$eq")
_WHERE_ROUTE = " (filter= with exact_filter=True is the general route)"
WHERE_MAX_PAIRS = 64


def _is_number(v: Any) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and \
        not isinstance(v, (bool, np.bool_))


def _where_conditions(pred: Any) -> List[Tuple[str, str, Any]]:
    """[(field, operator, value)] of one predicate."""
    if not isinstance(pred, dict):
        raise ValueError("where: a predicate is a dict over metadata fields" + _WHERE_ROUTE)
    out = []
    for field, cond in pred.items():
        if isinstance(field, str) and field.startswith("$"):
            raise ValueError(f"where: operator {field} is not supported" + _WHERE_ROUTE)
        if isinstance(cond, dict):
            for op, value in cond.items():
                out.append((field, op, value))
        else:
            out.append((field, "$eq", cond))
    return out


def _where_values(op: str, value: Any) -> List[Any]:
    if op in ("$in", "$all", "$nin"):
        if not isinstance(value, (list, tuple, set, frozenset)):
            raise ValueError(f"where: {op} takes a list of values")
        return list(value)
    return [value]


def where_layout(preds, is_numeric: Callable[[str], bool]):
    """What the predicates need of an attribute handle: (the numeric fields,
    the (field, value) pairs of the tag vocabulary), both sorted.  More than 4
    numeric fields, more than 64 pairs or an operator outside the grammar is a
    ValueError."""
    nums: List[str] = []
    pairs: List[Tuple[str, Any]] = []
    for pred in preds:
        if pred is None:
            continue
        for field, op, value in _where_conditions(pred):
            if is_numeric(field):
                if op not in _WHERE_NUM_OPS:
                    raise ValueError(f"where: operator {op} on the numeric field {field!r} is "
                                     "not supported" + _WHERE_ROUTE)
                if not _is_number(value) or math.isnan(float(value)):
                    raise ValueError(f"where: {field!r} {op} takes a number")
                if field not in nums:
                    nums.append(field)
            else:
                if op not in _WHERE_TAG_OPS:
                    raise ValueError(f"where: operator {op} on the field {field!r} is not "
                                     "supported" + _WHERE_ROUTE)
                for v in _where_values(op, value):
                    if (field, v) not in pairs:
                        pairs.append((field, v))
    if len(nums) > vfaiss.MAX_WHERE_COLUMNS:
        raise ValueError(f"where: more than {vfaiss.MAX_WHERE_COLUMNS} numeric fields"
                         + _WHERE_ROUTE)
    if len(pairs) > WHERE_MAX_PAIRS:
        raise ValueError(f"where: more than {WHERE_MAX_PAIRS} (field, value) pairs" + _WHERE_ROUTE)
    return tuple(sorted(nums)), tuple(sorted(pairs, key=repr))


def where_predicate(pred, nums: Sequence[str], pairs: Sequence[Tuple[str, Any]]) -> Optional[dict]:
    """One predicate of the grammar as ``index.search_where`` takes it
    (``vfaiss.where_arrays``), over the columns ``nums`` and the tag bits
    ``pairs`` of ``where_layout``.  Conditions on one field intersect.  $in of
    several values sets any_of, which holds one such condition per predicate;
    $eq and $in of one value test the value's bit through all_of (the same
    test), so any number of fields may carry them."""
    if pred is None:
        return None
    lo = [-np.inf] * len(nums)
    hi = [np.inf] * len(nums)
    masks = {"any_of": 0, "all_of": 0, "none_of": 0}
    f32 = np.float32
    for field, op, value in _where_conditions(pred):
        if field in nums:
            c = nums.index(field)
            v = f32(value)
            if op == "$gt":
                v = np.nextafter(v, f32(np.inf))
            elif op == "$lt":
                v = np.nextafter(v, f32(-np.inf))
            if op in ("$gte", "$gt", "$eq"):
                lo[c] = max(lo[c], float(v))
            if op in ("$lte", "$lt", "$eq"):
                hi[c] = min(hi[c], float(v))
            continue
        bits = 0
        for v in _where_values(op, value):
            bits |= 1 << pairs.index((field, v))
        if op in ("$nin", "$neq"):
            masks["none_of"] |= bits
        elif op == "$all" or bin(bits).count("1") == 1:
            masks["all_of"] |= bits
        elif bits == 0:  # $in []: nothing matches (a bit must be set and none may be)
            masks["any_of"] = masks["none_of"] = 2**64 - 1
        elif masks["any_of"]:
            raise ValueError("where: $in of several values on more than one field"
                             + _WHERE_ROUTE)
        else:
            masks["any_of"] = bits
    return dict(lo=lo, hi=hi, **masks)


# ``boost=``: the grammar of the boosted search (``index.search_boost``).  A
# spec is a dict over metadata fields.  A numeric field takes
# {"$near": t, "scale": s, "weight": w[, "missing": m]} (w at t, falling to 0
# at distance s) or {"$ramp": [from, to], "weight": w[, "missing": m]} (0 at
# `from`, w from `to` on); m (default 0) is the term of a document without
# the field.  A categorical or list-valued field takes {"$in": [...],
# "weight": w} or {"$eq": v, "weight": w}: w when the document holds one of
# the values.
BOOST_MAX_TAGS = vfaiss.MAX_BOOST_TAGS
_BOOST_NUM_KEYS = {"$near": {"$near", "scale", "weight", "missing"},
                   "$ramp": {"$ramp", "weight", "missing"}}
_BOOST_TAG_KEYS = {"$in": {"$in", "weight"}, "$eq": {"$eq", "weight"}}


def _boost_terms(spec: Any, is_numeric: Callable[[str], bool]):
    """[(field, operator, term dict, numeric?)] of one spec, checked."""
    if not isinstance(spec, dict):
        raise ValueError("boost: a spec is a dict over metadata fields")
    out = []
    for field, term in spec.items():
        if isinstance(field, str) and field.startswith("$"):
            raise ValueError(f"boost: operator {field} is not supported")
        if not isinstance(term, dict):
            raise ValueError(f"boost: {field!r} takes a dict with an operator and a weight")
        numeric = is_numeric(field)
        table = _BOOST_NUM_KEYS if numeric else _BOOST_TAG_KEYS
        ops = [key for key in term if isinstance(key, str) and key.startswith("$")]
        if len(ops) != 1 or ops[0] not in table:
            raise ValueError(f"boost: {field!r} takes one of {sorted(table)}"
                             f" ({'a numeric' if numeric else 'a categorical'} field), got "
                             f"{sorted(ops)}")
        op = ops[0]
        unknown = set(term) - table[op]
        if unknown:
            raise ValueError(f"boost: unknown keys {sorted(unknown, key=repr)} on {field!r}")
        if not _is_number(term.get("weight")):
            raise ValueError(f"boost: {field!r} needs a numeric weight")
        if numeric:
            if op == "$near" and not (_is_number(term["$near"]) and _is_number(term.get("scale"))):
                raise ValueError(f"boost: {field!r} $near takes a number and a numeric scale")
            if op == "$ramp" and not (isinstance(term["$ramp"], (list, tuple))
                                      and len(term["$ramp"]) == 2
                                      and all(_is_number(v) for v in term["$ramp"])):
                raise ValueError(f"boost: {field!r} $ramp takes [from, to]")
            if not _is_number(term.get("missing", 0.0)):
                raise ValueError(f"boost: {field!r} missing takes a number")
        elif op == "$in" and not isinstance(term["$in"], (list, tuple, set, frozenset)):
            raise ValueError("boost: $in takes a list of values")
        out.append((field, op, term, numeric))
    return out


def boost_layout(specs, is_numeric: Callable[[str], bool]):
    """What the boost specs need of an attribute handle, as ``where_layout``:
    (the numeric fields, the (field, value) pairs), both sorted.  More than 4
    numeric fields, more than 4 tag terms in one spec or an operator outside
    the grammar is a ValueError."""
    nums: List[str] = []
    pairs: List[Tuple[str, Any]] = []
    for spec in specs:
        if spec is None:
            continue
        ntag = 0
        for field, op, term, numeric in _boost_terms(spec, is_numeric):
            if numeric:
                if field not in nums:
                    nums.append(field)
                continue
            ntag += 1
            for v in (list(term["$in"]) if op == "$in" else [term["$eq"]]):
                if (field, v) not in pairs:
                    pairs.append((field, v))
        if ntag > BOOST_MAX_TAGS:
            raise ValueError(f"boost: more than {BOOST_MAX_TAGS} categorical terms in one spec")
    if len(nums) > vfaiss.MAX_WHERE_COLUMNS:
        raise ValueError(f"boost: more than {vfaiss.MAX_WHERE_COLUMNS} numeric fields")
    if len(pairs) > WHERE_MAX_PAIRS:
        raise ValueError(f"boost: more than {WHERE_MAX_PAIRS} (field, value) pairs")
    return tuple(sorted(nums)), tuple(sorted(pairs, key=repr))


def boost_spec(spec, nums: Sequence[str], pairs: Sequence[Tuple[str, Any]],
               is_numeric: Callable[[str], bool]) -> Optional[dict]:
    """One spec of the grammar as ``index.search_boost`` takes it
    (``vfaiss.boost_arrays``), over the columns ``nums`` and the tag bits
    ``pairs`` of the handle."""
    if spec is None:
        return None
    columns: List[Any] = [None] * len(nums)
    tags = []
    for field, op, term, numeric in _boost_terms(spec, is_numeric):
        w = float(term["weight"])
        if numeric:
            miss = float(term.get("missing", 0.0))
            if op == "$near":
                columns[nums.index(field)] = ("near", float(term["$near"]), float(term["scale"]),
                                              w, miss)
            else:
                lo, hi = (float(v) for v in term["$ramp"])
                columns[nums.index(field)] = ("ramp", lo, hi - lo, w, miss)
            continue
        bits = 0
        for v in (list(term["$in"]) if op == "$in" else [term["$eq"]]):
            bits |= 1 << pairs.index((field, v))
        tags.append((bits, w))
    return {"columns": columns, "tags": tags}


class FAISS:
    """Vector store over a vsearch flat index (LangChain ``FAISS`` API)."""

    def __init__(self, embedding_function, index, docstore, index_to_docstore_id: Dict[int, str],
                 relevance_score_fn: Optional[Callable[[float], float]] = None,
                 normalize_L2: bool = False,
                 distance_strategy: DistanceStrategy = DistanceStrategy.EUCLIDEAN_DISTANCE):
        if not (hasattr(embedding_function, "embed_query") or callable(embedding_function)):
            logger.warning("`embedding_function` is expected to be an Embeddings object")
        self.embedding_function = embedding_function
        self.index = index
        self.docstore = docstore
        self.index_to_docstore_id = index_to_docstore_id
        self.distance_strategy = DistanceStrategy(distance_strategy)
        self.override_relevance_score_fn = relevance_score_fn
        self._normalize_L2 = normalize_L2
        self._keymap_field: Optional[str] = None  # metadata field indexed by _key_index
        self._keymap: Dict[Any, List[str]] = {}
        # exact_filter selectors by the filter's JSON; dropped by every add / delete / merge
        self._sel_cache: Dict[str, Any] = {}
        # distinct= groupings by metadata field; dropped whenever _sel_cache is
        self._grp_cache: Dict[str, Any] = {}
        # where= attribute handles by (numeric fields, tag vocabulary), and the
        # kind of every field a predicate named; dropped whenever _sel_cache is
        self._attr_cache: Dict[Any, Any] = {}
        # (field, metadata[field] -> labels), built once per store generation
        # (the labels move with every delete): dropped with _sel_cache
        self._keylabels: Optional[Tuple[str, Dict[Any, List[int]]]] = None
        if (self.distance_strategy != DistanceStrategy.EUCLIDEAN_DISTANCE
                and self._normalize_L2):
            warnings.warn(
                f"Normalizing L2 is not applicable for metric type: {self.distance_strategy}")

    # -- embeddings --------------------------------------------------------------------
    @property
    def embeddings(self):
        return self.embedding_function if hasattr(self.embedding_function, "embed_query") else None

    def _embed_documents(self, texts: List[str]) -> List[List[float]]:
        if hasattr(self.embedding_function, "embed_documents"):
            return self.embedding_function.embed_documents(texts)
        return [self.embedding_function(t) for t in texts]

    def _embed_query(self, text: str) -> List[float]:
        if hasattr(self.embedding_function, "embed_query"):
            return self.embedding_function.embed_query(text)
        return self.embedding_function(text)

    # -- writes ---------------------------------------------------------------------------
    def __add(self, texts: Iterable[str], embeddings: Iterable[List[float]],
              metadatas: Optional[Iterable[dict]] = None,
              ids: Optional[List[str]] = None) -> List[str]:
        if not hasattr(self.docstore, "add"):
            raise ValueError("If trying to add texts, the underlying docstore should support "
                             f"adding items, which {self.docstore} does not")
        _len_check_if_sized(texts, metadatas, "texts", "metadatas")
        ids = ids or [str(uuid.uuid4()) for _ in texts]
        _len_check_if_sized(texts, ids, "texts", "ids")
        _metadatas = metadatas or ({} for _ in texts)
        documents = [Document(id=id_, page_content=t, metadata=m)
                     for id_, t, m in zip(ids, texts, _metadatas)]
        _len_check_if_sized(documents, embeddings, "documents", "embeddings")
        if ids and len(ids) != len(set(ids)):
            raise ValueError("Duplicate ids found in the ids list.")
        vector = np.array(embeddings, dtype=np.float32)
        if vector.ndim == 1:
            vector = vector.reshape(len(documents), -1)
        if self._normalize_L2:
            vfaiss.normalize_L2(vector)
        self._sel_cache.clear()
        self._grp_cache.clear()
        self._attr_cache.clear()
        self._keylabels = None
        self.index.add(vector)
        self.docstore.add({id_: doc for id_, doc in zip(ids, documents)})
        starting_len = len(self.index_to_docstore_id)
        self.index_to_docstore_id.update({starting_len + j: id_ for j, id_ in enumerate(ids)})
        if self._keymap_field is not None:
            for doc in documents:
                key = doc.metadata.get(self._keymap_field)
                if key is not None:
                    self._keymap.setdefault(key, []).append(doc.id)
        return ids

    def add_texts(self, texts: Iterable[str], metadatas: Optional[List[dict]] = None,
                  ids: Optional[List[str]] = None, **kwargs: Any) -> List[str]:
        texts = list(texts)
        embeddings = self._embed_documents(texts)
        return self.__add(texts, embeddings, metadatas=metadatas, ids=ids)

    def add_embeddings(self, text_embeddings: Iterable[Tuple[str, List[float]]],
                       metadatas: Optional[List[dict]] = None, ids: Optional[List[str]] = None,
                       **kwargs: Any) -> List[str]:
        texts, embeddings = zip(*text_embeddings)
        return self.__add(texts, embeddings, metadatas=metadatas, ids=ids)

    def add_documents(self, documents: List[Document], **kwargs: Any) -> List[str]:
        texts = [d.page_content for d in documents]
        metadatas = [d.metadata for d in documents]
        if "ids" not in kwargs:
            ids = [d.id for d in documents]
            if any(ids):
                kwargs["ids"] = [i if i else str(uuid.uuid4()) for i in ids]
        return self.add_texts(texts, metadatas, **kwargs)

    def _key_index(self, field: str) -> Dict[Any, List[str]]:
        """metadata[field] -> docstore ids holding it.  Built by one scan on first use
        for `field`, then maintained by every add / delete (O(changed rows))."""
        if self._keymap_field != field:
            keymap: Dict[Any, List[str]] = {}
            for i in sorted(self.index_to_docstore_id):
                _id = self.index_to_docstore_id[i]
                doc = self.docstore.search(_id)
                if isinstance(doc, Document) and doc.metadata.get(field) is not None:
                    keymap.setdefault(doc.metadata[field], []).append(_id)
            self._keymap_field, self._keymap = field, keymap
        return self._keymap

    def ids_for_key(self, value: Any, field: str = "book_id") -> List[str]:
        """Docstore ids whose metadata[field] == value, in label order."""
        return list(self._key_index(field).get(value, ()))

    def upsert_embeddings(self, texts: Sequence[str], embeddings: Sequence[List[float]],
                          metadatas: Sequence[dict], key: str = "book_id",
                          ids: Optional[List[str]] = None, in_place: bool = False) -> List[str]:
        """Delete-then-add.  The reference appends a second row when a
        book is re-embedded (incremental_workers/book_vector/main.py:148,
        ingestion_service/pipeline.py:363), so searches return the stale copy too.
        Here every existing row whose metadata[key] matches an incoming row is
        removed first (one remove_ids compaction on the device), and within the
        batch the last row for a key wins.  Rows without the key are plain appends.

        ``in_place=True``: a key that has a stored row keeps that row's label —
        its vector is replaced where it is (``index.update``; no compaction)
        and its document by the new one, under the id a plain add would have
        given it.  A key with several rows keeps the lowest label, the others
        are deleted; a key without a row is appended.  A batch of pure
        re-embeddings (nothing appended or deleted, every replaced document's
        metadata equal to the old one's) keeps the cached ``filter=`` selectors
        and ``distinct=`` groupings."""
        texts, embeddings, metadatas = list(texts), list(embeddings), list(metadatas)
        _len_check_if_sized(texts, metadatas, "texts", "metadatas")
        _len_check_if_sized(texts, embeddings, "texts", "embeddings")
        if ids is not None:
            _len_check_if_sized(texts, ids, "texts", "ids")
        last = {m.get(key): j for j, m in enumerate(metadatas) if m.get(key) is not None}
        keep = [j for j, m in enumerate(metadatas)
                if m.get(key) is None or last[m.get(key)] == j]
        keymap = self._key_index(key)
        stale = [sid for j in keep if metadatas[j].get(key) is not None
                 for sid in keymap.get(metadatas[j][key], ())]
        if ids is not None:
            clash = set(ids[j] for j in keep).intersection(self.index_to_docstore_id.values())
            clash.difference_update(stale)
            if clash:
                raise ValueError(f"Tried to add ids that already exist: {clash}")
        if in_place:
            return self._upsert_in_place(texts, embeddings, metadatas, key, ids, keep)
        if stale:
            self.delete(stale)
        return self.__add([texts[j] for j in keep], [embeddings[j] for j in keep],
                          metadatas=[metadatas[j] for j in keep],
                          ids=None if ids is None else [ids[j] for j in keep])

    def _upsert_in_place(self, texts, embeddings, metadatas, key, ids, keep) -> List[str]:
        """``upsert_embeddings(in_place=True)`` after its checks: `keep` = the
        batch's rows that count (the last one per key)."""
        if not hasattr(self.index, "update"):
            raise ValueError("upsert with in_place=True needs an index with update(labels, x) "
                             f"(vsearch.faiss.IndexFlat); {type(self.index).__name__} has none")
        if not hasattr(self.docstore, "add"):
            raise ValueError("If trying to add texts, the underlying docstore should support "
                             f"adding items, which {self.docstore} does not")
        new_ids = {j: (ids[j] if ids is not None else str(uuid.uuid4())) for j in keep}
        if len(set(new_ids.values())) != len(new_ids):
            raise ValueError("Duplicate ids found in the ids list.")
        keylabels = self._key_labels(key)  # kept across pure re-embeddings
        replace, append, extra = [], [], []
        for j in keep:
            value = metadatas[j].get(key)
            labels = keylabels.get(value) if value is not None else None
            if labels:
                replace.append((j, labels[0]))
                extra.extend(self.index_to_docstore_id[i] for i in labels[1:])
            else:
                append.append(j)
        changed = False
        if replace:
            vector = np.array([embeddings[j] for j, _ in replace], dtype=np.float32)
            if vector.ndim == 1:
                vector = vector.reshape(len(replace), -1)
            if self._normalize_L2:
                vfaiss.normalize_L2(vector)
            self.index.update(np.array([i for _, i in replace], dtype=np.int64), vector)
            for j, label in replace:
                old_id = self.index_to_docstore_id[label]
                old = self.docstore.search(old_id)
                if not isinstance(old, Document) or old.metadata != metadatas[j]:
                    changed = True
                new_id = new_ids[j]
                self.docstore.delete([old_id])
                self.docstore.add({new_id: Document(id=new_id, page_content=texts[j],
                                                    metadata=metadatas[j])})
                self.index_to_docstore_id[label] = new_id
                # _key_labels indexed `key`: the old and the new document share its value
                lst = self._keymap.get(metadatas[j][key])
                if lst is not None and old_id in lst:
                    lst[lst.index(old_id)] = new_id
        if changed:  # a filter or a grouping may read the fields that changed
            self._sel_cache.clear()
            self._grp_cache.clear()
            self._attr_cache.clear()
            self._keylabels = None
        if extra:  # after the update: a delete renumbers the labels
            self.delete(extra)
        if append:
            self.__add([texts[j] for j in append], [embeddings[j] for j in append],
                       metadatas=[metadatas[j] for j in append],
                       ids=[new_ids[j] for j in append])
        return [new_ids[j] for j in keep]

    def upsert_texts(self, texts: Iterable[str], metadatas: List[dict], key: str = "book_id",
                     ids: Optional[List[str]] = None, in_place: bool = False,
                     **kwargs: Any) -> List[str]:
        """`add_texts` with delete-then-add on metadata[key] (or, with
        ``in_place=True``, ``upsert_embeddings``'s replacement in place); embeds
        before mutating, so an embedding failure leaves the store unchanged."""
        texts = list(texts)
        embeddings = self._embed_documents(texts)
        return self.upsert_embeddings(texts, embeddings, metadatas, key=key, ids=ids,
                                      in_place=in_place)

    def delete(self, ids: Optional[List[str]] = None, **kwargs: Any) -> Optional[bool]:
        if ids is None:
            raise ValueError("No ids provided to delete.")
        missing_ids = set(ids).difference(self.index_to_docstore_id.values())
        if missing_ids:
            raise ValueError(
                f"Some specified ids do not exist in the current store. Ids not found: "
                f"{missing_ids}")
        reversed_index = {id_: idx for idx, id_ in self.index_to_docstore_id.items()}
        index_to_delete = {reversed_index[id_] for id_ in ids}
        self._sel_cache.clear()
        self._grp_cache.clear()
        self._attr_cache.clear()
        self._keylabels = None
        self.index.remove_ids(np.fromiter(index_to_delete, dtype=np.int64))
        if self._keymap_field is not None:
            for id_ in ids:
                doc = self.docstore.search(id_)
                key = doc.metadata.get(self._keymap_field) if isinstance(doc, Document) else None
                lst = self._keymap.get(key)
                if lst is not None and id_ in lst:
                    lst.remove(id_)
                    if not lst:
                        del self._keymap[key]
        self.docstore.delete(ids)
        remaining_ids = [id_ for i, id_ in sorted(self.index_to_docstore_id.items())
                         if i not in index_to_delete]
        self.index_to_docstore_id = {i: id_ for i, id_ in enumerate(remaining_ids)}
        return True

    def get_by_ids(self, ids: Sequence[str], /) -> List[Document]:
        docs = [self.docstore.search(id_) for id_ in ids]
        return [d for d in docs if isinstance(d, Document)]

    def merge_from(self, target: "FAISS") -> None:
        if not hasattr(self.docstore, "add"):
            raise ValueError("Cannot merge with this type of docstore")
        index_offset = len(self.index_to_docstore_id)
        self._sel_cache.clear()
        self._grp_cache.clear()
        self._attr_cache.clear()
        self._keylabels = None
        if target.index.ntotal:
            self.index.add(target.index.reconstruct_n(0, target.index.ntotal))
        full_info = []
        for i, target_id in target.index_to_docstore_id.items():
            doc = target.docstore.search(target_id)
            if not isinstance(doc, Document):
                raise ValueError("Document should be returned")
            full_info.append((index_offset + i, target_id, doc))
        self.docstore.add({_id: doc for _, _id, doc in full_info})
        self.index_to_docstore_id.update({index: _id for index, _id, _ in full_info})

    # -- exact filters ------------------------------------------------------------------------
    def _filter_mask(self, filter: Any, use_key_index: bool = True) -> np.ndarray:
        """The labels (bool array over 0 .. ntotal) whose document passes `filter`.
        A dict on one field with $eq / $in / $nin / $neq, a bare value or a list
        is answered from ``_key_index(field)`` without reading the docstore;
        other dicts and callables scan the docstore once."""
        n = len(self.index_to_docstore_id)
        mask = np.zeros(n, dtype=bool)
        fast = self._key_index_values(filter) if use_key_index else None
        if fast is not None:
            field, values, negate = fast
            keymap = self._key_index(field)
            label_of = {id_: i for i, id_ in self.index_to_docstore_id.items()}
            for v in values:
                for id_ in keymap.get(v, ()):
                    mask[label_of[id_]] = True
            return ~mask if negate else mask
        filter_func = _create_filter_func(filter)
        for i, id_ in self.index_to_docstore_id.items():
            doc = self.docstore.search(id_)
            if isinstance(doc, Document) and filter_func(doc.metadata):
                mask[i] = True
        return mask

    @staticmethod
    def _key_index_values(filter: Any):
        """(field, values, negate) when `filter` is a one-field membership test the
        key index answers, else None.  None values and unhashable ones are left
        to the scan (the key index does not hold documents without the field)."""
        if not isinstance(filter, dict) or len(filter) != 1:
            return None
        (field, cond), = filter.items()
        if not isinstance(field, str) or field.startswith("$"):
            return None
        negate = False
        if isinstance(cond, dict):
            if len(cond) != 1:
                return None
            (op, value), = cond.items()
            if op in ("$eq", "$neq"):
                values = [value]
            elif op in ("$in", "$nin"):
                if not isinstance(value, (list, tuple, set, frozenset)):
                    return None
                values = list(value)
            else:
                return None
            negate = op in ("$neq", "$nin")
        elif isinstance(cond, list):
            values = cond
        else:
            values = [cond]
        try:
            if any(v is None for v in values):
                return None
            set(values)  # hashable
        except TypeError:
            return None
        return field, values, negate

    def _filter_selector(self, filter: Any):
        """What ``index.search(params=SearchParameters(sel=...))`` takes for
        `filter`: the index's device handle where it has one (built once per
        filter, kept until the store changes), else the label bitmap."""
        key = None
        if not callable(filter):
            try:
                key = json.dumps(filter, sort_keys=True, default=repr)
            except (TypeError, ValueError):
                key = None
        if key is not None and key in self._sel_cache:
            return self._sel_cache[key]
        mask = self._filter_mask(filter)
        sel = vfaiss.IDSelectorBitmap(mask.size, np.packbits(mask, bitorder="little"))
        if hasattr(self.index, "selector"):
            sel = self.index.selector(sel)
        if key is not None:
            self._sel_cache[key] = sel
        return sel

    def _distinct_grouping(self, field: str):
        """What ``index.search_distinct`` takes for ``distinct=field``: one key
        per label, metadata[field] of its document (a document without the
        field is its own group), as the index's device handle.  Built once per
        field and kept until the store changes."""
        grp = self._grp_cache.get(field)
        if grp is None:
            keys = []
            for i in range(len(self.index_to_docstore_id)):
                doc = self.docstore.search(self.index_to_docstore_id[i])
                keys.append(doc.metadata.get(field) if isinstance(doc, Document) else None)
            grp = self._grp_cache[field] = self.index.grouping(keys)
        return grp

    def _metadata_column(self, field: str) -> List[Any]:
        out = []
        for i in range(len(self.index_to_docstore_id)):
            doc = self.docstore.search(self.index_to_docstore_id[i])
            out.append(doc.metadata.get(field) if isinstance(doc, Document) else None)
        return out

    def _where_is_numeric(self, field: str) -> bool:
        """A field is numeric when every document that has it holds a number."""
        key = ("kind", field)
        if key not in self._attr_cache:
            vals = [v for v in self._metadata_column(field) if v is not None]
            self._attr_cache[key] = bool(vals) and all(_is_number(v) for v in vals)
        return self._attr_cache[key]

    def _where_attributes(self, nums, pairs):
        """The index's attribute handle over the numeric fields `nums` (NaN
        where a document has no value) and one tag bit per (field, value) pair
        of `pairs` (set where metadata[field] equals the value or, list-valued,
        holds it).  Built once per layout and kept until the store changes."""
        key = (nums, tuple(repr(p) for p in pairs))
        attrs = self._attr_cache.get(key)
        if attrs is None:
            n = len(self.index_to_docstore_id)
            cols = np.full((len(nums), n), np.nan, dtype=np.float32)
            for c, field in enumerate(nums):
                for i, v in enumerate(self._metadata_column(field)):
                    if v is not None:
                        cols[c, i] = v
            tags = np.zeros(n, dtype=np.uint64)
            for field in sorted({f for f, _ in pairs}):
                bit = {v: np.uint64(1 << j) for j, (f, v) in enumerate(pairs) if f == field}
                for i, v in enumerate(self._metadata_column(field)):
                    for x in (v if isinstance(v, (list, tuple, set, frozenset)) else (v,)):
                        if x in bit:
                            tags[i] |= bit[x]
            attrs = self._attr_cache[key] = self.index.attributes(
                cols if nums else None, tags if pairs or not nums else None)
        return attrs

    def _search_where(self, vec, k: int, where, exclude=None):
        """``index.search_where`` of the queries `vec` under the grammar's
        predicates: one dict for every query or one per query."""
        preds = [where] * vec.shape[0] if where is None or isinstance(where, dict) else list(where)
        if len(preds) != vec.shape[0]:
            raise ValueError(f"where: {len(preds)} predicates for {vec.shape[0]} queries")
        nums, pairs = where_layout(preds, self._where_is_numeric)
        attrs = self._where_attributes(nums, pairs)
        return self.index.search_where(vec, k, attrs,
                                       [where_predicate(p, nums, pairs) for p in preds],
                                       exclude=exclude)

    def _search_boost(self, vec, k: int, boost, where=None, exclude=None):
        """``index.search_boost`` of the queries `vec` under the grammar's
        boost specs (one dict for every query or one per query), composed with
        ``where`` predicates and exclusion lists.  One attribute handle serves
        the fields of both grammars."""
        attrs, specs, preds = self._boost_args(vec.shape[0], boost, where)
        return self.index.search_boost(vec, k, attrs, specs, where=preds, exclude=exclude)

    def _boost_args(self, n: int, boost, where):
        """What ``index.search_boost`` / ``index.search_bonus`` take for the
        grammar's boost specs and ``where`` predicates of n queries: (attribute
        handle, boost specs, predicates or None)."""
        specs = [boost] * n if boost is None or isinstance(boost, dict) else list(boost)
        if len(specs) != n:
            raise ValueError(f"boost: {len(specs)} specs for {n} queries")
        preds = [where] * n if where is None or isinstance(where, dict) else list(where)
        if len(preds) != n:
            raise ValueError(f"where: {len(preds)} predicates for {n} queries")
        bnums, bpairs = boost_layout(specs, self._where_is_numeric)
        wnums, wpairs = where_layout(preds, self._where_is_numeric)
        nums = tuple(sorted(set(bnums) | set(wnums)))
        pairs = tuple(sorted(set(bpairs) | set(wpairs), key=repr))
        if len(nums) > vfaiss.MAX_WHERE_COLUMNS:
            raise ValueError(f"boost and where: more than {vfaiss.MAX_WHERE_COLUMNS} numeric "
                             "fields together")
        if len(pairs) > WHERE_MAX_PAIRS:
            raise ValueError(f"boost and where: more than {WHERE_MAX_PAIRS} (field, value) pairs "
                             "together")
        attrs = self._where_attributes(nums, pairs)
        return (attrs, [boost_spec(sp, nums, pairs, self._where_is_numeric) for sp in specs],
                None if where is None else [where_predicate(p, nums, pairs) for p in preds])

    def _bonus_lists(self, bonus, n: int, bonus_key: str) -> List[Dict[int, float]]:
        """``bonus=`` of n queries as ``index.search_bonus`` takes it: one dict
        ``metadata[bonus_key] value -> number`` for every query or a sequence of
        n of them (``None``: no bonus) becomes one dict ``label -> number`` per
        query.  Every stored row with a value gets its number (a re-embedded
        book's rows all do); values the store does not hold are ignored."""
        entries = [bonus] * n if bonus is None or isinstance(bonus, dict) else list(bonus)
        if len(entries) != n:
            raise ValueError(f"bonus: {len(entries)} lists for {n} queries")
        table = self._key_labels(bonus_key)
        out = []
        for e in entries:
            lists: Dict[int, float] = {}
            if e is not None:
                if not isinstance(e, dict):
                    raise ValueError(f"bonus: a dict from {bonus_key} values to numbers "
                                     "(or None) per query")
                for value, s in e.items():
                    if not _is_number(s) or not math.isfinite(s):
                        raise ValueError(f"bonus: {value!r} needs a finite number")
                    for label in table.get(value, ()):
                        lists[label] = float(s)
            if len(lists) > vfaiss.MAX_BONUS_LIST:
                raise ValueError(f"bonus: more than {vfaiss.MAX_BONUS_LIST} documents in one "
                                 "query's list")
            out.append(lists)
        return out

    def _search_bonus(self, vec, k: int, bonus, bonus_key: str = "book_id", boost=None,
                      where=None, exclude=None):
        """``index.search_bonus`` of the queries `vec`: the ``bonus=`` lists
        composed with the grammar's boost specs, ``where`` predicates and
        exclusion lists."""
        n = vec.shape[0]
        lists = self._bonus_lists(bonus, n, bonus_key)
        if boost is None and where is None:
            return self.index.search_bonus(vec, k, lists, exclude=exclude)
        attrs, specs, preds = self._boost_args(n, boost, where)
        return self.index.search_bonus(vec, k, lists, attrs=attrs, boost=specs, where=preds,
                                       exclude=exclude)

    # -- reads ------------------------------------------------------------------------------
    def similarity_search_with_score_by_vector(self, embedding: List[float], k: int = 4,
                                               filter: Optional[Any] = None, fetch_k: int = 20,
                                               exact_filter: bool = False,
                                               **kwargs: Any) -> List[Tuple[Document, float]]:
        """``exact_filter=True``: the k nearest documents among those that pass
        `filter` (exactly min(k, matches) of them; `fetch_k` is ignored), by a
        selector search, instead of filtering the `fetch_k` nearest on the host.

        ``exclude_ids=[...]`` (docstore ids; unknown ones are ignored): those
        documents are left out of the search itself, so k others come back
        (library-specific; not together with ``exact_filter``).

        ``distinct="<metadata field>"``: at most one document per value of that
        field, each value's nearest document (``index.search_distinct``): the
        k nearest books of a store that holds several rows per book, where a
        plain search returns a re-ingested book twice.  Documents without the
        field count one by one.  With a host `filter` the distinct search
        fetches `fetch_k` values and the filter runs after it; not together
        with ``exact_filter`` (library-specific).

        ``where={...}``: the k nearest documents among those whose metadata
        pass the predicate, filtered on the device inside the search
        (``index.search_where``): exactly min(k, matches) of them.  The
        grammar is a dict over metadata fields: a numeric field takes ``$gte
        $lte $gt $lt $eq``, a categorical or list-valued field ``$in $all $nin
        $neq $eq``, a bare value is ``$eq``; at most 4 numeric fields and 64
        (field, value) pairs, anything else is a ValueError (`filter` with
        ``exact_filter=True`` takes any predicate).  Combines with
        ``exclude_ids``; not with ``distinct`` or ``exact_filter``
        (library-specific).

        ``boost={...}``: the k documents with the best similarity plus a
        boost of their metadata, ranked over every document on the device
        (``index.search_boost``) instead of re-scoring the ``k * 2`` nearest as
        the reference's ``score_candidates`` does.  A numeric field takes
        ``{"$near": t, "scale": s, "weight": w, "missing": m}`` (w at t,
        falling linearly to 0 at distance s; m for a document without the
        field) or ``{"$ramp": [from, to], "weight": w}``; a categorical or
        list-valued field ``{"$in": [...], "weight": w}`` or ``{"$eq": v,
        "weight": w}``.  At most 4 numeric fields and 4 categorical terms.  The
        returned scores are the boosted ones (score + boost for an
        inner-product store, distance - boost for an L2 store).  Combines with
        ``where`` and ``exclude_ids``; with ``distinct``, `filter` or MMR it is
        a ValueError (library-specific).

        ``bonus={value: number, ...}`` with ``bonus_key="book_id"``: every
        document whose ``metadata[bonus_key]`` is a listed value has the number
        added to its score (subtracted from its distance in an L2 store)
        before the ranking, over every document on the device
        (``index.search_bonus``): a book two neighbours just borrowed can
        enter the result from anywhere in the store, and a negative number
        demotes one.  Values the store does not hold are ignored.  The
        returned scores are the final ones.  Combines with ``where``,
        ``boost`` and ``exclude_ids``; with ``distinct``, `filter` or MMR it is
        a ValueError (library-specific)."""
        vector = np.array([embedding], dtype=np.float32)
        if self._normalize_L2:
            vfaiss.normalize_L2(vector)
        exclude_ids = kwargs.get("exclude_ids")
        distinct = kwargs.get("distinct")
        where = kwargs.get("where")
        if distinct is not None and exact_filter:
            raise ValueError("distinct and exact_filter cannot be combined")
        if where is not None and distinct is not None:
            raise ValueError("where and distinct cannot be combined")
        if where is not None and exact_filter:
            raise ValueError("where and exact_filter cannot be combined")
        boost = kwargs.get("boost")
        if boost is not None and (distinct is not None or filter is not None or exact_filter):
            raise ValueError("boost cannot be combined with distinct or filter (not built); "
                             "where= and exclude_ids compose with it")
        bonus = kwargs.get("bonus")
        if bonus is not None and (distinct is not None or filter is not None or exact_filter):
            raise ValueError("bonus cannot be combined with distinct or filter (not built); "
                             "where=, boost= and exclude_ids compose with it")
        drop = None
        if exclude_ids is not None:
            if exact_filter and filter is not None:
                raise ValueError("exclude_ids and exact_filter cannot be combined")
            wanted = set(exclude_ids)
            drop = [i for i, id_ in self.index_to_docstore_id.items() if id_ in wanted]
        if bonus is not None:
            scores, indices = self._search_bonus(
                vector, k, [bonus], kwargs.get("bonus_key", "book_id"), boost=boost, where=where,
                exclude=None if drop is None else [drop])
        elif boost is not None:
            scores, indices = self._search_boost(vector, k, boost, where=where,
                                                 exclude=None if drop is None else [drop])
        elif distinct is not None:
            scores, indices = self.index.search_distinct(
                vector, k if filter is None else fetch_k, self._distinct_grouping(distinct),
                exclude=None if drop is None else [drop])
        elif where is not None:
            scores, indices = self._search_where(vector, k if filter is None else fetch_k, where,
                                                 exclude=None if drop is None else [drop])
        elif drop is not None:
            scores, indices = self.index.search(vector, k if filter is None else fetch_k,
                                                exclude=[drop])
        elif exact_filter and filter is not None:
            scores, indices = self.index.search(
                vector, k, params=vfaiss.SearchParameters(sel=self._filter_selector(filter)))
            filter = None  # every label returned passes it
        else:
            scores, indices = self.index.search(vector, k if filter is None else fetch_k)
        docs = []
        filter_func = _create_filter_func(filter) if filter is not None else None
        for j, i in enumerate(indices[0]):
            if i == -1:
                continue
            _id = self.index_to_docstore_id[int(i)]
            doc = self.docstore.search(_id)
            if not isinstance(doc, Document):
                raise ValueError(f"Could not find document for id {_id}, got {doc}")
            if filter_func is None or filter_func(doc.metadata):
                docs.append((doc, scores[0][j]))
        score_threshold = kwargs.get("score_threshold")
        if score_threshold is not None:
            cmp = (operator.ge if self.distance_strategy in
                   (DistanceStrategy.MAX_INNER_PRODUCT, DistanceStrategy.JACCARD) else operator.le)
            docs = [(doc, s) for doc, s in docs if cmp(s, score_threshold)]
        return docs[:k]

    def similarity_search_with_score(self, query: str, k: int = 4, filter: Optional[Any] = None,
                                     fetch_k: int = 20, exact_filter: bool = False,
                                     **kwargs: Any):
        embedding = self._embed_query(query)
        return self.similarity_search_with_score_by_vector(embedding, k, filter=filter,
                                                           fetch_k=fetch_k,
                                                           exact_filter=exact_filter, **kwargs)

    def similarity_search_by_vector(self, embedding: List[float], k: int = 4,
                                    filter: Optional[Any] = None, fetch_k: int = 20,
                                    exact_filter: bool = False, **kwargs: Any) -> List[Document]:
        return [d for d, _ in self.similarity_search_with_score_by_vector(
            embedding, k, filter=filter, fetch_k=fetch_k, exact_filter=exact_filter, **kwargs)]

    def similarity_search(self, query: str, k: int = 4, filter: Optional[Any] = None,
                          fetch_k: int = 20, exact_filter: bool = False,
                          **kwargs: Any) -> List[Document]:
        return [d for d, _ in self.similarity_search_with_score(
            query, k, filter=filter, fetch_k=fetch_k, exact_filter=exact_filter, **kwargs)]

    def similarity_search_within_score_by_vector(self, embedding: List[float],
                                                 score_threshold: float,
                                                 filter: Optional[Any] = None
                                                 ) -> List[Tuple[Document, float]]:
        """Every document within `score_threshold` of `embedding`, however many
        there are, as (Document, score), best first (ties by label) — a range
        search (``index.range_search``) instead of a k-bounded search cut at a
        guessed k.  The comparison is faiss's strict one: distance <
        score_threshold for an L2 index, score > score_threshold for an
        inner-product index.  `filter` restricts the hits exactly, through the
        store's selector (as ``exact_filter=True``).  Library-specific, like
        ``upsert_texts``: LangChain's FAISS store has no counterpart."""
        vector = np.array([embedding], dtype=np.float32)
        if self._normalize_L2:
            vfaiss.normalize_L2(vector)
        params = None
        if filter is not None:
            params = vfaiss.SearchParameters(sel=self._filter_selector(filter))
        _, scores, labels = self.index.range_search(vector, float(score_threshold), params=params)
        scores = np.asarray(scores)
        labels = np.asarray(labels)
        key = -scores if self.index.metric_type == vfaiss.METRIC_INNER_PRODUCT else scores
        docs = []
        for j in np.lexsort((labels, key)):
            _id = self.index_to_docstore_id[int(labels[j])]
            doc = self.docstore.search(_id)
            if not isinstance(doc, Document):
                raise ValueError(f"Could not find document for id {_id}, got {doc}")
            docs.append((doc, scores[j]))
        return docs

    def similarity_search_within_score(self, query: str, score_threshold: float,
                                       filter: Optional[Any] = None
                                       ) -> List[Tuple[Document, float]]:
        """``similarity_search_within_score_by_vector`` of the embedded query
        (library-specific)."""
        return self.similarity_search_within_score_by_vector(self._embed_query(query),
                                                             score_threshold, filter=filter)

    def similarity_search_batch_by_vector(self, embeddings, k: int = 4,
                                          distinct: Optional[str] = None, where=None,
                                          boost=None, bonus=None, bonus_key: str = "book_id"):
        """Batched variant (one engine call for many queries): list of
        [(Document, score)] per query, label -1 skipped.  ``distinct`` as in
        ``similarity_search_with_score_by_vector``; ``where``: one predicate of
        its grammar per query (or one dict for all of them), not together with
        ``distinct``; ``boost``: one boost spec per query (or one dict for all
        of them), with ``where`` or alone, not together with ``distinct``;
        ``bonus``: one ``{bonus_key value: number}`` dict per query (or one
        dict for all of them), with ``where`` and ``boost`` or alone, not
        together with ``distinct``."""
        vec = np.array(embeddings, dtype=np.float32)
        if self._normalize_L2:
            vfaiss.normalize_L2(vec)
        if where is not None and distinct is not None:
            raise ValueError("where and distinct cannot be combined")
        if boost is not None and distinct is not None:
            raise ValueError("boost and distinct cannot be combined (not built)")
        if bonus is not None and distinct is not None:
            raise ValueError("bonus and distinct cannot be combined (not built)")
        if bonus is not None:
            scores, indices = self._search_bonus(vec, k, bonus, bonus_key, boost=boost,
                                                 where=where)
        elif boost is not None:
            scores, indices = self._search_boost(vec, k, boost, where=where)
        elif where is not None:
            scores, indices = self._search_where(vec, k, where)
        elif distinct is not None:
            scores, indices = self.index.search_distinct(vec, k,
                                                         self._distinct_grouping(distinct))
        else:
            scores, indices = self.index.search(vec, k)
        out = []
        for qi in range(vec.shape[0]):
            row = []
            for j, i in enumerate(indices[qi]):
                if i == -1:
                    continue
                doc = self.docstore.search(self.index_to_docstore_id[int(i)])
                row.append((doc, scores[qi][j]))
            out.append(row)
        return out

    # -- MMR searches -----------------------------------------------------------------------
    def max_marginal_relevance_search_with_score_by_vector(
            self, embedding: List[float], *, k: int = 4, fetch_k: int = 20,
            lambda_mult: float = 0.5, filter: Optional[Any] = None,
            exact_filter: bool = False) -> List[Tuple[Document, float]]:
        """LangChain's MMR search: the `fetch_k` nearest documents re-ranked by
        maximal marginal relevance (each pick trades its cosine to the query
        against its largest cosine to the picks before it, weighted by
        `lambda_mult`: 1 = relevance only, 0 = diversity only), the first k
        picks returned in pick order.  The score of a document is the faiss
        score of the search (squared L2 / inner product), not the MMR score.
        The re-rank runs on the device (``index.search_mmr``), where LangChain
        reconstructs every candidate and loops in Python.

        With `filter`, LangChain's behaviour: search ``fetch_k * 2``, filter on
        the host, re-rank what is left (``index.mmr_select``).
        ``exact_filter=True`` makes the filter a selector instead: exactly
        min(fetch_k, matches) candidates are re-ranked."""
        vector = np.array([embedding], dtype=np.float32)
        if self._normalize_L2:
            vfaiss.normalize_L2(vector)
        if filter is None:
            scores, labels = self.index.search_mmr(vector, k, fetch_k, lambda_mult)
            return self._docs_of_row(scores[0], labels[0])
        if exact_filter:
            scores, labels = self.index.search_mmr(
                vector, k, fetch_k, lambda_mult,
                params=vfaiss.SearchParameters(sel=self._filter_selector(filter)))
            return self._docs_of_row(scores[0], labels[0])
        scores, labels = self.index.search(vector, fetch_k * 2)
        filter_func = _create_filter_func(filter)
        kept = []
        for s, i in zip(scores[0], labels[0]):
            if i == -1:
                continue
            _id = self.index_to_docstore_id[int(i)]
            doc = self.docstore.search(_id)
            if not isinstance(doc, Document):
                raise ValueError(f"Could not find document for id {_id}, got {doc}")
            if filter_func(doc.metadata):
                kept.append((doc, s, int(i)))
        if not kept:
            return []
        cand = np.array([[i for _, _, i in kept]], dtype=np.int64)
        pos = self.index.mmr_select(vector, cand, k, lambda_mult)
        return [(kept[p][0], kept[p][1]) for p in pos[0] if p >= 0]

    def max_marginal_relevance_search_by_vector(self, embedding: List[float], k: int = 4,
                                                fetch_k: int = 20, lambda_mult: float = 0.5,
                                                filter: Optional[Any] = None,
                                                **kwargs: Any) -> List[Document]:
        if kwargs.get("where") is not None:
            raise ValueError("where and mmr cannot be combined")
        if kwargs.get("boost") is not None:
            raise ValueError("boost and mmr cannot be combined (not built)")
        if kwargs.get("bonus") is not None:
            raise ValueError("bonus and mmr cannot be combined (not built)")
        return [d for d, _ in self.max_marginal_relevance_search_with_score_by_vector(
            embedding, k=k, fetch_k=fetch_k, lambda_mult=lambda_mult, filter=filter,
            exact_filter=bool(kwargs.get("exact_filter", False)))]

    def max_marginal_relevance_search(self, query: str, k: int = 4, fetch_k: int = 20,
                                      lambda_mult: float = 0.5, filter: Optional[Any] = None,
                                      **kwargs: Any) -> List[Document]:
        return self.max_marginal_relevance_search_by_vector(
            self._embed_query(query), k=k, fetch_k=fetch_k, lambda_mult=lambda_mult,
            filter=filter, **kwargs)

    def max_marginal_relevance_search_batch_by_vector(self, embeddings, k: int = 4,
                                                      fetch_k: int = 20,
                                                      lambda_mult: float = 0.5):
        """Batched variant (one engine call for many queries, library-specific
        like ``similarity_search_batch_by_vector``): a list of [(Document,
        score)] per query."""
        vec = np.array(embeddings, dtype=np.float32)
        if self._normalize_L2:
            vfaiss.normalize_L2(vec)
        scores, labels = self.index.search_mmr(vec, k, fetch_k, lambda_mult)
        return [self._docs_of_row(scores[q], labels[q]) for q in range(vec.shape[0])]

    # -- profile searches -------------------------------------------------------------------
    def _key_labels(self, field: str) -> Dict[Any, List[int]]:
        """metadata[field] -> labels holding it, ascending.  Built once per
        store generation from ``_key_index`` (every add / delete drops it)."""
        if self._keylabels is None or self._keylabels[0] != field:
            label_of = {id_: i for i, id_ in self.index_to_docstore_id.items()}
            table = {value: sorted(label_of[id_] for id_ in ids)
                     for value, ids in self._key_index(field).items()}
            self._keylabels = (field, table)
        return self._keylabels[1]

    def _docs_of_row(self, scores, labels) -> List[Tuple[Document, float]]:
        out = []
        for s, i in zip(scores, labels):
            if i == -1:
                continue
            _id = self.index_to_docstore_id[int(i)]
            doc = self.docstore.search(_id)
            if not isinstance(doc, Document):
                raise ValueError(f"Could not find document for id {_id}, got {doc}")
            out.append((doc, s))
        return out

    def profile_requests(self, profiles, exclude=None, key: str = "book_id"):
        """What ``index.search_profiles`` takes for `profiles`: (kept, rows,
        lists).  kept = the positions of the profiles with at least one key in
        the store; rows[j] = (labels, weights) of profile kept[j], a key's
        first row standing for it as the reference's scan does
        (candidate_builder.py:159-163); lists[j] = every label of its rated and
        excluded keys."""
        table = self._key_labels(key)
        kept, rows, lists = [], [], []
        for p, profile in enumerate(profiles):
            labels, weights, drop = [], [], []
            for value, weight in profile:
                found = table.get(value)
                if found:
                    labels.append(found[0])
                    weights.append(weight)
                    drop.extend(found)
            if not labels:
                continue
            if exclude is not None:
                for value in exclude[p]:
                    drop.extend(table.get(value, ()))
            kept.append(p)
            rows.append((labels, weights))
            lists.append(drop)
        return kept, rows, lists

    def recommend_for_profiles(self, profiles, k: int = 4, *, exclude=None,
                               key: str = "book_id",
                               mmr: Optional[Tuple[int, float]] = None,
                               distinct: Optional[str] = None, where=None, boost=None,
                               bonus=None, bonus_key: str = "book_id"
                               ) -> List[List[Tuple[Document, float]]]:
        """The reference's per-student candidate path
        (candidate_builder.py:138-203) for many students in one device call.
        Each profile is a list of ``(metadata[key] value, weight)`` — a
        student's rated books with their ``RATING_WEIGHTS``; ``exclude[i]``
        holds further key values profile i must not get back (the books
        already read).  The query of a profile is the weighted mean of its
        books' stored embeddings, and its result the k nearest documents that
        are neither rated nor excluded: exactly min(k, allowed) ``(Document,
        score)`` pairs, where the reference's search of ``k * 2`` rows returns
        fewer when most of them were read.  A profile none of whose keys are
        in the store gets ``[]``, as the reference returns, and takes no part
        in the device call.  Library-specific: LangChain's store has no
        counterpart.

        ``mmr=(fetch_k, lambda_mult)`` re-ranks every profile's `fetch_k`
        nearest allowed documents by maximal marginal relevance on the device
        (``index.search_mmr`` over the same mean queries and exclusions) and
        returns the first k picks in pick order, so a recommendation list does
        not fill with near-copies of one book.

        ``distinct="<metadata field>"`` returns at most one document per value
        of that field (``distinct="author"``: no author twice per student): the
        means are computed on the device, come back to the host and are
        searched by ``index.search_distinct`` with the same exclusions.  Not
        together with ``mmr``.

        ``where=[...]`` gives every profile a predicate of the ``where=``
        grammar (``similarity_search_with_score_by_vector``; one dict: the same
        for all): the k nearest allowed documents that pass it, filtered on
        the device (``index.search_where`` over the means, with the same
        exclusions).  Not together with ``mmr`` or ``distinct``.

        ``boost=[...]`` gives every profile a boost spec of the ``boost=``
        grammar (one dict: the same for all), such as the student's reading
        level: the k allowed documents with the best boosted score over the
        whole store (``index.search_boost`` over the means, with the same
        exclusions and, if given, the ``where`` predicates), where the
        reference re-scores the ``k * 2`` nearest.  Not together with ``mmr``
        or ``distinct``.

        ``bonus=[...]`` gives every profile a dict ``metadata[bonus_key] value
        -> number`` (one dict: the same for all), such as
        ``students.neighbour_bonus``'s social term: the number is added to the
        score of every document with that value before the ranking over the
        whole store (``index.search_bonus`` over the means, with the same
        exclusions and, if given, the ``where`` predicates and ``boost``
        specs).  Not together with ``mmr`` or ``distinct``."""
        if distinct is not None and mmr is not None:
            raise ValueError("distinct and mmr cannot be combined")
        if boost is not None and (mmr is not None or distinct is not None):
            raise ValueError("boost cannot be combined with mmr or distinct (not built)")
        if bonus is not None and (mmr is not None or distinct is not None):
            raise ValueError("bonus cannot be combined with mmr or distinct (not built)")
        if where is not None and mmr is not None:
            raise ValueError("where and mmr cannot be combined")
        if where is not None and distinct is not None:
            raise ValueError("where and distinct cannot be combined")
        profiles = list(profiles)
        if where is not None and not isinstance(where, dict):
            where = list(where)
            _len_check_if_sized(profiles, where, "profiles", "where")
        if boost is not None and not isinstance(boost, dict):
            boost = list(boost)
            _len_check_if_sized(profiles, boost, "profiles", "boost")
        if bonus is not None and not isinstance(bonus, dict):
            bonus = list(bonus)
            _len_check_if_sized(profiles, bonus, "profiles", "bonus")
        if exclude is not None:
            exclude = list(exclude)
            _len_check_if_sized(profiles, exclude, "profiles", "exclude")
        out: List[List[Tuple[Document, float]]] = [[] for _ in profiles]
        kept, rows, lists = self.profile_requests(profiles, exclude, key)
        if not kept:
            return out
        if bonus is not None:
            vec = self.index.mean_rows(rows)
            if self._normalize_L2:
                vfaiss.normalize_L2(vec)
            scores, labels = self._search_bonus(
                vec, k, bonus if isinstance(bonus, dict) else [bonus[p] for p in kept], bonus_key,
                boost=boost if boost is None or isinstance(boost, dict)
                else [boost[p] for p in kept],
                where=where if where is None or isinstance(where, dict)
                else [where[p] for p in kept], exclude=lists)
        elif boost is not None:
            vec = self.index.mean_rows(rows)
            if self._normalize_L2:
                vfaiss.normalize_L2(vec)
            scores, labels = self._search_boost(
                vec, k, boost if isinstance(boost, dict) else [boost[p] for p in kept],
                where=where if where is None or isinstance(where, dict)
                else [where[p] for p in kept], exclude=lists)
        elif where is not None:
            vec = self.index.mean_rows(rows)
            if self._normalize_L2:
                vfaiss.normalize_L2(vec)
            scores, labels = self._search_where(
                vec, k, where if isinstance(where, dict) else [where[p] for p in kept],
                exclude=lists)
        elif distinct is not None:
            vec = self.index.mean_rows(rows)
            if self._normalize_L2:
                vfaiss.normalize_L2(vec)
            scores, labels = self.index.search_distinct(vec, k, self._distinct_grouping(distinct),
                                                        exclude=lists)
        elif mmr is not None:
            fetch_k, lambda_mult = mmr
            vec = self.index.mean_rows(rows)
            if self._normalize_L2:
                vfaiss.normalize_L2(vec)
            scores, labels = self.index.search_mmr(vec, k, int(fetch_k), float(lambda_mult),
                                                   exclude=lists)
        elif self._normalize_L2:  # the store normalises every query it searches
            vec = self.index.mean_rows(rows)
            vfaiss.normalize_L2(vec)
            scores, labels = self.index.search(vec, k, exclude=lists)
        else:
            scores, labels = self.index.search_profiles(rows, k, exclude=lists,
                                                        exclude_profile=False)
        for j, p in enumerate(kept):
            out[p] = self._docs_of_row(scores[j], labels[j])
        return out

    # -- example searches -------------------------------------------------------------------
    def example_requests(self, liked, disliked=None, exclude=None, key: str = "book_id"):
        """What ``index.search_examples`` takes for the users' liked and
        disliked key values: (kept, positive, negative, lists, names).  kept =
        the positions of the users with at least one liked key in the store;
        positive[j] / negative[j] = the example labels of user kept[j], a key's
        first row standing for it as in ``profile_requests`` (keys the store
        does not hold drop out); lists[j] = every label of its liked, disliked
        and excluded keys; names[j][i] = the key value of positive[j][i]."""
        table = self._key_labels(key)
        kept, positive, negative, lists, names = [], [], [], [], []
        for u, values in enumerate(liked):
            pos, neg, drop, name = [], [], [], []
            for value in values:
                found = table.get(value)
                if found:
                    pos.append(found[0])
                    name.append(value)
                    drop.extend(found)
            if not pos:
                continue
            for value in (disliked[u] if disliked is not None else ()):
                found = table.get(value)
                if found:
                    neg.append(found[0])
                    drop.extend(found)
            for value in (exclude[u] if exclude is not None else ()):
                drop.extend(table.get(value, ()))
            kept.append(u)
            positive.append(pos)
            negative.append(neg)
            lists.append(drop)
            names.append(name)
        return kept, positive, negative, lists, names

    def recommend_from_examples(self, liked, disliked=None, k: int = 4, *, exclude=None,
                                key: str = "book_id", with_reason: bool = False):
        """Recommendations from a reader's feedback itself instead of its mean
        (``index.search_examples``; Qdrant's ``recommend`` with
        ``strategy="best_score"``).  ``liked[i]`` / ``disliked[i]`` hold the
        ``metadata[key]`` values user i rated up / down, ``exclude[i]`` further
        values it must not get back.  A document is scored by its nearest liked
        book and dropped when a disliked book is at least as near, so a
        thumbs-down pushes away instead of pulling, and two tastes stay two
        tastes.  No row of a liked, disliked or excluded key comes back.
        Returns per user exactly min(k, such documents) ``(Document, score)``
        pairs, best first; ``with_reason`` appends the liked key value that
        decided each ("because you liked X").  A user none of whose liked keys
        are in the store gets ``[]``.  Library-specific: LangChain's store has
        no counterpart."""
        liked = [list(v) for v in liked]
        if disliked is not None:
            disliked = [list(v) for v in disliked]
            _len_check_if_sized(liked, disliked, "liked", "disliked")
        if exclude is not None:
            exclude = [list(v) for v in exclude]
            _len_check_if_sized(liked, exclude, "liked", "exclude")
        out: List[list] = [[] for _ in liked]
        kept, positive, negative, lists, names = self.example_requests(liked, disliked, exclude,
                                                                       key)
        if not kept:
            return out
        if self._normalize_L2:  # the store normalises every vector it searches

            def rows(labels):
                vec = np.stack([self.index.reconstruct(int(l)) for l in labels]) if labels else \
                    np.zeros((0, self.index.d), dtype=np.float32)
                vec = np.ascontiguousarray(vec, dtype=np.float32)
                vfaiss.normalize_L2(vec)
                return vec

            positive = [rows(p) for p in positive]
            negative = [rows(n) for n in negative]
        scores, labels, reason = self.index.search_examples(
            positive, negative, k, exclude=lists, exclude_examples=False, return_example=True)
        for j, u in enumerate(kept):
            docs = self._docs_of_row(scores[j], labels[j])
            if with_reason:
                docs = [(doc, s, names[j][int(e)])
                        for (doc, s), e in zip(docs, reason[j][labels[j] != -1])]
            out[u] = docs
        return out

    def _select_relevance_score_fn(self) -> Callable[[float], float]:
        if self.override_relevance_score_fn is not None:
            return self.override_relevance_score_fn
        if self.distance_strategy == DistanceStrategy.MAX_INNER_PRODUCT:
            return lambda s: 1.0 - s if s > 0 else -1.0 * s
        if self.distance_strategy == DistanceStrategy.EUCLIDEAN_DISTANCE:
            return lambda d: 1.0 - d / math.sqrt(2)
        if self.distance_strategy == DistanceStrategy.COSINE:
            return lambda d: 1.0 - d
        raise ValueError("Unknown distance strategy, must be cosine, max_inner_product,"
                         " or euclidean")

    def similarity_search_with_relevance_scores(self, query: str, k: int = 4,
                                                filter: Optional[Any] = None, fetch_k: int = 20,
                                                exact_filter: bool = False, **kwargs: Any):
        fn = self._select_relevance_score_fn()
        score_threshold = kwargs.pop("score_threshold", None)
        docs = self.similarity_search_with_score(query, k=k, filter=filter, fetch_k=fetch_k,
                                                 exact_filter=exact_filter, **kwargs)
        out = [(doc, fn(score)) for doc, score in docs]
        if score_threshold is not None:
            out = [(d, s) for d, s in out if s >= score_threshold]
        return out

    # -- construction -------------------------------------------------------------------------
    @classmethod
    def __from(cls, texts, embeddings, embedding, metadatas=None, ids=None,
               normalize_L2: bool = False,
               distance_strategy: DistanceStrategy = DistanceStrategy.EUCLIDEAN_DISTANCE,
               **kwargs: Any) -> "FAISS":
        device = kwargs.pop("device", None)
        dim = len(embeddings[0])
        if distance_strategy == DistanceStrategy.MAX_INNER_PRODUCT:
            index = vfaiss.IndexFlatIP(dim, device=device)
        else:
            index = vfaiss.IndexFlatL2(dim, device=device)
        docstore = kwargs.pop("docstore", InMemoryDocstore())
        index_to_docstore_id = kwargs.pop("index_to_docstore_id", {})
        vecstore = cls(embedding, index, docstore, index_to_docstore_id,
                       normalize_L2=normalize_L2, distance_strategy=distance_strategy, **kwargs)
        vecstore.__add(texts, embeddings, metadatas=metadatas, ids=ids)
        return vecstore

    @classmethod
    def from_texts(cls, texts: List[str], embedding, metadatas: Optional[List[dict]] = None,
                   ids: Optional[List[str]] = None, **kwargs: Any) -> "FAISS":
        embeddings = embedding.embed_documents(texts)
        return cls.__from(texts, embeddings, embedding, metadatas=metadatas, ids=ids, **kwargs)

    @classmethod
    def from_embeddings(cls, text_embeddings: Iterable[Tuple[str, List[float]]], embedding,
                        metadatas: Optional[List[dict]] = None, ids: Optional[List[str]] = None,
                        **kwargs: Any) -> "FAISS":
        texts, embeddings = zip(*text_embeddings)
        return cls.__from(list(texts), list(embeddings), embedding, metadatas=metadatas, ids=ids,
                          **kwargs)

    # -- persistence ----------------------------------------------------------------------------
    def save_local(self, folder_path: str, index_name: str = "index") -> None:
        path = Path(folder_path)
        path.mkdir(exist_ok=True, parents=True)
        vfaiss.write_index(self.index, str(path / f"{index_name}.faiss"))
        store = getattr(self.docstore, "_dict", None)
        if store is None:
            raise ValueError("save_local: only InMemoryDocstore-like docstores are supported")
        payload = {
            "format": "vsearch-docstore-v1",
            "index_to_docstore_id": [[int(i), _id] for i, _id in self.index_to_docstore_id.items()],
            "docstore": {k: v.to_json() for k, v in store.items()},
        }
        tmp = path / f"{index_name}.docstore.json.tmp"
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump(payload, f)
        tmp.replace(path / f"{index_name}.docstore.json")

    @classmethod
    def load_local(cls, folder_path: str, embeddings, index_name: str = "index", *,
                   allow_dangerous_deserialization: bool = False, **kwargs: Any) -> "FAISS":
        if not allow_dangerous_deserialization:
            raise ValueError(
                "The de-serialization relies loading a pickle file. Pickle files can be modified "
                "to deliver a malicious payload that results in execution of arbitrary code on "
                "your machine.You will need to set `allow_dangerous_deserialization` to `True` "
                "to enable deserialization. If you do this, make sure that you trust the source "
                "of the data. For example, if you are loading a file that you created, and know "
                "that no one else has modified the file, then this is safe to do. Do not set "
                "this to `True` if you are loading a file from an untrusted source (e.g., some "
                "random site on the internet.)."
            )
        path = Path(folder_path)
        if not (path / f"{index_name}.docstore.json").exists() and \
                (path / f"{index_name}.pkl").exists():
            # a store written by LangChain itself: its docstore is a pickle of
            # LangChain classes, which this loader never unpickles
            raise ReferenceStoreError(
                f"{path}: found {index_name}.pkl (a LangChain pickle) but no "
                f"{index_name}.docstore.json. Migrate it once with "
                "vsearch.langchain.migrate_reference_store (the vectors of "
                f"{index_name}.faiss kept, the docstore rebuilt from the catalog rows in "
                "label order, no re-embedding), or rebuild it with "
                "vsearch.langchain.full_faiss_rebuild (the reference's own book_vector "
                "full_faiss_rebuild, main.py:428-471); the pickle is not loaded.")
        index = vfaiss.read_index(str(path / f"{index_name}.faiss"),
                                  device=kwargs.pop("device", None),
                                  index_factory=kwargs.pop("index_factory", None))
        with open(path / f"{index_name}.docstore.json", "r", encoding="utf-8") as f:
            payload = json.load(f)
        docstore = InMemoryDocstore({k: Document.from_json(v)
                                     for k, v in payload["docstore"].items()})
        index_to_docstore_id = {int(i): _id for i, _id in payload["index_to_docstore_id"]}
        return cls(embeddings, index, docstore, index_to_docstore_id, **kwargs)


class ReferenceStoreError(ValueError):
    """load_local found a LangChain-written store (index.pkl docstore) that this
    drop-in does not unpickle; see full_faiss_rebuild."""


def migrate_reference_store(folder_path: str, texts: List[str], metadatas: List[dict],
                            embeddings=None, ids: Optional[List[str]] = None,
                            index_name: str = "index", *, verify_sample: int = 8,
                            verify_min_cosine: float = 0.999,
                            **kwargs: Any) -> "FAISS":
    """Migrates a store the reference wrote (``index.faiss`` + LangChain's pickled
    ``index.pkl``) WITHOUT re-embedding the catalogue: the vectors are read from
    ``index.faiss`` (faiss's flat format, vsearch.faiss.read_index) onto the GPU,
    and the docstore — which lives only in the pickle, never opened here — is
    rebuilt from the caller's catalogue rows.

    ``texts`` / ``metadatas`` must be the rows in the order the store was built,
    i.e. label order: the reference's full rebuild embeds
    ``SELECT ... FROM catalog`` row by row with the main.py:449-460 text and the
    main.py:461-465 metadata (vsearch.synth.book_text / book_metadata restate
    both) and appends incremental books with ``add_texts`` (main.py:148).  A row
    count that differs from ``index.faiss``'s ntotal is refused.  ``ids``
    default to fresh uuid4 strings, as ``FAISS.from_texts`` assigns them
    (docstore ids are internal to the store: the reference's readers use
    ``metadata["book_id"]``).

    The label order is checked by default: ``verify_sample`` (8) evenly spaced
    texts are embedded with ``embeddings`` and each must point the same way as
    its stored row (cosine >= ``verify_min_cosine``; a remote embedding API is
    not bit-reproducible, so no element-wise comparison), at that many
    embedding calls instead of the whole catalogue.  The reference's rebuild
    query has no ORDER BY (book_vector/main.py:439), so the caller must give
    the rows in the order that query returned them when the store was built;
    a store that ``ensure_store`` seeded (main.py:121: ``from_texts(["dummy"],
    metadatas=[{"book_id": "dummy"}])`` before the first ``add_texts``) holds
    that row at label 0, and it must be passed too.  ``verify_sample=0`` skips
    the check (only when the order is known by construction).
    Writes ``index.docstore.json`` beside the untouched ``index.faiss`` /
    ``index.pkl``; afterwards ``FAISS.load_local`` opens the directory."""
    path = Path(folder_path)
    index = vfaiss.read_index(str(path / f"{index_name}.faiss"),
                              device=kwargs.pop("device", None),
                              index_factory=kwargs.pop("index_factory", None))
    texts = list(texts)
    metadatas = list(metadatas)
    n = int(index.ntotal)
    if len(texts) != n or len(metadatas) != n:
        raise ValueError(f"migrate_reference_store: {index_name}.faiss holds {n} rows but "
                         f"{len(texts)} texts / {len(metadatas)} metadatas were given (the rows "
                         "must be the catalogue in the store's label order)")
    ids = list(ids) if ids is not None else [str(uuid.uuid4()) for _ in texts]
    if len(ids) != n or len(set(ids)) != n:
        raise ValueError("migrate_reference_store: ids must be n distinct strings")
    if verify_sample > 0 and n:
        if embeddings is None:
            raise ValueError("migrate_reference_store: the label-order check needs embeddings "
                             "(or verify_sample=0 when the row order is known)")
        pick = sorted({int(i) for i in np.linspace(0, n - 1, min(verify_sample, n))})
        got = np.asarray(embeddings.embed_documents([texts[i] for i in pick]), dtype=np.float64)
        for j, i in enumerate(pick):
            row = np.asarray(index.reconstruct(i), dtype=np.float64)
            den = float(np.linalg.norm(row) * np.linalg.norm(got[j]))
            cos = float(row @ got[j]) / den if den > 0 else (1.0 if not row.any() and
                                                             not got[j].any() else 0.0)
            if not cos >= verify_min_cosine:
                raise ValueError(f"migrate_reference_store: row {i} of {index_name}.faiss is "
                                 f"not the embedding of texts[{i}] (cosine {cos:.6f} < "
                                 f"{verify_min_cosine}): the rows are not in the store's "
                                 "label order (a store seeded by ensure_store holds its "
                                 "'dummy' row at label 0)")
    docstore = InMemoryDocstore({_id: Document(page_content=t, metadata=m, id=_id)
                                 for t, m, _id in zip(texts, metadatas, ids)})
    store = FAISS(embeddings, index, docstore, dict(enumerate(ids)), **kwargs)
    payload = {
        "format": "vsearch-docstore-v1",
        "index_to_docstore_id": [[i, _id] for i, _id in enumerate(ids)],
        "docstore": {k: v.to_json() for k, v in docstore._dict.items()},
    }
    tmp = path / f"{index_name}.docstore.json.tmp"
    with open(tmp, "w", encoding="utf-8") as f:
        json.dump(payload, f)
    tmp.replace(path / f"{index_name}.docstore.json")
    return store


def full_faiss_rebuild(texts: List[str], embeddings, metadatas: List[dict], folder_path: str,
                       ids: Optional[List[str]] = None, index_name: str = "index",
                       **kwargs: Any) -> "FAISS":
    """The migration path from a reference-written store: the reference's own
    full rebuild (src/incremental_workers/book_vector/main.py:428-471: one
    ``FAISS.from_texts`` over every catalog row with the main.py:449-466 text
    and metadata, then ``save_local(vec_dir)``), writing this drop-in's format
    (index.faiss + index.docstore.json) into the same directory.  Files the
    reference wrote there (index.pkl) are left untouched and no longer read."""
    store = FAISS.from_texts(list(texts), embeddings, metadatas=list(metadatas), ids=ids,
                             **kwargs)
    store.save_local(folder_path, index_name=index_name)
    return store

