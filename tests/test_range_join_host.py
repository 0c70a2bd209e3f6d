"""CPU: the host side of the range self-join (vs_range_selfjoin).

The C-ABI's argument checks run before any device call, so they are tested
without a GPU.  ``IndexFlat.range_selfjoin``'s chunking runs over a fake of the
one C call it makes, and ``vsearch.students``' edge functions over a numpy test
double of the index (JoinIndex below): the mirroring of the upper join, the
order of the rows and the key mapping are host logic.  The arithmetic on the
device is test_gpu_range_join.py's."""

import ctypes

import numpy as np
import pytest

from vsearch import _lib
from vsearch import faiss as vfaiss
from vsearch import students


def test_symbol_exported_and_in_signatures():
    lib = _lib.load()
    assert "vs_range_selfjoin" in _lib.SIGNATURES
    assert hasattr(lib, "vs_range_selfjoin")
    res, args = _lib.SIGNATURES["vs_range_selfjoin"]
    assert res is ctypes.c_int and len(args) == 9


def test_argument_checks_are_host_side():
    lib = _lib.load()
    out = ctypes.c_void_p()
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)

    def call(idx, q0, nq, outp):
        return lib.vs_range_selfjoin(idx, q0, nq, 0.75, 1, 0, 0, None, outp)

    assert call(None, 0, 1, ctypes.byref(out)) == _lib.E_INVALID
    assert _lib.last_error() == "vs_range_selfjoin: null index"
    assert not out.value
    # a null `out` is checked before the index is looked at
    assert call(None, 0, 1, None) == _lib.E_INVALID
    assert _lib.last_error() == "vs_range_selfjoin: null output"
    # the rows (the non-null "index" is a zeroed buffer these checks never read)
    for q0, nq in ((-1, 1), (0, -1)):
        assert call(fake, q0, nq, ctypes.byref(out)) == _lib.E_INVALID
        assert _lib.last_error() == "vs_range_selfjoin: query rows out of range"
    # the index is checked before the rows
    assert call(None, -1, -1, ctypes.byref(out)) == _lib.E_INVALID
    assert _lib.last_error() == "vs_range_selfjoin: null index"
    assert call(fake, 0, 65537, ctypes.byref(out)) == _lib.E_UNSUPPORTED
    assert "65536" in _lib.last_error()
    assert not out.value


def _bare_index(d):
    """An IndexFlat without a device: range_selfjoin with nq given needs only
    the one C call, which the tests replace."""
    index = object.__new__(vfaiss.IndexFlat)
    index._d = d
    index._h = None
    return index


def test_range_selfjoin_chunks_concatenate(monkeypatch):
    calls = []

    def fake_call(self, q0, nq, min_sim, exclude_self, upper):
        # row j has j % 4 hits: labels 100 j + i, similarities j + i / 8
        calls.append((q0, nq, min_sim, exclude_self, upper))
        counts = [(q0 + j) % 4 for j in range(nq)]
        lims = np.zeros(nq + 1, dtype=np.int64)
        lims[1:] = np.cumsum(counts)
        S = np.array([q0 + j + i / 8 for j, c in enumerate(counts) for i in range(c)],
                     dtype=np.float32)
        I = np.array([100 * (q0 + j) + i for j, c in enumerate(counts) for i in range(c)],
                     dtype=np.int64)
        return lims, S, I

    monkeypatch.setattr(vfaiss.IndexFlat, "_range_join_call", fake_call)
    index = _bare_index(4)
    lims, S, I = index.range_selfjoin(0.25, q0=3, nq=11, upper=True, chunk=4)
    assert [(c[0], c[1]) for c in calls] == [(3, 4), (7, 4), (11, 3)]
    assert all(c[2:] == (0.25, True, True) for c in calls)
    assert lims.dtype == np.uint64 and S.dtype == np.float32 and I.dtype == np.int64
    counts = [(3 + j) % 4 for j in range(11)]
    np.testing.assert_array_equal(lims, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64))
    for j in range(11):
        a, b = int(lims[j]), int(lims[j + 1])
        np.testing.assert_array_equal(I[a:b], 100 * (3 + j) + np.arange(counts[j]))
        np.testing.assert_array_equal(
            S[a:b], (3 + j + np.arange(counts[j]) / 8).astype(np.float32))
    # one chunk: the call's arrays, lims as uint64
    calls.clear()
    lims1, S1, I1 = index.range_selfjoin(0.25, q0=3, nq=11, exclude_self=False)
    assert calls == [(3, 11, 0.25, False, False)]
    np.testing.assert_array_equal(lims1, lims)
    np.testing.assert_array_equal(S1, S)
    np.testing.assert_array_equal(I1, I)
    # no rows: no call
    calls.clear()
    lims0, S0, I0 = index.range_selfjoin(0.25, q0=3, nq=0)
    assert calls == [] and lims0.tolist() == [0] and lims0.dtype == np.uint64
    assert S0.dtype == np.float32 and I0.dtype == np.int64 and S0.size == 0 and I0.size == 0


# ---- vsearch.students over a numpy double of the index ------------------------------------------
class JoinIndex:
    """What the edge functions use of an index: ``range_selfjoin`` in numpy,
    fp32 roundings of the fp64 cosines, >= min_sim, ascending rows."""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float64)
        self.calls = []

    @property
    def ntotal(self):
        return self.x.shape[0]

    def range_selfjoin(self, min_sim, *, q0=0, nq=None, exclude_self=True, upper=False,
                       chunk=65536):
        self.calls.append(dict(min_sim=min_sim, q0=q0, nq=nq, exclude_self=exclude_self,
                               upper=upper))
        n = self.ntotal
        nq = n - q0 if nq is None else nq
        nrm = np.sqrt((self.x * self.x).sum(axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            s = ((self.x[q0:q0 + nq] @ self.x.T) / (nrm[q0:q0 + nq, None] * nrm[None, :]))
        s = s.astype(np.float32)
        hit = s >= np.float32(min_sim)
        rows = np.arange(n)[None, :]
        qrow = np.arange(q0, q0 + nq)[:, None]
        if exclude_self:
            hit &= rows != qrow
        if upper:
            hit &= rows > qrow
        lims = np.zeros(nq + 1, dtype=np.uint64)
        lims[1:] = np.cumsum(hit.sum(axis=1))
        q, r = np.nonzero(hit)
        return lims, s[q, r], r.astype(np.int64)


KEYS = ["ann", "bob", "cy", "dee", "eve", "fay"]
# two tight groups (rows 0, 2, 5 and rows 1, 3), and row 4 on its own
VECS = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.99, 0.1, 0.0], [0.05, 1.0, 0.02],
                 [0.0, 0.0, 1.0], [0.98, 0.0, 0.15]], dtype=np.float32)


@pytest.fixture
def patched(monkeypatch):
    made = []

    def build(vectors, *, quantize=True, device=None):
        made.append(JoinIndex(vectors))
        return made[-1]

    monkeypatch.setattr(students, "build_student_index", build)
    return made


def _pairs(x, t):
    x = np.asarray(x, dtype=np.float64)
    nrm = np.sqrt((x * x).sum(axis=1))
    s = ((x @ x.T) / (nrm[:, None] * nrm[None, :])).astype(np.float32)
    return [(a, b, float(s[a, b])) for a in range(len(x)) for b in range(len(x))
            if a != b and s[a, b] >= np.float32(t)]


def test_student_edges_directed_and_undirected(patched):
    want = _pairs(VECS, 0.75)
    assert {(a, b) for a, b, _ in want} == {(0, 2), (2, 0), (0, 5), (5, 0), (2, 5), (5, 2),
                                            (1, 3), (3, 1)}
    rows = students.student_edges(KEYS, VECS, threshold=0.75)
    # both directions, ordered by a's position then b's, keys mapped
    assert rows == [(KEYS[a], KEYS[b], s) for a, b, s in want]
    # built from ONE upper join, mirrored on the host: (b, a) carries (a, b)'s value
    assert len(patched) == 1 and len(patched[0].calls) == 1
    assert patched[0].calls[0]["upper"] is True and patched[0].calls[0]["exclude_self"] is True
    assert patched[0].calls[0]["min_sim"] == 0.75
    sim = {(a, b): s for a, b, s in rows}
    assert all(sim[(b, a)] == s for (a, b), s in sim.items())
    # each pair once, a before b
    once = students.student_edges(KEYS, VECS, threshold=0.75, directed=False)
    assert once == [(KEYS[a], KEYS[b], s) for a, b, s in want if a < b]
    assert len(once) * 2 == len(rows)


def test_student_edges_empty_and_none_passing(patched):
    assert students.student_edges([], np.zeros((0, 3), dtype=np.float32)) == []
    assert patched == []  # no index is built for no students
    assert students.student_edges(KEYS, VECS, threshold=0.9999) == []
    assert students.student_edges(KEYS, VECS, threshold=0.9999, directed=False) == []


def test_student_index_edges_and_edges_of(patched):
    index = students.StudentIndex(KEYS, VECS)
    want = _pairs(VECS, 0.75)
    assert index.edges(0.75) == [(KEYS[a], KEYS[b], s) for a, b, s in want]
    assert index.edges(0.75, directed=False) == [(KEYS[a], KEYS[b], s) for a, b, s in want
                                                 if a < b]
    assert index.edges() == index.edges(students.DEFAULT_THRESHOLD)
    double = patched[0]
    for name in KEYS:
        double.calls.clear()
        a = KEYS.index(name)
        assert index.edges_of(name, 0.75) == [(name, KEYS[b], s) for x, b, s in want if x == a]
        # one row, the full (not the upper) join of it
        assert double.calls == [dict(min_sim=0.75, q0=a, nq=1, exclude_self=True, upper=False)]
    assert index.edges_of("eve", 0.75) == []
    with pytest.raises(KeyError):
        index.edges_of("nobody", 0.75)
