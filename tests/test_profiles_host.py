"""CPU: the host side of profile searches — argument checks of the C entry
points that need no device, the Python CSR builders, the store's and the
service's grouping with per-row exclusions (against an oracle index), and the
numpy statement of the mean that the kernel is tested against."""

import ctypes
import threading

import numpy as np
import pytest

from helpers import OracleIndex
from oracle import flat
from vsearch import _lib
from vsearch import faiss as vfaiss
from vsearch import langchain as vlc
from vsearch.service import IndexService, RemoteFAISS, _Coalescer
from vsearch.synth import SynthEmbeddings

KEY = b"test-secret"


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


# ---- C entry points -----------------------------------------------------------------
def test_null_index_is_invalid():
    lib = _lib.load()
    x = np.zeros((2, 8), dtype=np.float32)
    D = np.zeros((2, 3), dtype=np.float32)
    I = np.zeros((2, 3), dtype=np.int64)
    offs = _i64([0, 1, 2])
    labels = _i64([0, 1])
    w = np.ones(2, dtype=np.float32)
    assert lib.vs_search_excl(None, x.ctypes.data, 2, 3, offs.ctypes.data, labels.ctypes.data,
                              D.ctypes.data, I.ctypes.data, 0, None) == _lib.E_INVALID
    assert "null index" in _lib.last_error()
    assert lib.vs_mean_rows(None, offs.ctypes.data, labels.ctypes.data, w.ctypes.data, 2,
                            x.ctypes.data, 0, None) == _lib.E_INVALID
    assert "null index" in _lib.last_error()
    assert lib.vs_search_profiles(None, offs.ctypes.data, labels.ctypes.data, w.ctypes.data, 2, 3,
                                  None, None, 1, D.ctypes.data, I.ctypes.data, 0,
                                  None) == _lib.E_INVALID
    assert "null index" in _lib.last_error()


@pytest.fixture
def dummy_index():
    """A non-null handle that is never read.  vs_create needs a device, and the
    checks below are made before the index is touched, so zeroed memory stands
    in for the handle on a host without one."""
    buf = ctypes.create_string_buffer(4096)
    yield ctypes.cast(buf, ctypes.c_void_p)
    del buf


@pytest.mark.parametrize("offs", [[1, 1, 2], [0, 2, 1]])
def test_bad_offsets_are_invalid(dummy_index, offs):
    lib = _lib.load()
    x = np.zeros((2, 8), dtype=np.float32)
    D = np.zeros((2, 3), dtype=np.float32)
    I = np.zeros((2, 3), dtype=np.int64)
    offs = _i64(offs)
    good = _i64([0, 1, 2])
    labels = _i64([0, 1, 0])
    w = np.ones(3, dtype=np.float32)
    assert lib.vs_search_excl(dummy_index, x.ctypes.data, 2, 3, offs.ctypes.data,
                              labels.ctypes.data, D.ctypes.data, I.ctypes.data, 0,
                              None) == _lib.E_INVALID
    assert "offsets" in _lib.last_error()
    assert lib.vs_mean_rows(dummy_index, offs.ctypes.data, labels.ctypes.data, w.ctypes.data, 2,
                            x.ctypes.data, 0, None) == _lib.E_INVALID
    assert "offsets" in _lib.last_error()
    assert lib.vs_search_profiles(dummy_index, offs.ctypes.data, labels.ctypes.data,
                                  w.ctypes.data, 2, 3, None, None, 1, D.ctypes.data,
                                  I.ctypes.data, 0, None) == _lib.E_INVALID
    assert "offsets" in _lib.last_error()
    assert lib.vs_search_profiles(dummy_index, good.ctypes.data, labels.ctypes.data,
                                  w.ctypes.data, 2, 3, offs.ctypes.data, labels.ctypes.data, 1,
                                  D.ctypes.data, I.ctypes.data, 0, None) == _lib.E_INVALID
    assert "offsets" in _lib.last_error()


def test_empty_profile_and_bad_k_are_invalid(dummy_index):
    lib = _lib.load()
    x = np.zeros((2, 8), dtype=np.float32)
    D = np.zeros((2, 3), dtype=np.float32)
    I = np.zeros((2, 3), dtype=np.int64)
    offs = _i64([0, 0, 2])
    labels = _i64([0, 1])
    w = np.ones(2, dtype=np.float32)
    assert lib.vs_mean_rows(dummy_index, offs.ctypes.data, labels.ctypes.data, w.ctypes.data, 2,
                            x.ctypes.data, 0, None) == _lib.E_INVALID
    assert "empty profile" in _lib.last_error()
    good = _i64([0, 1, 2])
    assert lib.vs_search_profiles(dummy_index, good.ctypes.data, labels.ctypes.data,
                                  w.ctypes.data, 2, 0, None, None, 1, D.ctypes.data,
                                  I.ctypes.data, 0, None) == _lib.E_INVALID
    assert lib.vs_search_excl(dummy_index, x.ctypes.data, 2, 0, good.ctypes.data,
                              labels.ctypes.data, D.ctypes.data, I.ctypes.data, 0,
                              None) == _lib.E_INVALID
    assert lib.vs_search_excl(dummy_index, x.ctypes.data, -1, 3, None, None, D.ctypes.data,
                              I.ctypes.data, 0, None) == _lib.E_INVALID


# ---- CSR builders -------------------------------------------------------------------
def test_exclusion_csr_forms():
    offs, labels = vfaiss.exclusion_csr([[3, 1], [], np.asarray([7]), (), [2, 2, -1]], 5)
    assert offs.dtype == np.int64 and labels.dtype == np.int64
    assert offs.tolist() == [0, 2, 2, 3, 3, 6]
    assert labels.tolist() == [3, 1, 7, 2, 2, -1]
    o2, l2 = vfaiss.exclusion_csr((offs, labels), 5)
    assert o2.tolist() == offs.tolist() and l2.tolist() == labels.tolist()
    o3, l3 = vfaiss.exclusion_csr([[] for _ in range(4)], 4)
    assert o3.tolist() == [0] * 5 and l3.size == 0 and l3.dtype == np.int64
    o4, l4 = vfaiss.exclusion_csr(None, 3)
    assert o4.tolist() == [0] * 4 and l4.size == 0
    o5, l5 = vfaiss.exclusion_csr([], 0)
    assert o5.tolist() == [0] and l5.size == 0
    # two label lists given as a tuple of arrays stay two lists
    o6, l6 = vfaiss.exclusion_csr((np.asarray([5, 6, 7]), np.asarray([8])), 2)
    assert o6.tolist() == [0, 3, 4] and l6.tolist() == [5, 6, 7, 8]
    with pytest.raises(ValueError):
        vfaiss.exclusion_csr([[1], [2]], 3)


def test_profile_csr_forms():
    offs, labels, weights = vfaiss.profile_csr([([4, 5], [0.5, 1.0]), (np.asarray([9]), [0.1])])
    assert offs.tolist() == [0, 2, 3] and labels.tolist() == [4, 5, 9]
    assert weights.dtype == np.float32
    np.testing.assert_array_equal(weights, np.asarray([0.5, 1.0, 0.1], dtype=np.float32))
    offs, labels, weights = vfaiss.profile_csr([])
    assert offs.tolist() == [0] and labels.size == 0 and weights.size == 0
    with pytest.raises(ValueError):
        vfaiss.profile_csr([([1, 2], [1.0])])


def test_exclude_with_selector_raises():
    # the check comes before any library call: no handle is needed
    index = vfaiss.IndexFlat.__new__(vfaiss.IndexFlat)
    index._d = 4
    index._h = None
    x = np.zeros((2, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="not both"):
        index.search(x, 3, exclude=[[1], []],
                     params=vfaiss.SearchParameters(sel=vfaiss.IDSelectorAll()))


# ---- the mean's definition ------------------------------------------------------------
def mean_definition(rows, labels, weights):
    """include/vsearch.h vs_mean_rows, element by element in fp32:
    acc = x0 * w0; acc = fl(acc + fl(xi * wi)); q = fl(acc / W),
    W = the double sum of the fp32 weights in list order, rounded once."""
    w32 = np.asarray(weights, dtype=np.float32)
    acc = rows[labels[0]] * w32[0]
    total = float(w32[0])
    for l, w in zip(labels[1:], w32[1:]):
        acc = (acc + (rows[l] * w).astype(np.float32)).astype(np.float32)
        total += float(w)
    return (acc / np.float32(total)).astype(np.float32)


@pytest.mark.parametrize("d", [70, 1536])
def test_mean_definition_is_numpys_sum(d):
    rng = np.random.default_rng(d)
    rows = rng.standard_normal((300, d)).astype(np.float32)
    choices = np.asarray([0.1, 0.3, 0.5, 0.8, 1.0])
    for size in (1, 2, 3, 8, 9, 127, 128, 129, 257):
        labels = rng.integers(0, 300, size)
        w = rng.choice(choices, size)
        w32 = w.astype(np.float32)
        total = 0.0
        for v in w32:
            total += float(v)
        # candidate_builder.py:167-184 with float32 weights
        ref = np.sum([rows[l] * v for l, v in zip(labels, w32)], axis=0) / np.float32(total)
        assert ref.dtype == np.float32
        np.testing.assert_array_equal(mean_definition(rows, labels, w), ref, err_msg=str(size))


# ---- store and service over an oracle index -------------------------------------------
class ExclOracleIndex(OracleIndex):
    """OracleIndex with the profile surface of IndexFlat."""

    def __init__(self, d, metric=flat.METRIC_L2):
        super().__init__(d, metric)
        self.calls = []  # (rows, has exclusions)

    def search(self, x, k, raw=False, exclude=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self.calls.append((x.shape[0], exclude is not None))
        if exclude is None:
            return super().search(x, k, raw=raw)
        offs, labels = vfaiss.exclusion_csr(exclude, x.shape[0])
        valid = np.ones((x.shape[0], self.ntotal), dtype=bool)
        for q in range(x.shape[0]):
            seg = labels[offs[q]:offs[q + 1]]
            valid[q, seg[(seg >= 0) & (seg < self.ntotal)]] = False
        return flat.select_topk(flat.exact_scores(self._x, x, self.metric_type), k,
                                self.metric_type, valid=valid, rule="lex" if raw else "faiss")

    def mean_rows(self, profiles):
        return np.stack([mean_definition(self._x, np.asarray(l), w) for l, w in profiles])

    def search_profiles(self, profiles, k, *, exclude=None, exclude_profile=True):
        lists = [list(e) for e in exclude] if exclude is not None else [[] for _ in profiles]
        if exclude_profile:
            lists = [e + list(p[0]) for e, p in zip(lists, profiles)]
        return self.search(self.mean_rows(profiles), k, exclude=lists)


@pytest.fixture
def store(monkeypatch):
    monkeypatch.setattr(vfaiss, "IndexFlatL2", lambda d, **kw: ExclOracleIndex(d, flat.METRIC_L2))
    emb = SynthEmbeddings(48)
    texts = [f"book {i}" for i in range(120)]
    metas = [{"book_id": f"B{i:03d}"} for i in range(120)]
    # B005 is in the store twice: its first row stands for it, both are excluded
    texts.append("book 5, second edition")
    metas.append({"book_id": "B005"})
    return vlc.FAISS.from_texts(texts, emb, metadatas=metas)


PROFILES = [[("B005", 1.0), ("B017", 0.5), ("nope", 0.8)],
            [("nope", 1.0)],
            [("B100", 0.3)],
            [(f"B{i:03d}", 0.1 + 0.1 * (i % 5)) for i in range(0, 60, 3)]]
READ = [["B006", "B007"], ["B001"], [], [f"B{i:03d}" for i in range(60, 119)]]


def _ids(rows):
    return [[d.metadata["book_id"] for d, _ in r] for r in rows]


def test_store_recommend_for_profiles_on_oracle(store):
    res = store.recommend_for_profiles(PROFILES, k=6, exclude=READ)
    assert len(res) == 4 and res[1] == []
    for p, r, row in zip(PROFILES, READ, res):
        barred = {b for b, _ in p} | set(r)
        assert not barred.intersection(d.metadata["book_id"] for d, _ in row)
    assert [len(r) for r in res] == [6, 0, 6, 6]
    # the unknown profile took no part in the engine call
    assert store.index.calls[-1] == (3, True)
    # the query of profile 0 is the mean of the FIRST row of B005 and of B017
    want = mean_definition(store.index._x, np.asarray([5, 17]), [1.0, 0.5])
    D, I = store.index.search(want[None, :], 6, exclude=[[5, 120, 17, 6, 7]])
    assert _ids(res)[0] == [store.docstore.search(store.index_to_docstore_id[int(i)])
                            .metadata["book_id"] for i in I[0]]
    # all but min(k, allowed): profile 3 leaves 120 - 20 - 59 = 41 books; with more read, fewer
    few = store.recommend_for_profiles([PROFILES[3]], k=6,
                                       exclude=[[f"B{i:03d}" for i in range(120) if i % 3]])
    allowed = {f"B{i:03d}" for i in range(60, 120, 3)}
    assert len(few[0]) == 6 and set(_ids(few)[0]) <= allowed
    # the key -> labels table follows the store's generation
    first = store._key_labels("book_id")
    assert first["B005"] == [5, 120] and store._key_labels("book_id") is first
    store.delete([store.index_to_docstore_id[0]])
    assert store._key_labels("book_id")["B005"] == [4, 119]
    with pytest.raises(ValueError):
        store.recommend_for_profiles(PROFILES, exclude=READ[:2])


def test_store_exclude_ids_on_oracle(store):
    vec = store.index.reconstruct(10)
    first = store.similarity_search_with_score_by_vector(vec, k=3)
    drop = [first[0][0].id, first[1][0].id, "no-such-id"]
    again = store.similarity_search_with_score_by_vector(vec, k=3, exclude_ids=drop)
    assert len(again) == 3 and again[0][0].id == first[2][0].id
    assert not set(drop).intersection(d.id for d, _ in again)
    with pytest.raises(ValueError):
        store.similarity_search_with_score_by_vector(vec, k=3, exclude_ids=drop,
                                                     filter={"book_id": "B001"},
                                                     exact_filter=True)


def _until(cond, seconds=20.0):
    """Spins until cond() holds (another thread's next step); fails past the limit."""
    import time

    end = time.monotonic() + seconds
    while not cond():
        assert time.monotonic() < end, "the other thread did not get there"


def test_coalescer_groups_by_k_with_exclusions(store):
    """Requests of one k stack into one call; it carries exclusions as soon as
    one member has them, and the others' rows exclude nothing."""
    index = store.index
    xq = index._x[:6].copy()

    class Svc:
        pass

    svc = Svc()
    svc.store = store
    gate = threading.Event()
    entered = threading.Event()
    real = index.search

    def gated(x, k, exclude=None, raw=False):
        entered.set()
        gate.wait(10)
        return real(x, k, exclude=exclude, raw=raw)

    index.search = gated
    co = _Coalescer(svc, max_batch=64)
    out = {}

    def run(name, *a):
        out[name] = co.submit(*a)

    # the first request occupies the dispatcher; the others queue behind it
    first = threading.Thread(target=run, args=("first", xq[:1], 3))
    first.start()
    assert entered.wait(20)  # the dispatcher is inside the first call
    rest = [threading.Thread(target=run, args=("a", xq[1:3], 4, [[1], []])),
            threading.Thread(target=run, args=("b", xq[3:4], 4)),
            threading.Thread(target=run, args=("c", xq[4:6], 5))]
    for t in rest:
        t.start()
    _until(lambda: len(co._queue) == 3)
    index.calls.clear()
    gate.set()
    for t in [first] + rest:
        t.join(30)
    co.stop()
    assert sorted(index.calls) == [(1, False), (2, False), (3, True)]
    Da, Ia = out["a"]
    assert Ia.shape == (2, 4) and 1 not in Ia[0] and Ia[1, 0] == 2
    Db, Ib = out["b"]
    assert Ib.shape == (1, 4) and Ib[0, 0] == 3
    np.testing.assert_array_equal(out["c"][1], real(xq[4:6], 5)[1])
    with pytest.raises(ValueError):
        co.submit(xq[:2], 3, [[1]])


def test_service_recommend_and_search_with_exclusions(store):
    want = store.recommend_for_profiles(PROFILES, k=6, exclude=READ)
    got = {}
    with IndexService(store, authkey=KEY) as svc:
        barrier = threading.Barrier(2, timeout=30)

        def worker(i, sl):
            with RemoteFAISS(svc.address, KEY) as cli:
                barrier.wait()
                got[i] = cli.recommend_for_profiles(PROFILES[sl], k=6, exclude=READ[sl])

        ts = [threading.Thread(target=worker, args=(0, slice(0, 2))),
              threading.Thread(target=worker, args=(1, slice(2, 4)))]
        for t in ts:
            t.start()
        for t in ts:
            t.join(60)
        with RemoteFAISS(svc.address, KEY) as cli:
            xq = store.index._x[:3].copy()
            D, I = cli.index.search(xq, 4, exclude=[[0], [], [2, 3]])
            Dl, Il = store.index.search(xq, 4, exclude=[[0], [], [2, 3]])
            np.testing.assert_array_equal(I, Il)
            np.testing.assert_array_equal(D, Dl)
            assert 0 not in I[0] and I[1, 0] == 1 and not {2, 3} & set(I[2].tolist())
            assert cli.recommend_for_profiles([[("nope", 1.0)]]) == [[]]
            with pytest.raises(ValueError):
                cli.recommend_for_profiles(PROFILES, exclude=READ[:1])
        assert svc.stats["search_rows"] == 3 + 3
    both = got[0] + got[1]
    assert _ids(both) == _ids(want)
    for a, b in zip(both, want):
        assert [float(s) for _, s in a] == [float(s) for _, s in b]
