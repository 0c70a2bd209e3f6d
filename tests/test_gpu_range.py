"""GPU: range search (vs_range_search; faiss IndexFlat.range_search).

Oracle: the fp64 scores ``flat.exact_scores`` and the window ``flat.key_window``
an exactly computed, once-rounded key can sit in.  Every pair whose fp64 score
is farther than its window from the radius must be classified as that score
says (strict ``<`` for L2, ``>`` for inner product); the pairs inside the
window may go either way and are counted, so that a case cannot pass because
everything was "undecided".  The strictness cases use integer data, where every
sum is exact in fp32 and fp64 alike, and compare sets and D bit for bit.

Data as test_gpu_selector.py's ``_data``: default_rng(seed) standard normal,
rows first.  Shapes: 3000 = 23 * 128 + 56 rows (a partial last tile), d = 96 <
ld = 128 (column padding), 19 / 20 queries (faiss's sequential / BLAS L2 key),
130 and 300 queries (more than one query tile), 1536 columns (12 K stages), and
20000 rows (157 tiles: several splits)."""

import ctypes
import functools

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
N, DIM = 3000, 96


@pytest.fixture(scope="module")
def vf():
    from vsearch import _lib
    from vsearch import faiss as vfaiss

    assert _lib.device_count() >= 1
    return vfaiss


@functools.lru_cache(maxsize=None)
def _data(nq, n=N, d=DIM, seed=0):
    rng = np.random.default_rng(seed)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    xb.setflags(write=False)
    xq.setflags(write=False)
    return xb, xq


def _reference(xb, xq, metric):
    """(fp64 scores, windows) of every (query, row) pair."""
    s = flat.exact_scores(xb, xq, metric)
    qn2 = np.einsum("ij,ij->i", xq.astype(np.float64), xq.astype(np.float64))[:, None]
    xn2 = np.einsum("ij,ij->i", xb.astype(np.float64), xb.astype(np.float64))[None, :]
    return s, flat.key_window(metric, s, qn2, xn2, xb.shape[1])


@functools.lru_cache(maxsize=None)
def _reference_of(nq, n, d, metric, bf16=False):
    xb, xq = _data(nq, n, d)
    if bf16:
        xb, xq = flat.round_bf16(xb), flat.round_bf16(xq)
    return _reference(xb, xq, metric)


def _radius(s, metric, q):
    return np.float32(np.quantile(s, q if metric == L2 else 1.0 - q))


def _structure(lims, D, I, nq):
    assert lims.dtype == np.uint64 and D.dtype == np.float32 and I.dtype == np.int64
    assert lims.shape == (nq + 1,)
    assert lims[0] == 0 and lims[-1] == len(D) == len(I)
    li = lims.astype(np.int64)
    assert (np.diff(li) >= 0).all()
    for j in range(nq):
        seg = I[li[j]:li[j + 1]]
        assert (np.diff(seg) > 0).all(), f"query {j}: labels not strictly ascending"
    return li


def _hit_matrix(li, I, nq, n, base=0):
    got = np.zeros((nq, n), dtype=bool)
    q = np.repeat(np.arange(nq), np.diff(li))
    r = I - base
    assert ((r >= 0) & (r < n)).all(), "a label outside the index"
    got[q, r] = True
    return got, q, r


def _check(result, s, w, metric, radius, *, mask=None, base=0, timer=True):
    """The contract over one result; returns (hits, undecided)."""
    from vsearch import _lib

    lims, D, I = result
    nq, n = s.shape
    if timer:
        assert _lib.timer_kernel() == "gemm_range"
    li = _structure(lims, D, I, nq)
    got, q, r = _hit_matrix(li, I, nq, n, base)
    rad = float(radius)
    inside = s < rad - w if metric == L2 else s > rad + w
    outside = s > rad + w if metric == L2 else s < rad - w
    if mask is not None:
        inside &= mask[None, :]
        outside |= ~mask[None, :]
    undecided = int((~(inside | outside)).sum())
    print(f"hits {len(D)} undecided {undecided}")
    assert undecided <= 2, undecided
    assert got[inside].all(), "a row inside the radius is missing"
    assert not got[outside].any(), "a row outside the radius (or the selection) was returned"
    err = np.abs(D.astype(np.float64) - s[q, r])
    assert (err <= w[q, r]).all(), "D is not the exact key"
    return len(D), undecided


def _index(vf, xb, metric, dtype="f32"):
    index = vf.IndexFlat(xb.shape[1], metric, dtype=dtype)
    index.add(xb)
    return index


# ---- the contract over the shapes ---------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 19, 20, 37, 300])
def test_small_rows(vf, metric, nq):
    xb, xq = _data(nq)
    s, w = _reference_of(nq, N, DIM, metric)
    radius = _radius(s, metric, 0.01)
    index = _index(vf, xb, metric)
    hits, _ = _check(index.range_search(xq, radius), s, w, metric, radius)
    assert abs(hits - 0.01 * nq * N) <= 2


@pytest.mark.parametrize("metric", [L2, IP])
def test_long_rows(vf, metric):
    xb, xq = _data(37, 2000, 1536)
    s, w = _reference_of(37, 2000, 1536, metric)
    radius = _radius(s, metric, 0.01)
    hits, _ = _check(_index(vf, xb, metric).range_search(xq, radius), s, w, metric, radius)
    assert abs(hits - 740) <= 2


@pytest.mark.parametrize("metric", [L2, IP])
def test_many_tiles_two_query_tiles(vf, metric):
    xb, xq = _data(130, 20000, 1536)
    s, w = _reference_of(130, 20000, 1536, metric)
    radius = _radius(s, metric, 0.002)
    hits, _ = _check(_index(vf, xb, metric).range_search(xq, radius), s, w, metric, radius)
    assert abs(hits - 5200) <= 2


@pytest.mark.parametrize("metric", [L2, IP])
def test_bf16_index(vf, metric):
    """Rows and queries rounded to bf16; the exact key is over the stored values."""
    xb, xq = _data(37)
    s, w = _reference_of(37, N, DIM, metric, True)
    radius = _radius(s, metric, 0.01)
    _check(_index(vf, xb, metric, "bf16").range_search(xq, radius), s, w, metric, radius)


def test_bf16_tombstones(vf):
    """A bf16 index keeps removed rows in place, NaN-filled: they never match,
    and the labels are positions among the live rows.  The removed rows are
    copies of queries, so each of them would be a hit."""
    xb, xq = _data(37)
    xb = xb.copy()
    ids = np.random.default_rng(5).choice(N, 50, replace=False)
    xb[ids] = xq[np.arange(50) % 37]
    index = _index(vf, xb, L2, "bf16")
    assert index.remove_ids(ids) == 50
    live = np.delete(xb, ids, axis=0)
    s, w = _reference(flat.round_bf16(live), flat.round_bf16(xq), L2)
    radius = _radius(s, L2, 0.01)
    _check(index.range_search(xq, radius), s, w, L2, radius)


# ---- strictness, in exact arithmetic --------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [5, 37])
def test_strict_comparison_exact(vf, metric, nq):
    """Integers in [-3, 3]: every sum is an exact integer in fp32 and fp64, in
    any order, so the result is the fp64 one with no window.  radius = a score
    that occurs: the pairs at it are candidates the verification rejects."""
    rng = np.random.default_rng(11)
    xb = rng.integers(-3, 4, (N, DIM)).astype(np.float32)
    xq = rng.integers(-3, 4, (nq, DIM)).astype(np.float32)
    s = flat.exact_scores(xb, xq, metric)
    assert (s == np.rint(s)).all()
    t = float(np.rint(np.quantile(s, 0.01 if metric == L2 else 0.99)))
    at = s == t
    assert at.sum() >= 3, "no pair at the radius"
    index = _index(vf, xb, metric)
    strict = s < t if metric == L2 else s > t
    past = np.nextafter(np.float32(t), np.float32(np.inf if metric == L2 else -np.inf))
    for radius, want in ((np.float32(t), strict), (past, strict | at)):
        lims, D, I = index.range_search(xq, radius)
        li = _structure(lims, D, I, nq)
        got, q, r = _hit_matrix(li, I, nq, N)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(D, s[q, r].astype(np.float32))


# ---- extremes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_extreme_radii(vf, metric):
    xb, xq = _data(37)
    index = _index(vf, xb, metric)
    every, none = (3e38, -1.0) if metric == L2 else (-3e38, 3e38)
    lims, D, I = index.range_search(xq, every)
    _structure(lims, D, I, 37)
    np.testing.assert_array_equal(lims, (np.arange(38) * N).astype(np.uint64))
    np.testing.assert_array_equal(I.reshape(37, N), np.tile(np.arange(N), (37, 1)))
    s, w = _reference_of(37, N, DIM, metric)
    assert (np.abs(D.reshape(37, N).astype(np.float64) - s) <= w).all()
    for radius in (none, float("nan")):
        lims, D, I = index.range_search(xq, radius)
        _structure(lims, D, I, 37)
        assert not lims.any() and len(D) == 0


@pytest.mark.parametrize("metric", [L2, IP])
def test_empty_index_and_empty_batch(vf, metric):
    xb, xq = _data(37)
    empty = vf.IndexFlat(DIM, metric)
    lims, D, I = empty.range_search(xq, 1.0)
    _structure(lims, D, I, 37)
    assert not lims.any()
    index = _index(vf, xb, metric)
    lims, D, I = index.range_search(xq[:0], 1.0)
    _structure(lims, D, I, 0)
    assert lims.tolist() == [0]


# ---- selectors ----------------------------------------------------------------------------------
def _selection(vf, name):
    """(selector tree, bool mask over the rows)."""
    rng = np.random.default_rng(1)
    if name == "first_half":
        mask = np.zeros(N, dtype=bool)
        mask[: N // 2] = True
        return vf.IDSelectorRange(0, N // 2), mask
    if name == "5pct":
        mask = rng.random(N) < 0.05
        return vf.IDSelectorBitmap(N, np.packbits(mask, bitorder="little")), mask
    ids = rng.choice(N, 200, replace=False)
    mask = np.ones(N, dtype=bool)
    mask[ids] = False
    return vf.IDSelectorNot(vf.IDSelectorBatch(ids)), mask


def _plant(xb, xq, mask):
    """Copies of the queries into unselected rows (3 per query where they fit)."""
    xb = xb.copy()
    out = np.nonzero(~mask)[0]
    for j, r in enumerate(out[: 3 * xq.shape[0]]):
        xb[r] = xq[j % xq.shape[0]]
    return xb


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("name", ["first_half", "5pct", "not_batch_200"])
def test_selector(vf, metric, name):
    xb0, xq = _data(37)
    tree, mask = _selection(vf, name)
    xb = _plant(xb0, xq, mask)  # the nearest rows of every query are NOT selected
    s, w = _reference(xb, xq, metric)
    radius = _radius(s, metric, 0.01)
    index = _index(vf, xb, metric)
    res = index.range_search(xq, radius, params=vf.SearchParameters(sel=tree))
    hits, _ = _check(res, s, w, metric, radius, mask=mask)
    assert hits > 0
    # a Selector handle, reused across two calls
    sel = index.selector(tree)
    assert sel.count == int(mask.sum())
    params = vf.SearchParameters(sel=sel)
    for q in (0.01, 0.03):
        radius = _radius(s, metric, q)
        _check(index.range_search(xq, radius, params=params), s, w, metric, radius, mask=mask)
    index.add(xb[:1])
    with pytest.raises(RuntimeError, match="stale selector"):
        index.range_search(xq, radius, params=params)


# ---- labels, outputs, determinism -----------------------------------------------------------------
def test_id_base_offsets_labels(vf):
    xb, xq = _data(37)
    s, w = _reference_of(37, N, DIM, IP)
    radius = _radius(s, IP, 0.01)
    index = _index(vf, xb, IP)
    index.set_id_base(10**10)
    res = index.range_search(xq, radius)
    assert res[2].min() >= 10**10
    _check(res, s, w, IP, radius, base=10**10)


def test_device_outputs_match_host_copy(vf):
    import torch

    from vsearch import _lib

    xb, xq = _data(37)
    s, _ = _reference_of(37, N, DIM, L2)
    radius = _radius(s, L2, 0.01)
    index = _index(vf, xb, L2)
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.vs_range_search(index._h, None, xq.ctypes.data, 37, ctypes.c_float(radius), 0,
                                   None, ctypes.byref(h)), "vs_range_search")
    try:
        nq, total = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(lib.vs_range_size(h, ctypes.byref(nq), ctypes.byref(total)), "vs_range_size")
        assert nq.value == 37 and total.value > 0
        lims = np.empty(38, dtype=np.int64)
        D = np.empty(total.value, dtype=np.float32)
        I = np.empty(total.value, dtype=np.int64)
        _lib.check(lib.vs_range_copy(h, lims.ctypes.data, D.ctypes.data, I.ctypes.data, 0, None),
                   "vs_range_copy")
        dl = torch.empty(38, dtype=torch.int64, device="cuda")
        dD = torch.empty(total.value, dtype=torch.float32, device="cuda")
        dI = torch.empty(total.value, dtype=torch.int64, device="cuda")
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            _lib.check(lib.vs_range_copy(h, ctypes.c_void_p(dl.data_ptr()),
                                         ctypes.c_void_p(dD.data_ptr()),
                                         ctypes.c_void_p(dI.data_ptr()), _lib.OUT_DEVICE,
                                         ctypes.c_void_p(st.cuda_stream)), "vs_range_copy")
        st.synchronize()
    finally:
        lib.vs_range_destroy(h)
    np.testing.assert_array_equal(dl.cpu().numpy(), lims)
    np.testing.assert_array_equal(dD.cpu().numpy(), D)
    np.testing.assert_array_equal(dI.cpu().numpy(), I)
    assert lims[-1] == total.value


@pytest.mark.parametrize("metric", [L2, IP])
def test_two_calls_are_identical(vf, metric):
    xb, xq = _data(300)
    s, _ = _reference_of(300, N, DIM, metric)
    radius = _radius(s, metric, 0.01)
    index = _index(vf, xb, metric)
    a = index.range_search(xq, radius)
    b = index.range_search(xq, radius)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    # the answer does not depend on the batch a query arrives in (37 and 300
    # queries are both past faiss's switch of the L2 key)
    c = index.range_search(xq[:37], radius)
    k = int(a[0][37])
    np.testing.assert_array_equal(c[0], a[0][:38])
    np.testing.assert_array_equal(c[1], a[1][:k])
    np.testing.assert_array_equal(c[2], a[2][:k])


# ---- the store ------------------------------------------------------------------------------------
def test_store_within_score(golden, golden_vectors):
    """FAISS.similarity_search_within_score over the golden catalogue: exactly
    the documents whose full-length search score passes the threshold, best
    first; the same with a metadata filter."""
    from vsearch import langchain as vlc
    from vsearch.synth import SynthEmbeddings

    inputs, _ = golden
    store = vlc.FAISS.from_texts(inputs["book_texts"], SynthEmbeddings(),
                                 metadatas=inputs["book_metadata"])
    ntotal = store.index.ntotal
    genres = [m["genre"] for m in inputs["book_metadata"]]
    genre = max(sorted(set(genres)), key=genres.count)  # the largest one: 25 books
    for kw in inputs["keywords"][:4]:
        full = store.similarity_search_with_score(kw, k=ntotal)
        assert len(full) == ntotal
        for flt in (None, {"genre": genre}):
            passing = [(d, s) for d, s in full
                       if flt is None or d.metadata["genre"] == genre]
            assert len(passing) > 12
            sc = np.array([s for _, s in passing], dtype=np.float64)
            # a threshold between two scores that are clearly apart (the search's
            # scores are the fp32 engine's, the range search's the exact keys)
            hi = min(60, len(sc))
            j = 5 + int(np.argmax(np.diff(sc[5:hi])))
            assert sc[j + 1] - sc[j] > 1e-4 * max(1.0, sc[j + 1])
            t = float(0.5 * (sc[j] + sc[j + 1]))
            want = {d.metadata["book_id"]: float(s) for d, s in passing if s < t}
            got = store.similarity_search_within_score(kw, t, filter=flt)
            assert len(want) == j + 1
            assert sorted(d.metadata["book_id"] for d, _ in got) == sorted(want)
            gs = np.array([s for _, s in got], dtype=np.float64)
            assert (np.diff(gs) >= 0).all(), "not best first"
            ws = np.array([want[d.metadata["book_id"]] for d, _ in got])
            np.testing.assert_allclose(gs, ws, rtol=1e-5, atol=1e-5)
