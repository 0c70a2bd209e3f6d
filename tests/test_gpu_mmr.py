"""GPU: MMR searches (vs_mmr_select, vs_search_mmr) against tests/mmr_oracle.py.

Checking rule: the device's picks are replayed step by step; at each step the
oracle's scores for the device's own prefix are recomputed in fp64 and the
device's pick must score within slack(d) = (4d + 16) * 2^-53 of the oracle's
maximum (mmr_oracle.replay).  Every test also asserts that the oracle's own gap
between its best and second-best score exceeds 2 * slack(d) at every step of
its inputs; under that condition the replay must equal the oracle's sequence
outright, so zero differing steps are allowed.  (Equality with the oracle's
sequence implies the replay's rule; the literal replay runs on the short
cases and on any mismatch, for its message.)

Rows are clustered (4 centres + 0.3 * noise), so that the redundancy term
decides picks."""

import ctypes
import functools

import numpy as np
import pytest

import mmr_oracle
from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
NROWS = 2000
LAMBDAS = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def vf():
    from vsearch import _lib
    from vsearch import faiss as vfaiss

    assert _lib.device_count() >= 1
    return vfaiss


@functools.lru_cache(maxsize=None)
def _rows(d, n=NROWS, seed=0):
    """(xb, xq): n clustered rows and 300 queries near the same centres."""
    rng = np.random.default_rng(1000 * d + seed)
    centres = rng.standard_normal((4, d))
    xb = (centres[rng.integers(0, 4, n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    xq = (centres[rng.integers(0, 4, 300)] + 0.5 * rng.standard_normal((300, d))).astype(np.float32)
    xb.setflags(write=False)
    xq.setflags(write=False)
    return xb, xq


_INDEXES = {}


def _index(vf, d, metric=L2, dtype="f32"):
    """One index per (d, metric, dtype) for the module; never mutated."""
    key = (d, metric, dtype)
    if key not in _INDEXES:
        index = vf.IndexFlat(d, metric, dtype=dtype)
        index.add(_rows(d)[0])
        _INDEXES[key] = index
    return _INDEXES[key]


def _stored(d, dtype):
    xb = _rows(d)[0]
    return flat.round_bf16(xb) if dtype == "bf16" else xb


def _check(pos, stored, x, cand, k, lam, *, base=0, problems=None):
    """The device's pos (n, k) for queries x and candidate labels cand against
    the oracle over `stored` (label l = row l - base).  problems: a dict that
    caches the oracle's (Problem, picks, gaps) per (query, lambda)."""
    d = stored.shape[1]
    n, F = cand.shape
    assert pos.shape == (n, k) and pos.dtype == np.int32
    for i in range(n):
        key = (i, lam)
        if problems is None or key not in problems:
            valid = cand[i] != -1
            pr = mmr_oracle.Problem(x[i], stored[np.where(valid, cand[i] - base, 0)], valid)
            picks, gaps = pr.select(F, lam)  # every k's picks are a prefix of these
            if problems is not None:
                problems[key] = (pr, picks, gaps)
        else:
            pr, picks, gaps = problems[key]
        steps = min(k, len(picks))
        # the precondition: the oracle's own decisions are far outside the slack
        assert min(gaps[:steps], default=np.inf) > 2 * mmr_oracle.slack(d), (i, lam, min(gaps))
        want = picks[:steps] + [-1] * (k - steps)
        got = pos[i].tolist()
        if got != want or F * k <= 65 * 4:
            assert mmr_oracle.replay(pr, got, k, lam, d) == [], (i, lam)
        assert got == want, (i, lam, got[:8], want[:8])


def _cands(rng, n, F, nrows=NROWS):
    return np.stack([rng.choice(nrows, F, replace=False) for _ in range(n)]).astype(np.int64)


# ---- 1. mmr_select against the oracle -----------------------------------------------------
CASES = [(d, F) for d in (33, 100, 1536) for F in (1, 2, 20, 64, 65, 257)] + [(100, 1024)]


@pytest.mark.parametrize("d,F", CASES, ids=[f"d{d}-F{F}" for d, F in CASES])
def test_mmr_select_against_oracle(vf, d, F):
    index = _index(vf, d)
    stored = _stored(d, "f32")
    xq = _rows(d)[1]
    rng = np.random.default_rng(d * 7 + F)
    for n in (1, 37):
        cand = _cands(rng, n, F)
        x = xq[:n]
        problems = {}
        for k in sorted({1, 4, F, F + 3}):
            for lam in LAMBDAS:
                pos = index.mmr_select(x, cand, k, lam)
                _check(pos, stored, x, cand, k, lam, problems=problems)
                if k > F:
                    assert (pos[:, F:] == -1).all()
        # lambda = 1 is the candidates sorted by their cosine to the query
        pos = index.mmr_select(x, cand, F, 1.0)
        for i in range(n):
            s = mmr_oracle.cosines(x[i:i + 1], stored[cand[i]])[0]
            assert pos[i].tolist() == np.argsort(-s, kind="stable").tolist()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [33, 100])
def test_mmr_select_metric_and_dtype(vf, d, dtype, metric):
    """The re-rank reads the stored values (bf16: widened, the query not
    rounded) and does not depend on the index's metric."""
    index = _index(vf, d, metric, dtype)
    stored = _stored(d, dtype)
    xq = _rows(d)[1]
    rng = np.random.default_rng(d + 5)
    cand = _cands(rng, 37, 65)
    for k in (4, 68):
        for lam in LAMBDAS:
            _check(index.mmr_select(xq[:37], cand, k, lam), stored, xq[:37], cand, k, lam)


# ---- 2. empty slots -------------------------------------------------------------------------
def test_empty_slots(vf):
    d = 100
    index = _index(vf, d)
    stored = _stored(d, "f32")
    xq = _rows(d)[1][:6]
    rng = np.random.default_rng(2)
    cand = _cands(rng, 6, 70)
    cand[0, rng.choice(70, 30, replace=False)] = -1  # scattered
    cand[1, :] = -1                                   # no candidate at all
    cand[2, 0] = -1                                   # the first slot
    cand[3, 1:] = -1                                  # one candidate, at position 0
    cand[4, :69] = -1                                 # one candidate, at the last position
    for k in (4, 70, 75):
        for lam in LAMBDAS:
            pos = index.mmr_select(xq, cand, k, lam)
            _check(pos, stored, xq, cand, k, lam)
            assert (pos[1] == -1).all()
            assert pos[3].tolist() == [0] + [-1] * (k - 1)
            assert pos[4].tolist() == [69] + [-1] * (k - 1)
            for i in range(6):  # positions refer to the original list; no empty slot is picked
                got = pos[i][pos[i] >= 0]
                assert (cand[i][got] != -1).all() and len(set(got.tolist())) == got.size
                assert got.size == min(k, int((cand[i] != -1).sum()))


@pytest.mark.parametrize("metric", [L2, IP])
def test_fetch_k_past_the_index_pads_with_empty_slots(vf, metric):
    d, n = 33, 12
    xb, xq = _rows(d)
    index = vf.IndexFlat(d, metric)
    index.add(xb[:n])
    D, I = index.search_mmr(xq[:5], 6, fetch_k=20, lambda_mult=0.5)
    Dc, Ic = index.search(xq[:5], 20)
    assert (Ic[:, n:] == -1).all()
    pos = index.mmr_select(xq[:5], Ic, 6, 0.5)
    _check(pos, xb[:n], xq[:5], Ic, 6, 0.5)
    Dw, Iw = vf.gather_picks(Dc, Ic, pos, metric)
    np.testing.assert_array_equal(I, Iw)
    np.testing.assert_array_equal(D, Dw)
    D, I = index.search_mmr(xq[:5], 15, fetch_k=20, lambda_mult=0.5)
    assert (I[:, :n] >= 0).all() and (I[:, n:] == -1).all()
    assert (D[:, n:] == flat.neutral(metric)).all()
    assert all(sorted(I[q, :n].tolist()) == list(range(n)) for q in range(5))
    empty = vf.IndexFlat(d, metric)
    D, I = empty.search_mmr(xq[:3], 4, fetch_k=8)
    assert (I == -1).all() and (D == flat.neutral(metric)).all()


# ---- 3. duplicates and ties -------------------------------------------------------------------
def test_duplicates_ties_and_zero_rows(vf):
    d = 100
    xb, xq = _rows(d)
    rows = xb[:60].copy()
    rows[41] = rows[7]   # two labels of bit-identical rows
    rows[50] = 0.0       # a zero-norm row
    index = vf.IndexFlat(d, L2)
    index.add(rows)
    q = (rows[7] + 0.4 * rows[20] + 0.1 * xq[0]).astype(np.float32)[None, :]
    #            twin A  twin B (same row)  the same label twice     a zero row
    cand = np.asarray([[3, 7, 12, 41, 20, 12, 50, 33, 9]], dtype=np.int64)
    pr = mmr_oracle.Problem(q[0], rows[cand[0]])
    assert abs(pr.G[1, 3] - 1.0) < 1e-15 and abs(pr.G[2, 5] - 1.0) < 1e-15
    assert not pr.G[6].any() and pr.s[6] == 0.0
    for lam in LAMBDAS:
        pos = index.mmr_select(q, cand, 9, lam)[0].tolist()
        assert sorted(pos) == list(range(9))
        assert mmr_oracle.replay(pr, pos, 9, lam, d) == [], lam  # where the oracle puts them
        # of two equal candidates the lower position is picked first
        assert pos.index(1) < pos.index(3) and pos.index(2) < pos.index(5)
    pos = index.mmr_select(q, cand, 9, 0.5)[0].tolist()
    assert pos[0] == 1  # the row nearest to q; its twin then scores 0.5 * s - 0.5 * 1
    sc, _ = pr.scores([1], 0.5)
    assert abs(sc[3] - (0.5 * pr.s[3] - 0.5 * 1.0)) < 1e-15 and sc[3] < 0.0
    assert pos.index(3) > 1
    # twins and repeats get bit-identical scores: the result does not change
    # when they swap places in the list
    swapped = cand.copy()
    swapped[0, [1, 3]] = swapped[0, [3, 1]]
    assert index.mmr_select(q, swapped, 9, 0.5)[0].tolist() == pos
    # a zero query: every cosine to it is 0, lambda * 0 - (1 - lambda) * max cos
    # decides from the second pick on; nothing is NaN, every candidate is picked
    zq = np.zeros((1, d), dtype=np.float32)
    zpr = mmr_oracle.Problem(zq[0], rows[cand[0]])
    for lam in LAMBDAS:
        pos = index.mmr_select(zq, cand, 9, lam)[0].tolist()
        assert sorted(pos) == list(range(9)) and pos[0] == 0  # all s equal: list order
        assert mmr_oracle.replay(zpr, pos, 9, lam, d) == [], lam
    D, I = index.search_mmr(zq, 5, fetch_k=9)
    assert (I >= 0).all() and np.isfinite(D).all()


# ---- 4. labels ------------------------------------------------------------------------------------
def test_id_base(vf):
    d = 33
    xb, xq = _rows(d)
    index = vf.IndexFlat(d, L2)
    index.add(xb[:500])
    index.set_id_base(1000)
    rng = np.random.default_rng(4)
    cand = _cands(rng, 5, 20, 500) + 1000
    cand[2, 3] = -1
    _check(index.mmr_select(xq[:5], cand, 6, 0.5), xb[:500], xq[:5], cand, 6, 0.5, base=1000)
    D, I = index.search_mmr(xq[:5], 4, fetch_k=10)
    assert ((I >= 1000) & (I < 1500)).all()
    from vsearch import _lib
    for bad in (999, 1500, 5, -2):
        c = cand.copy()
        c[4, 19] = bad
        with pytest.raises(_lib.VSearchError) as ei:
            index.mmr_select(xq[:5], c, 6, 0.5)
        assert ei.value.code == _lib.E_INVALID and "key out of range" in str(ei.value)


def test_bf16_tombstones_and_bad_labels(vf):
    import torch

    from vsearch import _lib

    d = 100
    xb, xq = _rows(d)
    index = vf.IndexFlat(d, IP, dtype="bf16")
    index.add(xb)
    gone = np.asarray([0, 7, 8, 300, 1500, NROWS - 1])
    assert index.remove_ids(gone) == gone.size  # below the pack threshold: tombstones
    left = flat.round_bf16(np.delete(xb, gone, axis=0))
    live = NROWS - gone.size
    rng = np.random.default_rng(6)
    cand = _cands(rng, 9, 64, live)
    cand[0, :4] = [0, 6, 7, live - 1]  # labels next to every tombstone
    pos = index.mmr_select(xq[:9], cand, 10, 0.5)
    _check(pos, left, xq[:9], cand, 10, 0.5)
    # the picks reconstruct to the right rows
    for i in (0, 5):
        for p in pos[i][:3]:
            np.testing.assert_array_equal(index.reconstruct(int(cand[i, p])), left[cand[i, p]])
    # search_mmr maps the search's labels back to rows through the tombstones
    D, I = index.search_mmr(xq[:9], 5, fetch_k=30)
    Dc, Ic = index.search(xq[:9], 30)
    Dw, Iw = vf.gather_picks(Dc, Ic, index.mmr_select(xq[:9], Ic, 5, 0.5), IP)
    np.testing.assert_array_equal(I, Iw)
    np.testing.assert_array_equal(D, Dw)
    # a label past ntotal (the live rows): RuntimeError, as faiss reconstruct
    c = cand.copy()
    c[3, 10] = live
    with pytest.raises(RuntimeError):
        index.mmr_select(xq[:9], c, 10, 0.5)
    # the same through device buffers, where the check is made on the device
    xd = torch.from_numpy(xq[:9].copy()).cuda()
    pd = torch.full((9, 10), -7, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    for labels, rc in ((cand, 0), (c, _lib.E_INVALID)):
        cd = torch.from_numpy(labels).cuda()
        got = lib.vs_mmr_select(index._h, ctypes.c_void_p(xd.data_ptr()), 9,
                                ctypes.c_void_p(cd.data_ptr()), 64, 10, 0.5,
                                ctypes.c_void_p(pd.data_ptr()),
                                _lib.IN_DEVICE | _lib.OUT_DEVICE, None)
        assert got == rc
        torch.cuda.synchronize()
        if rc == 0:
            np.testing.assert_array_equal(pd.cpu().numpy(), pos)
        else:
            assert "key out of range" in _lib.last_error()


# ---- 5. search_mmr equals the composition ---------------------------------------------------------
def _composition(vf, index, x, k, fetch_k, lam, **kw):
    Dc, Ic = index.search(x, fetch_k, **kw)
    return vf.gather_picks(Dc, Ic, index.mmr_select(x, Ic, k, lam), index.metric_type)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", [L2, IP])
def test_search_mmr_equals_the_composition(vf, metric, dtype, monkeypatch):
    import torch

    d = 100
    index = _index(vf, d, metric, dtype)
    stored = _stored(d, dtype)
    xq = _rows(d)[1]
    for n, k, fetch_k, lam in ((300, 10, 64, 0.5), (1, 4, 20, 0.5), (37, 25, 20, 0.0),
                               (19, 6, 257, 0.7)):
        x = xq[:n]
        D, I = index.search_mmr(x, k, fetch_k, lam)
        Dw, Iw = _composition(vf, index, x, k, fetch_k, lam)
        np.testing.assert_array_equal(I, Iw)
        np.testing.assert_array_equal(D, Dw)
        assert (I[:, :min(k, fetch_k)] >= 0).all()
    # the picks are the oracle's over the search's own candidate order
    x = xq[:37]
    Dc, Ic = index.search(x, 64)
    _check(index.mmr_select(x, Ic, 10, 0.5), stored, x, Ic, 10, 0.5)
    # n = 300 in chunks of 128 queries: the same bytes as in one chunk
    x = xq[:300]
    D, I = index.search_mmr(x, 10, 64, 0.5)
    monkeypatch.setenv("VS_MMR_CHUNK", "128")
    D2, I2 = index.search_mmr(x, 10, 64, 0.5)
    pos2 = index.mmr_select(x, index.search(x, 64)[1], 10, 0.5)
    monkeypatch.delenv("VS_MMR_CHUNK")
    np.testing.assert_array_equal(I2, I)
    np.testing.assert_array_equal(D2, D)
    np.testing.assert_array_equal(pos2, index.mmr_select(x, index.search(x, 64)[1], 10, 0.5))
    # exclusion lists: the candidates are search(exclude=...)'s
    rng = np.random.default_rng(8)
    near = index.search(x, 30)[1]
    lists = [near[q, rng.choice(30, q % 7, replace=False)] for q in range(300)]
    D3, I3 = index.search_mmr(x, 10, 64, 0.5, exclude=lists)
    Dw, Iw = _composition(vf, index, x, 10, 64, 0.5, exclude=lists)
    np.testing.assert_array_equal(I3, Iw)
    np.testing.assert_array_equal(D3, Dw)
    assert not any(np.isin(I3[q], lists[q]).any() for q in range(300))
    # device buffers through the VS_*_DEVICE flags
    xd = torch.from_numpy(x.copy()).cuda()
    Dd = torch.empty((300, 10), dtype=torch.float32, device="cuda")
    Id = torch.empty((300, 10), dtype=torch.int64, device="cuda")
    index.search_mmr_device(xd.data_ptr(), 300, 10, 64, 0.5, Dd.data_ptr(), Id.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Id.cpu().numpy(), I)
    np.testing.assert_array_equal(Dd.cpu().numpy(), D)


@pytest.mark.parametrize("metric", [L2, IP])
def test_search_mmr_with_a_selector(vf, metric):
    d = 100
    index = _index(vf, d, metric)
    x = _rows(d)[1][:40]
    for sel in (vf.IDSelectorRange(100, 900), vf.IDSelectorBatch(np.arange(0, NROWS, 50)),
                vf.IDSelectorNot(vf.IDSelectorBatch([3, 4]))):
        params = vf.SearchParameters(sel=sel)
        D, I = index.search_mmr(x, 8, fetch_k=32, lambda_mult=0.5, params=params)
        Dw, Iw = _composition(vf, index, x, 8, 32, 0.5, params=params)
        np.testing.assert_array_equal(I, Iw)
        np.testing.assert_array_equal(D, Dw)
        got = I[I >= 0]
        assert vf._members(sel, got).all() and (I[:, 0] >= 0).all()
    with pytest.raises(ValueError):
        index.search_mmr(x, 8, params=vf.SearchParameters(sel=vf.IDSelectorAll()),
                         exclude=[[] for _ in range(40)])


def test_search_mmr_ip_tie_order(vf):
    """Inner product: the candidate order is faiss's tie order, not raw order."""
    d = 33
    xb, xq = _rows(d)
    rows = xb[:400].copy()
    twins = np.asarray([3, 40, 41, 200, 399])
    rows[twins] = 3.0 * xq[0]
    index = vf.IndexFlat(d, IP)
    index.add(rows)
    x = xq[:2]
    Dc, Ic = index.search(x, 12)
    assert set(twins.tolist()) <= set(Ic[0].tolist())
    assert Ic[0, :5].tolist() != sorted(Ic[0, :5].tolist())  # faiss's order of equal scores
    D, I = index.search_mmr(x, 12, fetch_k=12, lambda_mult=1.0)
    # lambda = 1 and equal cosines: list order, which is the search's order
    assert I[0, :5].tolist() == Ic[0, :5].tolist()
    Dw, Iw = _composition(vf, index, x, 12, 12, 1.0)
    np.testing.assert_array_equal(I, Iw)
    np.testing.assert_array_equal(D, Dw)


# ---- 6. determinism ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_determinism(vf, dtype):
    d = 1536
    index = _index(vf, d, L2, dtype)
    x = _rows(d)[1]
    D, I = index.search_mmr(x, 10, 64, 0.5)
    D2, I2 = index.search_mmr(x, 10, 64, 0.5)
    assert D.tobytes() == D2.tobytes() and I.tobytes() == I2.tobytes()
    rng = np.random.default_rng(9)
    cand = _cands(rng, 300, 64)
    pos = index.mmr_select(x, cand, 10, 0.5)
    assert pos.tobytes() == index.mmr_select(x, cand, 10, 0.5).tobytes()
    # a query's result at batch 1 and inside the batch of 300, and at another
    # place in the batch
    for q in (0, 123, 299):
        assert index.mmr_select(x[q:q + 1], cand[q:q + 1], 10, 0.5).tolist() == [pos[q].tolist()]
    order = rng.permutation(300)
    np.testing.assert_array_equal(index.mmr_select(x[order], cand[order], 10, 0.5), pos[order])
    # (the search's own L2 formula follows the call's size, so batch 1 is
    # compared on an inner-product index)
    ip = _index(vf, d, IP, dtype)
    D, I = ip.search_mmr(x, 10, 64, 0.5)
    for q in (0, 123, 299):
        D1, I1 = ip.search_mmr(x[q:q + 1], 10, 64, 0.5)
        assert I1.tolist() == [I[q].tolist()]


# ---- 7. the store -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def catalog(golden):
    """The golden catalogue with book 7 re-ingested: a second, identical row
    appended, as the reference's add_texts does."""
    from vsearch import langchain as vlc
    from vsearch.synth import SynthEmbeddings

    inputs, _ = golden
    texts = list(inputs["book_texts"]) + [inputs["book_texts"][7]]
    metas = list(inputs["book_metadata"]) + [dict(inputs["book_metadata"][7])]
    store = vlc.FAISS.from_texts(texts, SynthEmbeddings(), metadatas=metas)
    return store, store.index.reconstruct_n(0, len(texts))


def _mix(X, *labels):
    v = np.sum([X[l] * w for l, w in zip(labels, (1.0, 0.6, 0.4))], axis=0)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _book_ids(docs):
    return [d.metadata["book_id"] for d in docs]


def _oracle_docs(store, X, q, D, I, k, lam):
    """[(book_id, score)] of the oracle's picks over the candidates (D, I) of q."""
    valid = I != -1
    pr = mmr_oracle.Problem(q, X[np.where(valid, I, 0)], valid)
    picks, gaps = pr.select(k, lam)
    assert min(gaps) > 2 * mmr_oracle.slack(X.shape[1])
    return [(store.docstore.search(store.index_to_docstore_id[int(I[p])]).metadata["book_id"],
             D[p]) for p in picks]


def test_store_mmr_methods(catalog):
    store, X = catalog
    nb = X.shape[0]
    q = _mix(X, 11, 3, min(40, nb - 2))
    for k, fetch_k, lam in ((4, 20, 0.5), (6, 30, 0.2), (5, 12, 1.0)):
        D, I = store.index.search(q[None, :], fetch_k)
        want = _oracle_docs(store, X, q, D[0], I[0], k, lam)
        got = store.max_marginal_relevance_search_with_score_by_vector(
            q, k=k, fetch_k=fetch_k, lambda_mult=lam)
        assert [(d.metadata["book_id"], s) for d, s in got] == want  # scores: the faiss D
        assert _book_ids(store.max_marginal_relevance_search_by_vector(
            q, k=k, fetch_k=fetch_k, lambda_mult=lam)) == [b for b, _ in want]
    text = "a story about dragons and friendship"
    vec = np.asarray(store._embed_query(text), dtype=np.float32)
    assert store.max_marginal_relevance_search(text, k=3) == \
        store.max_marginal_relevance_search_by_vector(vec, k=3)
    # filter=: LangChain's search of fetch_k * 2, host filter, re-rank of the rest
    ids = [m["book_id"] for m in (store.docstore.search(store.index_to_docstore_id[i]).metadata
                                  for i in range(nb))]
    allowed = sorted(set(ids[::2]))
    flt = {"book_id": {"$in": allowed}}
    D, I = store.index.search(q[None, :], 24)
    keep = [j for j, i in enumerate(I[0]) if i != -1 and ids[int(i)] in allowed]
    want = _oracle_docs(store, X, q, D[0][keep], I[0][keep], 3, 0.5)
    got = store.max_marginal_relevance_search_with_score_by_vector(q, k=3, fetch_k=12, filter=flt)
    assert [(d.metadata["book_id"], s) for d, s in got] == want
    # exact_filter=True: exactly min(fetch_k, matches) candidates, by a selector
    members = np.asarray([i for i in range(nb) if ids[i] in allowed])
    dist = flat.exact_scores(X[members], q[None, :], L2)[0]
    order = members[np.argsort(dist, kind="stable")][:12]
    got = store.max_marginal_relevance_search_with_score_by_vector(q, k=3, fetch_k=12, filter=flt,
                                                                   exact_filter=True)
    Dsel, Isel = store.index.search(q[None, :], 12, params=store_sel(store, flt))
    assert Isel[0].tolist() == order.tolist()
    assert [(d.metadata["book_id"], s) for d, s in got] == _oracle_docs(
        store, X, q, Dsel[0], Isel[0], 3, 0.5)
    two = {"book_id": {"$in": [ids[1], ids[4]]}}
    got = store.max_marginal_relevance_search_by_vector(q, k=9, fetch_k=20, filter=two,
                                                        exact_filter=True)
    assert sorted(_book_ids(got)) == sorted([ids[1], ids[4]])


def store_sel(store, flt):
    from vsearch import faiss as vfaiss

    return vfaiss.SearchParameters(sel=store._filter_selector(flt))


def test_store_mmr_drops_the_reingested_copy(catalog):
    store, X = catalog
    nb = X.shape[0]
    assert np.array_equal(X[7], X[nb - 1])
    q = _mix(X, 7, 3, 20)
    dup = store.docstore.search(store.index_to_docstore_id[7]).metadata["book_id"]
    plain = store.similarity_search_by_vector(q, k=4)
    assert _book_ids(plain)[:2] == [dup, dup]  # the same book twice in the top 4
    mmr = store.max_marginal_relevance_search_by_vector(q, k=4, fetch_k=20, lambda_mult=0.5)
    assert _book_ids(mmr)[0] == dup and _book_ids(mmr).count(dup) == 1


def _students(golden):
    inputs, _ = golden
    ids = [m["book_id"] for m in inputs["book_metadata"]]
    rng = np.random.default_rng(21)
    profiles, read = [], []
    for s in range(5):
        rated = rng.choice(len(ids), 3 + 3 * s, replace=False)
        profiles.append([(ids[j], float(rng.choice((0.1, 0.3, 0.5, 0.8, 1.0)))) for j in rated])
        read.append([ids[j] for j in rng.choice(len(ids), 4 * s, replace=False)])
    profiles.append([("no-such-book", 1.0)])
    read.append([ids[0]])
    return profiles, read


def test_store_recommend_for_profiles_mmr(catalog, golden):
    store, X = catalog
    profiles, read = _students(golden)
    base = store.recommend_for_profiles(profiles, k=5, exclude=read)
    same = store.recommend_for_profiles(profiles, k=5, exclude=read, mmr=None)
    assert [[(d.id, s) for d, s in r] for r in same] == [[(d.id, s) for d, s in r] for r in base]
    got = store.recommend_for_profiles(profiles, k=5, exclude=read, mmr=(20, 0.5))
    assert got[-1] == [] and len(got) == len(profiles)
    kept, rows, lists = store.profile_requests(profiles, read)
    vec = store.index.mean_rows(rows)
    D, I = store.index.search(vec, 20, exclude=lists)
    for j, p in enumerate(kept):
        want = _oracle_docs(store, X, vec[j], D[j], I[j], 5, 0.5)
        assert [(d.metadata["book_id"], s) for d, s in got[p]] == want
        barred = {b for b, _ in profiles[p]} | set(read[p])
        assert not barred.intersection(_book_ids(d for d, _ in got[p]))


def test_service_mmr(catalog, golden):
    from vsearch.service import IndexService, RemoteFAISS

    store, X = catalog
    # (before a service is started: a build without the methods fails here)
    assert hasattr(RemoteFAISS, "max_marginal_relevance_search_with_score_by_vector")
    assert hasattr(store, "max_marginal_relevance_search_with_score_by_vector")
    profiles, read = _students(golden)
    q = _mix(X, 11, 3, 20)
    key = b"gpu-test-secret"
    flt = {"book_id": {"$in": [store.docstore.search(store.index_to_docstore_id[i])
                               .metadata["book_id"] for i in range(0, X.shape[0], 2)]}}
    with IndexService(store, authkey=key) as svc:
        with RemoteFAISS(svc.address, key) as cli:
            want = store.max_marginal_relevance_search_with_score_by_vector(q, k=5, fetch_k=15,
                                                                            lambda_mult=0.3)
            got = cli.max_marginal_relevance_search_with_score_by_vector(q, k=5, fetch_k=15,
                                                                         lambda_mult=0.3)
            assert [(d.id, np.float32(s)) for d, s in got] == \
                [(d.id, np.float32(s)) for d, s in want]
            assert cli.max_marginal_relevance_search_by_vector(q) == \
                store.max_marginal_relevance_search_by_vector(q)
            assert cli.max_marginal_relevance_search("a quiet book about the sea", k=3) == \
                store.max_marginal_relevance_search("a quiet book about the sea", k=3)
            for exact in (False, True):
                assert cli.max_marginal_relevance_search_by_vector(
                    q, k=3, fetch_k=12, filter=flt, exact_filter=exact) == \
                    store.max_marginal_relevance_search_by_vector(
                        q, k=3, fetch_k=12, filter=flt, exact_filter=exact)
            want = store.recommend_for_profiles(profiles, k=5, exclude=read, mmr=(20, 0.5))
            got = cli.recommend_for_profiles(profiles, k=5, exclude=read, mmr=(20, 0.5))
            assert [[(d.id, np.float32(s)) for d, s in r] for r in got] == \
                [[(d.id, np.float32(s)) for d, s in r] for r in want]
            plain = cli.recommend_for_profiles(profiles, k=5, exclude=read)
            assert [[d.id for d, _ in r] for r in plain] == \
                [[d.id for d, _ in r] for r in store.recommend_for_profiles(profiles, k=5,
                                                                            exclude=read)]
