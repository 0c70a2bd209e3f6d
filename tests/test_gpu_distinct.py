"""GPU: distinct searches (vs_search_distinct): the k nearest groups, one best
row per group.

Oracle: ``distinct_oracle.distinct_topk`` over ``flat.exact_scores``, compared
with ``flat.mismatches``.  That helper does not look at groups, so every check
also asserts that no two returned labels of a query share a group and that
every returned label is the lowest label of its group among the group's rows
with its score (``distinct_oracle.group_problems``).  Bit-identity claims use
small-integer rows, where every score is exact in fp32."""

import numpy as np
import pytest

import distinct_oracle as do
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


def _data(nq, n=N, d=DIM, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)).astype(np.float32),
            rng.standard_normal((nq, d)).astype(np.float32))


def _int_data(nq, n=N, d=DIM, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(-2, 3, size=(n, d)).astype(np.float32),
            rng.integers(-2, 3, size=(nq, d)).astype(np.float32))


def _valid(exclude, nq, n):
    if exclude is None:
        return None
    v = np.ones((nq, n), dtype=bool)
    for q, e in enumerate(exclude):
        e = np.asarray(e, dtype=np.int64)
        v[q, e[(e >= 0) & (e < n)]] = False
    return v


def _check(index, xb, xq, groups, k, *, raw=False, exclude=None, exact=False, grouping=None):
    """One distinct search of ``index`` (rows xb) against the oracle.  Returns (D, I)."""
    metric = index.metric_type
    nq, n = xq.shape[0], xb.shape[0]
    scores = flat.exact_scores(xb, xq, metric)
    valid = _valid(exclude, nq, n)
    Dr, Ir = do.distinct_topk(scores, groups, k, metric, valid=valid,
                              rule="lex" if raw else "faiss")
    D, I = index.search_distinct(xq, k, grouping if grouping is not None else groups,
                                 exclude=exclude, raw=raw)
    if valid is not None:
        for q in range(nq):
            assert valid[q][I[q][I[q] >= 0]].all(), "an excluded label came back"
    if exact:
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_array_equal(D, Dr)
    else:
        bad = flat.mismatches(D, I, Dr, Ir, metric, xb, xq)
        assert not bad, bad[:5]
    bad = do.group_problems(I, scores, groups, valid)
    assert not bad, bad[:5]
    return D, I


# ---- 1. identity ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def int_indexes(vf):
    xb, _ = _int_data(1)
    out = {}
    for metric in (L2, IP):
        index = vf.IndexFlat(DIM, metric)
        index.add(xb)
        out[metric] = (index, index.grouping(np.full(N, -1, dtype=np.int32)),
                       index.grouping(np.arange(N, dtype=np.int32)))
    return xb, out


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 40, 129])
@pytest.mark.parametrize("k", [1, 10, 40])
def test_every_row_its_own_group_is_the_plain_search(vf, int_indexes, metric, nq, k):
    xb, idx = int_indexes
    index, own, ar = idx[metric]
    assert own.groups == N and ar.groups == N
    _, xq = _int_data(nq, seed=3)
    for raw in (False, True):
        D0, I0 = index.search(xq, k, raw=raw)
        for grp in (own, ar):
            D, I = index.search_distinct(xq, k, grp, raw=raw)
            np.testing.assert_array_equal(I, I0)
            np.testing.assert_array_equal(D.view(np.uint32), D0.view(np.uint32))


# ---- 2. group counts -----------------------------------------------------------------
@pytest.fixture(scope="module")
def normal_indexes(vf):
    xb, _ = _data(1)
    out = {}
    for metric in (L2, IP):
        index = vf.IndexFlat(DIM, metric)
        index.add(xb)
        out[metric] = index
    return xb, out


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("G", [1, 5, 50, 1500])
def test_group_counts(vf, normal_indexes, metric, G):
    """G random groups and three rows of their own: G + 3 groups in all, so
    k = 10 pads for G = 1 and G = 5 (and G = 1 needs a window of every row)."""
    xb, idx = normal_indexes
    _, xq = _data(40, seed=4)
    rng = np.random.default_rng(G)
    groups = rng.integers(0, G, N).astype(np.int32)
    groups[rng.choice(N, 3, replace=False)] = -1
    with idx[metric].grouping(groups) as grp:
        assert grp.groups == np.unique(groups[groups >= 0]).size + 3
        for raw in (False, True):
            D, I = _check(idx[metric], xb, xq, groups, 10, raw=raw, grouping=grp)
            want = min(10, grp.groups)
            assert ((I >= 0).sum(axis=1) == want).all()
            assert (D[:, want:] == flat.neutral(metric)).all()


# ---- 3. planted duplicates -----------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_planted_duplicates_come_back_once(vf, metric):
    xb, xq = _data(40, seed=5)
    rng = np.random.default_rng(6)
    groups = (1000 + rng.integers(0, 500, N)).astype(np.int32)
    rows = rng.choice(N, (40, 3), replace=False)
    for q in range(40):
        xb[rows[q]] = xq[q]
        groups[rows[q]] = q
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    D, I = _check(index, xb, xq, groups, 10)
    for q in range(40):
        assert I[q, 0] == rows[q].min()
        assert not np.isin(np.sort(rows[q])[1:], I[q]).any()


# ---- 4. chunk and table edges of the collapse ----------------------------------------
@pytest.mark.parametrize("metric,k,live,w0", [(L2, 170, N, 255), (L2, 171, N, 256),
                                              (L2, 200, 257, 257), (IP, 200, 257, 257),
                                              (L2, 342, N, 513), (IP, 86, N, 256)])
def test_first_window_on_chunk_edges(vf, metric, k, live, w0):
    """Random groups of eight and a first window of 255, 256, 257 or 513
    entries (one chunk less one, one chunk, one more, two and one): at 3,000
    rows it holds about as many groups as the search needs, so some queries
    settle there and some go on; at 257 rows it is every row."""
    assert vf.distinct_plan(k, metric, False, live)[0] == w0
    xb, xq = _data(9, n=live, seed=7)
    groups = np.random.default_rng(8).permutation(live).astype(np.int32) // 8
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    _check(index, xb, xq, groups, k)


def test_k_1024_inner_product(vf):
    """need = 2k - 1 = 2047: the most groups the table is sized for."""
    n = 5000
    xb, xq = _data(5, n=n, seed=9)
    groups = np.random.default_rng(10).integers(0, 4000, n).astype(np.int32)
    index = vf.IndexFlat(DIM, IP)
    index.add(xb)
    _check(index, xb, xq, groups, 1024)
    with pytest.raises(RuntimeError, match="k > 1024"):
        index.search_distinct(xq, 1025, groups)


@pytest.mark.parametrize("metric", [L2, IP])
def test_group_ids_that_collide(vf, normal_indexes, metric):
    """Multiples of 4096 and 8192 (equal low bits), the largest id, and one
    group that fills a whole 256-entry chunk and more: the next chunk must see
    it as kept already."""
    xb0, _ = normal_indexes
    _, xq = _data(12, seed=11)
    rng = np.random.default_rng(12)
    groups = np.where(rng.random(N) < 0.5, rng.integers(0, 300, N) * 4096,
                      rng.integers(0, 200, N) * 8192).astype(np.int64)
    groups[rng.choice(N, 40, replace=False)] = 2**31 - 1
    xb = np.concatenate([xb0, np.repeat(xq[:1], 300, axis=0)])  # 300 copies of query 0
    groups = np.concatenate([groups, np.full(300, 7 * 4096)]).astype(np.int32)
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    for k in (40, 170):  # k = 170: a first window of 255, then 1020
        _check(index, xb, xq, groups, k)


# ---- 5. later rounds -----------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_a_group_of_700_copies_needs_later_rounds(vf, metric):
    xb0, xq = _data(4, seed=13)
    near = flat.knn_exact(xb0, xq, 1, metric)[1][:, 0]
    xb = np.concatenate([xb0] + [np.repeat(xb0[r:r + 1], 700, axis=0) for r in near])
    groups = np.full(xb.shape[0], -1, dtype=np.int32)
    for j, r in enumerate(near):
        groups[r] = j
        groups[N + 700 * j: N + 700 * (j + 1)] = j
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    vf.distinct_stats(reset=True)
    D, I = _check(index, xb, xq, groups, 10)
    assert (I[:, 0] == near).all()
    searches, rounds, requeried = vf.distinct_stats()
    assert searches == 4 and rounds >= 3 and requeried == 4, (searches, rounds, requeried)


@pytest.mark.parametrize("metric", [L2, IP])
def test_mixed_batch_leaves_the_easy_queries_alone(vf, metric):
    """Integer rows.  Half the queries get 700 copies of their nearest row.  A
    query is hard iff its first window holds fewer than `need` groups (worked
    out from the oracle's raw order): `requeried` counts exactly those, and
    the others' rows are the bits of a call with those queries alone."""
    k = 10
    xb0, xq = _int_data(16, seed=14)
    near = flat.knn_lex(xb0, xq[:8], 1, metric)[1][:, 0]
    xb = np.concatenate([xb0] + [np.repeat(xb0[r:r + 1], 700, axis=0) for r in near])
    n = xb.shape[0]
    groups = np.arange(n, dtype=np.int32)
    for j, r in enumerate(near):
        groups[N + 700 * j: N + 700 * (j + 1)] = groups[r]
    need = 2 * k - 1 if metric == IP else k
    w0 = vf.distinct_plan(k, metric, False, n)[0]
    scores = flat.exact_scores(xb, xq, metric)
    key = scores if metric == L2 else -scores
    hard = np.array([np.unique(groups[np.lexsort((np.arange(n), key[q]))[:w0]]).size < need
                     for q in range(16)])
    assert hard[:8].all() and 0 < hard.sum() < 16
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    with index.grouping(groups) as grp:
        vf.distinct_stats(reset=True)
        D, I = _check(index, xb, xq, groups, k, exact=True, grouping=grp)
        assert vf.distinct_stats()[2] == int(hard.sum())
        vf.distinct_stats(reset=True)
        De, Ie = index.search_distinct(xq[~hard], k, grp)
        assert vf.distinct_stats()[1:] == (1, 0)
        np.testing.assert_array_equal(I[~hard], Ie)
        np.testing.assert_array_equal(D[~hard].view(np.uint32), De.view(np.uint32))


# ---- 6. exclusions -------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("m", [0, 3, 300])
def test_exclusions(vf, normal_indexes, metric, m):
    """50 groups of 60 rows.  m = 3: every query's three best representatives
    are excluded, which promotes their groups' next rows; m = 300: every row of
    its five best groups, which removes those groups; query 1 excludes nothing
    and query 2 labels the index does not hold."""
    xb, idx = normal_indexes
    _, xq = _data(20, seed=15)
    groups = (np.random.default_rng(16).permutation(N) % 50).astype(np.int32)
    scores = flat.exact_scores(xb, xq, metric)
    _, I0 = do.distinct_topk(scores, groups, 5, metric)
    if m == 0:
        exclude = [[] for _ in range(20)]
    elif m == 3:
        exclude = [I0[q, :3].tolist() for q in range(20)]
    else:
        exclude = [np.nonzero(np.isin(groups, groups[I0[q]]))[0].tolist() for q in range(20)]
        assert all(len(e) == 300 for e in exclude)
    if m:
        exclude[1] = []
        exclude[2] = [-1, N, N + 5]
    with idx[metric].grouping(groups) as grp:
        for raw in (False, True):
            D, I = _check(idx[metric], xb, xq, groups, 10, raw=raw, exclude=exclude, grouping=grp)
            q = 0
            if m == 3:  # at k = 50 every group comes back, those three through other rows
                D, I = _check(idx[metric], xb, xq, groups, 50, raw=raw, exclude=exclude,
                              grouping=grp)
                assert np.unique(groups[I[q]]).size == 50
                assert not np.isin(I0[q, :3], I[q]).any()
            if m == 300:
                assert not np.isin(groups[I[q]], groups[I0[q]]).any()


# ---- 7. generations and storage ------------------------------------------------------
def test_stale_groupings_are_refused(vf):
    xb, xq = _data(3, n=500, seed=17)
    index = vf.IndexFlatL2(DIM)
    index.add(xb)
    groups = (np.arange(500) // 2).astype(np.int32)

    def stale_after(change):
        with pytest.raises(RuntimeError, match="live row count"):
            index.grouping(np.zeros(index.ntotal + 1, dtype=np.int32))
        grp = index.grouping(np.arange(index.ntotal, dtype=np.int32) // 2)
        index.search_distinct(xq, 5, grp)
        change()
        with pytest.raises(RuntimeError, match="stale grouping"):
            index.search_distinct(xq, 5, grp)
        grp.close()

    stale_after(lambda: index.add(xb[:7]))
    stale_after(lambda: index.remove_ids(np.array([3, 4], dtype=np.int64)))
    stale_after(index.reset)
    index.add(xb)
    with pytest.raises(ValueError):  # (group_ids; the library's own check: test_distinct_host.py)
        index.grouping(np.where(groups == 9, -2, groups))
    with index.grouping(groups) as grp:
        assert grp.groups == 250


@pytest.mark.parametrize("metric", [L2, IP])
def test_bf16_index_with_tombstones(vf, metric):
    """Removals below 1/16 of the rows stay in place as tombstones: a fresh
    grouping over the live labels maps to the rows in place."""
    xb, xq = _data(40, seed=18)
    index = vf.IndexFlat(DIM, metric, dtype="bf16")
    index.add(xb)
    rm = np.random.default_rng(19).choice(N, 100, replace=False).astype(np.int64)
    assert index.remove_ids(rm) == 100 and index.ntotal == N - 100
    live = np.delete(np.arange(N), rm)
    groups = np.random.default_rng(20).integers(0, 400, live.size).astype(np.int32)
    groups[::97] = -1
    ob, oq = flat.round_bf16(xb[live]), flat.round_bf16(xq)
    D, I = _check(index, ob, oq, groups, 10)
    assert I.max() < live.size  # labels are positions among the live rows


# ---- 8. device pointers --------------------------------------------------------------
def test_device_pointers_on_a_side_stream(vf, normal_indexes):
    torch = pytest.importorskip("torch")
    from vsearch import _lib

    xb, idx = normal_indexes
    index = idx[IP]
    _, xq = _data(40, seed=21)
    groups = (np.random.default_rng(22).permutation(N) // 3).astype(np.int32)
    k = 10
    with index.grouping(groups) as grp:
        Dh, Ih = index.search_distinct(xq, k, grp)
        q = torch.from_numpy(xq).cuda()
        D = torch.empty((40, k), dtype=torch.float32, device="cuda")
        I = torch.empty((40, k), dtype=torch.int64, device="cuda")
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            index.search_distinct_device(q.data_ptr(), 40, k, grp, D.data_ptr(), I.data_ptr(),
                                         stream=st.cuda_stream)
        st.synchronize()
        np.testing.assert_array_equal(I.cpu().numpy(), Ih)
        np.testing.assert_array_equal(D.cpu().numpy().view(np.uint32), Dh.view(np.uint32))
        # a capturing stream is refused before anything is enqueued
        g = torch.cuda.CUDAGraph()
        buf = torch.zeros(8, device="cuda")
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            g.capture_begin(capture_error_mode="thread_local")
            try:
                buf.add_(1.0)
                with pytest.raises(_lib.VSearchError, match="capturing stream") as ei:
                    index.search_distinct_device(q.data_ptr(), 40, k, grp, D.data_ptr(),
                                                 I.data_ptr(), stream=st.cuda_stream)
            finally:
                g.capture_end()
        assert ei.value.code == _lib.E_UNSUPPORTED
        del g


# ---- 9. store and service ------------------------------------------------------------
@pytest.fixture(scope="module")
def catalog(golden):
    """The golden CSV sample with the author taken from every book's text, and
    a third of the books re-added through add_texts (the reference's append)."""
    import re

    from vsearch import langchain as vlc
    from vsearch.synth import SynthEmbeddings

    inputs, _ = golden
    texts = inputs["book_texts"]
    metas = [dict(m, author=re.search(r" by (.+?)\. Genre", t).group(1))
             for m, t in zip(inputs["book_metadata"], texts)]
    store = vlc.FAISS.from_texts(texts, SynthEmbeddings(), metadatas=metas)
    again = list(range(0, len(texts), 3))
    store.add_texts([texts[i] for i in again], metadatas=[metas[i] for i in again])
    return store, inputs, metas


def _profiles(metas):
    profiles = [[(metas[(7 * s + j) % len(metas)]["book_id"], 1.0 - 0.2 * j) for j in range(4)]
                for s in range(12)]
    read = [[metas[(11 * s + j) % len(metas)]["book_id"] for j in range(5)] for s in range(12)]
    return profiles, read


def test_store_returns_five_different_books(vf, catalog):
    store, inputs, metas = catalog
    twice = 0
    for kw in inputs["keywords"][:8] + [inputs["book_texts"][0], inputs["book_texts"][3]]:
        plain = store.similarity_search(kw, k=5)
        got = store.similarity_search(kw, k=5, distinct="book_id")
        ids = [d.metadata["book_id"] for d in got]
        assert len(got) == 5 and len(set(ids)) == 5, (kw, ids)
        assert got[0] == plain[0]
        twice += len({d.metadata["book_id"] for d in plain}) < 5
    assert twice  # the plain search does return a re-added book twice
    profiles, read = _profiles(metas)
    rows = store.recommend_for_profiles(profiles, k=6, exclude=read, distinct="author")
    for row, p, r in zip(rows, profiles, read):
        authors = [d.metadata["author"] for d, _ in row]
        assert len(row) == 6 and len(set(authors)) == 6, authors
        assert not ({b for b, _ in p} | set(r)).intersection(d.metadata["book_id"] for d, _ in row)


def test_service_returns_five_different_books(vf, catalog):
    from vsearch.service import IndexService, RemoteFAISS

    store, inputs, metas = catalog
    profiles, read = _profiles(metas)
    with IndexService(store, authkey=b"k") as svc:
        with RemoteFAISS(svc.address, b"k") as cli:
            for kw in inputs["keywords"][:4] + [inputs["book_texts"][0]]:
                got = cli.similarity_search(kw, k=5, distinct="book_id")
                assert got == store.similarity_search(kw, k=5, distinct="book_id")
                assert len({d.metadata["book_id"] for d in got}) == 5
            rows = cli.recommend_for_profiles(profiles, k=6, exclude=read, distinct="author")
            want = store.recommend_for_profiles(profiles, k=6, exclude=read, distinct="author")
            assert [[d for d, _ in r] for r in rows] == [[d for d, _ in r] for r in want]
            for row in rows:
                assert len({d.metadata["author"] for d, _ in row}) == 6
