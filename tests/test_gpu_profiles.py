"""GPU: profile searches (vs_search_excl, vs_mean_rows, vs_search_profiles).

Oracle of the searches: ``flat.select_topk`` over the fp64 scores with
``valid=`` a mask per query, compared with ``flat.mismatches`` as
test_gpu_selector.py does.  Every exclusion case plants two copies of query q:
one in a row only q excludes (an engine that ignores the lists returns it), one
in a row q does not exclude but its neighbour (q + 1) does (an engine that
applies one query's list to another loses it).  The rest of a list is the
query's true nearest rows, then random ones, so the drop reaches as deep as
the list is long.  ``flat.mismatches`` does not check membership, so no
returned label may be in its query's list either.

Oracle of the mean: the numpy statement of the reference's formula
(candidate_builder.py:170-184), compared bit for bit."""

import ctypes
import functools
import threading

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
N, DIM = 3000, 96
# every class boundary of the engine's cap table (16, 64, 256, 1024) is crossed
LENS = (0, 1, 3, 16, 17, 64, 65, 256, 257, 300)
WEIGHTS = (0.1, 0.3, 0.5, 0.8, 1.0)


@pytest.fixture(scope="module")
def vf():
    from vsearch import _lib
    from vsearch import faiss as vfaiss

    assert _lib.device_count() >= 1
    return vfaiss


@functools.lru_cache(maxsize=None)
def _case(nq, lens=LENS, n=N, d=DIM, seed=0):
    """(xb, xq, lists): the planted database, the queries, one row list per
    query.  Rows [0, 2 nq) are the planted copies: row 2q and row 2q + 1 both
    hold query q; q excludes row 2q, query (q + 1) % nq excludes row 2q + 1."""
    rng = np.random.default_rng(seed)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    for q in range(nq):
        xb[2 * q] = xq[q]
        xb[2 * q + 1] = xq[q]
    near = np.argsort(flat.exact_scores(xb, xq, L2), axis=1)
    lists = []
    for q in range(nq):
        m = lens[q % len(lens)]
        rows = []
        if m >= 1:
            rows.append(2 * q)
        if m >= 2 and nq > 1:
            rows.append(2 * ((q - 1) % nq) + 1)
        free = [int(r) for r in near[q] if r >= 2 * nq]
        take = max(0, (m - len(rows)) // 2)
        rows += free[:take]
        rest = np.setdiff1d(np.arange(2 * nq, n), rows)
        rows += rng.choice(rest, m - len(rows), replace=False).tolist()
        lists.append(np.asarray(rows, dtype=np.int64))
    xb.setflags(write=False)
    xq.setflags(write=False)
    return xb, xq, tuple(lists)


def _mask(lists, n):
    valid = np.ones((len(lists), n), dtype=bool)
    for q, rows in enumerate(lists):
        valid[q, rows] = False
    return valid


def _check(vf, index, xb, xq, lists, k, *, raw=False, base=0):
    """index.search(xq, k, exclude=lists + base) against the masked oracle over
    xb (the index's live rows in label order).  Returns (D, I)."""
    metric = index.metric_type
    n = xb.shape[0]
    D, I = index.search(xq, k, exclude=[l + base for l in lists], raw=raw)
    ob, oq = (flat.round_bf16(xb), flat.round_bf16(xq)) if index.dtype == "bf16" else (xb, xq)
    valid = _mask(lists, n)
    Dr, Ir = flat.select_topk(flat.exact_scores(ob, oq, metric), k, metric, valid=valid,
                              rule="lex" if raw else "faiss")
    rows = np.where(I >= 0, I - base, -1)
    for q in range(len(lists)):
        got = rows[q][rows[q] >= 0]
        assert valid[q, got].all(), (q, "an excluded label came back")
    bad = flat.mismatches(D, rows, Dr, Ir, metric, ob, oq)
    assert not bad, bad[:5]
    return D, I


def _check_plants(I, lists, nq, base=0):
    """Row 2q + 1 (a copy of q that q does not exclude) is returned; row 2q is
    returned exactly when q's list is empty."""
    for q in range(nq):
        got = set((I[q][I[q] >= 0] - base).tolist())
        assert 2 * q + 1 in got, (q, "the copy another query excludes is missing")
        assert (2 * q in got) == (len(lists[q]) == 0), q


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("metric", [L2, IP])
def test_ragged_lists(vf, metric, k, raw):
    xb, xq, lists = _case(40)
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    _, I = _check(vf, index, xb, xq, lists, k, raw=raw)
    _check_plants(I, lists, 40)


@pytest.mark.parametrize("nq", [1, 24])
def test_ragged_lists_l2_small_calls(vf, nq):
    """nq = 1 is faiss's sequential branch; at nq = 24 (the BLAS branch) every
    class holds fewer than 20 queries and still takes the call's formula."""
    xb, xq, lists = _case(nq, lens=(65,) if nq == 1 else LENS)
    index = vf.IndexFlat(DIM, L2)
    index.add(xb)
    _, I = _check(vf, index, xb, xq, lists, 10)
    _check_plants(I, lists, nq)


@pytest.mark.parametrize("metric", [L2, IP])
def test_ragged_lists_bf16(vf, metric):
    xb, xq, lists = _case(40)
    index = vf.IndexFlat(DIM, metric, dtype="bf16")
    index.add(xb)
    _, I = _check(vf, index, xb, xq, lists, 10)
    _check_plants(I, lists, 40)


def test_csr_pair_equals_lists(vf):
    xb, xq, lists = _case(40)
    index = vf.IndexFlat(DIM, L2)
    index.add(xb)
    D, I = index.search(xq, 10, exclude=list(lists))
    D2, I2 = index.search(xq, 10, exclude=vf.exclusion_csr(list(lists), 40))
    np.testing.assert_array_equal(I, I2)
    np.testing.assert_array_equal(D, D2)


@pytest.mark.parametrize("metric", [L2, IP])
def test_ignored_labels(vf, metric):
    """Duplicates, -1, labels past the index and labels below its base are
    ignored: the result is that of the cleaned lists."""
    xb, xq, lists = _case(40)
    base = 1000
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    index.set_id_base(base)
    clean = [l + base for l in lists]
    junk = np.asarray([-1, base + N + 5, base - 1, base + N, 5], dtype=np.int64)
    dirty = [np.concatenate([junk, l, l[: 3], junk]) for l in clean]
    D, I = index.search(xq, 10, exclude=clean)
    D2, I2 = index.search(xq, 10, exclude=dirty)
    np.testing.assert_array_equal(I2, I)
    np.testing.assert_array_equal(D2, D)
    # junk alone excludes nothing: the plain search
    D3, I3 = index.search(xq, 10, exclude=[junk] * 40)
    Dp, Ip = index.search(xq, 10)
    np.testing.assert_array_equal(I3, Ip)
    np.testing.assert_array_equal(D3, Dp)


@pytest.mark.parametrize("metric", [L2, IP])
def test_padding(vf, metric):
    """One query excludes all but 3 rows: 3 entries, then (neutral, -1)."""
    n = 400
    rng = np.random.default_rng(7)
    xb = rng.standard_normal((n, DIM)).astype(np.float32)
    xq = rng.standard_normal((3, DIM)).astype(np.float32)
    keep = np.asarray([11, 200, 399])
    lists = (np.zeros(0, dtype=np.int64), np.setdiff1d(np.arange(n), keep),
             np.asarray([0], dtype=np.int64))
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    D, I = _check(vf, index, xb, xq, lists, 10)
    assert sorted(I[1, :3].tolist()) == keep.tolist()
    assert (I[1, 3:] == -1).all() and (D[1, 3:] == flat.neutral(metric)).all()
    assert (I[0] >= 0).all() and (I[2] >= 0).all()


@pytest.mark.parametrize("metric", [L2, IP])
def test_id_base(vf, metric):
    xb, xq, lists = _case(40)
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    index.set_id_base(1000)
    _, I = _check(vf, index, xb, xq, lists, 10, base=1000)
    _check_plants(I, lists, 40, base=1000)


@pytest.mark.parametrize("metric", [L2, IP])
def test_bf16_after_remove_ids(vf, metric):
    """A bf16 index keeps removed rows in place: labels are positions among
    the live rows, and so are the lists'."""
    xb, xq, lists = _case(40)
    gone = np.asarray([90, 91, 500, 1999, N - 1])  # none of the planted rows
    index = vf.IndexFlat(DIM, metric, dtype="bf16")
    index.add(xb)
    assert index.remove_ids(gone) == gone.size
    left = np.delete(xb, gone, axis=0)
    new_label = np.cumsum(~np.isin(np.arange(N), gone)) - 1
    moved = tuple(new_label[l[~np.isin(l, gone)]] for l in lists)
    _, I = _check(vf, index, left, xq, moved, 10)
    _check_plants(I, moved, 40)


def test_ip_tie_rule(vf):
    """12 identical rows that are every query's best, some of them excluded:
    faiss's order over the allowed rows, exactly."""
    rng = np.random.default_rng(11)
    xb = rng.standard_normal((N, DIM)).astype(np.float32)
    v = rng.standard_normal(DIM).astype(np.float32)
    twins = np.asarray([3, 40, 41, 700, 701, 702, 1500, 2000, 2001, 2500, 2998, 2999])
    xb[twins] = 2.0 * v
    xq = (v[None, :] + 0.05 * rng.standard_normal((4, DIM))).astype(np.float32)
    lists = (twins[[1, 4, 7, 10]], twins[[0, 2, 3, 8, 11]], np.zeros(0, dtype=np.int64),
             np.concatenate([twins[:6], np.arange(100, 120)]))
    index = vf.IndexFlat(DIM, IP)
    index.add(xb)
    for k in (5, 10):
        D, I = index.search(xq, k, exclude=list(lists))
        Dr, Ir = flat.select_topk(flat.exact_scores(xb, xq, IP), k, IP, valid=_mask(lists, N),
                                  rule="faiss")
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_allclose(D, Dr, rtol=1e-5)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 40])
def test_all_lists_empty_is_the_plain_search(vf, metric, nq):
    from vsearch import _lib

    xb, xq, _ = _case(40)
    xq = xq[:nq]
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    D, I = index.search(xq, 10)
    name = _lib.timer_kernel()
    D2, I2 = index.search(xq, 10, exclude=[[] for _ in range(nq)])
    assert _lib.timer_kernel() == name
    np.testing.assert_array_equal(I2, I)
    np.testing.assert_array_equal(D2, D)
    lib = _lib.load()
    D3 = np.empty_like(D)
    I3 = np.empty_like(I)
    _lib.check(lib.vs_search_excl(index._h, xq.ctypes.data, nq, 10, None, None, D3.ctypes.data,
                                  I3.ctypes.data, 0, None))
    assert _lib.timer_kernel() == name
    np.testing.assert_array_equal(I3, I)
    np.testing.assert_array_equal(D3, D)


def test_device_outputs(vf):
    import torch

    from vsearch import _lib

    xb, xq, lists = _case(40)
    index = vf.IndexFlat(DIM, L2)
    index.add(xb)
    D, I = index.search(xq, 10, exclude=list(lists))
    offs, labels = vf.exclusion_csr(list(lists), 40)
    q = torch.from_numpy(xq.copy()).cuda()
    Dd = torch.empty((40, 10), dtype=torch.float32, device="cuda")
    Id = torch.empty((40, 10), dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().vs_search_excl(
        index._h, ctypes.c_void_p(q.data_ptr()), 40, 10, offs.ctypes.data, labels.ctypes.data,
        ctypes.c_void_p(Dd.data_ptr()), ctypes.c_void_p(Id.data_ptr()),
        _lib.IN_DEVICE | _lib.OUT_DEVICE, None))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Id.cpu().numpy(), I)
    np.testing.assert_array_equal(Dd.cpu().numpy(), D)


# ---- the mean ---------------------------------------------------------------------------
def np_mean(rows, labels, weights):
    """The reference's formula: np.sum([emb * w ...], axis=0) / total_weight,
    float32 rows and weights, the total summed in double in list order."""
    w32 = np.asarray(weights, dtype=np.float32)
    total = 0.0
    for w in w32:
        total += float(w)
    return np.sum([rows[l] * w for l, w in zip(labels, w32)], axis=0) / np.float32(total)


def _profiles(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for size in (1, 2, 9, 257, 9, 1):
        labels = rng.integers(0, n, size)
        out.append((labels, rng.choice(WEIGHTS, size)))
    rep = np.asarray([5, 17, 5, 5, 300, 17])  # a repeated label inside one profile
    out.append((rep, rng.choice(WEIGHTS, rep.size)))
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [70, 96, 1536])
def test_mean_rows_is_the_numpy_formula(vf, d, dtype):
    import torch

    n = 600
    rng = np.random.default_rng(d)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    index = vf.IndexFlat(d, L2, dtype=dtype)
    index.add(xb)
    rows = flat.round_bf16(xb) if dtype == "bf16" else xb
    profiles = _profiles(n, seed=d + 1)
    got = index.mean_rows(profiles)
    assert got.dtype == np.float32 and got.shape == (len(profiles), d)
    for i, (labels, weights) in enumerate(profiles):
        np.testing.assert_array_equal(got[i], np_mean(rows, labels, weights), err_msg=str(i))
    dev = torch.full((len(profiles), d), float("nan"), dtype=torch.float32, device="cuda")
    index.mean_rows_device(profiles, dev.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy(), got)


def test_mean_rows_labels_follow_base_and_tombstones(vf):
    n, d = 600, 96
    rng = np.random.default_rng(3)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    index = vf.IndexFlat(d, IP, dtype="bf16")
    index.add(xb)
    index.remove_ids(np.asarray([0, 7, 8, 300]))
    index.set_id_base(50)
    left = flat.round_bf16(np.delete(xb, [0, 7, 8, 300], axis=0))
    labels = np.asarray([0, 6, 7, 298, 595])
    weights = np.asarray([0.5, 1.0, 0.1, 0.3, 0.8])
    got = index.mean_rows([(labels + 50, weights)])
    np.testing.assert_array_equal(got[0], np_mean(left, labels, weights))


def test_mean_rows_errors(vf):
    from vsearch import _lib

    rng = np.random.default_rng(4)
    index = vf.IndexFlat(DIM, L2, dtype="bf16")
    index.add(rng.standard_normal((100, DIM)).astype(np.float32))
    index.remove_ids(np.asarray([99]))
    bad = [[([100], [1.0])],                      # past the index
           [([99], [1.0])],                       # removed: 99 live labels are 0 .. 98
           [([-1], [1.0])],
           [([1], [1.0]), ([], [])],              # an empty profile
           [([1, 2], [0.5, -0.5])],               # zero total weight
           [([1], [float("inf")])]]
    for profiles in bad:
        with pytest.raises(_lib.VSearchError) as ei:
            index.mean_rows(profiles)
        assert ei.value.code == _lib.E_INVALID, profiles
        with pytest.raises(_lib.VSearchError) as ei:
            index.search_profiles(profiles, 5)
        assert ei.value.code == _lib.E_INVALID, profiles
    assert index.mean_rows([([98], [0.3])]).shape == (1, DIM)


# ---- both -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", [L2, IP])
def test_search_profiles_is_search_of_the_means(vf, metric, dtype):
    xb, _, lists = _case(40)
    index = vf.IndexFlat(DIM, metric, dtype=dtype)
    index.add(xb)
    rng = np.random.default_rng(5)
    profiles = [(rng.integers(0, N, s), rng.choice(WEIGHTS, s)) for s in rng.integers(1, 31, 40)]
    means = index.mean_rows(profiles)
    for extra in (None, list(lists)):
        D, I = index.search_profiles(profiles, 10, exclude=extra, exclude_profile=True)
        both = [np.concatenate([p[0], extra[q]]) if extra is not None else p[0]
                for q, p in enumerate(profiles)]
        D2, I2 = index.search(means, 10, exclude=both)
        np.testing.assert_array_equal(I, I2)
        np.testing.assert_array_equal(D, D2)
        for q, p in enumerate(profiles):
            assert not np.isin(I[q], both[q]).any()
    D, I = index.search_profiles(profiles, 10, exclude_profile=False)
    D2, I2 = index.search(means, 10)
    np.testing.assert_array_equal(I, I2)
    np.testing.assert_array_equal(D, D2)


@pytest.mark.parametrize("metric", [L2, IP])
def test_one_row_profile_returns_that_row_first(vf, metric):
    xb, _, _ = _case(40)
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    # rows past the planted twins; the norms of standard normal rows of DIM
    # entries differ, so inner product is checked on the row of largest norm
    rows = [100, 2999] if metric == L2 else [int(np.argmax((xb[80:] ** 2).sum(1))) + 80]
    profiles = [([r], [0.8]) for r in rows]
    _, I = index.search_profiles(profiles, 5, exclude_profile=False)
    assert I[:, 0].tolist() == rows
    _, I = index.search_profiles(profiles, 5, exclude_profile=True)
    assert not any(r in I[q] for q, r in enumerate(rows))


# ---- store and service ------------------------------------------------------------------
@pytest.fixture(scope="module")
def catalog_store(golden):
    from vsearch import langchain as vlc
    from vsearch.synth import SynthEmbeddings

    inputs, _ = golden
    return vlc.FAISS.from_texts(inputs["book_texts"], SynthEmbeddings(),
                                metadatas=inputs["book_metadata"])


def _students(golden, n=6):
    """Profiles of rated books with RATING_WEIGHTS-like weights, the books each
    student has read besides, and one student whose books the store lacks."""
    inputs, _ = golden
    ids = [m["book_id"] for m in inputs["book_metadata"]]
    rng = np.random.default_rng(21)
    profiles, read = [], []
    for s in range(n):
        rated = rng.choice(len(ids), 3 + 4 * s, replace=False)
        profiles.append([(ids[j], float(rng.choice(WEIGHTS))) for j in rated])
        read.append([ids[j] for j in rng.choice(len(ids), 5 * s, replace=False)])
    profiles.append([("no-such-book", 1.0), ("nor-this-one", 0.5)])
    read.append([ids[0]])
    # a student who has read all but two books
    profiles.append([(ids[1], 1.0), (ids[2], 0.3)])
    read.append(ids[4:])
    return profiles, read


def test_store_recommend_for_profiles(catalog_store, golden):
    profiles, read = _students(golden)
    nbooks = len(golden[0]["book_metadata"])
    k = 7
    res = catalog_store.recommend_for_profiles(profiles, k=k, exclude=read)
    assert len(res) == len(profiles)
    for p, r, row in zip(profiles, read, res):
        rated = {b for b, _ in p}
        if "no-such-book" in rated:
            assert row == []
            continue
        barred = rated | set(r)
        assert len(row) == min(k, nbooks - len(barred))
        got = [d.metadata["book_id"] for d, _ in row]
        assert len(set(got)) == len(got) and not barred.intersection(got)
        scores = [float(s) for _, s in row]
        assert scores == sorted(scores)  # an L2 store: ascending distance
    assert len(res[-1]) == 2  # the last student: every book but two is rated or read
    # the single-query form: exclude_ids drops documents from the search itself
    vec = catalog_store.index.reconstruct(10)
    first = catalog_store.similarity_search_with_score_by_vector(vec, k=3)
    drop = [d.id for d, _ in first[:2]]
    again = catalog_store.similarity_search_with_score_by_vector(vec, k=3, exclude_ids=drop)
    assert len(again) == 3 and not set(drop).intersection(d.id for d, _ in again)
    assert again[0][0].id == first[2][0].id


def test_service_recommend_for_profiles(catalog_store, golden):
    from vsearch.service import IndexService, RemoteFAISS

    profiles, read = _students(golden)
    k = 7
    want = catalog_store.recommend_for_profiles(profiles, k=k, exclude=read)
    halves = [slice(0, 4), slice(4, None)]
    got = {}
    key = b"gpu-test-secret"
    with IndexService(catalog_store, authkey=key) as svc:
        barrier = threading.Barrier(2, timeout=60)

        def worker(i):
            with RemoteFAISS(svc.address, key) as cli:
                barrier.wait()
                got[i] = cli.recommend_for_profiles(profiles[halves[i]], k=k,
                                                    exclude=read[halves[i]])

        ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(90)
        print("service stats:", svc.stats)
        # the faiss-level op with per-row lists
        with RemoteFAISS(svc.address, key) as cli:
            vec = catalog_store.index.reconstruct_n(0, 2)
            D, I = cli.index.search(vec, 3, exclude=[[0], []])
            assert I[1, 0] == 1 and 0 not in I[0]
    both = got[0] + got[1]
    assert len(both) == len(want)
    for a, b in zip(both, want):
        assert [d.id for d, _ in a] == [d.id for d, _ in b]
        # a stacked batch may take faiss's other L2 branch: scores to fp32 tolerance
        np.testing.assert_allclose([s for _, s in a], [s for _, s in b], rtol=1e-5, atol=1e-5)
