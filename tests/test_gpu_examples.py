"""GPU: example searches (vs_search_examples / vs_search_examples_x): the rows
nearest to any liked example that no disliked example is at least as near to.

Oracle: ``examples_oracle.search`` (the definition in fp64 over
``flat.exact_scores``).  Bit-identity claims use small-integer rows, where
every key is exact in fp32; random normal rows go through
``examples_oracle.problems`` after the test has asserted, from the oracle
alone, that no row is undecided — so the checker's leniency is never used."""

import itertools

import numpy as np
import pytest

import examples_oracle as eo
from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
N, DIM = 3000, 96
FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def vf():
    from vsearch import _lib
    from vsearch import faiss as vfaiss

    assert _lib.device_count() >= 1
    return vfaiss


def _int_rows(n=N, d=DIM, seed=0):
    return np.random.default_rng(seed).integers(-2, 3, size=(n, d)).astype(np.float32)


def _index(vf, xb, metric, dtype="float32"):
    index = vf.IndexFlat(xb.shape[1], metric, dtype=dtype)
    index.add(xb)
    return index


@pytest.fixture(scope="module")
def int_indexes(vf):
    xb = _int_rows()
    return xb, {m: _index(vf, xb, m) for m in (L2, IP)}


def _equal(got, want):
    for g, w, name in zip(got, want, "DIE"):
        np.testing.assert_array_equal(g, w, err_msg=name)


def _bits_equal(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert g.tobytes() == w.tobytes()


def _mixed_users(rng, n, count, amax=8, bmax=4):
    """(positive labels, negative labels) per user, lists of mixed lengths."""
    pos, neg = [], []
    for _ in range(count):
        a, b = int(rng.integers(1, amax + 1)), int(rng.integers(0, bmax + 1))
        lab = rng.choice(n, a + b, replace=False)
        pos.append(lab[:a].tolist())
        neg.append(lab[a:].tolist())
    return pos, neg


# ---- 1. identity ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("k", [1, 10, 40])
def test_one_positive_is_the_plain_raw_search(vf, int_indexes, metric, k):
    xb, idx = int_indexes
    index = idx[metric]
    first = None
    for nq in (40, 129):
        xq = np.random.default_rng(3).integers(-2, 3, size=(nq, DIM)).astype(np.float32)
        D0, I0 = index.search(xq, k, raw=True)
        D, I, E = index.search_examples([q[None, :] for q in xq], None, k, return_example=True)
        np.testing.assert_array_equal(I, I0)
        assert D.tobytes() == D0.tobytes()
        assert (E == 0).all()
        if first is None:
            first = (xq[:1], D[:1], I[:1])
    # one user alone: the same bits as in the 40-user call (one L2 form whatever the call holds)
    D1, I1 = index.search_examples([first[0]], None, k)
    _bits_equal((D1, I1), first[1:])


# ---- 2. label form = vector form ---------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_label_form_equals_vector_form(vf, metric, dtype):
    xb = np.random.default_rng(0).standard_normal((N, DIM)).astype(np.float32)
    index = _index(vf, xb, metric, dtype)
    stored = index.reconstruct_n(0, N)
    pos, neg = _mixed_users(np.random.default_rng(2), N, 24)
    vpos = [stored[p] for p in pos]
    vneg = [stored[n] if n else np.zeros((0, DIM), np.float32) for n in neg]
    a = index.search_examples(pos, neg, 10, exclude_examples=False, return_example=True)
    b = index.search_examples(vpos, vneg, 10, return_example=True)
    _bits_equal(a, b)
    a = index.search_examples(pos, neg, 10, exclude_examples=True, return_example=True)
    b = index.search_examples(vpos, vneg, 10, exclude=[p + n for p, n in zip(pos, neg)],
                              return_example=True)
    _bits_equal(a, b)
    for u in range(len(pos)):
        assert not set(a[1][u].tolist()) & set(pos[u] + neg[u])


# ---- 3. batch independence -----------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_a_user_alone_equals_the_user_in_a_batch(vf, int_indexes, metric):
    xb, idx = int_indexes
    index = idx[metric]
    pos, neg = _mixed_users(np.random.default_rng(4), N, 40)
    excl = [np.random.default_rng(u).choice(N, u % 5 * 7, replace=False).tolist()
            for u in range(40)]
    D, I, E = index.search_examples(pos, neg, 10, exclude=excl, return_example=True)
    for u in range(40):
        one = index.search_examples([pos[u]], [neg[u]], 10, exclude=[excl[u]],
                                    return_example=True)
        _bits_equal(one, (D[u:u + 1], I[u:u + 1], E[u:u + 1]))


# ---- 4. random normal rows against the checker ----------------------------------------------------
@pytest.fixture(scope="module")
def normal_case():
    xb = np.random.default_rng(0).standard_normal((N, DIM)).astype(np.float32)
    rng = np.random.default_rng(7)
    pos, neg = [], []
    for _ in range(40):
        a = int(rng.integers(1, 9))
        b = int(rng.integers(0, 5))
        lab = rng.choice(N, a + b, replace=False)
        pos.append(lab[:a].tolist())
        neg.append(lab[a:].tolist())
    return xb, pos, neg


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_normal_rows_against_the_checker(vf, normal_case, metric, dtype):
    xb, pos, neg = normal_case
    bf16 = dtype == "bfloat16"
    index = _index(vf, xb, metric, dtype)
    users = [(xb[p], xb[n] if n else None) for p, n in zip(pos, neg)]
    excl = [p + n for p, n in zip(pos, neg)]
    # the condition, from the oracle alone: no allowed row of any user is undecided
    for u, (p, n) in enumerate(users):
        und = eo.undecided(xb, p, n, metric, eo.allowed_mask(N, excl[u]), bf16)
        assert und.size == 0, (u, und[:5])
    for k in (1, 10, 40):
        D, I, E = index.search_examples(pos, neg, k, return_example=True)
        bad = eo.problems(D, I, E, xb, users, k, metric, exclude=excl, bf16=bf16)
        assert not bad, bad[:5]
        assert (I >= 0).all()  # every user has hundreds of favoured rows


# ---- 5. integer rows, bit-exact ------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_integer_rows_equal_the_oracle(vf, int_indexes, metric):
    xb, idx = int_indexes
    index = idx[metric]
    rng = np.random.default_rng(9)
    users, excl = [], []
    for u in range(12):
        a = int(rng.integers(2, 9))
        # positives near one stored row, so their windows overlap
        base = xb[int(rng.integers(N))]
        p = np.repeat(base[None, :], a, axis=0)
        for j in range(a):
            p[j, rng.choice(DIM, 3, replace=False)] += rng.integers(-1, 2, size=3)
        n = xb[rng.choice(N, int(rng.integers(0, 4)), replace=False)] + 0.0
        if u == 3:
            p[1] = p[0]  # two identical positives: E is the lower position
        users.append((p.astype(np.float32), n.astype(np.float32)))
        excl.append(rng.choice(N, int(rng.integers(0, 40)), replace=False).tolist())
    # one user whose liked and disliked vectors are the same: every row ties
    users.append((xb[5:6] + 0.0, xb[5:6] + 0.0))
    excl.append([])
    pos = [p for p, _ in users]
    neg = [n for _, n in users]
    for k in (1, 10, 40):
        got = index.search_examples(pos, neg, k, exclude=excl, return_example=True)
        want = eo.search(xb, users, k, metric, exclude=excl)
        _equal(got, want)
        assert (got[1][-1] == -1).all() and (got[2][-1] == -1).all()
        assert (got[2][3][got[2][3] == 1].size == 0)  # position 1 never decides for user 3


# ---- 6. a window that is too short ----------------------------------------------------------
def _short_window_case(metric):
    rng = np.random.default_rng(11)
    xb = rng.integers(-2, 3, size=(N, DIM)).astype(np.float32)
    g = rng.integers(-2, 3, size=DIM).astype(np.float32)
    g[0] = 0
    c = g if metric == L2 else 3 * g
    hots = [(i,) for i in range(1, DIM)] + list(itertools.combinations(range(1, DIM), 2))
    for j in range(200):
        xb[j] = c
        xb[j, list(hots[j])] += 1
    neg = g[None, :].copy()
    pos = g[None, :].copy()
    pos[0, 0] = -1
    return xb, pos, neg


@pytest.mark.parametrize("metric", [L2, IP])
def test_a_window_that_is_too_short_is_searched_again(vf, metric):
    xb, pos, neg = _short_window_case(metric)
    kp, kn = eo.user_keys(xb, pos, metric), eo.user_keys(xb, neg, metric)
    fav = kp[0] < kn[0]
    assert not fav[:200].any() and int(fav.sum()) == 1155
    if metric == IP:
        assert int((kp[0] == kn[0]).sum()) == 760
    order = np.lexsort((np.arange(N), kp[0]))
    tenth = int(np.nonzero(fav[order])[0][9])
    assert tenth == (222 if metric == L2 else 215)  # past the windows of 26 and 104, inside 416
    index = _index(vf, xb, metric)
    vf.examples_stats(reset=True)
    got = index.search_examples([pos], [neg], 10, return_example=True)
    assert vf.examples_stats() == (1, 3, 1)
    _equal(got, eo.search(xb, [(pos, neg)], 10, metric))


# ---- 7. padding ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_fewer_favoured_rows_than_k_pad(vf, metric):
    xb = _int_rows(50, DIM, seed=6)
    index = _index(vf, xb, metric)
    users = [(xb[[1, 2]], xb[[3]]), (xb[[4]], None), (xb[[7]], xb[[8, 9, 10]])]
    pos = [[1, 2], [4], [7]]
    neg = [[3], [], [8, 9, 10]]
    got = index.search_examples(pos, neg, 40, exclude_examples=False, return_example=True)
    want = eo.search(xb, users, 40, metric)
    _equal(got, want)
    D, I, E = got
    for u in range(3):
        m = int((want[1][u] >= 0).sum())
        assert 0 < m < 40 or u == 1
        assert (I[u, m:] == -1).all() and (E[u, m:] == -1).all()
        assert (D[u, m:] == (FMAX if metric == L2 else -FMAX)).all()
    # an empty index answers a vector call with padding alone
    empty = vf.IndexFlat(DIM, metric)
    D, I, E = empty.search_examples([xb[:2]], [xb[2:3]], 3, return_example=True)
    assert (I == -1).all() and (E == -1).all()


# ---- 8. mutations ----------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_removed_and_updated_rows(vf, metric):
    xb = _int_rows(600, DIM, seed=8)
    index = _index(vf, xb, metric, "bfloat16")  # bf16 indexes keep tombstones until a pack
    gone = [0, 5, 6, 299, 598]
    assert index.remove_ids(np.asarray(gone, dtype=np.int64)) == len(gone)
    keep = np.setdiff1d(np.arange(600), gone)
    cur = xb[keep]
    pos = [[0, 3], [10], [590, 2, 1]]
    neg = [[7], [], [594]]
    users = [(cur[p], cur[n] if n else None) for p, n in zip(pos, neg)]
    excl = [p + n for p, n in zip(pos, neg)]
    got = index.search_examples(pos, neg, 10, return_example=True)
    _equal(got, eo.search(cur, users, 10, metric, exclude=excl))
    with pytest.raises(RuntimeError, match="not a live label"):
        index.search_examples([[595]], None, 3)  # 595 live labels: 0 .. 594
    # an update of a liked row: the results follow the new value
    new = _int_rows(1, DIM, seed=12)
    index.update([10], new)
    cur[10] = new[0]
    users[1] = (cur[[10]], None)
    got = index.search_examples(pos, neg, 10, return_example=True)
    _equal(got, eo.search(cur, users, 10, metric, exclude=excl))


# ---- 9. the store -----------------------------------------------------------------------------
def test_recommend_from_examples_on_the_golden_store(golden, golden_vectors):
    from vsearch import langchain as vlc
    from vsearch.synth import SynthEmbeddings

    inputs, _ = golden
    xb, _, _ = golden_vectors
    store = vlc.FAISS.from_texts(inputs["book_texts"], SynthEmbeddings(),
                                 metadatas=inputs["book_metadata"])
    ids = [m["book_id"] for m in inputs["book_metadata"]]
    assert len(set(ids)) == len(ids)
    liked = [ids[0:3], ["not a book"], ids[10:11], ids[20:28]]
    disliked = [ids[3:5], ids[5:6], [], ids[28:30]]
    exclude = [ids[40:45], [], ids[50:51], []]
    k = 8
    res = store.recommend_from_examples(liked, disliked, k, exclude=exclude, with_reason=True)
    assert res[1] == []
    row = {b: i for i, b in enumerate(ids)}
    for u in (0, 2, 3):
        banned = set(liked[u]) | set(disliked[u]) | set(exclude[u])
        users = [(xb[[row[b] for b in liked[u]]],
                  xb[[row[b] for b in disliked[u]]] if disliked[u] else None)]
        D, I, E = eo.search(xb, users, len(ids), L2, exclude=[[row[b] for b in banned]])
        favoured = int((I[0] >= 0).sum())
        got = [doc.metadata["book_id"] for doc, _, _ in res[u]]
        assert len(got) == min(k, favoured) and len(set(got)) == len(got)
        assert not banned & set(got)
        assert all(reason in liked[u] for _, _, reason in res[u])
        scores = [float(s) for _, s, _ in res[u]]
        assert scores == sorted(scores)
    plain = store.recommend_from_examples(liked, disliked, k, exclude=exclude)
    assert [[d.metadata["book_id"] for d, _ in r] for r in plain] == \
        [[d.metadata["book_id"] for d, _, _ in r] for r in res]
