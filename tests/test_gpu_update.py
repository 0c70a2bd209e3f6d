"""GPU: in-place updates (vs_update_rows; IndexFlat.update) and the row-list
range self-join (vs_range_selfjoin_rows; IndexFlat.range_selfjoin(rows=...)).

An update must leave the index as an add of the same values would have: the
stored bytes (reconstruct_n, bit for bit) and every derived array — norms,
int8 codes and scales, the bf16 plane, residual and augmented norms, the bound
maxima.  The derived arrays cannot be read back, so they are checked through
what they decide: searches of every engine against candidates proven from the
final matrix (helpers.proven_candidates, strict wherever the staged engine
answers, as tests/test_gpu_parity.py is), with queries that a stale byte would
lose (the new vector itself) or keep answering (the replaced vector).

The row-list join is checked against the window form it restates (bytes), and
against the fp64 reference as tests/test_gpu_range_join.py checks the window
form: every pair with s >= t + w present, none with s < t - w, |S - s| <= w,
at most CAP = 4 undecided ordered pairs per case (that file's header: the fp64
reference leaves 0 on seed0 at 0.2, 2 on its bf16 rows, 0 on seed5 at 0.05; a
subset of the query rows has a subset of the pairs)."""

import functools

import numpy as np
import pytest

from helpers import assert_against_candidates, proven_candidates
from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
SHAPES = [(3000, 96), (700, 1536)]
EDGE_ROWS = (0, 127, 128, 255, 256, -1)
CAP = 4


@pytest.fixture(scope="module")
def vf():
    from vsearch import _lib
    from vsearch import faiss as vfaiss

    assert _lib.device_count() >= 1
    return vfaiss


@functools.lru_cache(maxsize=None)
def _rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    x.setflags(write=False)
    return x


def _stored(x, dtype):
    return flat.round_bf16(x) if dtype == "bf16" else np.asarray(x, dtype=np.float32)


def _staged(metric, nq, k, engine, dtype):
    """tests/test_gpu_parity.py _staged: the searches the staged engine answers
    (fp32 indexes, more than 32 queries), whose keys are exact roundings."""
    need = 2 * k - 1 if metric == IP else k
    return dtype == "f32" and engine != "fp32" and nq > 32 and need + 8 <= 64


def _check_searches(index, xs, metric, k, strict, dtype, base=0, m=64):
    """Every query of xs against candidates proven from the index's rows (which
    the caller has compared with the expected matrix bit for bit).  m: the
    preselected rows per query; their margin over the k-th must exceed the fp32
    preselection's own error, which grows with the largest row norm."""
    xs = np.ascontiguousarray(xs, dtype=np.float32)
    D, I = index.search(xs, k)
    qs = _stored(xs, dtype)  # a bf16 index rounds its queries
    cands = proven_candidates(index, qs, metric, index.ntotal, k, m=m)
    for q in range(xs.shape[0]):
        assert_against_candidates(D[q], I[q] - base, cands[q], metric, k, xs.shape[1], strict)
    return D, I


def _update_plan(n, d, seed):
    """Labels (the tile-edge rows, then 300 shuffled ones) and their new rows."""
    rng = np.random.default_rng(seed)
    edge = np.array([r % n for r in EDGE_ROWS], dtype=np.int64)
    rest = np.setdiff1d(np.arange(n), edge)
    many = rng.permutation(rest)[:300].astype(np.int64)
    new = rng.standard_normal((edge.size + many.size, d)).astype(np.float32)
    return edge, many, new


# ---- bytes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("metric,dtype", [(IP, "f32"), (L2, "f32"), (IP, "bf16"), (L2, "bf16")])
def test_bytes(vf, n, d, metric, dtype):
    x = _rows(n, d, 1)
    index = vf.IndexFlat(d, metric, dtype=dtype)
    index.add(x)
    edge, many, new = _update_plan(n, d, 2)
    want = _stored(x, dtype).copy()
    index.update(edge, new[:edge.size])
    want[edge] = _stored(new[:edge.size], dtype)
    assert index.reconstruct_n(0, n).tobytes() == want.tobytes()
    index.update(many, new[edge.size:])
    want[many] = _stored(new[edge.size:], dtype)
    assert index.ntotal == n
    assert index.reconstruct_n(0, n).tobytes() == want.tobytes()  # every untouched row too
    index.update(many, new[edge.size:])  # the same update again changes nothing
    index.update(edge, new[:edge.size])
    assert index.reconstruct_n(0, n).tobytes() == want.tobytes()
    np.testing.assert_array_equal(index.reconstruct(int(many[5])), want[many[5]])


# ---- stale derived data ---------------------------------------------------------------------------
ENGINES = {"f32": ("auto", "fp32", "i8v", "bf16v"), "bf16": ("auto", "fp32")}
STALE_CASES = [(n, d, metric, dtype, engine) for n, d in SHAPES for metric in (IP, L2)
               for dtype in ("f32", "bf16") for engine in ENGINES[dtype]]


@pytest.mark.parametrize("n,d,metric,dtype,engine", STALE_CASES)
def test_no_stale_derived_data(vf, n, d, metric, dtype, engine):
    k = 10
    x = _rows(n, d, 3)
    index = vf.IndexFlat(d, metric, dtype=dtype)
    index.set_engine(engine)
    index.add(x)
    edge, many, new = _update_plan(n, d, 4)
    labels = np.concatenate([edge, many])
    index.update(labels, new)
    want = _stored(x, dtype).copy()
    want[labels] = _stored(new, dtype)
    assert index.reconstruct_n(0, n).tobytes() == want.tobytes()
    fresh = _rows(256, d, 5)
    for batch in (1, 37, 256):
        strict = _staged(metric, batch, k, engine, dtype)
        # (a) the new vectors themselves: their labels come first
        D, I = _check_searches(index, new[:batch], metric, k, strict, dtype)
        np.testing.assert_array_equal(I[:, 0], labels[:batch])
        # (b) the vectors they replaced, (c) fresh queries
        _check_searches(index, x[labels[:batch]], metric, k, strict, dtype)
        _check_searches(index, fresh[:batch], metric, k, strict, dtype)


def test_bf16_int8_plane_follows_update(vf):
    """A bf16 inner-product index keeps an int8 plane, which only batches of at
    most 32 queries over at least 2^18 rows read (tests/test_gpu_bf16.py): the
    smallest index at which stale codes or scales of that plane can show."""
    from vsearch import _lib

    n, d = 1 << 18, 64
    rng = np.random.default_rng(6)
    x = rng.standard_normal((n, d)).astype(np.float32)
    index = vf.IndexFlat(d, IP, dtype="bf16")
    index.add(x)
    assert index.filter_planes == ("i8",)
    labels = rng.permutation(n)[:300].astype(np.int64)
    new = (1.5 * rng.standard_normal((300, d))).astype(np.float32)
    index.update(labels, new)
    want = flat.round_bf16(x)
    want[labels] = flat.round_bf16(new)
    for xs, first in ((new[:8], labels[:8]), (x[labels[:8]], None), (new[8:40], labels[8:40])):
        _lib.filter_stats(reset=True)
        D, I = index.search(xs, 10)
        fq, _ = _lib.filter_stats(reset=True)
        assert fq == xs.shape[0]  # the int8 plane's filter pass ran
        rq = flat.round_bf16(xs)
        Dr, Ir = flat.knn_exact(want, rq, 10, IP)
        bad = flat.mismatches(D, I, Dr, Ir, IP, want, rq, strict=True)
        assert not bad, bad[:3]
        if first is not None:
            np.testing.assert_array_equal(I[:, 0], first)


# ---- bound maxima and scales ----------------------------------------------------------------------
@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("engine", ["i8v", "bf16v"])
def test_bound_maxima_and_scales(vf, n, d, metric, engine):
    k = 10
    x = _rows(n, d, 7)
    index = vf.IndexFlat(d, metric)
    index.set_engine(engine)
    index.add(x)
    big = int(np.argmax(np.einsum("ij,ij->i", x, x, dtype=np.float64)))
    labels = np.array([n // 3, 2 * n // 3 + 1], dtype=np.int64)
    assert big not in labels
    new = np.stack([50.0 * x[big], np.float32(1e-3) * x[17]]).astype(np.float32)
    index.update(labels, new)
    want = x.copy()
    want[labels] = new
    assert index.reconstruct_n(0, n).tobytes() == want.tobytes()
    # a maximum that did not grow would let the filter prove wrong answers
    fresh = _rows(64, d, 8)
    xs = np.concatenate([new, x[labels], x[big:big + 1], fresh[:59]])  # 64 queries: staged
    # (m = 256: the 50x row multiplies the preselection's error bound by 50)
    _check_searches(index, xs, metric, k, True, "f32", m=256)
    D, I = _check_searches(index, np.concatenate([new[:1]] * 2 + [fresh[:35]]), metric, k, True,
                           "f32", m=256)
    if metric == L2:
        assert I[0, 0] == labels[0]
    # the exact key decides a range search: bit-equal to an index built from the final rows
    other = vf.IndexFlat(d, metric)
    other.add(want)
    xq = fresh[:25]
    s = flat.exact_scores(want, xq, metric)
    radius = float(np.median(s))
    got, ref = index.range_search(xq, radius), other.range_search(xq, radius)
    assert 0 < len(got[1]) < xq.shape[0] * n
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- tombstones and labels ------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1000])
def test_tombstones_and_labels(vf, base):
    n, d = 3000, 96
    x = _rows(n, d, 9)
    index = vf.IndexFlat(d, IP, dtype="bf16")
    index.add(x)
    if base:
        index.set_id_base(base)
    rm = np.array([5, 1500, 1501, 2990], dtype=np.int64)  # before, between and after; unpacked
    assert index.remove_ids(rm + base) == rm.size
    want, _ = flat.remove_ids(flat.round_bf16(x), rm)
    labels = np.array([100, 4, 1499, 1500, 2900, want.shape[0] - 1], dtype=np.int64)
    new = _rows(labels.size, d, 10)
    old = want[labels].copy()
    np.testing.assert_array_equal(old, flat.round_bf16(x[[101, 4, 1502, 1503, 2903, 2999]]))
    index.update(labels + base, new)
    want[labels] = flat.round_bf16(new)
    assert index.ntotal == want.shape[0]
    # (reconstruct_n takes positions among the live rows, whatever the base)
    assert index.reconstruct_n(0, want.shape[0]).tobytes() == want.tobytes()
    # the new vectors, the vectors they replaced, fresh queries
    for xs in (new, old, _rows(37, d, 11)):
        D, I = _check_searches(index, xs, IP, 10, False, "bf16", base=base)
        rq = flat.round_bf16(xs)
        Dr, Ir = flat.knn_exact(want, rq, 10, IP)
        assert not flat.mismatches(D, I - base, Dr, Ir, IP, want, rq)
        if xs is new:
            np.testing.assert_array_equal(I[:, 0], labels + base)


# ---- handles --------------------------------------------------------------------------------------
def test_handles_stay_valid(vf):
    n, d = 3000, 96
    x = _rows(n, d, 12)
    index = vf.IndexFlatL2(d)
    index.add(x)
    sel = index.selector(vf.IDSelectorRange(100, 400))
    groups = (np.arange(n) // 3).astype(np.int32)
    grp = index.grouping(groups)
    params = vf.SearchParameters(sel=sel)
    xq = _rows(40, d, 13)
    index.search(xq, 5, params=params)
    index.search_distinct(xq, 5, grp)
    labels = np.array([150, 399, 2000], dtype=np.int64)
    new = _rows(3, d, 14)
    index.update(labels, new)
    want = x.copy()
    want[labels] = new
    # no "stale" error, and both see the new vectors
    D, I = index.search(new, 5, params=params)
    assert I[0, 0] == 150 and I[1, 0] == 399 and D[0, 0] < 1e-3 and D[1, 0] < 1e-3
    assert ((I >= 100) & (I < 400)).all() and I[2, 0] != 2000
    mask = np.zeros(n, dtype=bool)
    mask[100:400] = True
    Dr, Ir = flat.select_topk(flat.exact_scores(want, new, L2), 5, L2,
                              valid=mask[None, :].repeat(3, 0), rule="faiss")
    assert not flat.mismatches(D, I, Dr, Ir, L2, want, new)
    D, I = index.search_distinct(new, 5, grp)
    np.testing.assert_array_equal(I[:, 0], labels)
    assert (D[:, 0] < 1e-3).all()
    for q in range(3):
        assert len(set(groups[I[q]].tolist())) == 5
    # an add still makes them stale
    index.add(x[:2])
    with pytest.raises(RuntimeError, match="stale selector"):
        index.search(xq, 5, params=params)
    with pytest.raises(RuntimeError, match="stale grouping"):
        index.search_distinct(xq, 5, grp)


# ---- errors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_errors_leave_the_index_unchanged(vf, dtype):
    from vsearch import _lib

    n, d = 700, 96
    x = _rows(n, d, 15)
    index = vf.IndexFlatIP(d, dtype=dtype)
    index.add(x)
    assert index.remove_ids(np.array([10], dtype=np.int64)) == 1
    live = n - 1
    want, _ = flat.remove_ids(_stored(x, dtype), np.array([10]))
    new = _rows(3, d, 16)
    # -1, ntotal, a label the removal retired (live before it, past the end now), a duplicate
    for labels in ([5, -1, 7], [5, live + 1, 7], [live, 6, 7], [5, 7, 5]):
        with pytest.raises(RuntimeError) as e:
            index.update(np.array(labels, dtype=np.int64), new)
        assert e.value.code == _lib.E_INVALID, labels
        assert "vs_update_rows: label" in str(e.value)
        assert index.reconstruct_n(0, live).tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        index.update([1, 2], new)
    index.update(np.empty(0, dtype=np.int64), np.empty((0, d), dtype=np.float32))  # n = 0
    assert index.reconstruct_n(0, live).tobytes() == want.tobytes()
    index.update([live - 1], new[:1])
    want[live - 1] = _stored(new[:1], dtype)[0]
    assert index.reconstruct_n(0, live).tobytes() == want.tobytes()


# ---- the row-list join ----------------------------------------------------------------------------
JOIN_DATA = {"seed0": (0, 3000, 96, 0.2), "seed5": (5, 700, 1536, 0.05)}


@functools.lru_cache(maxsize=None)
def _join_rows(name):
    seed, n, d, _ = JOIN_DATA[name]
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(name, bf16=False):
    """(fp64 cosines, windows) of every ordered pair of rows."""
    x = _join_rows(name)
    x64 = np.asarray(flat.round_bf16(x) if bf16 else x, dtype=np.float64)
    n2 = np.einsum("ij,ij->i", x64, x64)
    s = (x64 @ x64.T) / np.sqrt(np.outer(n2, n2))
    return s, flat.key_window(0, s, 0, 0, x.shape[1], cosine=True)


def _check_rows(result, s, w, t, rows, exclude_self=True):
    """tests/test_gpu_range_join.py _check with the query rows given as a list."""
    from vsearch import _lib

    lims, S, I = result
    n, nq = s.shape[0], len(rows)
    assert _lib.timer_kernel() == "gemm_range"
    assert lims.dtype == np.uint64 and S.dtype == np.float32 and I.dtype == np.int64
    assert lims.shape == (nq + 1,) and lims[0] == 0 and lims[-1] == len(S) == len(I)
    li = lims.astype(np.int64)
    assert (np.diff(li) >= 0).all()
    q = np.repeat(np.arange(nq), np.diff(li))
    assert ((I >= 0) & (I < n)).all()
    same_q = q[1:] == q[:-1]
    assert (np.diff(I)[same_q] > 0).all(), "labels not strictly ascending inside a query"
    got = np.zeros((nq, n), dtype=bool)
    got[q, I] = True
    s, w = s[rows], w[rows]
    valid = np.ones((nq, n), dtype=bool)
    if exclude_self:
        valid[np.arange(nq), rows] = False
    inside = (s >= t + w) & valid
    outside = ~(s >= t - w) | ~valid
    undecided = int((~(inside | outside)).sum())
    print(f"hits {len(S)} undecided {undecided}")
    assert undecided <= CAP, undecided
    assert got[inside].all(), "a pair at or above the threshold is missing"
    assert not got[outside].any(), "a pair below the threshold (or excluded) was returned"
    assert (np.abs(S.astype(np.float64) - s[q, I]) <= w[q, I]).all(), "S is not the exact key"
    return len(S)


def _same(a, b):
    for u, v in zip(a, b):
        assert u.dtype == v.dtype
        np.testing.assert_array_equal(u, v)
    assert a[1].tobytes() == b[1].tobytes()


def _segments(result):
    lims, S, I = result
    li = lims.astype(np.int64)
    return [(S[a:b].tobytes(), I[a:b].tobytes()) for a, b in zip(li[:-1], li[1:])]


@pytest.fixture(scope="module")
def join_indexes(vf):
    out = {}
    for name in JOIN_DATA:
        x = _join_rows(name)
        index = vf.IndexFlatIP(x.shape[1])
        index.add(np.ascontiguousarray(x))
        out[name] = index
    return out


@pytest.mark.parametrize("name", list(JOIN_DATA))
def test_row_list_equals_the_window(join_indexes, name):
    index, t = join_indexes[name], JOIN_DATA[name][3]
    n = index.ntotal
    # windows that start inside a tile and span a tile edge (128) or several
    for q0, nq in ((100, 60), (250, 300), (n - 130, 130), (0, 128)):
        for excl in (True, False):
            win = index.range_selfjoin(t, q0=q0, nq=nq, exclude_self=excl)
            lst = index.range_selfjoin(t, rows=np.arange(q0, q0 + nq), exclude_self=excl)
            _same(win, lst)
    assert len(win[1]) > 0


@pytest.mark.parametrize("name", list(JOIN_DATA))
def test_row_list_segments_and_contract(join_indexes, name):
    index, t = join_indexes[name], JOIN_DATA[name][3]
    n = index.ntotal
    rng = np.random.default_rng(20)
    rows = rng.permutation(n)[:150]
    rows = np.concatenate([rows, rows[:7], [0, n - 1, 127, 128, 0]])  # duplicates too
    rows = rows[rng.permutation(rows.size)].astype(np.int64)
    res = index.range_selfjoin(t, rows=rows)
    s, w = _reference(name)
    assert _check_rows(res, s, w, t, rows) > 0
    _check_rows(index.range_selfjoin(t, rows=rows[:5], exclude_self=False), s, w, t, rows[:5],
                exclude_self=False)
    segs = _segments(res)
    single = {}
    for i in list(range(10)) + [int(j) for j in np.flatnonzero(np.isin(rows, [0, n - 1, 127]))]:
        r = int(rows[i])
        if r not in single:
            single[r] = _segments(index.range_selfjoin(t, q0=r, nq=1))[0]
        assert segs[i] == single[r], (i, r)
    # symmetry: r is in q's segment iff q is in r's, with the same bits
    lims, S, I = res
    li = lims.astype(np.int64)
    pos = {}
    for i, r in enumerate(rows):
        pos.setdefault(int(r), i)
    for i in range(rows.size):
        for sim, r in zip(S[li[i]:li[i + 1]], I[li[i]:li[i + 1]]):
            j = pos.get(int(r))
            if j is not None:
                hit = np.flatnonzero(I[li[j]:li[j + 1]] == rows[i])
                assert hit.size == 1 and S[li[j] + hit[0]].tobytes() == sim.tobytes()


def test_row_list_on_bf16_after_removals(vf):
    name, t = "seed0", 0.2
    x = _join_rows(name)
    index = vf.IndexFlatIP(x.shape[1], dtype="bf16")
    index.add(np.ascontiguousarray(x))
    s, w = _reference(name, bf16=True)
    rm = np.array([3, 130, 2999], dtype=np.int64)
    assert index.remove_ids(rm) == 3  # tombstones: the join packs them first
    keep = np.setdiff1d(np.arange(x.shape[0]), rm)
    s, w = s[np.ix_(keep, keep)], w[np.ix_(keep, keep)]
    n = keep.size
    rng = np.random.default_rng(21)
    rows = np.concatenate([rng.permutation(n)[:60], [2, 3, 129, 129, n - 1]]).astype(np.int64)
    res = index.range_selfjoin(t, rows=rows)
    assert _check_rows(res, s, w, t, rows) > 0
    segs = _segments(res)
    for i in (0, 1, 60, 61, 62, 63, 64):
        assert segs[i] == _segments(index.range_selfjoin(t, q0=int(rows[i]), nq=1))[0]
    _same(index.range_selfjoin(t, q0=100, nq=60), index.range_selfjoin(t, rows=np.arange(100, 160)))
    assert segs[62] == segs[63]


def test_row_list_refuses_bad_positions(join_indexes):
    from vsearch import _lib

    index = join_indexes["seed0"]
    n = index.ntotal
    for rows in ([1, n], [-1], [n + 5, 2]):
        with pytest.raises(RuntimeError, match="out of range") as e:
            index.range_selfjoin(0.2, rows=rows)
        assert e.value.code == _lib.E_INVALID
    lims, S, I = index.range_selfjoin(0.2, rows=[])
    assert lims.tolist() == [0] and S.size == 0


# ---- students -------------------------------------------------------------------------------------
def test_students_reembed_is_the_complete_diff():
    from vsearch import students as vstudents

    n, d, t = 1000, 96, 0.75
    rng = np.random.default_rng(30)
    centres = rng.standard_normal((25, d))
    cluster = rng.integers(0, 25, n)
    x = (centres[cluster] + 0.35 * rng.standard_normal((n, d))).astype(np.float32)
    keys = [f"student-{i:04d}" for i in range(n)]
    index = vstudents.StudentIndex(keys, x)
    before = index.edges(t)
    # 40 students: two adjacent rows, two of one cluster, the rest scattered
    mates = np.flatnonzero(cluster == cluster[500])
    mates = mates[~np.isin(mates, (500, 200, 201))]
    chosen = [200, 201, 500, int(mates[0])]
    rest = [int(r) for r in rng.permutation(n) if r not in chosen][:36]
    chosen = chosen + rest
    moved = rng.integers(0, 25, len(chosen))
    moved[2] = moved[3] = cluster[7]  # the pair lands in one cluster: an edge between two updated
    new = (centres[moved] + 0.35 * rng.standard_normal((len(chosen), d))).astype(np.float32)
    rows = index.reembed([(keys[r], new[i]) for i, r in enumerate(chosen)], threshold=t)
    final = x.copy()
    final[chosen] = new
    want = vstudents.StudentIndex(keys, final).edges(t)
    after = index.edges(t)
    assert after == want and after != before
    named = {keys[r] for r in chosen}
    diff = [e for e in want if e[0] in named or e[1] in named]
    assert rows == diff and len(diff) > 0
    assert (keys[chosen[2]], keys[chosen[3]]) in {(a, b) for a, b, _ in rows}
    assert (keys[chosen[3]], keys[chosen[2]]) in {(a, b) for a, b, _ in rows}
    # edges_of_many is edges_of per student; replace is a one-row reembed without the join
    some = [keys[r] for r in chosen[:5]]
    assert index.edges_of_many(some, t) == [e for s_ in some for e in index.edges_of(s_, t)]
    index.replace(keys[3], x[4])
    final[3] = x[4]
    assert index.edges(t) == vstudents.StudentIndex(keys, final).edges(t)
    assert index.keys == keys and len(index) == n


# ---- the store ------------------------------------------------------------------------------------
def test_store_upsert_in_place():
    from vsearch import langchain as vlc
    from vsearch.synth import SynthEmbeddings

    emb = SynthEmbeddings()
    n = 60
    texts = [f"book {i}: a story about topic {i % 7} and place {i % 11}" for i in range(n)]
    metas = [{"book_id": f"B{i:03d}", "author": f"A{i % 9}"} for i in range(n)]
    store = vlc.FAISS.from_texts(texts, emb, metadatas=metas)
    flt = {"author": "A3"}
    first = store.similarity_search(texts[12], k=3, filter=flt, exact_filter=True)
    assert [d.metadata["author"] for d in first] == ["A3"] * 3
    assert len(store._sel_cache) == 1
    sel = next(iter(store._sel_cache.values()))
    d0 = store.similarity_search(texts[12], k=5, distinct="author")
    assert len({d.metadata["author"] for d in d0}) == 5
    grp = store._grp_cache["author"]
    before = dict(store.index_to_docstore_id)

    new = texts[12] + " (revised and much extended edition)"
    ids = store.upsert_texts([new], metadatas=[metas[12]], in_place=True)
    assert store.index.ntotal == n and sorted(store.index_to_docstore_id) == list(range(n))
    assert store.index_to_docstore_id[12] == ids[0]
    assert {i for i in before if before[i] != store.index_to_docstore_id[i]} == {12}  # labels kept
    want = np.stack([emb.embed_query(t) for t in texts[:12] + [new] + texts[13:]])
    np.testing.assert_array_equal(store.index.reconstruct_n(0, n), want.astype(np.float32))
    # the cached handles are the ones still used, and they still run
    assert next(iter(store._sel_cache.values())) is sel and store._grp_cache["author"] is grp
    again = store.similarity_search(new, k=3, filter=flt, exact_filter=True)
    assert again[0].page_content == new and again[0].metadata == metas[12]
    assert [d.metadata["author"] for d in again] == ["A3"] * 3
    d1 = store.similarity_search(new, k=5, distinct="author")
    assert d1[0].page_content == new and len({d.metadata["author"] for d in d1}) == 5
    hit = store.similarity_search(new, k=1)[0]
    assert hit.page_content == new and hit.metadata["book_id"] == "B012"
    assert len(store.ids_for_key("B012")) == 1
    assert store.similarity_search(texts[12], k=1)[0].page_content != texts[12]
