"""GPU: the range self-join (vs_range_selfjoin; IndexFlat.range_selfjoin).

Oracle: the fp64 cosines s = x.x' / (|x||x'|) of the stored rows and the window
w = ``flat.key_window(..., cosine=True)`` an exactly computed, once-rounded key
can sit in.  The contract is test_gpu_range.py's: every pair with s >= t + w is
present, no pair with s < t - w is, |S - s| <= w, labels strictly ascending per
query, lims well formed, the pass is gemm_range.  The pairs inside the window
may go either way and are counted: at most 4 ordered pairs per case (a cap, so
that a case cannot pass because everything was "undecided").

Data and thresholds (ordered hits / undecided pairs of the fp64 reference):
  seed0      default_rng(0) standard normal, 3000 x 96: 0.0 / 0.2 / 0.45 ->
             4,497,788 / 223,274 / 10 hits, 0 / 0 / 0 undecided (0.3 would leave
             2, no headroom); as bf16 rows 4,497,756 / 223,290 / 10 and 0 / 2 / 0
  clustered  default_rng(1): 40 centres, a centre per row, + 0.35 * noise,
             3000 x 96: 0.75 -> 224,932 hits, 0 undecided (0.9 would leave 12)
  seed5      default_rng(5), 700 x 1536: 0.05 / 0.08 -> 12,344 / 426, 0 / 0
  seed6      default_rng(6), 1000 x 2080 (ld past the streaming kernels' limit):
             0.05 -> 10,948, 0
A subset of a set's rows has a subset of its pairs, so the tile-edge cases (the
first n rows of seed0) and the windows stay inside the cap as well.

The exact-property tests compare the engine with itself by design (symmetry,
upper = the r > q half, thresholds at a returned value): conditions of the
contract, not parity evidence."""

import ctypes
import functools

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

CAP = 4  # undecided ordered pairs per case


@pytest.fixture(scope="module")
def vf():
    from vsearch import _lib
    from vsearch import faiss as vfaiss

    assert _lib.device_count() >= 1
    return vfaiss


@functools.lru_cache(maxsize=None)
def _data(name):
    if name == "seed0":
        x = np.random.default_rng(0).standard_normal((3000, 96))
    elif name == "clustered":
        rng = np.random.default_rng(1)
        centres = rng.standard_normal((40, 96))
        x = centres[rng.integers(0, 40, 3000)] + 0.35 * rng.standard_normal((3000, 96))
    elif name == "seed5":
        x = np.random.default_rng(5).standard_normal((700, 1536))
    elif name == "seed6":
        x = np.random.default_rng(6).standard_normal((1000, 2080))
    else:
        raise KeyError(name)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _reference(x):
    """(fp64 cosines, windows) of every ordered pair of rows; NaN for zero rows."""
    x64 = np.asarray(x, dtype=np.float64)
    n2 = np.einsum("ij,ij->i", x64, x64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (x64 @ x64.T) / np.sqrt(np.outer(n2, n2))
    return s, flat.key_window(0, s, 0, 0, x.shape[1], cosine=True)


@functools.lru_cache(maxsize=None)
def _reference_of(name, bf16=False):
    x = _data(name)
    s, w = _reference(flat.round_bf16(x) if bf16 else x)
    s.setflags(write=False)
    w.setflags(write=False)
    return s, w


def _index(vf, x, dtype="f32"):
    index = vf.IndexFlatIP(x.shape[1], dtype=dtype)
    index.add(np.ascontiguousarray(x))
    return index


def _structure(lims, S, I, nq):
    assert lims.dtype == np.uint64 and S.dtype == np.float32 and I.dtype == np.int64
    assert lims.shape == (nq + 1,)
    assert lims[0] == 0 and lims[-1] == len(S) == len(I)
    li = lims.astype(np.int64)
    assert (np.diff(li) >= 0).all()
    if len(I) > 1:
        inner = np.ones(len(I) - 1, dtype=bool)  # neighbours inside one query's segment
        seams = li[1:-1]
        inner[seams[(seams > 0) & (seams < len(I))] - 1] = False
        assert (np.diff(I)[inner] > 0).all(), "labels not strictly ascending inside a query"
    return li


def _hit_matrix(li, I, nq, n, base=0):
    got = np.zeros((nq, n), dtype=bool)
    q = np.repeat(np.arange(nq), np.diff(li))
    r = I - base
    assert ((r >= 0) & (r < n)).all(), "a label outside the index"
    got[q, r] = True
    return got, q, r


def _check(result, s, w, t, *, q0=0, nq=None, exclude_self=True, upper=False, base=0,
           timer=True):
    """The contract over one result (s, w: the whole matrix's); returns (hits,
    undecided)."""
    from vsearch import _lib

    lims, S, I = result
    n = s.shape[0]
    nq = n - q0 if nq is None else nq
    s, w = s[q0:q0 + nq], w[q0:q0 + nq]
    if timer:
        assert _lib.timer_kernel() == "gemm_range"
    li = _structure(lims, S, I, nq)
    got, q, r = _hit_matrix(li, I, nq, n, base)
    rows = np.arange(n)[None, :]
    qrow = np.arange(q0, q0 + nq)[:, None]
    valid = np.ones((nq, n), dtype=bool)
    if exclude_self:
        valid &= rows != qrow
    if upper:
        valid &= rows > qrow
    t = float(t)
    inside = (s >= t + w) & valid
    outside = ~(s >= t - w) | ~valid  # a NaN cosine (a zero row) is outside
    undecided = int((~(inside | outside)).sum())
    print(f"hits {len(S)} undecided {undecided}")
    assert undecided <= CAP, undecided
    assert got[inside].all(), "a pair at or above the threshold is missing"
    assert not got[outside].any(), "a pair below the threshold (or excluded) was returned"
    err = np.abs(S.astype(np.float64) - s[q, r])
    assert (err <= w[q, r]).all(), "S is not the exact key"
    return len(S), undecided


def _subset(result, keep):
    """The entries of a result for which keep(q, I, S) holds, as a result."""
    lims, S, I = result
    nq = len(lims) - 1
    li = lims.astype(np.int64)
    q = np.repeat(np.arange(nq), np.diff(li))
    m = keep(q, I, S)
    out = np.zeros(nq + 1, dtype=np.uint64)
    out[1:] = np.cumsum(np.bincount(q[m], minlength=nq))
    return out, S[m], I[m]


def _same(a, b):
    for u, v in zip(a, b):
        assert u.dtype == v.dtype
        np.testing.assert_array_equal(u, v)
    assert a[1].tobytes() == b[1].tobytes()


# ---- the contract over the shapes ---------------------------------------------------------------
@pytest.mark.parametrize("name,t,hits", [
    ("seed0", 0.0, 4_497_788), ("seed0", 0.2, 223_274), ("seed0", 0.45, 10),
    ("clustered", 0.75, 224_932),
    ("seed5", 0.05, 12_344), ("seed5", 0.08, 426),
    ("seed6", 0.05, 10_948),
])
def test_full_join(vf, name, t, hits):
    x = _data(name)
    s, w = _reference_of(name)
    got, undecided = _check(_index(vf, x).range_selfjoin(t), s, w, t)
    assert undecided == 0 and got == hits


@pytest.mark.parametrize("ntotal", [1, 2, 127, 128, 129, 257])
@pytest.mark.parametrize("upper", [False, True])
def test_tile_edges(vf, ntotal, upper):
    x = _data("seed0")[:ntotal]
    s, w = _reference_of("seed0")
    s, w = s[:ntotal, :ntotal], w[:ntotal, :ntotal]
    index = _index(vf, x)
    pairs = np.triu(np.ones((ntotal, ntotal), dtype=bool), 1) if upper \
        else ~np.eye(ntotal, dtype=bool)
    for t in (0.0, 0.2):
        hits, _ = _check(index.range_selfjoin(t, upper=upper), s, w, t, upper=upper)
        assert hits == int(((s >= t) & pairs).sum())


@pytest.fixture(scope="module")
def seed0_index(vf):
    return _index(vf, _data("seed0"))


@pytest.mark.parametrize("q0,nq", [(5, 37), (127, 2), (2999, 1), (0, 1), (130, 300)])
@pytest.mark.parametrize("upper", [False, True])
def test_windows(seed0_index, q0, nq, upper):
    s, w = _reference_of("seed0")
    res = seed0_index.range_selfjoin(0.2, q0=q0, nq=nq, upper=upper)
    _check(res, s, w, 0.2, q0=q0, nq=nq, upper=upper)
    # a window is those rows of the full join
    full = seed0_index.range_selfjoin(0.2, upper=upper)
    li = full[0].astype(np.int64)
    a, b = li[q0], li[q0 + nq]
    np.testing.assert_array_equal(res[0].astype(np.int64), li[q0:q0 + nq + 1] - a)
    np.testing.assert_array_equal(res[1], full[1][a:b])
    np.testing.assert_array_equal(res[2], full[2][a:b])


@pytest.mark.parametrize("upper", [False, True])
def test_chunk_seams(seed0_index, upper):
    s, w = _reference_of("seed0")
    res = seed0_index.range_selfjoin(0.2, q0=100, nq=1000, upper=upper, chunk=256)
    _check(res, s, w, 0.2, q0=100, nq=1000, upper=upper)
    _same(res, seed0_index.range_selfjoin(0.2, q0=100, nq=1000, upper=upper))


@pytest.mark.parametrize("t", [0.0, 0.2, 0.45])
def test_bf16_index(vf, t):
    """The exact key is over the stored bf16 values, on both sides."""
    s, w = _reference_of("seed0", True)
    index = _index(vf, _data("seed0"), "bf16")
    _check(index.range_selfjoin(t), s, w, t)
    _check(index.range_selfjoin(t, upper=True), s, w, t, upper=True)


def test_bf16_after_remove_ids(vf):
    """A bf16 index keeps removed rows in place until a pack; the join packs
    them first, the remaining rows are renumbered, and the answer is that of a
    fresh index of the remaining rows bit for bit."""
    x = _data("seed0")
    ids = np.random.default_rng(5).choice(len(x), 50, replace=False)
    index = _index(vf, x, "bf16")
    assert index.remove_ids(ids) == 50
    live = np.delete(x, ids, axis=0)
    s, w = _reference(flat.round_bf16(live))
    res = index.range_selfjoin(0.2)
    _check(res, s, w, 0.2)
    assert index.ntotal == len(live)
    fresh = _index(vf, live, "bf16")
    _same(res, fresh.range_selfjoin(0.2))
    _same(index.range_selfjoin(0.2, upper=True), fresh.range_selfjoin(0.2, upper=True))


# ---- exact properties (the engine against itself) -----------------------------------------------
@pytest.mark.parametrize("name,t", [("seed0", 0.2), ("clustered", 0.75), ("seed6", 0.05)])
def test_deterministic_symmetric_and_upper_half(vf, name, t):
    x = _data(name)
    n = len(x)
    index = _index(vf, x)
    full = index.range_selfjoin(t)
    _same(full, index.range_selfjoin(t))
    li = _structure(*full, n)
    got, q, r = _hit_matrix(li, full[2], n, n)
    np.testing.assert_array_equal(got, got.T)
    bits = np.zeros((n, n), dtype=np.uint32)
    bits[q, r] = full[1].view(np.uint32)
    np.testing.assert_array_equal(bits, bits.T)
    up = index.range_selfjoin(t, upper=True)
    _same(up, _subset(full, lambda q, I, S: I > q))
    _same(up, index.range_selfjoin(t, upper=True, exclude_self=False))


@pytest.mark.parametrize("q0,nq", [(5, 300), (130, 129), (2900, 100)])
def test_upper_window_inside_a_tile(seed0_index, q0, nq):
    full = seed0_index.range_selfjoin(0.2, q0=q0, nq=nq)
    up = seed0_index.range_selfjoin(0.2, q0=q0, nq=nq, upper=True)
    _same(up, _subset(full, lambda q, I, S: I > q + q0))
    assert 0 < len(up[1]) < len(full[1])


def test_exclude_self_off_adds_the_self_pairs(vf):
    x = _data("seed0")[:300].copy()
    x[7] = 0.0  # a zero row neither matches nor is matched, itself included
    s, w = _reference(x)
    index = _index(vf, x)
    without = index.range_selfjoin(0.2)
    _check(without, s, w, 0.2)
    with_self = index.range_selfjoin(0.2, exclude_self=False)
    _check(with_self, s, w, 0.2, exclude_self=False)
    li = with_self[0].astype(np.int64)
    assert li[7] == li[8], "the zero row has hits"
    assert not (with_self[2] == 7).any(), "the zero row was matched"
    _same(without, _subset(with_self, lambda q, I, S: I != q))
    assert len(with_self[1]) - len(without[1]) == 299
    q = np.repeat(np.arange(300), np.diff(li))
    selfs = with_self[1][with_self[2] == q]
    assert (np.abs(selfs.astype(np.float64) - 1.0) <= 8 * flat.U32 + 1e-12).all()


def test_threshold_at_a_returned_value(seed0_index):
    """min_sim = a value v the join returned: the comparison is >=, so every
    pair with S == v stays; one ulp above v exactly those go."""
    base = seed0_index.range_selfjoin(0.2, q0=0, nq=500)
    v = np.sort(base[1])[len(base[1]) // 2]
    at = int((base[1] == v).sum())
    assert at >= 1
    _same(seed0_index.range_selfjoin(float(v), q0=0, nq=500),
          _subset(base, lambda q, I, S: S >= v))
    above = np.nextafter(v, np.float32(np.inf))
    res = seed0_index.range_selfjoin(float(above), q0=0, nq=500)
    _same(res, _subset(base, lambda q, I, S: S > v))
    assert len(res[1]) == int((base[1] >= v).sum()) - at


def test_extreme_thresholds(vf):
    x = _data("seed0")[:129]
    s, w = _reference_of("seed0")
    index = _index(vf, x)
    lims, S, I = index.range_selfjoin(-np.inf)
    _structure(lims, S, I, 129)
    np.testing.assert_array_equal(lims, (np.arange(130) * 128).astype(np.uint64))
    off = ~np.eye(129, dtype=bool)
    rows = np.tile(np.arange(129), (129, 1))
    np.testing.assert_array_equal(I, rows[off])
    assert (np.abs(S.astype(np.float64) - s[:129, :129][off]) <= w[:129, :129][off]).all()
    for t in (2.0, float("nan")):
        for upper in (False, True):
            lims, S, I = index.range_selfjoin(t, upper=upper, exclude_self=False)
            _structure(lims, S, I, 129)
            assert not lims.any() and len(S) == 0
    # no query rows, and no index rows
    lims, S, I = index.range_selfjoin(0.2, q0=129, nq=0)
    assert lims.tolist() == [0] and len(S) == 0
    lims, S, I = vf.IndexFlatIP(96).range_selfjoin(0.2)
    assert lims.tolist() == [0] and len(S) == 0
    with pytest.raises(RuntimeError, match="query rows out of range"):
        index.range_selfjoin(0.2, q0=100, nq=30)


def test_id_base_shifts_labels_only(vf):
    x = _data("seed0")[:700]
    index = _index(vf, x)
    plain = index.range_selfjoin(0.2, q0=100, nq=300, upper=True)
    index.set_id_base(1000)
    moved = index.range_selfjoin(0.2, q0=100, nq=300, upper=True)
    np.testing.assert_array_equal(moved[0], plain[0])
    np.testing.assert_array_equal(moved[1], plain[1])
    np.testing.assert_array_equal(moved[2], plain[2] + 1000)
    s, w = _reference_of("seed0")
    _check(moved, s[:700, :700], w[:700, :700], 0.2, q0=100, nq=300, upper=True, base=1000)


def test_device_outputs_match_host_copy(seed0_index):
    import torch

    from vsearch import _lib

    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.vs_range_selfjoin(seed0_index._h, 5, 37, ctypes.c_float(0.2), 1, 0, 0, None,
                                     ctypes.byref(h)), "vs_range_selfjoin")
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
    res = seed0_index.range_selfjoin(0.2, q0=5, nq=37)
    np.testing.assert_array_equal(res[0].astype(np.int64), lims)
    np.testing.assert_array_equal(res[1], D)
    np.testing.assert_array_equal(res[2], I)


# ---- against the top-k self-join ----------------------------------------------------------------
def test_agrees_with_selfjoin_where_k_suffices(vf):
    """selfjoin(k, min_sim) is the same graph cut at k: with k past every row's
    degree the label sets agree on every decided pair."""
    x = _data("clustered")
    s, w = _reference_of("clustered")
    index = _index(vf, x)
    nq, k, t = 64, 512, 0.75
    Sk, Ik = index.selfjoin(k, q0=0, nq=nq, min_sim=t)
    assert ((Ik >= 0).sum(axis=1) < k).all(), "a row reaches k"
    lims, S, I = index.range_selfjoin(t, q0=0, nq=nq)
    _check((lims, S, I), s, w, t, q0=0, nq=nq)
    got, _, _ = _hit_matrix(lims.astype(np.int64), I, nq, len(x))
    topk = np.zeros_like(got)
    qq, jj = np.nonzero(Ik >= 0)
    topk[qq, Ik[qq, jj]] = True
    decided = np.abs(s[:nq] - t) > w[:nq]
    np.testing.assert_array_equal(got[decided], topk[decided])
    assert got.sum() > 0


# ---- students -----------------------------------------------------------------------------------
def test_student_edges_on_golden_students(golden_vectors):
    from vsearch import students

    _, _, xs = golden_vectors
    keys = [f"s{i:02d}" for i in range(len(xs))]
    assert len(keys) == 25
    s, w = _reference(students.pgvector_quantize(xs))
    off = ~np.eye(25, dtype=bool)
    # a threshold in the widest gap of the middle half of the pair similarities
    vals = np.sort(s[off])
    lo, hi = len(vals) // 4, 3 * len(vals) // 4
    j = lo + int(np.argmax(np.diff(vals[lo:hi])))
    t = float(0.5 * (vals[j] + vals[j + 1]))
    assert (np.abs(s[off] - t) > w[off]).all(), "a pair inside the window"
    pos = {key: i for i, key in enumerate(keys)}
    topk = students.student_neighbours(keys, xs, k=24, threshold=t)
    edges = students.student_edges(keys, xs, threshold=t)
    want = {(pos[a], pos[b]) for a, b, _ in topk}
    got = [(pos[a], pos[b]) for a, b, _ in edges]
    assert got == sorted(got) and len(set(got)) == len(got)
    assert set(got) == want == {(a, b) for a in range(25) for b in range(25)
                                if a != b and s[a, b] >= t}
    assert 0 < len(got) < 600
    for a, b, v in edges:
        assert abs(v - s[pos[a], pos[b]]) <= w[pos[a], pos[b]]
    once = students.student_edges(keys, xs, threshold=t, directed=False)
    assert once == [e for e in edges if pos[e[0]] < pos[e[1]]]
    index = students.StudentIndex(keys, xs)
    assert index.edges(t) == edges
    assert index.edges(t, directed=False) == once
    for key in (keys[0], keys[13], keys[24]):
        assert index.edges_of(key, t) == [e for e in edges if e[0] == key]
