"""GPU: the exact-key cuts of the int8 inner-product pass (vs_x1_cuts.hip
x1_ecut_kernel; env VS_X1_ECUT) and its quarter-length list
launch (env VS_X1_QUARTER).

The searches of test_gpu_cut_refresh.py: 4,096 queries (16 query tiles, 32
splits) over 300,000 x 128 uniform rows with launches of 8 tiles
(VS_X1_CHUNK_TILES=8): a list launch and four dump launches in three segments,
the smallest pass with two refreshed cuts.  Every cut is min(a_M + 2.000001 B,
e_M + 1.000001 B) with e_M the M-th smallest exact key over the query's M
best-approximate list entries; VS_X1_ECUT=0 keeps a_M + 2B alone.  Every result
is STRICT against the fp64 oracle on the 512-query sample; the exact cuts dump
no more rows (strictly fewer at k = 10), leave no list out of slots and hand no
more queries to the later stages.  Each setting searches a fresh index: the
automatic engine remembers how an index's earlier searches went
(test_gpu_dump_shape.py)."""

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

IP = flat.METRIC_INNER_PRODUCT
N, D_, B = 300_000, 128, 4096
SAMPLE = np.array(sorted({q for t in range(16) for q in range(256 * t, 256 * t + 256, 8)}))
KNOBS = ("VS_X1_ECUT", "VS_X1_RECUT", "VS_X1_QUARTER", "VS_X1_CHUNK_TILES", "VS_TAIL_WAIT")


@pytest.fixture(scope="module")
def lib():
    from vsearch import _lib

    assert _lib.device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def uniform():
    """Rows, queries, and the oracle's lists of the sample per k: computed
    once, shared, never written."""
    rng = np.random.default_rng(131)
    xb = rng.uniform(-1, 1, (N, D_)).astype(np.float32)
    xq = rng.uniform(-1, 1, (B, D_)).astype(np.float32)
    xb.setflags(write=False)
    xq.setflags(write=False)
    refs = {}

    def ref(k):
        if k not in refs:
            refs[k] = flat.knn_exact(xb, xq[SAMPLE], k, IP)
        return refs[k]

    return xb, xq, ref


@pytest.fixture(scope="module")
def runs(lib, uniform):
    """One search of the uniform rows per (k, settings) on a fresh index:
    (D, I, rows dumped, lists out of slots, queries filtered, queries the exact
    engine redid, queries handed to the bf16 stage).  Shared by the tests."""
    import os

    from vsearch import faiss as vfaiss

    xb, xq, _ = uniform
    made = {}

    def run(k, **env):
        key = (k, tuple(sorted(env.items())))
        if key not in made:
            env = {"VS_X1_CHUNK_TILES": "8", **env}
            old = {n: os.environ.get(n) for n in KNOBS}
            for n in KNOBS:
                os.environ.pop(n, None)
            os.environ.update(env)
            try:
                index = vfaiss.IndexFlat(D_, IP)
                index.add(xb)
                index.set_engine("auto")
                lib.filter_stats(reset=True)
                D, I = index.search(xq, k)
                dumps, over = lib.filter_dump_stats()
                second = lib.filter_second_stats()
                fq, ff = lib.filter_stats(reset=True)
            finally:
                for n in KNOBS:
                    os.environ.pop(n, None)
                    if old[n] is not None:
                        os.environ[n] = old[n]
            made[key] = (D, I, dumps, over, fq, ff, second)
        return made[key]

    return run


def _strict(D, I, ref, xb, xq):
    Dr, Ir = ref
    bad = flat.mismatches(D[SAMPLE], I[SAMPLE], Dr, Ir, IP, xb, xq[SAMPLE], strict=True)
    assert not bad, bad[:5]


@pytest.mark.parametrize("k", [1, 10])
def test_exact_cuts_are_exact_and_dump_fewer_rows(uniform, runs, k):
    xb, xq, ref = uniform
    D, I, dumps, over, fq, ff, second = runs(k)
    D0, I0, dumps0, over0, fq0, ff0, second0 = runs(k, VS_X1_ECUT="0")
    print(f"k {k}: rows_dumped {dumps} (exact cuts) / {dumps0} (VS_X1_ECUT=0); handed on "
          f"{second} + {ff} / {second0} + {ff0}")
    _strict(D, I, ref(k), xb, xq)
    _strict(D0, I0, ref(k), xb, xq)
    assert fq == B and fq0 == B
    assert over == 0 and over0 == 0
    assert 0 < dumps <= dumps0, (dumps, dumps0)
    if k == 10:
        assert dumps < dumps0, (dumps, dumps0)
    assert second <= second0 and ff <= ff0, (second, second0, ff, ff0)


@pytest.mark.parametrize("k", [1, 10])
def test_single_and_two_kernel_cuts(uniform, runs, k):
    """VS_X1_RECUT=0 (one cut, the exact one too) and =2 (x1_replay and x1_qcut
    back to back, then the same exact cut) are strict; =2 takes the fused
    form's cuts: the same rows dumped, bit-equal lists."""
    xb, xq, ref = uniform
    D, I, dumps, over, *_ = runs(k)
    D2, I2, dumps2, over2, *_ = runs(k, VS_X1_RECUT="2")
    Ds, Is, dumps_s, over_s, *_ = runs(k, VS_X1_RECUT="0")
    _, _, dumps_s0, _, *_ = runs(k, VS_X1_RECUT="0", VS_X1_ECUT="0")
    print(f"k {k}: rows_dumped {dumps} fused, {dumps2} two kernels, {dumps_s} single exact cut, "
          f"{dumps_s0} single a_M + 2B cut")
    _strict(D2, I2, ref(k), xb, xq)
    _strict(Ds, Is, ref(k), xb, xq)
    assert (dumps2, over2) == (dumps, 0)
    assert np.array_equal(I2, I) and np.array_equal(D2, D)
    assert over_s == 0 and dumps <= dumps_s <= dumps_s0


def test_shorter_list_launch(uniform, runs):
    """The list launch over 1/F of the first chunk (VS_X1_QUARTER=4, 8).  With
    37 tiles per workgroup the guard per_block / (F nchunk) >= 2 refuses it at
    8-tile launches (5 chunks) and at 4-tile launches (10 chunks): the results
    are those of the default.  10-tile launches (4 chunks, 37 / 16 = 2) pass it
    at F = 4, the default with exact cuts: a list launch of 2 tiles, then a
    dump launch over the other three quarters of the first chunk."""
    xb, xq, ref = uniform
    D, I, dumps, *_ = runs(10)
    for F in ("4", "8"):
        Df, If, dumps_f, over_f, *_ = runs(10, VS_X1_QUARTER=F)
        _strict(Df, If, ref(10), xb, xq)
        assert over_f == 0
        assert dumps_f == dumps and np.array_equal(If, I) and np.array_equal(Df, D)
    D4, I4, dumps4, over4, *_ = runs(10, VS_X1_CHUNK_TILES="4")
    _strict(D4, I4, ref(10), xb, xq)
    for F in ("4", "8"):
        Df, If, dumps_f, over_f, *_ = runs(10, VS_X1_CHUNK_TILES="4", VS_X1_QUARTER=F)
        assert (dumps_f, over_f) == (dumps4, over4) and over4 == 0
        assert np.array_equal(If, I4) and np.array_equal(Df, D4)
    # 10-tile launches: the quarter launch runs (the default with exact cuts)
    Dq, Iq, dumps_q, over_q, *_ = runs(10, VS_X1_CHUNK_TILES="10")
    Dn, In, dumps_n, over_n, *_ = runs(10, VS_X1_CHUNK_TILES="10", VS_X1_QUARTER="0")
    print(f"10-tile launches: rows_dumped {dumps_q} (list launch 1/4 chunk) / {dumps_n} (whole chunk)")
    _strict(Dq, Iq, ref(10), xb, xq)
    _strict(Dn, In, ref(10), xb, xq)
    assert over_q == 0 and over_n == 0
    assert dumps_q != dumps_n  # another launch structure: the quarter launch did run


def test_ties_at_the_cut(lib, uniform, runs):
    """One row duplicated 40 times next to a query: the query's M = 19 best
    approximate keys tie with 21 more rows, e_M ties with rows outside the top
    M, and no cut may drop any of them before the tie rule has ranked them."""
    import os

    from vsearch import faiss as vfaiss

    xb0, xq0, _ = uniform
    rng = np.random.default_rng(5)
    xb = xb0.copy()
    xq = xq0.copy()
    pos = np.sort(rng.choice(N, 40, replace=False))
    xq[77] = 4.0 * xb[pos[0]]  # far ahead of every other row for this query
    xb[pos] = xb[pos[0]]
    ref = flat.knn_exact(xb, xq[SAMPLE], 10, IP)
    one = flat.knn_exact(xb, xq[77:78], 10, IP)
    out = {}
    old = {n: os.environ.get(n) for n in KNOBS}
    try:
        for ecut in ("1", "0"):
            for n in KNOBS:
                os.environ.pop(n, None)
            os.environ["VS_X1_CHUNK_TILES"] = "8"
            os.environ["VS_X1_ECUT"] = ecut
            index = vfaiss.IndexFlat(D_, IP)
            index.add(xb)
            out[ecut] = index.search(xq, 10)
    finally:
        for n in KNOBS:
            os.environ.pop(n, None)
            if old[n] is not None:
                os.environ[n] = old[n]
    for D, I in out.values():
        _strict(D, I, ref, xb, xq)
        assert not flat.mismatches(D[77:78], I[77:78], one[0], one[1], IP, xb, xq[77:78],
                                   strict=True)
        assert set(I[77]) <= set(pos)
    assert np.array_equal(out["1"][1], out["0"][1]) and np.array_equal(out["1"][0], out["0"][0])


def test_lists_out_of_slots_stay_failed(lib, monkeypatch):
    """test_gpu_dump.py's 150,000 scaled copies of one row beside every query:
    lane lists meet more candidate rows per segment than their 128 slots, their
    queries' cuts become -FLT_MAX at the replay, and no exact cut revives one:
    the queries go to the later stages and the answer is exact."""
    from vsearch import faiss as vfaiss

    for n in KNOBS:
        monkeypatch.delenv(n, raising=False)
    monkeypatch.setenv("VS_X1_CHUNK_TILES", "8")
    rng = np.random.default_rng(77)
    xb = rng.uniform(-1, 1, (N, D_)).astype(np.float32)
    dup = rng.uniform(-1, 1, D_).astype(np.float32)
    pos = np.sort(rng.choice(N, 150_000, replace=False))
    xb[pos] = dup[None, :] * (1.0 + 0.3 * pos[:, None] / N).astype(np.float32)
    xq = (dup[None, :] + 0.3 * rng.uniform(-1, 1, (B, D_))).astype(np.float32)
    index = vfaiss.IndexFlat(D_, IP)
    index.add(xb)
    lib.filter_stats(reset=True)
    D, I = index.search(xq, 10)
    dumps, over = lib.filter_dump_stats()
    second = lib.filter_second_stats()
    lib.filter_stats(reset=True)
    print(f"scaled copies: rows_dumped {dumps}, lists out of slots {over}, handed on {second}")
    assert over > 0, (dumps, over)
    # a query with a list out of slots fails both checks: a revived cut would
    # let the int8 stage settle it
    assert second > 0
    _strict(D, I, flat.knn_exact(xb, xq[SAMPLE], 10, IP), xb, xq)


def test_exact_cut_is_stream_ordered(lib, uniform, runs, monkeypatch):
    """A device-output search on a non-default stream, with VS_TAIL_WAIT 1 and
    0 (no host wait inside the search), gives the host-output lists."""
    import torch

    from vsearch import faiss as vfaiss

    xb, xq, ref = uniform
    Dh, Ih, *_ = runs(10)
    for n in KNOBS:
        monkeypatch.delenv(n, raising=False)
    monkeypatch.setenv("VS_X1_CHUNK_TILES", "8")
    q = torch.from_numpy(xq.copy()).cuda()
    st = torch.cuda.Stream()
    for tw in ("1", "0"):
        monkeypatch.setenv("VS_TAIL_WAIT", tw)
        index = vfaiss.IndexFlat(D_, IP)
        index.add(xb)
        D = torch.empty(B, 10, device="cuda")
        I = torch.empty(B, 10, dtype=torch.int64, device="cuda")
        st.wait_stream(torch.cuda.current_stream())  # q's copy
        lib.filter_stats(reset=True)
        with torch.cuda.stream(st):
            index.search_device(q.data_ptr(), B, 10, D.data_ptr(), I.data_ptr(),
                                stream=st.cuda_stream)
        st.synchronize()
        dumps, over = lib.filter_dump_stats()
        lib.filter_stats(reset=True)
        assert dumps > 0 and over == 0
        assert np.array_equal(I.cpu().numpy(), Ih), tw
        assert np.array_equal(D.cpu().numpy(), Dh), tw
