"""GPU: the query cuts taken again after every replay (vs_x1_cuts.hip
x1_replay_cut_kernel, vs_gemm_x1.hip x1_plan; env VS_X1_RECUT).

The searches of test_gpu_dump.py: 4,096 queries (16 query tiles, 32 splits)
over 300,000 x 128 rows with launches of 8 tiles (VS_X1_CHUNK_TILES=8): a list
launch and four dump launches in three segments, so the cuts are taken again
twice (after launches 1 and 3) and the launches after them dump below lower
floors (the two cases whose passes take 64 splits of 19 tiles reach that
launch structure with 4-tile launches).  Every result is STRICT against the fp64 oracle on the 512-query
sample, no list runs out of slots on uniform rows, and the pass dumps strictly
fewer rows than with VS_X1_RECUT=0 on the same index (never more: every floor
is at most the old one; the counts depend on the data alone).  Lists out of
slots (the 150,000 scaled copies of test_gpu_dump.py) keep their queries
failed across a refresh; a search on a non-default stream and one with
VS_TAIL_WAIT=0 return the same lists."""

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

IP = flat.METRIC_INNER_PRODUCT
L2 = flat.METRIC_L2
N, D_, B = 300_000, 128, 4096
SAMPLE = np.array(sorted({q for t in range(16) for q in range(256 * t, 256 * t + 256, 8)}))


@pytest.fixture(scope="module")
def lib():
    """Launches of 8 tiles per workgroup (read at every search): 37-tile
    splits become a 5-launch pass."""
    import os

    from vsearch import _lib

    assert _lib.device_count() >= 1
    old = os.environ.get("VS_X1_CHUNK_TILES")
    os.environ["VS_X1_CHUNK_TILES"] = "8"
    yield _lib
    if old is None:
        del os.environ["VS_X1_CHUNK_TILES"]
    else:
        os.environ["VS_X1_CHUNK_TILES"] = old


@pytest.fixture(scope="module")
def uniform():
    """Rows, queries, and the oracle's lists of the sample per (metric, k):
    computed once, shared, never written."""
    rng = np.random.default_rng(131)
    xb = rng.uniform(-1, 1, (N, D_)).astype(np.float32)
    xq = rng.uniform(-1, 1, (B, D_)).astype(np.float32)
    xb.setflags(write=False)
    xq.setflags(write=False)
    refs = {}

    def ref(metric, k):
        if (metric, k) not in refs:
            refs[metric, k] = flat.knn_exact(xb, xq[SAMPLE], k, metric)
        return refs[metric, k]

    return xb, xq, ref


@pytest.fixture(scope="module")
def indexes(lib, uniform):
    """One index per (engine, metric) over the uniform rows."""
    from vsearch import faiss as vfaiss

    made = {}

    def get(engine, metric):
        if (engine, metric) not in made:
            index = vfaiss.IndexFlat(D_, metric)
            index.add(uniform[0])
            index.set_engine(engine)
            made[engine, metric] = index
        return made[engine, metric]

    return get


def _counted_search(lib, index, xq, k):
    lib.filter_stats(reset=True)
    D, I = index.search(xq, k)
    dumps, over = lib.filter_dump_stats()
    fq, ff = lib.filter_stats(reset=True)
    return D, I, dumps, over, fq, ff


def _strict(D, I, ref, metric, xb, xq):
    Dr, Ir = ref
    bad = flat.mismatches(D[SAMPLE], I[SAMPLE], Dr, Ir, metric, xb, xq[SAMPLE], strict=True)
    assert not bad, bad[:5]


@pytest.mark.parametrize("engine,metric,k,tiles", [("auto", IP, 1, 8), ("auto", IP, 10, 8),
                                                   ("auto", IP, 28, 4), ("bf16v", IP, 10, 4),
                                                   ("i8v", L2, 10, 8)])
def test_refreshed_cuts_are_exact_and_dump_fewer_rows(lib, uniform, indexes, monkeypatch, engine,
                                                      metric, k, tiles):
    """Inner product k = 28 (64 candidates) and the bf16 plane take 64 splits
    of 19 tiles instead of 32 of 37 (vs_engines.hip: twice the lists), which
    8-tile launches cut into 3: a split pass, one dump launch, no launch left
    for a refreshed cut to act on (measured: 3,788,717 rows dumped either way
    at k = 28).  Those two cases run 4-tile launches, which give them the
    five launches in three segments the other cases have at 8 (and 256 lists
    per query, the fused kernel's widest workgroup); at 8 tiles they are
    checked to stay exact and to dump no more rows."""
    xb, xq, ref = uniform
    index = indexes(engine, metric)
    monkeypatch.delenv("VS_X1_RECUT", raising=False)
    if tiles != 8:  # the split pass of 8-tile launches: exact, never more rows
        Ds, Is, dumps_s, over_s, _, _ = _counted_search(lib, index, xq, k)
        _strict(Ds, Is, ref(metric, k), metric, xb, xq)
        monkeypatch.setenv("VS_X1_RECUT", "0")
        _, _, dumps_s0, _, _, _ = _counted_search(lib, index, xq, k)
        monkeypatch.delenv("VS_X1_RECUT")
        print(f"{engine} k {k}, 8-tile launches: rows_dumped {dumps_s} / {dumps_s0} (cut set once)")
        assert 0 < dumps_s <= dumps_s0 and over_s == 0
    monkeypatch.setenv("VS_X1_CHUNK_TILES", str(tiles))
    D, I, dumps, over, fq, _ = _counted_search(lib, index, xq, k)
    print(f"{engine} metric {metric} k {k}: rows_dumped {dumps} (refreshed cuts), out of slots {over}")
    _strict(D, I, ref(metric, k), metric, xb, xq)
    assert fq == B and dumps > 0 and over == 0, (fq, dumps, over)
    monkeypatch.setenv("VS_X1_RECUT", "0")
    D0, I0, dumps0, over0, _, _ = _counted_search(lib, index, xq, k)
    print(f"{engine} metric {metric} k {k}: rows_dumped {dumps0} (cut set once)")
    _strict(D0, I0, ref(metric, k), metric, xb, xq)
    assert over0 == 0
    assert dumps < dumps0, (dumps, dumps0)
    # the replay and cut kernels back to back (the fused kernel's A/B) take
    # the same cuts: the same rows dumped, the same lists
    monkeypatch.setenv("VS_X1_RECUT", "2")
    D2, I2, dumps2, over2, _, _ = _counted_search(lib, index, xq, k)
    assert (dumps2, over2) == (dumps, 0)
    assert np.array_equal(I2, I) and np.array_equal(D2, D)


def test_lists_out_of_slots_stay_failed_across_a_refresh(lib, monkeypatch):
    """test_gpu_dump.py's test_dump_slot_overflow_hands_queries_on with the
    cuts refreshed: 150,000 scaled copies of one row beside every query, each
    better than every copy at a lower row, so lane lists meet more candidate
    rows per segment than their 128 slots.  Their queries' cuts become
    -FLT_MAX at the replay and no later refresh raises them: the queries go to
    the later stages and the answer is exact."""
    from vsearch import faiss as vfaiss

    monkeypatch.delenv("VS_X1_RECUT", raising=False)
    rng = np.random.default_rng(77)
    xb = rng.uniform(-1, 1, (N, D_)).astype(np.float32)
    dup = rng.uniform(-1, 1, D_).astype(np.float32)
    pos = np.sort(rng.choice(N, 150_000, replace=False))
    xb[pos] = dup[None, :] * (1.0 + 0.3 * pos[:, None] / N).astype(np.float32)
    xq = (dup[None, :] + 0.3 * rng.uniform(-1, 1, (B, D_))).astype(np.float32)
    index = vfaiss.IndexFlat(D_, IP)
    index.add(xb)
    D, I, dumps, over, _, _ = _counted_search(lib, index, xq, 10)
    print(f"scaled copies: rows_dumped {dumps}, lists out of slots {over}")
    assert over > 0, (dumps, over)
    _strict(D, I, flat.knn_exact(xb, xq[SAMPLE], 10, IP), IP, xb, xq)


def test_refresh_is_stream_ordered(lib, uniform, indexes, monkeypatch):
    """The refresh is a kernel on the search's stream between the replay's
    segment and the next launch: a device-output search on a non-default
    stream, and one with VS_TAIL_WAIT=0 (no host wait inside the search), give
    the lists of the host-output search."""
    import torch

    xb, xq, ref = uniform
    index = indexes("auto", IP)
    monkeypatch.delenv("VS_X1_RECUT", raising=False)
    Dh, Ih = index.search(xq, 10)
    _strict(Dh, Ih, ref(IP, 10), IP, xb, xq)
    q = torch.from_numpy(xq.copy()).cuda()
    st = torch.cuda.Stream()
    for tw in ("1", "0"):
        monkeypatch.setenv("VS_TAIL_WAIT", tw)
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
