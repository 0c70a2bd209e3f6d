"""GPU: the two MFMA shapes of the int8 inner-product dump launches
(vs_gemm_x1.hip, template flag S16).

The dump launches of an int8 inner-product pass run on v_mfma_i32_16x16x64_i8
by default and on v_mfma_i32_32x32x32_i8 with VS_X1_DUMP_MFMA=32 (read once per
search).  The accumulator layouts differ — in the 16x16 form lanes l and
l ^ 32 feed the same lane list and share its dump slots through a count
exchange — but both forms must leave the same lists: the same rows dumped, in
the same order, so every search below runs once per form on one index and
asserts the same dump counters and bit-identical (D, I), then strict agreement
with the fp64 oracle on the 512-query sample of tests/test_gpu_dump.py.

Sizing as in tests/test_gpu_dump.py: 300,000 rows, 4,096 queries,
VS_X1_CHUNK_TILES=8 — five launches in three segments (one list launch, four
dump launches), the last tile padded (300,000 = 1171 x 256 + 224)."""

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

IP = flat.METRIC_INNER_PRODUCT
N, B = 300_000, 4096
SAMPLE = np.array(sorted({q for t in range(16) for q in range(256 * t, 256 * t + 256, 8)}))


@pytest.fixture(scope="module")
def lib():
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


def _both_forms(lib, monkeypatch, xb, xq, k, engine="auto", metric=IP):
    """One search per form (32x32 first), each on a fresh index: the automatic
    engine adapts its stage order to how much the int8 stage settled in the
    index's earlier searches, so a second search on one index need not run the
    int8 pass at all.  Returns the two forms' (dumps, over, filtered, failed)
    — asserted equal — after checking that D and I are bit-identical between
    the forms and strict against the oracle."""
    from vsearch import faiss as vfaiss

    out = {}
    for form in ("32", "16"):
        index = vfaiss.IndexFlat(xb.shape[1], metric)
        index.add(xb)
        index.set_engine(engine)
        if form == "32":
            monkeypatch.setenv("VS_X1_DUMP_MFMA", "32")
        else:
            monkeypatch.delenv("VS_X1_DUMP_MFMA", raising=False)
        lib.filter_stats(reset=True)
        D, I = index.search(xq, k)
        dumps, over = lib.filter_dump_stats()
        fq, ff = lib.filter_stats(reset=True)
        out[form] = (D.copy(), I.copy(), (dumps, over, fq, ff))
        del index
    (D32, I32, s32), (D16, I16, s16) = out["32"], out["16"]
    print(f"32x32: dumps/over/filtered/failed = {s32}; 16x16: {s16}")
    assert s16 == s32, (s16, s32)
    assert np.array_equal(I16, I32)
    assert np.array_equal(D16.view(np.uint32), D32.view(np.uint32))
    Dr, Ir = flat.knn_exact(xb, xq[SAMPLE], k, metric)
    bad = flat.mismatches(D16[SAMPLE], I16[SAMPLE], Dr, Ir, metric, xb, xq[SAMPLE], strict=True)
    assert not bad, bad[:5]
    return s32


@pytest.mark.parametrize("d", [128, 192])
def test_uniform_rows_inner_product(lib, monkeypatch, d):
    """d = 192: three steps per tile, so tile starts land on every image of
    the ring of five."""
    rng = np.random.default_rng(131 + d)
    xb = rng.uniform(-1, 1, (N, d)).astype(np.float32)
    xq = rng.uniform(-1, 1, (B, d)).astype(np.float32)
    dumps, over, fq, _ = _both_forms(lib, monkeypatch, xb, xq, 10)
    assert fq == B and dumps > 0 and over == 0, (dumps, over)


def test_l2_augmented(lib, monkeypatch):
    """L2 through the int8 plane's augmented columns: an inner-product pass."""
    rng = np.random.default_rng(141)
    xb = rng.uniform(-1, 1, (N, 128)).astype(np.float32)
    xq = rng.uniform(-1, 1, (B, 128)).astype(np.float32)
    dumps, over, fq, ff = _both_forms(lib, monkeypatch, xb, xq, 10, engine="i8v",
                                      metric=flat.METRIC_L2)
    assert fq == B and dumps > 0 and over == 0 and ff == 0, (dumps, over, ff)


def test_queries_pointing_away(lib, monkeypatch):
    """Rows in [0, 1), queries in [-1, 0): every list's floor is above 0, and
    the padded rows of the last tile (zero sums) clear the threshold, so the
    rows-that-take-no-slot filter runs inside the count exchange."""
    rng = np.random.default_rng(123)
    xb = rng.uniform(0, 1, (N, 128)).astype(np.float32)
    xq = -rng.uniform(0, 1, (B, 128)).astype(np.float32)
    dumps, _, fq, _ = _both_forms(lib, monkeypatch, xb, xq, 10, engine="i8v")
    assert fq == B and dumps > 0


def _copies(n_copies, seed):
    """tests/test_gpu_dump.py's overflow data: scaled copies of one row, each
    better than every copy at a lower row, beside every query."""
    rng = np.random.default_rng(seed)
    xb = rng.uniform(-1, 1, (N, 128)).astype(np.float32)
    dup = rng.uniform(-1, 1, 128).astype(np.float32)
    pos = np.sort(rng.choice(N, n_copies, replace=False))
    xb[pos] = dup[None, :] * (1.0 + 0.3 * pos[:, None] / N).astype(np.float32)
    xq = (dup[None, :] + 0.3 * rng.uniform(-1, 1, (B, 128))).astype(np.float32)
    return xb, xq


def test_dense_candidates_within_slots(lib, monkeypatch):
    """15,000 copies (5 % of the rows; a tenth of the overflow case, whose
    lists meet ~230 candidate rows per segment: ~23 here, inside the 128
    slots): many 16-row blocks hold candidates in both partner lanes, so the
    slot exchange and the dump order decide the lists.  No list of the 32x32
    form runs out of slots, and the 16x16 form dumps exactly the same."""
    xb, xq = _copies(15_000, 177)
    dumps, over, _, _ = _both_forms(lib, monkeypatch, xb, xq, 10)
    assert dumps > 0 and over == 0, (dumps, over)


def test_slot_overflow_equal(lib, monkeypatch):
    """150,000 copies: lists run out of slots, and the count goes on past them
    equally in both forms (the same lists fail)."""
    xb, xq = _copies(150_000, 77)
    dumps, over, _, _ = _both_forms(lib, monkeypatch, xb, xq, 10)
    assert over > 0, (dumps, over)
