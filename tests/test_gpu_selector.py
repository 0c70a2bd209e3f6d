"""GPU: selector searches (vs_search_sel; faiss SearchParameters(sel=...)).

Oracle: ``flat.select_topk`` over the fp64 scores with ``valid=`` the selection.
Every case plants copies of the queries in UNSELECTED rows (three per query
where the complement has room, else as many as fit), so the unfiltered nearest
rows lie outside the selection: a kernel that ignores or misindexes the row
list fails at once.  ``flat.mismatches`` does not check membership, so every
returned label is also checked against the mask.  The route is read from
``_lib.timer_kernel()``: "gemv_topk_rows" / "gemm_topk_rows" are the gathered
kernels; a selection that leaves at most 256 rows out runs the unselected
engine (any other name) and drops the excluded entries."""

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
N, DIM = 3000, 96
ROWS_KERNELS = ("gemv_topk_rows", "gemm_topk_rows")


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


def _mask(spec, n, seed=1):
    """Selection by name or size (random positions)."""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, dtype=bool)
    if spec == "first_half":
        m[: n // 2] = True
    elif spec == "last_row":
        m[n - 1] = True
    elif isinstance(spec, str) and spec.startswith("all_but_"):
        m[:] = True
        m[rng.choice(n, int(spec[8:]), replace=False)] = False
    elif isinstance(spec, float):
        m[:] = rng.random(n) < spec
    else:
        m[rng.choice(n, int(spec), replace=False)] = True
    return m


def _plant(xb, xq, mask):
    """Copies of the queries into unselected rows (3 per query where they fit)."""
    xb = xb.copy()
    out = np.nonzero(~mask)[0]
    for j, r in enumerate(out[: 3 * xq.shape[0]]):
        xb[r] = xq[j % xq.shape[0]]
    return xb


def _gathered_kernel(nq, d):
    ld = (d + 63) // 64 * 64
    fits = 8 * ld * 4 + 4 * 8 * 64 * 8 <= 64 * 1024
    return "gemv_topk_rows" if nq <= 32 and fits else "gemm_topk_rows"


def _check(vf, metric, xb, xq, mask, k, *, route, dtype="f32", raw=False, exact=False):
    """One index, one selector search, against the masked oracle.  route:
    "rows" (the gathered kernels), "drop" (route (b)) or None (nothing selected).
    Returns (D, I)."""
    from vsearch import _lib

    n, d = xb.shape
    nq = xq.shape[0]
    xb = _plant(xb, xq, mask)
    index = vf.IndexFlat(d, metric, dtype=dtype)
    index.add(xb)
    sel = index.selector(vf.IDSelectorBitmap(n, np.packbits(mask, bitorder="little")))
    assert sel.count == int(mask.sum())
    D, I = index.search(xq, k, params=vf.SearchParameters(sel=sel), raw=raw)
    name = _lib.timer_kernel()
    if route == "rows":
        assert name == _gathered_kernel(nq, d), name
    elif route == "drop":
        assert name not in ROWS_KERNELS, name
    ob, oq = (flat.round_bf16(xb), flat.round_bf16(xq)) if dtype == "bf16" else (xb, xq)
    Dr, Ir = flat.select_topk(flat.exact_scores(ob, oq, metric), k, metric,
                              valid=mask[None, :].repeat(nq, 0), rule="lex" if raw else "faiss")
    assert mask[I[I >= 0]].all(), "a label outside the selection"
    if exact:
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_array_equal(D, Dr)
        return D, I
    # route (b) through the staged engine returns exactly rescored keys
    strict = route == "drop" and name.startswith("gemm_topk_x1")
    bad = flat.mismatches(D, I, Dr, Ir, metric, ob, oq, strict=strict)
    assert not bad, (name, bad[:5])
    return D, I


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 40])
@pytest.mark.parametrize("spec", [0, 1, 9, 10, 127, 128, 129, 257, "first_half", "last_row",
                                  "all_but_257"])
def test_selection_sizes_at_tile_edges(vf, metric, nq, spec):
    xb, xq = _data(nq)
    mask = _mask(spec, N)
    D, I = _check(vf, metric, xb, xq, mask, 10, route="rows" if spec != 0 else None)
    if mask.sum() < 10:  # k > count: padded with (neutral, -1) past the count
        c = int(mask.sum())
        assert (I[:, c:] == -1).all() and (D[:, c:] == flat.neutral(metric)).all()
        assert (I[:, :c] >= 0).all()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("nq", [1, 40, 129])
@pytest.mark.parametrize("out", [1, 5, 256])
def test_route_b_small_complements(vf, metric, k, nq, out):
    """k = 40 with inner product is past one exact page: only this route serves it."""
    xb, xq = _data(nq, seed=3)
    _check(vf, metric, xb, xq, _mask(f"all_but_{out}", N, seed=out), k, route="drop")


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 3, 8, 9, 20, 33, 129])
def test_query_classes(vf, metric, nq):
    xb, xq = _data(nq, seed=4)
    _check(vf, metric, xb, xq, _mask(0.3, N), 10, route="rows")


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 25])
@pytest.mark.parametrize("d", [3, 40, 100, 1536, 2049])
def test_dimensions(vf, metric, nq, d):
    """d = 2049 does not fit the streaming kernel's LDS: the MFMA kernel at nq = 1."""
    xb, xq = _data(nq, n=700, d=d, seed=5)
    if d == 2049:
        assert _gathered_kernel(1, d) == "gemm_topk_rows"
    _check(vf, metric, xb, xq, _mask(0.4, 700), 10, route="rows")


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 40])
@pytest.mark.parametrize("k", [1, 16, 32, 33, 64])
def test_k_values_and_the_one_page_limit(vf, metric, nq, k):
    from vsearch import _lib

    xb, xq = _data(nq, seed=6)
    mask = _mask(0.3, N)
    if metric == IP and k > 32:
        index = vf.IndexFlat(DIM, metric)
        index.add(xb)
        with pytest.raises(_lib.VSearchError, match="k <= 32") as ei:
            index.search(xq, k, params=vf.SearchParameters(sel=vf.IDSelectorBitmap(
                N, np.packbits(mask, bitorder="little"))))
        assert ei.value.code == _lib.E_UNSUPPORTED
    else:
        _check(vf, metric, xb, xq, mask, k, route="rows")
    # the same k where at most 256 rows are left out: any k
    _check(vf, metric, xb, xq, _mask("all_but_5", N), k, route="drop")


@pytest.mark.parametrize("nq", [1, 40])
def test_l2_past_one_page(vf, nq):
    from vsearch import _lib

    xb, xq = _data(nq, seed=7)
    index = vf.IndexFlatL2(DIM)
    index.add(xb)
    sel = index.selector(vf.IDSelectorRange(0, N // 2))
    with pytest.raises(_lib.VSearchError, match="k <= 64") as ei:
        index.search(xq, 65, params=vf.SearchParameters(sel=sel))
    assert ei.value.code == _lib.E_UNSUPPORTED
    _check(vf, L2, xb, xq, _mask("all_but_5", N), 65, route="drop")


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("k", [1, 5, 16, 32])
@pytest.mark.parametrize("nq", [1, 7, 40])
@pytest.mark.parametrize("spec,route", [(0.5, "rows"), ("all_but_100", "drop")])
def test_ties_on_integer_data(vf, metric, k, nq, spec, route):
    """Small integers: every score is exact in fp32, so I and D must equal the
    masked oracle exactly — faiss's inner-product tie order over the selected
    rows only (test_selectors_host.py checks the oracle is deterministic)."""
    rng = np.random.default_rng(8)
    xb = rng.integers(-2, 3, size=(600, 3)).astype(np.float32)
    xq = rng.integers(-2, 3, size=(nq, 3)).astype(np.float32)
    _check(vf, metric, xb, xq, _mask(spec, 600), k, route=route, exact=True)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 40])
@pytest.mark.parametrize("spec,route", [(0.3, "rows"), ("all_but_5", "drop")])
def test_bf16_index_with_tombstones(vf, metric, nq, spec, route):
    """Removals below 1/16 of the rows stay in place as tombstones: the
    selector's label bits map to rows in place through the dead list."""
    from vsearch import _lib

    xb, xq = _data(nq, seed=9)
    rm = np.random.default_rng(10).choice(N, 100, replace=False).astype(np.int64)
    live = np.delete(np.arange(N), rm)
    mask = _mask(spec, live.size, seed=11)  # over the labels (the live positions)
    full = np.zeros(N, dtype=bool)
    full[live[mask]] = True
    xb = _plant(xb, xq, full | np.isin(np.arange(N), rm))  # plants in live unselected rows
    index = vf.IndexFlat(DIM, metric, dtype="bf16")
    index.add(xb)
    assert index.remove_ids(rm) == 100 and index.ntotal == live.size
    sel = index.selector(vf.IDSelectorBitmap(live.size, np.packbits(mask, bitorder="little")))
    assert sel.count == int(mask.sum())
    D, I = index.search(xq, 10, params=vf.SearchParameters(sel=sel))
    name = _lib.timer_kernel()
    assert (name in ROWS_KERNELS) == (route == "rows"), name
    rb, rq = flat.round_bf16(xb[live]), flat.round_bf16(xq)
    Dr, Ir = flat.select_topk(flat.exact_scores(rb, rq, metric), 10, metric,
                              valid=mask[None, :].repeat(nq, 0))
    assert mask[I[I >= 0]].all()
    bad = flat.mismatches(D, I, Dr, Ir, metric, rb, rq)
    assert not bad, (name, bad[:5])


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("spec", [0.3, "all_but_5"])
def test_id_base(vf, metric, spec):
    """Bit i of the bitmap selects label id_base + i."""
    xb, xq = _data(5, seed=12)
    mask = _mask(spec, N)
    xb = _plant(xb, xq, mask)
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    index.set_id_base(1000)
    Dr, Ir = flat.select_topk(flat.exact_scores(xb, xq, metric), 10, metric,
                              valid=mask[None, :].repeat(5, 0))
    handle = vf.Selector(index, np.packbits(mask, bitorder="little"), N)
    tree = vf.IDSelectorArray(1000 + np.nonzero(mask)[0])
    for sel in (handle, tree):
        D, I = index.search(xq, 10, params=vf.SearchParameters(sel=sel))
        assert (I >= 1000).all() and mask[I - 1000].all()
        assert not flat.mismatches(D, I - 1000, Dr, Ir, metric, xb, xq)
    # labels below the base select nothing
    D, I = index.search(xq, 3, params=vf.SearchParameters(sel=vf.IDSelectorRange(0, 1000)))
    assert (I == -1).all() and (D == flat.neutral(metric)).all()


def test_reuse_and_staleness(vf):
    xb, xq = _data(40, seed=13)
    mask = _mask(0.3, N)
    index = vf.IndexFlatL2(DIM)
    index.add(xb)
    sel = index.selector(vf.IDSelectorBitmap(N, np.packbits(mask, bitorder="little")))
    params = vf.SearchParameters(sel=sel)
    first = index.search(xq, 10, params=params)
    for _ in range(2):
        D, I = index.search(xq[:1], 10, params=params)
        np.testing.assert_array_equal(I, index.search(xq[:1], 10, params=params)[1])
        D, I = index.search(xq, 10, params=params)
        np.testing.assert_array_equal(I, first[1])
        np.testing.assert_array_equal(D, first[0])
    index.add(xb[:3])
    with pytest.raises(RuntimeError, match="stale selector"):
        index.search(xq, 10, params=params)
    sel = index.selector(vf.IDSelectorRange(0, 100))
    assert sel.count == 100
    assert index.remove_ids(np.array([N + 1], dtype=np.int64)) == 1
    with pytest.raises(RuntimeError, match="stale selector"):
        index.search(xq, 10, params=vf.SearchParameters(sel=sel))
    sel = index.selector(vf.IDSelectorRange(0, 100))
    index.reset()
    with pytest.raises(RuntimeError, match="stale selector"):
        index.search(xq, 10, params=vf.SearchParameters(sel=sel))
    other = vf.IndexFlatL2(DIM)
    other.add(xb)
    with pytest.raises(ValueError):
        other.search(xq, 10, params=vf.SearchParameters(sel=sel))


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("spec", [0.3, "all_but_5"])
def test_device_buffers_on_a_stream(vf, metric, spec):
    import torch

    xb, xq = _data(40, seed=14)
    index = vf.IndexFlat(DIM, metric)
    index.add(xb)
    sel = index.selector(vf.IDSelectorBitmap(N, np.packbits(_mask(spec, N), bitorder="little")))
    Dh, Ih = index.search(xq, 10, params=vf.SearchParameters(sel=sel))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        q = torch.from_numpy(xq).cuda()
        D = torch.empty((40, 10), dtype=torch.float32, device="cuda")
        I = torch.empty((40, 10), dtype=torch.int64, device="cuda")
        index.search_device(q.data_ptr(), 40, 10, D.data_ptr(), I.data_ptr(),
                            stream=st.cuda_stream, selector=sel)
        Dd, Id = D.cpu().numpy(), I.cpu().numpy()
    np.testing.assert_array_equal(Id, Ih)
    np.testing.assert_array_equal(Dd, Dh)


@pytest.mark.parametrize("nq", [1, 40])
@pytest.mark.parametrize("spec,route", [(0.3, "rows"), ("all_but_5", "drop")])
def test_raw_order(vf, nq, spec, route):
    xb, xq = _data(nq, seed=15)
    _check(vf, IP, xb, xq, _mask(spec, N), 10, route=route, raw=True)


def test_store_exact_filter(vf, golden):
    """A heavy reader: the nearest books are all read, so filtering the default
    fetch_k on the host returns fewer than k; the exact filter returns k."""
    from vsearch import langchain as vlc
    from vsearch.synth import SynthEmbeddings

    inputs, _ = golden
    store = vlc.FAISS.from_texts(inputs["book_texts"], SynthEmbeddings(),
                                 metadatas=inputs["book_metadata"])
    vec = store.embedding_function.embed_query(inputs["keywords"][0])
    read = [d.metadata["book_id"] for d in store.similarity_search_by_vector(vec, k=18)]
    flt = {"book_id": {"$nin": read}}
    loose = store.similarity_search_by_vector(vec, k=10, filter=flt)
    exact = store.similarity_search_by_vector(vec, k=10, filter=flt, exact_filter=True)
    assert len(loose) < 10 and len(exact) == 10
    assert not {d.metadata["book_id"] for d in exact} & set(read)
    assert isinstance(next(iter(store._sel_cache.values())), vf.Selector)
    want = [d.metadata["book_id"]
            for d in store.similarity_search_by_vector(vec, k=40)
            if d.metadata["book_id"] not in read][:10]
    assert [d.metadata["book_id"] for d in exact] == want
