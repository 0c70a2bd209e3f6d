"""CPU: boosted searches without a device — vs_boost_eval against the numpy
restatement of the definition bit for bit (bounds included), the bounds, the
spec arrays of ``boost_arrays``, the store's boost grammar, the argument checks
and the oracle on a hand-derived case."""

import ctypes

import numpy as np
import pytest

import boost_oracle as bo
from oracle import flat
from vsearch import _lib
from vsearch import faiss as vfaiss
from vsearch import langchain as vlc

L2, IP = flat.METRIC_L2, flat.METRIC_INNER_PRODUCT
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _random_case(seed, n=2000, ncol=4, nq=5):
    rng = np.random.default_rng(seed)
    cols = rng.uniform(-3.0, 12.0, size=(ncol, n)).astype(np.float32)
    cols[rng.random((ncol, n)) < 0.1] = np.nan
    cols[0, :7] = [0.0, -0.0, 4.2, 1e-40, -1e-40, 3.4e38, -3.4e38]  # edge values
    tags = rng.integers(0, 2**63, size=n, dtype=np.uint64) & np.uint64(0x3F)
    kinds = rng.integers(0, 3, size=(nq, ncol)).astype(np.int32)
    kinds[0] = [1, 2, 1, 2][:ncol]
    kinds[1] = [2, 1, 0, 1][:ncol]
    params = np.zeros((nq, ncol, 4), dtype=np.float32)
    params[:, :, 0] = rng.uniform(-1.0, 9.0, size=(nq, ncol)) + 0.1  # t: non-dyadic
    params[:, :, 1] = rng.uniform(0.3, 7.0, size=(nq, ncol))         # s
    params[:, :, 2] = rng.uniform(-0.7, 0.9, size=(nq, ncol))        # w: negative ones too
    params[:, :, 3] = rng.uniform(-1.5, 1.5, size=(nq, ncol))        # miss: outside [0, w] too
    params[0, 0] = [4.2, 5.0, 0.4, 0.2]  # the reference's reading-level term
    params[1, ncol - 1] = [4.2, 5.0, -0.3, 0.7]
    tag_masks = (rng.integers(0, 64, size=(nq, 4))).astype(np.uint64)
    tag_bonus = rng.uniform(-0.2, 0.3, size=(nq, 4)).astype(np.float32)
    tag_masks[0] = [1, 2, 0, 63]
    tag_bonus[0] = [0.05, -0.07, 0.9, 0.013]
    return cols, tags, kinds, params, tag_masks, tag_bonus


@pytest.mark.parametrize("seed,ncol", [(1, 4), (2, 3), (3, 1)])
def test_boost_eval_equals_the_numpy_definition_bit_for_bit(seed, ncol):
    cols, tags, kinds, params, tm, tb = _random_case(seed, ncol=ncol)
    b, bounds = vfaiss.boost_eval(cols, tags, (kinds, params, tm, tb))
    br, boundsr = bo.boost_values(cols, tags, kinds, params, tm, tb)
    assert b.shape == br.shape == (5, cols.shape[1])
    assert np.array_equal(_bits(b), _bits(br))
    assert np.array_equal(_bits(bounds), _bits(boundsr))
    # every evaluated b lies in [L, U]
    assert (b >= bounds[:, :1]).all() and (b <= bounds[:, 1:]).all()
    # the cases meant to be covered are: NaN values, every kind, negative weights,
    # miss above and below the term's range, tag terms that hit and miss
    assert np.isnan(cols).mean() > 0.05 and (params[:, :, 2] < 0).any()
    if ncol == 4:
        assert set(np.unique(kinds)) == {0, 1, 2}
        assert (params[:, :, 3] > 0.9).any() and (params[:, :, 3] < -0.7).any()


def test_boost_eval_tags_only_and_no_columns():
    tags = np.array([0, 1, 2, 3, 1 << 40], dtype=np.uint64)
    spec = {"tags": [(1, 0.125), (1 << 40, -2.0)]}
    b, bounds = vfaiss.boost_eval(None, tags, spec)
    assert b.tolist() == [[0.0, 0.125, 0.0, 0.125, -2.0]]
    assert bounds.tolist() == [[-2.0, 0.125]]
    br, boundsr = bo.boost_values(None, tags, None, None, *vfaiss.boost_arrays(spec, 0, 1)[2:])
    assert np.array_equal(_bits(b), _bits(br)) and np.array_equal(_bits(bounds), _bits(boundsr))


def test_hand_derived_values():
    # near: w max(0, 1 - |v - t| / s); ramp: w min(1, max(0, (v - t) / s))
    cols = np.array([[4.0, 6.5, 9.0, np.nan, 1.5]], dtype=np.float32)
    b, bounds = vfaiss.boost_eval(cols, None, {"columns": [("near", 4.0, 5.0, 0.5, 0.25)]})
    assert b[0].tolist() == [0.5, 0.25, 0.0, 0.25, 0.25]
    assert bounds.tolist() == [[0.0, 0.5]]
    b, bounds = vfaiss.boost_eval(cols, None, {"columns": [("ramp", 4.0, 5.0, -2.0)]})
    assert b[0].tolist() == [0.0, -1.0, -2.0, 0.0, 0.0]
    assert bounds.tolist() == [[-2.0, 0.0]]
    # a miss above the term's range raises U
    _, bounds = vfaiss.boost_eval(cols, None, {"columns": [("near", 4.0, 5.0, 0.5, 0.75)]})
    assert bounds.tolist() == [[0.0, 0.75]]


def test_boost_arrays_shapes_defaults_and_errors():
    kinds, params, tm, tb = vfaiss.boost_arrays(None, 3, 2)
    assert kinds.shape == (2, 3) and kinds.dtype == np.int32 and not kinds.any()
    assert params.shape == (2, 3, 4) and params.dtype == np.float32
    assert (params[:, :, 1] == 1).all() and not params[:, :, [0, 2, 3]].any()
    assert tm.shape == (2, 4) and tm.dtype == np.uint64 and tb.shape == (2, 4)
    spec = {"columns": [None, ("near", 4.2, 5, 0.4, 0.2), ("ramp", 1, 2, 0.5)],
            "tags": [(0b101, 0.05)]}
    kinds, params, tm, tb = vfaiss.boost_arrays([spec, None], 3, 2)
    assert kinds.tolist() == [[0, 1, 2], [0, 0, 0]]
    assert params[0, 1].tolist() == [f32(4.2), 5.0, f32(0.4), f32(0.2)]
    assert params[0, 2].tolist() == [1.0, 2.0, 0.5, 0.0]
    assert tm[0].tolist() == [5, 0, 0, 0] and tb[0, 0] == f32(0.05)
    # ready arrays pass through
    again = vfaiss.boost_arrays((kinds, params, tm, tb), 3, 2)
    assert all(np.array_equal(a, b) for a, b in zip(again, (kinds, params, tm, tb)))
    for bad, msg in [
        ([spec], "1 specs for 2 queries"),
        ({"column": []}, "unknown keys"),
        ({"columns": [None]}, "1 entries for 3 columns"),
        ({"columns": [None, ("exp", 1, 1, 1), None]}, "a column term is"),
        ({"columns": [None, ("near", 1, 1), None]}, "a column term is"),
        ({"tags": [(1, 0.1)] * 5}, "more than 4 tag terms"),
        ({"columns": [None, ("near", 1, 0, 1), None]}, "s must be > 0"),
        ({"columns": [None, ("near", 1, -2, 1), None]}, "s must be > 0"),
        ({"columns": [None, ("near", np.nan, 1, 1), None]}, "not finite"),
        ({"columns": [None, ("ramp", 1, 1, np.inf), None]}, "not finite"),
        ({"columns": [None, ("ramp", 1, 1, 1, -np.inf), None]}, "not finite"),
        ({"tags": [(1, np.nan)]}, "not finite"),
    ]:
        with pytest.raises(ValueError, match=msg):
            vfaiss.boost_arrays(bad, 3, 2)


def _eval_raw(kinds, params, tm=None, tb=None, ncol=1, nq=1):
    lib = _lib.load()
    cols = np.zeros((ncol, 3), dtype=np.float32)
    b = np.zeros((nq, 3), dtype=np.float32)
    bounds = np.zeros((nq, 2), dtype=np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return lib.vs_boost_eval(ncol, cols.ctypes.data, None, 3, ptr(kinds), ptr(params), ptr(tm),
                             ptr(tb), nq, b.ctypes.data, bounds.ctypes.data)


@pytest.mark.parametrize("pos,value", [(1, 0.0), (1, -1.0), (1, np.nan), (0, np.nan), (0, np.inf),
                                       (2, -np.inf), (3, np.nan), (1, np.inf)])
def test_bad_parameters_are_invalid_without_a_device(pos, value):
    kinds = np.array([[1]], dtype=np.int32)
    params = np.array([[[4.0, 5.0, 0.4, 0.2]]], dtype=np.float32)
    assert _eval_raw(kinds, params) == 0
    params[0, 0, pos] = value
    assert _eval_raw(kinds, params) == _lib.E_INVALID
    assert b"vs_boost_eval" in _lib.load().vs_last_error()
    kinds[0, 0] = 0  # a column of kind 0 is checked too
    assert _eval_raw(kinds, params) == _lib.E_INVALID


def test_other_argument_checks_without_a_device():
    kinds = np.array([[1]], dtype=np.int32)
    params = np.array([[[4.0, 5.0, 0.4, 0.2]]], dtype=np.float32)
    tm = np.ones((1, 4), dtype=np.uint64)
    tb = np.zeros((1, 4), dtype=np.float32)
    assert _eval_raw(kinds, params, tm, tb) == 0
    assert _eval_raw(np.array([[3]], dtype=np.int32), params) == _lib.E_INVALID
    assert _eval_raw(kinds, params, tm, None) == _lib.E_INVALID  # masks without bonuses
    tb[0, 2] = np.inf
    assert _eval_raw(kinds, params, tm, tb) == _lib.E_INVALID
    assert _eval_raw(None, params) == _lib.E_INVALID
    assert _eval_raw(kinds, params, ncol=5) == _lib.E_INVALID
    lib = _lib.load()
    # the search's checks come in vs_search_where's order: index, handle
    z = ctypes.c_void_p(None)
    assert lib.vs_search_boost(z, z, None, 1, 1, None, None, None, None, None, None, None, None,
                               None, None, None, 0, None) == _lib.E_INVALID
    assert b"vs_search_boost: null index" in lib.vs_last_error()
    assert lib.vs_boost_stats(None, None, None, None, 0) == _lib.E_INVALID
    assert _lib.BOOST_SCAN == 16
    s = vfaiss.boost_stats()
    assert len(s) == 4 and all(isinstance(v, int) for v in s)


# ---- the store grammar ----------------------------------------------------------------
NUMERIC = {"level", "pages", "year", "rating", "price"}


def _numeric(field):
    return field in NUMERIC


def test_grammar_maps_to_spec_arrays():
    spec = {"level": {"$near": 4.2, "scale": 5, "weight": 0.4, "missing": 0.2},
            "year": {"$ramp": [1990, 2020], "weight": 0.1},
            "genre": {"$in": ["fantasy", "adventure"], "weight": 0.05},
            "staff_pick": {"$eq": True, "weight": 0.05}}
    nums, pairs = vlc.boost_layout([spec, None], _numeric)
    assert nums == ("level", "year")
    assert set(pairs) == {("genre", "fantasy"), ("genre", "adventure"), ("staff_pick", True)}
    out = vlc.boost_spec(spec, nums, pairs, _numeric)
    assert out["columns"] == [("near", 4.2, 5.0, 0.4, 0.2), ("ramp", 1990.0, 30.0, 0.1, 0.0)]
    bit = {p: 1 << j for j, p in enumerate(pairs)}
    assert out["tags"] == [(bit[("genre", "fantasy")] | bit[("genre", "adventure")], 0.05),
                           (bit[("staff_pick", True)], 0.05)]
    assert vlc.boost_spec(None, nums, pairs, _numeric) is None
    kinds, params, tm, tb = vfaiss.boost_arrays(out, 2, 1)
    assert kinds.tolist() == [[1, 2]] and params[0, 1].tolist() == [1990.0, 30.0, f32(0.1), 0.0]
    # a wider handle (where= fields too): the columns land by name
    out = vlc.boost_spec(spec, ("level", "pages", "year"), pairs, _numeric)
    assert out["columns"][1] is None and out["columns"][2][0] == "ramp"


@pytest.mark.parametrize("spec,msg", [
    ({"level": {"$near": 1, "scale": 1, "weight": 1}, "pages": {"$near": 1, "scale": 1, "weight": 1},
      "year": {"$near": 1, "scale": 1, "weight": 1}, "rating": {"$near": 1, "scale": 1, "weight": 1},
      "price": {"$near": 1, "scale": 1, "weight": 1}}, "more than 4 numeric fields"),
    ({f"f{i}": {"$eq": 1, "weight": 0.1} for i in range(5)}, "more than 4 categorical terms"),
    ({"level": {"$exp": 1, "weight": 1}}, r"takes one of \['\$near', '\$ramp'\]"),
    ({"level": {"$in": [1, 2], "weight": 1}}, "takes one of"),
    ({"genre": {"$near": 1, "scale": 1, "weight": 1}}, r"takes one of \['\$eq', '\$in'\]"),
    ({"genre": {"$in": ["a"], "$eq": "b", "weight": 1}}, "takes one of"),
    ({"genre": {"$in": "a", "weight": 1}}, "takes a list"),
    ({"genre": {"$in": ["a"]}}, "numeric weight"),
    ({"level": {"$near": 1, "weight": 1}}, "numeric scale"),
    ({"level": {"$ramp": [1], "weight": 1}}, r"takes \[from, to\]"),
    ({"level": {"$near": 1, "scale": 1, "weight": 1, "decay": 2}}, "unknown keys"),
    ({"level": 4.2}, "takes a dict"),
    ({"$or": []}, "operator .or is not supported"),
    ("level", "a spec is a dict"),
])
def test_grammar_errors(spec, msg):
    with pytest.raises(ValueError, match=msg):
        vlc.boost_layout([spec], _numeric)


# ---- the oracle itself ------------------------------------------------------------------
def test_oracle_topk_on_a_hand_derived_case():
    # scores of 5 rows for one query; b lifts row 4 over row 0 and ties rows 1 and 2
    scores = np.array([[1.0, 0.75, 0.5, 0.25, 0.875]])
    b = np.array([[0.0, 0.0, 0.25, 0.0, 0.25]], dtype=np.float32)
    D, I = bo.boost_topk(scores, b, None, 3, IP)
    assert I.tolist() == [[4, 0, 1]] and D.tolist() == [[1.125, 1.0, 0.75]]
    D, I = bo.boost_topk(scores, b, None, 4, IP, exclude=[[4]])
    assert I.tolist() == [[0, 1, 2, 3]]  # the lower label wins the 0.75 tie
    D, I = bo.boost_topk(scores, b, np.array([[True, False, True, False, False]]), 3, IP)
    assert I.tolist() == [[0, 2, -1]] and D[0, 2] == flat.neutral(IP)
    # L2: the boost is subtracted and the result may be negative
    D, I = bo.boost_topk(scores, b, None, 2, L2)
    assert I.tolist() == [[2, 3]] and D.tolist() == [[0.25, 0.25]]
    D, I = bo.boost_topk(np.array([[0.125, 3.0]]), np.array([[0.5, 0.0]], dtype=np.float32), None,
                         1, L2)
    assert I.tolist() == [[0]] and D.tolist() == [[-0.375]]


def test_oracle_mismatches_tolerance():
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((50, 8)).astype(np.float32)
    xq = rng.standard_normal((2, 8)).astype(np.float32)
    b = rng.uniform(0, 0.5, size=(2, 50)).astype(np.float32)
    for metric in (IP, L2):
        s = flat.exact_scores(xb, xq, metric)
        Dr, Ir = bo.boost_topk(s, b, None, 5, metric)
        assert bo.mismatches(Dr, Ir, Dr, Ir, metric, xb, xq, b) == []
        D = Dr.copy()
        D[0, 0] += 1e-3
        assert [p[2] for p in bo.mismatches(D, Ir, Dr, Ir, metric, xb, xq, b)] == ["score"]
        I = Ir.copy()
        I[1, 0] = Ir[1, 4]
        I[1, 4] = Ir[1, 0]
        assert any(p[2] == "label" for p in bo.mismatches(Dr, I, Dr, Ir, metric, xb, xq, b))
