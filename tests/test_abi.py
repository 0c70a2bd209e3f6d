"""CPU: libvsearch.so loads and exports exactly the C-ABI that include/vsearch.h
declares; the ctypes signatures match the header.  No compute calls (no GPU here)."""

import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "vsearch.h")


def header_functions():
    text = open(HEADER, encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?(?:int|char\s*\*|const\s+char\s*\*)\s*\**\s*(vs_\w+)\s*\(",
                       text, flags=re.M)
    return sorted(set(names))


def test_header_parses():
    names = header_functions()
    assert "vs_search" in names and "vs_last_error" in names
    assert len(names) >= 20


def test_library_exports_every_declared_symbol():
    from vsearch import _lib

    lib = _lib.load()
    for name in header_functions():
        assert hasattr(lib, name), name


def test_ctypes_table_matches_header():
    from vsearch import _lib

    assert sorted(_lib.SIGNATURES) == header_functions()


def test_header_arg_counts_match_ctypes():
    from vsearch import _lib

    text = open(HEADER, encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, args) in _lib.SIGNATURES.items():
        m = re.search(name + r"\s*\(([^)]*)\)", text)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(args), (name, params, args)


def test_constants_match_header():
    from vsearch import _lib

    text = open(HEADER, encoding="utf-8").read()

    def const(name):
        return int(re.search(r"#define\s+" + name + r"\s+\(?(-?\d+)\)?", text).group(1))

    assert const("VS_METRIC_INNER_PRODUCT") == _lib.METRIC_INNER_PRODUCT == 0
    assert const("VS_METRIC_L2") == _lib.METRIC_L2 == 1
    assert const("VS_IN_DEVICE") == _lib.IN_DEVICE
    assert const("VS_OUT_DEVICE") == _lib.OUT_DEVICE
    assert const("VS_MAX_K") == _lib.MAX_K
    assert const("VS_E_INVALID") == _lib.E_INVALID


def test_error_path_without_device():
    """On a host with no GPU the library reports an error instead of falling back."""
    from vsearch import _lib

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.vs_create(8, 1, 0, 0, ctypes.byref(h))
    assert rc != 0
    assert "device" in _lib.last_error()
    from vsearch import faiss as vfaiss

    with pytest.raises(RuntimeError):
        vfaiss.IndexFlatL2(8)


def test_argument_validation_is_host_side():
    from vsearch import _lib

    lib = _lib.load()
    assert lib.vs_create(0, 1, 0, 0, ctypes.byref(ctypes.c_void_p())) == _lib.E_INVALID
    assert lib.vs_create(8, 7, 0, 0, ctypes.byref(ctypes.c_void_p())) == _lib.E_INVALID
    assert lib.vs_search(None, None, 1, 1, None, None, 0, None) == _lib.E_INVALID
    assert lib.vs_merge_topk(None, None, 0, 1, 1, 1, 1, None, None, None) == _lib.E_INVALID
    assert "bad sizes" in _lib.last_error()


INT_MAX = 2**31 - 1


def _search_calls():
    """(name, call(lib, idx, n, k)) of the five searches, with null buffers: the
    checks below return before anything is read through a pointer."""
    return [
        ("vs_search", lambda lib, idx, n, k: lib.vs_search(idx, None, n, k, None, None, 0, None)),
        ("vs_search_sel", lambda lib, idx, n, k: lib.vs_search_sel(
            idx, idx, None, n, k, None, None, 0, None)),
        ("vs_search_excl", lambda lib, idx, n, k: lib.vs_search_excl(
            idx, None, n, k, None, None, None, None, 0, None)),
        ("vs_search_profiles", lambda lib, idx, n, k: lib.vs_search_profiles(
            idx, None, None, None, n, k, None, None, 1, None, None, 0, None)),
        ("vs_selfjoin", lambda lib, idx, n, k: lib.vs_selfjoin(
            idx, 0, n, k, 1, 0.0, None, None, 0, None)),
    ]


@pytest.mark.parametrize("name,call", _search_calls(), ids=[c[0] for c in _search_calls()])
def test_search_argument_messages(name, call):
    """The code and the exact message of the bad-argument calls no device is
    needed for, for each search entry point (the checks they share live in one
    function, vs_api.hip check_search_args).  The strings were taken from a run
    of the library as it was before that function existed (every entry point
    with its checks written out), so they pin what it must not change:
    index, then n, then k, and for vs_search_profiles / vs_selfjoin k before the
    count.  The non-null "index" is a zeroed buffer: none of these checks
    reads it."""
    from vsearch import _lib

    lib = _lib.load()
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)

    def expect(idx, n, k, tail):
        assert call(lib, idx, n, k) == _lib.E_INVALID, (name, tail)
        assert _lib.last_error() == f"{name}: {tail}"

    expect(None, 1, 1, "null index")
    expect(None, -1, 0, "null index")  # the index is checked first
    expect(fake, 1, 0, "k must be > 0")
    expect(fake, 1, -3, "k must be > 0")
    expect(fake, 1, INT_MAX // 2 + 1, "k too large")
    if name == "vs_selfjoin":
        expect(fake, -1, 1, "query rows out of range")
        expect(fake, -1, 0, "k must be > 0")  # k before the rows
    elif name == "vs_search_profiles":
        expect(fake, -1, 1, "n < 0")
        expect(fake, -1, 0, "k must be > 0")  # k before n
    else:
        expect(fake, -1, 1, "n < 0")
        expect(fake, -1, 0, "n < 0")  # n before k
    # k = INT_MAX / 2 passes the bound: the next check answers
    assert call(lib, fake, 1, INT_MAX // 2) == _lib.E_INVALID
    # (vs_search_excl without lists is vs_search itself, message included)
    assert _lib.last_error() == {"vs_search_profiles": "vs_search_profiles: null offsets",
                                 "vs_search_excl": "vs_search: null buffer"}.get(
                                     name, name + ": null buffer")


def test_search_sel_null_selector_message():
    from vsearch import _lib

    lib = _lib.load()
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    # the selector is checked after the index and before n
    assert lib.vs_search_sel(fake, None, None, -1, 0, None, None, 0, None) == _lib.E_INVALID
    assert _lib.last_error() == "vs_search_sel: null selector"
    assert lib.vs_search_sel(None, None, None, 1, 1, None, None, 0, None) == _lib.E_INVALID
    assert _lib.last_error() == "vs_search_sel: null index"


def test_search_excl_checks_offsets_before_buffers():
    """vs_search_excl with lists: its offsets are checked before its buffers
    (strings from the same earlier run as above)."""
    import numpy as np

    from vsearch import _lib

    lib = _lib.load()
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    labels = np.zeros(1, dtype=np.int64)

    def call(offs, lab):
        offs = np.asarray(offs, dtype=np.int64)
        return lib.vs_search_excl(fake, None, 1, 1, offs.ctypes.data, lab, None, None, 0, None)

    assert call([1, 1], labels.ctypes.data) == _lib.E_INVALID
    assert _lib.last_error() == "vs_search_excl: offsets must start at 0 and not decrease"
    assert call([0, 1], None) == _lib.E_INVALID
    assert _lib.last_error() == "vs_search_excl: null exclusion labels"
    assert call([0, 1], labels.ctypes.data) == _lib.E_INVALID
    assert _lib.last_error() == "vs_search_excl: null buffer"
