"""CPU: the launch plan of a filter pass (vs_gemm_x1.hip x1_plan, through the
diagnostic export vs_x1_plan): which launches a pass makes over which parts of
every workgroup's tiles, of which kind, and which replay and cut kernels run
between them.  x1_launch executes this plan and the search allocates its dump
buffers by it (x1_pass_dumps), so the invariants here are what keeps a pass
from dumping into memory it never got.  No device is touched."""

import ctypes
import itertools
import operator

import pytest

from vsearch import _lib

IP, I8, BF16 = 0, 1, 0
LIST, DUMP32, DUMP16 = 0, 2, 3  # kind 1 (the retired hybrid launch) is never produced
REPLAY, FIRST_CUT, REPLAY_CUT, EXACT_CUT = 1, 2, 4, 8
CAP = 704  # VS_X1_CHUNK_TILES >= 4 and 700 tiles: at most 176 launches
KNOBS = ("VS_X1_CHUNK_TILES", "VS_X1_SPLIT", "VS_X1_QUARTER", "VS_X1_DUMP_MFMA")

_out = (ctypes.c_int32 * (5 + 4 * CAP))()
_n = ctypes.c_int(0)


def plan(per_block, can_dump=1, plane=I8, ecut=0, gathered=0, recut=1, nsplit=1):
    """(nparts, cutting, 0, later_dump, pass_dumps, [(p0, p1, kind, after), ...]) of a
    pass of per_block tiles per workgroup."""
    ntotal = 256 * per_block * nsplit
    rc = _lib.load().vs_x1_plan(IP, plane, ntotal, nsplit, can_dump, ecut, gathered, recut, _out,
                                CAP, ctypes.byref(_n))
    assert rc == 0
    n = _n.value
    assert n <= CAP
    v = _out[:5 + 4 * n]
    return v[0], v[1], v[2], v[3], v[4], [tuple(v[5 + 4 * c:9 + 4 * c]) for c in range(n)]


def set_knobs(monkeypatch, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        if v is not None:
            monkeypatch.setenv("VS_X1_" + k, str(v))


# Every knob value against every (can_dump, ecut) the search can ask for; None
# is "not set" on a knob axis and "not asked for" on the other two.
SWEEP = list(itertools.product((None, 4, 8, 64), (None, 0, 4, 8), (None, 1), (None, 1),
                               (None, 0, 1, 8)))


def raw_plan(per_block, can_dump, plane, ecut, gathered=0):
    """The same as flat lists: head, p0s, p1s, kinds, afters (the sweep's fast path)."""
    rc = _lib.load().vs_x1_plan(IP, plane, 256 * per_block, 1, can_dump, ecut, gathered, 1, _out,
                                CAP, ctypes.byref(_n))
    assert rc == 0 and 0 < _n.value <= CAP
    v = _out[:5 + 4 * _n.value]
    return v[:5], v[5::4], v[6::4], v[7::4], v[8::4]


@pytest.mark.parametrize("chunk,split,can_dump,ecut,quarter", SWEEP)
def test_plan_invariants(monkeypatch, chunk, split, can_dump, ecut, quarter):
    set_knobs(monkeypatch, CHUNK_TILES=chunk, SPLIT=split, QUARTER=quarter)
    can_dump, ecut = can_dump or 0, ecut or 0
    for per_block in range(1, 701):
        # what the search asks before it allocates dump buffers (x1_pass_dumps)
        want_dumps = raw_plan(per_block, 1, I8, 0)[0][3]
        for plane in (I8, BF16):
            head, p0s, p1s, kinds, after = raw_plan(per_block, can_dump, plane, ecut)
            nparts, cutting, unused, later_dump, pass_dumps = head
            ctx = (per_block, can_dump, plane, ecut, head, p0s, p1s, kinds, after)
            assert unused == 0, ctx  # was "launch 0 is a hybrid launch"
            # contiguous, non-empty ranges covering [0, nparts) once
            assert p0s[0] == 0 and p1s[-1] == nparts and p0s[1:] == p1s[:-1], ctx
            assert all(map(operator.lt, p0s, p1s)), ctx
            # launch 0 lists; the later ones are all dump launches of one form, or
            # all list launches
            rest = set(kinds[1:])
            assert kinds[0] == LIST, ctx
            if later_dump:
                assert rest in (set(), {DUMP16}, {DUMP32}), ctx
            else:
                assert rest <= {LIST}, ctx
            # the dump buffers exist exactly when the plan needs them: the plane and
            # the exact-key cuts have no say in it
            assert pass_dumps == want_dumps, ctx
            if can_dump:
                assert later_dump == pass_dumps, ctx
            else:
                assert not later_dump and not cutting and not any(after), ctx
            assert not cutting or later_dump, ctx
            # after launch 0: the first cut of a cutting pass (no replay: launch 0
            # dumps nothing), an exact cut with it only when asked for
            ex = EXACT_CUT if ecut and plane == I8 else 0
            assert after[0] == (FIRST_CUT | ex if cutting else 0), ctx
            # after a dump launch: nothing, a replay, or (cutting passes) a replay and
            # a new cut, with its exact cut exactly when asked for
            allowed = {0} if not later_dump else {0, REPLAY, REPLAY_CUT | ex} if cutting \
                else {0, REPLAY}
            assert set(after[1:]) <= allowed, ctx
            # the last launch's dumps are replayed, and no cut follows that replay
            if rest and later_dump:
                assert after[-1] == REPLAY, ctx
        # a gathered batch: one list launch, whatever else is asked for
        for plane in (I8, BF16):
            g = raw_plan(per_block, 1, plane, 1, gathered=1)
            assert g[0][:4] == [1, 0, 0, 0] and [x[0] for x in g[1:]] == [0, 1, LIST, 0], g


def test_recut_off_sets_cuts_once(monkeypatch):
    set_knobs(monkeypatch)
    for per_block in (40, 150, 320, 700):
        for ecut in (0, 1):
            a = plan(per_block, ecut=ecut, recut=1)
            b = plan(per_block, ecut=ecut, recut=0)
            assert a[:5] == b[:5]
            assert [s[:3] for s in a[5]] == [s[:3] for s in b[5]]
            for (_, _, _, x), (_, _, _, y) in zip(a[5][1:], b[5][1:]):
                assert y == (REPLAY if x else 0)
            assert a[5][0] == b[5][0]
            assert plan(per_block, ecut=ecut, recut=2) == a  # the A/B of the fusion: same plan


def test_dump_form(monkeypatch):
    """The dump launches' MFMA form: 16x16x64 on the int8 plane unless
    VS_X1_DUMP_MFMA=32, 32x32 on bf16."""
    set_knobs(monkeypatch)
    assert {s[2] for s in plan(320)[5][1:]} == {DUMP16}
    assert {s[2] for s in plan(320, plane=BF16)[5][1:]} == {DUMP32}
    set_knobs(monkeypatch, DUMP_MFMA=32)
    assert {s[2] for s in plan(320)[5][1:]} == {DUMP32}


def test_split_count_keeps_per_block(monkeypatch):
    set_knobs(monkeypatch)
    assert plan(320, nsplit=8) == plan(320, nsplit=1)
    assert plan(40, nsplit=3) == plan(40, nsplit=1)


# The exact plans of the passes the GPU tests and the benchmarks run (int8
# plane, inner product, recut = 1, nsplit = 1), traced by hand.
D = DUMP16
RC = REPLAY_CUT
EXACT = [
    # one short launch
    (dict(), 15, 1, 0, (1, 0, 0, 0), [(0, 1, LIST, 0)]),
    # split pass
    (dict(), 40, 1, 0, (8, 1, 0, 1), [(0, 1, LIST, FIRST_CUT), (1, 8, D, REPLAY)]),
    # five launches in three segments
    (dict(), 320, 1, 0, (5, 1, 0, 1),
     [(0, 1, LIST, FIRST_CUT), (1, 2, D, RC), (2, 3, D, 0), (3, 4, D, RC), (4, 5, D, REPLAY)]),
    # exact-key cuts: the quarter list launch
    (dict(), 320, 1, 1, (20, 1, 0, 1),
     [(0, 1, LIST, FIRST_CUT | EXACT_CUT), (1, 4, D, RC | EXACT_CUT), (4, 8, D, 0),
      (8, 12, D, RC | EXACT_CUT), (12, 16, D, 0), (16, 20, D, REPLAY)]),
    # 40-tile launches
    (dict(), 150, 1, 0, (4, 1, 0, 1),
     [(0, 1, LIST, FIRST_CUT), (1, 2, D, RC), (2, 3, D, 0), (3, 4, D, REPLAY)]),
    (dict(), 150, 0, 0, (3, 0, 0, 0), [(0, 1, LIST, 0), (1, 2, LIST, 0), (2, 3, LIST, 0)]),
]


@pytest.mark.parametrize("knobs,per_block,can_dump,ecut,head,launches", EXACT)
def test_exact_plans(monkeypatch, knobs, per_block, can_dump, ecut, head, launches):
    set_knobs(monkeypatch, **knobs)
    got = plan(per_block, can_dump, I8, ecut)
    assert got[:4] == head
    assert got[5] == launches


def test_rejects_impossible_passes():
    lib = _lib.load()
    for args in ((IP, 2, 1000, 1), (7, I8, 1000, 1), (IP, I8, 0, 1), (IP, I8, 1000, 0),
                 (IP, I8, 1 << 31, 1)):
        assert lib.vs_x1_plan(*args, 1, 0, 0, 1, _out, CAP, ctypes.byref(_n)) != 0
    assert lib.vs_x1_plan(IP, I8, 1000, 1, 1, 0, 0, 1, None, 0, ctypes.byref(_n)) != 0
